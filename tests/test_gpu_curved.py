"""clwh_render_curved and clwh_curve_profile on the GPU against the numpy restatement of their contract (tests/curved_ref.py), bit for
bit: the frame, the values and t_extreme on every pixel of the region in all three modes, skipping and dense; every record of every
station.  The cases are tests/curved_cases.py's, chosen with the reference on the CPU (tests/test_curved_cpu.py asserts what they
reach); the view's family counts what it exercised, as tests/test_gpu_slice.py does."""
import ctypes as C

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import costpath_ref as cp
from tests import curved_cases as cc
from tests import curved_ref as cr
from tests.test_gpu_slice import Tally
from tests.view_helpers import F, Outputs, Slice, host_lib, image_of

pytestmark = pytest.mark.gpu

INVALID_VALUE, BAD_NDRANGE, SIZE_MISMATCH = 1, 8, 9


class Curved(Outputs):
    NAMES, FLOATS = ("values", "t_extreme"), (1, 1)

    def run(self, volume, case, mode, flags=0):
        c = case
        return self.render(self.ctx.render_curved, (volume, c["rows"]), mode=mode, slab_samples=c["n"], step=c["step"], window=c["window"],
                           flags=flags)


def test_twisted_rows_through_the_phantoms(gpu_ctx):
    """reference == skipping walk == dense walk for every case and mode"""
    ctx = gpu_ctx
    tally = Tally()
    images = {}
    out = Curved(ctx, cc.FRAME, cc.REGION)
    for c in cc.twisted_cases():
        vol = c["vol"]
        if id(vol) not in images:
            images[id(vol)] = image_of(ctx, vol)
        volume = images[id(vol)][0]
        want, stats = cc.reference_of(c)
        what = "dims %s n %d step %r" % (vol.shape[::-1], c["n"], c["step"])
        for mode in cc.MODES:
            Curved.check(out.run(volume, c, mode), want[mode], "skipping, mode %d, %s" % (mode, what))
            Curved.check(out.run(volume, c, mode, flags=cr.DENSE), want[mode], "dense, mode %d, %s" % (mode, what))
        tally.add(stats)
    out.release()
    for volume, owner in images.values():
        volume.release()
        if owner is not None:
            owner.release()
    tally.assert_all()


def test_a_row_is_the_slice_with_its_frame(gpu_ctx):
    """device against device: row y of the curved view == region row 0 of clwh_render_slice with origin, du and normal of that row"""
    ctx = gpu_ctx
    w, h = cc.REGION
    curved, one = Curved(ctx, cc.FRAME, cc.REGION), Slice(ctx, cc.FRAME, (w, 8))
    compared = 0
    for c in cc.planar_cases() + cc.twisted_cases()[3:6]:
        volume, owner = image_of(ctx, c["vol"])
        for mode in cc.MODES:
            got = curved.run(volume, c, mode)
            for y in (0, 3, 5, 11, 12, 14, 17, 39):
                r = c["rows"][y]
                row = one.run(volume, dict(origin=r[0:3], du=r[3:6], dv=np.zeros(3, F), normal=r[6:9], n=c["n"], step=c["step"], window=c["window"]), mode)
                Curved.check([a[y:y + 1] for a in got], [a[0:1] for a in row], "row %d mode %d n %d" % (y, mode, c["n"]))
                compared += 1
        volume.release()
        if owner is not None:
            owner.release()
    curved.release()
    one.release()
    assert compared == 6 * 3 * 8


def _upload_mask(ctx, mask, garbage_seed=None):
    """the mask in grow's layout, the padding bits of every row filled with garbage"""
    Z, Y, X = mask.shape
    words = scene.mask_pack(mask).reshape(Z, Y, -1).copy()
    if garbage_seed is not None:
        rng = np.random.default_rng(garbage_seed)
        padded = np.unpackbits(words.view(np.uint8).reshape(Z, Y, -1), axis=2, bitorder="little")
        padded[:, :, X:] = rng.integers(0, 2, size=padded[:, :, X:].shape, dtype=np.uint8)
        assert padded[:, :, X:].any() and padded.shape[2] > X
        words = np.packbits(padded, axis=2, bitorder="little").view("<u4").astype(np.uint32).reshape(Z, Y, -1)
    return ctx.buffer_from(np.ascontiguousarray(words).reshape(-1))


def test_section_records_equal_the_search(gpu_ctx):
    ctx = gpu_ctx
    mask, rows = cc.painted_mask()
    dims = cc.SECTION_DIMS
    assert dims[0] % 32 != 0 and len(rows) % 8 != 0
    m = _upload_mask(ctx, mask, garbage_seed=4)
    for width, slab in cc.SECTION_SHAPES:
        for connected in (True, False):
            want, _ = cc.section_reference(width, slab, connected)
            got = ctx.curve_profile(m, dims, rows, width, slab, 1.0, connected=connected)
            assert got.dtype == cr.RECORD and np.array_equal(got, want), (width, slab, connected, got.tolist(), want.tolist())
    # the tube, its sections perpendicular to the traced centreline: rows of many directions, a quarter voxel apart
    tube = cp.tube()[0]
    t = _upload_mask(ctx, tube, garbage_seed=5)
    frames, _, n = scene.curve_frames(cp.tube_paths()[0], (1.0, 1.0, 1.0), 64, pixel_mm=0.25, station_mm=0.25, slab_samples=64)
    for connected in (True, False):
        want = cr.section_records(tube, frames[:n], 64, 64, 0.25, connected)
        got = ctx.curve_profile(t, (44, 44, 14), frames[:n], 64, 64, 0.25, connected=connected)
        assert np.array_equal(got, want) and want["count"].min() > 100, connected
    m.release()
    t.release()


def test_argument_errors_of_the_view(gpu_ctx):
    ctx = gpu_ctx
    vol = scene.phantom(16)
    volume = ctx.image_from(vol)
    frame = ctx.image([64, 32], 4, np.uint8, (32, 64, 4))
    plain = ctx.buffer(64 * 32 * 4, np.float32, (32, 64))
    small = ctx.buffer(64 * 32 * 4 - 4, np.float32)
    good = cc.twisted_rows((16, 16, 16), (64, 32), n=5)

    def status(**kw):
        args = dict(frame=frame, volume=volume, rows=good, width=64, height=32, mode=cr.MAX, slab_samples=5)
        args.update(kw)
        if args["rows"] is not None and len(args["rows"]) < args["height"]:  # (the library reads `height` rows before it checks the region)
            args["rows"] = np.concatenate([args["rows"], np.tile(cc.PADDING_ROW, (args["height"] - len(args["rows"]), 1))])
        return ctx.render_curved_raw(**args)

    assert status() == 0 and status(flags=cr.DENSE) == 0 and status(values=plain, t_extreme=plain) == 0
    assert all(status(mode=m) == 0 for m in cc.MODES) and status(mode=cr.MEAN, flags=cr.DENSE) == 0
    assert status(slab_samples=1) == 0 and status(slab_samples=8192, step=1e-3) == 0
    ctx.finish()
    frame.push(np.full((32, 64, 4), 9, np.uint8))
    plain.push(np.full((32, 64), 5.0, F))
    call = ffi.lib().clwh_render_curved
    zero = ffi.CurvedDesc()
    assert call(ctx.h, C.byref(zero)) == INVALID_VALUE and call(ctx.h, None) == INVALID_VALUE and call(None, C.byref(zero)) == INVALID_VALUE
    out = dict(values=plain, t_extreme=plain)
    assert status(rows=None, **out) == INVALID_VALUE
    assert status(frame=None, **out) == INVALID_VALUE and status(volume=None, **out) == INVALID_VALUE
    assert status(volume=frame, **out) == INVALID_VALUE and status(frame=volume, **out) == INVALID_VALUE
    assert status(frame=plain) == INVALID_VALUE and status(volume=plain, **out) == INVALID_VALUE
    assert status(mode=3, **out) == INVALID_VALUE and status(mode=-1, **out) == INVALID_VALUE
    assert status(flags=2, **out) == INVALID_VALUE and status(flags=-1, **out) == INVALID_VALUE
    assert status(slab_samples=0, **out) == INVALID_VALUE and status(slab_samples=8193, **out) == INVALID_VALUE
    for step in (0.0, -1.0, float("nan"), float("inf")):
        assert status(step=step, **out) == INVALID_VALUE
    for window in ((float("nan"), 1.0), (float("inf"), 1.0), (0.0, 0.0), (0.0, -1.0), (0.0, float("nan")), (0.0, float("inf"))):
        assert status(window=window, **out) == INVALID_VALUE
    for y in (0, 17, 31):  # any row
        for k in range(9):
            for bad in (float("nan"), float("inf"), float("-inf")):
                rows = good.copy()
                rows[y, k] = bad
                assert status(rows=rows, **out) == INVALID_VALUE, (y, k, bad)
    ctx.finish()
    assert np.all(frame.pull() == 9) and np.all(plain.pull() == F(5.0)), "nothing is written on an error"
    # the reach |origin| + (width - 1) |du| + (slab_samples - 1) step |normal| per axis and row: just below 2^30, and at it (the calls
    # that pass write the frame; those that fail are given the pre-filled outputs)
    below = float(2 ** 30 - 64)  # the largest float32 below 2^30

    def reach(y, origin, du, normal, **kw):
        rows = good.copy()
        rows[y] = np.concatenate([np.asarray(v, F) for v in (origin, du, normal)])
        return status(rows=rows, **kw)

    none = np.zeros(3, F)
    for k in range(3):
        e = np.zeros(3, F)
        e[k] = 1.0
        for y in (0, 31):
            assert reach(y, e * below, none, none) == 0 and reach(y, -e * below, none, none) == 0
            assert reach(y, e * 2.0 ** 30, none, none, **out) == INVALID_VALUE
            assert reach(y, e * 2.0 ** 24, e * 2.0 ** 24, none, **out) == INVALID_VALUE          # 2^24 + 63 * 2^24 = 2^30
            assert reach(y, e * (2.0 ** 24 - 1.0), -e * 2.0 ** 24, none) == 0                     # one below
            assert reach(y, none, none, e * 2.0 ** 28, step=1.0, **out) == INVALID_VALUE         # 4 * 1 * 2^28 = 2^30
            assert reach(y, e * below, none, e * 16.0, step=1.0, **out) == INVALID_VALUE         # 2^30 - 64 + 4 * 16
            assert reach(y, -e * (below - 64.0), none, e * 16.0, step=1.0) == 0                   # 2^30 - 128 + 64
    ctx.finish()
    assert np.all(plain.pull() == F(5.0))
    frame.push(np.full((32, 64, 4), 9, np.uint8))
    assert status(width=0, **out) == BAD_NDRANGE and status(height=0, **out) == BAD_NDRANGE
    assert status(width=12, **out) == BAD_NDRANGE and status(height=12, **out) == BAD_NDRANGE
    assert status(width=72, **out) == BAD_NDRANGE and status(height=40, **out) == BAD_NDRANGE
    assert status(width=65536, **out) == BAD_NDRANGE and status(height=65536, **out) == BAD_NDRANGE
    assert status(values=small, t_extreme=plain) == SIZE_MISMATCH and status(t_extreme=small, values=plain) == SIZE_MISMATCH
    # the order of the kinds: a value error wins over a region error, a region error over a size error
    assert status(step=0.0, width=12, values=small) == INVALID_VALUE and status(width=12, values=small) == BAD_NDRANGE
    ctx.finish()
    assert np.all(frame.pull() == 9) and np.all(plain.pull() == F(5.0)), "nothing is written on an error"
    assert status(values=small, t_extreme=small, width=56) == 0 and status(values=small, height=24) == 0
    ctx.finish()
    for m in (small, plain, frame, volume):
        m.release()


def test_argument_errors_of_the_profile(gpu_ctx):
    ctx = gpu_ctx
    mask, rows = cc.painted_mask()
    dims = cc.SECTION_DIMS
    n = len(rows)
    m = _upload_mask(ctx, mask)
    records = ctx.buffer(16 * n, cr.RECORD, (n,))
    fill = np.full(n, 0xABABABAB, np.uint32).repeat(4).view(cr.RECORD)
    vol_image = ctx.image_from(scene.phantom(16))

    def status(**kw):
        args = dict(mask=m, dims=dims, rows=rows, n_rows=n, width=64, slab_samples=64, step=1.0, flags=0, records=records)
        args.update(kw)
        return ctx.curve_profile_raw(**args)

    assert status() == 0 and status(flags=cr.CONNECTED) == 0 and status(n_rows=1) == 0 and status(width=1, slab_samples=1) == 0
    ctx.finish()
    records.push(fill)
    call = ffi.lib().clwh_curve_profile
    assert call(ctx.h, None) == INVALID_VALUE and call(None, C.byref(ffi.CurveProfileDesc())) == INVALID_VALUE
    assert call(ctx.h, C.byref(ffi.CurveProfileDesc())) == INVALID_VALUE
    assert status(mask=None) == INVALID_VALUE and status(records=None) == INVALID_VALUE and status(rows=None) == INVALID_VALUE
    assert status(mask=vol_image) == INVALID_VALUE and status(records=vol_image) == INVALID_VALUE
    off_mask = ctx.wrap(m.device_ptr + 4, m.nbytes - 4)
    off_records = ctx.wrap(records.device_ptr + 8, records.nbytes - 8)
    assert status(mask=off_mask) == INVALID_VALUE and status(records=off_records, n_rows=1) == INVALID_VALUE
    assert status(flags=2) == INVALID_VALUE and status(flags=-1) == INVALID_VALUE
    assert status(width=0) == INVALID_VALUE and status(width=65) == INVALID_VALUE
    assert status(slab_samples=0) == INVALID_VALUE and status(slab_samples=65) == INVALID_VALUE and status(slab_samples=-1) == INVALID_VALUE
    assert status(n_rows=0) == INVALID_VALUE and status(n_rows=65536, rows=np.tile(cc.PADDING_ROW, (65536, 1))) == INVALID_VALUE
    for step in (0.0, -1.0, float("nan"), float("inf")):
        assert status(step=step) == INVALID_VALUE
    assert status(dims=(0, 70, 13)) == INVALID_VALUE and status(dims=(2 ** 16, 2 ** 16, 2)) == INVALID_VALUE
    for k in range(9):
        for bad in (float("nan"), float("inf")):
            r = rows.copy()
            r[n - 1, k] = bad
            assert status(rows=r) == INVALID_VALUE, (k, bad)
    r = rows.copy()
    r[2, 0:3], r[2, 3:6] = (2.0 ** 24, 0, 0), (2.0 ** 24, 0, 0)  # 2^24 + 63 * 2^24 = 2^30
    assert status(rows=r) == INVALID_VALUE
    ctx.finish()
    assert np.array_equal(records.pull(), fill), "nothing is written on an error"
    assert status(rows=r, width=63) == 0  # one below
    ctx.finish()
    records.push(fill)
    assert status(dims=(75, 70, 14)) == SIZE_MISMATCH and status(dims=(129, 70, 13)) == SIZE_MISMATCH
    short = ctx.buffer(16 * n - 16, cr.RECORD, (n - 1,))
    assert status(records=short) == SIZE_MISMATCH and status(records=short, n_rows=n - 1) == 0
    assert status(width=0, records=short) == INVALID_VALUE, "a value error wins over a size error"
    ctx.finish()
    assert np.array_equal(records.pull(), fill), "nothing is written on an error"
    for b in (short, off_records, off_mask, vol_image, records, m):
        b.release()


def test_two_calls_back_to_back_keep_their_rows(gpu_ctx):
    """the staging discipline: the second call may not overwrite the page-locked rows before the first call's copy has left them,
    and the caller's array is free once a call has returned"""
    ctx = gpu_ctx
    a, b = cc.twisted_cases()[1], cc.planar_cases()[1]
    images = [image_of(ctx, c["vol"])[0] for c in (a, b)]
    w, h = cc.REGION
    frames = [ctx.image([w, h], 4, np.uint8, (h, w, 4)) for _ in range(4)]
    ctx.finish()
    for round_ in range(2):
        ra, rb = a["rows"].copy(), b["rows"].copy()
        ctx.render_curved(frames[2 * round_], images[0], ra, w, h, mode=cr.MAX, slab_samples=a["n"], step=a["step"], window=a["window"])
        ra[:] = 0
        ctx.render_curved(frames[2 * round_ + 1], images[1], rb, w, h, mode=cr.MIN, slab_samples=b["n"], step=b["step"], window=b["window"])
        rb[:] = 0
    ctx.finish()
    for round_ in range(2):
        assert np.array_equal(frames[2 * round_].pull(), cc.reference_of(a)[0][cr.MAX][0])
        assert np.array_equal(frames[2 * round_ + 1].pull(), cc.reference_of(b)[0][cr.MIN][0])
    for m in frames + images:
        m.release()


def test_host_mirror_reformat_and_profile_equal_the_binding(gpu_ctx):
    """renderer::render_curved and renderer::vessel_profile through the host library: the same bytes"""
    ctx = gpu_ctx
    mask, start, end = cp.tube()
    points = np.array(cp.tube_paths()[0], np.uint32)
    vol = np.where(mask, 100, 0).astype(np.int16)
    Z, Y, X = vol.shape
    env = scene.env_map(64, 32)
    L = host_lib(clvr_host_grow_region=(None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]),
                 clvr_host_render_curved=(C.c_void_p, [C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_int, C.c_double, C.c_int, C.c_int, C.c_float,
                                                       C.c_float, C.c_float, C.c_int]),
                 clvr_host_vessel_profile=(C.c_ulonglong, [C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.c_ulonglong]))
    volume, m = ctx.image_from(vol), _upload_mask(ctx, mask)
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, X, Y, Z, env.ctypes.data, 64, 32)
        grown = ffi.GrowResult()
        L.clvr_host_grow_region(h, np.array(start, np.uint32).ctypes.data, 1, 100, 100, 0, C.byref(grown))
        assert grown.count == int(mask.sum())
        for mode, n_slab, step in ((cr.MAX, 1, 0.25), (cr.MEAN, 9, 0.5)):
            rows, _, n = scene.curve_frames(points, (1.0, 1.0, 1.0), 64, pixel_mm=0.25, station_mm=0.25, slab_samples=n_slab, step_mm=step)
            H = len(rows)
            frame = ctx.image([64, H], 4, np.uint8, (H, 64, 4))
            ctx.render_curved(frame, volume, rows, 64, H, mode=mode, slab_samples=n_slab, step=step, window=(50.0, 100.0))
            mine = frame.pull()
            ptr = L.clvr_host_render_curved(h, points.ctypes.data, len(points), 64, 0.25, mode, n_slab, step, 50.0, 100.0, 0)
            host = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(1024, 2048, 4))[:H, :64].copy()
            assert np.array_equal(host, mine), (mode, n_slab)
            assert (mine[:n, :, 3] == 255).sum() > 1000 and (mine[n:] == 0).all() and len(np.unique(mine[..., 0])) > 3
            frame.release()
        want = ctx.vessel_profile(m, (X, Y, Z), points, (1.0, 1.0, 1.0), pixel_mm=0.25)
        n = len(want["records"])
        records, area, diameter = np.zeros(n + 2, cr.RECORD), np.zeros(n + 2), np.zeros(n + 2)
        got_n = L.clvr_host_vessel_profile(h, points.ctypes.data, len(points), 0.25, 64, 1, records.ctypes.data, area.ctypes.data,
                                           diameter.ctypes.data, n + 2)
        assert got_n == n and np.array_equal(records[:n], want["records"]) and want["records"]["count"].min() > 100
        assert np.array_equal(area[:n], want["area_mm2"]) and np.array_equal(diameter[:n], want["diameter_mm"])
    finally:
        L.clvr_host_destroy(h)
        volume.release()
        m.release()


def test_headless_curved_and_profile(tmp_path):
    import json
    import os
    import subprocess

    from tests.view_helpers import ROOT

    mask, start, end = cp.tube()
    W, H = 64, 328  # 318 stations: the last rows lie beyond the curve's end
    scene.write_nrrd(str(tmp_path / "v.nrrd"), np.where(mask, 100, 0).astype(np.int16))
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(np.random.default_rng(5).random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", str(W), str(H)]
    grow = "--grow=%d,%d,%d,100,100,centerline=%d,%d,%d" % (start + end)
    out = subprocess.run([exe, grow + ",profile", "--curved=16,slab=9,mean"] + files + [str(tmp_path / "p.ppm")], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")]
    points = np.array(cp.tube_paths()[0], np.uint32)[::-1]  # the seed first
    want = None
    for line in lines:
        want = line.get("profile", want)
    frames, s_mm, n = scene.curve_frames(points, (1.0, 1.0, 1.0), 64, pixel_mm=0.25, station_mm=0.25, slab_samples=64)
    records = cr.section_records(mask, frames[:n], 64, 64, 0.25, connected=True)
    measures = scene.profile_measures(records, 0.25, 0.25)
    assert want is not None and len(want["s_mm"]) == n and want["cut"] == [bool(c) for c in measures["cut"]]
    for key, ref in (("s_mm", s_mm), ("area_mm2", measures["area_mm2"]), ("diameter_mm", measures["diameter_mm"])):
        assert np.allclose(want[key], ref, rtol=0, atol=1e-6), key  # (printed with six decimals)
    last = lines[-1]
    assert last["curved"] == {"window_mm": 16.0, "angle": 0.0, "slab": 9, "mode": "mean", "stations": n} and last["frames"] == 1
    raw = open(tmp_path / "p.ppm", "rb").read()
    header = b"P6\n%d %d\n255\n" % (W, H)
    assert raw.startswith(header)
    ppm = np.frombuffer(raw[len(header):], np.uint8).reshape(H, W, 3)[::-1]  # the PPM's first row is the frame's last
    rows, _, n_rows = scene.curve_frames(points, (1.0, 1.0, 1.0), W, pixel_mm=0.25, station_mm=0.25, slab_samples=9, step_mm=0.125)
    rows = np.concatenate([rows, np.tile(cc.PADDING_ROW, (H - len(rows), 1))])
    kept = np.where(mask, 100, -32768).astype(np.int16)  # the view shows the masked volume
    ref, stats = cr.curved_view(kept, rows, (W, H), modes=(cr.MEAN,), slab_samples=9, step=0.125, window_cw=(0.0, 4000.0))
    assert n_rows == n and np.array_equal(ppm, ref[cr.MEAN][0][..., :3]) and stats["none"][n:].all() and len(np.unique(ppm)) > 5
    for bad in ("--curved=", "--curved=0", "--curved=16,slab=0", "--curved=16,median", "--curved=16,", "--curvedx", "--curved=slab=2,16"):
        assert subprocess.run([exe, grow, bad] + files, capture_output=True, text=True, timeout=120).returncode == 1, bad
    assert subprocess.run([exe, "--curved"] + files, capture_output=True, text=True, timeout=120).returncode == 1  # no centreline
    assert subprocess.run([exe, grow[:grow.index(",centerline")] + ",profile"] + files, capture_output=True, text=True, timeout=120).returncode == 1
    for other in ("--projection=max", "--composite", "--isosurface=300", "--slice=axial", "--mesh=50"):
        assert subprocess.run([exe, grow, "--curved", other] + files, capture_output=True, text=True, timeout=120).returncode == 1, other
    assert subprocess.run([exe, grow + ",show", "--curved"] + files, capture_output=True, text=True, timeout=120).returncode == 1


def test_from_the_clicks_to_the_reformat_and_the_stenosis_curve(gpu_ctx):
    """Context.centerline -> scene.curve_frames -> render_curved and vessel_profile on the tube at its native 44 x 44 x 14 equal the
    reference chain exactly"""
    ctx = gpu_ctx
    mask, start, end = cp.tube()
    rng = np.random.default_rng(8)
    vol = (np.where(mask, 300, -200) + rng.integers(-40, 41, size=mask.shape)).astype(np.int16)
    m, volume = _upload_mask(ctx, mask), ctx.image_from(vol)
    points, n_points = ctx.centerline(m, (44, 44, 14), start, end)
    want_points = cp.tube_paths()[0]
    assert n_points == len(want_points) and points.tolist() == [list(p) for p in want_points]
    rows, s_mm, n = scene.curve_frames(points, (1.0, 1.0, 1.0), 64, pixel_mm=0.25, station_mm=0.25, slab_samples=9, step_mm=0.5)
    H = len(rows)
    out = Curved(ctx, (64, H), (64, H))
    for mode, n_slab in ((cr.MAX, 1), (cr.MAX, 9), (cr.MEAN, 9)):
        case = dict(rows=rows, n=n_slab, step=0.5, window=(50.0, 600.0))
        want, stats = cr.curved_view(vol, rows, (64, H), modes=(mode,), slab_samples=n_slab, step=0.5, window_cw=case["window"])
        Curved.check(out.run(volume, case, mode), want[mode], "mode %d, %d samples" % (mode, n_slab))
        assert stats["none"][n:].all() and not stats["none"][:n, 24:40].any(), "the padding rows are transparent, the lumen is not"
    got = ctx.vessel_profile(m, (44, 44, 14), points, (1.0, 1.0, 1.0), pixel_mm=0.25)
    frames, want_s, want_n = scene.curve_frames(want_points, (1.0, 1.0, 1.0), 64, pixel_mm=0.25, station_mm=0.25, slab_samples=64)
    records = cr.section_records(mask, frames[:want_n], 64, 64, 0.25, connected=True)
    measures = scene.profile_measures(records, 0.25, 0.25)
    assert np.array_equal(got["records"], records) and np.array_equal(got["s_mm"], want_s) and len(records) == want_n > 200
    for key in ("area_mm2", "diameter_mm", "cut"):
        assert np.array_equal(got[key], measures[key]), key
    assert np.array_equal(got["offset_mm"], measures["offset_mm"], equal_nan=True)
    out.release()
    volume.release()
    m.release()
