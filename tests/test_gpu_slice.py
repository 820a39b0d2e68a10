"""clwh_render_slice on the GPU against the numpy restatement of its contract (tests/slice_ref.py), bit for bit: the frame, the values
and t_extreme on every pixel of the region, in all three modes.  The brick-skipping walk must equal the dense walk (CLWH_SLICE_DENSE)
and both the reference.  Every family counts what it exercised -- pixels without a kept sample, with a cut and with a full slab, ties
of the extreme, samples whose cell straddles a brick face or was clamped at a volume face, samples in bricks the skip rule steps over
-- so that no comparison is empty.  The inputs of a family are lists of cases (the *_cases functions), chosen with the reference on
the CPU; tests/test_slice_cpu.py asserts every family's tally with the reference alone."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import slice_ref as sr
from tests.view_helpers import ROOT, F, bits, image_of, pose as _pose, plant_blocks, quiet_phantom, host_lib, Slice, Iso, Proj

pytestmark = pytest.mark.gpu

INVALID_VALUE, BAD_NDRANGE, SIZE_MISMATCH = 1, 8, 9
FRAME, REGION = (64, 48), (56, 40)
MODES = (sr.MAX, sr.MIN, sr.MEAN)


class Tally:
    """what a family's comparisons exercised"""
    KINDS = ("none", "cut", "full", "tie", "straddle", "clamped", "skipped")

    def __init__(self):
        for k in self.KINDS:
            setattr(self, k, 0)
        self.comparisons = 0

    def add(self, stats):
        for k in ("none", "cut", "full"):
            setattr(self, k, getattr(self, k) + int(stats[k].sum()))
        self.tie += sum(int(m.sum()) for m in stats["tie"].values())
        self.straddle += stats["straddle"]
        self.clamped += stats["clamped"]
        self.skipped += sum(stats["skipped"].values())
        self.comparisons += 1

    def assert_all(self):
        assert all(getattr(self, k) > 0 for k in self.KINDS) and self.comparisons > 0, vars(self)


def _case(vol, origin, du, dv, normal, n=1, step=0.5, window=(0.0, 2000.0), frame_wh=FRAME, region_wh=REGION):
    origin, du, dv, normal = (np.asarray(v, F) for v in (origin, du, dv, normal))
    return dict(vol=vol, origin=origin, du=du, dv=dv, normal=normal, n=n, step=step, window=window, frame_wh=frame_wh, region_wh=region_wh)


def reference_of(case):
    """({mode: (frame, values, t_extreme)}, stats) of a case, computed once"""
    c = case
    if "_want" not in c:
        c["_want"] = sr.slice_view(c["vol"], c["origin"], c["du"], c["dv"], c["normal"], c["region_wh"], modes=MODES, slab_samples=c["n"],
                                   step=c["step"], window_cw=c["window"])
    return c["_want"]


def reference_tally(cases):
    tally = Tally()
    for c in cases:
        tally.add(reference_of(c)[1])
    return tally


def _run_family(ctx, cases):
    """reference == skipping walk == dense walk for every case and mode; returns the family's tally"""
    tally = Tally()
    images, outputs = {}, {}
    for c in cases:
        vol = c["vol"]
        if id(vol) not in images:
            images[id(vol)] = image_of(ctx, vol)
        key = (c["frame_wh"], c["region_wh"])
        if key not in outputs:
            outputs[key] = Slice(ctx, *key)
        volume, out = images[id(vol)][0], outputs[key]
        want, stats = reference_of(c)
        what = "dims %s n %d step %r origin %s normal %s" % (vol.shape[::-1], c["n"], c["step"], c["origin"], c["normal"])
        for mode in MODES:
            Slice.check(out.run(volume, c, mode), want[mode], "skipping, mode %d, %s" % (mode, what))
            Slice.check(out.run(volume, c, mode, flags=sr.DENSE), want[mode], "dense, mode %d, %s" % (mode, what))
        tally.add(stats)
    for out in outputs.values():
        out.release()
    for volume, owner in images.values():
        volume.release()
        if owner is not None:
            owner.release()
    return tally


def oblique(dims, region_wh=REGION, n=1, step=0.5, a=0.6, b=0.35, spacing=None):
    """(origin, du, dv, normal) of a plane about the volume's centre whose in-plane axes are rotated by a and b rad, the slab centred
    on it; the default pixel spacing of 1.3 * max(dims) / 56 leaves part of the plane outside the volume"""
    X, Y, Z = dims
    w, h = region_wh
    c = np.array([X / 2, Y / 2, Z / 2])
    u = np.array([np.cos(a), np.sin(a) * np.cos(b), np.sin(a) * np.sin(b)])
    v = np.array([-np.sin(a), np.cos(a) * np.cos(b), np.cos(a) * np.sin(b)])
    nn = np.cross(u, v)
    sp = 1.3 * max(dims) / 56 if spacing is None else spacing
    du, dv = u * sp, v * sp
    origin = c - du * w / 2 - dv * h / 2 - nn * (n - 1) * step / 2
    return origin.astype(F), du.astype(F), dv.astype(F), nn.astype(F)


PHANTOM_DIMS = [(64, 64, 64), (70, 33, 45), (130, 20, 9), (5, 4, 3), (1, 1, 1)]
SLABS = [(1, 0.5), (7, 0.37), (64, 0.5)]


@functools.lru_cache(maxsize=None)
def phantom_cases():
    cases = []
    for dims in PHANTOM_DIMS:
        vol = scene.phantom(max(dims), dims=dims)
        for n, step in SLABS:
            cases.append(_case(vol, *oblique(dims, n=n, step=step), n=n, step=step))
    quiet = quiet_phantom(48)  # constant regions: whole bricks are stepped over as soon as the slab has entered the air
    for n in (64, 200):
        cases.append(_case(quiet, *oblique((48, 48, 48), n=n, step=0.5), n=n, step=0.5))
    return cases


def test_phantoms_on_oblique_planes(gpu_ctx):
    _run_family(gpu_ctx, phantom_cases()).assert_all()


@functools.lru_cache(maxsize=None)
def random_cases():
    rng = np.random.default_rng(2025)
    cases = []
    for dims in [(24, 24, 24), (17, 9, 33)]:
        X, Y, Z = dims
        vol = plant_blocks(rng.integers(0, 1 << 16, size=(Z, Y, X), dtype=np.uint16).view(np.int16))
        diag = np.array([X, Y, Z], np.float64) / 56  # du along the volume's diagonal: pixel x runs from corner to corner
        side = np.cross(diag, [0.0, 0.0, 1.0])
        side *= 0.4 / np.linalg.norm(side)
        nn = np.cross(diag, side)
        nn /= np.linalg.norm(nn)
        for i, (n, step) in enumerate([(1, 0.37), (12, 0.5), (40, 1.3)]):
            cases.append(_case(vol, *oblique(dims, n=n, step=step, a=1.1, b=-0.4, spacing=max(dims) / 40), n=n, step=step, window=(0.0, 65536.0)))
            origin = -side * 20 - nn * (n - 1) * step / 2
            cases.append(_case(vol, origin, diag, side, nn, n=n, step=step, window=(0.0, 65536.0)))
            far = oblique(dims, n=n, step=step)
            cases.append(_case(vol, far[0] + F(1000.0), *far[1:], n=n, step=step))  # far outside: nothing is kept
    return cases


def test_random_bit_volumes(gpu_ctx):
    cases = random_cases()
    _run_family(gpu_ctx, cases).assert_all()
    assert all(reference_of(c)[1]["none"].all() for c in cases[2::3])  # the far planes keep nothing


def _axial_identity_cases(vol):
    """thin axial slices through the voxel centres: all weights are 0 and the value is the voxel"""
    Z, Y, X = vol.shape
    return [_case(vol, (0.5, 0.5, z + 0.5), (1, 0, 0), (0, 1, 0), (0, 0, 1), region_wh=(16, 16)) for z in range(Z)]


@functools.lru_cache(maxsize=None)
def axis_cases():
    X, Y, Z = 40, 24, 32
    vol = quiet_phantom(40)[:Z, :Y, :X].copy()
    cases = []
    for normal, n in (((0, 0, 1), 9), ((0, 0, -1), 9), ((0, 0, 1), 60)):  # the plane lies in the face z = 0; -z leaves at once
        cases.append(_case(vol, (0.25, 0.25, 0.0), (0.75, 0, 0), (0, 0.65, 0), normal, n=n))
    for normal, n in (((0, 1, 0), 5), ((0, -1, 0), 5), ((0, 1, 0), 40)):      # in the face y = 0
        cases.append(_case(vol, (0.5, 0.0, 0.5), (0.7, 0, 0), (0, 0, 0.8), normal, n=n))
    for normal, n in (((1, 0, 0), 7), ((-1, 0, 0), 7), ((-1, 0, 0), 1)):      # in the face x = X, which is outside; -x enters at sample 1
        cases.append(_case(vol, (40.0, 0.3, 0.2), (0, 0.5, 0), (0, 0, 0.7), normal, n=n))
    for v in (32767, -32768):  # a slab that never moves: 8192 samples of one position, the sum at the ends of int64's exact doubles
        extreme = np.full((8, 8, 8), v, np.int16)
        cases.append(_case(extreme, (0.3, 0.4, 3.7), (0.9, 0, 0), (0, 0.9, 0), (0, 0, 0), n=8192, window=(0.0, 65536.0), region_wh=(8, 8)))
    rng = np.random.default_rng(77)
    cases += _axial_identity_cases(rng.integers(-32768, 32768, size=(9, 10, 12)).astype(np.int16))
    return cases


def check_axis_expectations(cases):
    """what the axis family's reference must show, GPU or not"""
    want = [reference_of(c) for c in cases]
    assert want[1][1]["cut"].sum() > 0 and not want[1][1]["full"].any()          # normal -z from the face z = 0: sample 0 alone
    assert want[6][1]["none"].all() and want[8][1]["none"].all()                   # x = X is outside
    assert want[7][1]["cut"].sum() > 0                                            # ... and entered at sample 1
    assert np.all(bits(want[7][0][sr.MAX][2][want[7][1]["cut"]]) >= bits(F(0.5)))  # t_extreme counts from sample 0
    for c, w, v in ((cases[9], want[9], 32767), (cases[10], want[10], -32768)):
        for mode in MODES:
            assert np.all(w[0][mode][1] == F(v)) and w[1]["full"].all()
    ident = cases[11:]
    for z, c in enumerate(ident):
        vol = c["vol"]
        for mode in MODES:
            values = reference_of(c)[0][mode][1]
            assert np.array_equal(values[:10, :12], vol[z].astype(F)) and np.isnan(values[10:]).all() and np.isnan(values[:, 12:]).all()


def test_axis_aligned_and_grazing_planes(gpu_ctx):
    cases = axis_cases()
    check_axis_expectations(cases)
    _run_family(gpu_ctx, cases).assert_all()


@functools.lru_cache(maxsize=None)
def window_cases():
    vol = quiet_phantom(40)
    cases = []
    for window in ((1.0e6, 10.0), (-1.0e6, 10.0), (40.0, 0.001), (40.0, 1.0e-30), (0.0, 3.0e38)):
        for n, step in ((1, 0.5), (16, 0.5)):
            cases.append(_case(vol, *oblique((40, 40, 40), n=n, step=step), n=n, step=step, window=window))
    return cases


def check_window_expectations(cases):
    """far above: every kept pixel is black; far below: white; narrower than one grey level around the ball's value: 0, 128 and 255"""
    for c in cases:
        for mode in MODES:
            frame, values, _ = reference_of(c)[0][mode]
            kept = ~np.isnan(values)
            grey = frame[kept][:, 0]
            assert kept.sum() > 100 and np.all(frame[kept][:, 3] == 255) and np.all(frame[~kept] == 0)
            if c["window"][0] == 1.0e6:
                assert np.all(grey == 0)
            elif c["window"][0] == -1.0e6:
                assert np.all(grey == 255)
            elif c["window"][1] == 0.001 and mode != sr.MEAN:
                assert set(np.unique(grey)) >= {0, 128, 255} if mode == sr.MAX else {0, 128} <= set(np.unique(grey))
                assert np.all(grey[values[kept] == 40] == 128)


def test_windowing_at_its_ends(gpu_ctx):
    cases = window_cases()
    check_window_expectations(cases)
    assert _run_family(gpu_ctx, cases).comparisons == len(cases)


def derived_data_volumes():
    X, Y, Z = 24, 16, 40
    a = quiet_phantom(40)[:Z, :Y, :X].copy()
    b = np.where(a < -500, 900, -1000).astype(np.int16)  # air and ball swap: a stale dilated table skips the bricks that now hold the extreme
    return a, b


def derived_data_case(vol):
    """a slab that starts on the plane through the centre, inside the ball, and runs out through the air"""
    return _case(vol, *oblique(vol.shape[::-1], FRAME, n=1, spacing=0.6), n=80, step=0.5, region_wh=FRAME)


def test_derived_data_follows_the_volume_and_invalidation():
    from tests import isosurface_ref as ir
    from tests import projection_ref as pr

    a, b = derived_data_volumes()
    ctx = ffi.Context(0)  # a fresh context: nothing derived yet, no isosurface call before the first slice
    try:
        volume = ctx.image_from(a)
        out = Slice(ctx, FRAME, FRAME)
        tally = Tally()

        def slices(vol, what, modes=MODES):
            c = derived_data_case(vol)
            want, stats = reference_of(c)
            for mode in modes:
                Slice.check(out.run(volume, c, mode), want[mode], "%s, mode %d" % (what, mode))
            tally.add(stats)

        slices(a, "first call of the context", modes=(sr.MAX,))
        slices(a, "first volume")
        volume.push(b)
        slices(b, "after a push")
        ctx.invalidate_derived(scene=False, camera=False, projection=True)
        slices(b, "after invalidate")
        iso, proj = Iso(ctx, FRAME, FRAME), Proj(ctx, FRAME, FRAME)
        pos, d = _pose("default", b.shape[::-1])
        for flags in (0, ir.BELOW):
            Iso.check(iso.run(volume, pos, d, 300.0, flags=flags), ir.isosurface(b, pos, d, FRAME, FRAME, 300.0, flags=flags), "isosurface")
        want_p = pr.project(b, pos, d, FRAME, FRAME, modes=(pr.MAX,), window_cw=(0.0, 1000.0))
        Proj.check(proj.run(volume, pos, d, pr.MAX, window=(0.0, 1000.0)), want_p[pr.MAX], "projection")
        slices(b, "after an isosurface and a projection")
        ctx.finish()
        for o in (out, iso, proj):
            o.release()
        volume.release()
        assert tally.skipped > 0 and tally.cut > 0, vars(tally)
    finally:
        ctx.destroy()


def test_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    vol = scene.phantom(16)
    volume = ctx.image_from(vol)
    frame = ctx.image([64, 32], 4, np.uint8, (32, 64, 4))
    plain = ctx.buffer(64 * 32 * 4, np.float32)
    small = ctx.buffer(64 * 32 * 4 - 4, np.float32)
    origin, du, dv, normal = oblique((16, 16, 16), (64, 32), n=5)

    def status(**kw):
        args = dict(frame=frame, volume=volume, origin=origin, du=du, dv=dv, normal=normal, width=64, height=32, mode=sr.MAX, slab_samples=5)
        args.update(kw)
        try:
            ctx.render_slice(**args)
            return 0
        except ffi.ClwhError as e:
            return e.status

    call = ffi.lib().clwh_render_slice
    assert status() == 0 and status(flags=sr.DENSE) == 0 and status(values=plain, t_extreme=plain) == 0
    assert all(status(mode=m) == 0 for m in MODES) and status(mode=sr.MEAN, flags=sr.DENSE) == 0
    assert status(slab_samples=1) == 0 and status(slab_samples=8192, step=1e-3) == 0 and status(normal=(0, 0, 0)) == 0
    zero = ffi.SliceDesc()
    assert call(ctx.h, C.byref(zero)) == INVALID_VALUE
    zero.frame, zero.volume, zero.width, zero.height, zero.slab_samples, zero.window_width = frame.h, volume.h, 64, 32, 1, 1.0
    assert call(ctx.h, C.byref(zero)) == INVALID_VALUE  # everything but the step
    zero.step = 0.5
    assert call(ctx.h, C.byref(zero)) == 0  # (mode MAX, every vector 0: one position for all pixels)
    assert call(ctx.h, None) == INVALID_VALUE and call(None, C.byref(zero)) == INVALID_VALUE
    zero.frame = None
    assert call(ctx.h, C.byref(zero)) == INVALID_VALUE
    zero.frame, zero.volume = frame.h, None
    assert call(ctx.h, C.byref(zero)) == INVALID_VALUE
    assert status(volume=frame) == INVALID_VALUE and status(frame=volume) == INVALID_VALUE
    assert status(frame=plain) == INVALID_VALUE and status(volume=plain) == INVALID_VALUE
    assert status(mode=3) == INVALID_VALUE and status(mode=-1) == INVALID_VALUE
    assert status(flags=2) == INVALID_VALUE and status(flags=-1) == INVALID_VALUE and status(flags=1 << 16) == INVALID_VALUE
    assert status(slab_samples=0) == INVALID_VALUE and status(slab_samples=8193) == INVALID_VALUE and status(slab_samples=-5) == INVALID_VALUE
    for step in (0.0, -1.0, float("nan"), float("inf")):
        assert status(step=step) == INVALID_VALUE
    for window in ((float("nan"), 1.0), (float("inf"), 1.0), (0.0, 0.0), (0.0, -1.0), (0.0, float("nan")), (0.0, float("inf"))):
        assert status(window=window) == INVALID_VALUE
    for name in ("origin", "du", "dv", "normal"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            for k in range(3):
                v = [0.25, 0.25, 0.25]
                v[k] = bad
                assert status(**{name: v}) == INVALID_VALUE, (name, bad, k)
    # the reach |origin| + (width - 1) |du| + (height - 1) |dv| + (slab_samples - 1) step |normal| per axis: just below 2^30, and at it
    below = float(2 ** 30 - 64)  # the largest float32 below 2^30
    for k in range(3):
        e = np.zeros(3, F)
        e[k] = 1.0
        none = np.zeros(3, F)
        assert status(origin=e * below, du=none, dv=none, normal=none) == 0 and status(origin=-e * below, du=none, dv=none, normal=none) == 0
        assert status(origin=e * 2.0 ** 30, du=none, dv=none, normal=none) == INVALID_VALUE
        assert status(origin=e * 2.0 ** 24, du=e * 2.0 ** 24, dv=none, normal=none) == INVALID_VALUE               # 2^24 + 63 * 2^24 = 2^30
        assert status(origin=e * (2.0 ** 24 - 1.0), du=-e * 2.0 ** 24, dv=none, normal=none) == 0                  # one below
        assert status(origin=-e * (33.0 * 2.0 ** 24), du=none, dv=e * 2.0 ** 24, normal=none) == INVALID_VALUE     # 33 * 2^24 + 31 * 2^24
        assert status(origin=e * (33.0 * 2.0 ** 24 - 64.0), du=none, dv=e * 2.0 ** 24, normal=none) == 0
        assert status(origin=none, du=none, dv=none, normal=e * 2.0 ** 28, step=1.0) == INVALID_VALUE      # 4 * 1 * 2^28 = 2^30
        assert status(origin=e * below, du=none, dv=none, normal=e * 16.0, step=1.0) == INVALID_VALUE      # 2^30 - 64 + 4 * 16
        assert status(origin=-e * (below - 64.0), du=none, dv=none, normal=e * 16.0, step=1.0) == 0        # 2^30 - 128 + 64
    assert status(width=0) == BAD_NDRANGE and status(height=0) == BAD_NDRANGE and status(width=12) == BAD_NDRANGE and status(height=12) == BAD_NDRANGE
    assert status(width=72) == BAD_NDRANGE and status(height=40) == BAD_NDRANGE and status(width=65536) == BAD_NDRANGE and status(height=65536) == BAD_NDRANGE
    assert status(values=small) == SIZE_MISMATCH and status(t_extreme=small) == SIZE_MISMATCH
    assert status(values=small, t_extreme=small, width=56) == 0 and status(values=small, height=24) == 0
    # the order of the kinds: a value error wins over a region error, a region error over a size error
    assert status(step=0.0, width=12, values=small) == INVALID_VALUE and status(width=12, values=small) == BAD_NDRANGE
    ctx.finish()
    for m in (small, plain, frame, volume):
        m.release()


def _host_lib():
    return host_lib(clvr_host_render_slice=(C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float,
                                                         C.c_float, C.c_int]))


def test_host_mirror_slice_equals_the_binding(gpu_ctx):
    ctx = gpu_ctx
    dims = (48, 40, 36)
    W, H = 256, 128
    vol = scene.phantom(48, dims=dims)
    env = scene.env_map(64, 32)
    volume = ctx.image_from(vol)
    frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
    L = _host_lib()
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, dims[0], dims[1], dims[2], env.ctypes.data, 64, 32)
        L.clvr_host_flush(h, scene.tf_default_source().encode())
        for orientation, (name, position, mode, n, step) in enumerate((("axial", 17.0, sr.MAX, 1, 0.5), ("coronal", 20.25, sr.MEAN, 33, 0.37),
                                                                       ("sagittal", 30.5, sr.MIN, 16, 0.5))):
            ptr = L.clvr_host_render_slice(h, W, H, orientation, position, mode, n, step, 0.0, 2000.0, 0)
            host = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(1024, 2048, 4))[:H, :W].copy()
            plane = scene.slice_plane(dims, name, position, W, H, slab_samples=n, step=step)
            ctx.render_slice(frame, volume, *plane, W, H, mode=mode, slab_samples=n, step=step, window=(0.0, 2000.0))
            mine = frame.pull()
            assert np.array_equal(host, mine), name
            assert (mine[..., 3] == 255).sum() > 1000 and (mine[..., 3] == 0).sum() > 1000 and len(np.unique(mine[..., 0])) > 3
    finally:
        L.clvr_host_destroy(h)
        frame.release()
        volume.release()


def test_headless_slice_writes_the_slab(tmp_path):
    import json
    import subprocess

    dims, W, H = (64, 48, 40), 256, 128
    vol = scene.phantom(64, dims=dims)
    scene.write_nrrd(str(tmp_path / "v.nrrd"), vol)
    rng = np.random.default_rng(5)
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(rng.random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", str(W), str(H)]
    out = subprocess.run([exe, "--slice=coronal,slab=64,mean"] + files + [str(tmp_path / "p.ppm")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert (line["slice"], line["position"], line["slab"], line["mode"], line["frames"]) == ("coronal", 23.5, 64, "mean", 1)
    assert "projection" not in line and "composite" not in line and "isosurface" not in line
    raw = open(tmp_path / "p.ppm", "rb").read()
    header = b"P6\n%d %d\n255\n" % (W, H)
    assert raw.startswith(header)
    ppm = np.frombuffer(raw[len(header):], np.uint8).reshape(H, W, 3)[::-1]  # the PPM's first row is the frame's last
    plane = scene.slice_plane(dims, "coronal", 23.5, W, H, slab_samples=64, step=0.5)
    want, stats = sr.slice_view(vol, *plane, (W, H), modes=(sr.MEAN,), slab_samples=64, step=0.5, window_cw=(0.0, 4000.0))
    assert np.array_equal(ppm, want[sr.MEAN][0][..., :3])
    # (64 samples of 0.5 about row 23.5 of 48 stay inside the volume: every pixel on the cross-section keeps the whole slab)
    assert stats["full"].sum() > 1000 and stats["none"].sum() > 1000 and not stats["cut"].any() and len(np.unique(ppm)) > 10
    for bad in ("--slice=oblique", "--slice=axial,slab=0", "--slice=axial,slab=8193", "--slice=axial,median", "--slice=", "--slice", "--slice=axial,"):
        assert subprocess.run([exe, bad] + files, capture_output=True, text=True, timeout=120).returncode == 1, bad
    for other in ("--projection=max", "--composite", "--isosurface=300"):
        assert subprocess.run([exe, "--slice=axial", other] + files, capture_output=True, text=True, timeout=120).returncode == 1
