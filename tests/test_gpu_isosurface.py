"""clwh_render_isosurface on the GPU against the numpy restatement of its contract (tests/isosurface_ref.py), bit for bit: the frame,
t_hit and normal on every pixel of the region.  The brick-skipping walk must equal the dense walk (CLWH_ISO_DENSE) wherever both run.
Every family counts what it exercised -- misses with kept samples, refined hits, hits at the first kept sample, hits with a zero
gradient, hits whose cell straddles a brick face and hits whose corners were clamped at a volume face -- so that no comparison is
empty.  The inputs of a family are lists of cases (the *_cases functions), chosen with the reference on the CPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import isosurface_ref as ir
from tests.view_helpers import ROOT, F, toward, image_of, pose as _pose, plant_blocks, quiet_phantom, host_lib, Iso, Comp, Proj

pytestmark = pytest.mark.gpu

INVALID_VALUE, BAD_NDRANGE, SIZE_MISMATCH = 1, 8, 9
FRAME, REGION = (64, 48), (56, 40)


class Tally:
    """what a family's comparisons exercised"""
    KINDS = ("miss_with_samples", "refined", "first", "flat", "straddle", "clamped")

    def __init__(self):
        for k in self.KINDS:
            setattr(self, k, 0)
        self.comparisons = 0

    def add(self, want):
        stats = want[3]
        self.miss_with_samples += int((~stats["hit"] & (stats["n"] > 0)).sum())
        for k in self.KINDS[1:]:
            setattr(self, k, getattr(self, k) + int(stats[k].sum()))
        self.comparisons += 1

    def assert_all(self):
        assert all(getattr(self, k) > 0 for k in self.KINDS) and self.comparisons > 0, vars(self)


def _case(vol, pos, d, iso, frame_wh=FRAME, region_wh=REGION, **kw):
    return dict(vol=vol, pos=pos, d=d, iso=iso, frame_wh=frame_wh, region_wh=region_wh, kw=kw)


def reference_of(case, rows=None):
    c = case
    return ir.isosurface(c["vol"], c["pos"], c["d"], c["frame_wh"], c["region_wh"], c["iso"], rows=rows, **c["kw"])


def _run_family(ctx, cases):
    """reference == skipping walk == dense walk for every case; returns the family's tally"""
    tally = Tally()
    images, outputs = {}, {}
    for c in cases:
        vol = c["vol"]
        if id(vol) not in images:
            images[id(vol)] = image_of(ctx, vol)
        key = (c["frame_wh"], c["region_wh"])
        if key not in outputs:
            outputs[key] = Iso(ctx, *key)
        volume, out = images[id(vol)][0], outputs[key]
        want = reference_of(c)
        kw = dict(c["kw"])
        flags = kw.pop("flags", 0)
        what = "dims %s iso %r %r" % (vol.shape[::-1], c["iso"], c["kw"])
        Iso.check(out.run(volume, c["pos"], c["d"], c["iso"], flags=flags, **kw), want, "skipping, " + what)
        Iso.check(out.run(volume, c["pos"], c["d"], c["iso"], flags=flags | ir.DENSE, **kw), want, "dense, " + what)
        tally.add(want)
    for out in outputs.values():
        out.release()
    for volume, owner in images.values():
        volume.release()
        if owner is not None:
            owner.release()
    return tally


PHANTOM_DIMS = [(64, 64, 64), (70, 33, 45), (130, 20, 9), (5, 4, 3), (1, 1, 1)]
# the shell, inside the ball's range (40 +- 20), above the maximum, below the minimum, exactly a voxel value of the shell
PHANTOM_ISOS = [300.0, 45.5, 1000.0, -1100.0, 900.0]
REFINES = [0, 1, 8, 24]


def phantom_cases(pose):
    """every (dims, iso, above / below); the refinement depths rotate so that each meets every dims and every iso"""
    cases = []
    for i, dims in enumerate(PHANTOM_DIMS):
        vol = scene.phantom(max(dims), dims=dims)
        pos, d = _pose(pose, dims)
        for j, iso in enumerate(PHANTOM_ISOS):
            for b, flags in enumerate((0, ir.BELOW)):
                cases.append(_case(vol, pos, d, iso, flags=flags, refine=REFINES[(i + j + 2 * b) % 4], color=(1.0, 0.8, 0.6)))
    return cases


@pytest.mark.parametrize("pose", ["default", "close", "inside"])
def test_phantoms_from_several_poses(gpu_ctx, pose):
    _run_family(gpu_ctx, phantom_cases(pose)).assert_all()


def random_cases():
    rng = np.random.default_rng(2024)
    cases = []
    for dims in [(24, 24, 24), (17, 9, 33)]:
        X, Y, Z = dims
        vol = plant_blocks(rng.integers(0, 1 << 16, size=(Z, Y, X), dtype=np.uint16).view(np.int16))
        poses = [(np.array([-7.0, -5.0, -9.0], F), toward((-7.0, -5.0, -9.0), (X * 0.3, Y * 0.3, Z * 0.3))),
                 (np.array([X + 6.0, Y + 4.0, Z + 8.0], F), toward((X + 6.0, Y + 4.0, Z + 8.0), (X * 0.7, Y * 0.7, Z * 0.7))),
                 _pose("inside", dims)]
        isos = [float(v) for v in rng.uniform(-30000, 30000, 3).astype(F)] + [32767.0, -32768.0, 25000.25, -25000.75]
        for i, (pos, d) in enumerate(poses):
            for j, iso in enumerate(isos):
                flags = ir.BELOW if (iso < 0) != (j == 2) else 0
                cases.append(_case(vol, pos, d, iso, flags=flags, refine=REFINES[(i + j) % 4], step=(0.5, 0.37, 1.3)[(i + j) % 3],
                                   color=(0.3, 2.0, -1.0), ambient=(0.0, 1.0, 0.3)[j % 3]))
    return cases


def test_random_bit_volumes(gpu_ctx):
    _run_family(gpu_ctx, random_cases()).assert_all()


def slab_and_step_cases():
    n = 48
    noisy, quiet = scene.phantom(n), quiet_phantom(n)
    pos, d = scene.default_camera(n)
    centre = float(np.linalg.norm(np.array([(n - 1) / 2] * 3) - pos))
    cases = []
    for i, step in enumerate([0.37, 0.5, 2.5]):
        for j, (tn, tf) in enumerate([(0.0, np.inf), (centre - 0.33 * n, centre + 0.1 * n), (centre - 0.2 * n, centre), (-5.0, centre - 0.31 * n)]):
            for b, (iso, flags) in enumerate([(300.0, 0), (40.0, 0), (40.0, ir.BELOW), (-1000.0, ir.BELOW)]):
                vol = quiet if (i + j + b) % 2 == 0 else noisy
                cases.append(_case(vol, pos, d, iso, flags=flags, refine=REFINES[(i + j + b) % 4], step=step, t_near=tn, t_far=tf))
    return cases


def test_steps_and_slabs_that_cut_the_surface(gpu_ctx):
    cases = slab_and_step_cases()
    _run_family(gpu_ctx, cases).assert_all()
    # a slab that starts inside the shell: rays whose FIRST kept sample is inside, on a volume where others are refined
    cut = [c for c in cases if c["kw"]["t_near"] > 0 and c["iso"] == 300.0]
    assert cut and all(reference_of(c)[3]["first"].sum() > 0 and reference_of(c)[3]["refined"].sum() > 0 for c in cut[:2])


def axis_cases():
    X, Y, Z = 40, 24, 32
    vol = quiet_phantom(40)[:Z, :Y, :X].copy()
    poses = {
        "axis": (np.array([20.0, 12.0, -6.0], F), np.array([0, 0, 1], F)),
        "face_y0": (np.array([20.0, 0.0, -6.0], F), np.array([0, 0, 1], F)),          # central row runs in the face y = 0
        "edge_x0y0": (np.array([0.0, 0.0, -6.0], F), np.array([0, 0, 1], F)),        # central ray runs along an edge
        "face_xdim": (np.array([40.0, 12.0, -6.0], F), np.array([0, 0, 1], F)),      # x == X is outside
        "straight_up": (np.array([20.0, -5.0, 16.0], F), np.array([0, 1, 0], F)),    # degenerate basis: NaN rays, nothing kept
    }
    cases = []
    for i, (name, (pos, d)) in enumerate(poses.items()):
        for j, (iso, flags) in enumerate([(300.0, 0), (40.0, 0), (-1000.0, ir.BELOW), (2000.0, 0)]):
            cases.append(_case(vol, pos, d, iso, flags=flags, refine=REFINES[(i + j) % 4]))
    return cases


def test_axis_parallel_and_grazing_rays(gpu_ctx):
    cases = axis_cases()
    _run_family(gpu_ctx, cases).assert_all()
    assert not reference_of(cases[-1])[3]["n"].any()  # straight up: no ray keeps a sample


def test_derived_data_follows_the_volume_and_invalidation(gpu_ctx):
    from tests import composite_ref as cr
    from tests import projection_ref as pr

    ctx = gpu_ctx
    X, Y, Z = 24, 16, 40
    a = scene.phantom(40, dims=(X, Y, Z))
    # a's air becomes dense and its ball air: a stale dilated table skips the bricks that now hold the surface
    b = np.where(a < -500, 900, -1000).astype(np.int16)
    c3 = (a[::-1] // 2 + 300).astype(np.int16)
    pos, d = _pose("default", (X, Y, Z))
    wh = (64, 48)
    volume = ctx.image_from(a)
    table = cr.hard_table()
    lut = ctx.buffer_from(table)
    out, comp, proj = Iso(ctx, wh, wh), Comp(ctx, wh, wh), Proj(ctx, wh, wh)
    tally = Tally()
    ctx.invalidate_derived(scene=False, camera=False, projection=True)

    def others(vol, what):
        """a projection and a composite: unchanged bytes whether or not an isosurface call came before"""
        want_p = pr.project(vol, pos, d, wh, wh, modes=(pr.MAX,), window_cw=(0.0, 1000.0))
        Proj.check(proj.run(volume, pos, d, pr.MAX, window=(0.0, 1000.0)), want_p[pr.MAX], "projection " + what)
        Comp.check(comp.run(volume, pos, d, lut, -1024), cr.composite(vol, pos, d, wh, wh, table, -1024), "composite " + what)

    def iso(vol, what, through=None):
        for flags in (0, ir.BELOW):
            want = ir.isosurface(vol, pos, d, wh, wh, 300.0, flags=flags)
            Iso.check(out.run(through or volume, pos, d, 300.0, flags=flags), want, what)
            tally.add(want)

    others(a, "before any isosurface")  # builds the bricked copy; the dilated table does not exist yet
    iso(a, "first")
    others(a, "after the first isosurface")
    volume.push(b)
    iso(b, "after a push")
    alias = ctx.image_wrap(volume.device_ptr, (X, Y, Z), 1, np.int16)
    alias.push(c3)  # rewritten through another object of the same pointer
    iso(c3, "after a push through a wrap")
    iso(c3, "through the wrap", through=alias)
    others(c3, "after the pushes")
    import torch  # another owner of device memory: what it writes, the library does not see

    theirs = torch.from_numpy(a.reshape(-1).copy()).to("cuda")
    torch.cuda.synchronize()
    foreign = ctx.image_wrap(theirs.data_ptr(), (X, Y, Z), 1, np.int16)
    iso(a, "foreign memory", through=foreign)
    ctx.finish()
    theirs.copy_(torch.from_numpy(b.reshape(-1).copy()))
    torch.cuda.synchronize()
    ffi._check(ffi.lib().clwh_mem_mark_dirty(foreign.h), "clwh_mem_mark_dirty")
    iso(b, "after mark_dirty", through=foreign)
    ctx.finish()
    foreign.release()
    iso(c3, "the library's own image again")
    volume.push(a)
    ctx.invalidate_derived(scene=False, camera=False, projection=True)
    iso(a, "after invalidate")
    others(a, "after invalidate")
    ctx.finish()
    for m in (alias, lut, volume):
        m.release()
    for o in (out, comp, proj):
        o.release()
    assert tally.refined > 0 and tally.miss_with_samples > 0 and tally.straddle > 0


def test_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    vol = scene.phantom(16)
    volume = ctx.image_from(vol)
    frame = ctx.image([64, 32], 4, np.uint8, (32, 64, 4))
    plain = ctx.buffer(64 * 32 * 16, np.float32)
    small = ctx.buffer(64 * 32 * 4 - 4, np.float32)
    small_normal = ctx.buffer(64 * 32 * 16 - 4, np.float32)
    pos, d = scene.default_camera(16)

    def status(**kw):
        args = dict(frame=frame, volume=volume, cam_pos=pos, cam_dir=d, width=64, height=32, iso=300.0)
        args.update(kw)
        try:
            ctx.render_isosurface(**args)
            return 0
        except ffi.ClwhError as e:
            return e.status

    assert status() == 0 and status(flags=3) == 0 and status(t_hit=plain, normal=plain) == 0
    assert status(refine=0) == 0 and status(refine=24) == 0 and status(ambient=0.0) == 0 and status(ambient=1.0) == 0
    assert status(iso=65536.0) == 0 and status(iso=-65536.0) == 0 and status(iso=65536.0, flags=ir.BELOW) == 0
    assert status(color=(-3.0, 0.0, 1e30)) == 0
    zero = ffi.IsosurfaceDesc()
    assert ffi.lib().clwh_render_isosurface(ctx.h, C.byref(zero)) == INVALID_VALUE
    zero.frame, zero.volume, zero.width, zero.height = frame.h, volume.h, 64, 32  # everything but the step
    assert ffi.lib().clwh_render_isosurface(ctx.h, C.byref(zero)) == INVALID_VALUE
    zero.step = 0.5
    assert ffi.lib().clwh_render_isosurface(ctx.h, C.byref(zero)) == 0  # (iso 0, refine 0, black, ambient 0: all valid)
    assert ffi.lib().clwh_render_isosurface(ctx.h, None) == INVALID_VALUE and ffi.lib().clwh_render_isosurface(None, C.byref(zero)) == INVALID_VALUE
    zero.frame = None
    assert ffi.lib().clwh_render_isosurface(ctx.h, C.byref(zero)) == INVALID_VALUE
    zero.frame, zero.volume = frame.h, None
    assert ffi.lib().clwh_render_isosurface(ctx.h, C.byref(zero)) == INVALID_VALUE
    assert status(volume=frame) == INVALID_VALUE and status(frame=volume) == INVALID_VALUE
    assert status(frame=plain) == INVALID_VALUE and status(volume=plain) == INVALID_VALUE
    assert status(flags=4) == INVALID_VALUE and status(flags=-1) == INVALID_VALUE and status(flags=1 << 16) == INVALID_VALUE
    for iso in (float("nan"), float("inf"), float("-inf"), 65536.01, -65537.0, 1e30):
        assert status(iso=iso) == INVALID_VALUE
    assert status(refine=-1) == INVALID_VALUE and status(refine=25) == INVALID_VALUE and status(refine=1 << 20) == INVALID_VALUE
    for amb in (-0.01, 1.01, float("nan"), float("inf")):
        assert status(ambient=amb) == INVALID_VALUE
    for bad in (float("nan"), float("inf"), float("-inf")):
        for k in range(3):
            color = [1.0, 1.0, 1.0]
            color[k] = bad
            assert status(color=color) == INVALID_VALUE
    assert status(step=0.0) == INVALID_VALUE and status(step=-1.0) == INVALID_VALUE and status(step=float("nan")) == INVALID_VALUE
    assert status(step=float("inf")) == INVALID_VALUE
    assert status(step=1e-9) == INVALID_VALUE  # the farthest corner lies more than 2^29 steps away
    assert status(cam_pos=(float("nan"), 0.0, 0.0)) == INVALID_VALUE and status(cam_pos=(float("inf"), 0.0, 0.0)) == INVALID_VALUE
    assert status(t_near=5.0, t_far=4.0) == INVALID_VALUE and status(t_near=float("nan")) == INVALID_VALUE
    assert status(t_near=float("inf")) == INVALID_VALUE
    assert status(width=0) == BAD_NDRANGE and status(width=60) == BAD_NDRANGE and status(height=12) == BAD_NDRANGE
    assert status(width=72) == BAD_NDRANGE and status(height=40) == BAD_NDRANGE
    assert status(t_hit=small) == SIZE_MISMATCH and status(normal=small_normal) == SIZE_MISMATCH and status(normal=small) == SIZE_MISMATCH
    assert status(t_hit=small, normal=small_normal, width=56) == 0 and status(t_hit=small, height=24) == 0
    ctx.finish()
    for m in (small_normal, small, plain, frame, volume):
        m.release()


def full_size_pose(n, W, H):
    """the default camera moved sideways so that the middle of the region (the frame's corner) looks at the volume's centre"""
    from tests import projection_ref as pr

    pos, d = scene.default_camera(n)
    centre = np.array([(n - 1) / 2] * 3, np.float64)
    through = pr.generate_ray(d, np.array(W // 2), np.array(H // 2), 1920, 1080).astype(np.float64)
    return (centre - through * np.linalg.norm(centre - pos)).astype(F), d


def test_full_size_512(gpu_ctx):
    ctx = gpu_ctx
    n, W, H = 512, 256, 128
    vol = scene.phantom(n)
    pos, d = full_size_pose(n, W, H)
    volume = ctx.image_from(vol)
    out = Iso(ctx, (1920, 1080), (W, H))
    rows = np.arange(4, H, 16)
    tally = Tally()
    depth = float(np.linalg.norm(np.array([(n - 1) / 2] * 3) - pos))
    # the shell from outside; from a slab that starts inside the shell, the first noisy voxel of the ball at or below 20
    for iso, flags, refine, t_near in ((300.0, 0, 8, 0.0), (20.0, ir.BELOW, 24, depth - 0.33 * n)):
        want = ir.isosurface(vol, pos, d, (1920, 1080), (W, H), iso, flags=flags, refine=refine, t_near=t_near, rows=rows)
        got = out.run(volume, pos, d, iso, flags=flags, refine=refine, t_near=t_near)
        Iso.check(tuple(g[rows] for g in got), want[:3], "skipping")
        Iso.check(out.run(volume, pos, d, iso, flags=flags | ir.DENSE, refine=refine, t_near=t_near), got, "dense")
        tally.add(want)
    assert tally.refined > 1000 and tally.first > 1000 and tally.straddle > 0 and tally.miss_with_samples > 0, vars(tally)
    out.release()
    volume.release()


def _host_lib():
    return host_lib(clvr_host_render_isosurface=(C.c_void_p, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_float,
                                                              C.c_int, C.c_float, C.c_int, C.c_float, C.POINTER(C.c_float)]))


def test_host_mirror_isosurface_equals_the_reference():
    n, W, H = 64, 2048, 1024  # the renderer's whole frame: the view's centre is the frame's
    vol = scene.phantom(n)
    env = scene.env_map(64, 32)
    L = _host_lib()
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, n, n, n, env.ctypes.data, 64, 32)
        L.clvr_host_flush(h, scene.tf_default_source().encode())
        pos, d = scene.default_camera(n)[0], scene.camera_direction(0.9, 6.183)
        c_pos, c_look = (C.c_float * 3)(*pos), (C.c_float * 2)(0.9, 6.183)
        rows = np.arange(3, H, 24)
        for iso, flags, step, refine, ambient, color in ((300.0, 0, 0.5, 8, 0.3, (1.0, 0.8, 0.6)), (0.0, ir.BELOW, 0.37, 3, 0.0, (0.2, 0.4, 1.0)),
                                                        (300.0, ir.DENSE, 1.0, 24, 1.0, (1.0, 1.0, 1.0))):
            ptr = L.clvr_host_render_isosurface(h, c_pos, c_look, W, H, iso, flags, step, refine, ambient, (C.c_float * 3)(*color))
            host = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(1024, 2048, 4))[:H, :W].copy()
            want = ir.isosurface(vol, pos, d, (2048, 1024), (W, H), iso, step=step, refine=refine, flags=flags, color=color, ambient=ambient,
                                 rows=rows)
            assert np.array_equal(host[rows], want[0])
            assert want[3]["hit"].sum() > 1000 and (~want[3]["hit"]).sum() > 1000
    finally:
        L.clvr_host_destroy(h)


@pytest.mark.parametrize("option,iso,flags", [("--isosurface=300", 300.0, 0), ("--isosurface=-200.5,below", -200.5, ir.BELOW)])
def test_headless_isosurface_writes_the_isosurface(tmp_path, option, iso, flags):
    n, W, H = 64, 2048, 1024
    vol = scene.phantom(n)
    scene.write_nrrd(str(tmp_path / "v.nrrd"), vol)
    rng = np.random.default_rng(5)
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(rng.random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    out = subprocess.run([exe, option, str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", str(W), str(H), str(tmp_path / "p.ppm")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["isosurface"] == iso and line["below"] == bool(flags) and line["frames"] == 1
    assert "projection" not in line and "composite" not in line
    raw = open(tmp_path / "p.ppm", "rb").read()
    header = b"P6\n%d %d\n255\n" % (W, H)
    assert raw.startswith(header)
    ppm = np.frombuffer(raw[len(header):], np.uint8).reshape(H, W, 3)[::-1]  # the PPM's first row is the frame's last
    pos, d = scene.default_camera(n)
    rows = np.arange(5, H, 24)
    want = ir.isosurface(vol, pos, d, (2048, 1024), (W, H), iso, step=0.5, refine=8, flags=flags, color=(1.0, 1.0, 1.0), ambient=0.3, rows=rows)
    assert np.array_equal(ppm[rows], want[0][..., :3])
    assert want[3]["hit"].sum() > 1000
    for other in ("--projection=max", "--composite"):
        both = subprocess.run([exe, option, other, str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", str(W), str(H)],
                              capture_output=True, text=True, timeout=120)
        assert both.returncode == 1  # the views exclude each other
    bad = subprocess.run([exe, "--isosurface=bone", str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", str(W), str(H)],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1
