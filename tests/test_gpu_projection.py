"""clwh_render_projection on the GPU against the numpy restatement of its contract (tests/projection_ref.py), bit for bit: the frame,
the projected values and t_extreme.  Skipping (MAX / MIN without CLWH_PROJ_DENSE) must equal the dense walk on every pixel."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import projection_ref as pr
from tests.view_helpers import ROOT, F, bits, toward, image_of, pose as _pose, host_lib, Proj

pytestmark = pytest.mark.gpu

MODES = (pr.MAX, pr.MIN, pr.MEAN)


def _compare_all(ctx, vol, pos, d, frame_wh, region_wh, step=0.5, window=(0.0, 1000.0), t_near=0.0, t_far=np.inf, skip_vs_dense=True):
    volume, owner = image_of(ctx, vol)
    p = Proj(ctx, frame_wh, region_wh)
    want = pr.project(vol, pos, d, frame_wh, region_wh, modes=MODES, step=step, window_cw=window, t_near=t_near, t_far=t_far)
    kept = 0
    for mode in MODES:
        got = p.run(volume, pos, d, mode, step=step, window=window, t_near=t_near, t_far=t_far)
        Proj.check(got, want[mode], "mode %d" % mode)
        if mode != pr.MEAN and skip_vs_dense:
            Proj.check(p.run(volume, pos, d, mode, dense=True, step=step, window=window, t_near=t_near, t_far=t_far), want[mode],
                   "dense mode %d" % mode)
        kept = int((~np.isnan(want[mode][1])).sum())
    p.release()
    volume.release()
    if owner is not None:
        owner.release()
    return kept


@pytest.mark.parametrize("dims", [(64, 64, 64), (70, 33, 45), (130, 20, 9), (5, 4, 3), (1, 1, 1)])
@pytest.mark.parametrize("pose", ["default", "close", "inside"])
def test_phantoms_from_several_poses(gpu_ctx, dims, pose):
    vol = scene.phantom(max(dims), dims=dims)
    pos, d = _pose(pose, dims)
    kept = _compare_all(gpu_ctx, vol, pos, d, (104, 72), (96, 64), window=(200.0, 1500.0))
    assert kept > 0


@pytest.mark.parametrize("step", [0.37, 0.5, 1.0, 3.0])
def test_steps_and_slabs(gpu_ctx, step):
    vol = scene.phantom(64)
    pos, d = scene.default_camera(64)
    _compare_all(gpu_ctx, vol, pos, d, (96, 64), (96, 64), step=step)
    _compare_all(gpu_ctx, vol, pos, d, (96, 64), (96, 64), step=step, t_near=40.0, t_far=70.0)
    _compare_all(gpu_ctx, vol, pos, d, (96, 64), (96, 64), step=step, t_near=-5.0, t_far=41.0)


@pytest.mark.parametrize("window", [(40.0, 1.0), (900.0, 0.25), (0.0, 1e6), (-30000.0, 3.0)])
def test_windows(gpu_ctx, window):
    vol = scene.phantom(48)
    pos, d = scene.close_camera(48)
    _compare_all(gpu_ctx, vol, pos, d, (64, 64), (64, 64), window=window, skip_vs_dense=False)


@pytest.mark.parametrize("case", ["axis", "face_y0", "edge_x0y0", "face_xdim", "diagonal", "straight_up"])
def test_axis_parallel_and_grazing_rays(gpu_ctx, case):
    X, Y, Z = 40, 24, 32
    vol = scene.phantom(40, dims=(X, Y, Z))
    pos, d = {
        "axis": (np.array([20.0, 12.0, -6.0], F), np.array([0, 0, 1], F)),
        "face_y0": (np.array([20.0, 0.0, -6.0], F), np.array([0, 0, 1], F)),          # central row runs in the face y = 0
        "edge_x0y0": (np.array([0.0, 0.0, -6.0], F), np.array([0, 0, 1], F)),        # central ray runs along an edge
        "face_xdim": (np.array([40.0, 12.0, -6.0], F), np.array([0, 0, 1], F)),      # x == X is outside
        "diagonal": (np.array([-8.0, -8.0, -8.0], F), toward((-8, -8, -8), (40, 24, 32))),
        "straight_up": (np.array([20.0, -5.0, 16.0], F), np.array([0, 1, 0], F)),    # degenerate basis: NaN rays, nothing kept
    }[case]
    kept = _compare_all(gpu_ctx, vol, pos, d, (64, 48), (64, 48))
    assert (kept == 0) == (case == "straight_up")


def _adversarial_volumes():
    rng = np.random.default_rng(7)
    X, Y, Z = 72, 40, 56
    noise = rng.integers(-50, 51, size=(Z, Y, X)).astype(np.int16)
    for (z, y, x) in [(0, 0, 0), (Z - 1, Y - 1, X - 1), (0, Y - 1, 8), (Z - 1, 0, X - 9)]:  # corners and faces: grazed bricks
        noise[z, y, x] = 32767
    noise[Z - 1, Y - 1, 0] = -32768
    noise[0, 0, X - 1] = -32768
    extremes = rng.choice(np.array([-32768, 32767, 0, -1], np.int16), size=(Z, Y, X)).astype(np.int16)
    ties = rng.integers(0, 2, size=(Z, Y, X)).astype(np.int16)
    sparse = np.full((Z, Y, X), -1000, np.int16)
    sparse[rng.integers(0, Z, 40), rng.integers(0, Y, 40), rng.integers(0, X, 40)] = rng.integers(-32768, 32768, 40).astype(np.int16)
    return {"noise": noise, "extremes": extremes, "ties": ties, "sparse": sparse}


@pytest.mark.parametrize("name", ["noise", "extremes", "ties", "sparse"])
def test_adversarial_volumes_skipping_equals_dense(gpu_ctx, name):
    vol = _adversarial_volumes()[name]
    Z, Y, X = vol.shape
    poses = [scene.default_camera(X), scene.close_camera(X),
             (np.array([-10.0, -3.0, -10.0], F), toward((-10, -3, -10), (X, 0, Z))),          # rays graze the far corner
             (np.array([X + 5.0, Y * 0.5, Z * 0.5], F), np.array([-1, 0, 0], F)),
             (np.array([X * 0.5, Y * 0.5, Z * 0.5], F), scene.camera_direction(4.0, 0.3))]
    for pos, d in poses:
        _compare_all(gpu_ctx, vol, pos, d, (80, 64), (80, 64), window=(0.0, 65536.0))


def test_cache_follows_pushes_wraps_and_invalidation(gpu_ctx):
    ctx = gpu_ctx
    X, Y, Z = 24, 16, 40
    a = scene.phantom(40, dims=(X, Y, Z))
    b = (a[::-1] // 2 + 300).astype(np.int16)
    pos, d = scene.default_camera(40)
    volume = ctx.image_from(a)
    p = Proj(ctx, (64, 48), (64, 48))
    first = p.run(volume, pos, d, pr.MAX)
    Proj.check(first, pr.project(a, pos, d, (64, 48), (64, 48))[pr.MAX])
    volume.push(b)  # a changed volume: rebuilt at the next projection
    Proj.check(p.run(volume, pos, d, pr.MAX), pr.project(b, pos, d, (64, 48), (64, 48))[pr.MAX], "after push")
    ctx.invalidate_derived(scene=False, camera=False, projection=True)
    Proj.check(p.run(volume, pos, d, pr.MAX), pr.project(b, pos, d, (64, 48), (64, 48))[pr.MAX], "after invalidate")
    # two wraps of one pointer with permuted dims: same content version, different layouts
    w1 = ctx.image_wrap(volume.device_ptr, (X, Y, Z), 1, np.int16)
    w2 = ctx.image_wrap(volume.device_ptr, (Z, Y, X), 1, np.int16)
    as2 = b.reshape(X, Y, Z)  # the same bytes read as a Z x Y x X image (x fastest)
    for _ in range(2):
        Proj.check(p.run(w1, pos, d, pr.MIN), pr.project(b, pos, d, (64, 48), (64, 48), modes=(pr.MIN,))[pr.MIN], "wrap 1")
        Proj.check(p.run(w2, pos, d, pr.MIN), pr.project(as2, pos, d, (64, 48), (64, 48), modes=(pr.MIN,))[pr.MIN], "wrap 2")
    # a rewrite through one wrap is seen through the other object of the same pointer
    w1.push(a)
    Proj.check(p.run(volume, pos, d, pr.MEAN), pr.project(a, pos, d, (64, 48), (64, 48), modes=(pr.MEAN,))[pr.MEAN], "after wrap push")
    ctx.finish()
    for m in (w1, w2, volume):
        m.release()
    p.release()


def test_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    vol = scene.phantom(16)
    volume = ctx.image_from(vol)
    frame = ctx.image([64, 32], 4, np.uint8, (32, 64, 4))
    small = ctx.buffer(64 * 32 * 4 - 4, np.float32)
    pos, d = scene.default_camera(16)

    def status(**kw):
        args = dict(frame=frame, volume=volume, cam_pos=pos, cam_dir=d, width=64, height=32)
        args.update(kw)
        try:
            ctx.render_projection(**args)
            return 0
        except ffi.ClwhError as e:
            return e.status

    assert status() == 0
    assert status(mode=3) == 1 and status(mode=-1) == 1
    assert status(step=0.0) == 1 and status(step=-1.0) == 1 and status(step=float("nan")) == 1 and status(step=float("inf")) == 1
    assert status(step=1e-9) == 1  # the farthest corner lies more than 2^29 steps away
    assert status(window=(0.0, 0.0)) == 1 and status(window=(float("nan"), 1.0)) == 1 and status(window=(0.0, float("inf"))) == 1
    assert status(t_near=5.0, t_far=4.0) == 1 and status(t_near=float("nan")) == 1 and status(t_near=float("inf")) == 1
    assert status(volume=frame) == 1 and status(frame=volume) == 1
    assert status(width=0) == 8 and status(width=60) == 8 and status(height=12) == 8 and status(width=72) == 8 and status(height=40) == 8
    assert status(values=small) == 9 and status(t_extreme=small) == 9
    for m in (volume, frame, small):
        m.release()


def test_nan_camera_position_is_accepted_and_keeps_no_sample(gpu_ctx):
    """the one difference between the views' camera checks (include/clwh.h): the projection does not refuse a NaN camera position --
    every pixel has no kept sample -- while the compositor and the isosurface return CLWH_ERR_INVALID_VALUE for the same camera"""
    ctx = gpu_ctx
    volume = ctx.image_from(scene.phantom(16))
    frame = ctx.image([16, 16], 4, np.uint8, (16, 16, 4))
    values, t_extreme = ctx.buffer(16 * 16 * 4, np.float32, (16, 16)), ctx.buffer(16 * 16 * 4, np.float32, (16, 16))
    lut = ctx.buffer_from(np.ones((16, 4), np.float32))
    frame.push(np.full((16, 16, 4), 255, np.uint8))
    pos, d = np.array([np.nan, 0.0, 0.0], F), scene.default_camera(16)[1]

    def status(render, **kw):
        try:
            render(frame, volume, pos, d, 16, 16, **kw)
            return 0
        except ffi.ClwhError as e:
            return e.status

    assert status(ctx.render_projection, mode=pr.MAX, values=values, t_extreme=t_extreme) == 0
    assert not frame.pull().any()
    assert (bits(values.pull()) == 0x7FC00000).all() and (bits(t_extreme.pull()) == 0x7FC00000).all()
    assert status(ctx.render_composite, lut=lut, lut_first=0) == 1
    assert status(ctx.render_isosurface, iso=300.0) == 1
    pos = scene.default_camera(16)[0]  # the same calls with a finite position: the camera was what they refused
    assert status(ctx.render_composite, lut=lut, lut_first=0) == 0
    assert status(ctx.render_isosurface, iso=300.0) == 0
    for m in (volume, frame, values, t_extreme, lut):
        m.release()


def test_no_interference_with_the_path_tracer(gpu_ctx, orc):
    """projections interleaved with multi-seed render passes on one context: the path tracer's frame and voxel cache equal those of a
    context that never projected"""
    from tests.gpu_util import GpuScene

    n = 48
    vol = scene.phantom(n)
    tf = scene.tf_default_source()
    sdf, _, _ = orc.sdf_build(vol, orc.parse_tf(tf))
    env = scene.env_map(256, 128)
    pos, d = scene.default_camera(n)
    seeds = scene.glibc_rand(8)
    other = ffi.Context(0)
    results = []
    for ctx, project in ((gpu_ctx, True), (other, False)):
        s = GpuScene(ctx, vol, sdf, env, tf, (128, 128))
        p = Proj(ctx, (128, 128), (128, 128)) if project else None
        for i in range(4):
            if project:
                p.run(s.volume, pos, d, MODES[i % 3], window=(0.0, 1000.0))
            s.render(pos, d, 0, seeds=seeds[2 * i:2 * i + 2], debug=False)
            if project:
                got = p.run(s.volume, pos, d, pr.MAX, window=(0.0, 1000.0))
        ctx.finish()
        results.append((s.frame.pull(), s.cache.pull()))
        if project:
            Proj.check(got, pr.project(vol, pos, d, (128, 128), (128, 128), window_cw=(0.0, 1000.0))[pr.MAX])
            p.release()
        s.release()
    other.destroy()
    assert np.array_equal(results[0][0], results[1][0])
    assert np.array_equal(results[0][1], results[1][1])


def test_full_size_512(gpu_ctx):
    ctx = gpu_ctx
    n, W, H = 512, 1920, 1080 // 8 * 8
    vol = scene.phantom(n)
    pos, d = scene.default_camera(n)
    volume = ctx.image_from(vol)
    p = Proj(ctx, (1920, 1080), (W, H))
    rows = np.arange(0, H, 16)
    window = (0.0, 2000.0)
    want = pr.project(vol, pos, d, (1920, 1080), (W, H), modes=MODES, window_cw=window, rows=rows)
    for mode in MODES:
        f, v, t = p.run(volume, pos, d, mode, window=window)
        Proj.check((f[rows], v[rows], t[rows]), want[mode], "mode %d" % mode)
        if mode != pr.MEAN:
            Proj.check(p.run(volume, pos, d, mode, dense=True, window=window), (f, v, t), "dense mode %d" % mode)
    assert (~np.isnan(want[pr.MAX][1])).sum() > 10000
    p.release()
    volume.release()


def _host_lib():
    return host_lib(clvr_host_render_projection=(C.c_void_p, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int,
                                                              C.c_float, C.c_float, C.c_float]))


def test_host_mirror_projection_equals_the_ffi_frame(gpu_ctx):
    n, W, H = 64, 2048, 1024  # the renderer's whole frame: the view's centre is the frame's
    vol = scene.phantom(n)
    env = scene.env_map(64, 32)
    L = _host_lib()
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, n, n, n, env.ctypes.data, 64, 32)
        L.clvr_host_flush(h, scene.tf_default_source().encode())
        pos = (C.c_float * 3)(*scene.default_camera(n)[0])
        look = (C.c_float * 2)(0.9, 6.183)
        volume = gpu_ctx.image_from(vol)
        p = Proj(gpu_ctx, (2048, 1024), (W, H))
        for mode, step in ((pr.MAX, 0.5), (pr.MIN, 0.37), (pr.MEAN, 1.0)):
            ptr = L.clvr_host_render_projection(h, pos, look, W, H, mode, 100.0, 1800.0, step)
            host = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(1024, 2048, 4))[:H, :W].copy()
            got = p.run(volume, np.array(list(pos), F), scene.camera_direction(0.9, 6.183), mode, step=step, window=(100.0, 1800.0))
            assert np.array_equal(host, got[0])
            assert (host[..., 3] == 255).sum() > 1000
        p.release()
        volume.release()
    finally:
        L.clvr_host_destroy(h)


def test_headless_projection_writes_the_projection(tmp_path):
    n, W, H = 96, 2048, 1024
    vol = scene.phantom(n)
    scene.write_nrrd(str(tmp_path / "v.nrrd"), vol)
    rng = np.random.default_rng(5)
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(rng.random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    out = subprocess.run([exe, "--projection=max", str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", str(W), str(H),
                          str(tmp_path / "p.ppm")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["projection"] == "max" and line["frames"] == 1
    raw = open(tmp_path / "p.ppm", "rb").read()
    header = b"P6\n%d %d\n255\n" % (W, H)
    assert raw.startswith(header)
    ppm = np.frombuffer(raw[len(header):], np.uint8).reshape(H, W, 3)[::-1]  # the PPM's first row is the frame's last
    pos, d = scene.default_camera(n)
    rows = np.arange(0, H, 8)
    want = pr.project(vol, pos, d, (2048, 1024), (W, H), window_cw=(0.0, 4000.0), rows=rows)[pr.MAX][0]
    assert np.array_equal(ppm[rows], want[..., :3])
    assert (want[..., 3] == 255).sum() > 1000
