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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MODES = (pr.MAX, pr.MIN, pr.MEAN)


class Proj:
    """a frame + the optional outputs on one context"""

    def __init__(self, ctx, frame_wh, region_wh):
        self.ctx, self.frame_wh, self.region_wh = ctx, frame_wh, region_wh
        fw, fh = frame_wh
        w, h = region_wh
        self.frame = ctx.image([fw, fh], 4, np.uint8, (fh, fw, 4))
        self.values = ctx.buffer(w * h * 4, np.float32, (h, w))
        self.t = ctx.buffer(w * h * 4, np.float32, (h, w))

    def run(self, volume, pos, d, mode, dense=False, **kw):
        fw, fh = self.frame_wh
        self.frame.push(np.full((fh, fw, 4), 7, np.uint8))  # pixels outside the region keep this
        self.ctx.render_projection(self.frame, volume, pos, d, self.region_wh[0], self.region_wh[1], mode=mode, values=self.values,
                                   t_extreme=self.t, dense=dense, **kw)
        frame = self.frame.pull()
        w, h = self.region_wh
        assert np.all(frame[h:] == 7) and np.all(frame[:, w:] == 7)
        return frame[:h, :w], self.values.pull(), self.t.pull()

    def release(self):
        for m in (self.frame, self.values, self.t):
            m.release()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _check(got, want, what=""):
    gf, gv, gt = got
    wf, wv, wt = want
    assert np.array_equal(gf, wf), "frame differs %s: %d pixels" % (what, int((gf != wf).any(axis=-1).sum()))
    assert np.array_equal(_bits(gv), _bits(wv)), "values differ %s: %d pixels" % (what, int((_bits(gv) != _bits(wv)).sum()))
    assert np.array_equal(_bits(gt), _bits(wt)), "t_extreme differs %s: %d pixels" % (what, int((_bits(gt) != _bits(wt)).sum()))


def _compare_all(ctx, vol, pos, d, frame_wh, region_wh, step=0.5, window=(0.0, 1000.0), t_near=0.0, t_far=np.inf, skip_vs_dense=True):
    Z, Y, X = vol.shape
    if X > 1:
        volume, owner = ctx.image_from(vol), None
    else:  # (clwh_image_create refuses a width of 1, as clw_image does; a wrap takes any dims)
        owner = ctx.buffer_from(vol)
        volume = ctx.image_wrap(owner.device_ptr, (X, Y, Z), 1, np.int16)
    p = Proj(ctx, frame_wh, region_wh)
    want = pr.project(vol, pos, d, frame_wh, region_wh, modes=MODES, step=step, window_cw=window, t_near=t_near, t_far=t_far)
    kept = 0
    for mode in MODES:
        got = p.run(volume, pos, d, mode, step=step, window=window, t_near=t_near, t_far=t_far)
        _check(got, want[mode], "mode %d" % mode)
        if mode != pr.MEAN and skip_vs_dense:
            _check(p.run(volume, pos, d, mode, dense=True, step=step, window=window, t_near=t_near, t_far=t_far), want[mode],
                   "dense mode %d" % mode)
        kept = int((~np.isnan(want[mode][1])).sum())
    p.release()
    volume.release()
    if owner is not None:
        owner.release()
    return kept


def _toward(pos, target):
    v = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    return (v / np.linalg.norm(v)).astype(F)


@pytest.mark.parametrize("dims", [(64, 64, 64), (70, 33, 45), (130, 20, 9), (5, 4, 3), (1, 1, 1)])
@pytest.mark.parametrize("pose", ["default", "close", "inside"])
def test_phantoms_from_several_poses(gpu_ctx, dims, pose):
    X, Y, Z = dims
    n = max(dims)
    vol = scene.phantom(n, dims=dims)
    centre = np.array([(X - 1) / 2, (Y - 1) / 2, (Z - 1) / 2], F)
    if pose == "default":  # (aimed at the centre when the default direction would miss a flat or tiny volume)
        pos, d = scene.default_camera(n)
        d = d if X == Y == Z and n >= 8 else _toward(pos, centre)
    elif pose == "close":  # scene.close_camera about the centre of a box that need not be a cube
        d = scene.camera_direction(0.9, 6.183)
        pos = (centre - d * F(0.6 * n)).astype(F)
    else:
        pos, d = np.array([X * 0.45, Y * 0.55, Z * 0.5], F), scene.camera_direction(2.1, 0.4)
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
        "diagonal": (np.array([-8.0, -8.0, -8.0], F), _toward((-8, -8, -8), (40, 24, 32))),
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
             (np.array([-10.0, -3.0, -10.0], F), _toward((-10, -3, -10), (X, 0, Z))),          # rays graze the far corner
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
    _check(first, pr.project(a, pos, d, (64, 48), (64, 48))[pr.MAX])
    volume.push(b)  # a changed volume: rebuilt at the next projection
    _check(p.run(volume, pos, d, pr.MAX), pr.project(b, pos, d, (64, 48), (64, 48))[pr.MAX], "after push")
    ctx.invalidate_derived(scene=False, camera=False, projection=True)
    _check(p.run(volume, pos, d, pr.MAX), pr.project(b, pos, d, (64, 48), (64, 48))[pr.MAX], "after invalidate")
    # two wraps of one pointer with permuted dims: same content version, different layouts
    w1 = ctx.image_wrap(volume.device_ptr, (X, Y, Z), 1, np.int16)
    w2 = ctx.image_wrap(volume.device_ptr, (Z, Y, X), 1, np.int16)
    as2 = b.reshape(X, Y, Z)  # the same bytes read as a Z x Y x X image (x fastest)
    for _ in range(2):
        _check(p.run(w1, pos, d, pr.MIN), pr.project(b, pos, d, (64, 48), (64, 48), modes=(pr.MIN,))[pr.MIN], "wrap 1")
        _check(p.run(w2, pos, d, pr.MIN), pr.project(as2, pos, d, (64, 48), (64, 48), modes=(pr.MIN,))[pr.MIN], "wrap 2")
    # a rewrite through one wrap is seen through the other object of the same pointer
    w1.push(a)
    _check(p.run(volume, pos, d, pr.MEAN), pr.project(a, pos, d, (64, 48), (64, 48), modes=(pr.MEAN,))[pr.MEAN], "after wrap push")
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
            _check(got, pr.project(vol, pos, d, (128, 128), (128, 128), window_cw=(0.0, 1000.0))[pr.MAX])
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
        _check((f[rows], v[rows], t[rows]), want[mode], "mode %d" % mode)
        if mode != pr.MEAN:
            _check(p.run(volume, pos, d, mode, dense=True, window=window), (f, v, t), "dense mode %d" % mode)
    assert (~np.isnan(want[pr.MAX][1])).sum() > 10000
    p.release()
    volume.release()


def _host_lib():
    L = C.CDLL(os.path.join(ROOT, "cl_volume_renderer_amd", "libclvr_host.so"))
    L.clvr_host_create.restype = C.c_void_p
    L.clvr_host_destroy.argtypes = [C.c_void_p]
    L.clvr_host_load.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint]
    L.clvr_host_flush.argtypes = [C.c_void_p, C.c_char_p]
    L.clvr_host_render_projection.restype = C.c_void_p
    L.clvr_host_render_projection.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int,
                                              C.c_float, C.c_float, C.c_float]
    return L


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
