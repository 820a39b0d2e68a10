"""-m gpu: hull grants from a plane tilted towards the march's direction (csrc/scene_kernels.hip k_hull_finish: the
table's h_k alone; csrc/render_kernels.hip k_bounce: the tilted-plane test in the opening half, the grant in the certificate phase;
csrc/bounce_device.hpp hull_cell; csrc/clwh_internal.hpp: the constants and the proof, restated in tests/test_hull_tilt_cpu.py).

A grant ends a march in Exit, which is what the literal march does, so every frame must equal, bit for bit, the frame without the rule
(CLWH_TUNE_HULL_TILT=0) and the same seeds one pass per launch -- short launches, which march every leg literally.  The contexts are made
under CLWH_TUNE_LONG_LAUNCH=1 (tests/test_gpu_long_launch.py): at these sizes a launch is otherwise a short one and tests nothing."""
import os
import sys

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests.gpu_util import GpuScene, look_at_centre
from tests.test_gpu_hull_cert import BORDER_TF, DEFAULT_TF, _radius, _scene, _start_points

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import hull_certificate as hc  # noqa: E402
import hull_tilt as restated  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = 64


def _ctx(**env):
    env = {k: str(v) for k, v in env.items()}
    os.environ.update(env)
    try:
        return ffi.Context(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def ctx_on():
    ctx = _ctx(CLWH_TUNE_LONG_LAUNCH=1)
    yield ctx
    ctx.destroy()


@pytest.fixture(scope="module")
def ctx_off():
    ctx = _ctx(CLWH_TUNE_LONG_LAUNCH=1, CLWH_TUNE_HULL_TILT=0)
    yield ctx
    ctx.destroy()


# ---- scenes: (volume, camera position, camera direction, frame, transfer function)

def _ball(n, centre, radius):
    vol = np.full((n, n, n), -1000, np.int16)
    vol[_radius(vol.shape, centre) < radius] = 900
    return vol


def _case(name):
    if name == "shell":   # the 64^3 convex shell of tests/test_gpu_hull_cert.py
        vol, eye, _ = _scene("convex")
        return (vol,) + look_at_centre(vol, eye) + ((128, 96), DEFAULT_TF)
    if name in ("phantom", "phantom_close"):
        vol = scene.phantom(64)
        return (vol,) + tuple(scene.close_camera(64) if name == "phantom_close" else scene.default_camera(64)) + ((160, 96), DEFAULT_TF)
    if name == "non_cubic":   # 64 x 48 x 80: two balls, the smaller one towards the camera
        vol = np.full((80, 48, 64), -900, np.int16)
        vol[_radius(vol.shape, (30.0, 22.0, 44.0)) < 13.0] = 1000
        vol[_radius(vol.shape, (14.0, 34.0, 18.0)) < 6.0] = 800
        return (vol,) + look_at_centre(vol, (-25.0, 90.0, -30.0)) + ((160, 96), DEFAULT_TF)
    if name == "cube16":   # the cap is 8, the bound 1/64: every direction that passes the guards qualifies
        vol = _ball(16, (7.5, 7.5, 7.5), 3.5)
        return (vol,) + look_at_centre(vol, (-8.0, 22.0, -10.0)) + ((128, 96), DEFAULT_TF)
    if name == "no_table":   # the border value 0 is an event: no start table, hence no hull table
        vol, eye, _ = _scene("convex")
        return (vol,) + look_at_centre(vol, eye) + ((128, 96), BORDER_TF)
    vol, eye, d = _scene(name)   # corner_posts, piecewise_constant, on_the_lattice, touching_a_face (tests/test_gpu_hull_cert.py)
    pos, d = look_at_centre(vol, eye) if d is None else (np.array(eye, np.float32), np.array(d, np.float32))
    return vol, pos, d, (128, 96), DEFAULT_TF


class _Cases:
    def __init__(self, orc):
        self.orc, self.env, self._made = orc, scene.env_map(256, 128), {}

    def get(self, name):
        if name not in self._made:
            vol, pos, d, frame, tf = _case(name)
            self._made[name] = (vol, self.orc.sdf_build(vol, self.orc.parse_tf(tf))[0], pos, d, frame, tf)
        return self._made[name]


@pytest.fixture(scope="module")
def cases(orc):
    return _Cases(orc)


def _render(ctx, cases, name, seeds, mode, fused=True):
    vol, sdf, pos, d, frame, tf = cases.get(name)
    g = GpuScene(ctx, vol, sdf, cases.env, tf, frame)
    if fused:
        g.render(pos, d, None, mode=mode, seeds=seeds, debug=True)   # (debug: the pixels' cache entries)
    else:
        for s in seeds:
            g.render(pos, d, s, mode=mode, debug=False)
    out = dict(accum=g.accum[0].pull(np.float32).copy(), cache=g.cache.pull().reshape(-1, 4).copy(), frame=g.frame.pull().copy(),
               entry=g.hit_index.pull().copy(), hits=ctx.hit_records().copy(), planes=ctx.hull_planes().copy(), table=ctx.hull_table(), h=ctx.hull_h())
    g.release()
    return out


def _same(a, b, mode, what, capped=False):
    assert np.array_equal(a["frame"], b["frame"]) or capped, what + ": frame"
    if mode == ffi.ACCUM_IMAGE_SPACE:
        assert np.array_equal(a["accum"], b["accum"]), what + ": accumulator"
    elif not capped:
        assert np.array_equal(a["cache"], b["cache"]), what + ": voxel cache"
    else:
        # Fused, the tokens of a voxel are dealt to its hits in hit order; one pass per launch, to whoever reaches the atomic first.  The
        # counts are equal everywhere, the sums bit for bit wherever the cap of 256 was not reached (planned launches).
        assert np.array_equal(a["cache"][:, 3], b["cache"][:, 3]), what + ": counts"
        below = a["cache"][:, 3] < 256
        assert np.array_equal(a["cache"][below], b["cache"][below]), what + ": entries below the cap"
        assert np.count_nonzero(below & (a["cache"][:, 3] > 0)) > 100, what + ": entries below the cap that hold samples"
        # ... and the frame at every pixel whose voxel stayed below the cap (a pixel's colour is its own entry's mean), misses included
        entry = a["entry"].reshape(-1)
        settled = (entry < 0) | below[np.maximum(entry, 0)]
        assert np.count_nonzero(settled & (entry >= 0)) > 100, what + ": hit pixels whose voxel stayed below the cap"
        assert np.array_equal(a["frame"].reshape(-1, 4)[settled], b["frame"].reshape(-1, 4)[settled]), what + ": frame below the cap"
        print("%s: %d entries hold samples, %d of them at the cap" % (what, np.count_nonzero(a["cache"][:, 3]), np.count_nonzero(~below)))


# ---- bit for bit

@pytest.mark.parametrize("mode", [ffi.ACCUM_IMAGE_SPACE, ffi.ACCUM_VOXEL_CACHE], ids=["image", "planned_voxel_cache"])
@pytest.mark.parametrize("name", ["shell", "phantom", "phantom_close", "non_cubic"])
def test_64_fused_seeds_equal_the_knob_off_and_one_pass_per_launch(gpu_ctx, ctx_on, ctx_off, cases, name, mode):
    seeds = scene.glibc_rand(SEEDS)
    on = _render(ctx_on, cases, name, seeds, mode)
    assert len(on["hits"]) > 300 and on["h"] is not None and on["planes"].any()
    # (voxel-cache mode: a voxel that several hits share reaches its cap of 256 samples with 64 seeds, and which of its hits the tokens
    # go to follows k_primary's hit order, which its per-wave atomic leaves open from camera to camera: two renders of ONE build agree
    # there in the counts only.  Everything else is compared bit for bit.)
    voxel = mode == ffi.ACCUM_VOXEL_CACHE
    _same(on, _render(ctx_off, cases, name, seeds, mode), mode, name + ", against CLWH_TUNE_HULL_TILT=0", capped=voxel)
    _same(on, _render(gpu_ctx, cases, name, seeds, mode, fused=False), mode, name + ", against one pass per launch", capped=voxel)


# ---- the smallest shapes at which the rule can go wrong

@pytest.mark.parametrize("name", ["cube16", "no_table", "corner_posts", "touching_a_face", "on_the_lattice", "piecewise_constant"])
def test_edge_cases_equal_the_knob_off_and_one_pass_per_launch(gpu_ctx, ctx_on, ctx_off, cases, name):
    seeds = scene.glibc_rand(16)
    mode = ffi.ACCUM_IMAGE_SPACE
    on = _render(ctx_on, cases, name, seeds, mode)
    assert len(on["hits"]) > (300 if name != "cube16" else 100)
    _same(on, _render(ctx_off, cases, name, seeds, mode), mode, name + ", against CLWH_TUNE_HULL_TILT=0")
    _same(on, _render(gpu_ctx, cases, name, seeds, mode, fused=False), mode, name + ", against one pass per launch")
    if name == "cube16":
        assert ffi.hull_tilt_bound(16, 16, 16)[0] == 1.0 / 64.0 and on["h"] is not None
    if name == "no_table":
        assert on["table"] is None and on["h"] is None and not on["planes"].any(), "no table: the test is branched out"
    if name == "piecewise_constant":
        nan_normal = np.isnan(_start_points(on["hits"])[1]).any(axis=1)
        assert nan_normal.any(), "the scene is meant to produce NaN normals"
        assert not on["planes"][nan_normal].any(), "hits whose word is 0: the bounce's own (NaN) normal is what gets tilted"
    # (on_the_lattice: an axis-aligned camera on integer coordinates; in every scene three bounce directions in 2048 -- lattice
    # directions of [-1024, 1023]^3 -- have a component of 0, below the 2^-10 guard)


# ---- the derived data

@pytest.mark.parametrize("name", ["shell", "non_cubic", "corner_posts"])
def test_h_alone_holds_the_bits_of_the_tables_fourth_column(ctx_on, ctx_off, cases, name):
    on = _render(ctx_on, cases, name, scene.glibc_rand(1), ffi.ACCUM_IMAGE_SPACE)
    assert on["h"].shape == (64 * 64,) and on["h"].dtype == np.float32
    assert np.array_equal(on["h"].view(np.uint32), on["table"][:, 3].view(np.uint32))
    assert np.isfinite(on["h"]).all()
    off = _render(ctx_off, cases, name, scene.glibc_rand(1), ffi.ACCUM_IMAGE_SPACE)
    assert np.array_equal(off["h"].view(np.uint32), on["h"].view(np.uint32)), "written beside the table under the same condition, whatever the knob"
    by_pixel = lambda out: out["planes"][np.argsort(out["hits"][:, 12], kind="stable")]   # (k_primary's hit order varies from camera to camera)
    assert np.array_equal(by_pixel(off), by_pixel(on)), "the per-hit words do not depend on the knob"


# ---- the device's own encode (any cell is safe, so a wrong one would pass every frame comparison and only lose the yield)

def test_device_hull_cell_inverts_hull_direction_for_all_4096_cells(gpu_ctx):
    k = np.arange(64 * 64, dtype=np.uint32)
    rng = np.random.default_rng(21)
    v = rng.normal(size=(len(k), 3)).astype(np.float32)
    v[0] = (np.nan, 1.0, 0.0)
    v[1] = (0.0, 0.0, 0.0)
    v[2:5] = np.eye(3, dtype=np.float32)
    v[5:8] = -np.eye(3, dtype=np.float32)
    for scale in (1.0, 0.3, 7.0):
        rec = np.empty((len(k), 5), np.uint32)
        rec[:, 0] = k
        rec[:, 1] = np.float32(scale).view(np.uint32)
        rec[:, 2:] = v.view(np.uint32)
        got = gpu_ctx.device_probe(ffi.PROBE_HULL, rec)
        n = got[:, :3].copy().view(np.float32)
        assert np.allclose(n, hc.oct_directions(64), rtol=0, atol=2.0 ** -21), "hull_direction: the table's cell centres, normalised"
        assert np.array_equal(got[:, 3], k), "hull_cell(scale * hull_direction(k)) == k"
        assert got[:, 4].max() < 64 * 64, "whatever it is given, a cell of the table"
        want = restated.encode(v)
        ok = np.isfinite(v).all(axis=1) & (np.abs(v).sum(axis=1) > 0)
        # (v_rcp_f32 against numpy's division: a vector within an ulp of a cell border may land next door)
        assert np.count_nonzero(got[ok, 4] != want[ok]) <= 4
        assert got[0, 4] % 64 == 0, "a NaN is dropped by the clamp: column 0"
