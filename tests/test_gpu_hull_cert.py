"""-m gpu: hull certificates -- a first leg that heads away from a plane with every event voxel behind it ends before its first step
(csrc/scene_kernels.hip k_hull_*: the support table; csrc/primary_kernels.hip: the plane search per hit; csrc/render_kernels.hip
k_bounce, opening half: the grant; csrc/clwh_internal.hpp hull_cert_delta0: the step bound).

The table, the planes the hits carry and the bound are compared with the numpy / Python restatements of tools/hull_certificate.py;
the frames with the certificate on are compared, bit for bit, with CLWH_TUNE_HULL_CERT=0 and with one pass per launch (single-pass
launches are short launches: they march literally)."""
import math
import os
import sys

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests.gpu_util import GpuScene, look_at_centre

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import hull_certificate as restated  # noqa: E402

pytestmark = pytest.mark.gpu

FRAME = (128, 96)
GRID = 64
DEFAULT_TF = scene.tf_default_source()   # event: 500 <= value <= 1200
BORDER_TF = scene.tf_rect_source([(-100.0, 1200.0, 0.0, 4000.0, (0.9, 0.6, 0.3, 0.7))])   # the border value 0 is an event


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
    ctx = _ctx(CLWH_TUNE_LONG_LAUNCH=1, CLWH_TUNE_HULL_CERT=0)
    yield ctx
    ctx.destroy()


# ---- scenes

def _radius(shape, centre):
    Z, Y, X = shape
    z, y, x = np.mgrid[0:Z, 0:Y, 0:X].astype(np.float32)
    return np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)


def _shell(n=64, slab=False):
    """a ball shell of `bone` around soft tissue; `slab`: cut open, the phantom's shape"""
    c = (n - 1) / 2.0
    r = _radius((n, n, n), (c, c, c))
    vol = np.full((n, n, n), -1000, np.int16)
    vol[r < 0.42 * n] = 40
    vol[(r > 0.30 * n) & (r < 0.36 * n)] = 900
    if slab:
        x = np.arange(n, dtype=np.float32)[None, None, :]
        vol[np.broadcast_to(np.abs(x - c) < 0.05 * n, vol.shape)] = -1000
    return vol


def _scene(name):
    """(volume, eye, explicit direction or None: look at the centre)"""
    if name == "convex":
        return _shell(), (-30.0, 80.0, -40.0), None
    if name == "corner_posts":   # an event voxel in every corner: the hull is the whole volume, no start point is outside it
        vol = _shell()
        for z in (0, 63):
            for y in (0, 63):
                for x in (0, 63):
                    vol[z, y, x] = 900
        return vol, (-30.0, 80.0, -40.0), None
    if name == "touching_a_face":
        vol = np.full((72, 72, 72), -1000, np.int16)
        vol[_radius(vol.shape, (3.0, 36.0, 30.0)) < 20.0] = 900
        return vol, (-25.0, 70.0, -30.0), None
    if name == "inside_a_cavity":
        return _shell(slab=True), (31.5, 31.5, 31.5 - 6.0), (0.0, 0.6, 0.8)
    if name == "grazing":
        return _shell(), (-20.0, 31.5 + 0.36 * 64 - 1.0, 31.5), (1.0, 0.0, 0.0)
    if name == "non_cubic":   # 40 x 56 x 72: two balls
        vol = np.full((72, 56, 40), -900, np.int16)
        vol[_radius(vol.shape, (18.0, 25.0, 30.0)) < 11.0] = 1000
        vol[_radius(vol.shape, (26.0, 38.0, 52.0)) < 7.0] = 800
        return vol, (-25.0, 90.0, -30.0), None
    if name == "piecewise_constant":   # zero gradients -> NaN normals (tests/test_gpu_long_launch.py)
        coarse = np.random.default_rng(77).choice(np.array([-1000, 700, 900, 1100, 40], np.int16), size=(11, 11, 11))
        return np.ascontiguousarray(np.kron(coarse, np.ones((6, 6, 6), np.int16)).astype(np.int16)), (-15.0, 30.0, -20.0), None
    if name == "on_the_lattice":   # an axis-aligned camera on integer coordinates: positions on the faces, direction components of 0
        vol = np.full((64, 64, 64), -700, np.int16)
        vol[24:40, 24:40, 24:40] = 1000
        return vol, (32.0, 32.0, -24.0), (0.0, 0.0, 1.0)
    raise ValueError(name)


class _Scenes:
    def __init__(self, orc):
        self.orc, self.env, self._sdf = orc, scene.env_map(256, 128), {}

    def get(self, name, tf=DEFAULT_TF):
        vol, eye, d = _scene(name)
        if (name, tf) not in self._sdf:
            self._sdf[(name, tf)] = self.orc.sdf_build(vol, self.orc.parse_tf(tf))[0]
        if d is None:
            pos, d = look_at_centre(vol, eye)
        else:
            pos, d = np.array(eye, np.float32), np.array(d, np.float32)
        return vol, self._sdf[(name, tf)], pos, d


@pytest.fixture(scope="module")
def scenes(orc):
    return _Scenes(orc)


def _render(ctx, scenes, vol, sdf, tf, pos, d, seeds, fused):
    g = GpuScene(ctx, vol, sdf, scenes.env, tf, FRAME)
    if fused:
        g.render(pos, d, None, mode=ffi.ACCUM_IMAGE_SPACE, seeds=seeds, debug=False)
    else:
        for s in seeds:
            g.render(pos, d, s, mode=ffi.ACCUM_IMAGE_SPACE, debug=False)
    out = dict(accum=g.accum[0].pull(np.float32).copy(), frame=g.frame.pull().copy(), hits=ctx.hit_records().copy(),
               codes=ctx.hull_codes().copy(), table=ctx.hull_table())
    g.release()
    return out


def _three_ways(gpu_ctx, ctx_on, ctx_off, scenes, name, tf=DEFAULT_TF, sdf=None, n_seeds=8):
    vol, sdf0, pos, d = scenes.get(name, tf)
    sdf = sdf0 if sdf is None else sdf
    seeds = scene.glibc_rand(n_seeds)
    on = _render(ctx_on, scenes, vol, sdf, tf, pos, d, seeds, fused=True)
    off = _render(ctx_off, scenes, vol, sdf, tf, pos, d, seeds, fused=True)
    one_by_one = _render(gpu_ctx, scenes, vol, sdf, tf, pos, d, seeds, fused=False)
    assert off["table"] is None and not off["codes"].any()
    # (the hits are compacted in the order the waves arrive: compared by pixel)
    by_pixel = lambda hits: hits[np.argsort(hits[:, 12], kind="stable")]
    assert np.array_equal(by_pixel(on["hits"]), by_pixel(off["hits"])), "the hit records do not depend on the certificate"
    for key in ("accum", "frame"):
        assert np.array_equal(on[key], off[key]), "%s, on against off: %s" % (name, key)
        assert np.array_equal(on[key], one_by_one[key]), "%s, fused against one pass per launch: %s" % (name, key)
    return vol, on


def _start_points(hits):
    f = hits[:, :9].copy().view(np.float32)
    return ((f[:, 0:3] + f[:, 3:6]) + f[:, 6:9] * np.float32(2.0)).astype(np.float32), f[:, 6:9]


def _exact_support(event, normals):
    return restated.support_table(event, normals.astype(np.float64))


def _check_table_and_codes(vol, out, event):
    """the table against its restatement; every code against the table"""
    table, codes, hits = out["table"], out["codes"], out["hits"]
    delta0, slack = ffi.hull_cert_bound(vol.shape[2], vol.shape[1], vol.shape[0])
    assert table is not None and table.shape == (GRID * GRID, 4) and len(codes) == len(hits)
    want_n = restated.oct_directions(GRID, unit=True)
    assert np.abs(table[:, :3].astype(np.float64) - want_n).max() < 1e-6
    # h_k is an upper bound of the support in the direction the kernels use (the table's own binary32 n_k), by the slack within 2^-9
    support = _exact_support(event, table[:, :3])
    over = table[:, 3].astype(np.float64) - support
    assert over.min() >= slack - 2.0 ** -9 and over.max() <= slack + 2.0 ** -9, (over.min(), over.max(), slack)
    # codes: a named plane has every corner of every event voxel behind it (the line above) and the hit's start point in front of it
    # by at least the stored margin
    P, normal = _start_points(hits)
    k = (codes & 0x1FFF).astype(np.int64) - 1
    has = k >= 0
    assert not (codes[~has]).any()
    assert k.max() < GRID * GRID
    n_k = table[np.maximum(k, 0), :3].astype(np.float64)
    margin = (P.astype(np.float64) * n_k).sum(axis=1) - support[np.maximum(k, 0)]
    stored = (codes >> 16).astype(np.float64) / 256.0
    assert np.all(stored[has] <= margin[has])
    assert np.all(margin[has] > 0)
    with np.errstate(invalid="ignore"):
        assert not has[np.isnan(P).any(axis=1)].any(), "a start point with a NaN has no plane"
    return has


# ---- table and plane choice

@pytest.mark.parametrize("name", ["convex", "non_cubic", "touching_a_face"])
def test_table_and_codes_equal_their_numpy_restatement(ctx_on, scenes, name):
    vol, sdf, pos, d = scenes.get(name)
    out = _render(ctx_on, scenes, vol, sdf, DEFAULT_TF, pos, d, scene.glibc_rand(1), fused=True)
    assert len(out["hits"]) > 300
    has = _check_table_and_codes(vol, out, (vol >= 500) & (vol <= 1200))
    if name == "convex":
        # not vacuous: at least one hit in three carries a plane (tests/test_hull_certificate_tool.py: the restatement alone agrees)
        assert 3 * np.count_nonzero(has) >= len(has), "%d of %d hits carry a plane" % (np.count_nonzero(has), len(has))
        # the kernel's two-level search finds a plane for nearly every hit the whole table has one for
        P, _ = _start_points(out["hits"])
        best = (P.astype(np.float64) @ out["table"][:, :3].astype(np.float64).T - out["table"][None, :, 3]).max(axis=1)
        assert np.count_nonzero(has) >= 0.9 * np.count_nonzero(best >= 0)


# ---- bit-exactness

@pytest.mark.parametrize("name", ["convex", "touching_a_face", "inside_a_cavity", "grazing", "non_cubic", "piecewise_constant", "on_the_lattice"])
def test_frames_equal_with_and_without_hull_certificates(gpu_ctx, ctx_on, ctx_off, scenes, name):
    vol, on = _three_ways(gpu_ctx, ctx_on, ctx_off, scenes, name)
    assert len(on["hits"]) > (300 if name != "grazing" else 50)
    has = _check_table_and_codes(vol, on, (vol >= 500) & (vol <= 1200))
    if name in ("convex", "touching_a_face", "non_cubic", "grazing"):
        assert has.any()
    if name == "piecewise_constant":
        _, normal = _start_points(on["hits"])
        assert np.isnan(normal).any(), "the scene is meant to produce NaN normals"


def test_no_hit_has_a_plane_when_the_hull_is_the_volume(gpu_ctx, ctx_on, ctx_off, scenes):
    vol, on = _three_ways(gpu_ctx, ctx_on, ctx_off, scenes, "corner_posts")
    assert len(on["hits"]) > 300
    has = _check_table_and_codes(vol, on, (vol >= 500) & (vol <= 1200))
    assert not has.any() and not on["codes"].any()


def test_switched_off_where_it_must_be(gpu_ctx, ctx_on, ctx_off, scenes):
    """an SDF image whose steps do not grow with the distance from the events (capped at 4): every h_k is +inf, no hit has a plane;
    a table under which the border value 0 is an event: no hull table at all"""
    vol, sdf, _, _ = scenes.get("convex")
    assert sdf.max() > 8
    _, on = _three_ways(gpu_ctx, ctx_on, ctx_off, scenes, "convex", sdf=np.minimum(sdf, 4).astype(np.int8), n_seeds=4)
    assert on["table"] is not None and np.isposinf(on["table"][:, 3]).all() and not on["codes"].any()
    _, on = _three_ways(gpu_ctx, ctx_on, ctx_off, scenes, "convex", tf=BORDER_TF, n_seeds=4)
    assert on["table"] is None and len(on["hits"]) > 300 and not on["codes"].any()


# ---- the host bound

def _delta0_restated(X, Y, Z):
    """the worst-case recurrence: after a path t the step is at least max(1, min(cap, floor(t * delta0 / sqrt 3) - 2))"""
    reach = math.sqrt(3.0) * (max(X, Y, Z) + 1)
    cap = min(127, max(X, Y, Z) // 2)
    for k in range(1, 65):
        t = 0.0
        for _ in range(70 - 5):
            if t > reach:
                break
            t += max(1.0, min(float(cap), math.floor(t * (k / 64.0) / math.sqrt(3.0)) - 2.0))
        if t > reach:
            return k / 64.0
    return 2.0


@pytest.mark.parametrize("dims", [(64, 64, 64), (512, 512, 512), (300, 40, 1000)])
def test_hull_cert_delta0_equals_its_python_restatement(dims):
    delta0, slack = ffi.hull_cert_bound(*dims)
    assert delta0 == _delta0_restated(*dims) == restated.hull_delta0(*dims, m0=0.0)
    assert slack == 0.0625
    assert 2.0 ** -10 < delta0 <= 1.0
