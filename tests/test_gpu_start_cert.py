"""-m gpu: start certificates -- a first leg that is proven to leave the volume ends before its first step (csrc/scene_kernels.hip
k_start_*: the per-voxel, per-octant "free from here" table; csrc/primary_kernels.hip: its byte travels with the hit;
csrc/render_kernels.hip k_bounce, opening half: the grant; csrc/clwh_internal.hpp start_cert_dmin: the step bound).

The table and the bound are compared with numpy / Python restatements; the frames with the certificate on are compared, bit for
bit, with the certificate off and with one pass per launch (single-pass launches are short launches: they march literally)."""
import math
import os

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests.gpu_util import GpuScene, look_at_centre

pytestmark = pytest.mark.gpu

TF_GT_800 = scene.TF_TEST_VALUE_GT_800   # event: value > 800
FRAME = (96, 64)


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
    ctx = _ctx(CLWH_TUNE_LONG_LAUNCH=1, CLWH_TUNE_START_CERT=0)
    yield ctx
    ctx.destroy()


def _expected_table(event):
    """uint8 [z][y][x]: bit o set = no event voxel in the box from the voxel (inclusive) to the volume corner octant o heads for"""
    out = np.zeros(event.shape, np.uint8)
    for o in range(8):
        flips = [ax for ax, bit in ((2, 1), (1, 2), (0, 4)) if not (o & bit)]   # positive direction: accumulate from the far end
        b = np.flip(event, flips) if flips else event
        for ax in range(3):
            b = np.logical_or.accumulate(b, axis=ax)
        b = np.flip(b, flips) if flips else b
        out |= (~b).astype(np.uint8) << o
    return out


def _table_of(ctx, orc, vol, tf):
    """the table the context builds for (vol, the oracle's SDF, tf): one tiny render binds the scene"""
    sdf, _, _ = orc.sdf_build(vol, orc.parse_tf(tf))
    g = GpuScene(ctx, vol, sdf, scene.env_map(64, 32), tf, (8, 8))
    pos, d = look_at_centre(vol, [-20.0, 30.0, -25.0])
    g.render(pos, d, 1, debug=False)
    table = ctx.start_table()
    g.release()
    return table


def _blobs(seed, faces):
    """40 x 24 x 56 voxels (no dimension a multiple of 8), a few random blobs; `faces`: events that touch each face of the volume"""
    rng = np.random.default_rng(seed)
    X, Y, Z = 40, 24, 56
    vol = np.full((Z, Y, X), -900, np.int16)
    z, y, x = np.mgrid[0:Z, 0:Y, 0:X].astype(np.float32)
    for _ in range(4):
        c = rng.random(3) * np.array([X, Y, Z])
        r = float(rng.integers(3, 8))
        vol[(x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 < r * r] = 1000
    if faces:
        vol[0, 5, 7] = vol[Z - 1, 20, 30] = vol[30, 0, 12] = vol[11, Y - 1, 33] = vol[40, 9, 0] = vol[17, 14, X - 1] = 1000
    return vol


@pytest.mark.parametrize("case", ["blobs", "faces", "empty"])
def test_table_equals_its_numpy_restatement(ctx_on, orc, case):
    vol = np.full((56, 24, 40), -900, np.int16) if case == "empty" else _blobs(11 if case == "blobs" else 12, case == "faces")
    table = _table_of(ctx_on, orc, vol, TF_GT_800)
    assert table is not None and table.shape == vol.shape
    want = _expected_table(vol > 800)
    if case == "empty":
        assert want.min() == 255
    else:
        assert 0 < np.count_nonzero(want) < want.size and np.count_nonzero(want == 0) > 0
    assert np.array_equal(table, want)


def _dmin_restated(X, Y, Z):
    """the worst-case recurrence: after a path of length t the step is at least max(1, min(cap, floor(t * dmin) - 2)); cap: the value
    at which the volume's SDF saturates, min(127, largest dimension / 2)"""
    reach = math.sqrt(3.0) * (max(X, Y, Z) + 1)
    cap = min(127, max(X, Y, Z) // 2)
    for k in range(1, 65):
        t = 0
        for _ in range(70 - 5):
            t += max(1, min(cap, (t * k) // 64 - 2))   # floor(t * dmin) with dmin = k / 64
        if t > reach:
            return k / 64.0
    return 2.0


@pytest.mark.parametrize("dims", [(64, 64, 64), (512, 512, 512), (300, 40, 1000)])
def test_start_cert_dmin_equals_its_python_restatement(dims):
    got = ffi.start_cert_dmin(*dims)
    assert got == _dmin_restated(*dims)
    assert 2.0 ** -10 <= got
    if dims == (512, 512, 512):
        assert 0.125 <= got <= 0.1875   # "near 0.15"


# ---- parity

def _phantom_shape():
    """64^3: a ball shell (value 900) cut by a slab of background, the phantom's shape without its noise"""
    n = 64
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(np.float32)
    c = (n - 1) / 2.0
    r = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    vol = np.full((n, n, n), -1000, np.int16)
    vol[r < 0.42 * n] = 40
    vol[(r > 0.30 * n) & (r < 0.36 * n)] = 900
    vol[np.abs(x - c) < 0.05 * n] = -1000
    return vol


OUTSIDE_EYE = (-30.0, 80.0, -40.0)
INSIDE_EYE = (31.5, 31.5, 31.5 - 6.0)   # in the slab, inside the shell


class _Shape:
    def __init__(self, orc):
        self.vol = _phantom_shape()
        self.env = scene.env_map(256, 128)
        self.orc = orc
        self._sdf = {}

    def sdf(self, tf):
        if tf not in self._sdf:
            self._sdf[tf] = self.orc.sdf_build(self.vol, self.orc.parse_tf(tf))[0]
        return self._sdf[tf]

    def camera(self, eye):
        if eye == INSIDE_EYE:
            return np.array(eye, np.float32), np.array([0.0, 0.6, 0.8], np.float32)
        return look_at_centre(self.vol, eye)


@pytest.fixture(scope="module")
def shape(orc):
    return _Shape(orc)


def _render(ctx, shape, tf, eye, mode, seeds, fused, vol=None, sdf=None):
    """what the passes of `seeds` leave behind: one launch of all of them, or a launch per seed with its per-pixel contributions"""
    vol = shape.vol if vol is None else vol
    sdf = shape.sdf(tf) if sdf is None else sdf
    pos, d = shape.camera(eye)
    gmode = ffi.ACCUM_VOXEL_CACHE if mode == "voxel" else ffi.ACCUM_IMAGE_SPACE
    g = GpuScene(ctx, vol, sdf, shape.env, tf, FRAME)
    contrib = []
    if fused:
        g.render(pos, d, None, mode=gmode, seeds=seeds, debug=False)
    else:
        for s in seeds:
            g.render(pos, d, s, mode=gmode, debug=True)
            contrib.append(g.contrib.pull().copy())
    out = dict(accum=g.accum[0].pull(np.float32).copy(), cache=g.cache.pull().copy(), frame=g.frame.pull().copy(), contrib=contrib,
               hits=ctx.hit_records().copy(), table=ctx.start_table())
    g.release()
    return out


def _same(a, b, what):
    for key in ("accum", "cache", "frame"):
        assert np.array_equal(a[key], b[key]), "%s: %s" % (what, key)
    assert len(a["contrib"]) == len(b["contrib"])
    for k, (p, q) in enumerate(zip(a["contrib"], b["contrib"])):
        assert np.array_equal(p, q), "%s: per-pixel contributions of pass %d" % (what, k)


@pytest.mark.parametrize("eye", [OUTSIDE_EYE, INSIDE_EYE], ids=["outside", "inside_the_slab"])
@pytest.mark.parametrize("mode", ["image", "voxel"])
def test_frames_equal_with_and_without_start_certificates(gpu_ctx, ctx_on, ctx_off, shape, mode, eye):
    """8 seeds fused into one long launch (image space; the planned voxel-cache launch) with the certificate on and off and as 8
    single-pass launches; then pass by pass with the per-pixel contributions (long-launch scheduling forced: certificates on)"""
    tf = scene.tf_default_source()
    seeds = scene.glibc_rand(8)
    on = _render(ctx_on, shape, tf, eye, mode, seeds, fused=True)
    off = _render(ctx_off, shape, tf, eye, mode, seeds, fused=True)
    one_by_one = _render(gpu_ctx, shape, tf, eye, mode, seeds, fused=False)
    assert on["table"] is not None and off["table"] is None
    assert len(on["hits"]) > (500 if eye == OUTSIDE_EYE else 0)
    assert not off["hits"][:, 14].any()
    for key in ("accum", "cache", "frame"):
        assert np.array_equal(on[key], off[key]), "on against off: " + key
        assert np.array_equal(on[key], one_by_one[key]), "fused against one pass per launch: " + key
    passes_on = _render(ctx_on, shape, tf, eye, mode, seeds[:3], fused=False)
    passes_off = _render(ctx_off, shape, tf, eye, mode, seeds[:3], fused=False)
    _same(passes_on, passes_off, "pass by pass, on against off")
    for k in range(3):
        assert np.array_equal(passes_on["contrib"][k], one_by_one["contrib"][k]), "per-pixel contributions of pass %d against the short launch" % k


def test_hits_carry_the_tables_byte(ctx_on, shape):
    """not vacuous: at least a quarter of the outside view's hits carry a non-zero mask, and every hit's mask is the restated
    table's byte at the voxel of P = (origin + direction) + normal * 2 (0 where P has no voxel)"""
    tf = scene.tf_default_source()
    out = _render(ctx_on, shape, tf, OUTSIDE_EYE, "image", scene.glibc_rand(1), fused=True)
    hits = out["hits"]
    assert len(hits) > 500
    f = hits[:, :9].copy().view(np.float32)
    p = (f[:, 0:3] + f[:, 3:6]) + f[:, 6:9] * np.float32(2.0)
    assert p.dtype == np.float32
    want_table = _expected_table((shape.vol >= 500) & (shape.vol <= 1200))
    assert np.array_equal(out["table"], want_table)
    n = np.float32(64.0)
    with np.errstate(invalid="ignore"):
        has_voxel = np.all((p >= 0) & (p < n) & ~np.signbit(p), axis=1)
    idx = np.where(has_voxel[:, None], p, 0).astype(np.int64)
    want = np.where(has_voxel, want_table[idx[:, 2], idx[:, 1], idx[:, 0]], 0)
    got = hits[:, 14]
    assert np.array_equal(got, want)
    assert not hits[:, 15].any()
    assert np.count_nonzero(got) * 4 >= len(hits), "%d of %d hits carry a mask" % (np.count_nonzero(got), len(hits))


def test_switched_off_where_it_must_be(gpu_ctx, ctx_on, ctx_off, shape):
    """a table under which the border value 0 is an event, and a table with a `gradient` clause: no start-certificate table, masks
    of 0, and the frames of the path without (CLWH_TUNE_START_CERT=0 is the third way to switch it off: the tests above)"""
    seeds = scene.glibc_rand(4)
    border_tf = scene.tf_rect_source([(-100.0, 1200.0, 0.0, 4000.0, (0.9, 0.6, 0.3, 0.7))])
    for tf in (border_tf, scene.tf_gradient_source()):
        on = _render(ctx_on, shape, tf, OUTSIDE_EYE, "image", seeds, fused=True)
        assert on["table"] is None
        assert len(on["hits"]) > 500 and not on["hits"][:, 14].any()
        off = _render(ctx_off, shape, tf, OUTSIDE_EYE, "image", seeds, fused=True)
        one_by_one = _render(gpu_ctx, shape, tf, OUTSIDE_EYE, "image", seeds, fused=False)
        for key in ("accum", "frame"):
            assert np.array_equal(on[key], off[key]), key
            assert np.array_equal(on[key], one_by_one[key]), key


def test_irregular_sdf_gets_no_certificates(ctx_on, ctx_off, shape):
    """the step bound is proven from step values that grow with the distance from the events; an SDF image that does not (here:
    capped at 4, far below what the volume's own SDF reaches) leaves the table 0, and the frames stay those of the path without"""
    tf = scene.tf_default_source()
    assert shape.sdf(tf).max() > 8
    sdf = np.minimum(shape.sdf(tf), 4).astype(np.int8)
    seeds = scene.glibc_rand(4)
    on = _render(ctx_on, shape, tf, OUTSIDE_EYE, "image", seeds, fused=True, sdf=sdf)
    assert on["table"] is not None and not on["table"].any() and not on["hits"][:, 14].any()
    off = _render(ctx_off, shape, tf, OUTSIDE_EYE, "image", seeds, fused=True, sdf=sdf)
    for key in ("accum", "frame"):
        assert np.array_equal(on[key], off[key]), key
