"""Hull certificates for marches that start just behind their plane and for rebounds from secondary hits (DESIGN.md 4 item 13;
csrc/primary_kernels.hip: the second word per hit; csrc/render_kernels.hip k_bounce: the relative margin in the opening half, the armed
counter in the step loop, the grant in the certificate phase; csrc/clwh_internal.hpp hull_defer_delta0: the bound and the proof).

The proof, restated: a march of fresh budget 70 that starts at `start` with direction d has the margin m = m_q + n_k . (start - P)
against the plane k of its primary hit (P: the first legs' start point, m_q: P's margin rounded down to 1/16 voxel).  With m >= 0 and
d . n_k >= hull_cert_delta0 it is granted at once (item 12's theorem).  With 0 < -m <= D and d . n_k >= hull_defer_delta0 it is granted
once its counted path has reached ceil(-m / d . n_k), if no event has ended it and it has taken at most J steps: its position is in front
of the plane then and the theorem holds for the 70 - J steps it has left.  A grant ends the march in Exit, which is what the literal march
does, so every frame must equal, bit for bit, the frames without the new grants, without hull certificates, and of short launches (one
pass per launch), which march literally."""
import math
import os
import sys

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests.gpu_util import GpuScene
from tests.test_gpu_hull_cert import DEFAULT_TF, FRAME, GRID, _exact_support, _Scenes, _start_points

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import hull_defer as restated  # noqa: E402

SCENES = ["convex", "grazing", "touching_a_face", "non_cubic", "inside_a_cavity", "piecewise_constant", "on_the_lattice", "corner_posts"]


def _ctx(**env):
    env = {k: str(v) for k, v in env.items()}
    os.environ.update(env)
    try:
        return ffi.Context(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in made:
            made[key] = _ctx(CLWH_TUNE_LONG_LAUNCH=1, **env)
        return made[key]

    yield get
    for ctx in made.values():
        ctx.destroy()


@pytest.fixture(scope="module")
def scenes(orc):
    return _Scenes(orc)


def _render(ctx, scenes, name, seeds, fused=True):
    vol, sdf, pos, d = scenes.get(name)
    g = GpuScene(ctx, vol, sdf, scenes.env, DEFAULT_TF, FRAME)
    if fused:
        g.render(pos, d, None, mode=ffi.ACCUM_IMAGE_SPACE, seeds=seeds, debug=False)
    else:
        for s in seeds:
            g.render(pos, d, s, mode=ffi.ACCUM_IMAGE_SPACE, debug=False)
    out = dict(vol=vol, accum=g.accum[0].pull(np.float32).copy(), frame=g.frame.pull().copy(), hits=ctx.hit_records().copy(),
               codes=ctx.hull_codes().copy(), planes=ctx.hull_planes().copy(), table=ctx.hull_table())
    g.release()
    return out


@pytest.fixture(scope="module")
def literal(gpu_ctx, scenes):
    """per scene, computed once: eight passes, one per launch (short launches march every leg literally)"""
    done = {}

    def get(name):
        if name not in done:
            done[name] = _render(gpu_ctx, scenes, name, scene.glibc_rand(8), fused=False)
        return done[name]

    return get


def _same_frames(a, b, what):
    for key in ("accum", "frame"):
        assert np.array_equal(a[key], b[key]), "%s: %s" % (what, key)


# ---- bit-exactness

@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_frames_equal_with_and_without_the_new_grants(contexts, scenes, literal, name):
    seeds = scene.glibc_rand(8)
    on = _render(contexts(), scenes, name, seeds)
    assert len(on["hits"]) > (300 if name != "grazing" else 50)
    _same_frames(on, _render(contexts(CLWH_TUNE_HULL_DEFER=0), scenes, name, seeds), name + ", against CLWH_TUNE_HULL_DEFER=0")
    _same_frames(on, _render(contexts(CLWH_TUNE_HULL_CERT=0), scenes, name, seeds), name + ", against CLWH_TUNE_HULL_CERT=0")
    _same_frames(on, literal(name), name + ", against one pass per launch")
    if name == "corner_posts":
        # the hull is the whole volume: no start point is in front of a plane; one just inside a face still carries that face's plane
        assert on["table"] is not None and not on["codes"].any()
        assert np.all(((on["planes"] >> 16) & 0xFF).astype(np.int8)[on["planes"] != 0] < 0)
    if name == "piecewise_constant":
        assert np.isnan(_start_points(on["hits"])[1]).any(), "the scene is meant to produce NaN normals"


@pytest.mark.gpu
@pytest.mark.parametrize("cert", [4, 12])
@pytest.mark.parametrize("hint", [1, 0])
@pytest.mark.parametrize("name", ["convex", "grazing"])
def test_frames_equal_along_the_axes_the_armed_counter_shares_its_word_with(contexts, scenes, literal, name, hint, cert):
    on = _render(contexts(CLWH_TUNE_CERT_HINT=hint, CLWH_TUNE_CERT=cert), scenes, name, scene.glibc_rand(8))
    _same_frames(on, literal(name), "%s, hints %d, threshold %d, against one pass per launch" % (name, hint, cert))


# ---- the per-hit word

def _margin32(table, P, k):
    """k_primary's own margin of P against plane k, operation for operation in binary32"""
    e = table[k]
    return ((e[:, 0] * P[:, 0] + e[:, 1] * P[:, 1]) + e[:, 2] * P[:, 2]) - e[:, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["convex", "non_cubic", "touching_a_face", "piecewise_constant"])
def test_the_second_word_per_hit(contexts, scenes, name):
    seeds = scene.glibc_rand(1)
    on = _render(contexts(), scenes, name, seeds)
    off = _render(contexts(CLWH_TUNE_HULL_DEFER=0), scenes, name, seeds)
    by_pixel = lambda out, key: out[key][np.argsort(out["hits"][:, 12], kind="stable")]
    assert np.array_equal(by_pixel(on, "codes"), by_pixel(off, "codes")), "hull_codes does not depend on the knob"
    assert not off["planes"].any()
    vol, table, planes, codes = on["vol"], on["table"], on["planes"], on["codes"]
    _, J, D, scale = ffi.hull_defer_bound(vol.shape[2], vol.shape[1], vol.shape[0])
    assert len(planes) == len(on["hits"]) > 300 and scale == 16
    P, _ = _start_points(on["hits"])
    k = (planes & 0x1FFF).astype(np.int64) - 1
    has = k >= 0
    assert not planes[~has].any() and k.max() < GRID * GRID and not (planes & 0xFF00E000).any()
    with np.errstate(invalid="ignore"):
        assert not has[np.isnan(P).any(axis=1)].any(), "a start point with a NaN has no word"
    stored = ((planes >> 16) & 0xFF).astype(np.int8).astype(np.float64) / scale
    # against the exact support of the event voxels (the table's h_k lies `slack` above it): never more than the true margin
    support = _exact_support((vol >= 500) & (vol <= 1200), table[:, :3])
    kk = np.maximum(k, 0)
    exact = (P.astype(np.float64) * table[kk, :3].astype(np.float64)).sum(axis=1) - support[kk]
    assert np.all(stored[has] <= exact[has])
    # against the table itself: the kernel's binary32 margin, rounded down on the grid; the same sign class; nothing below -D
    m32 = _margin32(table, P, kk)
    assert np.array_equal(stored[has], np.minimum(np.floor(m32[has].astype(np.float64) * scale), 127) / scale)
    assert np.array_equal(stored[has] < 0, m32[has] < 0) and np.all(m32[has] >= -D)
    # the first word names the same plane wherever it names one, and it names one exactly where the margin is not negative
    assert np.array_equal(codes != 0, has & (stored >= 0))
    assert np.array_equal((codes & 0x1FFF)[codes != 0], (planes & 0x1FFF)[codes != 0])
    if name == "convex":
        # Not vacuous.  `python tools/hull_defer.py --shell --rules 3 1.5` (this scene, the restatement alone, on the CPU) reports 18.0 % of the hits
        # with a plane at -1.5 <= margin < 0; the bound stands a fifth below that.
        share = np.count_nonzero(has & (stored < 0)) / len(has)
        assert share >= 0.8 * 0.180, "%.3f of the hits carry a plane behind which they start" % share


# ---- the host bound

def _delta0_restated(X, Y, Z, steps):
    reach = math.sqrt(3.0) * (max(X, Y, Z) + 1)
    cap = min(127, max(X, Y, Z) // 2)
    for k in range(1, 65):
        t = 0.0
        for _ in range(steps):
            if t > reach:
                break
            t += max(1.0, min(float(cap), math.floor(t * (k / 64.0) / math.sqrt(3.0)) - 2.0))
        if t > reach:
            return k / 64.0
    return 2.0


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(64, 64, 64), (512, 512, 512), (300, 40, 1000)])
def test_hull_defer_delta0_equals_its_python_restatement(dims):
    delta0, J, D, scale = ffi.hull_defer_bound(*dims)
    assert (J, D, scale) == (3, 1.5, restated.SCALE)   # what tools/hull_defer.py chooses at 256^3 (profiles/bounce_hull_defer_counters.txt)
    assert delta0 == _delta0_restated(*dims, 70 - 5 - J) == restated.defer_delta0(*dims, J)
    assert ffi.hull_cert_bound(*dims)[0] <= delta0 <= 1.0
    assert D * scale <= 128, "the stored margin's field holds every deficit up to D"


# ---- the restatement alone (no GPU)

def test_restatement_finds_no_wrong_grant_on_a_ball(orc):
    n = 64
    c = (n - 1) / 2.0
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(np.float32)
    vol = np.full((n, n, n), -1000, np.int16)
    vol[np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) < 0.25 * n] = 900
    vol[np.sqrt((x - 10.0) ** 2 + (y - 44.0) ** 2 + (z - 8.0) ** 2) < 0.1 * n] = 900   # and a small one beside it, towards the camera: some first legs hit again and rebound
    sdf = orc.sdf_build(vol, orc.parse_tf(scene.tf_default_source()))[0]
    _, pos, d, (w, h) = restated.shell(n)
    res = restated.measure(vol, sdf, (vol >= 500) & (vol <= 1200), pos, d, w, h, rounds=4)
    for J, D in ((3, 1.5), (9, 8.0)):
        first, rebound = (restated.grants(res[kind], res["dims"], J, D) for kind in ("first", "rebound"))
        assert first["n"] > 1000 and rebound["n"] > 0
        assert first["wrong_at_once"] == first["wrong_deferred"] == rebound["wrong_at_once"] == rebound["wrong_deferred"] == 0
        assert first["at_once"] > 0 and first["deferred"] > 0
        assert rebound["at_once"] + rebound["deferred"] > 0
