"""-m gpu: k_bounce's refill in the middle of a launch -- a lane whose sample ends takes its next item and starts it in the
same event phase (csrc/render_kernels.hip, k_bounce: closing half, refill, opening half) -- against the oracle.

launch_bounce never starts more lanes than items, so on the small scenes of the other tests every lane gets exactly one item
and the refill runs once, on an empty wave.  The contexts here are created under CLWH_TUNE_LONG_LAUNCH=1 and
CLWH_TUNE_BLOCKS=2: a persistent grid of two blocks (eight waves, 512 lanes), on which every lane works through dozens of
items, with CLWH_TUNE_REFILL = 1 (every finished lane is refilled at once), 16 (the long launch's default) and 64 (a wave
refills only when it is empty).  Placement only: every setting must give the oracle's bits.

The oracle's SDFs and passes are computed once per scene (module fixtures) and shared by the three settings."""
import os

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests.gpu_util import GpuScene, look_at_centre, small_scene
from tests.test_gpu_long_launch import _ball_in_empty_space
from tests.test_gpu_render import _compare_passes

pytestmark = pytest.mark.gpu

BALL_FRAME = (320, 200)


@pytest.fixture(scope="module", params=[1, 16, 64])
def ctx_two_blocks(request):
    """every launch scheduled like a long one, on two blocks, refilling at `param` idle lanes (the knobs are read when the
    context is created: set the environment, create the context, restore the environment)"""
    env = {"CLWH_TUNE_LONG_LAUNCH": "1", "CLWH_TUNE_BLOCKS": "2", "CLWH_TUNE_REFILL": str(request.param)}
    os.environ.update(env)
    try:
        ctx = ffi.Context(0)
    finally:
        for k in env:
            del os.environ[k]
    yield ctx
    ctx.destroy()


class _Ball:
    """the 160^3 ball of test_ball_in_empty_space_certificates_granted and, per (TF, camera, mode, seeds), the oracle's result"""

    def __init__(self, orc):
        self.orc = orc
        self.vol = _ball_in_empty_space(160, 30.0, centre=[70, 90, 80])
        self.env = scene.env_map(512, 256)
        self._sdf = {}
        self._ref = {}

    def sdf(self, tf):
        if tf not in self._sdf:
            self._sdf[tf] = self.orc.sdf_build(self.vol, self.orc.parse_tf(tf))[0]
        return self._sdf[tf]

    def reference(self, tf, eye, mode, n_seeds):
        key = (tf, tuple(eye), mode, n_seeds)
        if key not in self._ref:
            orc = self.orc
            pos, d = look_at_centre(self.vol, eye)
            o = orc.Scene(self.vol, self.sdf(tf), self.env, orc.parse_tf(tf), BALL_FRAME,
                          mode=orc.MODE_VOXEL_CACHE if mode == "voxel" else orc.MODE_IMAGE_SPACE)
            for s in scene.glibc_rand(n_seeds):
                o.render(pos, d, s)
            o.resolve(pos, d)
            for arr in (o.hit_index, o.frame, o.accum, o.cache):
                if arr is not None:
                    arr.setflags(write=False)
            self._ref[key] = o
        return self._ref[key]


@pytest.fixture(scope="module")
def ball(orc):
    return _Ball(orc)


def _render_ball(ctx, ball, tf, eye, mode, seeds, fused):
    """(accumulation buffer as stored, voxel cache, frame) after the passes of `seeds`: one launch, or one launch per seed"""
    pos, d = look_at_centre(ball.vol, eye)
    gmode = ffi.ACCUM_VOXEL_CACHE if mode == "voxel" else ffi.ACCUM_IMAGE_SPACE
    g = GpuScene(ctx, ball.vol, ball.sdf(tf), ball.env, tf, BALL_FRAME)
    if fused:
        g.render(pos, d, None, mode=gmode, seeds=seeds, debug=False)
    else:
        for s in seeds:
            g.render(pos, d, s, mode=gmode, debug=False)
    out = dict(accum=g.accum[0].pull(np.float32).copy(), accum_rows=g.accum_row_major(0), cache=g.cache.pull().copy(), frame=g.frame.pull().copy())
    g.release()
    return out


def _check_ball(out, o, mode):
    if mode == "voxel":
        assert o.cache.reshape(-1, 4)[:, 3].max() < 256, "test must stay below the token cap"
        assert np.array_equal(out["cache"], o.cache), "voxel cache"
    else:
        hit = o.hit_index.reshape(BALL_FRAME[1], BALL_FRAME[0]) >= 0
        assert np.array_equal(out["accum_rows"][hit], o.accum[hit]), "image-space accumulation"
        assert not out["accum_rows"][~hit].any()
    assert np.array_equal(out["frame"], o.frame), "resolved frame"


NEAR_EYE = (-40.0, 200.0, -60.0)
FAR_EYE = (-880.0, 1040.0, -1040.0)  # eight times as far from the volume's centre: the ball covers a few dozen pixels


@pytest.fixture(scope="module")
def ball_one_by_one(gpu_ctx, ball):
    """the eight passes of case 1 as eight short launches of the plain context, per mode"""
    cache = {}

    def get(mode):
        if mode not in cache:
            cache[mode] = _render_ball(gpu_ctx, ball, scene.tf_default_source(), NEAR_EYE, mode, scene.glibc_rand(8), fused=False)
        return cache[mode]

    return get


@pytest.mark.parametrize("mode", ["image", "voxel"])
def test_ball_eight_seeds_fused_on_two_blocks(ctx_two_blocks, ball, ball_one_by_one, mode):
    """more than 2000 hits x 8 seeds on 512 lanes: some forty items per lane, nearly all fetched by a mid-launch refill"""
    tf = scene.tf_default_source()
    o = ball.reference(tf, NEAR_EYE, mode, 8)
    assert int((o.hit_index >= 0).sum()) > 2000
    out = _render_ball(ctx_two_blocks, ball, tf, NEAR_EYE, mode, scene.glibc_rand(8), fused=True)
    _check_ball(out, o, mode)
    single = ball_one_by_one(mode)
    for what in ("accum", "cache", "frame"):
        assert np.array_equal(out[what], single[what]), what + ": fused on two blocks against one seed per launch"


def test_fewer_hits_than_lanes(ctx_two_blocks, ball):
    """39 hits x 64 seeds: one chunk of hits with 25 padding items in each of its 64 units (skipped by the refill: `everything
    fetched was padding` fetches again), seven of the eight queues empty, waves that find nothing at their first refill"""
    tf = scene.tf_default_source()
    o = ball.reference(tf, FAR_EYE, "image", 64)
    n_hits = int((o.hit_index >= 0).sum())
    assert n_hits == 39 and 1 <= n_hits <= 63
    out = _render_ball(ctx_two_blocks, ball, tf, FAR_EYE, "image", scene.glibc_rand(64), fused=True)
    hit = o.hit_index.reshape(BALL_FRAME[1], BALL_FRAME[0]) >= 0
    assert np.array_equal(out["accum_rows"][hit][:, 3], np.full(n_hits, 64.0, np.float32)), "every (hit, seed) item exactly once"
    _check_ball(out, o, "image")


@pytest.fixture(scope="module")
def token_reference(orc):
    """test_token_cap_regime_against_the_oracle's scene: 40 passes over 256 x 256 pixels that hit a 32^3 phantom"""
    vol, sdf, env, tf = small_scene(orc, 32)
    pos, d = look_at_centre(vol, [-12, 25, -12])
    o = orc.Scene(vol, sdf, env, orc.parse_tf(tf), (256, 256))
    for s in scene.glibc_rand(40):
        o.render(pos, d, s)
    o.cache.setflags(write=False)
    return (vol, sdf, env, tf, pos, d), o.cache.reshape(-1, 4)


def test_tokens_run_out_at_the_refill(ctx_two_blocks, token_reference):
    """one seed per launch in voxel-cache mode takes a token per sample when the item is fetched (utility.cl:20-31).  Past 256
    samples of a voxel the refill refuses: the lane stays idle across the refill point, and a fetch that grants nothing fetches
    again.  Counts are min(requests, 256) in any order; voxels below the cap equal the oracle's entry for entry."""
    (vol, sdf, env, tf, pos, d), want = token_reference
    g = GpuScene(ctx_two_blocks, vol, sdf, env, tf, (256, 256))
    for s in scene.glibc_rand(40):
        g.render(pos, d, s, debug=False)
    got = g.cache.pull().reshape(-1, 4)
    g.release()
    assert want[:, 3].max() == 256 and (want[:, 3] == 256).sum() > 100 and ((want[:, 3] > 0) & (want[:, 3] < 256)).sum() > 100
    assert np.array_equal(got[:, 3], want[:, 3])
    below = want[:, 3] < 256
    assert np.array_equal(got[below], want[below])
    assert got[~below, :3].max() <= 256 * 255


def test_gradient_instance_fused_on_two_blocks(ctx_two_blocks, ball):
    """case 1 in image mode through k_bounce<true, ...>: the table's `gradient` clauses classify every step literally"""
    tf = scene.tf_gradient_source()
    o = ball.reference(tf, NEAR_EYE, "image", 8)
    assert int((o.hit_index >= 0).sum()) > 2000
    _check_ball(_render_ball(ctx_two_blocks, ball, tf, NEAR_EYE, "image", scene.glibc_rand(8), fused=True), o, "image")


@pytest.fixture(scope="module")
def phantom128(orc):
    return small_scene(orc, 128)


def test_phantom_128_on_two_blocks(ctx_two_blocks, orc, phantom128):
    """secondary hits and fix-up records in numbers; 256 x 144 pixels, eight passes, about seventy items per lane and launch"""
    vol, sdf, env, tf = phantom128
    pos, d = scene.default_camera(128)
    st = _compare_passes(orc, ctx_two_blocks, vol, sdf, env, tf, (256, 144), pos, d, scene.glibc_rand(8))
    assert st["hits"] > 5000
