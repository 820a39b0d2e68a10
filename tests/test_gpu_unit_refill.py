"""-m gpu: k_bounce's refill by whole units (csrc/render_kernels.hip, the UNITS instances: one atomicAdd(head, 64) per unit, the
unit decoded once on scalar operands, a refill that straddles two units).  Long launches of tables without `gradient` rules take
that form; `gradient` tables and short launches keep the dealing by refill.  CLWH_TUNE_UNIT_AHEAD=1 asks for the next unit a pass
ahead: off in every launch the library chooses itself (measured slower), so these tests are what runs it.

What can go wrong is a dropped item, a doubled item, a wrong seed for a unit, and a wave that never learns that a queue is dry (a
hang: every launch here sits under the suite's ordinary time limit).  Image-space accumulation adds integers, so S seeds fused
into one long launch must equal the same seeds one per launch on a plain context bit for bit, whichever wave traced an item, and
the count channel says how often every hit pixel was served.  (The single launches are short ones: the other form of the refill.)
The knobs are read when a context is created, so every case creates its own.  The scene is the ball of
test_fused_long_launch_equals_the_passes_one_by_one at 64^3: 651 hits = 11 chunks from the near camera (not a multiple of 64),
13 hits = one chunk from the far one (seven queues dry from the start), none looking away."""
import os

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests.gpu_util import GpuScene, look_at_centre

pytestmark = pytest.mark.gpu

FRAME = (160, 96)
SEED_COUNTS = (1, 2, 5, 64)
EYES = {"near": [-20, 85, -25], "far": [-200, 500, -250]}


def _ball_in_empty_space(n, radius, centre):
    """an object the rays leave for good (the scene of tests/test_gpu_long_launch.py)"""
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(np.float32)
    c = np.array(centre, np.float32)
    r = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    vol = np.where(r < radius, 900.0 - 6.0 * r, -900.0 + 3.0 * np.sin(0.3 * x) * np.cos(0.2 * y + 0.1 * z))
    return np.ascontiguousarray(vol.astype(np.int16))


def _context(env):
    """a context created under the given CLWH_TUNE_* settings (None: the default of that knob)"""
    env = {k: str(v) for k, v in env.items() if v is not None}
    os.environ.update(env)
    try:
        return ffi.Context(0)
    finally:
        for k in env:
            del os.environ[k]


def _camera(vol, name):
    if name == "away":
        pos, d = look_at_centre(vol, EYES["near"])
        return pos, (-d).astype(np.float32)
    return look_at_centre(vol, EYES[name])


def _accumulate(ctx, vol, sdf, env, tf, pos, d, seeds, fused, snapshots=()):
    """image-space accumulation of `seeds`: one launch (fused) or one launch per seed; the tile-major float4 buffer afterwards, or
    {n: the buffer after the first n seeds} for the counts in `snapshots`"""
    g = GpuScene(ctx, vol, sdf, env, tf, FRAME)
    ctx.buffer_reset(g.accum[0])
    out = {}
    if fused:
        g.render(pos, d, None, mode=ffi.ACCUM_IMAGE_SPACE, seeds=list(seeds), debug=False, write_frame=False)
    else:
        for n, s in enumerate(seeds, 1):
            g.render(pos, d, s, mode=ffi.ACCUM_IMAGE_SPACE, debug=False, write_frame=False)
            if n in snapshots:
                out[n] = g.accum[0].pull(np.float32).reshape(-1, 4).copy()
    if not snapshots:
        out = g.accum[0].pull(np.float32).reshape(-1, 4).copy()
    g.release()
    return out


@pytest.fixture(scope="module")
def ball(orc):
    vol = _ball_in_empty_space(64, 13.0, centre=[30, 35, 29])
    env = scene.env_map(128, 64)
    sdfs = {}
    for name, tf in (("default", scene.tf_default_source()), ("gradient", scene.tf_gradient_source())):
        sdfs[name] = (tf, orc.sdf_build(vol, orc.parse_tf(tf))[0])
    return vol, env, sdfs


@pytest.fixture(scope="module")
def one_per_launch(gpu_ctx, ball):
    """the reference, computed once and left alone: {(table, camera): {S: the accumulator after the first S seeds, one launch each,
    on the plain context}}"""
    vol, env, sdfs = ball
    seeds = scene.glibc_rand(64)
    ref = {}
    for table, cameras in (("default", ("near", "far", "away")), ("gradient", ("near",))):
        tf, sdf = sdfs[table]
        for cam in cameras:
            pos, d = _camera(vol, cam)
            n = 64 if (table, cam) == ("default", "near") else 5
            ref[(table, cam)] = _accumulate(gpu_ctx, vol, sdf, env, tf, pos, d, seeds[:n], False, snapshots=SEED_COUNTS)
    return ref


def _check_fused(ball, one_per_launch, table, cam, S, knobs):
    vol, env, sdfs = ball
    tf, sdf = sdfs[table]
    ref = one_per_launch[(table, cam)]
    pos, d = _camera(vol, cam)
    ctx = _context(dict(knobs, CLWH_TUNE_LONG_LAUNCH=1))
    try:
        got = _accumulate(ctx, vol, sdf, env, tf, pos, d, scene.glibc_rand(64)[:S], True)
    finally:
        ctx.destroy()
    hit = ref[1][:, 3] == 1.0  # the hit mask: the count channel after the first of the single launches
    assert np.array_equal(ref[1][:, 3] != 0.0, hit)
    assert np.array_equal(got[:, 3], np.where(hit, np.float32(S), np.float32(0)))  # every item once: none dropped, none doubled
    assert np.array_equal(got, ref[S])                                              # ... and with its own seed
    return int(hit.sum())


# S, CLWH_TUNE_BLOCKS, _QUEUES, _GROUP, _CHUNK_BLOCK_LOG2, _UNIT_AHEAD (None: the knob's default); every value of the issue's grid
# occurs, and GROUP=3 beside the default (which is 1) so that the grouped queue order is decoded as well.
# One or three blocks: 4 or 12 waves walk through up to 704 units -- promotions, tickets ahead, refills that straddle two units,
# stealing from every queue.  Default grid and S = 1: twelve waves for eleven units.  CHUNK_BLOCK_LOG2=0: no padding, all eight
# queues hold chunks; default (4): one block of 16 chunks, five of them padding, in queue 0 and seven queues without any.
GRID = [
    (1, None, 8, None, None, 1),
    (1, 1, 1, 1, 0, 0),
    (1, 3, 8, 3, 0, 1),
    (2, 3, 8, None, 0, 1),
    (2, None, 1, 1, None, 0),
    (5, 3, 1, 3, None, 1),
    (5, 1, 8, 1, None, 0),
    (5, None, 8, None, 0, 1),
    (64, 3, 8, None, None, 1),
    (64, 1, 1, 1, 0, 1),
    (64, None, 8, 3, 0, 0),
    (64, 3, 8, 1, 0, 0),
]


def _knobs(blocks, queues, group, block_log2, ahead):
    return {"CLWH_TUNE_BLOCKS": blocks, "CLWH_TUNE_QUEUES": queues, "CLWH_TUNE_GROUP": group,
            "CLWH_TUNE_CHUNK_BLOCK_LOG2": block_log2, "CLWH_TUNE_UNIT_AHEAD": ahead}


@pytest.mark.parametrize("S,blocks,queues,group,block_log2,ahead", GRID)
def test_fused_seeds_equal_the_seeds_one_per_launch(ball, one_per_launch, S, blocks, queues, group, block_log2, ahead):
    hits = _check_fused(ball, one_per_launch, "default", "near", S, _knobs(blocks, queues, group, block_log2, ahead))
    assert hits > 64 and hits % 64 != 0  # several chunks, the last one short


@pytest.mark.parametrize("S,blocks,block_log2,ahead", [(5, 3, None, 1), (2, None, 0, 0), (5, 1, 0, 1)])
def test_fewer_hits_than_one_chunk(ball, one_per_launch, S, blocks, block_log2, ahead):
    """one chunk: a unit per seed in one queue, the other seven dry from the start"""
    hits = _check_fused(ball, one_per_launch, "default", "far", S, _knobs(blocks, 8, None, block_log2, ahead))
    assert 0 < hits < 64


@pytest.mark.parametrize("ahead", [0, 1])
def test_no_hit_at_all(ball, one_per_launch, ahead):
    """the camera looks away from the volume: the launch returns and the accumulator stays zero"""
    hits = _check_fused(ball, one_per_launch, "default", "away", 5, _knobs(None, 8, None, None, ahead))
    assert hits == 0
    assert not one_per_launch[("default", "away")][5].any()


def test_gradient_table(ball, one_per_launch):
    """the USE_GRAD instances (they deal by refill in long launches too): five seeds on three blocks"""
    hits = _check_fused(ball, one_per_launch, "gradient", "near", 5, _knobs(3, 8, None, None, 1))
    assert hits > 64 and hits % 64 != 0


def test_planned_voxel_cache_launch_against_the_oracle(ball, orc):
    """five seeds fused in voxel-cache mode (the tokens dealt before the launch, grants[h] seeds per hit): below the cap of 256
    samples per voxel the whole cache -- counts and sums -- is the oracle's, whichever wave traced an item"""
    vol, env, sdfs = ball
    tf, sdf = sdfs["default"]
    pos, d = _camera(vol, "near")
    seeds = scene.glibc_rand(5)
    o = orc.Scene(vol, sdf, env, orc.parse_tf(tf), FRAME, mode=orc.MODE_VOXEL_CACHE)
    for s in seeds:
        o.render(pos, d, s)
    counts = o.cache.reshape(-1, 4)[:, 3]
    assert 0 < counts.max() < 256  # the precondition: no voxel reaches the cap, so no sample's fate depends on order
    ctx = _context(dict(_knobs(3, 8, None, None, 1), CLWH_TUNE_LONG_LAUNCH=1))
    try:
        g = GpuScene(ctx, vol, sdf, env, tf, FRAME)
        g.render(pos, d, None, mode=ffi.ACCUM_VOXEL_CACHE, seeds=seeds, debug=False, write_frame=False)
        cache = g.cache.pull()
        g.release()
    finally:
        ctx.destroy()
    assert np.array_equal(cache, o.cache)
