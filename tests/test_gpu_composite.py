"""clwh_render_composite on the GPU against the numpy restatement of its contract (tests/composite_ref.py), bit for bit: the frame,
rgba, t_first and t_stop on every pixel of the region.  The brick-skipping walk must equal the dense walk (CLWH_COMP_DENSE) wherever
both run.  Every family counts what it exercised -- terminated pixels, pixels with 0 < A < alpha_stop, and pixels with kept samples
that stay at A == 0 -- so that no comparison is empty."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import composite_ref as cr
from tests import projection_ref as pr
from tests.view_helpers import ROOT, F, toward, image_of, pose as _pose, host_lib, Comp, Proj

pytestmark = pytest.mark.gpu

INVALID_VALUE, BAD_NDRANGE, SIZE_MISMATCH = 1, 8, 9
LUT_FIRST = -1024


class Tally:
    """what a family's comparisons exercised"""

    def __init__(self):
        self.terminated = self.partial = self.transparent_with_samples = self.comparisons = 0

    def add(self, want, alpha_stop):
        _, rgba, _, t_stop, stats = want
        A = rgba[..., 3]
        self.terminated += int((~np.isnan(t_stop)).sum())
        self.partial += int(((A > 0) & (A < F(alpha_stop))).sum())
        self.transparent_with_samples += int(((A == 0) & (stats["n"] > 0)).sum())
        self.comparisons += 1

    def merge(self, other):
        for k in vars(self):
            setattr(self, k, getattr(self, k) + getattr(other, k))

    def assert_all_three(self):
        assert self.terminated > 0 and self.partial > 0 and self.transparent_with_samples > 0, vars(self)


def _compare(ctx, vol, pos, d, frame_wh, region_wh, table, lut_first=LUT_FIRST, tally=None, flag_sets=(0, cr.SHADE), step=0.5,
             alpha_stop=0.95, ambient=0.3, t_near=0.0, t_far=np.inf):
    """reference == skipping walk == dense walk, for every set of flags"""
    volume, owner = image_of(ctx, vol)
    lut = ctx.buffer_from(np.ascontiguousarray(table, F))
    c = Comp(ctx, frame_wh, region_wh)
    kw = dict(step=step, alpha_stop=alpha_stop, ambient=ambient, t_near=t_near, t_far=t_far)
    for flags in flag_sets:
        want = cr.composite(vol, pos, d, frame_wh, region_wh, table, lut_first, flags=flags, **kw)
        Comp.check(c.run(volume, pos, d, lut, lut_first, flags=flags, **kw), want, "skipping, flags %d" % flags)
        Comp.check(c.run(volume, pos, d, lut, lut_first, flags=flags | cr.DENSE, **kw), want, "dense, flags %d" % flags)
        if tally is not None:
            tally.add(want, alpha_stop)
    c.release()
    lut.release()
    volume.release()
    if owner is not None:
        owner.release()


@pytest.mark.parametrize("pose", ["default", "close", "inside"])
def test_phantoms_from_several_poses(gpu_ctx, pose):
    tally = Tally()
    for dims in [(64, 64, 64), (70, 33, 45), (130, 20, 9), (5, 4, 3), (1, 1, 1)]:
        vol = scene.phantom(max(dims), dims=dims)
        pos, d = _pose(pose, dims)
        for table in (cr.soft_table(), cr.hard_table()):
            _compare(gpu_ctx, vol, pos, d, (104, 72), (96, 64), table, tally=tally)
    tally.assert_all_three()


@pytest.mark.parametrize("step", [0.37, 0.5, 1.0, 3.0])
def test_steps_and_slabs(gpu_ctx, step):
    vol = scene.phantom(64)
    pos, d = scene.default_camera(64)
    tally = Tally()
    for table in (cr.soft_table(), cr.hard_table()):
        _compare(gpu_ctx, vol, pos, d, (96, 64), (96, 64), table, tally=tally, step=step)
        _compare(gpu_ctx, vol, pos, d, (96, 64), (96, 64), table, tally=tally, step=step, t_near=40.0, t_far=70.0)
        _compare(gpu_ctx, vol, pos, d, (96, 64), (96, 64), table, tally=tally, step=step, t_near=-5.0, t_far=41.0)
    tally.assert_all_three()


def test_axis_parallel_and_grazing_rays(gpu_ctx):
    X, Y, Z = 40, 24, 32
    vol = scene.phantom(40, dims=(X, Y, Z))
    cases = {
        "axis": (np.array([20.0, 12.0, -6.0], F), np.array([0, 0, 1], F)),
        "face_y0": (np.array([20.0, 0.0, -6.0], F), np.array([0, 0, 1], F)),          # central row runs in the face y = 0
        "edge_x0y0": (np.array([0.0, 0.0, -6.0], F), np.array([0, 0, 1], F)),        # central ray runs along an edge
        "face_xdim": (np.array([40.0, 12.0, -6.0], F), np.array([0, 0, 1], F)),      # x == X is outside
        "diagonal": (np.array([-8.0, -8.0, -8.0], F), toward((-8, -8, -8), (40, 24, 32))),
        "straight_up": (np.array([20.0, -5.0, 16.0], F), np.array([0, 1, 0], F)),    # degenerate basis: NaN rays, nothing kept
    }
    tally = Tally()
    for name, (pos, d) in cases.items():
        mine = Tally()
        for table in (cr.soft_table(), cr.hard_table()):
            _compare(gpu_ctx, vol, pos, d, (64, 48), (64, 48), table, tally=mine)
        tally.merge(mine)
        contributed = mine.terminated + mine.partial
        assert (contributed == 0) == (name == "straight_up"), name
    tally.assert_all_three()


def _tables():
    rng = np.random.default_rng(11)
    step_fn = cr.soft_table()
    step_fn[:, 3] = np.where(np.arange(4096) + LUT_FIRST >= 800, F(0.3), F(0.0))
    one_opaque = np.zeros((4096, 4), F)
    one_opaque[900 - LUT_FIRST] = (0.2, 0.9, 0.4, 1.0)
    one_faint = np.zeros((4096, 4), F)
    one_faint[40 - LUT_FIRST] = (0.5, 0.5, 1.0, 0.01)
    all_transparent = np.zeros((4096, 4), F)
    all_transparent[:, :3] = 1
    all_opaque = np.ones((4096, 4), F)
    random_bits = rng.integers(0, 1 << 32, size=(4096, 4), dtype=np.uint64).astype(np.uint32).view(F)
    random_bits[:1024, 3] = 0  # transparent below value 0: air bricks to skip
    return {
        "soft": (cr.soft_table(), LUT_FIRST), "hard": (cr.hard_table(), LUT_FIRST), "step": (step_fn, LUT_FIRST),
        "one_opaque": (one_opaque, LUT_FIRST), "one_faint": (one_faint, LUT_FIRST),
        "all_transparent": (all_transparent, LUT_FIRST), "all_opaque": (all_opaque, LUT_FIRST),
        "len_1": (np.array([[0.3, 0.6, 0.9, 0.02]], F), 0),
        "first_far_above": (cr.hard_table(lut_len=64), 65535),    # every value clamps to entry 0 (alpha 0)
        "first_far_below": (cr.hard_table(lut_first=-65536, lut_len=64), -65536),  # every value clamps to the last entry (alpha 0)
        "first_far_below_opaque": (cr.ramp_table(-65536, -65500, 0.04, lut_first=-65536, lut_len=64), -65536),  # ... alpha 0.04
        "first_far_above_faint": (np.tile(np.array([[0.9, 0.1, 0.1, 0.03]], F), (64, 1)), 65535),  # ... entry 0, alpha 0.03
        "random_bits": (random_bits, LUT_FIRST),
    }


@pytest.mark.parametrize("alpha_stop", [0.5, 0.95, 1.0, np.inf])
def test_tables_and_alpha_stops(gpu_ctx, alpha_stop):
    vol = scene.phantom(64)
    tally = Tally()
    seen_nan = 0
    for name, (table, lut_first) in _tables().items():
        for pos, d in (scene.default_camera(64), scene.close_camera(64)):
            mine = Tally()
            _compare(gpu_ctx, vol, pos, d, (96, 64), (96, 64), table, lut_first, tally=mine, alpha_stop=alpha_stop)
            if name in ("all_transparent", "first_far_above", "first_far_below"):
                assert mine.terminated == mine.partial == 0 and mine.transparent_with_samples > 0
            if name == "all_opaque" and np.isfinite(alpha_stop):
                assert mine.terminated > 0 and mine.partial == mine.transparent_with_samples == 0
            if name == "random_bits":
                seen_nan += int(np.isnan(cr.composite(vol, pos, d, (96, 64), (96, 64), table, lut_first, alpha_stop=alpha_stop)[1]).sum())
            else:  # (A can reach +inf through that table, and +inf >= +inf ends the ray)
                tally.merge(mine)
    assert seen_nan > 0  # the random table drives NaNs through the accumulation
    if np.isfinite(alpha_stop):
        tally.assert_all_three()
    else:
        assert tally.terminated == 0 and tally.partial > 0 and tally.transparent_with_samples > 0


def _adversarial_volumes():
    rng = np.random.default_rng(7)
    X, Y, Z = 72, 40, 56
    noise = rng.integers(-50, 51, size=(Z, Y, X)).astype(np.int16)
    for (z, y, x) in [(0, 0, 0), (Z - 1, Y - 1, X - 1), (0, Y - 1, 8), (Z - 1, 0, X - 9)]:  # corners and faces: grazed bricks
        noise[z, y, x] = 32767
    noise[Z - 1, Y - 1, 0] = -32768
    noise[0, 0, X - 1] = -32768
    extremes = rng.choice(np.array([-32768, 32767, 0, -1], np.int16), size=(Z, Y, X)).astype(np.int16)
    sparse = np.full((Z, Y, X), -1000, np.int16)
    sparse[rng.integers(0, Z, 40), rng.integers(0, Y, 40), rng.integers(0, X, 40)] = rng.integers(-32768, 32768, 40).astype(np.int16)
    sparse[20:24, 16:22, 30:40] = 700  # something a ray can accumulate in
    # whole-range tables (lut_first -32768, 65536 entries)
    v = np.arange(65536) - 32768
    base = np.zeros((65536, 4), F)
    base[:, :3] = rng.random((65536, 3)).astype(F)
    t_noise, t_extremes, t_sparse = base.copy(), base.copy(), base.copy()
    t_noise[:, 3] = np.where(np.abs(v) >= 49, F(0.2), F(0.0))        # only the tails of the noise and the planted extremes
    t_extremes[:, 3] = np.where(v == -1, F(0.01), np.where(v == 32767, F(0.3), F(0.0)))
    t_sparse[:, 3] = np.where(v == -1000, F(0.0), F(0.35))           # everything but the background
    return {"noise": (noise, t_noise), "extremes": (extremes, t_extremes), "sparse": (sparse, t_sparse)}


@pytest.mark.parametrize("name", ["noise", "extremes", "sparse"])
def test_adversarial_volumes_skipping_equals_dense(gpu_ctx, name):
    vol, table = _adversarial_volumes()[name]
    Z, Y, X = vol.shape
    poses = [scene.default_camera(X), scene.close_camera(X),
             (np.array([-10.0, -3.0, -10.0], F), toward((-10, -3, -10), (X, 0, Z))),          # rays graze the far corner
             (np.array([X + 5.0, Y * 0.5, Z * 0.5], F), np.array([-1, 0, 0], F)),
             (np.array([X * 0.5, Y * 0.5, Z * 0.5], F), scene.camera_direction(4.0, 0.3))]
    tally = Tally()
    for pos, d in poses:
        _compare(gpu_ctx, vol, pos, d, (80, 64), (80, 64), table, -32768, tally=tally)
    tally.assert_all_three()


def test_derived_data_follows_tables_volumes_and_invalidation(gpu_ctx):
    ctx = gpu_ctx
    X, Y, Z = 24, 16, 40
    a = scene.phantom(40, dims=(X, Y, Z))
    b = (a[::-1] // 2 + 300).astype(np.int16)
    pos, d = _pose("default", (X, Y, Z))
    wh = (64, 48)
    soft, hard = cr.soft_table(), cr.hard_table()
    shell = np.zeros((4096, 4), F)  # opaque exactly where `soft` and `hard` are transparent: a stale prefix table skips the wrong bricks
    shell[:300 - LUT_FIRST] = (0.1, 0.2, 0.3, 0.02)
    volume = ctx.image_from(a)
    lut = ctx.buffer_from(hard)
    c = Comp(ctx, wh, wh)
    tally = Tally()

    def both(vol, table, what, through=None):
        for flags in (0, cr.SHADE):
            want = cr.composite(vol, pos, d, wh, wh, table, LUT_FIRST, flags=flags)
            Comp.check(c.run(through or volume, pos, d, lut, LUT_FIRST, flags=flags), want, what)
            tally.add(want, 0.95)

    both(a, hard, "first")
    lut.push(shell)  # a changed table: the prefix count is rebuilt at the next composite
    both(a, shell, "after table push")
    alias = ctx.wrap(lut.device_ptr, lut.nbytes, np.float32)
    alias.push(soft)  # rewritten through another object of the same pointer
    both(a, soft, "after a push through a wrap")
    volume.push(b)  # a changed volume: the bricked copy is rebuilt
    both(b, soft, "after volume push")
    lut.push(shell)
    ctx.invalidate_derived(scene=False, camera=False, projection=True)
    both(b, shell, "after invalidate")
    short = ctx.wrap(lut.device_ptr, 16 * 1500, np.float32)  # same pointer and content, shorter table: lut_len is part of the key
    want = cr.composite(b, pos, d, wh, wh, shell[:1500], LUT_FIRST)
    Comp.check(c.run(volume, pos, d, short, LUT_FIRST), want, "shorter table")
    lut.push(hard)
    both(b, hard, "after the last push")
    ctx.finish()
    for m in (alias, short, lut, volume):
        m.release()
    c.release()
    tally.assert_all_three()


def test_projections_and_composites_share_the_bricked_copy(gpu_ctx):

    ctx = gpu_ctx
    a = scene.phantom(48)
    b = (a[:, ::-1] // 2 + 200).astype(np.int16)
    pos, d = scene.default_camera(48)
    wh = (96, 64)
    volume = ctx.image_from(a)
    lut = ctx.buffer_from(cr.hard_table())
    c, p = Comp(ctx, wh, wh), Proj(ctx, wh, wh)
    tally = Tally()
    ctx.invalidate_derived(scene=False, camera=False, projection=True)
    for round_, vol in enumerate((a, b, a)):
        if round_:
            volume.push(vol)
        want_c = cr.composite(vol, pos, d, wh, wh, cr.hard_table(), LUT_FIRST)
        want_p = pr.project(vol, pos, d, wh, wh, modes=(pr.MAX, pr.MEAN), window_cw=(0.0, 1000.0))
        order = ("c", "p", "c") if round_ % 2 == 0 else ("p", "c", "p")  # whichever comes first builds the copy the other reads
        for what in order:
            if what == "c":
                Comp.check(c.run(volume, pos, d, lut, LUT_FIRST), want_c, "composite, round %d" % round_)
                tally.add(want_c, 0.95)
            else:
                for mode in (pr.MAX, pr.MEAN):
                    Proj.check(p.run(volume, pos, d, mode, window=(0.0, 1000.0)), want_p[mode], "projection, round %d" % round_)
    ctx.finish()
    c.release()
    p.release()
    lut.release()
    volume.release()
    tally.assert_all_three()


def test_no_interference_with_the_path_tracer(gpu_ctx, orc):
    """composites interleaved with multi-seed render passes on one context: the path tracer's frame and voxel cache equal those of a
    context that never composited"""
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
    table = cr.hard_table()
    tally = Tally()
    for ctx, composite in ((gpu_ctx, True), (other, False)):
        s = GpuScene(ctx, vol, sdf, env, tf, (128, 128))
        c = Comp(ctx, (128, 128), (128, 128)) if composite else None
        lut = ctx.buffer_from(table) if composite else None
        for i in range(4):
            if composite:
                c.run(s.volume, pos, d, lut, LUT_FIRST, flags=(0, cr.SHADE, cr.DENSE, cr.SHADE | cr.DENSE)[i])
            s.render(pos, d, 0, seeds=seeds[2 * i:2 * i + 2], debug=False)
            if composite:
                got = c.run(s.volume, pos, d, lut, LUT_FIRST, flags=cr.SHADE)
        ctx.finish()
        results.append((s.frame.pull(), s.cache.pull()))
        if composite:
            want = cr.composite(vol, pos, d, (128, 128), (128, 128), table, LUT_FIRST, flags=cr.SHADE)
            Comp.check(got, want)
            tally.add(want, 0.95)
            c.release()
            lut.release()
        s.release()
    other.destroy()
    assert np.array_equal(results[0][0], results[1][0])
    assert np.array_equal(results[0][1], results[1][1])
    tally.assert_all_three()


def test_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    vol = scene.phantom(16)
    volume = ctx.image_from(vol)
    frame = ctx.image([64, 32], 4, np.uint8, (32, 64, 4))
    lut = ctx.buffer_from(cr.hard_table())
    small = ctx.buffer(64 * 32 * 4 - 4, np.float32)
    small_rgba = ctx.buffer(64 * 32 * 16 - 4, np.float32)
    misaligned = ctx.wrap(lut.device_ptr + 4, 16 * 64, np.float32)
    pos, d = scene.default_camera(16)

    def status(**kw):
        args = dict(frame=frame, volume=volume, cam_pos=pos, cam_dir=d, width=64, height=32, lut=lut, lut_first=LUT_FIRST)
        args.update(kw)
        try:
            ctx.render_composite(**args)
            return 0
        except ffi.ClwhError as e:
            return e.status

    assert status() == 0 and status(flags=3) == 0 and status(alpha_stop=float("inf")) == 0
    assert status(flags=cr.SHADE, ambient=0.0) == 0 and status(flags=cr.SHADE, ambient=1.0) == 0
    assert status(ambient=7.0) == 0 and status(ambient=float("nan")) == 0  # read with CLWH_COMP_SHADE only
    zero = ffi.CompositeDesc()
    assert ffi.lib().clwh_render_composite(ctx.h, C.byref(zero)) == INVALID_VALUE
    zero.frame, zero.volume, zero.lut, zero.width, zero.height = frame.h, volume.h, lut.h, 64, 32
    zero.lut_len, zero.alpha_stop = 4096, 0.95  # everything but the step (and the camera, which a zero step hides)
    assert ffi.lib().clwh_render_composite(ctx.h, C.byref(zero)) == INVALID_VALUE
    assert status(lut=None, lut_len=4096) == INVALID_VALUE and status(volume=frame) == INVALID_VALUE and status(frame=volume) == INVALID_VALUE
    assert status(frame=lut) == INVALID_VALUE and status(volume=lut) == INVALID_VALUE and status(lut=misaligned, lut_len=64) == INVALID_VALUE
    assert status(flags=4) == INVALID_VALUE and status(flags=-1) == INVALID_VALUE and status(flags=1 << 16) == INVALID_VALUE
    assert status(lut_len=0) == INVALID_VALUE and status(lut_len=-1) == INVALID_VALUE and status(lut_len=65537) == INVALID_VALUE
    assert status(lut_first=-65537) == INVALID_VALUE and status(lut_first=65536) == INVALID_VALUE
    assert status(lut_first=-65536) == 0 and status(lut_first=65535) == 0
    assert status(alpha_stop=0.0) == INVALID_VALUE and status(alpha_stop=-1.0) == INVALID_VALUE and status(alpha_stop=float("nan")) == INVALID_VALUE
    for amb in (-0.01, 1.01, float("nan"), float("inf")):
        assert status(flags=cr.SHADE, ambient=amb) == INVALID_VALUE
    assert status(step=0.0) == INVALID_VALUE and status(step=-1.0) == INVALID_VALUE and status(step=float("nan")) == INVALID_VALUE
    assert status(step=float("inf")) == INVALID_VALUE
    assert status(step=1e-9) == INVALID_VALUE  # the farthest corner lies more than 2^29 steps away
    assert status(cam_pos=(float("nan"), 0.0, 0.0)) == INVALID_VALUE and status(cam_pos=(float("inf"), 0.0, 0.0)) == INVALID_VALUE
    assert status(t_near=5.0, t_far=4.0) == INVALID_VALUE and status(t_near=float("nan")) == INVALID_VALUE
    assert status(t_near=float("inf")) == INVALID_VALUE
    assert status(width=0) == BAD_NDRANGE and status(width=60) == BAD_NDRANGE and status(height=12) == BAD_NDRANGE
    assert status(width=72) == BAD_NDRANGE and status(height=40) == BAD_NDRANGE
    assert status(lut_len=4097) == SIZE_MISMATCH and status(lut_len=65536) == SIZE_MISMATCH
    assert status(rgba=small_rgba) == SIZE_MISMATCH and status(t_first=small) == SIZE_MISMATCH and status(t_stop=small) == SIZE_MISMATCH
    assert status(rgba=small_rgba, width=56) == 0 and status(t_first=small, t_stop=small, height=24) == 0
    ctx.finish()
    for m in (misaligned, small_rgba, small, lut, frame, volume):
        m.release()


@pytest.mark.parametrize("flags", [0, cr.SHADE])
def test_full_size_512(gpu_ctx, flags):
    ctx = gpu_ctx
    n, W, H = 512, 1920, 1080 // 8 * 8
    vol = scene.phantom(n)
    pos, d = scene.default_camera(n)
    volume = ctx.image_from(vol)
    table = cr.hard_table()
    lut = ctx.buffer_from(table)
    c = Comp(ctx, (1920, 1080), (W, H))
    rows = np.arange(0, H, 16)
    want = cr.composite(vol, pos, d, (1920, 1080), (W, H), table, LUT_FIRST, flags=flags, rows=rows)
    got = c.run(volume, pos, d, lut, LUT_FIRST, flags=flags)
    Comp.check(tuple(g[rows] for g in got), want, "skipping")
    Comp.check(c.run(volume, pos, d, lut, LUT_FIRST, flags=flags | cr.DENSE), got, "dense")
    tally = Tally()
    tally.add(want, 0.95)
    tally.assert_all_three()
    assert tally.terminated > 10000
    c.release()
    lut.release()
    volume.release()


def _host_lib():
    return host_lib(clvr_host_render_composite=(C.c_void_p, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p,
                                                             C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float]))


def test_host_mirror_composite_equals_the_ffi_frame(gpu_ctx):
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
        c = Comp(gpu_ctx, (2048, 1024), (W, H))
        # the second and third calls change the table's contents, the fourth repeats the third's
        for table, step, stop, flags in ((cr.hard_table(), 0.5, 0.95, 0), (cr.soft_table(), 0.37, 0.5, cr.SHADE),
                                         (cr.hard_table(), 1.0, 0.95, cr.SHADE | cr.DENSE), (cr.hard_table(), 0.5, 0.95, 0)):
            ptr = L.clvr_host_render_composite(h, pos, look, W, H, table.ctypes.data, LUT_FIRST, 4096, step, stop, flags, 0.3)
            host = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(1024, 2048, 4))[:H, :W].copy()
            lut = gpu_ctx.buffer_from(table)
            got = c.run(volume, np.array(list(pos), F), scene.camera_direction(0.9, 6.183), lut, LUT_FIRST, step=step, alpha_stop=stop,
                        flags=flags, ambient=0.3)
            lut.release()
            assert np.array_equal(host, got[0])
            assert (host[..., 3] > 0).sum() > 1000 and (~np.isnan(got[3])).sum() > 0
        c.release()
        volume.release()
    finally:
        L.clvr_host_destroy(h)


@pytest.mark.parametrize("option,flags,name", [("--composite", 0, "plain"), ("--composite=shaded", cr.SHADE, "shaded")])
def test_headless_composite_writes_the_composite(tmp_path, option, flags, name):
    n, W, H = 96, 2048, 1024
    vol = scene.phantom(n)
    scene.write_nrrd(str(tmp_path / "v.nrrd"), vol)
    rng = np.random.default_rng(5)
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(rng.random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    out = subprocess.run([exe, option, str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", str(W), str(H), str(tmp_path / "p.ppm")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["composite"] == name and line["frames"] == 1 and "projection" not in line
    raw = open(tmp_path / "p.ppm", "rb").read()
    header = b"P6\n%d %d\n255\n" % (W, H)
    assert raw.startswith(header)
    ppm = np.frombuffer(raw[len(header):], np.uint8).reshape(H, W, 3)[::-1]  # the PPM's first row is the frame's last
    pos, d = scene.default_camera(n)
    rows = np.arange(0, H, 8)
    table = cr.tf_composite_lut([(500.0, 1200.0, (1.0, 1.0, 1.0, 1.0))], LUT_FIRST, 4096, 0.05)
    want = cr.composite(vol, pos, d, (2048, 1024), (W, H), table, LUT_FIRST, step=0.5, alpha_stop=0.95, flags=flags, ambient=0.3, rows=rows)
    assert np.array_equal(ppm[rows], want[0][..., :3])
    assert (want[0][..., 3] > 0).sum() > 1000
    both = subprocess.run([exe, option, "--projection=max", str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", str(W), str(H)],
                          capture_output=True, text=True, timeout=120)
    assert both.returncode == 1  # the two views exclude each other
