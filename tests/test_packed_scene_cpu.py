"""No GPU: the numpy restatements of the derived scene data (tests/packed_scene_ref.py) against plain per-voxel Python loops on small
volumes, and the non-vacuity conditions of every input of the GPU read-back tests (tests/packed_scene_cases.py), so that an input that
stops exercising a path fails here."""
import math
import struct

import numpy as np
import pytest

from cl_volume_renderer_amd import scene
from tests import isosurface_ref as ir
from tests import packed_scene_cases as pc
from tests import packed_scene_ref as ps


# ---- brick order

def test_slot_index_is_a_bijection_on_a_brick_and_the_documented_formula():
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    slots = ps.slot_index(x, y, z, 1, 1)
    assert sorted(slots.reshape(-1).tolist()) == list(range(512))
    # packed_volume.hpp: ((z & 4) << 6) | ((y & 4) << 5) | ((x & 4) << 4) | ((z & 3) << 4) | ((y & 3) << 2) | (x & 3), behind
    # brick ((z >> 3) * NBY + (y >> 3)) * NBX + (x >> 3), 512 slots each
    rng = np.random.default_rng(5)
    nbx, nby, nbz = 5, 3, 4
    for _ in range(2000):
        x, y, z = int(rng.integers(0, 8 * nbx)), int(rng.integers(0, 8 * nby)), int(rng.integers(0, 8 * nbz))
        inner = ((z & 4) << 6) | ((y & 4) << 5) | ((x & 4) << 4) | ((z & 3) << 4) | ((y & 3) << 2) | (x & 3)
        assert int(ps.slot_index(x, y, z, nbx, nby)) == ((((z >> 3) * nby + (y >> 3)) * nbx + (x >> 3)) << 9) + inner
    # a sub-brick is 64 consecutive slots: the voxels of one 4^3 box
    sub = ps.slot_index(np.arange(4)[None, None, :] + 4, np.arange(4)[None, :, None], np.arange(4)[:, None, None] + 4, 1, 1)
    assert sorted(sub.reshape(-1).tolist()) == list(range(5 * 64, 6 * 64))


@pytest.mark.parametrize("dims", [(9, 7, 5), (16, 8, 8), (1, 1, 1), (17, 3, 10)])
def test_scatter_and_gather(dims):
    X, Y, Z = dims
    a = np.arange(1, X * Y * Z + 1, dtype=np.int32).reshape(Z, Y, X)
    b = ps.scatter(a, -7)
    nbx, nby, nbz = ps.brick_counts(dims)
    assert b.shape == (nbx * nby * nbz, 512)
    assert np.array_equal(ps.gather(b, dims), a)
    assert np.array_equal(b != -7, ps.real_slots(dims)) and int(ps.real_slots(dims).sum()) == X * Y * Z
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                assert b.reshape(-1)[int(ps.slot_index(x, y, z, nbx, nby))] == a[z, y, x]


# ---- render side, voxel by voxel

def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _loop_scene(vol, sdf, rules):
    """class, maybe, step byte, record words and free value of every voxel in plain Python"""
    Z, Y, X = vol.shape

    def at(x, y, z):
        return int(vol[z, y, x]) if 0 <= x < X and 0 <= y < Y and 0 <= z < Z else 0

    out = {}
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                value = at(x, y, z)
                gx, gy, gz = at(x + 1, y, z) - at(x - 1, y, z), at(x, y + 1, z) - at(x, y - 1, z), at(x, y, z + 1) - at(x, y, z - 1)
                s = _f32(_f32(_f32(float(gx) * gx) + _f32(float(gy) * gy)) + _f32(float(gz) * gz))
                g = int(_f32(math.sqrt(s)))   # (sqrt of a binary32 in binary64, rounded once more: correctly rounded)
                g = ((g + 32768) & 0xFFFF) - 32768
                cls, maybe = 0, False
                for k, (v_lo, v_hi, g_lo, g_hi, use_g, _w, terminal, _c) in enumerate(rules):
                    in_window = v_lo <= value <= v_hi
                    maybe = maybe or in_window
                    if in_window and (not use_g or g_lo <= g <= g_hi):
                        cls = k + 1
                        break
                    if terminal:
                        break
                maybe = maybe or cls != 0
                sd = int(sdf[z, y, x])
                w0 = ((gx & 0x1FFFF) | ((gy & 0x1FFFF) << 17)) & 0xFFFFFFFF
                w1 = ((gy & 0x1FFFF) >> 15) | ((gz & 0x1FFFF) << 2) | (cls << 19)
                out[(x, y, z)] = (cls, maybe, (0x80 if cls else 0) | max(sd, 0), (w0, w1), 0 if (maybe or sd <= 0) else sd)
    return out


LOOP_TFS = dict(pc.RULE_TFS, all_class_2=pc.TF_ALL_CLASS_2,
                terminal_with_gradient="inline bool is_event_gen(short value, short gradient, int4 *color){ return (value >= -5 && gradient < 7.5f); }")


@pytest.mark.parametrize("tf", sorted(LOOP_TFS))
@pytest.mark.parametrize("kind", ["phantom", "random"])
def test_packed_scene_against_a_per_voxel_loop(orc, kind, tf):
    dims = (11, 7, 9)
    vol = pc.phantom(dims) if kind == "phantom" else pc.random_volume(dims)
    if kind == "phantom":
        vol[2:5, 1:4, 3:9] = 900   # a piece of the shell: events, and their faces
    sdf = pc.random_sdf(dims)
    rules = orc.parse_tf(LOOP_TFS[tf]).as_tuples()
    p = ps.PackedScene(vol, sdf, rules)
    want = _loop_scene(vol, sdf, rules)
    X, Y, Z = dims
    nbx, nby, nbz = p.nb
    stepb = np.zeros(p.stepb.shape, np.uint8).reshape(-1)
    grec = np.zeros(p.grec.shape, np.uint32).reshape(-1, 2)
    brick_min = np.full(nbx * nby * nbz, 255, np.uint32)
    written = np.zeros((nbx * nby * nbz, 8), bool)
    for (x, y, z), (cls, maybe, q, words, free) in want.items():
        assert p.cls[z, y, x] == cls and p.maybe[z, y, x] == maybe, (x, y, z)
        slot = int(ps.slot_index(x, y, z, nbx, nby))
        stepb[slot] = q
        grec[slot] = words
        brick_min[slot >> 9] = min(brick_min[slot >> 9], free)
        written[slot >> 9, (slot >> 6) & 7] |= maybe
    assert np.array_equal(p.stepb.reshape(-1), stepb)
    assert np.array_equal(p.grec.reshape(-1, 2), grec)
    assert np.array_equal(p.brick_min, brick_min) and brick_min.max() < 255   # every brick of the grid has a real voxel
    assert np.array_equal(p.written, written)
    assert np.array_equal(ps.unpack_class(p.grec), ps.scatter(p.cls, 0))
    if kind == "random" and tf in ("gradient", "three_rects", "terminal_with_gradient"):
        assert (p.maybe & (p.cls == 0)).any()   # a value window entered, the gradient clause failed


def test_free_form_classes_are_the_scene_of_the_equivalent_rule(orc):
    dims = (11, 7, 9)
    vol = pc.free_form_volume(dims)
    sdf = pc.random_sdf(dims)
    cls = pc.free_form_classes(vol)
    assert (vol == 31000).any() and (cls[vol == 31000] == 1).all()
    p = ps.PackedScene(vol, sdf, classes=cls)
    assert np.array_equal(p.maybe, cls != 0)
    plain = np.where(vol == 31000, 0, vol).astype(np.int16)   # without the `||` the event set is one rectangle's
    rules = orc.parse_tf(scene.tf_rect_source([(-100.0, 300.0, 0.0, 4000.0, (0.9, 0.6, 0.3, 0.7))])).as_tuples()
    q = ps.PackedScene(plain, sdf, rules)
    same = vol == plain
    assert np.array_equal(p.cls[same], q.cls[same]) and np.array_equal(ps.PackedScene(plain, sdf, classes=pc.free_form_classes(plain)).stepb, q.stepb)


def test_gradient_short_wraps_and_fills_the_fields():
    g = ps.gradient_short(np.array([65535, 3, 0, -65535]), np.array([65535, 4, 0, 0]), np.array([65535, 0, 0, 0]))
    assert g.tolist() == [((113509 + 32768) & 0xFFFF) - 32768, 5, 0, -1]   # sqrt(3) * 65535 = 113509.9.. ; 65535 wraps to -1
    r = ps.pack_record(np.array([-65535, 65535]), np.array([65535, -65535]), np.array([-1, 1]), np.array([255, 0]))
    assert r.dtype == np.uint32
    for (w0, w1), (gx, gy, gz, c) in zip(r.tolist(), [(-65535, 65535, -1, 255), (65535, -65535, 1, 0)]):
        assert w0 & 0x1FFFF == gx & 0x1FFFF and ((w0 >> 17) | ((w1 & 3) << 15)) == gy & 0x1FFFF
        assert (w1 >> 2) & 0x1FFFF == gz & 0x1FFFF and w1 >> 19 == c


# ---- views side

def test_dilated_brick_bounds_equal_a_triple_loop():
    dims = (10, 9, 17)
    X, Y, Z = dims
    vol = pc.random_volume(dims)
    dmin, dmax = ir.dilated_brick_bounds(vol)
    nbx, nby, nbz = ps.brick_counts(dims)
    assert dmin.shape == (nbz, nby, nbx)
    for bz in range(nbz):
        for by in range(nby):
            for bx in range(nbx):
                seen = []
                for z in range(8 * bz - 1, 8 * bz + 9):
                    for y in range(8 * by - 1, 8 * by + 9):
                        for x in range(8 * bx - 1, 8 * bx + 9):
                            if 0 <= x < X and 0 <= y < Y and 0 <= z < Z:
                                seen.append(int(vol[z, y, x]))
                assert (dmin[bz, by, bx], dmax[bz, by, bx]) == (min(seen), max(seen))


@pytest.mark.parametrize("dims", [(10, 9, 17), (41, 8, 33)])
def test_view_data_against_loops(dims):
    X, Y, Z = dims
    vol = pc.random_volume(dims)
    v = ps.ViewData(vol)
    nbx, nby, nbz = v.nb
    bricks = np.zeros(nbx * nby * nbz * 512, np.int16)
    lo = np.full(nbx * nby * nbz, 1 << 20)
    hi = -lo
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                slot = int(ps.slot_index(x, y, z, nbx, nby))
                bricks[slot] = vol[z, y, x]
                lo[slot >> 9], hi[slot >> 9] = min(lo[slot >> 9], vol[z, y, x]), max(hi[slot >> 9], vol[z, y, x])
    assert np.array_equal(v.bricks.reshape(-1), bricks)
    assert v.table.tolist() == [(int(a) & 0xFFFF) | ((int(b) & 0xFFFF) << 16) for a, b in zip(lo, hi)]
    dmin, dmax = ir.dilated_brick_bounds(vol)
    assert v.dilated.tolist() == [(int(a) & 0xFFFF) | ((int(b) & 0xFFFF) << 16) for a, b in zip(dmin.reshape(-1), dmax.reshape(-1))]
    cnx, cny, cnz = (nbx + 3) // 4, (nby + 3) // 4, (nbz + 3) // 4
    assert v.coarse.shape == (cnx * cny * cnz,)
    for cz in range(cnz):
        for cy in range(cny):
            for cx in range(cnx):
                a = dmin[4 * cz:4 * cz + 4, 4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4].min()
                b = dmax[4 * cz:4 * cz + 4, 4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4].max()
                assert int(v.coarse[(cz * cny + cy) * cnx + cx]) == (int(a) & 0xFFFF) | ((int(b) & 0xFFFF) << 16)


# ---- the GPU tests' inputs exercise what they are for

# measured with scene.phantom and tf_gradient_source(): (voxels in a value window, class != 0, maybe with class 0, sub-bricks written, all)
GRADIENT_COUNTS = {(64, 64, 64): (18864, 8504, 10360, 760, 4096), (80, 9, 9): (786, 500, 286, 50, 320),
                   (72, 40, 56): (22456, 9440, 13016, 696, 2520)}


@pytest.mark.parametrize("dims", pc.GRADIENT_SHAPES)
def test_gradient_inputs_have_every_kind_of_voxel_and_sub_brick(orc, dims):
    vol = pc.phantom(dims)
    p = ps.PackedScene(vol, np.ones(vol.shape, np.int8), orc.parse_tf(scene.tf_gradient_source()).as_tuples())
    event, undecided, neither = p.cls != 0, p.maybe & (p.cls == 0), ~p.maybe
    assert min(int(event.sum()), int(undecided.sum()), int(neither.sum())) >= 100
    written, total = int(p.written.sum()), p.written.size
    assert written * 10 >= total and (total - written) * 10 >= total
    v = vol.astype(np.int32)
    assert (int(((v >= 500) & (v <= 1200)).sum()), int(event.sum()), int(undecided.sum()), written, total) == GRADIENT_COUNTS[dims]


def _written_without_an_event(p):
    return p.written & ~ps.scatter(p.cls != 0, False).reshape(-1, 8, ps.SUB_SLOTS).any(axis=2)


def test_maybe_decides_sub_bricks_that_class_alone_would_not(orc):
    """The phantom's shell is thinner than a sub-brick: every sub-brick with an undecided voxel holds an event too, so on the phantoms
    `maybe` computed as class != 0 would write the same sub-bricks.  The random volumes and the rebuild test's mixed volume are what
    tells the two apart."""
    rules = orc.parse_tf(scene.tf_gradient_source()).as_tuples()
    for dims in pc.GRADIENT_SHAPES:
        vol = pc.phantom(dims)
        assert not _written_without_an_event(ps.PackedScene(vol, np.ones(vol.shape, np.int8), rules)).any()
    for dims in pc.RANDOM_SHAPES:
        vol = pc.random_volume(dims)
        assert _written_without_an_event(ps.PackedScene(vol, np.ones(vol.shape, np.int8), rules)).sum() >= (40 if min(dims) >= 9 else 1)
    vol = pc.mixed_volume((64, 64, 64))
    p = ps.PackedScene(vol, np.ones(vol.shape, np.int8), rules)
    event, undecided, neither = p.cls != 0, p.maybe & (p.cls == 0), ~p.maybe
    assert min(int(event.sum()), int(undecided.sum()), int(neither.sum())) >= 100
    written, total = int(p.written.sum()), p.written.size
    assert written * 10 >= total and (total - written) * 10 >= total and _written_without_an_event(p).sum() >= 100
    assert p.brick_min.max() == 1   # minima that the zeros of a build with every voxel an event would hide


def test_shapes_reach_each_staging_path():
    def fast_blocks(X):   # k_repack's blocks along x that take the 16-byte path / that do not
        blocks = (X + 63) // 64
        fast = sum(1 for b in range(blocks) if X % 16 == 0 and 64 * b + 64 <= X)
        return fast, blocks - fast
    paths = {dims: fast_blocks(dims[0]) for dims in pc.REPACK_SHAPES}
    assert paths[(64, 8, 8)] == (1, 0) and paths[(128, 16, 16)] == (2, 0) and paths[(80, 9, 9)] == (1, 1)
    assert paths[(16, 8, 8)] == (0, 1) and paths[(72, 40, 56)] == (0, 2) and paths[(144, 24, 40)] == (2, 1)
    assert any(d[1] % 8 and d[2] % 8 for d in pc.REPACK_SHAPES)          # padding rows in y and z
    assert {d[0] % 8 == 0 for d in pc.VIEW_SHAPES} == {True, False}      # both paths of k_proj_repack
    nb = ps.brick_counts((40, 40, 136))
    assert nb == (5, 5, 17) and all(n % 4 == 1 for n in nb)              # a last cell one brick thick on every axis
    assert pc.LARGE_SHAPE[0] % 8 == 0 and pc.LARGE_SHAPE[0] % 16 != 0    # the views' 16-byte path, k_repack voxel by voxel


@pytest.mark.parametrize("dims", pc.RANDOM_SHAPES)
def test_random_volume_fills_the_fields_and_the_keys(dims):
    vol = pc.random_volume(dims)
    g = np.stack(ps.central_differences(vol))
    for axis in range(3):
        assert g[axis].max() == 65535 and g[axis].min() == -65535
    assert np.abs(g[:, 0, 0, 0]).max() == 32768   # against the border
    v = vol.astype(np.int32)
    assert (v + 32768).min() == 0 and (32767 - v).min() == 0 and (v + 32768).max() == 65535 and (32767 - v).max() == 65535
    t = ps.ViewData(vol)
    assert (t.table & 0xFFFF).max() >= 0x8000 and (t.table >> 16).min() < 0x8000   # negative minima, positive maxima in the pairs


def test_random_sdf_has_every_value():
    for dims in pc.RANDOM_SHAPES:
        sdf = pc.random_sdf(dims)
        assert len(np.unique(sdf)) == 256


def test_three_rects_first_match_wins_and_border_window(orc):
    rules = orc.parse_tf(pc.TF_THREE_RECTS).as_tuples()
    assert [r[4] for r in rules] == [1, 0, 0]                                # the gradient clause stands ahead
    assert rules[0][0] <= 0 <= rules[0][1] and rules[2][0] <= 0 <= rules[2][1]   # windows that contain the border value
    assert max(r[0] for r in rules) <= min(r[1] for r in rules)               # a value all three windows hold
    for dims in [(128, 16, 16), (72, 40, 56)]:
        for vol, least in ((pc.phantom(dims), 1000), (pc.random_volume(dims), 10)):   # (the windows are narrow for uniform values)
            p = ps.PackedScene(vol, np.ones(vol.shape, np.int8), rules)
            v = vol.astype(np.int32)
            assert all(int((p.cls == c).sum()) >= least for c in (0, 1, 2, 3))
            in_both = (v >= 30) & (v <= 950)
            assert (p.cls[in_both] == 1).any() and (p.cls[in_both] == 2).any() and not (p.cls[in_both] == 3).any()


def test_other_tables_have_events_and_the_rebuild_leaves_stale_sub_bricks(orc):
    vol = pc.phantom((64, 64, 64))
    ones = np.ones(vol.shape, np.int8)
    for name in ("default", "gt800"):
        p = ps.PackedScene(vol, ones, orc.parse_tf(pc.RULE_TFS[name]).as_tuples())
        assert (p.cls != 0).sum() >= 100 and np.array_equal(p.maybe, p.cls != 0)
    rules = orc.parse_tf(scene.TF_TEST_VALUE_GT_800).as_tuples()
    assert len(rules) == 1 and rules[0][6] == 1 and rules[0][5] == 0          # terminal, writes no colour
    vol = pc.mixed_volume((64, 64, 64))   # the rebuild test's
    first = ps.PackedScene(vol, ones, orc.parse_tf(pc.TF_ALL_CLASS_2).as_tuples())
    assert (first.cls == 2).all() and first.written.all() and not first.brick_min.any()
    second = ps.PackedScene(vol, ones, orc.parse_tf(scene.tf_gradient_source()).as_tuples())
    assert second.brick_min.max() == 1 and not second.written.all()           # minima the first build's zeros would hide
    free = ps.PackedScene(pc.free_form_volume((72, 40, 56)), np.ones((56, 40, 72), np.int8), classes=pc.free_form_classes(pc.free_form_volume((72, 40, 56))))
    assert (free.cls != 0).sum() >= 100 and not free.written.all() and (pc.free_form_volume((72, 40, 56)) == 31000).sum() >= 100
