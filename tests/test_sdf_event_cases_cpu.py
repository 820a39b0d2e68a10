"""No GPU: the inputs of tests/test_gpu_sdf_events.py (tests/sdf_event_cases.py) decide events by what they are here for, so that an
input that stops exercising a path fails here.  The oracle's event set is checked against a second restatement in numpy first; the
figures in the comments were measured with the oracle, the assertions are floors below them."""
import re

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi
from oracle import orc_volume
from tests import sdf_event_cases as ec


def _ids(cases):
    return [ec.case_id(c) for c in cases]


@pytest.mark.parametrize("case", ec.CASES + [ec.RENDER_CASE], ids=_ids(ec.CASES + [ec.RENDER_CASE]))
def test_the_oracles_events_equal_the_numpy_restatement(orc, case):
    kind, dims, seed, table = case
    vol = ec.volume(kind, dims, seed)
    assert vol.shape == dims[::-1] and vol.dtype == np.int16
    want, _ = ec.oracle_sdf(orc, *case)
    length = orc_volume.gradient_length_int(vol)
    assert np.array_equal(length, ec.length_int(*ec.differences(vol, "zero")))   # (the two ways this file takes differences)
    events = ec.events_of(vol, table, length)
    assert np.array_equal(want < 0, events)
    assert 100 <= int(events.sum()) <= events.size - 100 and not (want == 0).any()


def test_tables_and_their_free_form_twins(orc):
    for name, source in ec.TABLES.items():
        twin = ec.FREE_FORM[name]
        rule = ffi.parse_tf(source).as_tuples()
        assert rule == orc.parse_tf(source).as_tuples() and len(rule) == 1 and rule[0][4] == 1   # one rule, and it reads `gradient`
        with pytest.raises(ffi.ClwhError):   # outside the product's grammar: the compiled classifier takes it
            ffi.parse_tf(twin)
        comparisons = lambda text: re.findall(r"(value|gradient) (>=|<=|>|<) ([-+.\w]+)", text[text.index("{"):])  # noqa: E731
        assert comparisons(twin) == comparisons(source) and len(comparisons(twin)) == 4 and "||" not in twin
        colour = lambda text: re.search(r"= \{(\d+),(\d+),(\d+),(\d+)\};", text).groups()  # noqa: E731
        assert colour(twin) == colour(source) == tuple(str(c) for c in rule[0][7])
    assert ec.window_and_bounds("gradient") == ((500, 1200), (101, 3999))
    assert ec.window_and_bounds("wrap") == ((600, 1200), (101, 39999))
    g = orc.parse_tf(ec.TF_WRAP).as_tuples()[0]
    assert (g[2], g[3]) == (101, 32767)   # `gradient < 40000` holds for every short


def test_shapes_reach_each_event_kernel_and_several_regions():
    assert all(d[0] % 8 != 0 for d in ec.PER_VOXEL_SHAPES + [ec.PER_VOXEL_REGIONS_SHAPE])   # k_sdfbit_events
    assert all(d[0] % 8 == 0 for d in ec.EIGHT_VOXEL_SHAPES + [ec.WIDE_ROW_SHAPE])          # k_sdfbit_events8
    assert {d[0] % 8 == 0 for d in ec.EXTREME_SHAPES} == {True, False}                      # the wrap in both
    regions = lambda d: ((d[0] + 63) // 64, (d[1] + 47) // 48, (d[2] + 15) // 16)  # noqa: E731  (8-wave blocks: cores of 64 x 48 x 16)
    assert regions(ec.PER_VOXEL_REGIONS_SHAPE) == (3, 3, 3) and regions((136, 100, 40)) == (3, 3, 3)
    assert ((ec.WIDE_ROW_SHAPE[0] + 63) // 64 * 2) % 16 == 0                                # rows of 16 words: the sixteen-row seed kernel
    assert all(n % 8 for case in ec.GENERIC_LAUNCH_CASES for n in case[1])                  # the global size, rounded up to 8, exceeds the volume


# events that flip when the differences take the nearest voxel instead of the border texel 0 (measured)
BORDER_FLIPS = {(70, 33, 45): 5557, (65, 49, 17): 3832, (130, 3, 7): 1488, (72, 40, 56): 4406, (512, 17, 6): 13068}


@pytest.mark.parametrize("case", ec.BLOB_CASES, ids=_ids(ec.BLOB_CASES))
def test_blobs_the_zero_border_and_the_gradient_clause_decide_events(orc, case):
    kind, dims, seed, table = case
    vol = ec.volume(kind, dims, seed)
    want, launches = ec.oracle_sdf(orc, *case)
    events = want < 0
    # the border texel: surfaces run into the faces, where a plateau (gradient 0 inside) is an event only because the texel outside is 0
    replicated = ec.events_of(vol, table, ec.length_int(*ec.differences(vol, "edge")))
    flips = int((replicated != events).sum())
    print("%s: %d events, %d flip under a replicated border (measured %s)" % (dims, int(events.sum()), flips, BORDER_FLIPS.get(dims)))
    assert flips >= 1000
    on_face = np.zeros(events.shape, bool)
    for axis in range(3):
        for side in (0, -1):
            on_face[tuple(side if k == axis else slice(None) for k in range(3))] = True
    assert not (replicated != events)[~on_face].any()   # (differences reach one voxel: the flips lie on the faces)
    # the gradient clause: plateaus at 1100 with gradient 0 are events under the default table only
    default, _ = ec.oracle_sdf(orc, kind, dims, seed, "default")
    differing = int((default != want).sum())
    print("%s: the field differs from the default table's in %d voxels (measured 2247 to 282484)" % (dims, differing))
    if dims == (2, 40, 40):
        assert differing == 0   # two voxels along x: every voxel has a zero texel next to it, no gradient is below 100
    else:
        assert differing > 1000
    # propagation: more than one launch of eight layers in the bit-parallel build
    reach = int(np.abs(want.astype(np.int32)).max())
    print("%s: max |sdf| %d, %d launches (measured 15 to 127; (130, 100, 40): 53 and 55)" % (dims, reach, launches))
    assert reach > 8 and launches > 8


# (in the window, no event because the short is negative; events because the short wrapped back; voxels a saturating conversion changes)
WRAP_COUNTS = {(37, 21, 13): (1561, 930, 1695), (24, 24, 24): (2053, 1222, 2239), (64, 8, 8): (664, 333, 734)}


@pytest.mark.parametrize("case", ec.EXTREME_CASES + [ec.RENDER_CASE], ids=_ids(ec.EXTREME_CASES + [ec.RENDER_CASE]))
def test_extremes_the_wrap_decides_events(orc, case):
    kind, dims, seed, table = case
    vol = ec.volume(kind, dims, seed)
    want, _ = ec.oracle_sdf(orc, *case)
    events = want < 0
    length = orc_volume.gradient_length_int(vol)
    (v_lo, v_hi), _ = ec.window_and_bounds(table)
    window = (vol >= v_lo) & (vol <= v_hi)
    negative = window & (length >= 32768) & (length < 65536)
    assert not events[negative].any()                     # ... although 100 < length < 40000 holds for some of them as ints
    wrapped_back = events & (length >= 65536)
    saturated = ec.events_of(vol, table, length, convert="saturate") != events
    kept_int = ec.events_of(vol, table, length, convert="int") != events
    counts = (int(negative.sum()), int(wrapped_back.sum()), int(saturated.sum()))
    print("%s: %s, %d differ when the int is compared (measured %s)" % (dims, counts, int(kept_int.sum()), WRAP_COUNTS.get(dims)))
    assert min(counts) >= 300 and int(kept_int.sum()) >= 300
    # every one of these lengths has a square above 2^24: the products and their sums round in binary32
    assert int(length[negative | wrapped_back].min()) ** 2 > 1 << 24
    gx, gy, gz = (g.astype(np.int64) for g in ec.differences(vol, "zero"))
    exact = gx * gx + gy * gy + gz * gz
    rounded = ((gx.astype(np.float32) ** 2 + gy.astype(np.float32) ** 2) + gz.astype(np.float32) ** 2).astype(np.float64)
    assert int((rounded != exact)[negative | wrapped_back].sum()) >= 300
