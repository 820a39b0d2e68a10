"""The thinning contract on the CPU: the reference's bit test against the classical definition of a simple voxel, the independence of
a sub-pass from any order, the invariants of every GPU case, the closed forms, the non-vacuity of the GPU cases, the skeleton's graph,
and the compiled kernels' resource usage.  No device is needed."""
import math
import os
import re

import numpy as np
import pytest

from cl_volume_renderer_amd import scene
from tests import thin_cases as tc
from tests import thin_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(keep_ends, anchored) for keep_ends in (False, True) for anchored in (False, True)]


# ---- 1. the bit test is the classical definition
def test_simple_equals_the_classical_definition():
    rng = np.random.default_rng(1)
    blocks = [rng.random((3, 3, 3)) < rng.choice([0.2, 0.5, 0.8]) for _ in range(3000)]
    blocks += [np.zeros((3, 3, 3), bool), np.ones((3, 3, 3), bool)]
    words, classical = [], []
    for block in blocks:
        block[1, 1, 1] = True
        without = block.copy()
        without[1, 1, 1] = False
        words.append(int(tr.neighbour_words(block)[1, 1, 1]))
        classical.append(tr.invariants(block) == tr.invariants(without))
    got = tr.simple(np.array(words, np.int64))
    assert np.array_equal(got, np.array(classical))
    assert got.tolist() == [tr.simple_word(w) for w in words]  # the array form is the scalar form
    assert 0.25 < got.mean() < 0.6  # both verdicts, in numbers
    assert not tr.simple(np.array([0], np.int64))[0]  # an isolated voxel is not simple


# ---- 2. a sub-pass does not depend on any order
@pytest.mark.parametrize("name", ["noise 65 x 17 x 17 at 0.5", "torus"])
def test_a_subpass_in_any_order_gives_the_parallel_result(name):
    mask, _ = tc.cases()[name]
    M, par, rng = mask.copy(), tr.parity(mask.shape), np.random.default_rng(2)
    C = tr.candidates(M)
    deleted = 0
    for s in range(8):
        together = M & ~tr.subpass(M, C, s, par)
        at = np.argwhere(C & M & (par == s))
        for _ in range(3):
            one_by_one = M.copy()
            for z, y, x in at[rng.permutation(len(at))]:
                if tr.simple_word(tr.word_at(one_by_one, z, y, x)):  # re-tested on the mask as it stands now
                    one_by_one[z, y, x] = False
            assert np.array_equal(one_by_one, together), (name, s)
        deleted += int((M & ~together).sum())
        M = together
    assert deleted > 0


# ---- 3. parts, cavities and the Euler number of every case survive every mode
@pytest.mark.parametrize("name", sorted(tc.cases()))
def test_invariants_of_every_case(name):
    mask, anchors = tc.cases()[name]
    want = tr.invariants(mask)
    for keep_ends, anchored in MODES:
        ref = tc.reference(name, keep_ends, anchored)
        for k in tc.MAX_ITERATIONS:
            thin, result = ref[k]
            assert tr.invariants(thin) == want, (name, keep_ends, anchored, k)
            assert (thin <= mask).all() and result["count_out"] == int(thin.sum()) == result["count_in"] - result["deleted"]
            assert not anchored or (thin & anchors).sum() == anchors.sum()
        assert (ref[0][0] <= ref[2][0]).all() and (ref[2][0] <= ref[1][0]).all()  # max_iterations 1 >= 2 >= final
        again, result = tr.thin(ref[0][0], tr.KEEP_ENDS if keep_ends else 0, anchors if anchored else None)
        assert np.array_equal(again, ref[0][0]) and result["iterations"] == 1 and result["deleted"] == 0  # a result is a fixpoint


# ---- 4. closed forms
def _ball(n, r):
    z, y, x = np.mgrid[:n, :n, :n]
    c = (n - 1) / 2
    return (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 <= r * r


def _segment_tube(shape, p0, p1, r):
    z, y, x = np.mgrid[:shape[0], :shape[1], :shape[2]]
    p0, p1 = np.array(p0, float), np.array(p1, float)
    d = p1 - p0
    P = np.stack([x, y, z], -1) - p0
    t = np.clip((P @ d) / (d @ d), 0, 1)
    return ((P - t[..., None] * d) ** 2).sum(-1) <= r * r


def test_ball_and_plate_thin_to_one_voxel():
    plate = np.zeros((8, 20, 22), bool)
    plate[3:6, 2:18, 3:19] = True
    for shape in (_ball(17, 7.0), plate):
        for flags in (0, tr.KEEP_ENDS):
            thin, result = tr.thin(shape, flags)
            assert int(thin.sum()) == 1 == result["count_out"], flags


def test_hollow_ball_keeps_its_cavity():
    hollow = _ball(19, 8.0) & ~_ball(19, 4.0)
    for flags in (0, tr.KEEP_ENDS):
        thin, _ = tr.thin(hollow, flags)
        assert tr.invariants(thin) == tr.invariants(hollow) == (1, 2, 2)
        assert (tr.count26(thin)[thin] >= 3).all()  # a closed shell: no end, no curve


def test_torus_thins_to_a_ring():
    torus, _ = tc.cases()["torus"]
    for flags in (0, tr.KEEP_ENDS):
        thin, _ = tr.thin(torus, flags)
        assert (tr.count26(thin)[thin] == 2).all() and 35 <= int(thin.sum()) <= 50
        assert tr.structure(thin) == {"ends": 0, "junction_voxels": 0, "isolated": 0, "loops": 1}


def test_bars_thin_to_six_ends():
    bars, _ = tc.cases()["bars"]
    thin, _ = tr.thin(bars, tr.KEEP_ENDS)
    assert tr.structure(thin)["ends"] == 6 and tr.structure(thin)["loops"] == 0
    assert int(tr.thin(bars, 0)[0].sum()) == 1  # without ends to keep nothing holds a bar


def test_anchored_tube_has_three_ends():
    shape = (36, 36, 36)
    tips = ((4, 4, 4), (30, 20, 31), (29, 31, 6))
    tube = np.zeros(shape, bool)
    for tip, r in zip(tips, (3.5, 3.0, 2.5)):
        tube |= _segment_tube(shape, (18, 18, 15), tip, r)
    anchors = np.zeros(shape, bool)
    for x, y, z in tips:
        assert tube[z, y, x]
        anchors[z, y, x] = True
    thin, _ = tr.thin(tube, 0, anchors)
    what = tr.structure(thin)
    assert what["ends"] == 3 and what["loops"] == 0 and (thin & anchors).sum() == 3
    assert (tr.count26(thin)[anchors] == 1).all()  # the ends are the anchors
    assert tr.invariants(thin) == tr.invariants(tube)


# ---- 5. the GPU cases are not vacuous
def test_gpu_cases_reach_the_tile_borders_with_both_verdicts():
    on_face = on_edge = on_corner = at_63 = at_64 = 0
    corner_verdicts = set()
    for name, (mask, anchors) in tc.cases().items():
        z, y, x = np.nonzero(tr.candidates(mask))
        lim = [(x % 64 == 0) | (x % 64 == 63), (y % 16 == 0) | (y % 16 == 15), (z % 16 == 0) | (z % 16 == 15)]
        # a border of the tile that is not a border of the volume: a neighbouring tile is read
        inner = [lim[0] & (x > 0) & (x < mask.shape[2] - 1), lim[1] & (y > 0) & (y < mask.shape[1] - 1), lim[2] & (z > 0) & (z < mask.shape[0] - 1)]
        n = inner[0].astype(int) + inner[1] + inner[2]
        on_face += int((n == 1).sum())
        on_edge += int((n == 2).sum())
        on_corner += int((n == 3).sum())
        at_63 += int(((x == 63) & (mask.shape[2] > 64)).sum())
        at_64 += int((x == 64).sum())
        if (n == 3).any():
            corner_verdicts |= set(tr.simple(tr.neighbour_words(mask)[z[n == 3], y[n == 3], x[n == 3]]).tolist())
        if mask.sum() > 1:
            assert max(tc.reference(name, k, a)[0][1]["deleted"] for k, a in MODES) > 0, name
    assert min(on_face, on_edge, at_63, at_64) >= 100 and on_corner >= 10
    assert corner_verdicts == {True, False}


# ---- 6. the graph
def test_skeleton_graph_of_the_torus_and_the_bars():
    torus, _ = tc.cases()["torus"]
    points, _ = tr.points(tr.thin(torus, tr.KEEP_ENDS)[0])
    graph = scene.skeleton_graph(points[:, :3], points[:, 3], (0.5, 0.5, 0.5))
    assert graph["nodes"] == [] and len(graph["branches"]) == 1
    loop = graph["branches"][0]
    assert loop["nodes"] == (-1, -1) and sorted(loop["voxels"].tolist()) == list(range(len(points)))
    steps = np.abs(np.diff(points[np.append(loop["voxels"], loop["voxels"][0]), :3].astype(int), axis=0)).max(axis=1)
    assert (steps == 1).all()  # walked in order, closed
    ratio = loop["length"] / (2 * math.pi * 7.0 * 0.5)
    print("loop length / 2 pi R = %.4f" % ratio)
    assert math.isfinite(ratio) and ratio > 0
    assert loop["mean_radius"] is None

    bars, _ = tc.cases()["bars"]
    thin = tr.thin(bars, tr.KEEP_ENDS)[0]
    depth = np.full(bars.shape, 9 * 256, np.uint32)
    points, depths = tr.points(thin, depth)
    graph = scene.skeleton_graph(points[:, :3], points[:, 3], (1, 1, 1), depths)
    kinds = [n["kind"] for n in graph["nodes"]]
    assert kinds.count("end") == 6 == tr.structure(thin)["ends"] and kinds.count("isolated") == 0 and kinds.count("junction") >= 1
    arms = [b for b in graph["branches"] if "end" in (graph["nodes"][b["nodes"][0]]["kind"], graph["nodes"][b["nodes"][1]]["kind"])]
    assert len(arms) == 6 and all(8 <= b["length"] <= 16 for b in arms)
    assert all(b["mean_radius"] == b["min_radius"] == 3.0 for b in graph["branches"])  # sqrt(9 * 256) / 16
    listed = sorted(v for n in graph["nodes"] for v in n["voxels"].tolist()) + sorted(v for b in graph["branches"] for v in b["voxels"].tolist())
    assert sorted(listed) == list(range(len(points)))  # every voxel is in one node or one branch


# ---- 7. resource usage
def test_no_kernel_uses_scratch_memory():
    text = open(os.path.join(ROOT, "profiles", "thin_resource_usage.txt")).read()
    kernels = re.findall(r"Function Name: (\S+)", text)
    for name in ("k_thin_begin", "k_thin_candidates", "k_thin_subpass", "k_points_count", "k_points_fill"):
        assert any(name in k for k in kernels), name
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)
    spills = re.findall(r"[SV]GPRs Spill: (\d+)", text)
    assert len(scratch) == len(kernels) >= 5 and set(scratch) == {"0"} and set(spills) == {"0"}
