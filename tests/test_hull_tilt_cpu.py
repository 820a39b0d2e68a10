"""Tilted hull planes, what can be checked without a GPU: the host's bound and target against the numpy
restatement of tools/hull_tilt.py, the octahedral encode against the table's directions, the tilt formula, the arming path's rounding,
and the restated rule on the convex shell of tests/test_gpu_hull_cert.py: no grant that the literal march does not end in Exit.

The proof, restated (csrc/clwh_internal.hpp): every corner of every event voxel lies behind EVERY plane k of the support table, so item
12's theorem -- a position in front of the plane, a constant direction with d . n_k >= delta, enough steps left -- holds for whichever
plane a march names.  The tilted rule names the cell k' of n' = n0 + lambda d (n0: the hit's plane normal, d: the march's direction),
and from there on uses only n_k' = hull_direction(k') and the table's h_k': granted at once with M' = n_k' . start - h_k' >= 0 and
d . n_k' >= delta0(70 - 5); armed with M' < 0, d . n_k' >= delta(J) = delta0(70 - 5 - J) and need = ceil(-M' / d . n_k') <= P, granted
once the counted path has reached `need` with at most J steps taken and no event.  The choice of k' is no part of the proof."""
import math
import os
import sys

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import hull_certificate as hc  # noqa: E402
import hull_defer as hd  # noqa: E402
import hull_tilt as restated  # noqa: E402

F = np.float32


# ---- the host's numbers

def _delta_restated(X, Y, Z, steps):
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


@pytest.mark.parametrize("dims", [(16, 16, 16), (64, 64, 64), (64, 48, 80), (512, 512, 512), (300, 40, 1000), (2048, 2048, 2048)])
def test_host_bound_and_target_equal_their_restatement(dims):
    delta, J, P, margin, target, gain = ffi.hull_tilt_bound(*dims)
    assert margin == restated.TARGET_MARGIN == 1.0 / 16.0
    assert 3 <= J <= 32 and 1 <= P <= 127 * J < 2 ** 22, "the armed path fits the low field of the lane's march word"
    assert delta == _delta_restated(*dims, 70 - 5 - J) == hd.defer_delta0(*dims, J)
    assert ffi.hull_defer_bound(*dims)[0] <= delta, "fewer steps left never lower the bound"
    if delta <= 1.0:
        t = delta + margin
        assert target == F(t) and gain == F(t / math.sqrt(1.0 - t * t))
    else:
        assert delta == 2.0 and 0.0 < target < 1.0, "no direction qualifies: any target below 1 will do, nothing is granted"


def test_the_16_cube_saturates():
    """cap = 8 and a reach of 30 voxels: steps of one voxel get there, the bound sits at its floor of 1/64 whatever J; the recurrence
    itself answers 2 -- no direction qualifies -- when even steps of `cap` do not reach"""
    assert ffi.hull_tilt_bound(16, 16, 16)[0] == 1.0 / 64.0 == ffi.hull_cert_bound(16, 16, 16)[0]
    assert [hd.defer_delta0(16, 16, 16, J) for J in (3, 16, 32)] == [1.0 / 64.0] * 3
    assert hd.defer_delta0(16, 16, 16, 60) == 2.0 and hd.defer_delta0(512, 512, 512, 50) == 2.0
    bounds = [hd.defer_delta0(512, 512, 512, J) for J in range(0, 33)]
    assert bounds == sorted(bounds) and bounds[0] == ffi.hull_cert_bound(512, 512, 512)[0]


# ---- the encode

def test_encode_inverts_hull_direction_for_all_4096_cells():
    dirs = hc.oct_directions(64, unit=True)
    want = np.arange(64 * 64)
    assert np.array_equal(restated.encode(dirs), want)
    assert np.array_equal(restated.encode(dirs.astype(F)), want)
    for scale in (0.3, 7.0, 1.0 - 2.0 ** -22, 1.0 + 2.0 ** -22):   # any length: v_rsq_f32 leaves the table's normals 2^-22 off 1
        assert np.array_equal(restated.encode((dirs * scale).astype(F)), want)
    assert np.array_equal(restated.encode(hc.oct_directions(64, unit=False)), want)
    i, j = hc.oct_cell(dirs, 64)
    assert np.array_equal(j * 64 + i, want), "tools/hull_certificate.py's float64 cell agrees"


def test_encode_lands_in_the_table_whatever_it_is_given():
    rng = np.random.default_rng(11)
    v = rng.normal(size=(20000, 3)).astype(F)
    v[:100] *= F(1e-30)
    v[100:200] *= F(1e30)
    v[200] = (0.0, 0.0, 0.0)
    v[201] = (np.nan, 1.0, 0.0)
    v[202] = (np.inf, -np.inf, 1.0)
    v[203:206] = np.eye(3, dtype=F)
    v[206:209] = -np.eye(3, dtype=F)
    k = restated.encode(v)
    assert k.min() >= 0 and k.max() < 64 * 64
    assert k[201] % 64 == 0, "a NaN is dropped by the clamp: column 0"
    # away from degenerate input it is the cell the direction's octahedral coordinates (in binary64) lie in, up to the rounding at a border
    ok = np.isfinite(v).all(axis=1) & (np.abs(v).sum(axis=1) > 1e-20) & (np.abs(v).sum(axis=1) < 1e20)
    p = v[ok].astype(np.float64)
    p /= np.abs(p).sum(axis=1, keepdims=True)
    uu = np.where(p[:, 2] >= 0, p[:, 0], np.copysign(1.0 - np.abs(p[:, 1]), p[:, 0]))
    vv = np.where(p[:, 2] >= 0, p[:, 1], np.copysign(1.0 - np.abs(p[:, 0]), p[:, 1]))
    centre_u, centre_v = (k[ok] % 64 + 0.5) / 32.0 - 1.0, (k[ok] // 64 + 0.5) / 32.0 - 1.0
    assert np.abs(uu - centre_u).max() <= 1.0 / 64.0 + 1e-6 and np.abs(vv - centre_v).max() <= 1.0 / 64.0 + 1e-6


# ---- the tilt

def test_tilt_reaches_its_target_and_leaves_good_normals_alone():
    rng = np.random.default_rng(4)
    n0 = rng.normal(size=(50000, 3))
    n0 /= np.linalg.norm(n0, axis=1, keepdims=True)
    d = rng.normal(size=(50000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for target in (1.0 / 64 + 1.0 / 16, 0.25 + 1.0 / 16, 0.390625, 0.9):
        npr, lam = restated.tilt(n0, d, target)
        c = (d * n0).sum(axis=1)
        assert np.all(lam[c >= target] == 0.0) and np.array_equal(npr[c >= target], n0[c >= target])
        assert np.all(lam[c < target] > 0.0)
        got = (d * npr).sum(axis=1) / np.linalg.norm(npr, axis=1)
        assert np.allclose(got[c < target], target, rtol=0, atol=1e-9)
        # ... and of all vectors at that angle to d it is the one nearest n0: it lies in the plane of n0 and d, on n0's side
        side = np.cross(np.cross(d, n0), d)
        assert np.all((npr * side).sum(axis=1)[c < target] >= -1e-12)
    # the kernel's expression, in binary32 with an approximate square root: the same cell except at cell borders
    target = 0.390625
    gain = F(target / math.sqrt(1.0 - target * target))
    c32 = (d.astype(F) * n0.astype(F)).sum(axis=1, dtype=F)
    lam32 = np.where(c32 >= F(target), F(0), gain * np.sqrt(np.maximum(F(1) - c32 * c32, F(0))).astype(F) - c32).astype(F)
    k32 = restated.encode(n0.astype(F) + lam32[:, None] * d.astype(F))
    k64 = restated.encode(restated.tilt(n0, d, target)[0])
    assert np.mean(k32 == k64) > 0.99


# ---- the arming path

def test_the_armed_path_never_falls_below_the_quotient():
    """need = ceil(-M' * rcp(d . n_k') * (1 + 2^-19)) in binary32, the reciprocal good to 2^-22 either way: at least -M' / d . n_k'"""
    rng = np.random.default_rng(8)
    M = -(rng.random(200000) * 40.0 + 2.0 ** -12).astype(F)
    dn = (1.0 / 64.0 + rng.random(200000) * (1.0 - 1.0 / 64.0)).astype(F)
    exact = -M.astype(np.float64) / dn.astype(np.float64)
    for err in (-2.0 ** -22, 0.0, 2.0 ** -22):
        r = ((1.0 / dn.astype(np.float64)) * (1.0 + err)).astype(F)
        need = np.ceil((((-M) * r).astype(F) * F(1.0 + 2.0 ** -19)).astype(F))
        assert np.all(need >= exact) and np.all(need >= 1.0)
        assert np.all(need <= np.ceil(exact * (1.0 + 2.0 ** -18)) + 0.0)
    assert np.array_equal(restated.need_of(M.astype(np.float64), dn.astype(np.float64)), np.ceil(exact * (1.0 + 2.0 ** -19)))


def test_fired_at_reads_the_kernels_counter():
    counts = np.full((3, 71), -1, np.int16)
    counts[0, 1:6] = (0, 0, 3, 9, 30)      # two half-voxel steps count 0; gone after five steps
    counts[1, 1:4] = (5, 5, -1)            # alive without a voxel after step 3: no grant there
    counts[2, 1:3] = (1, 2)
    assert list(restated.fired_at(counts, np.array([3.0, 6.0, np.inf]))) == [3, 0, 0]
    assert list(restated.fired_at(counts, np.array([10.0, 5.0, 2.0]))) == [5, 1, 2]
    assert list(restated.fired_at(counts, np.array([31.0, 1.0, 1.0]))) == [0, 1, 1]


# ---- the rule as a whole, restated, on the shell

@pytest.fixture(scope="module")
def shell(orc):
    vol, pos, d, (w, h) = hd.shell(64)
    sdf = orc.sdf_build(vol, orc.parse_tf(scene.tf_default_source()))[0]
    return restated.measure(vol, sdf, (vol >= 500) & (vol <= 1200), pos, d, w, h, rounds=4)


def test_restated_rule_grants_nothing_but_exits_on_the_shell(shell):
    dims, table = shell["dims"], shell["table"]
    _, J, P, _, _, _ = ffi.hull_tilt_bound(*dims)
    for which in ("plane", "bounce"):
        for j, p in ((J, P), (J, None), (3, None), (20, None), (32, 8)):
            for replace in (False, True):
                for kind in ("first", "rebound"):
                    g = restated.beside(shell[kind], table, dims, j, np.inf, which, replace, p)
                    assert g["wrong_once"] == g["wrong_deferred"] == g["shipped_wrong"] == 0, (which, j, p, replace, kind)
    first = restated.beside(shell["first"], table, dims, J, np.inf, "plane", P=P)
    assert first["n"] > 5000 and first["tried"] > 1000
    # not vacuous: on this scene the rule ends more than one in three of the first legs that reach it, nearly all that exit
    assert 3 * first["granted"] >= first["tried"] and 10 * first["granted"] >= 8 * first["exits_left"]
    assert first["deferred"] > 0 and np.all(first["fired"] <= J) and np.all(first["fired"] >= 1)


def test_item_13_keeps_its_grants_under_the_shared_step_count(shell):
    """with the rule on, item 13's armed marches get the kernel's one J and its higher bound: what they lose the tilted rule takes"""
    dims, table = shell["dims"], shell["table"]
    _, J, P, _, _, _ = ffi.hull_tilt_bound(*dims)
    rec = shell["first"]
    _, _, parent_deferred, _ = restated.shipped(rec, table, dims, restated.J13)
    once, _, deferred, _ = restated.shipped(rec, table, dims, J)
    g = restated.beside(rec, table, dims, J, np.inf, "plane", P=P)
    assert int(deferred.sum()) + g["granted"] >= int(parent_deferred.sum())


def test_directions_with_a_small_or_missing_component_are_never_granted(shell):
    """the guards of items 12 and 13: a component below 2^-10 (the far-face crawl) or a NaN -- neither granted at once nor armed"""
    dims, table = shell["dims"], shell["table"]
    _, J, P, _, _, _ = ffi.hull_tilt_bound(*dims)
    rec = {key: val[:2000].copy() for key, val in shell["first"].items()}
    d = rec["d"]
    d[0::4, 0] = 0.0
    d[1::4, 1] = np.float32(2.0 ** -11)
    d[2::4, 2] = np.nan
    d[3::4, 0] = -np.float32(2.0 ** -11)
    with np.errstate(invalid="ignore"):
        rec["ok_dir"] = (np.abs(d).min(axis=1) >= 2.0 ** -10) & ~np.isnan(d).any(axis=1)   # (as tools/hull_tilt.py forms it)
    assert not rec["ok_dir"].any()
    for which in ("plane", "bounce"):
        once, armed, deferred, _, k2 = restated.tilted(rec, table, dims, J, np.inf, which, P)
        assert not once.any() and not armed.any() and not deferred.any()
        assert k2.min() >= 0 and k2.max() < 64 * 64
