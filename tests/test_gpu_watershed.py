"""clwh_watershed on the GPU against the contract's Python restatement (tests/watershed_ref.py) over the shared cases
(tests/watershed_cases.py): equal bytes of both maps, no tolerance anywhere.  Every case runs for 6 and 26 neighbours, twice on one
context by the worklist and twice with CLWH_GEO_DENSE; the maps are allocated four words too long and pre-filled with a pattern that
must survive behind X * Y * Z; cost, domain and a separate seed_labels are read only; the domain's padding bits are set.  Then device
against device where two calls must agree, the composition from a volume, the host mirror and the headless program."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import costpath_ref as cp
from tests import watershed_cases as wc
from tests import watershed_ref as w
from tests.view_helpers import ROOT, host_lib

pytestmark = pytest.mark.gpu

NONE = w.NONE
PATTERN = 0xA5A5A5A5
BOTH = (6, 26)


def dims_of(a):
    Z, Y, X = a.shape
    return X, Y, Z


def same(got, want, what):
    assert got.dtype == want.dtype and np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:3].tolist())


def flag_of(connectivity):
    return ffi.GEO_26 if connectivity == 26 else 0


def pack_with_padding_set(mask):
    """scene.mask_pack with every bit at x >= X set: the call ignores them"""
    m = np.asarray(mask, bool)
    Z, Y, X = m.shape
    wpr = scene.mask_words_per_row(X)
    padded = np.ones((Z, Y, wpr * 32), np.uint8)
    padded[:, :, :X] = m
    words = np.packbits(padded, axis=2, bitorder="little").view("<u4").reshape(-1).astype(np.uint32, copy=False)
    assert np.array_equal(scene.mask_unpack(words, (X, Y, Z)), m) and (X % 64 == 0 or not np.array_equal(words, scene.mask_pack(m)))
    return words


def run(ctx, k, connectivity, outputs="both"):
    """(labels, level, result dict) as the device wrote them, uint32 [z][y][x]; an output that was not asked for is None"""
    cost = np.ascontiguousarray(k["cost"], np.uint16)
    dims = X, Y, Z = dims_of(cost)
    n = X * Y * Z
    d_cost = ctx.buffer_from(cost)
    words = pack_with_padding_set(k["domain"]) if k["domain"] is not None else None
    d_domain = ctx.buffer_from(words) if words is not None else None
    labels = ctx.buffer(4 * (n + 4), np.uint32, (n + 4,)) if outputs in ("both", "labels") else None
    level = ctx.buffer(4 * (n + 4), np.uint32, (n + 4,)) if outputs in ("both", "level") else None
    seed_labels, in_place = k["seed_labels"], k["in_place"] and labels is not None
    given = None
    if seed_labels is not None:
        given = labels if in_place else ctx.buffer_from(np.ascontiguousarray(seed_labels, np.uint32))
    base = flag_of(connectivity) | (ffi.GEO_FROM_LABELS if seed_labels is not None else 0)
    first = None
    for turn, dense in (("first", 0), ("again", 0), ("dense", ffi.GEO_DENSE), ("dense again", ffi.GEO_DENSE)):
        for m in (labels, level):
            if m is not None:
                m.push(np.full(n + 4, PATTERN, np.uint32))
        if in_place:
            labels.push(np.concatenate([np.asarray(seed_labels, np.uint32).reshape(-1), np.full(4, PATTERN, np.uint32)]))
        status, res = ctx.watershed_raw(d_cost, dims, k["seeds"], d_domain, given, base | dense, k["plateau_cap"], k["level_cap"], labels,
                                        level)
        assert status == 0, (status, k["name"], turn)
        got = []
        for m in (labels, level):
            a = m.pull() if m is not None else None
            assert a is None or (a[n:] == PATTERN).all(), (k["name"], turn, "written behind X * Y * Z")
            got.append(a[:n].reshape(Z, Y, X).copy() if a is not None else None)
        got.append(res.as_dict())
        if first is None:
            first = got + [int(res.rounds)]
        for a, b in zip(first[:2], got[:2]):
            assert (a is None and b is None) or np.array_equal(a, b), (k["name"], turn, "differs from the first call")
        assert first[2] == got[2], (k["name"], turn)
    assert np.array_equal(d_cost.pull().reshape(cost.shape), cost), "the cost is read only"
    assert d_domain is None or np.array_equal(d_domain.pull(), words), "the domain is read only"
    if given is not None and not in_place:
        assert np.array_equal(given.pull().reshape(-1), np.asarray(seed_labels, np.uint32).reshape(-1)), "seed_labels is read only"
        given.release()
    for m in (d_cost, d_domain, labels, level):
        if m is not None:
            m.release()
    return first


# ---- 1. every shared case against the reference
@pytest.mark.parametrize("connectivity", BOTH)
@pytest.mark.parametrize("name", wc.NAMES)
def test_cases_equal_the_reference(gpu_ctx, name, connectivity):
    k = wc.case(name)
    want_labels, want_level = wc.expected(name, connectivity)
    labels, level, res, rounds = run(gpu_ctx, k, connectivity)
    same(level, want_level, (name, connectivity, "level"))
    same(labels, want_labels, (name, connectivity, "labels"))
    assert res == w.result(want_level), (name, connectivity)
    if name == "corridor":
        assert rounds > 2 * 8, "more than one host read in each phase"


# ---- 2. one output at a time
@pytest.mark.parametrize("outputs", ("labels", "level"))
def test_one_output(gpu_ctx, outputs):
    for name in ("low-17x17x9", "from-labels", "from-labels-in-place"):
        want_labels, want_level = wc.expected(name, 26)
        labels, level, res, _ = run(gpu_ctx, wc.case(name), 26, outputs)
        assert (labels is None) == (outputs == "level") and (level is None) == (outputs == "labels")
        if labels is not None:
            same(labels, want_labels, (name, outputs))
        if level is not None:
            same(level, want_level, (name, outputs))
        assert res == w.result(want_level)


# ---- 3. device against device
@pytest.mark.parametrize("connectivity", BOTH)
def test_constant_cost_equals_mask_geodesic_on_the_device(gpu_ctx, connectivity):
    ctx = gpu_ctx
    k = wc.case("constant-plateau%d" % w.PLATEAU_MAX)
    dims = X, Y, Z = dims_of(k["cost"])
    n = X * Y * Z
    d_cost, d_domain = ctx.buffer_from(np.ascontiguousarray(k["cost"])), ctx.buffer_from(scene.mask_pack(np.ones((Z, Y, X), bool)))
    maps = [ctx.buffer(4 * n, np.uint32, (n,)) for _ in range(4)]
    a, ra = ctx.mask_geodesic_raw(d_domain, dims, k["seeds"], None, flag_of(connectivity), None, NONE, maps[0], maps[1])
    b, rb = ctx.watershed_raw(d_cost, dims, k["seeds"], None, None, flag_of(connectivity), labels=maps[2], level=maps[3])
    assert (a, b) == (0, 0) and ra.reached == rb.reached == n and rb.max_level == 7
    same(maps[2].pull(), maps[1].pull(), (connectivity, "labels"))
    dist, level = maps[0].pull(), maps[3].pull()
    away = dist != 0
    same(level[away], (7 << 16 | (dist[away] - 1)).astype(np.uint32), (connectivity, "level"))
    for m in maps + [d_cost, d_domain]:
        m.release()


@pytest.mark.parametrize("connectivity", BOTH)
def test_ridge_against_the_cost_geodesic_on_the_device(gpu_ctx, connectivity):
    ctx = gpu_ctx
    cost = wc.ridge()
    dims = X, Y, Z = dims_of(cost)
    d_cost = ctx.buffer_from(np.ascontiguousarray(cost))
    flooded, level, _ = ctx.watershed(d_cost, dims, wc.RIDGE_SEEDS, connectivity=connectivity)
    dist, summed, _ = ctx.cost_geodesic(d_cost, dims, wc.RIDGE_SEEDS, connectivity=connectivity)
    flooded, summed = flooded.pull().reshape(Z, Y, X), summed.pull().reshape(Z, Y, X)
    wall = wc.RIDGE_WALL_X
    assert (flooded[:, :, :wall] == 1).all() and (flooded[:, :, wall + 1:] == 2).all()
    assert (summed[:, :, wall + 1:] == 1).sum() > 0, "the sum spills over the ridge"
    assert (flooded == summed)[:, :, :wall].all()


def two_blocks():
    """24^3: two blocks of different value in a noisy background, a click in each"""
    rng = np.random.default_rng(31)
    v = rng.integers(-30, 31, (24, 24, 24)).astype(np.int16)
    v[4:20, 4:20, 3:11] += 800
    v[4:20, 4:20, 13:21] += 1500
    return v, [(7, 12, 12, 1), (17, 12, 12, 2)]


@pytest.mark.parametrize("connectivity", BOTH)
def test_watershed_edges_from_a_volume(gpu_ctx, connectivity):
    ctx = gpu_ctx
    vol, seeds = two_blocks()
    dims = X, Y, Z = dims_of(vol)
    image = ctx.image_from(vol)
    for g_max in (4096, 300):
        table, shift = scene.watershed_gradient_table(g_max)
        cost = cp.cost_from_field(vol, table, 0, shift, cp.SRC_GRADIENT)
        want_labels, want_level = w.watershed(cost, seeds, connectivity)
        labels, level, res = ctx.watershed_edges(image, dims, seeds, connectivity=connectivity, g_max=g_max)
        same(labels.pull().reshape(Z, Y, X), want_labels, (g_max, "labels"))
        same(level.pull().reshape(Z, Y, X), want_level, (g_max, "level"))
        assert res.as_dict() == w.result(want_level)
        labels.release()
        level.release()
    # the border lies between the blocks: each block's core belongs to its own click
    assert (want_labels[5:19, 5:19, 4:10] == 1).all() and (want_labels[5:19, 5:19, 14:20] == 2).all()
    assert np.array_equal(image.pull().reshape(vol.shape), vol)
    image.release()


# ---- 4. the host mirror and the headless program
def test_host_mirror_watershed_and_its_table():
    vol, seeds = two_blocks()
    Z, Y, X = vol.shape
    env = scene.env_map(64, 32)
    L = host_lib(clvr_host_watershed_table=(C.c_uint, [C.c_uint, C.c_void_p, C.c_uint, C.POINTER(C.c_uint)]),
                 clvr_host_watershed_edges=(C.c_ulonglong, [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_uint, C.c_uint, C.c_void_p,
                                                            C.c_void_p, C.POINTER(C.c_uint)]))
    for g_max in (1, 255, 256, 4096, 65535 * 2):
        want, want_shift = scene.watershed_gradient_table(g_max)
        got, shift = np.zeros(65536, np.uint16), C.c_uint(99)
        n = L.clvr_host_watershed_table(g_max, got.ctypes.data, len(got), C.byref(shift))
        assert n == len(want) and shift.value == want_shift and np.array_equal(got[:n], want), g_max
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, X, Y, Z, env.ctypes.data, 64, 32)
        table, shift = scene.watershed_gradient_table(4096)
        cost = cp.cost_from_field(vol, table, 0, shift, cp.SRC_GRADIENT)
        rows = np.array(seeds, np.uint32)
        for flags, plateau in ((0, w.PLATEAU_MAX), (ffi.GEO_26, 0)):
            want_labels, want_level = w.watershed(cost, seeds, 26 if flags else 6, plateau)
            labels, level, max_level = np.zeros((Z, Y, X), np.uint32), np.zeros((Z, Y, X), np.uint32), C.c_uint(0)
            reached = L.clvr_host_watershed_edges(h, rows.ctypes.data, len(rows), flags, 4096, plateau, labels.ctypes.data, level.ctypes.data,
                                                  C.byref(max_level))
            assert {"reached": reached, "max_level": max_level.value} == w.result(want_level)
            same(labels, want_labels, (flags, "labels"))
            same(level, want_level, (flags, "level"))
    finally:
        L.clvr_host_destroy(h)


def test_headless_watershed(tmp_path):
    vol, seeds = two_blocks()
    scene.write_nrrd(str(tmp_path / "v.nrrd"), vol)
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(np.random.default_rng(5).random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", "64", "64", str(tmp_path / "out")]

    def headless(*options):
        out = subprocess.run([exe] + list(options) + files, capture_output=True, text=True, timeout=120)
        return out.returncode, [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")], out.stderr

    clicks = ",".join("%d:%d:%d" % s[:3] for s in seeds)
    for extra, connectivity, g_max, plateau in ((",26,gmax=300,plateau=0", 26, 300, 0), ("", 6, 4096, w.PLATEAU_MAX)):  # the defaults last
        table, shift = scene.watershed_gradient_table(g_max)
        cost = cp.cost_from_field(vol, table, 0, shift, cp.SRC_GRADIENT)
        labels, level = w.watershed(cost, seeds, connectivity, plateau)
        code, lines, err = headless("--watershed=" + clicks + extra, "--mesh=50")
        assert code == 0, err
        want = dict(w.result(level), counts=[int((labels == i).sum()) for i in (1, 2)], seeds=2, connectivity=connectivity, gmax=g_max,
                    plateau=plateau, mode="none", fill=-32768)
        assert lines[0] == {"watershed": want}, (extra, lines[0])
    for tail, view in ((",show", "--slice=axial"), (",show=outline", "--projection=max"), (",keep=2", "--mesh=50"), (",remove=1,fill=-500", "--mesh=50")):
        code, lines, err = headless("--watershed=" + clicks + tail, view)
        assert code == 0 and lines[0]["watershed"]["counts"] == want["counts"], (tail, err)
        assert lines[0]["watershed"]["mode"] == tail.split("=")[0].split(",")[1]
    assert headless("--watershed=" + clicks + ",show", "--mesh=50")[0] == 1, "show needs a view"
    for bad in ("--watershed=", "--watershed=1:2", "--watershed=1:2:x", "--watershed=99:2:3", "--watershed=1:2:3,gmax=0",
                "--watershed=1:2:3,plateau=65535", "--watershed=1:2:3,keep=3", "--watershed=1:2:3,show,keep=1", "--watershed=1:2:3,what",
                "--watershed=1:2:3,", "--watershed=26,1:2:3", "--watershed=1:2:3,fill=5", "--watershed=1:-2:3", "--watershed=1:2:3:4"):
        assert headless(bad, "--mesh=50")[0] == 1, bad
    assert headless("--watershed=" + clicks, "--grow=1,2,3,0,100", "--mesh=50")[0] == 1
    assert headless("--watershed=" + clicks, "--components=0,100", "--mesh=50")[0] == 1
