"""clwh_mask_geodesic and clwh_geodesic_trace on the GPU against the contract's Python restatement (tests/geodesic_ref.py): equal bytes
of both maps, no tolerance anywhere.  Every case runs twice on one context, by the worklist and with CLWH_GEO_DENSE; the maps are
allocated four words too long and pre-filled with a pattern that must survive behind X * Y * Z; the domain is read only."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import geodesic_ref as g
from tests import label_ref as lr
from tests.grow_ref import RANDOM_DIMS
from tests import overlay_ref as ovr
from tests import slice_ref as sr
from tests.test_gpu_distance import garbage
from tests.view_helpers import ROOT, host_lib

pytestmark = pytest.mark.gpu

INVALID_VALUE, SIZE_MISMATCH = 1, 9
NONE = g.NONE
PATTERN = 0xA5A5A5A5
TILE = (16, 16, 8)  # geodesic_kernels.hip's


def dims_of(a):
    Z, Y, X = a.shape
    return X, Y, Z


def same(got, want, what):
    assert got.dtype == want.dtype and np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:3].tolist())


class Device:
    def __init__(self, ctx):
        self.ctx = ctx

    def geodesic(self, words, dims, seeds=None, connectivity=6, weights=None, cap=None, seed_labels=None, outputs="both", in_place=False):
        """(dist, labels, result dict) as the device wrote them, uint32 [z][y][x]; an output that was not asked for is None"""
        X, Y, Z = dims
        n = X * Y * Z
        domain = self.ctx.buffer_from(words)
        dist = self.ctx.buffer(4 * (n + 4), np.uint32, (n + 4,)) if outputs in ("both", "dist") else None
        labels = self.ctx.buffer(4 * (n + 4), np.uint32, (n + 4,)) if outputs in ("both", "labels") else None
        given = None
        if seed_labels is not None:
            given = labels if in_place else self.ctx.buffer_from(np.ascontiguousarray(seed_labels, np.uint32))
        base = (ffi.GEO_26 if connectivity == 26 else 0) | (ffi.GEO_FROM_LABELS if seed_labels is not None else 0)
        first = None
        for turn, dense in (("first", 0), ("again", 0), ("dense", ffi.GEO_DENSE), ("dense again", ffi.GEO_DENSE)):
            for m in (dist, labels):
                if m is not None:
                    m.push(np.full(n + 4, PATTERN, np.uint32))
            if in_place:
                labels.push(np.concatenate([np.asarray(seed_labels, np.uint32).reshape(-1), np.full(4, PATTERN, np.uint32)]))
            status, res = self.ctx.mask_geodesic_raw(domain, dims, seeds, given, base | dense, weights, NONE if cap is None else cap, dist, labels)
            assert status == 0, (status, dims, turn)
            got = []
            for m in (dist, labels):
                a = m.pull() if m is not None else None
                assert a is None or (a[n:] == PATTERN).all(), (dims, turn, "written behind X * Y * Z")
                got.append(a[:n].reshape(Z, Y, X).copy() if a is not None else None)
            got.append(res.as_dict())
            if first is None:
                first = got
            for a, b in zip(first[:2], got[:2]):
                assert (a is None and b is None) or np.array_equal(a, b), (dims, turn, "differs from the first call")
            assert first[2] == got[2], (dims, turn)
        assert np.array_equal(domain.pull(), words), "the domain is read only"
        if given is not None and not in_place:
            assert np.array_equal(given.pull().reshape(-1), np.asarray(seed_labels, np.uint32).reshape(-1)), "seed_labels is read only"
            given.release()
        for m in (domain, dist, labels):
            if m is not None:
                m.release()
        return first

    def check(self, domain, seeds, connectivity=6, weights=None, cap=None, seed_labels=None, want=None, words=None, **kw):
        want = want if want is not None else g.geodesic(domain, seeds, connectivity, weights, cap, seed_labels)
        what = (dims_of(domain), connectivity, weights, cap, kw)
        dist, labels, res = self.geodesic(scene.mask_pack(domain) if words is None else words, dims_of(domain), seeds, connectivity, weights,
                                          cap, seed_labels, **kw)
        if dist is not None:
            same(dist, want[0], what + ("dist",))
        if labels is not None:
            same(labels, want[1], what + ("labels",))
        assert res == g.result(want[0]), what
        return want


# ---- 1. random domains: ragged in every axis, two or more tiles along x, several along y and z
@pytest.mark.parametrize("connectivity", (6, 26))
@pytest.mark.parametrize("dims", RANDOM_DIMS)
def test_random_domains_equal_the_reference(gpu_ctx, dims, connectivity):
    dev = Device(gpu_ctx)
    assert scene.geodesic_weights((1, 1, 1), 10) == g.CHAMFER and scene.geodesic_weights((0.7, 0.7, 2.5), 10) == g.ANISO
    for weights in (g.UNIT, g.ANISO, g.CHAMFER):
        for cap in (None, 40 * min(weights[0])):
            domain, seeds, dist, labels = g.random_case(dims, connectivity, weights, cap)
            dev.check(domain, seeds, connectivity, weights, cap, want=(dist, labels))


def test_garbage_outside_the_volume_is_ignored(gpu_ctx):
    dev = Device(gpu_ctx)
    for dims in ((65, 17, 17), (33, 40, 35)):
        domain, seeds, dist, labels = g.random_case(dims, 6, g.CHAMFER, None)
        words = garbage(domain)
        assert not np.array_equal(words, scene.mask_pack(domain))
        dev.check(domain, seeds, 6, g.CHAMFER, want=(dist, labels), words=words)


# ---- 2. long paths that cross tile faces many times
@pytest.mark.parametrize("shape", ("serpentines", "comb"))
def test_long_paths(gpu_ctx, shape):
    dev = Device(gpu_ctx)
    domain = (lr.two_serpentines() if shape == "serpentines" else lr.comb()) == 100
    seed = (0, 0, 1, 7) if shape == "serpentines" else (0, 0, 0, 7)
    assert domain[seed[2], seed[1], seed[0]]
    for connectivity, weights in ((6, (3, 5, 11)), (26, g.CHAMFER)):
        want = dev.check(domain, [seed], connectivity, weights)
        free = g.geodesic(np.ones_like(domain), [seed], connectivity, weights)[0].astype(np.int64)
        far = (want[0] != NONE) & (want[0].astype(np.int64) >= (20 if shape == "serpentines" else 3) * free)
        assert int(far.sum()) > 100, "many voxels lie several times as far through the domain as through the box"
        if shape == "serpentines":  # the second serpentine has no seed: unreached, label 0
            assert (want[1][3] == 0).all() and domain[3].any() and (want[1][1][domain[1]] == 7).all()


# ---- 3. ties across a tile face, and domains that touch only diagonally at a tile corner
def test_ties_across_a_tile_face(gpu_ctx):
    """two seeds mirrored about a plane of voxels: the last plane in front of the face between two tiles, and the first one behind it"""
    dev = Device(gpu_ctx)
    box = np.ones((12, 20, 40), bool)
    for axis in range(3):
        for plane in (TILE[axis] - 1, TILE[axis]):
            for connectivity, weights in ((6, (3, 5, 11)), (26, g.CHAMFER)):
                a, b = [4, 4, 4], [4, 4, 4]
                a[axis], b[axis] = plane - 2, plane + 2
                seeds = [tuple(b) + (9,), tuple(a) + (4,)]
                want = dev.check(box, seeds, connectivity, weights)
                tie = g.ties(box, seeds, connectivity, weights)
                on_plane = [slice(None)] * 3
                on_plane[2 - axis] = plane
                assert tie[tuple(on_plane)].all() and int(tie.sum()) == tie[tuple(on_plane)].size, (axis, plane, connectivity)
                assert (want[1][tie] == 4).all() and {int(v) for v in np.unique(want[1])} == {4, 9}


def test_diagonal_contact_at_a_tile_corner(gpu_ctx):
    dev = Device(gpu_ctx)
    cx, cy, cz = 2 * TILE[0], TILE[1], TILE[2]  # a corner that eight tiles share
    block = lambda x, y, z: (slice(z, z + 4), slice(y, y + 4), slice(x, x + 4))
    domain = np.zeros((2 * cz, 2 * cy, 2 * cx), bool)
    domain[block(cx - 4, cy - 4, cz - 4)] = True  # ends at the corner
    domain[block(cx, cy, cz)] = True              # begins there, in the tile across the corner
    seeds = [(cx - 3, cy - 3, cz - 3, 3)]
    apart = dev.check(domain, seeds, 6, (10, 10, 10))
    assert (apart[1][block(cx, cy, cz)] == 0).all(), "no face in common: unreached under 6-connectivity"
    joined = dev.check(domain, seeds, 26, g.CHAMFER)
    assert (joined[1][domain] == 3).all() and int(joined[0][cz, cy, cx]) == int(joined[0][cz - 1, cy - 1, cx - 1]) + 17
    # and along a tile edge only: the second block moves back into the first one's z range
    domain[block(cx, cy, cz)] = False
    domain[block(cx, cy, cz - 4)] = True
    joined = dev.check(domain, seeds, 26, g.CHAMFER)
    assert (joined[1][domain] == 3).all() and int(joined[0][cz - 3, cy, cx]) == int(joined[0][cz - 3, cy - 1, cx - 1]) + 14
    # seeds of two ids, one in each block, two corner steps each from the last voxel in front of the corner: a tie there
    domain[:] = False
    domain[block(cx - 4, cy - 4, cz - 4)] = domain[block(cx, cy, cz)] = True
    seeds = [(cx + 1, cy + 1, cz + 1, 8), (cx - 3, cy - 3, cz - 3, 6)]
    want = dev.check(domain, seeds, 26, g.CHAMFER)
    assert g.ties(domain, seeds, 26, g.CHAMFER)[cz - 1, cy - 1, cx - 1]
    assert int(want[1][cz - 1, cy - 1, cx - 1]) == 6 and int(want[1][cz, cy, cx]) == 8


# ---- 4. the seed rules, the extremes, the outputs
def test_seed_rules_and_extremes(gpu_ctx):
    dev = Device(gpu_ctx)
    dims = X, Y, Z = (70, 19, 18)
    domain = np.zeros((Z, Y, X), bool)
    domain[2:16, 2:17, 2:30] = True
    domain[2:16, 2:17, 40:68] = True  # a component without a seed
    seeds = [(5, 5, 5, 9), (5, 5, 5, 3), (5, 5, 5, 12), (20, 10, 10, 3), (35, 9, 9, 1), (20, 10, 10, 3), (0, 0, 0, 2)]
    want = dev.check(domain, seeds, 6, (2, 3, 4))
    assert int(want[1][5, 5, 5]) == 3 and (want[1][:, :, 40:] == 0).all() and (want[0][:, :, 40:] == NONE).all()
    assert not (want[1] == 1).any() and not (want[1] == 2).any(), "a seed outside D contributes nothing"
    for outputs in ("dist", "labels"):
        dev.check(domain, seeds, 6, (2, 3, 4), want=want, outputs=outputs)
    for cap in (0, 1, 7, ffi.GEO_CAP_MAX):
        capped = dev.check(domain, seeds, 26, g.ANISO, cap)
        assert cap != 0 or g.result(capped[0]) == {"reached": 2, "max_dist": 0}
    # all seeds outside D; an empty D; a full D
    none = dev.check(domain, [(0, 0, 0, 2)], 6)
    assert g.result(none[0]) == {"reached": 0, "max_dist": 0}
    dev.check(np.zeros((Z, Y, X), bool), seeds, 26)
    for d in ((1, 1, 1), (7, 1, 1), (33, 9, 9), (64, 3, 2), (65, 3, 2)):
        full = np.ones(d[::-1], bool)
        want = dev.check(full, [(d[0] - 1, 0, d[2] - 1, 5)], 26, g.CHAMFER)
        assert g.result(want[0])["reached"] == full.size
    # the largest weights and the largest cap: no sum wraps
    line = np.ones((1, 1, 40), bool)
    want = dev.check(line, [(0, 0, 0, 0xFFFFFFFF)], 6, (65535, 65535, 65535))
    assert int(want[0][0, 0, 39]) == 39 * 65535 and int(want[1][0, 0, 39]) == 0xFFFFFFFF
    dev.check(line, [(0, 0, 0, 1)], 6, (65535, 1, 1), cap=3 * 65535)


def test_offsets_past_two_to_the_31(gpu_ctx):
    """1024 x 1024 x 513 voxels: the byte offsets of the last keys pass 2^32 and those of both maps 2^31.  The domain is two lines along
    x, the first and the last row of the volume, with a seed each; only the ends of the maps and samples between them are pulled"""
    ctx = gpu_ctx
    dims = X, Y, Z = (1024, 1024, 513)
    n, wpr = X * Y * Z, scene.mask_words_per_row(X)
    assert 2 ** 29 < n < 2 ** 31
    words = np.zeros(wpr * Y * Z, np.uint32)
    words[:wpr] = words[-wpr:] = 0xFFFFFFFF
    domain = ctx.buffer_from(words)
    dist, labels = ctx.buffer(4 * n, np.uint32), ctx.buffer(4 * n, np.uint32)
    seeds = [(1000, 0, 0, 7), (10, Y - 1, Z - 1, 9)]
    status, res = ctx.mask_geodesic_raw(domain, dims, seeds, None, 0, (3, 5, 11), NONE, dist, labels)
    assert status == 0 and res.as_dict() == {"reached": 2 * X, "max_dist": 3 * (X - 1 - 10)}
    x = np.arange(X, dtype=np.int64)

    def part(m, first, count):
        view = ctx.wrap(m.device_ptr + 4 * first, 4 * count)
        out = view.pull(np.uint32)
        view.release()
        return out

    assert np.array_equal(part(dist, 0, X), 3 * abs(x - 1000)) and (part(labels, 0, X) == 7).all()
    assert np.array_equal(part(dist, n - X, X), 3 * abs(x - 10)) and (part(labels, n - X, X) == 9).all()
    for first in (X, n // 2 - 5000, 2 ** 29 - 4096, n - X - 8192):  # behind the first line, the middle, across 2^31 bytes, before the last line
        assert (part(dist, first, 8192) == NONE).all() and not part(labels, first, 8192).any(), first
    points, count = ctx.geodesic_trace(dist, dims, (X - 1, Y - 1, Z - 1), labels, weights=(3, 5, 11), capacity=8)
    assert count == X - 10 and points.tolist() == [[X - 1 - k, Y - 1, Z - 1] for k in range(8)]
    for m in (labels, dist, domain):
        m.release()


def test_seeds_from_labels(gpu_ctx):
    dev = Device(gpu_ctx)
    dims = (70, 40, 36)
    domain, seeds, _, _ = g.random_case(dims, 6, g.CHAMFER, None)
    rng = np.random.default_rng(3)
    given = np.where(rng.random(domain.shape) < 0.002, rng.integers(1, 50, domain.shape), 0).astype(np.uint32)
    assert (given[domain] != 0).sum() > 10 and (given[~domain] != 0).sum() > 10, "nonzero words inside D and outside it"
    alone = dev.check(domain, None, 6, g.CHAMFER, seed_labels=given)
    both = dev.check(domain, seeds, 6, g.CHAMFER, seed_labels=given)
    assert not np.array_equal(alone[1], both[1])
    dev.check(domain, None, 6, g.CHAMFER, seed_labels=given, want=alone, in_place=True)
    dev.check(domain, seeds, 26, g.CHAMFER, seed_labels=given, in_place=True, outputs="labels")


# ---- 5. the split
def test_split_of_two_balls(gpu_ctx):
    ctx = gpu_ctx
    mask, _, want, n_parts = g.two_balls_split()
    dims = dims_of(mask)
    volume = ctx.image_from(np.zeros(mask.shape, np.int16))
    words = scene.mask_pack(mask)
    m = ctx.buffer_from(words)
    for _ in range(2):
        labels, n = ctx.split_mask(volume, m, dims, g.TWO_BALLS_RADIUS_SQ)
        assert n == n_parts == 2
        same(labels.pull().reshape(mask.shape), want, "territories")
        labels.release()
    assert np.array_equal(m.pull(), words)
    labels, n = ctx.split_mask(volume, m, dims, 10000)  # nothing survives the erosion
    assert n == 0 and not labels.pull().any()
    for x in (labels, m, volume):
        x.release()


def two_ball_volume():
    mask = g.two_balls_split()[0]
    return np.where(mask, 100, 0).astype(np.int16)


def test_host_mirror_split_map_and_path():
    """renderer::split_mask, geodesic_map and trace_path; a radius of 6 x-voxels is radius_sq 36 in voxels"""
    mask, _, parts, n_parts = g.two_balls_split()
    vol = two_ball_volume()
    Z, Y, X = vol.shape
    env = scene.env_map(64, 32)
    L = host_lib(clvr_host_grow_region=(None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]),
                 clvr_host_split_mask=(C.c_ulonglong, [C.c_void_p, C.c_float, C.c_int, C.POINTER(C.c_uint)]),
                 clvr_host_measure_labels=(None, [C.c_void_p, C.c_uint, C.c_void_p]),
                 clvr_host_geodesic_map=(None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_uint, C.c_void_p, C.POINTER(C.c_ulonglong)]),
                 clvr_host_trace_path=(C.c_ulonglong, [C.c_void_p, C.POINTER(C.c_uint), C.c_int, C.c_void_p, C.c_ulonglong]))
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, X, Y, Z, env.ctypes.data, 64, 32)
        click = np.array([56, 12, 12], np.uint32)
        grown = ffi.GrowResult()
        L.clvr_host_grow_region(h, click.ctypes.data, 1, 100, 100, 0, C.byref(grown))
        assert grown.count == int(mask.sum())
        info = (C.c_uint * 4)()
        assert L.clvr_host_split_mask(h, 6.0, 0, info) == n_parts == 2 and list(info) == [36 * 256, 256, 256, 256]
        records = np.zeros(2, scene.REGION_STATS_DTYPE)
        L.clvr_host_measure_labels(h, 2, records.ctypes.data)
        assert records["count"].tolist() == [int((parts == 1).sum()), int((parts == 2).sum())]
        weights = scene.geodesic_weights((1, 1, 1), 16)
        seeds = np.array([(56, 12, 12, 5), (70, 12, 12, 9)], np.uint32)
        for flags, connectivity in ((0, 6), (ffi.GEO_26, 26)):
            want = g.geodesic(mask, seeds, connectivity, weights)
            got, res = np.empty(vol.shape, np.uint32), (C.c_ulonglong * 2)()
            L.clvr_host_geodesic_map(h, seeds.ctypes.data, 2, flags, NONE, got.ctypes.data, res)
            same(got, want[0], ("host map", connectivity))
            assert {"reached": res[0], "max_dist": res[1]} == g.result(want[0])
            for target in ((48, 12, 12), (66, 10, 14), (0, 0, 0)):
                path, complete = g.trace(want[0], target, connectivity, weights, want[1])
                out = np.zeros((200, 3), np.uint32)
                n = L.clvr_host_trace_path(h, (C.c_uint * 3)(*target), flags, out.ctypes.data, 200)
                assert complete and n == len(path) and out[:n].tolist() == [list(p) for p in path], (target, connectivity)
            assert len(path) == 0 and len(g.trace(want[0], (66, 10, 14), connectivity, weights, want[1])[0]) > 3
    finally:
        L.clvr_host_destroy(h)


def test_headless_split(tmp_path):
    mask, _, parts, _ = g.two_balls_split()
    vol = two_ball_volume()
    dims, W, H = dims_of(vol), 256, 128
    scene.write_nrrd(str(tmp_path / "v.nrrd"), vol)
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(np.random.default_rng(5).random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", str(W), str(H)]

    def run(*options):
        out = subprocess.run([exe] + list(options) + files + [str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
        return out.returncode, [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")], out.stderr

    split = {"radius_sq": 36 * 256, "weight": [256, 256, 256], "connectivity": 6, "parts": 2,
             "counts": [int((parts == 1).sum()), int((parts == 2).sum())]}
    code, lines, err = run("--grow=56,12,12,100,100,split=6", "--mesh=50")
    assert code == 0, err
    assert lines[0]["count"] == int(mask.sum()) and lines[1] == {"split": split}
    code, lines, err = run("--components=100,100,measure,split=6", "--mesh=50")
    assert code == 0, err
    assert lines[0]["n_components"] == 1 and lines[1]["measure_components"][0]["count"] == int(mask.sum()) and lines[2] == {"split": split}
    code, lines, err = run("--grow=56,12,12,100,100,erode=1,split=100", "--mesh=50")  # nothing survives that erosion
    assert code == 0 and lines[1]["split"]["parts"] == 0 and lines[1]["split"]["counts"] == [], err
    assert len(run("--grow=56,12,12,100,100", "--mesh=50")[1]) == len(lines) - 1  # no item: no line
    for bad in ("split=", "split=-1", "split=x", "split=2,split=3", "split"):
        assert run("--grow=56,12,12,100,100," + bad, "--mesh=50")[0] == 1, bad
    assert run("--components=100,100,split=")[0] == 1
    # show: the parts are coloured by their id over the slice of the volume as loaded
    code, lines, err = run("--components=100,100,split=6,show=both", "--slice=axial")
    assert code == 0, err
    assert lines[0]["mode"] == "show" and lines[1] == {"split": split} and lines[-1]["overlay"] == "both"
    raw = open(tmp_path / "out", "rb").read()
    header = b"P6\n%d %d\n255\n" % (W, H)
    ppm = np.frombuffer(raw[len(header):], np.uint8).reshape(H, W, 3)[::-1]  # the PPM's first row is the frame's last
    plane = scene.slice_plane(dims, "axial", (dims[2] - 1) / 2, W, H)
    grey = sr.slice_view(vol, *plane, (W, H), modes=(sr.MAX,), window_cw=(0.0, 4000.0))[0][sr.MAX][0]
    want = ovr.overlay(parts, ovr.plane(*plane, 1), (W, H), 0.5, scene.overlay_palette(20), grey)
    assert np.array_equal(ppm, want[0][..., :3])
    colours = {tuple(c) for c in ppm[(ppm[..., 0] != ppm[..., 1]) | (ppm[..., 1] != ppm[..., 2])].tolist()}
    assert len(colours) >= 2, "two parts, two colours"


# ---- 6. the trace
@pytest.mark.parametrize("connectivity", (6, 26))
def test_trace(gpu_ctx, connectivity):
    ctx = gpu_ctx
    dims = (70, 40, 36)
    weights = g.CHAMFER
    domain, seeds, dist, labels = g.random_case(dims, connectivity, weights, None)
    d_dist, d_labels = ctx.buffer_from(dist), ctx.buffer_from(labels)
    reached = np.argwhere(dist != NONE)
    targets = [reached[np.argmax(dist[dist != NONE])]] + list(reached[:: len(reached) // 7])
    assert len({(x // TILE[0], y // TILE[1], z // TILE[2]) for z, y, x in targets}) >= 5, "targets in different tiles"
    longest = 0
    for z, y, x in targets:
        for with_labels in (None, labels):
            want, complete = g.trace(dist, (x, y, z), connectivity, weights, with_labels)
            assert complete
            for _ in range(2):
                got, n = ctx.geodesic_trace(d_dist, dims, (x, y, z), d_labels if with_labels is not None else None, connectivity, weights)
                assert n == len(want) and got.tolist() == [list(p) for p in want], (x, y, z)
            longest = max(longest, len(want))
            if len(want) > 3:  # a capacity below the count: the true count, the first points, nothing behind them
                buf = ctx.buffer_from(np.full(3 * len(want), PATTERN, np.uint32))
                status, n = ctx.geodesic_trace_raw(d_dist, dims, (x, y, z), None if with_labels is None else d_labels,
                                                   ffi.GEO_26 if connectivity == 26 else 0, weights, buf, 3)
                got = buf.pull()
                assert (status, n) == (0, len(want)) and got[:9].reshape(3, 3).tolist() == [list(p) for p in want[:3]]
                assert (got[9:] == PATTERN).all()
                assert ctx.geodesic_trace_raw(d_dist, dims, (x, y, z), None, ffi.GEO_26 if connectivity == 26 else 0, weights, None, 0) == (0, len(want))
                buf.release()
    assert longest > 20
    z, y, x = np.argwhere(domain & (dist == NONE))[0]
    got, n = ctx.geodesic_trace(d_dist, dims, (x, y, z), None, connectivity, weights)
    assert n == 0 and len(got) == 0
    # a map that clwh_mask_geodesic did not write: the path ends where no direction qualifies
    broken = dist.copy()
    z, y, x = targets[0]
    broken[z, y, x] += 1000  # no neighbour is that far
    d_broken = ctx.buffer_from(broken)
    buf = ctx.buffer_from(np.full(12, PATTERN, np.uint32))
    status, n = ctx.geodesic_trace_raw(d_broken, dims, (x, y, z), None, ffi.GEO_26 if connectivity == 26 else 0, weights, buf, 4)
    assert (status, n) == (INVALID_VALUE, 1) and buf.pull()[:3].tolist() == [x, y, z]
    for m in (buf, d_broken, d_labels, d_dist):
        m.release()


# ---- 7. status
def test_status_codes_and_nothing_written(gpu_ctx):
    ctx = gpu_ctx
    dims = X, Y, Z = (70, 12, 9)
    n, words = X * Y * Z, scene.mask_words_per_row(X) * Y * Z
    fill = lambda k: ctx.buffer_from(np.full(k, PATTERN, np.uint32))
    domain, short_domain = fill(words), fill(words - 1)
    dist, labels, given, short_map, points, short_points = fill(n + 4), fill(n + 4), fill(n), fill(n - 1), fill(30), fill(29)
    as_image = ctx.image([4, 4, n // 16 + 1], 1, np.uint32)
    odd_domain = ctx.wrap(domain.device_ptr + 4, 4 * words - 4)
    odd_map = ctx.wrap(dist.device_ptr + 2, 4 * n)
    seeds = [(1, 2, 3, 4)]
    bad_dims = ((0, 12, 9), (70, 0, 9), (70, 12, 0), (1 << 31, 1, 1), (1 << 16, 1 << 15, 1))
    w6 = lambda *face: (face, (0, 0, 0), 0)  # edge and corner weights are not in use without CLWH_GEO_26
    bad_weights_6 = (w6(0, 1, 1), w6(1, 0, 1), w6(1, 1, 0), w6(65536, 1, 1), w6(1, 1, 1 << 31))
    bad_weights_26 = (((1, 1, 1), (0, 1, 1), 1), ((1, 1, 1), (1, 1, 65536), 1), ((1, 1, 1), (1, 1, 1), 0), ((1, 1, 1), (1, 1, 1), 65536),
                      ((1, 0, 1), (1, 1, 1), 1))

    def geo(**kw):
        args = dict(domain=domain, dims=dims, seeds=seeds, seed_labels=None, flags=0, weights=None, cap=NONE, dist=dist, labels=labels)
        args.update(kw)
        return ctx.mask_geodesic_raw(**args)[0]

    def trace(**kw):
        args = dict(dist=given, dims=dims, target=(1, 2, 3), labels=None, flags=0, weights=None, points=points, capacity=10)
        args.update(kw)
        return ctx.geodesic_trace_raw(**args)[0]

    L = ffi.lib()
    for name, desc in (("clwh_mask_geodesic", ffi.GeodesicDesc()), ("clwh_geodesic_trace", ffi.GeodesicTraceDesc())):
        assert getattr(L, name)(None, C.byref(desc)) == INVALID_VALUE and getattr(L, name)(ctx.h, None) == INVALID_VALUE
    cases = [geo(result=False), trace(result=False)]
    cases += [geo(domain=bad) for bad in (None, as_image, odd_domain)]
    cases += [geo(dist=None, labels=None)]
    for bad in (as_image, odd_map):
        cases += [geo(dist=bad), geo(labels=bad), geo(dist=None, labels=bad), geo(seed_labels=bad, flags=ffi.GEO_FROM_LABELS)]
        cases += [trace(dist=bad), trace(labels=bad), trace(points=bad)]
    cases += [geo(seed_labels=None, flags=ffi.GEO_FROM_LABELS), trace(dist=None), trace(points=None)]
    cases += [geo(flags=8), geo(flags=-1), geo(flags=1 << 16), trace(flags=2), trace(flags=4), trace(flags=-1)]
    for bad in bad_dims:
        cases += [geo(dims=bad), trace(dims=bad)]
    for bad in bad_weights_6:
        cases += [geo(weights=bad[0]), trace(weights=bad[0]), geo(weights=bad[0], flags=ffi.GEO_26)]
    for bad in bad_weights_26:
        cases += [geo(weights=bad, flags=ffi.GEO_26), trace(weights=bad, flags=ffi.GEO_26)]
    cases += [geo(cap=ffi.GEO_CAP_MAX + 1), geo(cap=NONE - 1)]
    cases += [geo(seeds=[(1, 2, 3, 4)] * (ffi.GROW_MAX_SEEDS + 1)), geo(seeds=None), geo(seeds=[]), geo(seeds=None, seed_labels=given)]
    cases += [geo(seeds=[(1, 2, 3, 4), bad]) for bad in ((70, 2, 3, 4), (1, 12, 3, 4), (1, 2, 9, 4), (1, 2, 3, 0))]
    cases += [trace(target=bad) for bad in ((70, 2, 3), (1, 12, 3), (1, 2, 9))]
    assert cases == [INVALID_VALUE] * len(cases), cases
    # n_seeds > 0 with NULL seeds
    d, res = ffi.GeodesicDesc(), ffi.GeodesicResult()
    d.domain, d.dist, d.n_seeds, d.result, d.cap = domain.h, dist.h, 1, C.pointer(res), NONE
    for k in range(3):
        d.dims[k], d.weight_face[k] = dims[k], 1
    assert L.clwh_mask_geodesic(ctx.h, C.byref(d)) == INVALID_VALUE
    sizes = [geo(domain=short_domain), geo(dist=short_map), geo(labels=short_map), geo(seed_labels=short_map, flags=ffi.GEO_FROM_LABELS),
             trace(dist=short_map), trace(labels=short_map), trace(points=short_points)]
    assert sizes == [SIZE_MISMATCH] * len(sizes), sizes
    # INVALID_VALUE before SIZE_MISMATCH
    assert geo(dist=short_map, weights=(0, 1, 1)) == INVALID_VALUE and geo(domain=short_domain, seeds=[(1, 2, 3, 0)]) == INVALID_VALUE
    assert trace(points=short_points, target=(70, 2, 3)) == INVALID_VALUE
    for m in (domain, short_domain, dist, labels, given, short_map, points, short_points):
        assert (m.pull(np.uint32, (m.nbytes // 4,)) == PATTERN).all()  # nothing was written
    # and the same arguments without the defect are accepted, limits included
    assert geo() == 0 and geo(weights=w6(65535, 1, 65535), cap=ffi.GEO_CAP_MAX) == 0 and geo(cap=0, flags=ffi.GEO_DENSE, dist=None) == 0
    assert geo(seed_labels=as_image) == 0, "ignored without the flag"
    assert geo(seeds=None, seed_labels=given, flags=ffi.GEO_FROM_LABELS) == 0
    assert (dist.pull()[n:] == PATTERN).all() and (labels.pull()[n:] == PATTERN).all() and (domain.pull() == PATTERN).all()
    want = g.geodesic(scene.mask_unpack(np.full(words, PATTERN, np.uint32), dims), None, 6, None, None, np.full((Z, Y, X), PATTERN, np.uint32))
    same(dist.pull()[:n].reshape(Z, Y, X), want[0], "the pattern as domain and as labels")
    assert trace(dist=dist, points=short_points, capacity=9) == 0 and trace(dist=dist, points=None, capacity=0) == 0
    for x in (odd_map, odd_domain, as_image, short_points, points, short_map, given, labels, dist, short_domain, domain):
        x.release()
