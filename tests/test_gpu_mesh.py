"""clwh_mesh_isosurface on the GPU against the contract's numpy restatement (tests/mesh_ref.py), bit for bit.  The output order is
free, so every comparison goes through the canonical form: vertices by key, triangles as key triples rotated to their smallest key
and sorted.  Every family keeps a tally so that no comparison is empty."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import isosurface_ref as ir
from tests import mesh_ref as mr
from tests.view_helpers import ROOT, host_lib

pytestmark = pytest.mark.gpu

INVALID_VALUE, OUT_OF_MEMORY, SIZE_MISMATCH = 1, 3, 9
DENSE, BELOW = ffi.MESH_DENSE, ffi.MESH_BELOW


class Tally:
    def __init__(self):
        self.dirs = np.zeros(8, np.int64)
        self.cases = np.zeros((6, 16), np.int64)
        self.w0 = self.w1 = self.flat_normal = self.clamped = self.split_edge = self.three_bricks = 0
        self.vertices = self.triangles = self.meshes = self.empty = 0

    def add(self, m: mr.Mesh):
        self.meshes += 1
        self.empty += len(m.keys) == 0
        self.vertices += len(m.keys)
        self.triangles += len(m.tris)
        self.cases += m.cases
        if len(m.keys) == 0:
            return
        P, d = mr.split_key(m.keys, m.dims)
        Q = P + np.stack([d & 1, (d >> 1) & 1, d >> 2], axis=1)
        self.dirs += np.bincount(d, minlength=8)
        self.w0 += int((m.w == 0).sum())
        self.w1 += int((m.w == 65536).sum())
        self.flat_normal += int((m.nrm.view(np.float32) == 0).all(1).sum())
        top = np.array(m.dims) - 1
        self.clamped += int(((P == 0) | (Q == top)).any(1).sum())  # an end on a face of the volume: a neighbour is clamped
        self.split_edge += int(((P >> 3) != (Q >> 3)).any(1).sum())
        Pt, _ = mr.split_key(m.tris.reshape(-1), m.dims)
        nb = (np.array(m.dims) + 7) // 8
        brick = (((Pt[:, 2] >> 3) * nb[1] + (Pt[:, 1] >> 3)) * nb[0] + (Pt[:, 0] >> 3)).reshape(-1, 3)
        self.three_bricks += int(((brick[:, 0] != brick[:, 1]) & (brick[:, 1] != brick[:, 2]) & (brick[:, 0] != brick[:, 2])).sum())

    def complete(self):
        return ((self.dirs[1:] > 0).all() and (self.cases[:, 1:15] > 0).all() and self.w0 > 0 and self.w1 > 0 and self.flat_normal > 0 and
                self.clamped > 0 and self.split_edge > 0 and self.three_bricks > 0)


def run(ctx, volume, iso, flags=0, box=None):
    """(keys, position bits, normal bits, index triples) as the device wrote them"""
    pos, nrm, tri, keys = ctx.mesh_isosurface(volume, iso, flags=flags, box=box, normals=True, keys=True)
    return keys, pos.view(np.uint32), nrm.view(np.uint32), tri


def check(got, want: mr.Mesh, what=""):
    keys, pos, nrm, tri = got
    assert len(keys) == len(want.keys) and len(tri) == len(want.tris), (what, len(keys), len(want.keys), len(tri), len(want.tris))
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(keys[order], want.keys), what  # (the reference's keys are distinct and ascending)
    assert np.array_equal(pos[order], want.pos), what
    assert np.array_equal(nrm[order], want.nrm), what
    if len(tri):
        assert int(tri.max()) < len(keys), what
        assert np.array_equal(mr.canonical(keys[tri]), mr.canonical(want.tris)), what
        assert len(np.unique(tri)) == len(keys), what  # every vertex is used


def same_bytes(a, b, what=""):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what


def _random(dims, seed, lo=-300, hi=300):
    X, Y, Z = dims
    return np.random.default_rng(seed).integers(lo, hi + 1, (Z, Y, X)).astype(np.int16)


def _spike():
    v = np.zeros((7, 5, 6), np.int16)
    v[3, 2, 2] = 100  # the central differences vanish at the spike and at its diagonal neighbours: normals (0, 0, 0)
    return v


# (volume [z][y][x], iso values)
SMALL = {
    "one brick 8x8x8": (_random((8, 8, 8), 1), (0.0, 45.5)),
    "9x9x9": (_random((9, 9, 9), 2), (0.0, 45.5)),
    "ragged 19x13x11": (_random((19, 13, 11), 3), (0.0, -120.25)),
    "2x2x2": (_random((2, 2, 2), 4), (0.0, 10.0)),
    "17x2x9": (_random((17, 2, 9), 5), (0.0, 45.5)),
    "axis of one": (_random((5, 1, 4), 6), (0.0,)),
    "ties": (mr.ties(), (0.0, 0.5)),
    "ties 25x9x10": (_random((25, 9, 10), 8, -2, 2), (0.0, 1.0)),
    "noisy sphere": (mr.noisy_sphere(), (100.0,)),
    "spike": (_spike(), (50.0, 100.0)),
}


def _family(ctx, volumes):
    """reference == skipping == dense (byte for byte, order included), plain and BELOW; returns the tally"""
    tally = Tally()
    for name, (vol, isos) in volumes.items():
        volume = ctx.image_from(vol)
        for iso in isos:
            for below in (0, BELOW):
                want = mr.mesh(vol, iso, below=bool(below))
                got = run(ctx, volume, iso, flags=below)
                check(got, want, (name, iso, below, "skipping"))
                same_bytes(run(ctx, volume, iso, flags=below | DENSE), got, (name, iso, below, "dense"))
                tally.add(want)
        volume.release()
    return tally


def test_small_volumes_equal_the_reference_skipping_and_dense(gpu_ctx):
    tally = _family(gpu_ctx, SMALL)
    assert tally.complete(), vars(tally)
    assert tally.empty >= 2 and tally.meshes == 2 * sum(len(isos) for _, isos in SMALL.values())  # (the axis of one: no cell)


def test_phantom_equals_the_reference_skipping_and_dense(gpu_ctx):
    tally = _family(gpu_ctx, {"phantom": (scene.phantom(64), (300.0, -200.0))})
    assert tally.vertices > 100000 and tally.triangles > 200000 and (tally.dirs[1:] > 1000).all() and tally.split_edge > 1000
    assert tally.three_bricks > 0 and (tally.cases[:, 1:15] > 0).all(), vars(tally)


def test_boxes(gpu_ctx):
    ctx = gpu_ctx
    vol, _ = SMALL["ragged 19x13x11"]
    volume = ctx.image_from(vol)
    n = 0
    for below in (0, BELOW):
        whole = run(ctx, volume, 0.0, flags=below)
        index = {int(k): i for i, k in enumerate(whole[0])}
        whole_tris = {tuple(t) for t in mr.canonical(whole[0][whole[3]]).tolist()}
        for box, empty in ((((3, 2, 1), (17, 11, 9)), False),  # unaligned to the bricks
                           (((0, 0, 4), (18, 12, 5)), False),  # one cell thick
                           (((9, 1, 8), (10, 2, 9)), False),   # one cell, across a brick boundary
                           (((2, 3, 4), (10, 3, 9)), True),    # lo == hi on one axis
                           (((0, 0, 0), (0, 0, 0)), False)):   # hi all zero: the whole volume
            want = mr.mesh(vol, 0.0, below=bool(below), box=box)
            assert (len(want.keys) == 0) == empty
            got = run(ctx, volume, 0.0, flags=below, box=box)
            check(got, want, (box, below))
            same_bytes(run(ctx, volume, 0.0, flags=below | DENSE, box=box), got, (box, below, "dense"))
            # the mesh of a box is the sub-mesh of the whole: same bits for the shared keys, and its triangles are the whole's
            at = np.array([index[int(k)] for k in got[0]], np.int64)
            assert np.array_equal(whole[1][at], got[1]) and np.array_equal(whole[2][at], got[2])
            assert all(tuple(t) in whole_tris for t in mr.canonical(got[0][got[3]]).tolist())
            n += len(got[0])
    assert n > 1000
    volume.release()


def test_watertight_on_the_device(gpu_ctx):
    """closed, consistently oriented, with the reference's Euler characteristic -- from the device's own arrays"""
    ctx = gpu_ctx
    degenerate = 0
    for vol, iso, chi in ((mr.sphere(), 100.0, 2), (mr.noisy_sphere(), 100.0, None), (mr.ties(), 0.0, None), (mr.ties(), 0.5, None)):
        volume = ctx.image_from(vol)
        keys, pos, nrm, tri = run(ctx, volume, iso)
        ok, v, e, f = mr.topology(tri)
        assert ok and v == len(keys) and f == len(tri)
        rv, re_, rf = mr.topology(mr.mesh(vol, iso).tris)[1:]
        assert (v, e, f) == (rv, re_, rf)
        if chi is not None:
            assert v - e + f == chi and (v, f) == (2016, 4028)
            volume_of = mr.signed_volume(pos.view(np.float32), tri)
            analytic = 4.0 / 3.0 * np.pi * 6.0 ** 3
            assert volume_of > 0 and abs(volume_of - analytic) < 0.03 * analytic
        degenerate += mr.degenerate(pos, tri)
        volume.release()
    assert degenerate > 100  # the ties: triangles with coinciding positions are kept


def test_vertices_lie_on_the_isosurface_of_the_renderers_field(gpu_ctx):
    """For a vertex on an axis-aligned edge P -> Q = P + e_c the trilinear field S of clwh_render_isosurface at the vertex position is
    linear between A(P) and A(Q): S(pos) = A(P) + t8 * (A(Q) - A(P)), t8 the renderer's 8-bit weight / 256.  The bound on |S - T|:
      * T = A(P) + t * (A(Q) - A(P)) with the exact t in [0, 1];
      * w = floor(t * 2^16): w / 2^16 in (t - 2^-16, t];
      * F = P.c * 65536 + 32768 + w < 2^24 for dims <= 255 (asserted), so (float)F is exact, the scaling by 2^-16 is exact, and so are
        the renderer's q = pos - 0.5f and q - floorf(q): the float32 rounding of pos contributes 0 here;
      * the renderer's weight is floor(frac * 256) with frac = w / 2^16 exactly: t8 in (w / 2^16 - 2^-8, w / 2^16]; for w = 65536 the
        position is Q itself and S = A(Q) (t8 = 1 = w / 2^16).
    Hence t - 2^-16 - 2^-8 < t8 <= t and |S - T| < (2^-8 + 2^-16) * |A(Q) - A(P)|, S never beyond T as seen from P."""
    ctx = gpu_ctx
    vol = scene.phantom(64)
    assert max(vol.shape) <= 255
    volume = ctx.image_from(vol)
    n = 0
    for iso, below in ((300.0, 0), (-200.0, 0), (300.0, BELOW)):
        keys, pos, _, _ = run(ctx, volume, iso, flags=below)
        P, d = mr.split_key(keys, vol.shape[::-1])
        axial = (d == 1) | (d == 2) | (d == 4)
        P, d, p = P[axial], d[axial], pos.view(np.float32)[axial]
        Q = P + np.stack([d & 1, (d >> 1) & 1, d >> 2], axis=1)
        AP = vol[P[:, 2], P[:, 1], P[:, 0]].astype(np.int64) << 24
        AQ = vol[Q[:, 2], Q[:, 1], Q[:, 0]].astype(np.int64) << 24
        S, T = ir.field_at(vol, p), mr.threshold(iso)
        assert (np.abs(S - T) * 65536 < 257 * np.abs(AQ - AP)).all()
        assert (((S - T) * (AQ - AP) <= 0)).all()  # on P's side of T, or on it
        n += int(axial.sum())
    assert n > 30000
    volume.release()


def test_counts_and_capacities(gpu_ctx):
    ctx = gpu_ctx
    vol = mr.noisy_sphere()
    volume = ctx.image_from(vol)
    want = mr.mesh(vol, 100.0)
    nv, nt = len(want.keys), len(want.tris)
    assert ctx.mesh_isosurface_raw(volume, 100.0) == (0, nv, nt)  # counting only
    assert ctx.mesh_isosurface_raw(volume, 100.0, flags=DENSE) == (0, nv, nt)
    pattern = np.full(nv * 3 + 6, 0xA5A5A5A5, np.uint32)
    bufs = [ctx.buffer_from(pattern) for _ in range(3)] + [ctx.buffer_from(np.full(nt * 3 + 6, 0xA5A5A5A5, np.uint32))]
    keys = ctx.buffer_from(np.full(nv + 2, 0xA5A5A5A5A5A5A5A5, np.uint64))

    def untouched():
        return all((b.pull() == 0xA5A5A5A5).all() for b in bufs) and (keys.pull() == 0xA5A5A5A5A5A5A5A5).all()

    for cap_v, cap_t in ((nv - 1, nt), (nv, nt - 1), (0, 0), (1, 1)):
        got = ctx.mesh_isosurface_raw(volume, 100.0, positions=bufs[0], normals=bufs[1], keys=keys, triangles=bufs[3],
                                      vertex_capacity=cap_v, triangle_capacity=cap_t)
        assert got == (SIZE_MISMATCH, nv, nt) and untouched(), (cap_v, cap_t)
    # exactly enough, and more than enough: filled up to the counts and not past them
    for cap_v, cap_t in ((nv, nt), (nv + 2, nt + 2)):
        got = ctx.mesh_isosurface_raw(volume, 100.0, positions=bufs[0], normals=bufs[1], keys=keys, triangles=bufs[3],
                                      vertex_capacity=cap_v, triangle_capacity=cap_t)
        assert got == (0, nv, nt)
        k = keys.pull()
        out = (k[:nv], bufs[0].pull()[:nv * 3].reshape(nv, 3), bufs[1].pull()[:nv * 3].reshape(nv, 3), bufs[3].pull()[:nt * 3].reshape(nt, 3))
        check(out, want, "filled")
        assert (k[nv:] == 0xA5A5A5A5A5A5A5A5).all() and all((b.pull()[n * 3:] == 0xA5A5A5A5).all() for b, n in ((bufs[0], nv), (bufs[1], nv), (bufs[3], nt)))
    # positions and triangles alone
    assert ctx.mesh_isosurface_raw(volume, 100.0, positions=bufs[0], triangles=bufs[3], vertex_capacity=nv, triangle_capacity=nt) == (0, nv, nt)
    assert np.array_equal(bufs[0].pull()[:nv * 3], out[1].reshape(-1)) and np.array_equal(bufs[3].pull()[:nt * 3], out[3].reshape(-1))
    for b in bufs + [keys, volume]:
        b.release()
    # nothing crosses: all inside, all outside
    flat = ctx.image_from(np.full((9, 10, 11), 7, np.int16))
    for iso, flags in ((7.0, 0), (7.5, 0), (-100.0, 0), (7.0, BELOW), (6.5, BELOW), (100.0, BELOW), (7.0, DENSE), (7.5, DENSE | BELOW)):
        assert ctx.mesh_isosurface_raw(flat, iso, flags=flags) == (0, 0, 0)
    pos, nrm, tri, k = ctx.mesh_isosurface(flat, 7.0, keys=True)
    assert pos.shape == (0, 3) and nrm.shape == (0, 3) and tri.shape == (0, 3) and k.shape == (0,)
    flat.release()


def test_determinism_and_derived_data(gpu_ctx):
    ctx = gpu_ctx
    a = scene.phantom(40, dims=(24, 16, 40))
    b = np.where(a < -500, 900, -1000).astype(np.int16)  # a's air becomes dense: a stale dilated table skips the bricks that now cross
    volume = ctx.image_from(a)
    ctx.invalidate_derived(scene=False, camera=False, projection=True)
    n = 0

    def follows(vol, what, through=None):
        nonlocal n
        for flags in (0, BELOW):
            want = mr.mesh(vol, 300.0, below=bool(flags))
            got = run(ctx, through or volume, 300.0, flags=flags)
            check(got, want, what)
            same_bytes(run(ctx, through or volume, 300.0, flags=flags), got, what + ": again")
            same_bytes(run(ctx, through or volume, 300.0, flags=flags | DENSE), got, what + ": dense")
            n += len(want.keys)

    follows(a, "first")
    volume.push(b)
    follows(b, "after a push")
    alias = ctx.image_wrap(volume.device_ptr, (24, 16, 40), 1, np.int16)
    alias.push(a)
    follows(a, "after a push through a wrap")
    follows(a, "through the wrap", through=alias)
    ctx.invalidate_derived(scene=False, camera=False, projection=True)
    follows(a, "after invalidate")
    # an isosurface render between two extractions shares the copy and the dilated table and changes nothing
    frame = ctx.image([64, 48], 4, np.uint8, (48, 64, 4))
    pos, d = scene.default_camera(40)
    ctx.render_isosurface(frame, volume, pos, d, 64, 48, 300.0)
    follows(a, "after a render")
    ctx.finish()
    for m in (frame, alias, volume):
        m.release()
    assert n > 10000


def test_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    vol = _random((12, 10, 9), 21)
    want = mr.mesh(vol, 0.0)
    nv, nt = len(want.keys), len(want.tris)
    volume = ctx.image_from(vol)
    pos, nrm, tri = (ctx.buffer(nv * 12, np.uint32), ctx.buffer(nv * 12, np.uint32), ctx.buffer(nt * 12, np.uint32))
    keys = ctx.buffer(nv * 8, np.uint64)
    frame = ctx.image([64, 32], 4, np.uint8, (32, 64, 4))
    short12, short8 = ctx.buffer(nv * 12 - 4, np.uint32), ctx.buffer(nv * 8 - 8, np.uint64)
    short_t = ctx.buffer(nt * 12 - 4, np.uint32)

    def status(**kw):
        args = dict(volume=volume, iso=0.0)
        args.update(kw)
        return ctx.mesh_isosurface_raw(**args)[0]

    full = dict(positions=pos, normals=nrm, keys=keys, triangles=tri, vertex_capacity=nv, triangle_capacity=nt)
    assert status() == 0 and status(flags=3) == 0 and status(**full) == 0
    assert status(iso=65536.0) == 0 and status(iso=-65536.0, flags=BELOW) == 0
    assert status(box=((0, 0, 0), (11, 9, 8))) == 0 and status(box=((11, 9, 8), (11, 9, 8))) == 0 and status(box=((4, 4, 4), (4, 9, 8))) == 0
    # CLWH_ERR_INVALID_VALUE, in the header's order
    L = ffi.lib()
    d = ffi.MeshDesc()
    counts = (C.c_uint64 * 2)(7, 7)
    d.volume = volume.h
    d.n_vertices = C.cast(C.byref(counts, 0), C.POINTER(C.c_uint64))
    d.n_triangles = C.cast(C.byref(counts, 8), C.POINTER(C.c_uint64))
    assert L.clwh_mesh_isosurface(ctx.h, C.byref(d)) == 0 and tuple(counts) == (nv, nt)
    assert L.clwh_mesh_isosurface(None, C.byref(d)) == INVALID_VALUE and L.clwh_mesh_isosurface(ctx.h, None) == INVALID_VALUE
    d.n_vertices = None
    assert L.clwh_mesh_isosurface(ctx.h, C.byref(d)) == INVALID_VALUE
    d.n_vertices, d.n_triangles = d.n_triangles, None
    assert L.clwh_mesh_isosurface(ctx.h, C.byref(d)) == INVALID_VALUE
    assert status(volume=None) == INVALID_VALUE and status(volume=frame) == INVALID_VALUE and status(volume=pos) == INVALID_VALUE
    assert status(flags=4) == INVALID_VALUE and status(flags=-1) == INVALID_VALUE and status(flags=1 << 16) == INVALID_VALUE
    for iso in (float("nan"), float("inf"), float("-inf"), 65536.01, -65537.0, 1e30):
        assert status(iso=iso) == INVALID_VALUE
    for box in (((0, 0, 0), (12, 9, 8)), ((0, 0, 0), (11, 10, 8)), ((0, 0, 0), (11, 9, 9)), ((5, 0, 0), (4, 9, 8)), ((0, 0, 3), (11, 9, 2)),
                ((0, 10, 0), (0, 0, 0)), ((0, 0, 0), (0, 0, 1 << 31))):
        assert status(box=box) == INVALID_VALUE, box
    for name in ("positions", "normals", "keys", "triangles"):
        assert status(**dict(full, **{name: frame})) == INVALID_VALUE and status(**dict(full, **{name: volume})) == INVALID_VALUE
    assert status(**dict(full, positions=None)) == INVALID_VALUE and status(**dict(full, triangles=None)) == INVALID_VALUE
    assert status(normals=nrm) == INVALID_VALUE and status(keys=keys) == INVALID_VALUE
    assert status(vertex_capacity=1) == INVALID_VALUE and status(triangle_capacity=1) == INVALID_VALUE
    huge = ctx.image_wrap(volume.device_ptr, (1 << 31, 1, 1), 1, np.int16)  # never read: refused by its dims
    assert status(volume=huge) == INVALID_VALUE
    # CLWH_ERR_SIZE_MISMATCH: a buffer smaller than its capacity says
    assert status(**dict(full, positions=short12)) == SIZE_MISMATCH and status(**dict(full, normals=short12)) == SIZE_MISMATCH
    assert status(**dict(full, keys=short8)) == SIZE_MISMATCH and status(**dict(full, triangles=short_t)) == SIZE_MISMATCH
    assert status(**dict(full, vertex_capacity=nv + 1)) == SIZE_MISMATCH and status(**dict(full, triangle_capacity=1 << 62)) == SIZE_MISMATCH
    # ... before the capacity rule, and INVALID_VALUE before either
    assert status(**dict(full, positions=short12, vertex_capacity=nv - 1)) == SIZE_MISMATCH
    assert status(**dict(full, positions=short12, flags=8)) == INVALID_VALUE
    assert status(**dict(full, vertex_capacity=nv - 1, triangle_capacity=nt)) == SIZE_MISMATCH
    assert status(**full) == 0
    check((keys.pull(), pos.pull().reshape(nv, 3), nrm.pull().reshape(nv, 3), tri.pull().reshape(nt, 3)), want, "after the errors")
    for m in (huge, short_t, short8, short12, frame, keys, tri, nrm, pos, volume):
        m.release()


def _host_lib():
    return host_lib(clvr_host_extract_mesh=(None, [C.c_void_p, C.c_float, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong),
                                                   C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_float)),
                                                   C.POINTER(C.POINTER(C.c_ulonglong)), C.POINTER(C.POINTER(C.c_uint))]),
                    clvr_host_write_mesh_ply=(C.c_int, [C.c_void_p, C.c_char_p]))


def test_host_mirror_extracts_the_same_mesh(tmp_path):
    n = 64
    vol = scene.phantom(n)
    env = scene.env_map(64, 32)
    L = _host_lib()
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, n, n, n, env.ctypes.data, 64, 32)
        for iso, flags in ((300.0, 0), (-200.0, BELOW), (300.0, DENSE)):
            nv, nt = C.c_ulonglong(0), C.c_ulonglong(0)
            p, q = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
            k, t = C.POINTER(C.c_ulonglong)(), C.POINTER(C.c_uint)()
            L.clvr_host_extract_mesh(h, iso, flags, C.byref(nv), C.byref(nt), C.byref(p), C.byref(q), C.byref(k), C.byref(t))
            want = mr.mesh(vol, iso, below=bool(flags & BELOW))
            assert (nv.value, nt.value) == (len(want.keys), len(want.tris)) and nv.value > 10000
            got = (np.ctypeslib.as_array(k, shape=(nv.value,)).astype(np.uint64), np.ctypeslib.as_array(p, shape=(nv.value, 3)).view(np.uint32).copy(),
                   np.ctypeslib.as_array(q, shape=(nv.value, 3)).view(np.uint32).copy(), np.ctypeslib.as_array(t, shape=(nt.value, 3)).copy())
            check(got, want, ("host", iso, flags))
            # the C++ writer's bytes are scene.write_ply's
            assert L.clvr_host_write_mesh_ply(h, str(tmp_path / "host.ply").encode()) == 1
            scene.write_ply(str(tmp_path / "py.ply"), got[1].view(np.float32), got[2].view(np.float32), got[3])
            assert open(tmp_path / "host.ply", "rb").read() == open(tmp_path / "py.ply", "rb").read()
    finally:
        L.clvr_host_destroy(h)


@pytest.mark.parametrize("option,iso,below", [("--mesh=300", 300.0, False), ("--mesh=-200.5,below", -200.5, True)])
def test_headless_mesh_writes_the_ply(tmp_path, option, iso, below):
    n = 64
    vol = scene.phantom(n)
    scene.write_nrrd(str(tmp_path / "v.nrrd"), vol)
    rng = np.random.default_rng(5)
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(rng.random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    out = subprocess.run([exe, option, str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", "64", "64", str(tmp_path / "m.ply")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want = mr.mesh(vol, iso, below=below)
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["mesh"] == iso and line["below"] == below and (line["vertices"], line["triangles"]) == (len(want.keys), len(want.tris))
    pos, nrm, tri = scene.read_ply(str(tmp_path / "m.ply"))
    assert len(pos) == len(want.keys) > 10000 and len(tri) == len(want.tris)
    # no keys in a PLY: vertices compare as sorted (position, normal) rows, triangles as triples of position ids (edges that tie at a
    # grid point share a position, so the id triples may repeat an id: canonical() handles that)
    rows = lambda p, q: np.sort(np.ascontiguousarray(np.concatenate([p, q], axis=1)).view([("", np.uint32)] * 6).reshape(-1))
    assert np.array_equal(rows(pos.view(np.uint32), nrm.view(np.uint32)), rows(want.pos, want.nrm))
    _, ids = np.unique(np.concatenate([pos.view(np.uint32), want.pos]), axis=0, return_inverse=True)
    ids = ids.reshape(-1)
    mine, theirs = ids[:len(pos)], ids[len(pos):]
    assert np.array_equal(mr.canonical(mine[tri]), mr.canonical(theirs[mr.index_triangles(want)]))
    for other in ("--projection=max", "--composite", "--isosurface=300", "--slice=axial"):
        both = subprocess.run([exe, option, other, str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", "64", "64"],
                              capture_output=True, text=True, timeout=120)
        assert both.returncode == 1  # the mesh excludes the views
    bad = subprocess.run([exe, "--mesh=bone", str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr")], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1
