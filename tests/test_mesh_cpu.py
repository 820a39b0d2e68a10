"""CPU checks of the mesh contract's restatement (tests/mesh_ref.py) and of what sits above the C ABI: the reference's meshes are
closed, consistently oriented surfaces of the right size and genus, ties included; w stays in range; the brick-skipping rule loses
no crossing; BELOW mirrors the plain mesh; the PLY files round-trip."""
import os

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import mesh_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ffi_names_the_values_of_the_header():
    assert (ffi.MESH_DENSE, ffi.MESH_BELOW) == (ffi.ISO_DENSE, ffi.ISO_BELOW) == (1, 2)
    assert "clwh_mesh_isosurface" in ffi.EXPORTED_SYMBOLS
    d = ffi.MeshDesc()
    assert (d.iso, d.flags, len(d.box_lo), len(d.box_hi), d.vertex_capacity, d.triangle_capacity) == (0.0, 0, 3, 3, 0, 0)
    header = open(os.path.join(ROOT, "include", "clwh.h")).read()
    assert "CLWH_MESH_DENSE = 1," in header and "CLWH_MESH_BELOW = 2 " in header
    assert "int clwh_mesh_isosurface(clwh_ctx *ctx, const clwh_mesh_desc *desc);" in header


def _closed(m, chi=None):
    ok, v, e, f = mr.topology(m.tris)
    assert ok  # every directed edge once, its reverse once
    assert v == len(m.keys)  # every vertex is used
    if chi is not None:
        assert v - e + f == chi
    return v, e, f


def test_sphere_is_a_closed_oriented_surface_of_the_analytic_volume():
    m = mr.mesh(mr.sphere(), 100.0)
    assert (len(m.keys), len(m.tris)) == (2016, 4028)
    _closed(m, chi=2)
    vol = mr.signed_volume(m.positions(), mr.index_triangles(m))
    analytic = 4.0 / 3.0 * np.pi * 6.0 ** 3  # 1000 - 150 r = 100 at r = 6
    assert vol > 0 and abs(vol - analytic) < 0.03 * analytic, vol
    # the normals point outwards: away from the centre
    out = m.positions() - np.array([9.3 + 0.5, 9.7 + 0.5, 10.1 + 0.5], np.float32)
    assert ((out * m.nrm.view(np.float32)).sum(1) > 0).all()


def test_noisy_sphere_is_closed_and_oriented():
    m = mr.mesh(mr.noisy_sphere(), 100.0)
    _closed(m)
    assert len(m.tris) > 4028


@pytest.mark.parametrize("iso,ties", [(0.0, True), (0.5, False)])
def test_small_integer_volume_with_ties_is_closed_and_oriented(iso, ties):
    m = mr.mesh(mr.ties(), iso)
    _closed(m)
    n_deg = mr.degenerate(m.pos, mr.index_triangles(m))
    assert (n_deg > 100) == ties
    assert ((m.w == 0).any() or (m.w == 65536).any()) == ties
    assert (m.cases[:, 1:15] > 0).all()  # every tetrahedron shows each of its 14 non-trivial cases


@pytest.mark.parametrize("below", [False, True])
@pytest.mark.parametrize("iso", [0.0, 0.5, -3.0, 2.25])
def test_w_stays_in_range_and_the_position_on_its_edge(iso, below):
    m = mr.mesh(mr.ties(3), iso, below=below)
    assert len(m.keys) > 0 and (m.w >= 0).all() and (m.w <= 65536).all()
    P, d = mr.split_key(m.keys, m.dims)
    off = m.positions().astype(np.float64) - (P + 0.5)
    step = np.stack([d & 1, (d >> 1) & 1, d >> 2], axis=1)
    assert np.array_equal(off, step * (m.w[:, None] / 65536.0))  # exact at this size


@pytest.mark.parametrize("below", [False, True])
def test_no_crossing_edge_is_owned_by_a_rejected_brick(below):
    rng = np.random.default_rng(11)
    V = np.full((20, 27, 33), -800, np.int16)
    V[3:9, 10:20, 7:30] = rng.integers(-900, 900, (6, 10, 23))
    V[17, 26, 32] = 900  # a corner voxel: its crossings are owned by the neighbours' bricks too
    V[8, 8, 8] = 500
    for iso in (0.0, 499.5, 500.0, -800.0, 900.0):
        m = mr.mesh(V, iso, below=below)
        T = m.T
        dmin, dmax = mr.dilated_pairs(V)
        visited = ((dmin << 24) <= T) & (T < (dmax << 24)) if below else ((dmin << 24) < T) & (T <= (dmax << 24))
        assert (~visited).any()
        P, _ = mr.split_key(m.keys, m.dims)
        assert visited[P[:, 2] >> 3, P[:, 1] >> 3, P[:, 0] >> 3].all()
        # and no cell with a triangle has its origin in a rejected brick (its corners lie within one voxel of the brick)
        inside = ((V.astype(np.int64) << 24) <= T) if below else ((V.astype(np.int64) << 24) >= T)
        corners = [inside[(k >> 2):inside.shape[0] - 1 + (k >> 2), ((k >> 1) & 1):inside.shape[1] - 1 + ((k >> 1) & 1), (k & 1):inside.shape[2] - 1 + (k & 1)]
                   for k in range(8)]
        n_in = sum(c.astype(np.int64) for c in corners)
        at = np.argwhere((n_in > 0) & (n_in < 8))
        assert visited[at[:, 0] >> 3, at[:, 1] >> 3, at[:, 2] >> 3].all()


@pytest.mark.parametrize("iso", [0.0, 1.0, -2.5])
def test_below_is_the_plain_mesh_of_the_negated_volume(iso):
    V = mr.ties(9)
    assert float(np.float32(iso)) * 16777216.0 == int(float(np.float32(iso)) * 16777216.0)
    a, b = mr.mesh(V, iso, below=True), mr.mesh((-V).astype(np.int16), -iso)
    assert len(a.keys) > 0 and np.array_equal(a.keys, b.keys)
    assert np.array_equal(a.pos, b.pos) and np.array_equal(a.w, b.w)
    assert np.array_equal(mr.canonical(a.tris), mr.canonical(b.tris))  # same triangles, winding kept
    # g(-V) = -g(V) and the sign of the normal flips with the mode: the same normals (up to the sign of a zero)
    assert np.array_equal(a.nrm.view(np.float32), b.nrm.view(np.float32))


def test_box_mesh_is_the_sub_mesh_of_the_whole():
    V = mr.noisy_sphere()
    whole = mr.mesh(V, 100.0)
    part = mr.mesh(V, 100.0, box=((3, 5, 2), (13, 11, 17)))
    assert 0 < len(part.keys) < len(whole.keys)
    pos, nrm = mr.restrict(whole, part.keys)
    assert np.array_equal(pos, part.pos) and np.array_equal(nrm, part.nrm)
    canon = {tuple(t) for t in mr.canonical(whole.tris).tolist()}
    assert all(tuple(t) in canon for t in mr.canonical(part.tris).tolist())
    assert len(mr.mesh(V, 100.0, box=((3, 5, 2), (13, 5, 17))).keys) == 0  # lo == hi on one axis


def test_ply_round_trip(tmp_path):
    m = mr.mesh(mr.sphere(), 100.0)
    tri = mr.index_triangles(m).astype(np.uint32)
    path = str(tmp_path / "s.ply")
    scene.write_ply(path, m.positions(), m.nrm.view(np.float32), tri)
    raw = open(path, "rb").read()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 2016\n")
    assert len(raw) == raw.index(b"end_header\n") + 11 + 2016 * 24 + 4028 * 13
    pos, nrm, t = scene.read_ply(path)
    assert pos.dtype == np.float32 and t.dtype == np.uint32
    assert np.array_equal(pos.view(np.uint32), m.pos) and np.array_equal(nrm.view(np.uint32), m.nrm) and np.array_equal(t, tri)
    scene.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    pos, nrm, t = scene.read_ply(path)
    assert pos.shape == (0, 3) and nrm.shape == (0, 3) and t.shape == (0, 3)
    open(path, "wb").write(raw[:-1])
    with pytest.raises(ValueError):
        scene.read_ply(path)
