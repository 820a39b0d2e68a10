"""The contract of clwh_mesh_isosurface (include/clwh.h) restated in numpy / int64: marching tetrahedra on the voxel centres, every
decision an integer comparison.  Written from the contract, not from the kernels: no bricks, no scans, no table of cases -- the
winding is decided here by the contract's own rule (edge midpoints against the centroids), in exact rational arithmetic.

Vectorised over edges and cells per (dir) and per (tetrahedron, case), so 64^3 takes seconds.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

# the six tetrahedra: one per permutation (a, b, c) of the axis bits, lexicographic in (a, b); corners 0, a, a|b, 7
TETS = [(0, a, a | b, 7) for a, b in [(1, 2), (1, 4), (2, 1), (2, 4), (4, 1), (4, 2)]]


def threshold(iso) -> int:
    """T = (int64)floor((double)iso * 2^24) of the float32 the descriptor carries"""
    return int(math.floor(float(np.float32(iso)) * 16777216.0))


def _corner(m):
    return [Fraction(m & 1), Fraction((m >> 1) & 1), Fraction((m >> 2) & 1)]


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def case_triangles(tet: int, case: int):
    """the triangles of tetrahedron `tet` whose corner at position p is inside iff bit p of `case`: a list of triangles, each
    three edges (p, q) between corner positions, in the order the contract emits them"""
    corners = TETS[tet]
    ins = [p for p in range(4) if (case >> p) & 1]
    outs = [p for p in range(4) if not (case >> p) & 1]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        tris = [[(ins[0], outs[0]), (ins[0], outs[1]), (ins[0], outs[2])]]
    elif len(ins) == 3:
        tris = [[(ins[0], outs[0]), (ins[1], outs[0]), (ins[2], outs[0])]]
    else:
        a, b = ins
        c, d = outs
        q = [(a, c), (a, d), (b, d), (b, c)]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    centroid = lambda ps: [sum(_corner(corners[p])[k] for p in ps) / len(ps) for k in range(3)]
    c_in, c_out = centroid(ins), centroid(outs)
    out = []
    for tri in tris:
        m = [[(_corner(corners[e[0]])[k] + _corner(corners[e[1]])[k]) / 2 for k in range(3)] for e in tri]
        n = _cross([m[1][k] - m[0][k] for k in range(3)], [m[2][k] - m[0][k] for k in range(3)])
        s = sum(n[k] * (c_out[k] - c_in[k]) for k in range(3))
        assert s != 0
        out.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
    return out


class Mesh:
    """keys uint64[n] (ascending), w int64[n], pos / nrm uint32[n][3] (the float32 bits), tris uint64[m][3] (key triples in emission
    winding), cases int[6][16] (how many cells showed each tetrahedron case), T"""

    def __init__(self, keys, w, pos, nrm, tris, cases, T, dims):
        self.keys, self.w, self.pos, self.nrm, self.tris, self.cases, self.T, self.dims = keys, w, pos, nrm, tris, cases, T, dims

    @property
    def vertices(self):
        """key -> (position bits, normal bits)"""
        return {int(k): (tuple(int(x) for x in p), tuple(int(x) for x in n)) for k, p, n in zip(self.keys, self.pos, self.nrm)}

    def positions(self):
        return self.pos.view(np.float32)


def split_key(keys, dims):
    """keys -> (P [n][3] as x, y, z, dir [n])"""
    X, Y, Z = dims
    keys = np.asarray(keys, np.uint64)
    d = (keys & np.uint64(7)).astype(np.int64)
    lin = (keys >> np.uint64(3)).astype(np.int64)
    return np.stack([lin % X, (lin // X) % Y, lin // (X * Y)], axis=1), d


def gradients(V):
    """g_c(R) = V(R + e_c) - V(R - e_c), each neighbour coordinate clamped: three int64 arrays [Z][Y][X] for c = x, y, z"""
    A = V.astype(np.int64)
    out = []
    for axis in (2, 1, 0):
        n = A.shape[axis]
        idx = np.arange(n)
        out.append(np.take(A, np.minimum(idx + 1, n - 1), axis=axis) - np.take(A, np.maximum(idx - 1, 0), axis=axis))
    return out


def mesh(V: np.ndarray, iso, below: bool = False, box=None) -> Mesh:
    V = np.asarray(V, np.int16)
    Z, Y, X = V.shape
    dims = (X, Y, Z)
    T = threshold(iso)
    A = V.astype(np.int64) << 24
    inside = (A <= T) if below else (A >= T)
    lo, hi = ((0, 0, 0), (X - 1, Y - 1, Z - 1)) if box is None else (tuple(box[0]), tuple(box[1]))
    if box is not None and tuple(hi) == (0, 0, 0):
        hi = (X - 1, Y - 1, Z - 1)
    assert all(0 <= lo[k] <= hi[k] <= dims[k] - 1 for k in range(3))
    if any(hi[k] == lo[k] for k in range(3)):  # no cell: the empty mesh
        e3 = np.zeros((0, 3), np.uint32)
        return Mesh(np.zeros(0, np.uint64), np.zeros(0, np.int64), e3, e3, np.zeros((0, 3), np.uint64), np.zeros((6, 16), np.int64), T, dims)
    g = gradients(V)

    keys_l, w_l, pos_l, nrm_l = [], [], [], []
    for d in range(1, 8):
        dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
        if hi[0] - dx < lo[0] or hi[1] - dy < lo[1] or hi[2] - dz < lo[2]:
            continue
        sp = (slice(lo[2], hi[2] + 1 - dz), slice(lo[1], hi[1] + 1 - dy), slice(lo[0], hi[0] + 1 - dx))
        sq = (slice(lo[2] + dz, hi[2] + 1), slice(lo[1] + dy, hi[1] + 1), slice(lo[0] + dx, hi[0] + 1))
        at = np.argwhere(inside[sp] != inside[sq])
        if len(at) == 0:
            continue
        pz, py, px = at[:, 0] + lo[2], at[:, 1] + lo[1], at[:, 2] + lo[0]
        qz, qy, qx = pz + dz, py + dy, px + dx
        AP, AQ = A[pz, py, px], A[qz, qy, qx]
        assert (AP != AQ).all()
        w = (np.abs(T - AP) << 16) // np.abs(AQ - AP)
        assert ((w >= 0) & (w <= 65536)).all()
        F = np.stack([px * 65536 + 32768 + dx * w, py * 65536 + 32768 + dy * w, pz * 65536 + 32768 + dz * w], axis=1)
        pos = F.astype(np.float64).astype(np.float32) * np.float32(2.0 ** -16)  # F < 2^53: the float32 conversion is the one rounding
        G = np.stack([(65536 - w) * gc[pz, py, px] + w * gc[qz, qy, qx] for gc in g], axis=1)
        assert (np.abs(G) < 2 ** 34).all()
        gf = G.astype(np.float64).astype(np.float32)
        l2 = (gf[:, 0] * gf[:, 0] + gf[:, 1] * gf[:, 1]) + gf[:, 2] * gf[:, 2]
        assert l2.dtype == np.float32
        with np.errstate(invalid="ignore", divide="ignore"):
            n = (gf if below else -gf) / np.sqrt(l2)[:, None]
        n = np.where((l2 > 0)[:, None], n, np.float32(0.0)).astype(np.float32)
        keys_l.append((((pz * Y + py) * X + px) * 8 + d).astype(np.uint64))
        w_l.append(w)
        pos_l.append(pos.view(np.uint32))
        nrm_l.append(n.view(np.uint32))
    if keys_l:
        keys, w, pos, nrm = np.concatenate(keys_l), np.concatenate(w_l), np.concatenate(pos_l), np.concatenate(nrm_l)
        order = np.argsort(keys)
        keys, w, pos, nrm = keys[order], w[order], pos[order], nrm[order]
    else:
        keys, w = np.zeros(0, np.uint64), np.zeros(0, np.int64)
        pos = nrm = np.zeros((0, 3), np.uint32)

    tris_l = []
    cases = np.zeros((6, 16), np.int64)
    if all(hi[k] > lo[k] for k in range(3)):
        corner_in = [inside[lo[2] + (m >> 2):hi[2] + (m >> 2), lo[1] + ((m >> 1) & 1):hi[1] + ((m >> 1) & 1), lo[0] + (m & 1):hi[0] + (m & 1)]
                     for m in range(8)]
        for t, corners in enumerate(TETS):
            case = sum(corner_in[corners[p]].astype(np.int64) << p for p in range(4))
            cases[t] = np.bincount(case.ravel(), minlength=16)
            for cv in range(1, 15):
                at = np.argwhere(case == cv)
                if len(at) == 0:
                    continue
                cz, cy, cx = at[:, 0] + lo[2], at[:, 1] + lo[1], at[:, 2] + lo[0]
                for tri in case_triangles(t, cv):
                    cols = []
                    for e in tri:
                        m_lo, m_hi = corners[min(e)], corners[max(e)]  # the corners form a chain: the lower position is the lower end
                        d = m_hi ^ m_lo
                        assert (m_lo & m_hi) == m_lo and d != 0
                        px, py, pz = cx + (m_lo & 1), cy + ((m_lo >> 1) & 1), cz + (m_lo >> 2)
                        cols.append((((pz * Y + py) * X + px) * 8 + d).astype(np.uint64))
                    tris_l.append(np.stack(cols, axis=1))
    tris = np.concatenate(tris_l) if tris_l else np.zeros((0, 3), np.uint64)
    return Mesh(keys, w, pos, nrm, tris, cases, T, dims)


# ---------------------------------------------------------------------------------------------
# the canonical form and the checks the tests share


def canonical(tris):
    """key triples -> each rotated so that its smallest key comes first (the winding survives), rows sorted.  (The rotation taken is
    the lexicographically smallest one, which is the same thing for three different keys and still unique when two coincide.)"""
    t = np.asarray(tris, np.uint64).reshape(-1, 3)
    if len(t) == 0:
        return t
    best = t
    for r in (t[:, [1, 2, 0]], t[:, [2, 0, 1]]):
        less = (r[:, 0] < best[:, 0]) | ((r[:, 0] == best[:, 0]) & ((r[:, 1] < best[:, 1]) | ((r[:, 1] == best[:, 1]) & (r[:, 2] < best[:, 2]))))
        best = np.where(less[:, None], r, best)
    return best[np.lexsort((best[:, 2], best[:, 1], best[:, 0]))]


def restrict(m: Mesh, keys):
    """the rows of m for `keys` (all must exist): (pos bits, nrm bits)"""
    at = np.searchsorted(m.keys, keys)
    assert (at < len(m.keys)).all() and (m.keys[at] == keys).all()
    return m.pos[at], m.nrm[at]


def topology(tris):
    """(closed_and_oriented, n_vertices_used, n_edges, n_faces) of key (or index) triples: closed and consistently oriented iff every
    directed edge appears exactly once and its reverse exactly once"""
    t = np.asarray(tris).reshape(-1, 3).astype(np.uint64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    directed, counts = np.unique(e, axis=0, return_counts=True)
    ok = bool((counts == 1).all())
    rev = np.unique(directed[:, ::-1], axis=0)
    ok = ok and len(rev) == len(directed) and bool((rev == directed).all())
    undirected = np.unique(np.sort(e, axis=1), axis=0)
    return ok, len(np.unique(t)), len(undirected), len(t)


def signed_volume(positions, tri_index):
    p = np.asarray(positions, np.float64)
    t = np.asarray(tri_index, np.int64)
    p0, p1, p2 = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return float((p0 * np.cross(p1, p2)).sum() / 6.0)


def degenerate(positions_bits, tri_index):
    """how many triangles have two vertices at one position"""
    p = np.asarray(positions_bits).view(np.float32)
    t = np.asarray(tri_index, np.int64)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return int(((a == b).all(1) | (b == c).all(1) | (a == c).all(1)).sum())


def index_triangles(m: Mesh):
    """m.tris as indices into m.keys"""
    return np.searchsorted(m.keys, m.tris).astype(np.int64)


def dilated_pairs(V):
    """(dmin, dmax) [NBZ][NBY][NBX]: per 8^3 brick the extremes over the brick dilated by one voxel, clamped at the volume's faces"""
    Z, Y, X = V.shape
    nb = [(n + 7) // 8 for n in (Z, Y, X)]
    dmin, dmax = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                box = V[max(bz * 8 - 1, 0):bz * 8 + 9, max(by * 8 - 1, 0):by * 8 + 9, max(bx * 8 - 1, 0):bx * 8 + 9]
                dmin[bz, by, bx], dmax[bz, by, bx] = box.min(), box.max()
    return dmin, dmax


# ---------------------------------------------------------------------------------------------
# the volumes the CPU and the GPU tests share


def sphere(n=20, centre=(9.3, 9.7, 10.1)):
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    r = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return (1000.0 - 150.0 * r).astype(np.int16)  # (truncated towards zero)


def bordered(V, value):
    V = V.copy()
    V[0], V[-1], V[:, 0], V[:, -1], V[:, :, 0], V[:, :, -1] = value, value, value, value, value, value
    return V


def noisy_sphere(seed=5):
    rng = np.random.default_rng(seed)
    return bordered((sphere().astype(np.int64) + rng.integers(-300, 301, (20, 20, 20))).astype(np.int16), -1000)


def ties(seed=7):
    rng = np.random.default_rng(seed)
    return bordered(rng.integers(-3, 4, (11, 10, 9)).astype(np.int16), -5)
