"""The contract of clwh_mask_thin and clwh_mask_points (include/clwh.h) restated in numpy and Python, taken literally: the 26
neighbours as a 26-bit word in the order of OFFSETS, the two adjacency tables, the fill of the lowest set bit, the candidates fixed
per iteration and the eight sub-passes by parity.  Beside it the classical definition of a simple voxel (parts, cavities, Euler
number) that pins the bit test, the voxel list, and a walk of the skeleton that does not share scene.skeleton_graph's code."""
import numpy as np

OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
N6 = sum(1 << i for i, o in enumerate(OFFSETS) if sum(map(abs, o)) == 1)
N18 = sum(1 << i for i, o in enumerate(OFFSETS) if sum(map(abs, o)) <= 2)
# position i's neighbours among the 26 (largest coordinate difference 1), and among the 18 under 6-adjacency (summed difference 1)
ADJ26 = [sum(1 << j for j, b in enumerate(OFFSETS) if i != j and max(abs(a[k] - b[k]) for k in range(3)) <= 1) for i, a in enumerate(OFFSETS)]
ADJ6_18 = [sum(1 << j for j, b in enumerate(OFFSETS) if (N18 >> i) & (N18 >> j) & 1 and sum(abs(a[k] - b[k]) for k in range(3)) == 1)
           for i, a in enumerate(OFFSETS)]
KEEP_ENDS, DENSE = 1, 2


def fill(seed, allowed, adj):
    """the component of `allowed` that holds `seed`, for arrays of words: at most 26 expansions"""
    g = seed.copy()
    for _ in range(26):
        n = g.copy()
        for i in range(26):
            n |= np.where((g >> i) & 1 == 1, np.int64(adj[i]), np.int64(0))
        n &= allowed
        if np.array_equal(n, g):
            break
        g = n
    return g


def simple(nb):
    """bool per word of the int64 array nb"""
    nb = np.asarray(nb, dtype=np.int64)
    one = fill(nb & -nb, nb, ADJ26) == nb
    clear = ~nb & N18
    faces = clear & N6
    return (nb != 0) & one & (faces != 0) & ((fill(faces & -faces, clear, ADJ6_18) & N6) == faces)


def fill_word(seed, allowed, adj):
    """fill for one Python integer"""
    g = seed
    for _ in range(26):
        n = g
        for i in range(26):
            if (g >> i) & 1:
                n |= adj[i]
        n &= allowed
        if n == g:
            break
        g = n
    return g


def simple_word(nb):
    """simple for one Python integer"""
    if nb == 0 or fill_word(nb & -nb, nb, ADJ26) != nb:
        return False
    clear = ~nb & N18
    faces = clear & N6
    return faces != 0 and (fill_word(faces & -faces, clear, ADJ6_18) & N6) == faces


def word_at(M, z, y, x):
    """the 26 neighbours of one voxel as a Python integer"""
    Z, Y, X = M.shape
    return sum(1 << i for i, (dx, dy, dz) in enumerate(OFFSETS)
               if 0 <= x + dx < X and 0 <= y + dy < Y and 0 <= z + dz < Z and M[z + dz, y + dy, x + dx])


def neighbour_words(M):
    """int64 [z][y][x]: bit i = the neighbour at OFFSETS[i] is set; outside the volume is clear"""
    P = np.pad(np.asarray(M, dtype=bool), 1)
    Z, Y, X = M.shape
    nb = np.zeros(M.shape, np.int64)
    for i, (dx, dy, dz) in enumerate(OFFSETS):
        nb |= P[1 + dz:1 + dz + Z, 1 + dy:1 + dy + Y, 1 + dx:1 + dx + X].astype(np.int64) << i
    return nb


def count26(M):
    nb = neighbour_words(M)
    return sum((nb >> i) & 1 for i in range(26))


def parity(shape):
    z, y, x = np.indices(shape)
    return (x & 1) | (y & 1) << 1 | (z & 1) << 2


def candidates(M, keep_ends=False, anchors=None):
    """C = B \\ E \\ anchors on M as it stands"""
    nb = neighbour_words(M)
    C = M & ((nb & N6) != N6)
    if keep_ends:
        C &= count26(M) != 1
    if anchors is not None:
        C &= ~anchors
    return C


def subpass(M, C, s, par):
    """the voxels sub-pass s deletes from M"""
    at = np.nonzero(C & M & (par == s))
    gone = np.zeros(M.shape, bool)
    if len(at[0]):
        gone[at] = simple(neighbour_words(M)[at])
    return gone


def thin(M, flags=0, anchors=None, max_iterations=0, snapshots=()):
    """(mask, result dict); snapshots: iteration numbers whose (mask, result) are also wanted, as a dict beside"""
    M = np.asarray(M, dtype=bool).copy()
    count_in, par, kept = int(M.sum()), parity(M.shape), {}
    iterations = deleted = 0
    while True:
        iterations += 1
        C = candidates(M, bool(flags & KEEP_ENDS), anchors)
        before = deleted
        for s in range(8):
            gone = subpass(M, C, s, par)
            M &= ~gone
            deleted += int(gone.sum())
        done = deleted == before or iterations == max_iterations
        result = {"count_in": count_in, "count_out": count_in - deleted, "deleted": deleted, "iterations": iterations}
        if iterations in snapshots:
            kept[iterations] = (M.copy(), result)
        if done:
            for k in snapshots:  # a limit the thinning never reached gives the final answer
                kept.setdefault(k, (M, result))
            return (M, result, kept) if snapshots else (M, result)


# ---- the classical definition: deleting the centre keeps the parts, the cavities and the Euler number
def _labels(A, connectivity):
    """the number of components of the bool image A"""
    from tests import grow_ref

    lab = grow_ref.labels(A, connectivity)
    return len(np.unique(lab[lab >= 0]))


def euler(M):
    """of the union of the closed unit cubes of M: vertices - edges + faces - cubes"""
    P = np.pad(np.asarray(M, dtype=bool), 1)

    def cells(axes):  # a cell exists if a cube that touches it does
        A = P
        for ax in axes:
            A = A | np.roll(A, 1, ax)
        return int(A.sum())

    return cells((0, 1, 2)) - sum(cells(t) for t in ((0, 1), (0, 2), (1, 2))) + sum(cells((a,)) for a in range(3)) - cells(())


def invariants(M):
    """(26-components, 6-components of the zero-padded complement, Euler number)"""
    P = np.pad(np.asarray(M, dtype=bool), 1)
    return _labels(P, 26), _labels(~P, 6), euler(M)


# ---- the voxel list
def points(M, sampled=None):
    """uint32 [n][4] = x, y, z, n26 in ascending flat index, and the map's words there"""
    z, y, x = np.nonzero(M)  # (row-major: ascending (z * Y + y) * X + x)
    n26 = count26(M)[z, y, x]
    rows = np.stack([x, y, z, n26], axis=1).astype(np.uint32)
    return rows, (None if sampled is None else np.asarray(sampled)[z, y, x].astype(np.uint32))


# ---- the skeleton's structure, counted without building the graph
def structure(M):
    """{"ends", "junction_voxels", "isolated", "loops"}: voxels by n26, and the rings of n26 == 2 voxels that touch no other voxel"""
    n = count26(M)
    chain = M & (n == 2)
    loops = 0
    if chain.any():
        from tests import grow_ref

        lab = grow_ref.labels(chain, 26)
        touching = set(np.unique(lab[chain & (count26(M & ~chain) > 0)]).tolist())
        loops = len(set(np.unique(lab[chain]).tolist()) - touching)
    return {"ends": int((M & (n == 1)).sum()), "junction_voxels": int((M & (n >= 3)).sum()), "isolated": int((M & (n == 0)).sum()),
            "loops": loops}

