"""clwh_segment_label and clwh_labels_to_mask restated in numpy (include/clwh.h), on top of tests/grow_ref.py: the admissible image and
the minimum flat index per component come from there; here they become the rank image, the table, the result and the packed
selection.  Ranks: descending voxel count, ties by ascending flat index of the first voxel.  Pure numpy."""
import numpy as np

from cl_volume_renderer_amd import ffi, scene
from tests import grow_ref as gr


def label_admissible(adm, connectivity=6, capacity=None):
    """(ranks uint32 [z][y][x], table (ffi.LABEL_COMPONENT_DTYPE, min(n, capacity) records), {"n_components", "n_voxels"})"""
    Z, Y, X = adm.shape
    lab = gr.labels(adm, connectivity)
    inside = lab >= 0
    first, inverse, count = np.unique(lab[inside], return_inverse=True, return_counts=True)
    order = np.lexsort((first, -count))  # by count descending, then by first ascending
    rank_of = np.empty(len(first), np.int64)
    rank_of[order] = np.arange(1, len(first) + 1)
    ranks = np.zeros(adm.shape, np.uint32)
    ranks[inside] = rank_of[inverse.reshape(-1)]
    n = len(first) if capacity is None else min(len(first), int(capacity))
    table = np.zeros(n, ffi.LABEL_COMPONENT_DTYPE)
    z, y, x = np.nonzero(inside)
    r = ranks[inside].astype(np.int64) - 1
    for axis, c in enumerate((x, y, z)):
        lo = np.full(len(first), np.iinfo(np.int64).max)
        hi = np.zeros(len(first), np.int64)
        np.minimum.at(lo, r, c)
        np.maximum.at(hi, r, c + 1)
        table["bbox_lo"][:, axis] = lo[:n]
        table["bbox_hi"][:, axis] = hi[:n]
    f = first[order][:n]
    table["count"] = count[order][:n]
    table["first"] = np.stack([f % X, f // X % Y, f // (X * Y)], axis=1)
    return ranks, table, {"n_components": len(first), "n_voxels": int(inside.sum())}


def label(vol, lo, hi, connectivity=6, box=None, mask=None, capacity=None):
    """the contract's outputs for a volume; mask: the bool image CLWH_LABEL_FROM_MASK finds in `mask`"""
    adm = gr.admissible(vol, lo, hi, box)
    if mask is not None:
        adm = adm & mask
    return label_admissible(adm, connectivity, capacity)


def selection(ranks, rank_lo, rank_hi):
    """bool [z][y][x] of clwh_labels_to_mask"""
    assert 1 <= rank_lo <= rank_hi
    return (ranks >= rank_lo) & (ranks <= rank_hi)


def packed_selection(ranks, rank_lo, rank_hi):
    return scene.mask_pack(selection(ranks, rank_lo, rank_hi))


# ---- the hand-made volumes the tests share: admissible = 100, everything else 0
def two_serpentines():
    """136 x 40 x 5: grow_ref.serpentine()'s plane at z = 1, its copy reversed in x and y at z = 3: two components of 2739 voxels"""
    plane = gr.serpentine()[1]
    v = np.zeros((5, 40, 136), np.int16)
    v[1] = plane
    v[3] = plane[::-1, ::-1]
    return v


def comb(joined=True):
    """129 x 33 x 18: the even rows of the even planes along all of x, joined by the column x = 128 within a plane and (joined) the
    planes by the line (128, 32, z): one component of 19 890 voxels, or nine"""
    v = np.zeros((18, 33, 129), np.int16)
    v[0::2, 0::2, :] = 100
    v[0::2, :, 128] = 100
    if joined:
        v[:, 32, 128] = 100
    return v


def checkerboard():
    """70 x 19 x 18, (x + y + z) even: 11 970 single voxels under 6-connectivity, one component under 26"""
    z, y, x = np.indices((18, 19, 70))
    return np.where((x + y + z) % 2 == 0, 100, 0).astype(np.int16)


def contact(a, b, dims=(130, 33, 33)):
    v = np.zeros(dims[::-1], np.int16)
    v[a[2], a[1], a[0]] = v[b[2], b[1], b[0]] = 100
    return v
