"""clwh_mask_statistics and clwh_label_statistics restated in numpy, straight from the definitions of include/clwh.h: the record of a
bool image over a volume (counts by np.count_nonzero, sums in int64 -- exact under the contract's limits --, faces by comparing shifted
slices), the table of a label image, and the histogram.  Records are rows of scene.REGION_STATS_DTYPE: what the device's bytes are
compared with.  Pure numpy."""
import numpy as np

from cl_volume_renderer_amd import scene

DTYPE = scene.REGION_STATS_DTYPE


def record(vol, region):
    """the record of the bool image `region` [z][y][x] over `vol`, as a DTYPE scalar array of shape ()"""
    region = np.asarray(region, bool)
    assert region.shape == vol.shape
    out = np.zeros((), DTYPE)
    n = int(np.count_nonzero(region))
    if n == 0:
        return out
    z, y, x = np.nonzero(region)
    v = vol[region].astype(np.int64)
    out["count"] = n
    out["sum"] = int(v.sum())
    out["sum_sq"] = int((v * v).sum())
    out["vmin"], out["vmax"] = int(v.min()), int(v.max())
    for c, p in enumerate((x, y, z)):
        p = p.astype(np.int64)
        axis = 2 - c  # of the [z][y][x] array
        out["sum_pos"][c] = int(p.sum())
        out["bbox_lo"][c], out["bbox_hi"][c] = int(p.min()), int(p.max()) + 1
        here, there = [slice(None)] * 3, [slice(None)] * 3
        here[axis], there[axis] = slice(0, -1), slice(1, None)
        out["faces"][c] = int(np.count_nonzero(region[tuple(here)] != region[tuple(there)]))
        out["border_faces"][c] = int(np.count_nonzero(p == 0)) + int(np.count_nonzero(p == vol.shape[axis] - 1))
    return out


def label_records(vol, labels, capacity):
    """record k = the record of {labels == k + 1}, k < capacity: a DTYPE array of `capacity` rows"""
    cap = int(capacity)
    lab = np.asarray(labels).astype(np.int64)
    assert lab.shape == vol.shape
    out = np.zeros(cap, DTYPE)
    ranked = lambda a: (a >= 1) & (a <= cap)
    valid = ranked(lab)
    if not valid.any():
        return out
    k = lab[valid] - 1
    v = vol[valid].astype(np.int64)
    z, y, x = np.nonzero(valid)
    count = np.bincount(k, minlength=cap)
    has = count > 0
    out["count"] = count

    def summed(values):  # exact: int64 additions, not bincount's float weights
        s = np.zeros(cap, np.int64)
        np.add.at(s, k, values)
        return s

    def extreme(values, ufunc, start):
        e = np.full(cap, start, np.int64)
        ufunc.at(e, k, values)
        return np.where(has, e, 0)

    out["sum"], out["sum_sq"] = summed(v), summed(v * v)
    out["vmin"], out["vmax"] = extreme(v, np.minimum, 1 << 40), extreme(v, np.maximum, -(1 << 40))
    for c, p in enumerate((x, y, z)):
        p = p.astype(np.int64)
        axis = 2 - c
        out["sum_pos"][:, c] = summed(p)
        out["bbox_lo"][:, c], out["bbox_hi"][:, c] = extreme(p, np.minimum, 1 << 40), extreme(p + 1, np.maximum, 0)
        here, there = [slice(None)] * 3, [slice(None)] * 3
        here[axis], there[axis] = slice(0, -1), slice(1, None)
        a, b = lab[tuple(here)], lab[tuple(there)]
        differ = a != b
        faces = np.zeros(cap, np.int64)
        for side in (a, b):  # a face between two ranks counts for both
            sel = differ & ranked(side)
            faces += np.bincount(side[sel] - 1, minlength=cap)
        out["faces"][:, c] = faces
        out["border_faces"][:, c] = np.bincount(k[p == 0], minlength=cap) + np.bincount(k[p == vol.shape[axis] - 1], minlength=cap)
    return out


def histogram(vol, region, lo, width, n_bins):
    """(uint64[n_bins], below, above) of vol over region: bin b holds lo + b width <= V < lo + (b + 1) width"""
    v = vol[np.asarray(region, bool)].astype(np.int64)
    b = (v - int(lo)) // int(width)  # floor: negative exactly for V < lo
    inside = (b >= 0) & (b < int(n_bins))
    counts = np.bincount(b[inside], minlength=int(n_bins)).astype(np.uint64)
    return counts, int(np.count_nonzero(b < 0)), int(np.count_nonzero(b >= int(n_bins)))


def record_by_loops(vol, region):
    """the same record by a triple loop over the voxels and their +x, +y, +z neighbours (for volumes of a few hundred voxels)"""
    Z, Y, X = vol.shape
    dims = (X, Y, Z)
    r = {"count": 0, "sum": 0, "sum_sq": 0, "vmin": None, "vmax": None, "sum_pos": [0, 0, 0], "lo": [None] * 3, "hi": [None] * 3,
         "faces": [0, 0, 0], "border": [0, 0, 0]}
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                p = (x, y, z)
                inside = bool(region[z, y, x])
                for c in range(3):
                    q = list(p)
                    q[c] += 1
                    if q[c] < dims[c] and bool(region[q[2], q[1], q[0]]) != inside:
                        r["faces"][c] += 1
                if not inside:
                    continue
                v = int(vol[z, y, x])
                r["count"] += 1
                r["sum"] += v
                r["sum_sq"] += v * v
                r["vmin"] = v if r["vmin"] is None else min(r["vmin"], v)
                r["vmax"] = v if r["vmax"] is None else max(r["vmax"], v)
                for c in range(3):
                    r["sum_pos"][c] += p[c]
                    r["lo"][c] = p[c] if r["lo"][c] is None else min(r["lo"][c], p[c])
                    r["hi"][c] = p[c] + 1 if r["hi"][c] is None else max(r["hi"][c], p[c] + 1)
                    r["border"][c] += (p[c] == 0) + (p[c] == dims[c] - 1)
    out = np.zeros((), DTYPE)
    if r["count"]:
        out["count"], out["sum"], out["sum_sq"], out["vmin"], out["vmax"] = r["count"], r["sum"], r["sum_sq"], r["vmin"], r["vmax"]
        out["sum_pos"], out["bbox_lo"], out["bbox_hi"] = r["sum_pos"], r["lo"], r["hi"]
        out["faces"], out["border_faces"] = r["faces"], r["border"]
    return out


def as_dict(rec):
    """a record's fields as Python ints and tuples (ffi.RegionStats.as_dict's form)"""
    return {k: (tuple(int(v) for v in rec[k]) if rec[k].shape else int(rec[k])) for k in DTYPE.names}
