"""numpy restatement of the isosurface contract (include/clwh.h, clwh_render_isosurface).  The camera rays and the kept range are the
projections' (tests/projection_ref.py); this file adds the fixed-point trilinear field S (int64, value * 2^24), the threshold T, the
first inside sample, the bisection between the last outside and the first inside sample, and the normal from the corners' clamped
central differences.

isosurface() is vectorised over pixels (all pixels of the region, or a subset of its rows) and always walks densely: brick skipping
must not change a byte.  isosurface_scalar() reads the contract literally for one pixel, over every k, in Python integers."""
import math

import numpy as np

from tests import composite_ref as cr
from tests import projection_ref as pr

F = np.float32
DENSE, BELOW = 1, 2
CANONICAL_NAN = cr.CANONICAL_NAN
TWO_M24 = F(2.0 ** -24)


def threshold(iso):
    """T = (int64)floor((double)iso * 2^24): the product is exact in binary64"""
    return int(math.floor(float(F(iso)) * 16777216.0))


def cell(p):
    """per axis i0 = (int)floorf(p - 0.5f) and w = min((int)((q - f) * 256.0f), 255) for positions p [m][3] float32 -> (i0, w) int64 [m][3]"""
    q = np.asarray(p, F) - F(0.5)
    f = np.floor(q)
    w = np.minimum(((q - f) * F(256.0)).astype(np.int64), 255)
    return f.astype(np.int64), w


def _corner(vol, i0, w, corner):
    """clamped coordinates [m][3] (x, y, z) and the int64 weight [m] of corner number `corner` (bit c = upper corner on axis c)"""
    Z, Y, X = vol.shape
    hi = np.array([X - 1, Y - 1, Z - 1], np.int64)
    bits = np.array([corner & 1, (corner >> 1) & 1, corner >> 2], np.int64)
    xyz = np.minimum(np.maximum(i0 + bits, 0), hi)
    wt = np.where(bits == 1, w, 256 - w).prod(axis=1)
    return xyz, wt


def field(vol, i0, w):
    """S = sum over the 8 corners of wx * wy * wz * V(corner), int64 [m]"""
    S = np.zeros(i0.shape[0], np.int64)
    for corner in range(8):
        xyz, wt = _corner(vol, i0, w, corner)
        S += wt * vol[xyz[:, 2], xyz[:, 1], xyz[:, 0]].astype(np.int64)
    return S


def field_at(vol, p):
    return field(vol, *cell(p))


def gradient(vol, i0, w):
    """G [m][3] int64: sum over the corners of weight * (V(corner + e_c) - V(corner - e_c)), neighbour coordinates clamped"""
    Z, Y, X = vol.shape
    hi = np.array([X - 1, Y - 1, Z - 1], np.int64)
    G = np.zeros((i0.shape[0], 3), np.int64)
    for corner in range(8):
        xyz, wt = _corner(vol, i0, w, corner)
        for c in range(3):
            up, dn = xyz.copy(), xyz.copy()
            up[:, c] = np.minimum(xyz[:, c] + 1, hi[c])
            dn[:, c] = np.maximum(xyz[:, c] - 1, 0)
            diff = vol[up[:, 2], up[:, 1], up[:, 0]].astype(np.int64) - vol[dn[:, 2], dn[:, 1], dn[:, 0]].astype(np.int64)
            G[:, c] += wt * diff
    return G


def inside(S, T, flags):
    return S <= T if flags & BELOW else S >= T


def shade(G, d, ambient):
    """(n [m][3], s [m]) float32 from the integer gradient: one rounding of G, then the compositor's words"""
    g = G.astype(np.float64).astype(F)
    amb = F(ambient)
    l2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ln = np.sqrt(l2)
        n = g / ln[:, None]
        c = np.abs((g[:, 0] * d[:, 0] + g[:, 1] * d[:, 1]) + g[:, 2] * d[:, 2]) / ln
        s = amb + (F(1.0) - amb) * np.fmin(c, F(1.0))
    ok = l2 > 0
    return np.where(ok[:, None], n, F(0.0)).astype(F), np.where(ok, s, F(1.0)).astype(F), l2


def isosurface(vol, cam_pos, cam_dir, frame_wh, region_wh, iso, step=0.5, refine=8, flags=0, color=(1.0, 1.0, 1.0), ambient=0.3,
               t_near=0.0, t_far=np.inf, rows=None):
    """(frame [rows][w][4] uint8, t_hit [rows][w] float32, normal [rows][w][4] float32, stats) of the launched region.  stats: per
    pixel the number of kept samples ("n") and the masks "hit", "refined" (hit after the first kept sample), "first" (hit at the
    first kept sample), "flat" (hit with l2 == 0), "straddle" (the hit's cell crosses an 8^3 brick face), "clamped" (a corner of the
    hit's cell was clamped at a volume face)."""
    Z, Y, X = vol.shape
    dims = (X, Y, Z)
    T = threshold(iso)
    o = np.asarray(cam_pos, F)
    xs, ys = pr.pixel_grid(region_wh, rows)
    d = pr.generate_ray(cam_dir, xs, ys, frame_wh[0], frame_wh[1]).reshape(-1, 3)
    ka, kb = pr.kept_range_dirs(o, d, dims, step, t_near, t_far)
    n = np.maximum(kb - ka + 1, 0)
    npx = d.shape[0]
    k_hit = np.full(npx, -1, np.int64)
    S_hit = np.zeros(npx, np.int64)
    idx = np.nonzero(n > 0)[0]
    j = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while idx.size:
            _, p = pr._sample(o, d[idx], ka[idx] + j, step)
            S = field_at(vol, p)
            ins = inside(S, T, flags)
            k_hit[idx[ins]] = ka[idx[ins]] + j
            S_hit[idx[ins]] = S[ins]
            j += 1
            idx = idx[~ins & (n[idx] > j)]
        hit = np.nonzero(k_hit >= 0)[0]
        dh = d[hit]
        hi = k_hit[hit].astype(F) * F(step)
        lo = (k_hit[hit] - 1).astype(F) * F(step)
        refined = k_hit[hit] > ka[hit]
        Sh = S_hit[hit]
        for _ in range(int(refine)):
            m = lo + (hi - lo) * F(0.5)
            p = o + dh * m[:, None]
            p = np.where(refined[:, None], p, F(0.5))  # (rays hit at their first kept sample are not refined: any valid position)
            S = field_at(vol, p)
            ins = inside(S, T, flags)
            hi = np.where(refined & ins, m, hi)
            lo = np.where(refined & ~ins, m, lo)
            Sh = np.where(refined & ins, S, Sh)
        p_hit = o + dh * hi[:, None]
        i0, w = cell(p_hit)
        nrm, s, l2 = shade(gradient(vol, i0, w), dh, ambient)
    t_hit = np.full(npx, np.nan, F)
    t_hit[hit] = hi
    normal = np.full((npx, 4), CANONICAL_NAN, F)
    normal[hit, :3] = nrm
    normal[hit, 3] = Sh.astype(np.float64).astype(F) * TWO_M24
    frame = np.zeros((npx, 4), np.uint8)
    col = np.asarray(color, F)
    frame[hit, :3] = cr.quantise(col[None, :] * s[:, None])
    frame[hit, 3] = 255
    shape = xs.shape
    top = np.array([X - 1, Y - 1, Z - 1], np.int64)

    def mask(values):
        m = np.zeros(npx, bool)
        m[hit] = values
        return m.reshape(shape)

    stats = {"n": n.reshape(shape), "hit": mask(True), "refined": mask(refined), "first": mask(~refined), "flat": mask(~(l2 > 0)),
             "straddle": mask(((i0 >= 0) & (i0 < top) & ((i0 & 7) == 7)).any(axis=1)),
             "clamped": mask(((i0 < 0) | (i0 >= top)).any(axis=1))}
    return frame.reshape(shape + (4,)), t_hit.reshape(shape), cr.canonical(normal).reshape(shape + (4,)), stats


def isosurface_scalar(vol, cam_pos, cam_dir, frame_wh, x, y, iso, step=0.5, refine=8, flags=0, color=(1.0, 1.0, 1.0), ambient=0.3,
                      t_near=0.0, t_far=np.inf):
    """one pixel, sample by sample over every k up to past the farthest corner, the field in Python integers:
    (pixel [4] uint8, t_hit float32, normal [4] float32)"""
    Z, Y, X = vol.shape
    dims = (X, Y, Z)
    T = threshold(iso)
    o = np.asarray(cam_pos, F)
    d = pr.generate_ray(cam_dir, np.array(x), np.array(y), frame_wh[0], frame_wh[1])
    corners = np.array([[cx, cy, cz] for cx in (0, X) for cy in (0, Y) for cz in (0, Z)], np.float64)
    far = np.sqrt(((corners - o.astype(np.float64)) ** 2).sum(axis=1)).max()

    def V(cx, cy, cz):
        return int(vol[min(max(cz, 0), Z - 1), min(max(cy, 0), Y - 1), min(max(cx, 0), X - 1)])

    def cell_of(p):
        i0, w = [], []
        for c in range(3):
            q = F(p[c]) - F(0.5)
            f = np.floor(q)
            i0.append(int(f))
            w.append(min(int((q - f) * F(256.0)), 255))
        return i0, w

    def corners_of(i0, w):
        for bz in (0, 1):
            for by in (0, 1):
                for bx in (0, 1):
                    wt = (w[0] if bx else 256 - w[0]) * (w[1] if by else 256 - w[1]) * (w[2] if bz else 256 - w[2])
                    yield wt, [min(max(i0[c] + b, 0), dims[c] - 1) for c, b in enumerate((bx, by, bz))]

    def S_of(p):
        return sum(wt * V(*xyz) for wt, xyz in corners_of(*cell_of(p)))

    def is_inside(S):
        return S <= T if flags & BELOW else S >= T

    miss = (np.zeros(4, np.uint8), F(np.nan), np.full(4, CANONICAL_NAN, F))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        first_kept, k_hit = None, None
        for k in range(int(far / step * 1.001) + 4):
            if not pr.kept(o, d, np.int64(k), step, dims, t_near, t_far):
                continue
            if first_kept is None:
                first_kept = k
            _, p = pr._sample(o, d, np.int64(k), step)
            if is_inside(S_of(p)):
                k_hit = k
                break
        if k_hit is None:
            return miss
        hi = F(k_hit) * F(step)
        if k_hit != first_kept:
            lo = F(k_hit - 1) * F(step)
            for _ in range(int(refine)):
                m = lo + (hi - lo) * F(0.5)
                if is_inside(S_of(o + d * m)):
                    hi = m
                else:
                    lo = m
        p_hit = o + d * hi
        i0, w = cell_of(p_hit)
        G = [0, 0, 0]
        for wt, (cx, cy, cz) in corners_of(i0, w):
            G[0] += wt * (V(cx + 1, cy, cz) - V(cx - 1, cy, cz))
            G[1] += wt * (V(cx, cy + 1, cz) - V(cx, cy - 1, cz))
            G[2] += wt * (V(cx, cy, cz + 1) - V(cx, cy, cz - 1))
        g = [F(float(v)) for v in G]  # |G| < 2^41 is exact in binary64: one rounding
        l2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        one, amb = F(1.0), F(ambient)
        if l2 > 0:
            ln = np.sqrt(l2)
            nrm = [g[0] / ln, g[1] / ln, g[2] / ln]
            c = np.abs((g[0] * d[0] + g[1] * d[1]) + g[2] * d[2]) / ln
            s = amb + (one - amb) * np.fmin(c, one)
        else:
            nrm, s = [F(0.0)] * 3, one
        px = np.array([cr.quantise(F(color[0]) * s), cr.quantise(F(color[1]) * s), cr.quantise(F(color[2]) * s), 255], np.uint8)
        value = F(float(S_of(p_hit))) * TWO_M24
        return px, F(hi), cr.canonical(np.array(nrm + [value], F))


def dilated_brick_bounds(vol):
    """(dmin, dmax) int64 [NBZ][NBY][NBX]: minimum and maximum of every 8^3 brick dilated by one voxel, clamped at the volume's faces"""
    Z, Y, X = vol.shape
    nb = [(n + 7) // 8 for n in (Z, Y, X)]
    dmin = np.zeros(nb, np.int64)
    dmax = np.zeros(nb, np.int64)
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                box = vol[max(8 * bz - 1, 0):8 * bz + 9, max(8 * by - 1, 0):8 * by + 9, max(8 * bx - 1, 0):8 * bx + 9]
                dmin[bz, by, bx], dmax[bz, by, bx] = box.min(), box.max()
    return dmin, dmax
