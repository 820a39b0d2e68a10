"""numpy float32 restatement of the compositing contract (include/clwh.h, clwh_render_composite).  The camera rays and the kept
range are the projections' (tests/projection_ref.py); this file adds the per-sample arithmetic: table lookup, optional two-sided
headlight shading from clamped central differences, front-to-back accumulation and early termination.

composite() is vectorised over pixels (all pixels of the region, or a subset of its rows); composite_scalar() reads the contract
literally for one pixel, over every k."""
import numpy as np

from tests import projection_ref as pr

F = np.float32
DENSE, SHADE = 1, 2
CANONICAL_NAN = np.array([0x7FC00000], np.uint32).view(F)[0]


def lut_index(v, lut_first, lut_len):
    return np.minimum(np.maximum(np.asarray(v, np.int64) - int(lut_first), 0), int(lut_len) - 1)


def quantise(x):
    """q(x) = (int)fminf(fmaxf(x * 255 + 0.5, 0), 255): fmaxf / fminf return the other operand for a NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.fmin(np.fmax(np.asarray(x, F) * F(255.0) + F(0.5), F(0.0)), F(255.0))
        return u.astype(np.int32).astype(np.uint8)


def canonical(x):
    """IEEE 754 leaves a NaN's sign and payload open; the contract stores every NaN as 0x7FC00000"""
    x = np.asarray(x, F)
    return np.where(np.isnan(x), CANONICAL_NAN, x).astype(F)


def _gradient(vol, ix):
    """clamped central differences in int32 at integer voxel coordinates ix [m][3] (x, y, z) -> three float32 [m]"""
    Z, Y, X = vol.shape
    dims = (X, Y, Z)
    out = []
    for c in range(3):
        hi, lo = ix.copy(), ix.copy()
        hi[:, c] = np.minimum(ix[:, c] + 1, dims[c] - 1)
        lo[:, c] = np.maximum(ix[:, c] - 1, 0)
        g = vol[hi[:, 2], hi[:, 1], hi[:, 0]].astype(np.int32) - vol[lo[:, 2], lo[:, 1], lo[:, 0]].astype(np.int32)
        out.append(g.astype(F))
    return out


def _shade_factor(gx, gy, gz, d, ambient):
    amb = F(ambient)
    l2 = (gx * gx + gy * gy) + gz * gz
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = np.abs((gx * d[..., 0] + gy * d[..., 1]) + gz * d[..., 2]) / np.sqrt(l2)
        s = amb + (F(1.0) - amb) * np.fmin(c, F(1.0))
    return np.where(l2 > 0, s, F(1.0)).astype(F)


def composite(vol, cam_pos, cam_dir, frame_wh, region_wh, lut, lut_first, step=0.5, alpha_stop=0.95, flags=0, ambient=0.3,
              t_near=0.0, t_far=np.inf, rows=None):
    """(frame [rows][w][4] uint8, rgba [rows][w][4] float32, t_first [rows][w], t_stop [rows][w], stats) of the launched region.
    stats: kept samples read up to termination ("read"), kept samples in all ("kept"), pixels with kept samples ("rays"), kept samples per pixel ("n")."""
    Z, Y, X = vol.shape
    lut = np.ascontiguousarray(lut, F).reshape(-1, 4)
    L = lut.shape[0]
    o = np.asarray(cam_pos, F)
    xs, ys = pr.pixel_grid(region_wh, rows)
    d = pr.generate_ray(cam_dir, xs, ys, frame_wh[0], frame_wh[1]).reshape(-1, 3)
    ka, kb = pr.kept_range_dirs(o, d, (X, Y, Z), step, t_near, t_far)
    n = np.maximum(kb - ka + 1, 0)
    npx = d.shape[0]
    C = np.zeros((npx, 3), F)
    A = np.zeros(npx, F)
    t_first = np.full(npx, np.nan, F)
    t_stop = np.full(npx, np.nan, F)
    stop = F(alpha_stop)
    idx = np.nonzero(n > 0)[0]
    read = 0
    j = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while idx.size:
            read += idx.size
            t, p = pr._sample(o, d[idx], ka[idx] + j, step)
            ix = p.astype(np.int64)  # kept: 0 <= p < dim, truncation is floor
            v = vol[ix[:, 2], ix[:, 1], ix[:, 0]]
            e = lut[lut_index(v, lut_first, L)]
            hit = e[:, 3] > 0
            done = np.zeros(idx.size, bool)
            if hit.any():
                sub = idx[hit]
                col = e[hit, :3].copy()
                al = e[hit, 3]
                if flags & SHADE:
                    gx, gy, gz = _gradient(vol, ix[hit])
                    s = _shade_factor(gx, gy, gz, d[sub], ambient)
                    col = col * s[:, None]
                w = (F(1.0) - A[sub]) * al
                C[sub] = C[sub] + w[:, None] * col
                A[sub] = A[sub] + w
                first = np.isnan(t_first[sub])
                t_first[sub] = np.where(first, t[hit], t_first[sub])
                ended = A[sub] >= stop
                t_stop[sub] = np.where(ended, t[hit], t_stop[sub])
                done[hit] = ended
            j += 1
            idx = idx[~done & (n[idx] > j)]
    shape = xs.shape
    rgba = canonical(np.concatenate([C, A[:, None]], axis=1)).reshape(shape + (4,))
    frame = quantise(rgba)
    stats = {"read": int(read), "kept": int(n.sum()), "rays": int((n > 0).sum()), "n": n.reshape(shape)}
    return frame, rgba, t_first.reshape(shape), t_stop.reshape(shape), stats


def composite_scalar(vol, cam_pos, cam_dir, frame_wh, x, y, lut, lut_first, step=0.5, alpha_stop=0.95, flags=0, ambient=0.3,
                     t_near=0.0, t_far=np.inf):
    """one pixel, sample by sample over every k up to past the farthest corner: (rgba [4] float32, t_first, t_stop)"""
    Z, Y, X = vol.shape
    dims = (X, Y, Z)
    lut = np.ascontiguousarray(lut, F).reshape(-1, 4)
    L = lut.shape[0]
    o = np.asarray(cam_pos, F)
    d = pr.generate_ray(cam_dir, np.array(x), np.array(y), frame_wh[0], frame_wh[1])
    corners = np.array([[cx, cy, cz] for cx in (0, X) for cy in (0, Y) for cz in (0, Z)], np.float64)
    far = np.sqrt(((corners - o.astype(np.float64)) ** 2).sum(axis=1)).max()
    one, amb, stop = F(1.0), F(ambient), F(alpha_stop)
    C = [F(0.0), F(0.0), F(0.0)]
    A = F(0.0)
    t_first, t_stop = F(np.nan), F(np.nan)

    def V(cx, cy, cz):
        return int(vol[min(max(cz, 0), Z - 1), min(max(cy, 0), Y - 1), min(max(cx, 0), X - 1)])

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(int(far / step * 1.001) + 4):
            if not pr.kept(o, d, np.int64(k), step, dims, t_near, t_far):
                continue
            t, p = pr._sample(o, d, np.int64(k), step)
            vx, vy, vz = int(np.floor(p[0])), int(np.floor(p[1])), int(np.floor(p[2]))
            i = min(max(int(vol[vz, vy, vx]) - int(lut_first), 0), L - 1)
            r, g, b, a = lut[i]
            if not (a > 0):
                continue
            if flags & SHADE:
                gx = F(V(vx + 1, vy, vz) - V(vx - 1, vy, vz))
                gy = F(V(vx, vy + 1, vz) - V(vx, vy - 1, vz))
                gz = F(V(vx, vy, vz + 1) - V(vx, vy, vz - 1))
                l2 = (gx * gx + gy * gy) + gz * gz
                if l2 > 0:
                    c = np.abs((gx * d[0] + gy * d[1]) + gz * d[2]) / np.sqrt(l2)
                    s = amb + (one - amb) * np.fmin(c, one)
                else:
                    s = one
                r, g, b = r * s, g * s, b * s
            w = (one - A) * a
            C = [C[0] + w * r, C[1] + w * g, C[2] + w * b]
            A = A + w
            if np.isnan(t_first):
                t_first = t
            if A >= stop:
                t_stop = t
                break
    return canonical(np.array([C[0], C[1], C[2], A], F)), F(t_first), F(t_stop)


def ramp_table(lo, hi, a_max, lut_first=-1024, lut_len=4096, color=(1.0, 0.8, 0.6)):
    """alpha rising linearly from 0 at value lo to a_max at value hi (and staying there), one colour"""
    v = np.arange(lut_len, dtype=np.float64) + lut_first
    a = np.clip((v - lo) / (hi - lo), 0.0, 1.0) * a_max
    lut = np.zeros((lut_len, 4), F)
    lut[:, 0], lut[:, 1], lut[:, 2] = color
    lut[:, 3] = a.astype(F)
    return lut


def soft_table(**kw):
    return ramp_table(300, 1500, 0.05, **kw)


def hard_table(**kw):
    return ramp_table(500, 1200, 0.6, **kw)


def tf_composite_lut(selections, lut_first, lut_len, opacity):
    """app/tf_part.cpp tf_composite_lut restated: selections = [(min_v, max_v, (r, g, b, a)), ...]"""
    lut = np.zeros((lut_len, 4), F)
    for i in range(lut_len):
        for lo, hi, c in selections:
            if F(lo) <= F(i + lut_first) <= F(hi):
                lut[i] = (F(c[0]), F(c[1]), F(c[2]), F(c[3]) * F(opacity))
                break
    return lut
