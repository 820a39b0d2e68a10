"""numpy float32 restatement of the intensity-projection contract (include/clwh.h, clwh_render_projection), vectorised over pixels.

Sample k of a pixel's ray sits at t_k = (float)k * h, p_k = o + d * t_k (one float32 multiply, then one add, per component), and is
kept iff t_near <= t_k <= t_far and 0 <= p_k.c < dim_c on all three axes.  Every condition switches at most once as k grows (float
multiply and add are monotone), so a ray's kept samples are one range [k_a, k_b]: kept_range() finds it by bisection on the
conditions that can only turn true (rising) and those that can only turn false (falling).  project() then walks that range."""
import numpy as np

F = np.float32
MAX, MIN, MEAN = 0, 1, 2
K_CAP = 1 << 30  # every kept sample of an accepted call has k < K_CAP (clwh_render_projection checks camera distance / step)


def _normalize(v):
    ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    return v / ln[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def generate_ray(cam_dir, xs, ys, x_total, y_total):
    """directions (float32 [..., 3]) of the camera rays of pixels (xs, ys): utility_ray.cl:69-89 as render_device.hpp states it"""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.asarray(cam_dir, F)
        side = _normalize(_cross(np.array([0, 1, 0], F), d))
        up = _normalize(_cross(d, side))
        if up[1] < 0:
            up = -up
        x_f = (np.asarray(xs, np.int64) - x_total // 2).astype(F)
        y_f = (np.asarray(ys, np.int64) - y_total // 2).astype(F)
        aspect = F(x_total) / F(y_total)
        x_off = x_f / F(x_total) * aspect
        y_off = y_f / F(y_total)
        p = (d + side * x_off[..., None]) + up * y_off[..., None]
        return _normalize(p)


def _sample(o, d, k, h):
    t = np.asarray(k, np.int64).astype(F) * F(h)
    return t, o + d * t[..., None]


def _rising(t, p, d, dims, t_near):
    r = t >= F(t_near)
    for c in range(3):
        r &= np.where(d[..., c] > 0, p[..., c] >= 0, np.where(d[..., c] < 0, p[..., c] < F(dims[c]), True))
    return r


def _falling(t, p, d, dims, t_far):
    r = t <= F(t_far)
    for c in range(3):
        inside = (p[..., c] >= 0) & (p[..., c] < F(dims[c]))
        r &= np.where(d[..., c] > 0, p[..., c] < F(dims[c]), np.where(d[..., c] < 0, p[..., c] >= 0, inside))
    return r


def kept(o, d, k, h, dims, t_near=0.0, t_far=np.inf):
    """the contract's test of sample k, written out (no rising / falling split)"""
    with np.errstate(invalid="ignore", over="ignore"):
        t, p = _sample(o, d, k, h)
        ok = (t >= F(t_near)) & (t <= F(t_far))
        for c in range(3):
            ok &= (p[..., c] >= 0) & (p[..., c] < F(dims[c]))
        return ok


def kept_range_dirs(o, d, dims, h, t_near=0.0, t_far=np.inf):
    """per-ray [k_a, k_b] (int64; k_a > k_b when nothing is kept) for directions d [..., 3] from origin o"""
    o = np.asarray(o, F)
    d = np.asarray(d, F)
    shape = d.shape[:-1]
    with np.errstate(invalid="ignore", over="ignore"):
        def falling(k):
            t, p = _sample(o, d, k, h)
            return _falling(t, p, d, dims, t_far)

        def rising(k):
            t, p = _sample(o, d, k, h)
            return _rising(t, p, d, dims, t_near)

        zero = np.zeros(shape, np.int64)
        f0 = falling(zero)
        lo, hi = zero.copy(), np.full(shape, K_CAP, np.int64)  # falling(lo) true (where f0), hi: false or past the end
        while True:
            open_ = f0 & (hi - lo > 1)
            if not open_.any():
                break
            m = (lo + hi) // 2
            f = falling(m)
            lo = np.where(open_ & f, m, lo)
            hi = np.where(open_ & ~f, m, hi)
        kb = np.where(f0, lo, -1)
        r0 = rising(zero)
        lo, hi = zero.copy(), np.full(shape, K_CAP, np.int64)  # rising(lo) false (where not r0), hi: true or past the end
        while True:
            open_ = ~r0 & (hi - lo > 1)
            if not open_.any():
                break
            m = (lo + hi) // 2
            r = rising(m)
            lo = np.where(open_ & ~r, m, lo)
            hi = np.where(open_ & r, m, hi)
        ka = np.where(r0, 0, hi)
    return ka, kb


def pixel_grid(region_wh, rows=None):
    w, h = region_wh
    ys = np.arange(h) if rows is None else np.asarray(rows)
    return np.meshgrid(np.arange(w), ys)


def kept_range(cam_pos, cam_dir, dims, frame_wh, region_wh, step, t_near=0.0, t_far=np.inf, rows=None):
    """per-pixel [k_a, k_b] over the launched region (rows: a subset of its rows), each [len(rows)][width]"""
    xs, ys = pixel_grid(region_wh, rows)
    d = generate_ray(cam_dir, xs, ys, frame_wh[0], frame_wh[1])
    return kept_range_dirs(cam_pos, d, dims, step, t_near, t_far)


def window(values, center, width):
    """RGBA8 pixels of projected values (NaN: no kept sample -> 0, 0, 0, 0)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = ((values - F(center)) / F(width) + F(0.5)) * F(255.0) + F(0.5)
        grey = np.minimum(np.maximum(u, F(0)), F(255)).astype(np.int32).astype(np.uint8)
    out = np.zeros(values.shape + (4,), np.uint8)
    ok = ~np.isnan(values)
    out[ok, 0] = out[ok, 1] = out[ok, 2] = grey[ok]
    out[ok, 3] = 255
    return out


def project(vol, cam_pos, cam_dir, frame_wh, region_wh, modes=(MAX,), step=0.5, window_cw=(0.0, 1.0), t_near=0.0, t_far=np.inf,
            rows=None):
    """{mode: (frame [rows][w][4] uint8, values [rows][w] float32, t_extreme [rows][w] float32)} of the launched region"""
    Z, Y, X = vol.shape
    o = np.asarray(cam_pos, F)
    xs, ys = pixel_grid(region_wh, rows)
    d = generate_ray(cam_dir, xs, ys, frame_wh[0], frame_wh[1]).reshape(-1, 3)
    ka, kb = kept_range_dirs(o, d, (X, Y, Z), step, t_near, t_far)
    n = np.maximum(kb - ka + 1, 0)
    order = np.argsort(-n, kind="stable")  # longest ranges first: the rays still marching at step j are a prefix
    n_sorted = n[order]
    npx = d.shape[0]
    best = {MAX: np.full(npx, -32769, np.int32), MIN: np.full(npx, 32768, np.int32)}
    best_t = {MAX: np.full(npx, np.nan, F), MIN: np.full(npx, np.nan, F)}
    total = np.zeros(npx, np.int64)
    flat = vol.reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(n_sorted[0]) if npx else 0):
            m = int(np.searchsorted(-n_sorted, -j, side="left"))  # rays with n > j
            idx = order[:m]
            t, p = _sample(o, d[idx], ka[idx] + j, step)
            ix = p.astype(np.int64)  # kept: 0 <= p < dim, truncation is floor
            v = flat[(ix[:, 2] * Y + ix[:, 1]) * X + ix[:, 0]].astype(np.int32)
            total[idx] += v
            for mode, better in ((MAX, np.greater), (MIN, np.less)):
                b = better(v, best[mode][idx])
                best[mode][idx] = np.where(b, v, best[mode][idx])
                best_t[mode][idx] = np.where(b, t, best_t[mode][idx])
    out = {}
    shape = xs.shape
    for mode in modes:
        if mode == MEAN:
            with np.errstate(invalid="ignore", divide="ignore"):
                values = np.where(n > 0, (total.astype(np.float64) / n.astype(np.float64)).astype(F), F(np.nan)).astype(F)
            t_ext = np.full(npx, np.nan, F)
        else:
            values = np.where(n > 0, best[mode].astype(F), F(np.nan)).astype(F)
            t_ext = best_t[mode]
        values, t_ext = values.reshape(shape), t_ext.reshape(shape)
        out[mode] = (window(values, *window_cw), values, t_ext)
    return out


def project_scalar(vol, cam_pos, cam_dir, frame_wh, x, y, mode, step, t_near=0.0, t_far=np.inf):
    """one pixel, sample by sample over every k up to past the farthest corner: (value, t_extreme) -- the contract read literally"""
    Z, Y, X = vol.shape
    o = np.asarray(cam_pos, F)
    d = generate_ray(cam_dir, np.array(x), np.array(y), frame_wh[0], frame_wh[1])
    corners = np.array([[cx, cy, cz] for cx in (0, X) for cy in (0, Y) for cz in (0, Z)], np.float64)
    far = np.sqrt(((corners - o.astype(np.float64)) ** 2).sum(axis=1)).max()
    best, best_t, total, count = None, F(np.nan), 0, 0
    for k in range(int(far / step * 1.001) + 4):
        if not kept(o, d, np.int64(k), step, (X, Y, Z), t_near, t_far):
            continue
        t, p = _sample(o, d, np.int64(k), step)
        v = int(vol[int(np.floor(p[2])), int(np.floor(p[1])), int(np.floor(p[0]))])
        total, count = total + v, count + 1
        if best is None or (v > best if mode == MAX else v < best):
            best, best_t = v, t
    if count == 0:
        return F(np.nan), F(np.nan)
    if mode == MEAN:
        return F(np.float64(total) / np.float64(count)), F(np.nan)
    return F(best), F(best_t)
