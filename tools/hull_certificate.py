"""How many first legs could a 'hull certificate' end before their first step?  (candidate optimisation, restated in numpy and
measured on the CPU before k_bounce is touched):  python tools/hull_certificate.py [N] [--grid G] [--radius R | --all | --two-level] [--close]

A first leg starts at P = (hit origin + hit direction) + 2 * normal.  If every corner of every event voxel lies behind a plane
{x : n_k . x = h_k} and P lies m >= m0 in front of it, a leg whose direction has d . n_k >= delta0 moves away from every event voxel
linearly with its path; by the regularity of the step bytes (k_start_regular) its steps grow with that distance, so the march can only
leave the volume, and hull_delta0 below is the smallest delta0 with which it provably does so within 70 - 5 steps.

The table holds h_k (plus the device table's slack) for the K = G x G directions of an octahedral grid.  Per hit the plane with the
largest margin is chosen among the (2 R + 1)^2 grid directions around the normal's cell, in the whole table (--all), or by the
two-level search k_primary runs (--two-level).  Printed: the share of hits with a plane at margin >= m0, the share
that would reach one within a path of 4 voxels, the share of sampled hemisphere directions that would be granted, next to the share
the octant start certificate grants today and the share either proof grants."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cl_volume_renderer_amd import scene  # noqa: E402

F = np.float32
SQRT3 = 1.7320508075688772


# ---- the table

def oct_directions(G, unit=True):
    """[G * G][3] float64: direction k = j * G + i is the octahedral decode of the centre of cell (i, j); `unit`: normalised to
    length 1, else to |x| + |y| + |z| = 1 (every component a multiple of 1 / G: exact in binary32)"""
    c = (np.arange(G, dtype=np.float64) + 0.5) * (2.0 / G) - 1.0
    u, v = np.meshgrid(c, c, indexing="xy")
    z = 1.0 - np.abs(u) - np.abs(v)
    x = np.where(z >= 0, u, (1.0 - np.abs(v)) * np.where(u >= 0, 1.0, -1.0))
    y = np.where(z >= 0, v, (1.0 - np.abs(u)) * np.where(v >= 0, 1.0, -1.0))
    n = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    return n / np.linalg.norm(n, axis=1, keepdims=True) if unit else n


def oct_cell(n, G):
    """(i, j) of the octahedral cell a direction [..., 3] falls in"""
    n = np.asarray(n, np.float64)
    s = np.abs(n).sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = n / s[..., None]
    u, v = p[..., 0], p[..., 1]
    fold_u = (1.0 - np.abs(p[..., 1])) * np.where(p[..., 0] >= 0, 1.0, -1.0)
    fold_v = (1.0 - np.abs(p[..., 0])) * np.where(p[..., 1] >= 0, 1.0, -1.0)
    u, v = np.where(p[..., 2] >= 0, u, fold_u), np.where(p[..., 2] >= 0, v, fold_v)
    with np.errstate(invalid="ignore"):
        i = np.clip(np.floor((u + 1.0) * 0.5 * G), 0, G - 1)
        j = np.clip(np.floor((v + 1.0) * 0.5 * G), 0, G - 1)
    return np.nan_to_num(i).astype(np.int64), np.nan_to_num(j).astype(np.int64)


def support_table(event, dirs):
    """h_k = max of n_k . c over the eight corners c of every event voxel ([z][y][x] bool); -inf without events.  Along a row of
    voxels a linear function takes its maximum at the row's first or last event voxel: only those are visited."""
    Z, Y, X = event.shape
    any_row = event.any(axis=2)
    first = np.argmax(event, axis=2)
    last = X - 1 - np.argmax(event[:, :, ::-1], axis=2)
    zz, yy = np.nonzero(any_row)
    if len(zz) == 0:
        return np.full(len(dirs), -np.inf)
    pts = np.concatenate([np.stack([first[zz, yy], yy, zz], axis=1), np.stack([last[zz, yy], yy, zz], axis=1)]).astype(np.float64)
    h = np.full(len(dirs), -np.inf)
    for k0 in range(0, len(dirs), 256):
        n = dirs[k0:k0 + 256]
        h[k0:k0 + 256] = (pts @ n.T).max(axis=0) + np.maximum(n, 0.0).sum(axis=1)
    return h


def choose_plane(P, normal, dirs, h, G, radius=1):
    """per start point: (index of the plane with the largest margin among the cells around the normal's, that margin); index -1 and
    margin -inf where no plane is in front of the point (or P / the normal hold a NaN)"""
    best_m = np.full(len(P), -np.inf)
    best_k = np.full(len(P), -1, np.int64)
    P64 = P.astype(np.float64)
    if radius is None:  # the whole table: what no neighbourhood rule can beat
        for c0 in range(0, len(P), 4096):
            with np.errstate(invalid="ignore"):
                m = np.nan_to_num(P64[c0:c0 + 4096] @ dirs.T - h[None, :], nan=-np.inf)
            best_k[c0:c0 + 4096], best_m[c0:c0 + 4096] = m.argmax(axis=1), m.max(axis=1)
        best_k[best_m == -np.inf] = -1
        return best_k, best_m
    i0, j0 = oct_cell(normal, G)
    for dj in range(-radius, radius + 1):
        for di in range(-radius, radius + 1):
            i, j = np.clip(i0 + di, 0, G - 1), np.clip(j0 + dj, 0, G - 1)
            k = j * G + i
            with np.errstate(invalid="ignore"):
                m = (P64 * dirs[k]).sum(axis=1) - h[k]
                better = m > best_m
            best_m[better], best_k[better] = m[better], k[better]
    return best_k, best_m


def choose_plane_two_level(P, dirs, h, G):
    """k_primary's search: the best of every 4th cell in both directions, then the best of the 7 x 7 cells around it"""
    P64 = P.astype(np.float64)
    c = np.arange(2, G, 4)
    coarse = (c[:, None] * G + c[None, :]).reshape(-1)
    best_m = np.full(len(P), -np.inf)
    best_k = np.full(len(P), -1, np.int64)
    for c0 in range(0, len(P), 8192):
        with np.errstate(invalid="ignore"):
            m = np.nan_to_num(P64[c0:c0 + 8192] @ dirs[coarse].T - h[coarse][None, :], nan=-np.inf)
        best_k[c0:c0 + 8192], best_m[c0:c0 + 8192] = coarse[m.argmax(axis=1)], m.max(axis=1)
    i0, j0 = best_k % G, best_k // G
    for dj in range(-3, 4):
        for di in range(-3, 4):
            k = np.clip(j0 + dj, 0, G - 1) * G + np.clip(i0 + di, 0, G - 1)
            with np.errstate(invalid="ignore"):
                m = (P64 * dirs[k]).sum(axis=1) - h[k]
                better = m >= best_m
            best_m[better], best_k[better] = m[better], k[better]
    best_k[~(best_m >= 0)] = -1
    return best_k, best_m


# ---- the step bound (the host loop, restated)

def step_cap(X, Y, Z):
    return min(127, max(X, Y, Z) // 2)


def hull_steps_ok(X, Y, Z, delta0, m0, steps):
    """does the worst-case recurrence carry a leg out of the volume within `steps` steps?  After a path t the position is at least
    m0 + t * delta0 in front of the plane, its voxel at least floor(that / sqrt 3) - 2 voxels (Chebyshev) from every event voxel,
    and the step taken there at least min(cap, that), never below 1"""
    reach, cap, t = SQRT3 * (max(X, Y, Z) + 1.0), float(step_cap(X, Y, Z)), 0.0
    for _ in range(steps):
        if t > reach:
            break
        t += max(1.0, min(cap, math.floor((m0 + t * delta0) / SQRT3) - 2.0))
    return t > reach


def hull_delta0(X, Y, Z, m0, steps=70 - 5):
    """the smallest delta0 (a multiple of 1/64) that passes; 2.0: none does"""
    for k in range(1, 65):
        if hull_steps_ok(X, Y, Z, k / 64.0, m0, steps):
            return k / 64.0
    return 2.0


# ---- hits: a plain numpy restatement of the primary march (binary32 throughout)

def _normalize(v):
    v = v.astype(F)
    ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (v / ln[..., None]).astype(F)


def camera_rays(pos, d, w, h):
    up = np.array([0, 1, 0], F)
    side = _normalize(np.cross(up, d))
    cup = _normalize(np.cross(d, side))
    if cup[1] < 0:
        cup = -cup
    x, y = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    xo = ((x - w // 2).astype(F) / F(w) * (F(w) / F(h))).astype(F)
    yo = ((y - h // 2).astype(F) / F(h)).astype(F)
    p = (d[None, None, :] + side[None, None, :] * xo[..., None]) + cup[None, None, :] * yo[..., None]
    return _normalize(p.reshape(-1, 3))


def box_entry(pos, dirs, dims):
    """slab entry of rays that start outside (a measurement needs the rays that enter, not the reference's corner cases)"""
    dims = np.asarray(dims, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (0 - pos) / dirs, (dims - pos) / dirs
    tn, tf = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
    inside = np.all((pos >= 0) & (pos <= dims))
    ok = (tf >= np.maximum(tn, 0)) | inside
    t = np.where(inside, 0, np.maximum(tn, 0)).astype(F)
    return ok, (pos[None, :] + dirs * t[:, None]).astype(F)


def primary_hits(vol, sdf, event, pos, d, w, h):
    """(origin, direction, normal) of the camera rays whose first march ends in a Hit"""
    Z, Y, X = vol.shape
    dims = np.array([X, Y, Z], F)
    dirs = camera_rays(pos.astype(F), d.astype(F), w, h)
    ok, o = box_entry(pos.astype(F), dirs, dims)
    o, dirs = o[ok], dirs[ok]

    def voxel(p):
        inside = np.all((p >= 0) & (p < dims), axis=1)
        i = np.where(inside[:, None], p, 0).astype(np.int64)
        return inside, i

    inside, i = voxel(o)
    sd = np.where(inside, sdf[i[:, 2], i[:, 1], i[:, 0]], 0).astype(np.int32)
    alive = np.ones(len(o), bool)
    hit = np.zeros(len(o), bool)
    for _ in range(70):
        step = np.maximum(sd.astype(F), F(0.5))
        o = np.where(alive[:, None], o + dirs * step[:, None], o).astype(F)
        exited = np.any((o < 0) | (o > dims), axis=1)
        alive &= ~exited
        inside, i = voxel(o)
        ev = alive & inside & event[i[:, 2], i[:, 1], i[:, 0]]
        hit |= ev
        alive &= ~ev
        sd = np.where(inside, np.maximum(sdf[i[:, 2], i[:, 1], i[:, 0]], 0), 0).astype(np.int32)
        if not alive.any():
            break
    o, dirs = o[hit], dirs[hit]
    _, i = voxel(o)
    pad = np.pad(vol.astype(np.int32), 1)
    x, y, z = i[:, 0] + 1, i[:, 1] + 1, i[:, 2] + 1
    g = np.stack([pad[z, y, x + 1] - pad[z, y, x - 1], pad[z, y + 1, x] - pad[z, y - 1, x], pad[z + 1, y, x] - pad[z - 1, y, x]], axis=1)
    return o, dirs, (-_normalize(g.astype(F))).astype(F)


def sample_legs(normal, rng):
    """one first-leg direction per hit, as hemisphere_reflective draws it with roughness 1: a lattice direction of the cube
    [-1024, 1023]^3, flipped into the normal's hemisphere"""
    v = rng.integers(-1024, 1024, size=normal.shape).astype(F)
    dec = (v * normal).sum(axis=1, dtype=F)
    return _normalize(v * dec[:, None])


def start_table(event):
    """the octant start certificate's table (tests/test_gpu_start_cert.py states it the same way)"""
    out = np.zeros(event.shape, np.uint8)
    for o in range(8):
        flips = [ax for ax, bit in ((2, 1), (1, 2), (0, 4)) if not (o & bit)]
        b = np.flip(event, flips) if flips else event
        for ax in range(3):
            b = np.logical_or.accumulate(b, axis=ax)
        b = np.flip(b, flips) if flips else b
        out |= (~b).astype(np.uint8) << o
    return out


def start_cert_dmin(X, Y, Z):
    reach, cap = SQRT3 * (max(X, Y, Z) + 1), step_cap(X, Y, Z)
    for k in range(1, 65):
        t = 0
        for _ in range(70 - 5):
            t += max(1, min(cap, (t * k) // 64 - 2))
        if t > reach:
            return k / 64.0
    return 2.0


def main():
    args = sys.argv[1:]
    n = int(args[0]) if args and args[0].isdigit() else 256
    G = int(args[args.index("--grid") + 1]) if "--grid" in args else 64
    radius = int(args[args.index("--radius") + 1]) if "--radius" in args else 1
    if "--all" in args:
        radius = None  # the best plane of the whole table, wherever the normal points
    two_level = "--two-level" in args  # the search k_primary runs
    slack = 0.0625 if "--slack" not in args else float(args[args.index("--slack") + 1])  # what the device table adds to every h_k
    close = "--close" in args
    from oracle import orc_ffi
    w, h = (1920, 1080) if n >= 512 else (960, 544)
    vol = scene.phantom(n)
    cache = args[args.index("--sdf-cache") + 1] if "--sdf-cache" in args else None
    sdf = np.load(cache) if cache and os.path.exists(cache) else orc_ffi.sdf_build(vol, orc_ffi.parse_tf(scene.tf_default_source()))[0]
    event = (vol >= 500) & (vol <= 1200)
    pos, d = scene.close_camera(n) if close else scene.default_camera(n)
    print("scene: phantom(%d), %dx%d, %s camera, default TF; octahedral grid %dx%d, planes from %s" % (
        n, w, h, "close" if close else "default", G, G, "k_primary's two-level search" if two_level else "the whole table" if radius is None else "the %dx%d cells around the normal's" % (2 * radius + 1, 2 * radius + 1)))
    o, cd, normal = primary_hits(vol, sdf, event, pos, d, w, h)
    P = ((o + cd) + normal * F(2.0)).astype(F)
    print("%d primary hits" % len(o))
    rng = np.random.default_rng(1)
    legs = np.concatenate([sample_legs(normal, rng) for _ in range(4)])
    with np.errstate(invalid="ignore"):
        dmin_ok = (np.abs(legs).min(axis=1) >= 2.0 ** -10) & ~np.isnan(legs).any(axis=1)
    # today's proof
    tab = start_table(event)
    with np.errstate(invalid="ignore"):
        has = np.all((P >= 0) & (P < F(n)), axis=1)
    idx = np.where(has[:, None], P, 0).astype(np.int64)
    mask = np.where(has, tab[idx[:, 2], idx[:, 1], idx[:, 0]], 0)
    octant = (legs[:, 0] < 0) * 1 + (legs[:, 1] < 0) * 2 + (legs[:, 2] < 0) * 4
    with np.errstate(invalid="ignore"):
        oct_grant = (((np.tile(mask, 4) >> octant) & 1) != 0) & (np.abs(legs).min(axis=1) >= start_cert_dmin(n, n, n))
    print("octant start certificate: %.1f %% of the sampled first legs" % (100.0 * oct_grant.mean()))
    for unit in (True, False):
        dirs = oct_directions(G, unit)
        hk = support_table(event, dirs) + slack
        k, m = choose_plane_two_level(P, dirs, hk, G) if two_level else choose_plane(P, normal, dirs, hk, G, radius)
        print("table directions of %s:" % ("unit length" if unit else "unit 1-norm (exact in binary32)"))
        print("  margins at P: median %.2f, quartiles %.2f / %.2f voxels" % (np.median(m), np.percentile(m, 25), np.percentile(m, 75)))
        for m0 in (0.0, 0.25, 0.5, 1.0, 2.0):  # on top of the slack (the kernels use 0)
            d0 = hull_delta0(n, n, n, m0)
            nk = dirs[np.tile(np.maximum(k, 0), 4)]
            dn = (legs.astype(np.float64) * nk).sum(axis=1)
            mm = np.tile(m, 4)
            with np.errstate(invalid="ignore", divide="ignore"):
                now = (mm >= m0) & (dn >= d0) & dmin_ok
                t_need = (m0 - mm) / dn
                soon = (dn >= d0) & dmin_ok & (mm > -np.inf) & (t_need <= 4.0)
            print("  m0 = %-8g delta0 = %-8g hits with a plane at margin >= m0: %5.1f %%;  within t_need <= 4 for the median leg: %5.1f %%;  "
                  "legs granted at once: %5.1f %%, at once or deferred (t_need <= 4): %5.1f %%;  at once, either proof: %5.1f %%" % (
                      m0, d0, 100.0 * (m >= m0).mean(), 100.0 * (m >= m0 - 4.0 * 0.5).mean(), 100.0 * now.mean(), 100.0 * soon.mean(),
                      100.0 * (now | oct_grant).mean()))


if __name__ == "__main__":
    main()
