"""How many more marches would a hull certificate end if it could wait a few literal steps, and if rebounds from secondary hits asked
it too?  (restated in numpy and measured on the CPU before k_bounce is touched):
    python tools/hull_defer.py [N] [--close] [--shell] [--rounds R] [--rules J D] [--sdf-cache FILE]

tools/hull_certificate.py gives every primary hit the plane k of the support table with the largest margin m_P = n_k . P - h_k at the
first legs' start point P, and grants a first leg at once when m_P >= 0 and d . n_k >= delta0.  Here the plane is kept when m_P is
negative, every sampled first leg is marched literally through the SDF image, and so is one rebound from every leg that ends in a Hit.
The rules, as k_bounce applies them to a march that starts at `start` with direction d (clwh_internal.hpp: the proof):
    m = floor(16 m_P) / 16 + n_k . (start - P)                 (start == P for a first leg)
    at once:   m >= 0 and d . n_k >= delta0(70 - 5 steps)
    deferred:  0 < -m <= D and d . n_k >= delta0(70 - 5 - J steps); the march counts its path with the kernel's integer counter (the SDF
               value of every step taken: a step of 0.5 counts 0) and is granted when the count reaches ceil(-m / d . n_k), if no event
               has ended it and it has taken at most J steps.
A grant is WRONG unless the literal march ends in Exit.  Printed per kind of march: grants, wrong grants, steps taken before a
deferred grant, steps saved (all, and those before the march's first step of >= 12 voxels, where the macro-cell table cannot help),
then the table of candidates J / D against J = 9, D unbounded, and the smallest pair that keeps nine tenths of the deferred grants."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_certificate as hc  # noqa: E402
from cl_volume_renderer_amd import scene  # noqa: E402

F = np.float32
GRID = 64
SLACK = 0.0625          # kHullSlack
SCALE = 16              # kHullMarginScale: the stored margin's grid
FIELD_MIN = -128 / SCALE  # what eight signed bits hold: "D unbounded" ends here
FAR_STEP = 12           # configs[1]'s certificate threshold: shorter steps never ask the macro-cell table
EXIT, HIT, NONE = 0, 1, 2
J_CANDIDATES = (2, 3, 4, 5, 6, 7, 8, 9)
D_CANDIDATES = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, -FIELD_MIN)


def defer_delta0(X, Y, Z, J):
    """hull_defer_delta0: the host's recurrence over 70 - 5 - J steps"""
    return hc.hull_delta0(X, Y, Z, 0.0, steps=70 - 5 - J)


def best_plane(P, dirs, h):
    """k_primary's two-level search (hull_certificate.choose_plane_two_level), the plane kept whatever its margin's sign;
    index -1 where P holds a NaN or no h_k is finite"""
    G = GRID
    P64 = P.astype(np.float64)
    c = np.arange(2, G, 4)
    coarse = (c[:, None] * G + c[None, :]).reshape(-1)
    with np.errstate(invalid="ignore"):
        m = np.nan_to_num(P64 @ dirs[coarse].T - h[coarse][None, :], nan=-np.inf)
    best_k, best_m = coarse[m.argmax(axis=1)], m.max(axis=1)
    i0, j0 = best_k % G, best_k // G
    for dj in range(-3, 4):
        for di in range(-3, 4):
            k = np.clip(j0 + dj, 0, G - 1) * G + np.clip(i0 + di, 0, G - 1)
            with np.errstate(invalid="ignore"):
                m = (P64 * dirs[k]).sum(axis=1) - h[k]
                better = m >= best_m
            best_m[better], best_k[better] = m[better], k[better]
    best_k[~np.isfinite(best_m)] = -1
    return best_k, best_m


def stored_margin(m):
    """the margin as the per-hit word holds it: rounded down on the grid and clamped to the field from above; a margin below the
    field has no word (clamping it would raise it): NaN"""
    with np.errstate(invalid="ignore"):
        q = np.floor(m * SCALE)
        return np.where(q >= -128, np.minimum(q, 127), np.nan) / SCALE


def march(start, d, sdf, event, need):
    """literal marches of 70 steps (hull_certificate.primary_hits' loop); `need`: per march the path its integer counter has to reach
    (inf: never).  Returns (how it ends, steps taken, steps taken when the counter got there with the march still going and its
    position in a voxel -- 0: never, steps taken before the first step of >= FAR_STEP voxels, position and voxel at the end)"""
    Z, Y, X = sdf.shape
    dims = np.array([X, Y, Z], F)
    o = start.astype(F).copy()
    d = d.astype(F)

    def voxel(p):
        with np.errstate(invalid="ignore"):
            inside = np.all((p >= 0) & (p < dims), axis=1)
        return inside, np.where(inside[:, None], p, 0).astype(np.int64)

    n = len(o)
    inside, i = voxel(o)
    sd = np.where(inside, np.maximum(sdf[i[:, 2], i[:, 1], i[:, 0]], 0), 0).astype(np.int64)
    alive = np.ones(n, bool)
    end = np.full(n, NONE)
    steps = np.zeros(n, np.int64)
    count = np.zeros(n, np.int64)
    fired = np.zeros(n, np.int64)
    near = np.zeros(n, np.int64)
    seen_far = np.zeros(n, bool)
    for s in range(1, 71):
        seen_far |= alive & (sd >= FAR_STEP)
        near += alive & ~seen_far
        step = np.maximum(sd.astype(F), F(0.5))
        o = np.where(alive[:, None], o + d * step[:, None], o).astype(F)
        count += np.where(alive, sd, 0)
        steps += alive
        with np.errstate(invalid="ignore"):
            exited = alive & np.any((o < 0) | (o > dims), axis=1)
        end[exited] = EXIT
        alive &= ~exited
        inside, i = voxel(o)
        ev = alive & inside & event[i[:, 2], i[:, 1], i[:, 0]]
        end[ev] = HIT
        alive &= ~ev
        sd = np.where(inside, np.maximum(sdf[i[:, 2], i[:, 1], i[:, 0]], 0), 0).astype(np.int64)
        fired = np.where((fired == 0) & alive & inside & (count >= need) & (s < 70), s, fired)
        if not alive.any():
            break
    return end, steps, fired, near, o, i


def rules(m, dn, ok_dir, dims, J, D):
    """(granted at once, armed for a deferred grant, the path an armed march has to count)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        at_once = ok_dir & (m >= 0) & (dn >= hc.hull_delta0(*dims, 0.0))
        armed = ok_dir & (m < 0) & (m >= -D) & (dn >= defer_delta0(*dims, J))
        need = np.where(armed, np.ceil(-m / dn * (1.0 + 2.0 ** -19)), np.inf)
    return at_once, armed, need


def measure(vol, sdf, event, pos, d, w, h, rounds=4, seed=1):
    """the marches: a dict per kind of march ('first', 'rebound') with the margin, d . n_k, the direction guard and the literal march
    of every sample, with the step at which its counter got there; 'hits': the per-hit margins"""
    Z, Y, X = vol.shape
    o, cd, normal = hc.primary_hits(vol, sdf, event, pos, d, w, h)
    P = ((o + cd) + normal * F(2.0)).astype(F)
    dirs = hc.oct_directions(GRID, True)
    hk = hc.support_table(event, dirs) + SLACK
    k, mP = best_plane(P, dirs, hk)
    has = k >= 0
    rng = np.random.default_rng(seed)
    out = {"hits": dict(n=len(o), margin=np.where(has, mP, -np.inf)), "dims": (X, Y, Z)}
    first, rebound = [], []
    pad = np.pad(vol.astype(np.int32), 1)
    for _ in range(rounds):
        legs = hc.sample_legs(normal, rng)
        nk = dirs[np.maximum(k, 0)]
        mq = stored_margin(mP)
        rec = _one_kind(P, legs, nk, np.where(has, mq, np.nan), sdf, event, (X, Y, Z))
        first.append(rec)
        # one rebound from every first leg that ends in a Hit: the bounce of k_bounce's opening half around the hit voxel's normal
        hit = rec["end"] == HIT
        iv = rec["voxel"][hit]
        x, y, z = iv[:, 0] + 1, iv[:, 1] + 1, iv[:, 2] + 1
        g = np.stack([pad[z, y, x + 1] - pad[z, y, x - 1], pad[z, y + 1, x] - pad[z, y - 1, x], pad[z + 1, y, x] - pad[z - 1, y, x]], axis=1)
        bn = (-hc._normalize(g.astype(F))).astype(F)
        start = ((rec["pos"][hit] + legs[hit]) + bn * F(2.0)).astype(F)
        rd = hc.sample_legs(bn, rng)
        with np.errstate(invalid="ignore"):
            m = np.where(has, mq, np.nan)[hit] + ((start.astype(np.float64) - P[hit].astype(np.float64)) * nk[hit]).sum(axis=1)
        rebound.append(_one_kind(start, rd, nk[hit], m, sdf, event, (X, Y, Z)))
    for name, recs in (("first", first), ("rebound", rebound)):
        out[name] = {key: np.concatenate([r[key] for r in recs]) for key in recs[0]}
    return out


def _one_kind(start, d, nk, m, sdf, event, dims):
    dn = (d.astype(np.float64) * nk).sum(axis=1)
    with np.errstate(invalid="ignore"):
        ok_dir = (np.abs(d).min(axis=1) >= 2.0 ** -10) & ~np.isnan(d).any(axis=1)
    _, armed, need = rules(m, dn, ok_dir, dims, 0, -FIELD_MIN)  # (J = 0: the lowest threshold on d . n_k any candidate has)
    end, steps, fired, near, pos, voxel = march(start, d, sdf, event, need)
    return dict(m=m, dn=dn, ok_dir=ok_dir, need=need, end=end, steps=steps, fired=fired, near=near, pos=pos, voxel=voxel)


def grants(rec, dims, J, D):
    """the rules with candidate J / D on recorded marches: a dict of counts.  (`fired` was recorded with the march's own `need`, which
    does not depend on J or D; a smaller J or D only arms fewer marches and accepts fewer of the steps at which they fire.)"""
    at_once, armed, _ = rules(rec["m"], rec["dn"], rec["ok_dir"], dims, J, D)
    deferred = armed & (rec["fired"] > 0) & (rec["fired"] <= J)
    saved = np.where(deferred, rec["steps"] - rec["fired"], 0)
    return dict(n=len(rec["m"]), at_once=int(at_once.sum()), wrong_at_once=int((at_once & (rec["end"] != EXIT)).sum()),
                armed=int(armed.sum()), deferred=int(deferred.sum()), wrong_deferred=int((deferred & (rec["end"] != EXIT)).sum()),
                steps_before=float(rec["fired"][deferred].mean()) if deferred.any() else 0.0,
                steps=int(rec["steps"].sum()), near=int(rec["near"].sum()),
                saved_at_once=int(rec["steps"][at_once].sum()), near_at_once=int(rec["near"][at_once].sum()),
                saved_deferred=int(saved.sum()), near_deferred=int(np.where(deferred, np.maximum(rec["near"] - rec["fired"], 0), 0).sum()))


def choose(res):
    """the table of candidates and the pair to build: the smallest J, then the smallest D, that keeps nine tenths of the deferred
    grants (first legs and rebounds together) found with J = 9 and D unbounded"""
    dims = res["dims"]
    count = lambda J, D: sum(grants(res[kind], dims, J, D)["deferred"] for kind in ("first", "rebound"))
    base = count(9, -FIELD_MIN)
    table = {(J, D): count(J, D) for J in J_CANDIDATES for D in D_CANDIDATES}
    pick = next(((J, D) for J in J_CANDIDATES for D in D_CANDIDATES if 10 * table[(J, D)] >= 9 * base), (9, -FIELD_MIN))
    return base, table, pick


def shell(n=64):
    """the `convex` scene of tests/test_gpu_hull_cert.py: volume, camera position and direction, frame"""
    c = (n - 1) / 2.0
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(F)
    r = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    vol = np.full((n, n, n), -1000, np.int16)
    vol[r < 0.42 * n] = 40
    vol[(r > 0.30 * n) & (r < 0.36 * n)] = 900
    pos = np.array([-30.0, 80.0, -40.0], F)
    d = np.array([(n - 1) / 2.0] * 3, F) - pos
    return vol, pos, (d / np.linalg.norm(d)).astype(F), (128, 96)


def report(res, J, D, out=sys.stdout):
    dims = res["dims"]
    m = res["hits"]["margin"]
    print("%d primary hits; margins at P: median %.2f, quartiles %.2f / %.2f voxels; %.1f %% of the hits carry a plane with -%g <= margin < 0" % (
        res["hits"]["n"], np.median(m), np.percentile(m, 25), np.percentile(m, 75), 100.0 * negative_share(res, D), D), file=out)
    print("rules with J = %d, D = %g: delta0 %g at once, %g deferred" % (J, D, hc.hull_delta0(*dims, 0.0), defer_delta0(*dims, J)), file=out)
    for kind in ("first", "rebound"):
        rec = res[kind]
        g = grants(rec, dims, J, D)
        ends = [100.0 * np.mean(rec["end"] == e) for e in (EXIT, HIT, NONE)]
        print("%-8s %8d marches, %.1f %% Exit / %.1f %% Hit / %.1f %% out of steps, %.1f literal steps per march, %.1f %% of them before a step of >= %d" % (
            kind, g["n"], ends[0], ends[1], ends[2], g["steps"] / max(g["n"], 1), 100.0 * g["near"] / max(g["steps"], 1), FAR_STEP), file=out)
        print("         at once  %5.1f %% granted, wrong %d, carrying %5.1f %% of the near-field steps and %5.1f %% of all steps" % (
            100.0 * g["at_once"] / max(g["n"], 1), g["wrong_at_once"], 100.0 * g["near_at_once"] / max(g["near"], 1), 100.0 * g["saved_at_once"] / max(g["steps"], 1)), file=out)
        print("         deferred %5.1f %% armed, %5.1f %% granted after %.1f steps, wrong %d, saving %5.1f %% of the near-field steps and %5.1f %% of all steps" % (
            100.0 * g["armed"] / max(g["n"], 1), 100.0 * g["deferred"] / max(g["n"], 1), g["steps_before"], g["wrong_deferred"],
            100.0 * g["near_deferred"] / max(g["near"], 1), 100.0 * g["saved_deferred"] / max(g["steps"], 1)), file=out)


def negative_share(res, D):
    """the share of the hits whose best plane lies in front of the start point by less than D voxels (what the per-hit word adds)"""
    m = res["hits"]["margin"]
    return float(np.mean((m < 0) & (m >= -D)))


def main():
    args = sys.argv[1:]
    n = int(args[0]) if args and args[0].isdigit() else 256
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 4
    from oracle import orc_ffi
    if "--shell" in args:
        n = 64 if not (args and args[0].isdigit()) else n
        vol, pos, d, (w, h) = shell(n)
        print("scene: the convex shell of tests/test_gpu_hull_cert.py, %d^3, %dx%d" % (n, w, h))
    else:
        w, h = (1920, 1080) if n >= 512 else (960, 544)
        vol = scene.phantom(n)
        pos, d = scene.close_camera(n) if "--close" in args else scene.default_camera(n)
        print("scene: phantom(%d), %dx%d, %s camera, default TF" % (n, w, h, "close" if "--close" in args else "default"))
    cache = args[args.index("--sdf-cache") + 1] if "--sdf-cache" in args else None
    sdf = np.load(cache) if cache and os.path.exists(cache) else orc_ffi.sdf_build(vol, orc_ffi.parse_tf(scene.tf_default_source()))[0]
    event = (vol >= 500) & (vol <= 1200)
    res = measure(vol, sdf, event, np.asarray(pos, F), np.asarray(d, F), w, h, rounds)
    base, table, (J, D) = choose(res)
    if "--rules" in args:  # the report alone, with the J and D given
        report(res, int(args[args.index("--rules") + 1]), float(args[args.index("--rules") + 2]))
        return
    report(res, 9, -FIELD_MIN)
    print("deferred grants (first legs + rebounds) by candidate, of %d with J = 9 and D = %g (the field's range):" % (base, -FIELD_MIN))
    print("   J \\ D " + "".join("%9g" % D_ for D_ in D_CANDIDATES) + "    delta0")
    for J_ in J_CANDIDATES:
        print("   %5d " % J_ + "".join("%8.1f%%" % (100.0 * table[(J_, D_)] / max(base, 1)) for D_ in D_CANDIDATES) + "    %g" % defer_delta0(*res["dims"], J_))
    print("the smallest J, then D, that keeps nine tenths: J = %d, D = %g" % (J, D))
    report(res, J, D)


if __name__ == "__main__":
    main()
