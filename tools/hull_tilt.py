"""How many of the marches that no shipped hull rule reaches would a plane TILTED towards the march's direction end?  (DESIGN.md 4
item 14, restated in numpy and measured on the CPU before k_bounce is touched):
    python tools/hull_tilt.py [N] [--close] [--shell] [--rounds R] [--sdf-cache FILE]

tools/hull_defer.py restates the shipped rules: the plane k of the primary hit asked at once (item 12) or after at most J13 = 3 literal
steps by a march that starts up to 1.5 voxels behind it (item 13).  Here a march of fresh budget 70 that starts from a bounce and that
neither rule has granted or armed asks ANOTHER plane of the same table, found in closed form, exactly as k_bounce applies it:
    n0      the normal to tilt: the hit's plane normal n_k (where the hit has a word), or the bounce's own normal
    c       = d . n0,  t = delta(J) + 1/16 the target,  lambda = 0 if c >= t else -c + t sqrt(1 - c^2) / sqrt(1 - t^2)
    n'      = n0 + lambda d  (so that d . n' / |n'| = t),  k' its octahedral cell (`encode`, the inverse of hull_direction's cell centres)
    dn'     = d . n_k',  M' = n_k' . start - h_k'
    at once:   M' >= 0 and dn' >= delta0(70 - 5 steps)
    deferred:  0 < -M' <= D and dn' >= delta(J) = delta0(70 - 5 - J steps): ONE arming at the start, need = ceil(-M' / dn' (1 + 2^-19)),
               if need <= P (an armed lane cannot ask the macro-cell table before it has counted its path, which this restatement does
               not model: P keeps that path in the near field; P = 127 J, what J steps can count at most, is "unbounded");
               the march counts its path with the kernel's integer counter (the step byte's value per step: a step of 0.5 counts 0) and
               is granted when the count reaches `need`, if no event has ended it and it has taken at most J steps.
Item 13's armed marches share the kernel's one J (the step loop cannot afford a per-lane J), so with the rule on they are restated with
this J and delta(J) as well.  A grant is WRONG unless the literal march ends in Exit.
Printed per kind of march: grants, wrong grants, the step at which the deferred grants fire, steps saved (all / before the march's
first step of >= 12 voxels, where the macro-cell table cannot be asked yet); the table of candidates J x D; the pair chosen by item
13's rule (the smallest J, then D, that keeps nine tenths of the grants found with J = 20 and D unbounded), then the smallest path
limit P that keeps nine tenths of that pair's grants; n0 = the hit's plane normal
against n0 = the bounce's normal; and the tilted rule beside item 13's deferred rule against the tilted rule in its place."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_certificate as hc  # noqa: E402
import hull_defer as hd  # noqa: E402
from cl_volume_renderer_amd import scene  # noqa: E402

F = np.float32
GRID = hd.GRID
EXIT, HIT, NONE = hd.EXIT, hd.HIT, hd.NONE
FAR_STEP = hd.FAR_STEP
TARGET_MARGIN = 1.0 / 16.0   # kHullTiltMargin: the tilt aims this far above delta(J), so that the cell's own n_k' still qualifies
STEP_MAX = 127               # the largest step byte
J13, D13 = 3, 1.5            # kHullDeferSteps, kHullDeferDeficit: item 13 as shipped
J_CANDIDATES = (3, 6, 9, 12, 16, 20)
D_CANDIDATES = (1.5, 3.0, 6.0, np.inf)
P_CANDIDATES = (8, 16, 24, 32, 48, 64, 128)


def encode(n):
    """k_bounce's hull_cell: the octahedral cell of a direction [..., 3] of any length, in binary32 with the kernel's operations (the
    reciprocal is the only inexact one; any cell is safe, only the yield depends on it).  A NaN lands in cell 0."""
    n = np.asarray(n, F)
    s = ((np.abs(n[..., 0]) + np.abs(n[..., 1])) + np.abs(n[..., 2])).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (F(1.0) / s).astype(F)
        x, y, z = (n[..., 0] * r).astype(F), (n[..., 1] * r).astype(F), n[..., 2]
        u = np.where(z >= 0, x, np.copysign(F(1.0) - np.abs(y), x)).astype(F)
        v = np.where(z >= 0, y, np.copysign(F(1.0) - np.abs(x), y)).astype(F)
        i = np.floor((u * F(32.0) + F(32.0)).astype(F))
        j = np.floor((v * F(32.0) + F(32.0)).astype(F))
    i = np.nan_to_num(np.minimum(np.maximum(i, 0), GRID - 1), nan=0.0).astype(np.int64)
    j = np.nan_to_num(np.minimum(np.maximum(j, 0), GRID - 1), nan=0.0).astype(np.int64)
    return j * GRID + i


def tilt(n0, d, target):
    """(n', lambda): n0 turned towards d just far enough that d . n' / |n'| = target; lambda = 0 where c = d . n0 >= target"""
    n0, d = np.asarray(n0, np.float64), np.asarray(d, np.float64)
    c = (d * n0).sum(axis=-1)
    with np.errstate(invalid="ignore"):
        lam = np.where(c >= target, 0.0, -c + target * np.sqrt(np.maximum(1.0 - c * c, 0.0)) / np.sqrt(1.0 - target * target))
    return n0 + lam[..., None] * d, lam


def need_of(M, dn):
    """the path an armed march has to count (hull_defer.rules' expression)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.ceil(-M / dn * (1.0 + 2.0 ** -19))


def trace(start, d, sdf, event):
    """literal marches of 70 steps (hull_defer.march's loop).  Returns (how it ends, steps taken, steps taken before the first step of
    >= FAR_STEP voxels, position and voxel at the end, counts): counts[:, s] is the integer path counter after s steps where the march
    is still going and its position has a voxel, else -1 -- the step at which ANY `need` is reached can be read from it afterwards."""
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
    near = np.zeros(n, np.int64)
    seen_far = np.zeros(n, bool)
    counts = np.full((n, 71), -1, np.int16)
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
        if s < 70:
            counts[:, s] = np.where(alive & inside, count, -1)
        if not alive.any():
            break
    return end, steps, near, o, i, counts


def fired_at(counts, need):
    """the step after which the counter has reached `need` with the march still going (0: never)"""
    need = np.where(np.isfinite(need), need, 32767.0)
    reached = counts >= np.minimum(need, 32767.0)[:, None]
    reached[:, 0] = False
    s = reached.argmax(axis=1)
    return np.where(reached.any(axis=1), s, 0)


def measure(vol, sdf, event, pos, d, w, h, rounds=4, seed=1):
    """the marches: per kind ('first', 'rebound') start, direction, the hit's plane (index, margin as item 13 forms it), the bounce's
    normal and the literal march of every sample; 'table': (dirs, h_k)"""
    Z, Y, X = vol.shape
    o, cd, normal = hc.primary_hits(vol, sdf, event, pos, d, w, h)
    P = ((o + cd) + normal * F(2.0)).astype(F)
    dirs = hc.oct_directions(GRID, True)
    hk = hc.support_table(event, dirs) + hd.SLACK
    k, mP = hd.best_plane(P, dirs, hk)
    has = k >= 0
    mq = np.where(has, hd.stored_margin(mP), np.nan)
    rng = np.random.default_rng(seed)
    pad = np.pad(vol.astype(np.int32), 1)
    first, rebound = [], []
    for _ in range(rounds):
        legs = hc.sample_legs(normal, rng)
        rec = _one_kind(P, legs, k, mq, normal, sdf, event)
        first.append(rec)
        hit = rec["end"] == HIT
        iv = rec["voxel"][hit]
        x, y, z = iv[:, 0] + 1, iv[:, 1] + 1, iv[:, 2] + 1
        g = np.stack([pad[z, y, x + 1] - pad[z, y, x - 1], pad[z, y + 1, x] - pad[z, y - 1, x], pad[z + 1, y, x] - pad[z - 1, y, x]], axis=1)
        bn = (-hc._normalize(g.astype(F))).astype(F)
        start = ((rec["pos"][hit] + legs[hit]) + bn * F(2.0)).astype(F)
        rd = hc.sample_legs(bn, rng)
        nk = dirs[np.maximum(k[hit], 0)]
        with np.errstate(invalid="ignore"):
            m = mq[hit] + ((start.astype(np.float64) - P[hit].astype(np.float64)) * nk).sum(axis=1)
        rebound.append(_one_kind(start, rd, k[hit], m, bn, sdf, event))
    out = {"dims": (X, Y, Z), "table": (dirs, hk), "hits": len(o)}
    for name, recs in (("first", first), ("rebound", rebound)):
        out[name] = {key: np.concatenate([r[key] for r in recs]) for key in recs[0]}
    return out


def _one_kind(start, d, k, m, bn, sdf, event):
    end, steps, near, pos, voxel, counts = trace(start, d, sdf, event)
    with np.errstate(invalid="ignore"):
        ok_dir = (np.abs(d).min(axis=1) >= 2.0 ** -10) & ~np.isnan(d).any(axis=1)
    return dict(start=start, d=d, k=k, m=m, bn=bn, ok_dir=ok_dir, end=end, steps=steps, near=near, pos=pos, voxel=voxel, counts=counts)


def shipped(rec, table, dims, J):
    """items 12 and 13 on recorded marches, the deferred rule with the kernel's one J: (granted at once, armed, granted deferred, step)"""
    dirs, _ = table
    nk = dirs[np.maximum(rec["k"], 0)]
    dn = (rec["d"].astype(np.float64) * nk).sum(axis=1)
    at_once, armed, need = hd.rules(rec["m"], dn, rec["ok_dir"], dims, J, D13)
    fired = fired_at(rec["counts"], need)
    return at_once, armed, armed & (fired > 0) & (fired <= J), fired


def tilted(rec, table, dims, J, D, which, P=None):
    """the tilted rule on recorded marches, whatever else has granted them: (granted at once, armed, granted deferred, step, k')"""
    dirs, hk = table
    delta = hd.defer_delta0(*dims, J)
    n0 = rec["bn"].astype(np.float64)
    if which == "plane":  # the hit's plane normal where the hit has a word, else the bounce's own
        n0 = np.where((rec["k"] >= 0)[:, None], dirs[np.maximum(rec["k"], 0)], n0)
    npr, _ = tilt(n0, rec["d"], min(delta + TARGET_MARGIN, 0.99))
    k2 = encode(npr)
    nk2 = dirs[k2]
    dn = (rec["d"].astype(np.float64) * nk2).sum(axis=1)
    with np.errstate(invalid="ignore"):
        M = (rec["start"].astype(np.float64) * nk2).sum(axis=1) - hk[k2]
        at_once = rec["ok_dir"] & (M >= 0) & (dn >= hc.hull_delta0(*dims, 0.0))
        armed = rec["ok_dir"] & (M < 0) & (M >= -D) & (dn >= delta)
        armed &= need_of(M, dn) <= (J * STEP_MAX if P is None else P)
    fired = fired_at(rec["counts"], np.where(armed, need_of(M, dn), np.inf))
    return at_once, armed, armed & (fired > 0) & (fired <= J), fired, k2


def beside(rec, table, dims, J, D, which, replace=False, P=None):
    """what the tilted rule ADDS: marches that items 12 / 13 neither grant at once nor arm (replace: nor grant at once) -- a dict"""
    s_once, s_armed, s_def, s_fired = shipped(rec, table, dims, J)
    t_once, t_armed, t_def, t_fired, _ = tilted(rec, table, dims, J, D, which, P)
    free = ~s_once & (~s_armed if not replace else True)
    once, deferred = free & t_once, free & ~t_once & t_def
    if replace:
        s_def = np.zeros_like(s_def)
    saved = np.where(once, rec["steps"], 0) + np.where(deferred, rec["steps"] - t_fired, 0)
    near = np.where(once, rec["near"], 0) + np.where(deferred, np.maximum(rec["near"] - t_fired, 0), 0)
    s_saved = np.where(s_once, rec["steps"], 0) + np.where(s_def, rec["steps"] - s_fired, 0)
    granted = once | deferred
    return dict(n=len(rec["end"]), shipped_once=int(s_once.sum()), shipped_deferred=int(s_def.sum()), shipped_saved=int(s_saved.sum()),
                shipped_wrong=int(((s_once | s_def) & (rec["end"] != EXIT)).sum()),
                tried=int(free.sum()), once=int(once.sum()), armed=int((free & ~t_once & t_armed).sum()), deferred=int(deferred.sum()),
                wrong_once=int((once & (rec["end"] != EXIT)).sum()), wrong_deferred=int((deferred & (rec["end"] != EXIT)).sum()),
                exits_left=int((free & ~s_def & (rec["end"] == EXIT)).sum()), fired=t_fired[deferred],
                steps=int(rec["steps"].sum()), near=int(rec["near"].sum()), saved=int(saved.sum()), saved_near=int(near.sum()),
                granted=int(granted.sum()))


def report(res, J, D, which, out=sys.stdout, replace=False, P=None):
    dims, table = res["dims"], res["table"]
    print("rule: J = %d, D = %g, P = %s, n0 = %s, %s item 13's deferred rule; delta0 %g at once, delta(J) %g, target %g" % (
        J, D, "%d" % P if P is not None else "127 J", "the hit's plane normal" if which == "plane" else "the bounce's normal", "in place of" if replace else "beside",
        hc.hull_delta0(*dims, 0.0), hd.defer_delta0(*dims, J), hd.defer_delta0(*dims, J) + TARGET_MARGIN), file=out)
    for kind in ("first", "rebound"):
        g = beside(res[kind], table, dims, J, D, which, replace, P)
        pct = lambda a, b: 100.0 * a / max(b, 1)
        print("%-8s %8d marches, %d literal steps (%.1f %% before a step of >= %d); shipped rules: %.1f %% at once, %.1f %% deferred, wrong %d, %.1f %% of the steps" % (
            kind, g["n"], g["steps"], pct(g["near"], g["steps"]), FAR_STEP, pct(g["shipped_once"], g["n"]), pct(g["shipped_deferred"], g["n"]),
            g["shipped_wrong"], pct(g["shipped_saved"], g["steps"])), file=out)
        print("         tilted: %.1f %% of the marches reach the test, %d of them exit; granted at once %d (wrong %d), armed %d, granted deferred %d (wrong %d; %d armed lanes get there late or never): "
              "%.1f %% of the marches, %.1f %% of those tested, %.1f %% of the exits among them" % (
                  pct(g["tried"], g["n"]), g["exits_left"], g["once"], g["wrong_once"], g["armed"], g["deferred"], g["wrong_deferred"], g["armed"] - g["deferred"],
                  pct(g["granted"], g["n"]), pct(g["granted"], g["tried"]), pct(g["granted"], g["exits_left"])), file=out)
        f = g["fired"]
        if len(f):
            print("         deferred grants fire after a median %d steps (mean %.1f); by step 3 / 6 / 10 / 20: %.1f / %.1f / %.1f / %.1f %%" % (
                np.median(f), f.mean(), pct((f <= 3).sum(), len(f)), pct((f <= 6).sum(), len(f)), pct((f <= 10).sum(), len(f)), pct((f <= 20).sum(), len(f))), file=out)
        print("         steps saved: %.1f %% of all literal steps, %.1f %% of all counting only steps before the first step of >= %d" % (
            pct(g["saved"], g["steps"]), pct(g["saved_near"], g["steps"]), FAR_STEP), file=out)


def choose(res, which, out=sys.stdout):
    """the table of candidates and the pair to build: item 13's rule"""
    dims, table = res["dims"], res["table"]
    count = lambda J, D: sum(beside(res[kind], table, dims, J, D, which)["granted"] for kind in ("first", "rebound"))
    grid = {(J, D): count(J, D) for J in J_CANDIDATES for D in D_CANDIDATES}
    base = grid[(J_CANDIDATES[-1], np.inf)]
    print("grants the tilted rule adds (first legs + rebounds, n0 = %s), in %% of the %d with J = %d and D unbounded:" % (which, base, J_CANDIDATES[-1]), file=out)
    print("   J \\ D " + "".join("%9g" % D for D in D_CANDIDATES) + "    delta(J)", file=out)
    for J in J_CANDIDATES:
        print("   %5d " % J + "".join("%8.1f%%" % (100.0 * grid[(J, D)] / max(base, 1)) for D in D_CANDIDATES) + "    %g" % hd.defer_delta0(*dims, J), file=out)
    pick = next(((J, D) for J in J_CANDIDATES for D in D_CANDIDATES if 10 * grid[(J, D)] >= 9 * base), (J_CANDIDATES[-1], np.inf))
    print("the smallest J, then D, that keeps nine tenths: J = %d, D = %g" % pick, file=out)
    J, D = pick
    by_path = {P: sum(beside(res[kind], table, dims, J, D, which, P=P)["granted"] for kind in ("first", "rebound")) for P in P_CANDIDATES}
    print("   with that pair, by the path limit P: " + "  ".join("%d: %.1f%%" % (P, 100.0 * by_path[P] / max(grid[pick], 1)) for P in P_CANDIDATES), file=out)
    path = next((P for P in P_CANDIDATES if 10 * by_path[P] >= 9 * grid[pick]), J * STEP_MAX)
    print("the smallest P that keeps nine tenths of those: P = %d" % path, file=out)
    return (J, D, path), base


def main():
    args = sys.argv[1:]
    n = int(args[0]) if args and args[0].isdigit() else 256
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 4
    from oracle import orc_ffi
    if "--shell" in args:
        n = 64 if not (args and args[0].isdigit()) else n
        vol, pos, d, (w, h) = hd.shell(n)
        print("scene: the convex shell of tests/test_gpu_hull_cert.py, %d^3, %dx%d" % (n, w, h))
    else:
        w, h = (1920, 1080) if n >= 512 else (960, 544)
        vol = scene.phantom(n)
        pos, d = scene.close_camera(n) if "--close" in args else scene.default_camera(n)
        print("scene: phantom(%d), %dx%d, %s camera, default TF" % (n, w, h, "close" if "--close" in args else "default"))
    cache = args[args.index("--sdf-cache") + 1] if "--sdf-cache" in args else None
    sdf = np.load(cache) if cache and os.path.exists(cache) else orc_ffi.sdf_build(vol, orc_ffi.parse_tf(scene.tf_default_source()))[0]
    if cache and not os.path.exists(cache):
        np.save(cache, sdf)
    event = (vol >= 500) & (vol <= 1200)
    res = measure(vol, sdf, event, np.asarray(pos, F), np.asarray(d, F), w, h, rounds)
    print("%d primary hits, %d sampled first legs, %d rebounds" % (res["hits"], len(res["first"]["end"]), len(res["rebound"]["end"])))
    picks = {}
    for which in ("plane", "bounce"):
        picks[which] = choose(res, which)
    which = "plane" if picks["plane"][1] >= picks["bounce"][1] else "bounce"
    print("n0: the hit's plane normal finds %d grants, the bounce's normal %d (J = %d, D unbounded): kept: %s" % (
        picks["plane"][1], picks["bounce"][1], J_CANDIDATES[-1], which))
    J, D, P = picks[which][0]
    report(res, J, D, which, P=P)
    report(res, J, D, which, replace=True, P=P)
    print("as shipped (item 13 with its own J = %d), the shipped rules alone:" % J13)
    for kind in ("first", "rebound"):
        s_once, _, s_def, s_fired = shipped(res[kind], res["table"], res["dims"], J13)
        rec = res[kind]
        print("%-8s %.1f %% at once, %.1f %% deferred, %.1f %% of the steps" % (kind, 100.0 * s_once.mean(), 100.0 * s_def.mean(),
              100.0 * (np.where(s_once, rec["steps"], 0) + np.where(s_def, rec["steps"] - s_fired, 0)).sum() / max(rec["steps"].sum(), 1)))


if __name__ == "__main__":
    main()
