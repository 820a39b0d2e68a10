"""Time clwh_watershed (csrc/watershed_kernels.hip) with device events on the phantom: two clicks, one in the bone shell and one in the
ball inside it, over the cost from the gradient (scene.watershed_gradient_table(4096)), for 6 and 26 neighbours and for plateau_cap 0
and 65534.

    python tools/time_watershed.py [--size 512] [--repeats 10] [--out profiles/watershed_timing.json]

In the SAME run and loop: clwh_cost_geodesic on the same cost and seeds with every multiplier 1, the yardstick -- the sum along a path
where the watershed takes the maximum.  The calls are synchronous, so an event pair around them spans the host's waits as well: these
are the times a caller sees.  The variants run ALTERNATELY, one call each per round; medians over the rounds.  The rounds of the two
phases are reported apart: a call without `labels` runs phase 1 alone, and its rounds are taken from the whole call's."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (initialises the GPU before libclwhip.so does: tests/conftest.py)

from cl_volume_renderer_amd import ffi, scene  # noqa: E402
from tools.time_mesh import alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gmax", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n = args.size
    dims = (n, n, n)
    vol = scene.phantom(n)
    volume = ctx.image_from(vol)
    row = {"library": os.path.basename(ffi.LIB_PATH), "n": n, "repeats": args.repeats, "gmax": args.gmax}

    bone = (vol[n // 2] >= 500) & (vol[n // 2] <= 1200)
    y, x = np.argwhere(bone)[0]
    seeds = [(int(x), int(y), n // 2, 1), (n // 2 + int(0.15 * n), n // 2, n // 2, 2)]  # the shell; the ball inside it, beside the slab
    row["seeds"] = [list(s) for s in seeds]
    table, shift = scene.watershed_gradient_table(args.gmax)
    cost = ctx.cost_from_field(volume, dims, table, 0, shift, ffi.COST_SRC_GRADIENT)
    first = ctx.buffer(4 * n ** 3, np.uint32, (n, n, n))   # dist, level
    labels = ctx.buffer(4 * n ** 3, np.uint32, (n, n, n))
    info = {}

    def must(status, where):
        if status != ffi.OK:
            raise ffi.ClwhError(status, where)

    def watershed(connectivity, plateau, tag, with_labels=True):
        status, res = ctx.watershed_raw(cost, dims, seeds, None, None, ffi.GEO_26 if connectivity == 26 else 0, plateau, ffi.WATERSHED_LEVEL_MAX,
                                        labels if with_labels else None, first)
        must(status, "clwh_watershed")
        info[tag] = {"rounds": int(res.rounds), "reached": int(res.reached), "max_level": int(res.max_level)}

    def cost_geodesic(connectivity, tag):
        status, res = ctx.cost_geodesic_raw(cost, dims, seeds, None, None, ffi.GEO_26 if connectivity == 26 else 0, None, ffi.DIST_NONE, first,
                                            labels)
        must(status, "clwh_cost_geodesic")
        info[tag] = {"rounds": int(res.rounds), "reached": int(res.reached), "max_dist": int(res.max_dist)}

    variants = {}
    for connectivity in (6, 26):
        for plateau in (0, ffi.WATERSHED_PLATEAU_MAX):
            tag = "watershed_%d_plateau%d" % (connectivity, plateau)
            watershed(connectivity, plateau, tag + "_levels_only", False)  # phase 1's rounds
            variants[tag] = lambda k=connectivity, p=plateau, t=tag: watershed(k, p, t)
        tag = "cost_geodesic_%d" % connectivity
        variants[tag] = lambda k=connectivity, t=tag: cost_geodesic(k, t)
    for k, (ms, all_ms) in alternating(stream, variants, args.repeats, args.warmup).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    for connectivity in (6, 26):  # the figures README.md quotes
        for plateau in (0, ffi.WATERSHED_PLATEAU_MAX):
            tag = "watershed_%d_plateau%d" % (connectivity, plateau)
            level_rounds = info.pop(tag + "_levels_only")["rounds"]
            info[tag]["level_rounds"], info[tag]["label_rounds"] = level_rounds, info[tag]["rounds"] - level_rounds
            row[tag + "_over_cost_geodesic"] = round(row[tag + "_ms"] / row["cost_geodesic_%d_ms" % connectivity], 2)
    row["info"] = info
    ctx.finish()
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all_ms")}), flush=True)
    for m in (labels, first, cost, volume):
        m.release()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
