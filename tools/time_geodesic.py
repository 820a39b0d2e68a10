"""Time clwh_mask_geodesic (csrc/geodesic_kernels.hip) with device events on the phantom: the bone mask grown from one click, with that
click as the only seed, 6- and 26-connected with unit and with chamfer weights; the air mask from a corner voxel; and the split of the
bone mask (Context.split_mask: erode, label, grow back), whole and its geodesic step alone.

    python tools/time_geodesic.py [--size 512] [--repeats 10] [--out profiles/geodesic_timing.json] [--append]

Yardsticks of the SAME run: clwh_segment_grow of the same set from the same seed (the same reachability without distances, so the
natural floor: the same worklist, one bit per voxel where this call keeps 64) and clwh_mask_distance of the same mask (the other map
of 4 bytes per voxel).  clwh_mask_geodesic and clwh_segment_grow are synchronous, so an event pair around them spans the host's waits
as well: these are the times a caller sees.  The variants run ALTERNATELY, one call each per round; medians over the rounds.
CLWH_LIBRARY names another build of the library (another tile shape: -DCLVR_GEO_TILE_X/_Y/_Z); --append adds its row to the file."""
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
    ap.add_argument("--erode", type=float, default=2.0, help="the split's erosion radius in voxels")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n = args.size
    dims = (n, n, n)
    vol = scene.phantom(n)
    volume = ctx.image_from(vol)
    words = scene.mask_words_per_row(n) * n * n
    row = {"library": os.path.basename(ffi.LIB_PATH), "n": n, "repeats": args.repeats}

    bone = (vol[n // 2] >= 500) & (vol[n // 2] <= 1200)
    y, x = np.argwhere(bone)[0]
    cases = {"bone": ((int(x), int(y), n // 2), 500, 1200), "air": ((0, 0, 0), -1100, -900)}
    masks = {}
    for case, (seed, lo, hi) in cases.items():
        masks[case], res = ctx.grow_region(volume, [seed], lo, hi)
        row[case + "_count"] = int(res.count)
    scratch_mask = ctx.buffer(4 * words, np.uint32, (words,))
    dist = ctx.buffer(4 * n ** 3, np.uint32, (n, n, n))
    labels = ctx.buffer(4 * n ** 3, np.uint32, (n, n, n))
    info = {}

    def geodesic(case, connectivity, weights, tag):
        seed = cases[case][0]
        status, res = ctx.mask_geodesic_raw(masks[case], dims, [seed + (1,)], None, ffi.GEO_26 if connectivity == 26 else 0, weights,
                                            ffi.DIST_NONE, dist, labels)
        if status != ffi.OK:
            raise ffi.ClwhError(status, "clwh_mask_geodesic")
        info[tag] = {"rounds": int(res.rounds), "reached": int(res.reached), "max_dist": int(res.max_dist)}

    def grow(case, connectivity, tag):
        seed, lo, hi = cases[case]
        status, res = ctx.grow_region_raw(volume, [seed], lo, hi, ffi.GROW_26 if connectivity == 26 else 0, None, scratch_mask)
        if status != ffi.OK:
            raise ffi.ClwhError(status, "clwh_segment_grow")
        info[tag] = {"rounds": int(res.rounds), "count": int(res.count)}

    def split():
        out, parts = ctx.split_mask(volume, masks["bone"], dims, scene.radius_sq(args.erode, 1))
        info["split_bone"] = {"parts": parts}
        out.release()

    chamfer = scene.geodesic_weights((1, 1, 1), 10)
    variants = {}
    for case in cases:
        for connectivity in (6, 26):
            tag = "%s_%d" % (case, connectivity)
            variants["geodesic_" + tag] = lambda c=case, k=connectivity, t=tag: geodesic(c, k, None, "geodesic_" + t)
            variants["grow_" + tag] = lambda c=case, k=connectivity, t=tag: grow(c, k, "grow_" + t)
        variants["geodesic_%s_26_chamfer" % case] = lambda c=case: geodesic(c, 26, chamfer, "geodesic_%s_26_chamfer" % c)
        variants["distance_" + case] = lambda c=case: ctx.mask_distance(masks[c], dims, dist=dist)
    variants["split_bone"] = split
    for k, (ms, all_ms) in alternating(stream, variants, args.repeats, args.warmup).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    row["info"] = info
    for case in cases:  # the ratios the README quotes
        for tag in ("6", "26"):
            row["geodesic_over_grow_%s_%s" % (case, tag)] = round(row["geodesic_%s_%s_ms" % (case, tag)] / row["grow_%s_%s_ms" % (case, tag)], 2)
        row["geodesic_over_distance_%s_6" % case] = round(row["geodesic_%s_6_ms" % case] / row["distance_%s_ms" % case], 2)
    ctx.finish()
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all_ms")}), flush=True)
    for m in (labels, dist, scratch_mask, volume) + tuple(masks.values()):
        m.release()
    ctx.destroy()
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0), "runs": []}
        if args.append and os.path.exists(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc["runs"].append(row)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
