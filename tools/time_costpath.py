"""Time clwh_cost_geodesic, clwh_cost_from_field and Context.centerline (csrc/costpath_kernels.hip) with device events on the phantom: the
bone mask grown from one click, with that click as the only seed, 6- and 26-connected with the 10 / 14 / 17 chamfer.

    python tools/time_costpath.py [--size 512] [--repeats 10] [--out profiles/costpath_timing.json]

In the SAME run and loop: clwh_mask_geodesic of the mask with the chamfer as weights; clwh_cost_geodesic of the same mask with cost 1
everywhere and the chamfer as multipliers, which gives the same bytes, so the ratio is the price of carrying a cost; the same with
the centreline's cost (high at the wall, 1 from --radius voxels of depth on), which needs more rounds because a cheap detour lowers
tiles that an expensive direct route reached first -- the rounds are reported; clwh_cost_from_field for each source; and the whole
Context.centerline call from the click to the farthest voxel of the mask, with max_radius = --radius so that nothing is pulled.  The
geodesic calls are synchronous, so an event pair around them spans the host's waits as well: these are the times a caller sees.  The
variants run ALTERNATELY, one call each per round; medians over the rounds."""
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
    ap.add_argument("--radius", type=float, default=8.0, help="the centreline's largest radius of interest in voxels")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n = args.size
    dims = (n, n, n)
    vol = scene.phantom(n)
    volume = ctx.image_from(vol)
    row = {"library": os.path.basename(ffi.LIB_PATH), "n": n, "repeats": args.repeats, "radius": args.radius}

    bone = (vol[n // 2] >= 500) & (vol[n // 2] <= 1200)
    y, x = np.argwhere(bone)[0]
    seed = (int(x), int(y), n // 2)
    mask, res = ctx.grow_region(volume, [seed], 500, 1200)
    row["bone_count"] = int(res.count)
    chamfer = scene.geodesic_weights((1, 1, 1), 10)
    dist = ctx.buffer(4 * n ** 3, np.uint32, (n, n, n))
    labels = ctx.buffer(4 * n ** 3, np.uint32, (n, n, n))
    ones = ctx.buffer_from(np.ones((n, n, n), np.uint16))
    depth = ctx.mask_distance(mask, dims, scene.mask_weights((1, 1, 1)), to_clear=True)
    r_sq_max = scene.radius_sq(args.radius)
    shift = scene.centerline_shift(r_sq_max)
    table = scene.centerline_cost_table(r_sq_max >> shift)
    centre_cost = ctx.cost_from_field(depth, dims, table, 0, shift, ffi.COST_SRC_U32, mask)
    scratch_cost = ctx.buffer(2 * n ** 3, np.uint16, (n, n, n))
    gradient_table = np.maximum(1, 1000 - np.arange(1024)).astype(np.uint16)  # cheap along edges' ridges, a source like any other
    info = {}

    def must(status, where):
        if status != ffi.OK:
            raise ffi.ClwhError(status, where)

    def mask_geodesic(connectivity, tag):
        status, res = ctx.mask_geodesic_raw(mask, dims, [seed + (1,)], None, ffi.GEO_26 if connectivity == 26 else 0, chamfer, ffi.DIST_NONE,
                                            dist, labels)
        must(status, "clwh_mask_geodesic")
        info[tag] = {"rounds": int(res.rounds), "reached": int(res.reached), "max_dist": int(res.max_dist)}

    def cost_geodesic(cost, domain, connectivity, tag):
        status, res = ctx.cost_geodesic_raw(cost, dims, [seed + (1,)], domain, None, ffi.GEO_26 if connectivity == 26 else 0, chamfer,
                                            ffi.DIST_NONE, dist, labels)
        must(status, "clwh_cost_geodesic")
        info[tag] = {"rounds": int(res.rounds), "reached": int(res.reached), "max_dist": int(res.max_dist)}

    # the centreline's far end: the voxel of the mask farthest from the click
    mask_geodesic(26, "far_end")
    reached = dist.pull().reshape(-1)
    far = int(np.argmax(np.where(reached == ffi.DIST_NONE, 0, reached)))
    end = (far % n, (far // n) % n, far // (n * n))
    row["centerline_from"], row["centerline_to"] = list(seed), list(end)

    def centerline():
        points, count = ctx.centerline(mask, dims, seed, end, max_radius=args.radius)
        info["centerline"] = {"points": int(count), "length_voxels": round(scene.path_length(points), 2)}

    variants = {}
    for connectivity in (6, 26):
        tag = "_%d" % connectivity
        variants["mask_geodesic" + tag] = lambda k=connectivity, t=tag: mask_geodesic(k, "mask_geodesic" + t)
        variants["cost_geodesic_unit" + tag] = lambda k=connectivity, t=tag: cost_geodesic(ones, mask, k, "cost_geodesic_unit" + t)
        variants["cost_geodesic_centre" + tag] = lambda k=connectivity, t=tag: cost_geodesic(centre_cost, None, k, "cost_geodesic_centre" + t)
    variants["cost_field_u32"] = lambda: ctx.cost_from_field(depth, dims, table, 0, shift, ffi.COST_SRC_U32, mask, scratch_cost)
    variants["cost_field_value"] = lambda: ctx.cost_from_field(volume, dims, gradient_table, -1024, 2, ffi.COST_SRC_VALUE, None, scratch_cost)
    variants["cost_field_gradient"] = lambda: ctx.cost_from_field(volume, dims, gradient_table, 0, 8, ffi.COST_SRC_GRADIENT, None, scratch_cost)
    variants["centerline"] = centerline
    for k, (ms, all_ms) in alternating(stream, variants, args.repeats, args.warmup).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    row["info"] = info
    for tag in ("6", "26"):  # the ratios DESIGN.md quotes
        row["unit_cost_over_mask_geodesic_" + tag] = round(row["cost_geodesic_unit_%s_ms" % tag] / row["mask_geodesic_%s_ms" % tag], 2)
        row["centre_cost_over_unit_cost_" + tag] = round(row["cost_geodesic_centre_%s_ms" % tag] / row["cost_geodesic_unit_%s_ms" % tag], 2)
    ctx.finish()
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all_ms")}), flush=True)
    for m in (scratch_cost, centre_cost, depth, ones, labels, dist, mask, volume):
        m.release()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
