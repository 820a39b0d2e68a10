"""Time clwh_render_curved and clwh_curve_profile (csrc/curved_kernels.hip) with device events on the phantom: the reformat along the
centreline of the bone mask between tools/time_costpath.py's clicks, and that mask's section profile along it.

    python tools/time_curved.py [--size 512] [--repeats 10] [--out profiles/curved_timing.json]

In the SAME run and loop, one call each per round: the thin curved frame and a 64-sample MAX slab (skipping and dense) against
clwh_render_slice of the SAME region and slab on the oblique plane of tools/time_slice.py -- existing code, the yardstick; and
clwh_curve_profile, connected and not, against clwh_mask_statistics of the same mask.  The curved calls include staging their rows
(a copy of 36 bytes per row through page-locked memory); the profile calls are the raw asynchronous ones, into a buffer made once.  A
profile of one sample per station shows what staging the rows and launching costs by itself.  Medians over the rounds."""
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
from tools.time_slice import alternating, oblique  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radius", type=float, default=8.0, help="the centreline's largest radius of interest in voxels")
    ap.add_argument("--pixel", type=float, default=0.25, help="pixel, station and step size in voxels")
    ap.add_argument("--width", type=int, default=256, help="pixels across the reformat")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n = args.size
    dims = (n, n, n)
    vol = scene.phantom(n)
    volume = ctx.image_from(vol)
    row = {"library": os.path.basename(ffi.LIB_PATH), "n": n, "repeats": args.repeats, "pixel": args.pixel}

    # tools/time_costpath.py's clicks: the first bone voxel of the middle slice, and the voxel of its mask farthest from it
    bone = (vol[n // 2] >= 500) & (vol[n // 2] <= 1200)
    y, x = np.argwhere(bone)[0]
    seed = (int(x), int(y), n // 2)
    mask, res = ctx.grow_region(volume, [seed], 500, 1200)
    dist, labels, _ = ctx.mask_geodesic(mask, dims, [seed + (1,)], connectivity=26, weights=scene.geodesic_weights((1, 1, 1), 10))
    reached = dist.pull().reshape(-1)
    far = int(np.argmax(np.where(reached == ffi.DIST_NONE, 0, reached)))
    end = (far % n, (far // n) % n, far // (n * n))
    points, count = ctx.centerline(mask, dims, seed, end, max_radius=args.radius)
    row.update(bone_count=int(res.count), centerline_points=int(count), centerline_mm=round(scene.path_length(points), 2))

    W = args.width
    window = (0.0, 2000.0)
    thin_rows, s_mm, stations = scene.curve_frames(points, (1, 1, 1), W, pixel_mm=args.pixel, station_mm=args.pixel)
    slab_rows, _, _ = scene.curve_frames(points, (1, 1, 1), W, pixel_mm=args.pixel, station_mm=args.pixel, slab_samples=64, step_mm=0.5)
    H = len(thin_rows)
    row.update(width=W, height=H, stations=stations)
    frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
    thin_plane, slab_plane = oblique(n, W, H, 1, 0.5), oblique(n, W, H, 64, 0.5)

    def curved(rows, slab, flags=0):
        ctx.render_curved(frame, volume, rows, W, H, mode=ffi.SLICE_MAX, slab_samples=slab, step=0.5, window=window, flags=flags)

    def plane(p, slab, flags=0):
        ctx.render_slice(frame, volume, *p, W, H, mode=ffi.SLICE_MAX, slab_samples=slab, step=0.5, window=window, flags=flags)

    profile_rows, _, n_prof = scene.curve_frames(points, (1, 1, 1), 64, pixel_mm=args.pixel, station_mm=args.pixel, slab_samples=64)
    profile_rows = profile_rows[:n_prof]
    records = ctx.buffer(16 * n_prof, ffi.SECTION_RECORD_DTYPE, (n_prof,))

    def profile(flags):
        status = ctx.curve_profile_raw(mask, dims, profile_rows, n_prof, 64, 64, args.pixel, flags, records)
        if status != ffi.OK:
            raise ffi.ClwhError(status, "clwh_curve_profile")

    def profile_1x1():  # one sample per station: the staging of the rows and a kernel that has next to nothing to do
        status = ctx.curve_profile_raw(mask, dims, profile_rows, n_prof, 1, 1, args.pixel, 0, records)
        if status != ffi.OK:
            raise ffi.ClwhError(status, "clwh_curve_profile")

    variants = {
        "curved_thin": lambda: curved(thin_rows, 1),
        "slice_thin": lambda: plane(thin_plane, 1),
        "curved_slab64_max": lambda: curved(slab_rows, 64),
        "slice_slab64_max": lambda: plane(slab_plane, 64),
        "curved_slab64_max_dense": lambda: curved(slab_rows, 64, ffi.CURVED_DENSE),
        "slice_slab64_max_dense": lambda: plane(slab_plane, 64, ffi.SLICE_DENSE),
        "profile_connected": lambda: profile(ffi.PROFILE_CONNECTED),
        "profile_unconnected": lambda: profile(0),
        "profile_1x1": lambda: profile_1x1(),
        "mask_statistics": lambda: ctx.mask_statistics(volume, mask),
    }
    for k, (ms, all_ms) in alternating(stream, variants, args.repeats, args.warmup).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    row["curved_over_slice_thin"] = round(row["curved_thin_ms"] / row["slice_thin_ms"], 2)
    row["curved_over_slice_slab64_max"] = round(row["curved_slab64_max_ms"] / row["slice_slab64_max_ms"], 2)
    row["profile_connected_over_unconnected"] = round(row["profile_connected_ms"] / row["profile_unconnected_ms"], 2)
    profile(ffi.PROFILE_CONNECTED)
    got = records.pull()
    row["profile_stations"] = int(n_prof)
    row["profile_uncut_stations"] = int((got["border"] == 0).sum())
    row["profile_mean_count"] = round(float(got["count"].mean()), 1)
    ctx.finish()
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all_ms")}), flush=True)
    for m in (records, frame, labels, dist, mask, volume):
        m.release()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
