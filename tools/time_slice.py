"""Time clwh_render_slice (csrc/slice_kernels.hip) with device events on the phantom at 1920x1080: a thin axial and a thin oblique
slice, and 64- and 400-sample slabs (step 0.5) about the oblique plane in MAX / MIN / MEAN, each skipping and dense.

    python tools/time_slice.py [--size 512] [--repeats 10] [--out result.json]

Three builds of the walk run ALTERNATELY, one launch each per round, so that drift hits them alike: dense (CLWH_SLICE_DENSE), the
running-extreme skip over bricks only (a second context made with CLWH_TUNE_SLICE_COARSE=0) and the skip that asks the cell of 4^3
bricks first (the default).  Medians over the rounds.  Yardstick of the same run: the MEAN projection from the default pose.  The
first-call cost of the dilated tables is a skipping MAX slice after the derived data was dropped and the bricked copy rebuilt by a
dense slice, minus the median of the same slice afterwards."""
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

MODES = (("max", ffi.SLICE_MAX), ("min", ffi.SLICE_MIN), ("mean", ffi.SLICE_MEAN))


def oblique(n, W, H, slab, step):
    """a plane about the volume's centre, in-plane axes rotated by 0.6 and 0.35 rad, the volume's diagonal across the region's height"""
    a, b = 0.6, 0.35
    u = np.array([np.cos(a), np.sin(a) * np.cos(b), np.sin(a) * np.sin(b)])
    v = np.array([-np.sin(a), np.cos(a) * np.cos(b), np.cos(a) * np.sin(b)])
    nn = np.cross(u, v)
    sp = 1.2 * n / H
    origin = np.full(3, n / 2.0) - u * sp * W / 2 - v * sp * H / 2 - nn * (slab - 1) * step / 2
    return origin.astype(np.float32), (u * sp).astype(np.float32), (v * sp).astype(np.float32), nn.astype(np.float32)


def once(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def alternating(stream, fns, repeats, warmup):
    """{name: (median ms, all ms)} of the callables, run in turn `repeats` times after `warmup` rounds"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(once(stream, fn))
    return {k: (float(np.median(v)), [round(x, 4) for x in v]) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--slabs", default="64,400")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    os.environ["CLWH_TUNE_SLICE_COARSE"] = "0"
    try:
        ctx_bricks = ffi.Context(0, stream=stream.cuda_stream)  # the skip without the cells' table
    finally:
        del os.environ["CLWH_TUNE_SLICE_COARSE"]
    n, W, H = args.size, args.width, args.height
    vol = scene.phantom(n) if n <= 512 else scene.phantom_mt(n)
    volume = ctx.image_from(vol)
    volume_b = ctx_bricks.image_wrap(volume.device_ptr, (n, n, n), 1, np.int16)
    frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
    frame_b = ctx_bricks.image_wrap(frame.device_ptr, (W, H), 4, np.uint8)
    window = (0.0, 2000.0)
    row = {"n": n, "width": W, "height": H, "step": args.step, "repeats": args.repeats}

    def record(prefix, timings):
        for k, (ms, all_ms) in timings.items():
            row["%s_%s_ms" % (prefix, k)] = round(ms, 4)
            row["%s_%s_all_ms" % (prefix, k)] = all_ms

    pos, d = scene.default_camera(n)
    axial = scene.slice_plane((n, n, n), "axial", (n - 1) / 2.0, W, H)
    thin = oblique(n, W, H, 1, args.step)
    record("thin", alternating(stream, {
        "axial": lambda: ctx.render_slice(frame, volume, *axial, W, H, window=window),
        "oblique": lambda: ctx.render_slice(frame, volume, *thin, W, H, window=window),
        "projection_mean": lambda: ctx.render_projection(frame, volume, pos, d, W, H, mode=ffi.PROJ_MEAN, step=args.step, window=window),
    }, args.repeats, args.warmup))
    for slab in [int(s) for s in args.slabs.split(",")]:
        plane = oblique(n, W, H, slab, args.step)
        for name, mode in MODES:
            def run(c, v, f, flags):
                c.render_slice(f, v, *plane, W, H, mode=mode, slab_samples=slab, step=args.step, window=window, flags=flags)

            fns = {"dense": lambda: run(ctx, volume, frame, ffi.SLICE_DENSE), "skip_cells": lambda: run(ctx, volume, frame, 0)}
            if mode != ffi.SLICE_MEAN:
                fns["skip_bricks"] = lambda: run(ctx_bricks, volume_b, frame_b, 0)
            record("slab%d_%s" % (slab, name), alternating(stream, fns, args.repeats, args.warmup))
    # the first call that has to build the dilated tables
    plane = oblique(n, W, H, 64, args.step)

    def max_slab(flags):
        ctx.render_slice(frame, volume, *plane, W, H, mode=ffi.SLICE_MAX, slab_samples=64, step=args.step, window=window, flags=flags)

    first = []
    for _ in range(max(3, args.repeats // 2)):
        ctx.invalidate_derived(scene=False, camera=False, projection=True)
        max_slab(ffi.SLICE_DENSE)  # rebuilds the bricked copy; the dilated tables stay dropped
        first.append(once(stream, lambda: max_slab(0)))
    row["first_skipping_call_ms"] = round(float(np.median(first)), 4)
    row["dilated_tables_ms"] = round(float(np.median(first)) - row["slab64_max_skip_cells_ms"], 4)
    ctx.finish()
    ctx_bricks.finish()
    print(json.dumps(row), flush=True)
    for m in (frame_b, volume_b):
        m.release()
    ctx_bricks.destroy()
    for m in (frame, volume):
        m.release()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
