"""Time clwh_render_isosurface (csrc/isosurface_kernels.hip) with device events: the dense walk and the brick-skipping walk, above
and below, at refine 0 and 8, on the phantom at 1920x1080 from the default and close poses.

    python tools/time_isosurface.py [--sizes 512,1024] [--repeats 10] [--out result.json]

"above" is the shell from outside (iso 300: rays end at the first shell voxel or cross the whole volume).  "below" is CLWH_ISO_BELOW
at iso -1100, under the phantom's minimum: no ray ends, so the dense walk reads every kept sample -- eight gathers each -- and the
skipping walk steps over every brick.  Yardsticks of the same run: the dense MAX projection (the same kept samples with one gather
each) and the skipping MAX projection.  k_iso_dilate's time is the first isosurface after the derived data was dropped and the
bricked copy rebuilt by a projection, minus the median of the isosurfaces that follow it."""
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

ABOVE, BELOW = (300.0, 0), (-1100.0, ffi.ISO_BELOW)


def timed(stream, fn, repeats):
    """median ms of fn() over `repeats` runs, each between two events on the context's stream"""
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), [round(x, 4) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    W, H = args.width, args.height
    frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
    t_hit = ctx.buffer(W * H * 4, np.float32, (H, W))
    normal = ctx.buffer(W * H * 16, np.float32, (H, W, 4))
    results = []
    for n in [int(s) for s in args.sizes.split(",")]:
        vol = scene.phantom(n) if n <= 512 else scene.phantom_mt(n)
        volume = ctx.image_from(vol)
        for pose_name, (pos, d) in (("default", scene.default_camera(n)), ("close", scene.close_camera(n))):
            row = {"n": n, "pose": pose_name, "width": W, "height": H, "step": args.step}

            def isosurface(iso, flags, refine):
                ctx.render_isosurface(frame, volume, pos, d, W, H, iso, step=args.step, refine=refine, flags=flags, t_hit=t_hit,
                                      normal=normal)

            def projection(dense):
                ctx.render_projection(frame, volume, pos, d, W, H, mode=ffi.PROJ_MAX, step=args.step, window=(0.0, 2000.0), dense=dense)

            def measure(key, fn):
                for _ in range(args.warmup):
                    fn()
                ms, all_ms = timed(stream, fn, args.repeats)
                row[key + "_ms"] = round(ms, 4)
                row[key + "_all_ms"] = all_ms
                return ms

            measure("max_dense", lambda: projection(True))
            measure("max_skip", lambda: projection(False))
            for side_name, (iso, side) in (("above", ABOVE), ("below", BELOW)):
                for refine in (0, 8):
                    for walk_name, dense in (("dense", ffi.ISO_DENSE), ("skip", 0)):
                        measure("%s_refine%d_%s" % (side_name, refine, walk_name), lambda: isosurface(iso, side | dense, refine))
            row["below_dense_over_max_dense"] = round(row["below_refine0_dense_ms"] / row["max_dense_ms"], 3)
            steady = row["above_refine8_skip_ms"]
            first = []
            for _ in range(max(3, args.repeats // 2)):
                ctx.invalidate_derived(scene=False, camera=False, projection=True)
                projection(False)  # rebuilds the bricked copy; the dilated table stays dropped
                ms, _ = timed(stream, lambda: isosurface(ABOVE[0], ABOVE[1], 8), 1)
                first.append(ms)
            row["k_iso_dilate_ms"] = round(float(np.median(first)) - steady, 4)
            ctx.finish()
            row["hit_pixels_above"] = int((~np.isnan(t_hit.pull())).sum())
            print(json.dumps(row), flush=True)
            results.append(row)
        volume.release()
        del vol
    ctx.finish()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": results}, f, indent=1)


if __name__ == "__main__":
    main()
