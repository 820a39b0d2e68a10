"""Time clwh_render_projection (csrc/projection_kernels.hip) with device events: k_proj_repack, and per mode the dense walk and the
brick-skipping walk, on the phantom at 1920x1080 from the default and close poses.

    python tools/time_projection.py [--sizes 512,1024] [--repeats 10] [--out result.json]

k_proj_repack's time is the first projection after clwh_ctx_invalidate_derived(CLWH_DERIVED_PROJECTION) minus the median of the
projections that follow it.  Dense kept samples are counted exactly with tests/projection_ref.kept_range (the contract's sample set);
samples/s is that count over the dense walk's median time."""
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
from tests import projection_ref as pr  # noqa: E402

MODES = {"max": ffi.PROJ_MAX, "min": ffi.PROJ_MIN, "mean": ffi.PROJ_MEAN}


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
    results = []
    for n in [int(s) for s in args.sizes.split(",")]:
        vol = scene.phantom(n) if n <= 512 else scene.phantom_mt(n)
        volume = ctx.image_from(vol)
        del vol
        for pose_name, (pos, d) in (("default", scene.default_camera(n)), ("close", scene.close_camera(n))):
            ka, kb = pr.kept_range(pos, d, (n, n, n), (W, H), (W, H), args.step)
            samples = int(np.maximum(kb - ka + 1, 0).sum())
            rays = int((kb >= ka).sum())

            def project(mode, dense):
                ctx.render_projection(frame, volume, pos, d, W, H, mode=mode, step=args.step, window=(0.0, 2000.0), dense=dense)

            row = {"n": n, "pose": pose_name, "width": W, "height": H, "step": args.step, "rays_with_samples": rays,
                   "dense_kept_samples": samples}
            for _ in range(args.warmup):
                project(ffi.PROJ_MAX, False)
            steady, _ = timed(stream, lambda: project(ffi.PROJ_MAX, False), args.repeats)

            def rebuild():
                ctx.invalidate_derived(scene=False, camera=False, projection=True)
                project(ffi.PROJ_MAX, False)

            first, _ = timed(stream, rebuild, max(3, args.repeats // 2))
            row["k_proj_repack_ms"] = round(first - steady, 4)
            for name, mode in MODES.items():
                for dense in ((True, False) if mode != ffi.PROJ_MEAN else (True,)):
                    for _ in range(args.warmup):
                        project(mode, dense)
                    ms, all_ms = timed(stream, lambda: project(mode, dense), args.repeats)
                    key = "%s_%s" % (name, "dense" if dense else "skip")
                    row[key + "_ms"] = round(ms, 4)
                    row[key + "_all_ms"] = all_ms
                    if dense:
                        row[key + "_gsamples_per_s"] = round(samples / (ms * 1e-3) / 1e9, 2)
            print(json.dumps(row), flush=True)
            results.append(row)
        volume.release()
    ctx.finish()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": results}, f, indent=1)


if __name__ == "__main__":
    main()
