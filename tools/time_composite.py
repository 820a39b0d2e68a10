"""Time clwh_render_composite (csrc/composite_kernels.hip) with device events: the dense walk and the brick-skipping walk, plain and
shaded, for the soft and the hard test table (tests/composite_ref.py), on the phantom at 1920x1080 from the default and close poses.

    python tools/time_composite.py [--sizes 512,1024] [--repeats 10] [--out result.json]

Yardstick of the same run: the dense MEAN projection (it reads the same kept samples with one gather each), and a dense composite of
the soft table with alpha_stop = +inf, which reads every kept sample too and adds the table gather.  k_comp_prefix's time is the
first composite after a table push minus the median of the composites that follow it.  Samples are counted exactly with the numpy
restatement of the contract on every 16th row ("read": up to termination; "kept": all)."""
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
from tests import composite_ref as cr  # noqa: E402

LUT_FIRST = -1024


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
    ap.add_argument("--alpha-stop", type=float, default=0.95)
    ap.add_argument("--count-samples", action="store_true", help="count the samples read with the numpy reference (slow at 1024^3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    W, H = args.width, args.height
    frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
    tables = {"soft": cr.soft_table(), "hard": cr.hard_table()}
    luts = {name: ctx.buffer_from(t) for name, t in tables.items()}
    results = []
    for n in [int(s) for s in args.sizes.split(",")]:
        vol = scene.phantom(n) if n <= 512 else scene.phantom_mt(n)
        volume = ctx.image_from(vol)
        for pose_name, (pos, d) in (("default", scene.default_camera(n)), ("close", scene.close_camera(n))):
            row = {"n": n, "pose": pose_name, "width": W, "height": H, "step": args.step, "alpha_stop": args.alpha_stop}

            def composite(name, flags, alpha_stop=args.alpha_stop):
                ctx.render_composite(frame, volume, pos, d, W, H, luts[name], LUT_FIRST, step=args.step, alpha_stop=alpha_stop,
                                     flags=flags)

            def measure(key, fn):
                for _ in range(args.warmup):
                    fn()
                ms, all_ms = timed(stream, fn, args.repeats)
                row[key + "_ms"] = round(ms, 4)
                row[key + "_all_ms"] = all_ms
                return ms

            measure("mean_dense", lambda: ctx.render_projection(frame, volume, pos, d, W, H, mode=ffi.PROJ_MEAN, step=args.step,
                                                                window=(0.0, 2000.0), dense=True))
            measure("soft_plain_dense_never_stop", lambda: composite("soft", ffi.COMP_DENSE, float("inf")))
            row["dense_never_stop_over_mean"] = round(row["soft_plain_dense_never_stop_ms"] / row["mean_dense_ms"], 3)
            for name in tables:
                for shade_name, shade in (("plain", 0), ("shaded", ffi.COMP_SHADE)):
                    for walk_name, dense in (("dense", ffi.COMP_DENSE), ("skip", 0)):
                        measure("%s_%s_%s" % (name, shade_name, walk_name), lambda: composite(name, shade | dense))
            steady = row["hard_plain_skip_ms"]

            def rebuild():
                luts["hard"].push(tables["hard"])  # a new content version: k_comp_prefix runs again
                composite("hard", 0)

            # (the push is a blocking copy before the first event's work is reached; only the launches lie between the events)
            first = []
            for _ in range(max(3, args.repeats // 2)):
                luts["hard"].push(tables["hard"])
                ms, _ = timed(stream, lambda: composite("hard", 0), 1)
                first.append(ms)
            row["k_comp_prefix_ms"] = round(float(np.median(first)) - steady, 4)
            if args.count_samples:
                rows = np.arange(0, H, 16)
                for name, t in tables.items():
                    st = cr.composite(vol, pos, d, (W, H), (W, H), t, LUT_FIRST, step=args.step, alpha_stop=args.alpha_stop, rows=rows)[4]
                    row["%s_samples_read_every_16th_row" % name] = st["read"]
                    row["kept_samples_every_16th_row"] = st["kept"]
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
