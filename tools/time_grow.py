"""Time clwh_segment_grow and clwh_volume_apply_mask (csrc/grow_kernels.hip) with device events on the phantom: the bone window from a
seed in the skull, 6- and 26-connected, worklist and dense; the air window from a corner voxel (the largest component); the round count
of each; and the mask applied out of place.

    python tools/time_grow.py [--size 512] [--repeats 10] [--out profiles/grow_timing.json]

clwh_segment_grow is synchronous (it waits for the device after every batch of rounds), so an event pair around it spans the host's
waits as well: these are the times a caller sees.  The variants run ALTERNATELY, one call each per round, so that drift hits them
alike; medians over the rounds.  Yardsticks of the same run: clwh_sdf_build of the default transfer function (the other bit-parallel
search over the same volume; it ends with a host wait of its own) and k_proj_repack (a streaming pass over it), taken as the first
projection after the derived data was dropped minus the median of the projections that follow."""
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
from tools.time_mesh import alternating, once  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n = args.size
    vol = scene.phantom(n)
    volume = ctx.image_from(vol)
    out = ctx.image([n, n, n], 1, np.int16, (n, n, n))
    words = scene.mask_words_per_row(n) * n * n
    mask = ctx.buffer(4 * words, np.uint32, (words,))
    row = {"n": n, "repeats": args.repeats}

    bone = (vol[n // 2] >= 500) & (vol[n // 2] <= 1200)
    y, x = np.argwhere(bone)[0]
    cases = {"bone": ([(int(x), int(y), n // 2)], 500, 1200), "air": ([(0, 0, 0)], -1100, -900)}
    rounds = {}

    def grow(case, flags):
        seeds, lo, hi = cases[case]
        status, res = ctx.grow_region_raw(volume, seeds, lo, hi, flags, None, mask)
        if status != ffi.OK:
            raise ffi.ClwhError(status, "clwh_segment_grow")
        rounds[(case, flags)] = (int(res.rounds), int(res.count))

    variants = {}
    for case in cases:
        for name, flags in (("6", 0), ("26", ffi.GROW_26), ("6_dense", ffi.GROW_DENSE), ("26_dense", ffi.GROW_26 | ffi.GROW_DENSE)):
            variants["%s_%s" % (case, name)] = (lambda c=case, f=flags: grow(c, f))
    variants["apply_mask"] = lambda: ctx.apply_mask(volume, mask, out=out, fill=-32768)
    for k, (ms, all_ms) in alternating(stream, variants, args.repeats, args.warmup).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    for (case, flags), (r, count) in rounds.items():
        tag = "%s_%s%s" % (case, "26" if flags & ffi.GROW_26 else "6", "_dense" if flags & ffi.GROW_DENSE else "")
        row[tag + "_rounds"], row[tag + "_count"] = r, count

    # the yardsticks: the SDF build of the default transfer function, and k_proj_repack
    sdf = ctx.image([n, n, n], 1, np.int8, (n, n, n))
    tf = scene.tf_default_source()
    row["sdf_build_ms"] = round(alternating(stream, {"sdf": lambda: ctx.sdf_build(volume, tf, sdf)}, args.repeats, args.warmup)["sdf"][0], 4)
    W, H = 256, 128
    frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
    pos, d = scene.default_camera(n)
    project = lambda: ctx.render_projection(frame, volume, pos, d, W, H)
    steady = alternating(stream, {"p": project}, args.repeats, args.warmup)["p"][0]
    first = []
    for _ in range(max(3, args.repeats // 2)):
        ctx.invalidate_derived(scene=False, camera=False, projection=True)
        first.append(once(stream, project))
    row["k_proj_repack_ms"] = round(float(np.median(first)) - steady, 4)
    ctx.finish()
    print(json.dumps(row), flush=True)
    for m in (frame, sdf, mask, out, volume):
        m.release()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
