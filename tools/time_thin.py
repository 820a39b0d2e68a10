"""Time clwh_mask_thin and clwh_mask_points (csrc/thin_kernels.hip) with device events on the phantom's bone and air masks, in both
modes (curve skeleton with CLWH_THIN_KEEP_ENDS, and the topological kernel without), worklist and dense.

    python tools/time_thin.py [--size 512] [--repeats 5] [--out profiles/thin_timing.json]

The variants run ALTERNATELY, one call each per round, so that drift hits them alike; medians over the rounds.  Yardsticks of the same
run: clwh_mask_morph eroding the same mask by one voxel (three passes, no topology) and clwh_segment_grow of the bone from one seed
(the nearest sibling: tiles from a list, rounds read back in batches).  clwh_mask_thin waits for the device every four iterations, so
an event pair around it spans its kernels and those waits: the time a caller sees.
Beside the times the record holds, per thinning: iterations, count_in and count_out (exact, from the call), the kernels launched
(1 + 9 per enqueued iteration; iterations are enqueued four at a time) and the share of the sub-pass launches that belong to
iterations enqueued behind the last one (each reads one word and returns).  Whether a sub-pass of a live iteration found a candidate
of its parity is not recorded by the library and is not in the record."""
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

BATCH = 4  # kThinBatch of csrc/clwh_internal.hpp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="a JSON file; a run is appended to the runs it holds")
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n = args.size
    dims = (n, n, n)
    vol = scene.phantom(n)
    volume = ctx.image_from(vol)
    in_bone, in_air = (vol >= 500) & (vol <= 1200), (vol >= -1100) & (vol <= -900)
    masks = {"bone": ctx.buffer_from(scene.mask_pack(in_bone)), "air": ctx.buffer_from(scene.mask_pack(in_air))}
    seed = [int(v) for v in np.argwhere(in_bone[n // 2])[0][::-1]] + [n // 2]
    words = scene.mask_words_per_row(n) * n * n
    out = ctx.buffer(4 * words, np.uint32, (words,))
    row = {"n": n, "repeats": args.repeats, "bone_voxels": int(in_bone.sum()), "air_voxels": int(in_air.sum())}
    del in_bone, in_air
    results = {}

    def thin(name, mask, flags):
        def call():
            status, res = ctx.thin_mask_raw(mask, out, dims, flags)
            if status != ffi.OK:
                raise ffi.ClwhError(status, "clwh_mask_thin")
            results[name] = res.as_dict()
        return call

    def grow():
        status, _ = ctx.grow_region_raw(volume, [seed], 500, 1200, 0, None, out)
        if status != ffi.OK:
            raise ffi.ClwhError(status, "clwh_segment_grow")

    variants = {}
    for which, mask in masks.items():
        for mode, flags in (("ends", ffi.THIN_KEEP_ENDS), ("kernel", 0)):
            variants["thin_%s_%s" % (which, mode)] = thin("thin_%s_%s" % (which, mode), mask, flags)
        variants["thin_%s_ends_dense" % which] = thin("thin_%s_ends_dense" % which, mask, ffi.THIN_KEEP_ENDS | ffi.THIN_DENSE)
        variants["erode_%s_r1" % which] = lambda mask=mask: ctx.mask_morph(mask, dims, ffi.MORPH_ERODE, 1, out=out)
    variants["grow_bone_6"] = grow
    for k, (ms, all_ms) in alternating(stream, variants, args.repeats, args.warmup).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    for name, res in results.items():
        enqueued = -(-res["iterations"] // BATCH) * BATCH
        row[name] = dict(res, launches=1 + 9 * enqueued, idle_subpass_share=round((enqueued - res["iterations"]) / enqueued, 4))
    # the points of a skeleton and of a whole mask
    skeletons = {}
    for which, mask in masks.items():
        skeletons[which], _ = ctx.thin_mask(mask, dims, keep_ends=True)
    listed = {"points_%s_skeleton" % w: (lambda m=m: ctx.mask_points(m, dims)) for w, m in skeletons.items()}
    listed["points_bone_mask"] = lambda: ctx.mask_points(masks["bone"], dims)
    for k, (ms, all_ms) in alternating(stream, listed, args.repeats, args.warmup).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    ctx.finish()
    print(json.dumps(row), flush=True)
    for m in list(skeletons.values()) + list(masks.values()) + [out, volume]:
        m.release()
    ctx.destroy()
    if args.out:
        runs = json.load(open(args.out))["runs"] if os.path.exists(args.out) else []
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": runs + [row]}, f, indent=1)


if __name__ == "__main__":
    main()
