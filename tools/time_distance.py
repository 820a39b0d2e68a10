"""Time clwh_mask_distance, clwh_mask_morph and clwh_mask_combine (csrc/distance_kernels.hip) with device events on the phantom:
the distance to its bone mask, to one single set voxel (the worst case of the outward search: sqrt(D / w) steps per voxel and axis,
D up to three times the volume's edge squared), the depth inside its air mask (TO_CLEAR), dilation and closing by balls of 2 and 8
voxels, and one combine.

    python tools/time_distance.py [--size 512] [--repeats 10] [--lines scan|search] [--out profiles/distance_timing.json]

All three calls are asynchronous; an event pair around a call spans the kernels it enqueued.  The variants run ALTERNATELY, one call
each per round, so that drift hits them alike; medians over the rounds.  Yardsticks of the same run: hipMemsetAsync of the map's
4 * X * Y * Z bytes (the floor of anything that writes the map once) and clwh_segment_label of the bone window (the nearest sibling)."""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--single-repeats", type=int, default=3, help="rounds of the single-voxel case, which is far slower than the others")
    ap.add_argument("--lines", choices=("scan", "search"), default=None,
                    help="CLWH_TUNE_DIST_LINES: every pass along y and z of clwh_mask_distance by this method instead of by the cap")
    ap.add_argument("--out", default=None, help="a JSON file; a run is appended to the runs it holds")
    args = ap.parse_args()
    if args.lines:
        os.environ["CLWH_TUNE_DIST_LINES"] = args.lines  # (read when the context is created)
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n = args.size
    dims = (n, n, n)
    vol = scene.phantom(n)
    volume = ctx.image_from(vol)
    bone = ctx.buffer_from(scene.mask_pack((vol >= 500) & (vol <= 1200)))
    air = ctx.buffer_from(scene.mask_pack((vol >= -1100) & (vol <= -900)))
    one = np.zeros((n, n, n), bool)
    one[0, 0, 0] = True
    single = ctx.buffer_from(scene.mask_pack(one))
    del one
    words = scene.mask_words_per_row(n) * n * n
    out = ctx.buffer(4 * words, np.uint32, (words,))
    dist = ctx.buffer(4 * n ** 3, np.uint32, (n, n, n))
    labels = ctx.buffer(4 * n ** 3, np.uint32, (n, n, n))
    row = {"n": n, "lines": args.lines or "scan", "repeats": args.repeats, "single_repeats": args.single_repeats,
           "bone_voxels": int(((vol >= 500) & (vol <= 1200)).sum()), "air_voxels": int(((vol >= -1100) & (vol <= -900)).sum())}
    hip = C.CDLL("libamdhip64.so")  # (already loaded by torch)
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]

    def memset():
        if hip.hipMemsetAsync(dist.device_ptr, 0, 4 * n ** 3, stream.cuda_stream) != 0:
            raise RuntimeError("hipMemsetAsync")

    def label():
        status, _ = ctx.label_components_raw(volume, 500, 1200, 0, None, None, labels, None, 0)
        if status != ffi.OK:
            raise ffi.ClwhError(status, "clwh_segment_label")

    variants = {
        "distance_bone": lambda: ctx.mask_distance(bone, dims, dist=dist),
        "distance_bone_aniso_49_49_625": lambda: ctx.mask_distance(bone, dims, (49, 49, 625), dist=dist),
        "distance_to_clear_air": lambda: ctx.mask_distance(air, dims, to_clear=True, dist=dist),
        "distance_bone_cap_64": lambda: ctx.mask_distance(bone, dims, cap=64, dist=dist),
        "dilate_bone_r2": lambda: ctx.mask_morph(bone, dims, ffi.MORPH_DILATE, 4, out=out),
        "dilate_bone_r8": lambda: ctx.mask_morph(bone, dims, ffi.MORPH_DILATE, 64, out=out),
        "close_bone_r2": lambda: ctx.mask_morph(bone, dims, ffi.MORPH_CLOSE, 4, out=out),
        "close_bone_r8": lambda: ctx.mask_morph(bone, dims, ffi.MORPH_CLOSE, 64, out=out),
        "combine_andnot": lambda: ctx.mask_combine(air, bone, ffi.MASK_ANDNOT, dims, out=out),
        "memset_map": memset,
        "label_bone_6": label,
    }
    for k, (ms, all_ms) in alternating(stream, variants, args.repeats, args.warmup).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    slow = {"distance_single_voxel": lambda: ctx.mask_distance(single, dims, dist=dist)}
    for k, (ms, all_ms) in alternating(stream, slow, args.single_repeats, 1).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    ctx.finish()
    print(json.dumps(row), flush=True)
    for m in (labels, dist, out, single, air, bone, volume):
        m.release()
    ctx.destroy()
    if args.out:
        runs = json.load(open(args.out))["runs"] if os.path.exists(args.out) else []
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": runs + [row]}, f, indent=1)


if __name__ == "__main__":
    main()
