"""Time clwh_volume_filter (csrc/filter_kernels.hip) with device events on the phantom: every kind at the radii the tests use, out of
place; beside them, in the same loop, clwh_volume_apply_mask (one read and one write of the volume: the floor any filter can reach)
and the reference's bilateral_filter through clwh_launch (125 float taps).

    python tools/time_filter.py [--size 512] [--repeats 10] [--out profiles/filter_timing.json]

The variants run ALTERNATELY, one call each per round, so that drift hits them alike; medians over the rounds.  The record holds every
time, every filter as a multiple of the apply_mask floor, and for the line passes what one pass costs beside it: the single-axis
calls at radius 1, 3 and 16 along x, y and z."""
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
    ap.add_argument("--out", default=None, help="a JSON file; a run is appended to the runs it holds")
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n = args.size
    vol = scene.phantom(n)
    volume = ctx.image_from(vol)
    out = ctx.image([n, n, n], 1, np.int16, (n, n, n))
    words = scene.mask_words_per_row(n) * n * n
    mask = ctx.buffer_from(np.random.default_rng(1).integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32))
    bilateral = ctx.kernel("volume_filter.cl", "bilateral_filter")
    grid = [(n + 7) // 8 * 8] * 3
    row = {"n": n, "repeats": args.repeats}

    def call(kind, radius, weights=None, with_mask=False, dst=out):
        def run():
            status = ctx.filter_volume_raw(volume, dst, kind, radius, weights, mask if with_mask else None)
            if status != ffi.OK:
                raise ffi.ClwhError(status, "clwh_volume_filter")
        return run

    variants = {"apply_mask": lambda: ctx.apply_mask(volume, mask, out=out, fill=0),
                "bilateral_filter": lambda: bilateral.launch(grid, [4, 4, 4], volume, out)}
    for radius in ((1, 1, 1), (1, 1, 0), (0, 1, 1), (1, 0, 0), (0, 0, 0)):
        variants["median_%d%d%d" % radius] = call(ffi.FILTER_MEDIAN, radius)
    variants["median_111_masked"] = call(ffi.FILTER_MEDIAN, (1, 1, 1), with_mask=True)
    for kind, name in ((ffi.FILTER_MIN, "min"), (ffi.FILTER_MAX, "max")):
        for radius in ((1, 1, 1), (3, 0, 2), (16, 16, 16)):
            variants["%s_%d_%d_%d" % ((name,) + radius)] = call(kind, radius)
    gauss = {"gauss_1_1_0.6": scene.gaussian_weights((1.0, 1.0, 0.6)), "gauss_5.4": scene.gaussian_weights(5.4)}
    for name, w in gauss.items():
        variants["smooth_" + name] = call(ffi.FILTER_SMOOTH, [len(v) - 1 for v in w], w)
    variants["smooth_gauss_5.4_masked"] = call(ffi.FILTER_SMOOTH, [16] * 3, gauss["gauss_5.4"], with_mask=True)
    identity = np.array([4096], np.uint16)
    for r in (1, 3, 16):  # one pass: what a line pass costs beside the floor
        w = scene.gaussian_weights(r / 3.0)[0]
        assert len(w) == r + 1
        for axis, letter in enumerate("xyz"):
            radius = [0, 0, 0]
            radius[axis] = r
            one = [identity] * 3
            one[axis] = w
            variants["pass_smooth_%s_r%d" % (letter, r)] = call(ffi.FILTER_SMOOTH, radius, one)
            variants["pass_max_%s_r%d" % (letter, r)] = call(ffi.FILTER_MAX, radius)
    timed = alternating(stream, variants, args.repeats, args.warmup)
    floor = timed["apply_mask"][0]
    for k, (ms, all_ms) in timed.items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
        row[k + "_x_floor"] = round(ms / floor, 2)
    ctx.finish()
    print(json.dumps(row), flush=True)
    bilateral.release()
    for m in (mask, out, volume):
        m.release()
    ctx.destroy()
    if args.out:
        runs = json.load(open(args.out))["runs"] if os.path.exists(args.out) else []
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": runs + [row]}, f, indent=1)


if __name__ == "__main__":
    main()
