"""Time clwh_segment_label and clwh_labels_to_mask (csrc/label_kernels.hip) with device events on the phantom: the bone window (two
shells), the air window (one component of most of the volume: every count and box word is shared by the whole grid) and the
noisiest of a few narrow windows (the most components), each 6- and 26-connected; and a rank interval turned into a mask.

    python tools/time_label.py [--size 512] [--repeats 10] [--out profiles/label_timing.json]

clwh_segment_label is synchronous (it waits for the device once in the middle and once at the end), so an event pair around it spans
the host's waits as well: these are the times a caller sees.  The variants run ALTERNATELY, one call each per round, so that drift
hits them alike; medians over the rounds.  Yardsticks of the same run: clwh_segment_grow of the same windows from rank 1's first
voxel (one component, the worklist), clwh_sdf_build of the default transfer function and k_proj_repack (a streaming pass over the
volume), taken as the first projection after the derived data was dropped minus the median of the projections that follow."""
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

NOISE_CANDIDATES = ((38, 42), (30, 50), (0, 80), (-1002, -998), (895, 905))


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
    labels = ctx.buffer(4 * n * n * n, np.uint32, (n, n, n))
    table = ctx.buffer(48 * 16, np.uint8)
    words = scene.mask_words_per_row(n) * n * n
    mask = ctx.buffer(4 * words, np.uint32, (words,))
    row = {"n": n, "repeats": args.repeats}

    def label(lo, hi, flags):
        status, res = ctx.label_components_raw(volume, lo, hi, flags, None, None, labels, table, 16)
        if status != ffi.OK:
            raise ffi.ClwhError(status, "clwh_segment_label")
        return res

    # the noisiest window: one call each
    counts = {w: int(label(w[0], w[1], 0).n_components) for w in NOISE_CANDIDATES}
    noise = max(counts, key=counts.get)
    row["noise_candidates"] = {"%d..%d" % w: c for w, c in counts.items()}
    cases = {"bone": (500, 1200), "air": (-1100, -900), "noise": noise}
    row["windows"] = {k: list(v) for k, v in cases.items()}

    found, firsts = {}, {}
    variants = {}
    for case, (lo, hi) in cases.items():
        for name, flags in (("6", 0), ("26", ffi.LABEL_26)):
            def one(case=case, lo=lo, hi=hi, flags=flags, name=name):
                res = label(lo, hi, flags)
                found[(case, name)] = (int(res.n_components), int(res.n_voxels))
            one()
            rec = table.pull(np.uint8, (48 * 16,))[:48].view(ffi.LABEL_COMPONENT_DTYPE)[0]
            firsts[(case, name)] = (tuple(int(v) for v in rec["first"]), int(rec["count"]))
            variants["label_%s_%s" % (case, name)] = one
            seeds = [firsts[(case, name)][0]]
            gflags = ffi.GROW_26 if flags else 0

            def grow(seeds=seeds, lo=lo, hi=hi, gflags=gflags):
                status, _ = ctx.grow_region_raw(volume, seeds, lo, hi, gflags, None, mask)
                if status != ffi.OK:
                    raise ffi.ClwhError(status, "clwh_segment_grow")
            variants["grow_%s_%s" % (case, name)] = grow
    label(500, 1200, 0)  # (the labels the mask is made from)
    variants["labels_to_mask"] = lambda: ctx.labels_to_mask(labels, (n, n, n), 1, 1, mask)
    for k, (ms, all_ms) in alternating(stream, variants, args.repeats, args.warmup).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    for (case, name), (nc, nv) in found.items():
        row["%s_%s_components" % (case, name)], row["%s_%s_voxels" % (case, name)] = nc, nv
        row["%s_%s_rank1_count" % (case, name)] = firsts[(case, name)][1]
        grow_ms = row["grow_%s_%s_ms" % (case, name)]
        row["%s_%s_label_over_grow" % (case, name)] = round(row["label_%s_%s_ms" % (case, name)] / grow_ms, 3) if grow_ms > 0 else None

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
    for m in (frame, sdf, mask, table, labels, volume):
        m.release()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
