"""Time clwh_mask_statistics and clwh_label_statistics (csrc/region_stats_kernels.hip) with device events on the phantom: the mask
path on the bone mask and on the air mask (most of the volume), with and without a 4096-bin histogram; the label path with capacity
256 and 65536 on the labels of the bone window, of the air window (one rank owns most of the volume: every lane wants the same record)
and of the noisiest of a few narrow windows (millions of specks: every run is distinct, and all but `capacity` ranks are dropped).

    python tools/time_region_stats.py [--size 512] [--repeats 10] [--out profiles/region_stats_timing.json]

The variants run ALTERNATELY, one call each per round, so that drift hits them alike; medians over the rounds.  Yardsticks of the SAME
run: clwh_segment_grow of the bone and the air window (its time includes k_grow_reduce, the one-region reduction that existed before)
and clwh_segment_label of each window, the cost of making the labels that are measured.  Beside each time the bytes the call has to
read once (mask path: mask + volume; label path: labels + volume; the neighbour rows are expected from L2) and what that makes per
second.  --experiments also times the two label-path designs that lost, CLWH_TUNE_LABEL_STATS=item and =direct, each in a context
of its own on the same buffers; `direct` on the air window is called once, not in the rounds (every part of every lane then goes to
one record in memory)."""
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
from tools.time_label import NOISE_CANDIDATES  # noqa: E402
from tools.time_mesh import alternating, once  # noqa: E402

CAPACITIES = (256, 65536)
HIST = (-1100, 1, 4096)


def must(status, where):
    if status != ffi.OK:
        raise ffi.ClwhError(status, where)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--experiments", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n = args.size
    dims = (n, n, n)
    vol = scene.phantom(n)
    volume = ctx.image_from(vol)
    words = scene.mask_words_per_row(n) * n * n
    comp_table = ctx.buffer(48 * 16, np.uint8)
    stats = ctx.buffer(104 * max(CAPACITIES), np.uint8)
    hist = ctx.buffer(8 * HIST[2], np.uint64, (HIST[2],))
    scratch_labels = ctx.buffer(4 * n * n * n, np.uint32, (n, n, n))
    scratch_mask = ctx.buffer(4 * words, np.uint32, (words,))
    row = {"n": n, "repeats": args.repeats, "hist": list(HIST)}

    def label(lo, hi, into):
        status, res = ctx.label_components_raw(volume, lo, hi, 0, None, None, into, comp_table, 16)
        must(status, "clwh_segment_label")
        return res

    counts = {w: int(label(w[0], w[1], scratch_labels).n_components) for w in NOISE_CANDIDATES}
    noise = max(counts, key=counts.get)
    windows = {"bone": (500, 1200), "air": (-1100, -900), "noise": noise}
    row["windows"] = {k: list(v) for k, v in windows.items()}

    labels, masks, firsts, variants = {}, {}, {}, {}
    for case, (lo, hi) in windows.items():
        labels[case] = ctx.buffer(4 * n * n * n, np.uint32, (n, n, n))
        res = label(lo, hi, labels[case])
        rec = comp_table.pull(np.uint8, (48 * 16,))[:48].view(ffi.LABEL_COMPONENT_DTYPE)[0]
        firsts[case] = tuple(int(v) for v in rec["first"])
        row[case + "_components"], row[case + "_voxels"], row[case + "_rank1_count"] = int(res.n_components), int(res.n_voxels), int(rec["count"])
        variants["label_" + case] = lambda lo=lo, hi=hi: label(lo, hi, scratch_labels)
        for cap in CAPACITIES:
            variants["label_stats_%s_%d" % (case, cap)] = lambda case=case, cap=cap: must(
                ctx.label_statistics_raw(volume, labels[case], stats, cap), "clwh_label_statistics")
        if case == "noise":
            continue
        masks[case] = ctx.labels_to_mask(labels[case], dims, 1, 0xFFFFFFFF)  # every voxel of the window
        variants["mask_stats_" + case] = lambda case=case: must(ctx.mask_statistics_raw(volume, masks[case])[0], "clwh_mask_statistics")
        variants["mask_stats_hist_" + case] = lambda case=case: must(
            ctx.mask_statistics_raw(volume, masks[case], hist, *HIST)[0], "clwh_mask_statistics")
        variants["grow_" + case] = lambda case=case, lo=lo, hi=hi: must(
            ctx.grow_region_raw(volume, [firsts[case]], lo, hi, 0, None, scratch_mask)[0], "clwh_segment_grow")

    others, wrapped = [], []
    if args.experiments:
        for mode in ("item", "direct"):
            os.environ["CLWH_TUNE_LABEL_STATS"] = mode
            other = ffi.Context(0, stream=stream.cuda_stream)  # the knob is read when a context is created
            others.append(other)
            v2 = other.image_wrap(volume.device_ptr, dims, 1, np.int16)
            s2 = other.wrap(stats.device_ptr, stats.nbytes)
            wrapped += [v2, s2]
            for case in windows:
                l2 = other.wrap(labels[case].device_ptr, labels[case].nbytes)
                wrapped.append(l2)
                for cap in CAPACITIES:
                    fn = lambda other=other, v2=v2, l2=l2, s2=s2, cap=cap: must(other.label_statistics_raw(v2, l2, s2, cap), "clwh_label_statistics")
                    name = "label_stats_%s_%d_%s" % (case, cap, mode)
                    if mode == "direct" and case == "air":
                        row[name + "_once_ms"] = round(once(stream, fn), 4)
                    else:
                        variants[name] = fn
        del os.environ["CLWH_TUNE_LABEL_STATS"]

    for k, (ms, all_ms) in alternating(stream, variants, args.repeats, args.warmup).items():
        row[k + "_ms"] = round(ms, 4)
        row[k + "_all_ms"] = all_ms
    mask_bytes, label_bytes = 4 * words + 2 * n ** 3, 4 * n ** 3 + 2 * n ** 3
    row["mask_path_bytes"], row["label_path_bytes"] = mask_bytes, label_bytes
    for k in list(row):
        if k.endswith("_ms") and not k.endswith("_all_ms") and (k.startswith("mask_stats") or k.startswith("label_stats")) and row[k] > 0:
            row[k[:-3] + "_GBps"] = round((mask_bytes if k.startswith("mask") else label_bytes) / row[k] / 1e6, 1)
    for case in windows:
        for cap in CAPACITIES:
            row["%s_%d_stats_over_label" % (case, cap)] = round(row["label_stats_%s_%d_ms" % (case, cap)] / row["label_%s_ms" % case], 3)
    ctx.finish()
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all_ms")}), flush=True)
    for m in wrapped:
        m.release()
    for other in others:
        other.destroy()
    for m in list(masks.values()) + list(labels.values()) + [scratch_mask, scratch_labels, hist, stats, comp_table, volume]:
        m.release()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
