"""Time clwh_overlay_slice and clwh_overlay_camera (csrc/overlay_kernels.hip) with device events on the phantom at 1920x1080, step 0.5:
a thin axial overlay, a 64-sample slab about the oblique plane of tools/time_slice.py, and the camera overlay from the default and
the close pose -- of the bone labelling (clwh_segment_label of 300 .. 32767) and of the air mask (every component of -32768 .. -500
through clwh_labels_to_mask).

    python tools/time_overlay.py [--size 512] [--repeats 10] [--out result.json]

The camera's walk that steps over empty bricks -- its per-call occupancy build included, it is part of the call -- and its dense walk
(CLWH_OVERLAY_DENSE) run ALTERNATELY, one call each per round, so that drift hits them alike.  The plane's rays never step over a
brick, so the slab has no skipping leg: it is timed without and with the flag, `slab_dense` and `slab_dense_flag`, two
dense walks.  Medians over the rounds.  Yardsticks of the same run: the thin axial clwh_render_slice and the MAX
clwh_render_projection from the default pose."""
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
from time_slice import alternating, oblique  # noqa: E402  (tools/ is the script's directory)

BOTH = ffi.OVERLAY_FILL | ffi.OVERLAY_OUTLINE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--slab", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n, W, H = args.size, args.width, args.height
    dims = (n, n, n)
    vol = scene.phantom(n) if n <= 512 else scene.phantom_mt(n)
    volume = ctx.image_from(vol)
    frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
    palette = ctx.buffer_from(scene.overlay_palette(20))
    bone, bone_result, _ = ctx.label_components(volume, 300, 32767)
    air_labels, air_result, _ = ctx.label_components(volume, -32768, -500)
    air = ctx.labels_to_mask(air_labels, dims, 1, 0xFFFFFFFF)
    air_labels.release()
    row = {"n": n, "width": W, "height": H, "step": args.step, "slab": args.slab, "repeats": args.repeats,
           "bone_components": int(bone_result.n_components), "bone_voxels": int(bone_result.n_voxels), "air_voxels": int(air_result.n_voxels)}

    def record(prefix, timings):
        for k, (ms, all_ms) in timings.items():
            row["%s_%s_ms" % (prefix, k)] = round(ms, 4)
            row["%s_%s_all_ms" % (prefix, k)] = all_ms

    window = (0.0, 2000.0)
    pos, d = scene.default_camera(n)
    close_pos, close_d = scene.close_camera(n)
    axial = scene.slice_plane(dims, "axial", (n - 1) / 2.0, W, H)
    slab = oblique(n, W, H, args.slab, args.step)
    record("yardstick", alternating(stream, {
        "slice_thin_axial": lambda: ctx.render_slice(frame, volume, *axial, W, H, window=window),
        "projection_max": lambda: ctx.render_projection(frame, volume, pos, d, W, H, mode=ffi.PROJ_MAX, step=args.step, window=window),
    }, args.repeats, args.warmup))
    for name, source, kind in (("bone_labels", bone, ffi.REGION_LABELS), ("air_mask", air, ffi.REGION_MASK)):
        def plane(p, samples, flags):
            ctx.overlay_slice(frame, source, kind, dims, palette, *p, W, H, slab_samples=samples, step=args.step, flags=flags)

        def camera(p, direction, flags):
            ctx.overlay_camera(frame, source, kind, dims, palette, p, direction, W, H, step=args.step, flags=flags)

        record(name + "_thin_axial", alternating(stream, {"overlay": lambda: plane(axial, 1, BOTH), "ids_only": lambda: plane(axial, 1, 0)},
                                                 args.repeats, args.warmup))
        # the plane ships dense: both legs walk every kept sample, the second shows that the flag changes nothing
        record(name + "_slab", alternating(stream, {"dense": lambda: plane(slab, args.slab, BOTH),
                                                    "dense_flag": lambda: plane(slab, args.slab, BOTH | ffi.OVERLAY_DENSE)},
                                           args.repeats, args.warmup))
        record(name + "_camera_default", alternating(stream, {"skip": lambda: camera(pos, d, BOTH),
                                                              "dense": lambda: camera(pos, d, BOTH | ffi.OVERLAY_DENSE)}, args.repeats, args.warmup))
        record(name + "_camera_close", alternating(stream, {"skip": lambda: camera(close_pos, close_d, BOTH),
                                                            "dense": lambda: camera(close_pos, close_d, BOTH | ffi.OVERLAY_DENSE)},
                                                   args.repeats, args.warmup))
    ctx.finish()
    print(json.dumps(row), flush=True)
    for m in (frame, volume, palette, bone, air):
        m.release()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
