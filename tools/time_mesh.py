"""Time clwh_mesh_isosurface (csrc/mesh_kernels.hip) with device events on the phantom: the counting call and the whole extraction
(counting + filling, into buffers allocated once) at iso 300 and -200, each skipping and dense, and the first call after the bricked
copy was rebuilt.

    python tools/time_mesh.py [--size 512] [--repeats 10] [--out profiles/mesh_timing.json]

The call is synchronous (it waits for the device for its counts), so an event pair around it spans the host's wait as well: these are
the times a caller sees.  The variants run ALTERNATELY, one call each per round, so that drift hits them alike; medians over the
rounds.  Yardstick of the same run: k_iso_dilate + k_iso_coarse, the other full pass over the bricked copy, taken as a skipping
isosurface render after the derived data was dropped and the copy rebuilt by a projection, minus the median of the same render afterwards."""
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


def once(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def alternating(stream, fns, repeats, warmup):
    """{name: (median ms, all ms)} of the callables, run in turn `repeats` times after `warmup` rounds"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(once(stream, fn))
    return {k: (float(np.median(v)), [round(x, 4) for x in v]) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--isos", default="300,-200")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = ffi.Context(0, stream=stream.cuda_stream)
    n = args.size
    vol = scene.phantom(n) if n <= 512 else scene.phantom_mt(n)
    volume = ctx.image_from(vol)
    row = {"n": n, "repeats": args.repeats}

    def must(result):
        if result[0] != ffi.OK:
            raise ffi.ClwhError(result[0], "clwh_mesh_isosurface")
        return result

    for iso in [float(s) for s in args.isos.split(",")]:
        _, nv, nt = must(ctx.mesh_isosurface_raw(volume, iso))
        tag = "iso%g" % iso
        row[tag + "_vertices"], row[tag + "_triangles"] = nv, nt
        bufs = dict(positions=ctx.buffer(max(nv, 1) * 12), normals=ctx.buffer(max(nv, 1) * 12), keys=ctx.buffer(max(nv, 1) * 8),
                    triangles=ctx.buffer(max(nt, 1) * 12), vertex_capacity=nv, triangle_capacity=nt)

        def full(flags):
            must(ctx.mesh_isosurface_raw(volume, iso, flags=flags))
            must(ctx.mesh_isosurface_raw(volume, iso, flags=flags, **bufs))

        timings = alternating(stream, {
            "count_skip": lambda: must(ctx.mesh_isosurface_raw(volume, iso)),
            "count_dense": lambda: must(ctx.mesh_isosurface_raw(volume, iso, flags=ffi.MESH_DENSE)),
            "full_skip": lambda: full(0),
            "full_dense": lambda: full(ffi.MESH_DENSE),
        }, args.repeats, args.warmup)
        for k, (ms, all_ms) in timings.items():
            row["%s_%s_ms" % (tag, k)] = round(ms, 4)
            row["%s_%s_all_ms" % (tag, k)] = all_ms
        for k in ("positions", "normals", "keys", "triangles"):
            bufs[k].release()

    # the first extraction of a volume content: the bricked copy and the dilated tables are rebuilt inside the call
    first = []
    for _ in range(max(3, args.repeats // 2)):
        ctx.invalidate_derived(scene=False, camera=False, projection=True)
        first.append(once(stream, lambda: must(ctx.mesh_isosurface_raw(volume, 300.0))))
    row["first_count_after_rebuild_ms"] = round(float(np.median(first)), 4)

    # the yardstick: k_iso_dilate + k_iso_coarse at this size
    W, H = 256, 128
    frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
    pos, d = scene.default_camera(n)
    render = lambda flags: ctx.render_isosurface(frame, volume, pos, d, W, H, 300.0, flags=flags)
    steady = alternating(stream, {"render": lambda: render(0)}, args.repeats, args.warmup)["render"][0]
    built = []
    for _ in range(max(3, args.repeats // 2)):
        ctx.invalidate_derived(scene=False, camera=False, projection=True)
        ctx.render_projection(frame, volume, pos, d, W, H)  # rebuilds the bricked copy; the dilated tables stay dropped
        built.append(once(stream, lambda: render(0)))
    row["dilated_tables_ms"] = round(float(np.median(built)) - steady, 4)
    ctx.finish()
    print(json.dumps(row), flush=True)
    for m in (frame, volume):
        m.release()
    ctx.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
