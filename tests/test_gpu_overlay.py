"""clwh_overlay_slice and clwh_overlay_camera on the GPU against the numpy restatement of their contract (tests/overlay_ref.py), bit for
bit: the frame (pre-filled with random bytes, pixels outside the region included), ids and t_first.  The walk that steps over empty
bricks must equal the dense walk (CLWH_OVERLAY_DENSE) and both the reference.  Every family counts what it exercised (overlay_ref.KINDS)
so that no comparison is empty.  The inputs are lists of cases (the *_cases functions), chosen with the reference on the CPU;
tests/test_overlay_cpu.py asserts the tallies with the reference alone."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import label_ref as lr
from tests import overlay_ref as ovr
from tests import slice_ref as sr
from tests.test_gpu_slice import oblique
from tests.view_helpers import ROOT, F, bits, host_lib, pose

pytestmark = pytest.mark.gpu

INVALID_VALUE, BAD_NDRANGE, SIZE_MISMATCH = 1, 8, 9
FRAME, REGION = (64, 48), (56, 40)
BOTH = ovr.FILL | ovr.OUTLINE
ALL_IDS = (1, 0xFFFFFFFF)
SENTINEL = 0xDEADBEEF


class Tally:
    """what a family's comparisons exercised"""

    def __init__(self):
        self.counts = {k: 0 for k in ovr.KINDS}
        self.comparisons = 0

    def add(self, stats):
        for k in ovr.KINDS:
            self.counts[k] += stats[k]
        self.comparisons += 1

    def assert_kinds(self, kinds=ovr.KINDS):
        assert all(self.counts[k] > 0 for k in kinds) and self.comparisons > 0, self.counts


def buffer_words(kind, words, garbage_seed=None):
    """the uint32 words of the region buffer of word image `words`: a labelling's words, or a mask's layout with, for a garbage seed,
    random bits at x >= X and in the padding words"""
    if kind == ovr.LABELS:
        return np.ascontiguousarray(words, np.uint32).reshape(-1)
    Z, Y, X = words.shape
    packed = scene.mask_pack(words != 0)
    if garbage_seed is not None:
        wpr = scene.mask_words_per_row(X)
        rows = np.unpackbits(packed.astype("<u4").view(np.uint8).reshape(Z, Y, wpr * 4), axis=2, bitorder="little")
        rows[:, :, X:] = np.random.default_rng(garbage_seed).integers(0, 2, size=rows[:, :, X:].shape, dtype=np.uint8)
        packed = np.packbits(rows, axis=2, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)
    return packed


def frame_before(frame_wh, seed):
    """random bytes, with alpha 0 and 255 on many pixels"""
    fw, fh = frame_wh
    rng = np.random.default_rng(seed)
    frame = rng.integers(0, 256, size=(fh, fw, 4), dtype=np.uint8)
    pick = rng.integers(0, 3, size=(fh, fw))
    frame[..., 3] = np.where(pick == 0, 0, np.where(pick == 1, 255, frame[..., 3]))
    return frame


def _case(words, kind, ray, step=0.5, n_colours=20, flags=BOTH, fill_alpha=96, outline_alpha=255, id_range=ALL_IDS, garbage_seed=None,
          frame_wh=FRAME, region_wh=REGION, seed=1, palette=None):
    words = np.ascontiguousarray(words, np.uint32)
    if palette is None:
        palette = scene.overlay_palette(n_colours)
        palette[1::3] = (palette[1::3] & 0x00FFFFFF) | np.uint32(0x90000000)  # some colours with an alpha of their own
    return dict(words=words, kind=kind, dims=words.shape[::-1], buffer=buffer_words(kind, words, garbage_seed), ray=ray, step=step,
                palette=np.asarray(palette, np.uint32), flags=flags, fill_alpha=fill_alpha, outline_alpha=outline_alpha, id_range=id_range,
                frame_wh=frame_wh, region_wh=region_wh, frame_in=frame_before(frame_wh, seed))


def plane_case(words, kind, plane, n=1, step=0.5, **kw):
    origin, du, dv, normal = plane
    return _case(words, kind, ovr.plane(origin, du, dv, normal, n), step=step, **kw)


def camera_case(words, kind, pose_name, step=0.5, t_near=0.0, t_far=np.inf, **kw):
    pos, d = pose(pose_name, words.shape[::-1])
    return _case(words, kind, ovr.camera(pos, d, kw.get("frame_wh", FRAME), t_near, t_far), step=step, **kw)


def reference_of(case):
    """(frame, ids, t_first, stats) of a case, computed once -- from the BUFFER's words, so that a mask's padding is the reference's to ignore"""
    c = case
    if "_want" not in c:
        words = ovr.words_of(c["kind"], c["buffer"], c["dims"])
        assert np.array_equal(words, c["words"])
        c["_want"] = ovr.overlay(words, c["ray"], c["region_wh"], c["step"], c["palette"], c["frame_in"], c["flags"], c["fill_alpha"],
                                 c["outline_alpha"], c["id_range"])
    return c["_want"]


def reference_tally(cases):
    tally = Tally()
    for c in cases:
        tally.add(reference_of(c)[3])
    return tally


class Overlay:
    """a frame, ids and t_first on one context"""

    def __init__(self, ctx, frame_wh, region_wh):
        self.ctx, self.frame_wh, self.region_wh = ctx, frame_wh, region_wh
        (fw, fh), (w, h) = frame_wh, region_wh
        self.frame = ctx.image([fw, fh], 4, np.uint8, (fh, fw, 4))
        self.ids = ctx.buffer(w * h * 4, np.uint32, (h, w))
        self.t_first = ctx.buffer(w * h * 4, np.float32, (h, w))

    def call(self, source, palette, case, flags=None, ray=None, raw=False, **kw):
        """one call of the case's kind on whatever the frame holds; kw overrides the binding's arguments"""
        c = case
        ray = ray or c["ray"]
        w, h = self.region_wh
        args = dict(step=c["step"], flags=c["flags"] if flags is None else flags, fill_alpha=c["fill_alpha"], outline_alpha=c["outline_alpha"],
                    id_range=c["id_range"], ids=self.ids, t_first=self.t_first)
        if ray["kind"] == "plane":
            method = self.ctx.overlay_slice_raw
            before = (ray["origin"], ray["du"], ray["dv"], ray["normal"])
            args["slab_samples"] = ray["n"]
        else:
            method = self.ctx.overlay_camera_raw
            before = (ray["pos"], ray["dir"])
            args.update(t_near=ray["t_near"], t_far=ray["t_far"])
        args.update(kw)
        status = method(self.frame, source, c["kind"], c["dims"], palette, *before, w, h, **args)
        if not raw:
            assert status == 0, status
        return status

    def run(self, source, palette, case, flags=None):
        """(frame, ids, t_first) of the case's call over its frame_in"""
        self.frame.push(case["frame_in"])
        self.ids.push(np.full(self.ids.shape, SENTINEL, np.uint32))
        self.t_first.push(np.full(self.t_first.shape, SENTINEL, np.uint32))
        self.call(source, palette, case, flags)
        return self.frame.pull(), self.ids.pull(), self.t_first.pull()

    def release(self):
        for m in (self.frame, self.ids, self.t_first):
            m.release()


def check(got, want, what=""):
    """the whole frame's bytes, the ids and t_first's bit patterns"""
    assert np.array_equal(got[0], want[0]), "frame differs %s: %d pixels" % (what, int((got[0] != want[0]).any(axis=-1).sum()))
    assert np.array_equal(got[1], want[1]), "ids differ %s: %d pixels" % (what, int((got[1] != want[1]).sum()))
    bad = bits(got[2]) != bits(want[2])
    assert not bad.any(), "t_first differs %s: %d values, first at %s" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))


def _run_family(ctx, cases):
    """reference == skipping walk == dense walk for every case; returns the family's tally"""
    tally = Tally()
    outputs = {}
    for c in cases:
        key = (c["frame_wh"], c["region_wh"])
        if key not in outputs:
            outputs[key] = Overlay(ctx, *key)
        out = outputs[key]
        source, palette = ctx.buffer_from(c["buffer"]), ctx.buffer_from(c["palette"])
        want = reference_of(c)
        h, w = c["region_wh"][::-1]
        assert np.array_equal(want[0][h:], c["frame_in"][h:]) and np.array_equal(want[0][:, w:], c["frame_in"][:, w:])
        what = "dims %s kind %d %s step %r ids %s flags %d" % (c["dims"], c["kind"], c["ray"]["kind"], c["step"], c["id_range"], c["flags"])
        check(out.run(source, palette, c), want, "skipping, " + what)
        check(out.run(source, palette, c, c["flags"] | ovr.DENSE), want, "dense, " + what)
        tally.add(want[3])
        ctx.finish()
        source.release()
        palette.release()
    for out in outputs.values():
        out.release()
    return tally


SLABS = [(1, 0.5), (9, 0.37), (200, 0.5)]


@functools.lru_cache(maxsize=None)
def phantom_labels():
    """the 64^3 phantom's bone (2 components) and soft tissue (4 components) by rank"""
    vol = scene.phantom(64)
    bone, _, info_b = lr.label(vol, 300, 32767)
    soft, _, info_s = lr.label(vol, -200, 300)
    assert (info_b["n_components"], info_s["n_components"]) == (2, 4)
    return vol, bone, soft


@functools.lru_cache(maxsize=None)
def phantom_cases():
    _, bone, soft = phantom_labels()
    dims = (64, 64, 64)
    cases = []
    for n, step in SLABS:
        plane = oblique(dims, n=n, step=step)
        cases.append(plane_case(soft, ovr.LABELS, plane, n, step, seed=n))
        cases.append(plane_case(bone, ovr.LABELS, plane, n, step, seed=n + 1, flags=ovr.OUTLINE, outline_alpha=200))
        cases.append(plane_case((bone != 0).astype(np.uint32), ovr.MASK, plane, n, step, seed=n + 2, flags=ovr.FILL, fill_alpha=255))
        cases.append(plane_case(soft, ovr.LABELS, plane, n, step, seed=n + 3, id_range=(2, 3), n_colours=2))  # rank 1 rejected in front
    for name in ("default", "close"):
        cases.append(camera_case(soft, ovr.LABELS, name, seed=11, n_colours=1))                             # one colour: every other rank wraps
        cases.append(camera_case((bone != 0).astype(np.uint32), ovr.MASK, name, seed=12, garbage_seed=5))
        cases.append(camera_case(soft, ovr.LABELS, name, step=0.8, seed=13, id_range=(3, 4), flags=0))      # ids and t_first only
    cases.append(camera_case(bone, ovr.LABELS, "default", seed=14, t_near=70.0, t_far=100.0))                # the slab cuts the skull open
    # close-up planes: spacing 1 / 4 voxel, the region lies inside the soft tissue
    for a, b in ((0.6, 0.35), (0.0, 0.0)):
        cases.append(plane_case(soft, ovr.LABELS, oblique(dims, n=1, a=a, b=b, spacing=0.25), 1, 0.5, seed=15))
        cases.append(plane_case(soft, ovr.LABELS, oblique(dims, n=9, step=0.37, a=a, b=b, spacing=0.25), 9, 0.37, seed=16))
    return cases


def test_phantom_labellings_on_planes_and_cameras(gpu_ctx):
    _run_family(gpu_ctx, phantom_cases()).assert_kinds([k for k in ovr.KINDS if k != "halo_only"])


ODD_DIMS = [(70, 33, 45), (130, 20, 9), (5, 4, 3), (1, 1, 1)]


@functools.lru_cache(maxsize=None)
def odd_cases():
    """dims that are no multiple of a brick, mask rows of three 64-bit words, volumes smaller than a brick; masks carry garbage in
    their padding"""
    cases = []
    for i, dims in enumerate(ODD_DIMS):
        vol = scene.phantom(max(dims), dims=dims)
        labels = lr.label(vol, -200, 32767)[0]
        mask = (labels != 0).astype(np.uint32)
        for n, step in SLABS:
            plane = oblique(dims, n=n, step=step)
            cases.append(plane_case(labels, ovr.LABELS, plane, n, step, seed=20 + i))
            cases.append(plane_case(mask, ovr.MASK, plane, n, step, seed=30 + i, garbage_seed=i))
        cases.append(camera_case(labels, ovr.LABELS, "default", seed=40 + i))
        cases.append(camera_case(mask, ovr.MASK, "close", seed=50 + i, garbage_seed=10 + i))
    return cases


def test_odd_dims_and_masks_with_garbage_in_the_padding(gpu_ctx):
    _run_family(gpu_ctx, odd_cases()).assert_kinds(("none", "empty", "first", "later", "outline", "fill_only", "skipped"))


def synthetic_words():
    """48 x 40 x 24 words: boxes of 1, 5, 70 000, 2^31 and 2^32 - 1 in a volume of zeros, some touching, some nested"""
    w = np.zeros((24, 40, 48), np.uint32)
    w[2:20, 4:30, 3:20] = 1
    w[6:12, 10:20, 8:14] = 0x80000000
    w[4:22, 8:36, 24:44] = 70000
    w[10:16, 14:30, 20:30] = 5
    w[0:6, 30:40, 36:48] = 0xFFFFFFFF
    return w


@functools.lru_cache(maxsize=None)
def synthetic_cases():
    w = synthetic_words()
    dims = w.shape[::-1]
    cases = []
    for id_range in (ALL_IDS, (5, 0x80000000), (2, 69999), (0x80000000, 0xFFFFFFFF), (1, 1)):
        for n, step in SLABS:
            cases.append(plane_case(w, ovr.LABELS, oblique(dims, n=n, step=step), n, step, seed=60, id_range=id_range, n_colours=7))
        cases.append(camera_case(w, ovr.LABELS, "default", seed=61, id_range=id_range, n_colours=65536 if id_range[0] == 1 else 1))
    # a mask asked for ids 2 .. 3: a set bit is the word 1, so nothing is drawn
    cases.append(plane_case((w != 0).astype(np.uint32), ovr.MASK, oblique(dims, n=9, step=0.37), 9, 0.37, seed=62, id_range=(2, 3)))
    return cases


def edge_block():
    """64 x 48 x 4 words with a block of 3 that ends exactly at x = 56 and y = 40, the launched region's edges under an axis-aligned
    plane of spacing 1, and a block of 9 that runs on beyond them"""
    w = np.zeros((4, 48, 64), np.uint32)
    w[:, 8:40, 10:56] = 3
    w[:, 20:48, 30:64] = 9
    return w


@functools.lru_cache(maxsize=None)
def edge_cases():
    """pixel (x, y) is voxel (x, y, 1): the block of 3 has its last column at pixel x = 55 and its last row at y = 39 -- outline pixels
    whose only differing neighbour is the halo's; the block of 9 crosses the edge -- edge pixels that are no outline"""
    w = edge_block()
    plane = ((0.5, 0.5, 1.5), (1, 0, 0), (0, 1, 0), (0, 0, 1))
    return [plane_case(w, ovr.LABELS, plane, 1, 0.5, seed=70), plane_case(w, ovr.LABELS, plane, 3, 0.5, seed=71, flags=ovr.OUTLINE),
            plane_case((w == 3).astype(np.uint32), ovr.MASK, plane, 1, 0.5, seed=72, garbage_seed=3)]


def test_synthetic_words_filters_and_the_region_edge(gpu_ctx):
    tally = _run_family(gpu_ctx, synthetic_cases() + edge_cases())
    tally.assert_kinds()


# ---- a tiled call equals one call.  The API has no region offset: the region is the frame's top-left corner.  Tile (x0, y0) is
# therefore run with the origin moved to origin + x0 * du + y0 * dv -- every component a small multiple of 1 / 8, so that this sum and
# the kernel's (origin + x * du) + y * dv are exact and pixel (x, y) of the tile has the very ray of pixel (x0 + x, y0 + y) -- on a frame
# whose corner holds that part of the picture.
def tiling_case():
    _, _, soft = phantom_labels()
    plane = ((2.5, 30.0, 12.25), (0.75, 0.25, 0.5), (-0.25, 0.75, 0.125), (0.25, -0.5, 0.75))
    return plane_case(soft, ovr.LABELS, plane, 40, 0.5, seed=80)


TILES = [(0, 0, 24, 16), (24, 0, 32, 16), (0, 16, 56, 24)]  # x0, y0, width, height: whole 8 x 8 tiles that cover 56 x 40


def test_a_tiled_call_equals_one_call(gpu_ctx):
    ctx = gpu_ctx
    c = tiling_case()
    want = reference_of(c)
    assert want[3]["outline"] > 50 and want[3]["fill_only"] > 50
    source, palette = ctx.buffer_from(c["buffer"]), ctx.buffer_from(c["palette"])
    whole = Overlay(ctx, FRAME, REGION)
    check(whole.run(source, palette, c), want, "one call")
    ray = c["ray"]
    crossing = 0
    for x0, y0, w, h in TILES:
        moved = dict(ray, origin=(ray["origin"].astype(np.float64) + x0 * ray["du"].astype(np.float64) + y0 * ray["dv"].astype(np.float64)).astype(F))
        assert np.array_equal(ovr.pixel_origins(moved["origin"], ray["du"], ray["dv"], np.arange(w), 3),
                              ovr.pixel_origins(ray["origin"], ray["du"], ray["dv"], np.arange(x0, x0 + w), y0 + 3))
        tile = Overlay(ctx, (w, h), (w, h))
        tile_case = dict(c, frame_in=np.ascontiguousarray(c["frame_in"][y0:y0 + h, x0:x0 + w]))
        tile.frame.push(tile_case["frame_in"])
        tile.call(source, palette, tile_case, ray=moved)
        got = (tile.frame.pull(), tile.ids.pull(), tile.t_first.pull())
        check(got, tuple(a[y0:y0 + h, x0:x0 + w] for a in want[:3]), "tile %s" % ((x0, y0, w, h),))
        ids = want[1]
        if x0 > 0:
            crossing += int(((ids[y0:y0 + h, x0] != 0) & (ids[y0:y0 + h, x0] == ids[y0:y0 + h, x0 - 1])).sum())
        tile.release()
    assert crossing > 0  # a region runs across a tile border without an outline there
    ctx.finish()
    for m in (source, palette):
        m.release()
    whole.release()


def slice_then_overlay_case():
    vol, bone, _ = phantom_labels()
    n, step = 9, 0.37
    return vol, plane_case(bone, ovr.LABELS, oblique((64, 64, 64), n=n, step=step), n, step, seed=90)


def test_render_slice_followed_by_the_overlay(gpu_ctx):
    """the overlay over the frame clwh_render_slice has just written == the reference blend over the slice reference's frame"""
    ctx = gpu_ctx
    vol, c = slice_then_overlay_case()
    ray = c["ray"]
    w, h = REGION
    grey = sr.slice_view(vol, ray["origin"], ray["du"], ray["dv"], ray["normal"], REGION, modes=(sr.MAX,), slab_samples=ray["n"], step=c["step"],
                         window_cw=(0.0, 2000.0))[0][sr.MAX][0]
    frame_in = np.full((FRAME[1], FRAME[0], 4), 7, np.uint8)
    frame_in[:h, :w] = grey
    want = ovr.overlay(c["words"], ray, REGION, c["step"], c["palette"], frame_in)
    assert want[3]["outline"] > 20 and want[3]["fill_only"] > 20 and (grey[..., 3] == 0).sum() > 0 and len(np.unique(grey[..., 0])) > 10
    volume, source, palette = ctx.image_from(vol), ctx.buffer_from(c["buffer"]), ctx.buffer_from(c["palette"])
    out = Overlay(ctx, FRAME, REGION)
    out.frame.push(np.full((FRAME[1], FRAME[0], 4), 7, np.uint8))
    ctx.render_slice(out.frame, volume, ray["origin"], ray["du"], ray["dv"], ray["normal"], w, h, mode=sr.MAX, slab_samples=ray["n"], step=c["step"],
                     window=(0.0, 2000.0))
    out.call(source, palette, c)
    check((out.frame.pull(), out.ids.pull(), out.t_first.pull()), want, "slice, then overlay")
    ctx.finish()
    for m in (volume, source, palette):
        m.release()
    out.release()


def test_argument_errors(gpu_ctx):
    """every error clause: its exact status, and frame, ids and t_first untouched -- pulled and compared after each block of refused
    calls, before any accepted call draws into them"""
    ctx = gpu_ctx
    w = synthetic_words()
    dims = w.shape[::-1]
    c = plane_case(w, ovr.LABELS, oblique(dims, (64, 32), n=5), 5, 0.5, frame_wh=(64, 32), region_wh=(64, 32))
    cam = camera_case(w, ovr.LABELS, "default", frame_wh=(64, 32), region_wh=(64, 32))
    labels, palette = ctx.buffer_from(c["buffer"]), ctx.buffer_from(c["palette"])
    mask = ctx.buffer_from(buffer_words(ovr.MASK, w))
    out = Overlay(ctx, (64, 32), (64, 32))
    image3 = ctx.image_from(np.zeros((4, 8, 8), np.int16))
    small_out = ctx.buffer(64 * 32 * 4 - 4, np.uint32)
    small_labels = ctx.buffer(w.size * 4 - 4, np.uint32)
    small_mask = ctx.buffer(mask.nbytes - 8, np.uint32)
    small_palette = ctx.buffer(19 * 4, np.uint32)
    odd = ctx.buffer(w.size * 4 + 16, np.uint32)
    off4 = ctx.wrap(odd.device_ptr + 4, w.size * 4 + 8)   # 4-byte aligned, not 8
    off2 = ctx.wrap(odd.device_ptr + 2, w.size * 4 + 8)   # not 4-byte aligned

    frame_in = c["frame_in"]
    sentinel = np.full((32, 64), SENTINEL, np.uint32)

    def reset():
        out.frame.push(frame_in)
        out.ids.push(sentinel)
        out.t_first.push(sentinel)

    def untouched():
        return np.array_equal(out.frame.pull(), frame_in) and np.array_equal(out.ids.pull(), sentinel) and \
            np.array_equal(out.t_first.pull().view(np.uint32), sentinel)

    def checked_untouched(what):
        ctx.finish()
        assert untouched(), what

    def status(case, source=labels, pal=palette, kind=None, dims=None, frame=None, **kw):
        cc = dict(case, kind=case["kind"] if kind is None else kind, dims=case["dims"] if dims is None else dims)
        o = out
        if frame is not None:
            o = Overlay.__new__(Overlay)
            o.ctx, o.region_wh, o.frame, o.ids, o.t_first = ctx, out.region_wh, frame, out.ids, out.t_first
        return o.call(source, pal, cc, raw=True, **kw)

    # every refused call comes first, the outputs pulled after each block of them; the accepted calls next to the bounds draw, and follow
    reset()
    for case in (c, cam):
        which = case["ray"]["kind"]
        bad_values = [
            dict(frame=image3), dict(frame=labels), dict(source=None), dict(pal=None), dict(source=image3), dict(pal=image3),
            dict(source=off2), dict(pal=off2), dict(source=off4, kind=ovr.MASK), dict(ids=image3), dict(t_first=image3),
            dict(kind=2), dict(kind=-1), dict(flags=8), dict(flags=-1), dict(flags=1 << 16),
            dict(id_range=(0, 5)), dict(id_range=(6, 5)), dict(n_colours=0), dict(n_colours=65537), dict(fill_alpha=256), dict(outline_alpha=256),
            dict(dims=(0, 40, 24)), dict(dims=(48, 0, 24)), dict(dims=(48, 40, 0)), dict(dims=(1 << 31, 1, 1)), dict(dims=(1 << 16, 1 << 15, 1)),
            dict(step=0.0), dict(step=-1.0), dict(step=float("nan")), dict(step=float("inf")),
        ]
        if case is c:
            bad_values += [dict(slab_samples=0), dict(slab_samples=8193)]
        else:
            bad_values += [dict(t_near=2.0, t_far=1.0), dict(t_near=float("inf")), dict(t_near=float("nan")), dict(step=1e-9)]
        for kw in bad_values:
            assert status(case, **kw) == INVALID_VALUE, kw
        checked_untouched((which, "INVALID_VALUE"))
        for kw in (dict(width=0), dict(height=0), dict(width=12), dict(height=12), dict(width=72), dict(height=40), dict(width=65536)):
            wh = dict(width=64, height=32)
            wh.update(kw)
            cc = dict(case)
            o = Overlay.__new__(Overlay)
            o.ctx, o.region_wh, o.frame, o.ids, o.t_first = ctx, (wh["width"], wh["height"]), out.frame, out.ids, out.t_first
            assert o.call(labels, palette, cc, raw=True) == BAD_NDRANGE, kw
            assert o.call(labels, palette, cc, raw=True, step=0.0, ids=small_out) == INVALID_VALUE, kw  # a value error wins
            if wh["width"] in (12, 72):
                assert o.call(labels, palette, cc, raw=True, ids=small_out) == BAD_NDRANGE, kw            # a region error wins over a size error
        checked_untouched((which, "BAD_NDRANGE"))
        for kw in (dict(source=small_labels), dict(source=small_mask, kind=ovr.MASK), dict(pal=small_palette, n_colours=20), dict(ids=small_out),
                   dict(t_first=small_out), dict(dims=(48, 40, 25)), dict(dims=(49, 40, 24))):
            assert status(case, **kw) == SIZE_MISMATCH, kw
        checked_untouched((which, "SIZE_MISMATCH"))
    # the plane's own conditions: components that are not finite, and the reach with width and height (the halo is evaluated)
    ray = c["ray"]
    none = np.zeros(3, F)
    for name in ("origin", "du", "dv", "normal"):
        for bad in (float("nan"), float("inf")):
            v = np.array([0.25, 0.25, 0.25], F)
            v[1] = bad
            assert out.call(labels, palette, c, ray=dict(ray, **{name: v}), raw=True) == INVALID_VALUE, (name, bad)
    checked_untouched("a plane that is not finite")
    e = np.array([0, 1, 0], F)
    flat = dict(ray, du=none, dv=none, normal=none)
    assert out.call(labels, palette, c, ray=dict(flat, origin=e * F(2 ** 30)), raw=True) == INVALID_VALUE
    # |origin| + 64 |du| = 2^30: refused, though the slice's own bound, with 63, accepts it
    assert out.call(labels, palette, c, ray=dict(flat, origin=e * F(2 ** 24 * 0), du=e * F(2 ** 24)), raw=True) == INVALID_VALUE
    assert out.call(labels, palette, c, ray=dict(flat, dv=e * F(2 ** 25)), raw=True) == INVALID_VALUE            # 32 * 2^25
    assert out.call(labels, palette, c, ray=dict(flat, normal=e * F(2 ** 28)), step=1.0, raw=True) == INVALID_VALUE  # 4 * 2^28
    checked_untouched("the plane's reach")
    # a camera that is not finite
    for bad in (float("nan"), float("inf")):
        assert out.call(labels, palette, cam, ray=dict(cam["ray"], pos=np.array([bad, 0, 0], F)), raw=True) == INVALID_VALUE
    checked_untouched("a camera that is not finite")
    # NULL ctx and desc
    for call, desc in ((ffi.lib().clwh_overlay_slice, ffi.OverlaySliceDesc()), (ffi.lib().clwh_overlay_camera, ffi.OverlayCameraDesc())):
        assert call(ctx.h, None) == INVALID_VALUE and call(None, C.byref(desc)) == INVALID_VALUE and call(ctx.h, C.byref(desc)) == INVALID_VALUE
    checked_untouched("NULL handles")
    # just inside the bounds refused above, the calls are accepted: a palette of exactly n_colours, labels aligned to 4 bytes and not 8, a
    # mask of exactly its size; a reach one float below 2^30
    for case in (c, cam):
        assert status(case, pal=small_palette, n_colours=19) == 0 and status(case, source=off4) == 0 and status(case, source=mask, kind=ovr.MASK) == 0
    assert out.call(labels, palette, c, ray=dict(flat, origin=e * F(2 ** 30 - 64)), raw=True) == 0
    assert out.call(labels, palette, c, ray=dict(flat, origin=-e * F(1.0), du=e * F(2 ** 24 - 1)), raw=True) == 0
    ctx.finish()
    for m in (labels, palette, mask, image3, small_out, small_labels, small_mask, small_palette, off4, off2, odd):
        m.release()
    out.release()


def test_errors_leave_the_outputs_untouched_one_by_one(gpu_ctx):
    """one error of each kind, the outputs pulled after each"""
    ctx = gpu_ctx
    w = synthetic_words()
    c = plane_case(w, ovr.LABELS, oblique(w.shape[::-1], (64, 32), n=5), 5, 0.5, frame_wh=(64, 32), region_wh=(64, 32))
    labels, palette = ctx.buffer_from(c["buffer"]), ctx.buffer_from(c["palette"])
    out = Overlay(ctx, (64, 32), (64, 32))
    small = ctx.buffer(64 * 32 * 4 - 4, np.uint32)
    sentinel = np.full((32, 64), SENTINEL, np.uint32)
    out.frame.push(c["frame_in"])
    out.ids.push(sentinel)
    out.t_first.push(sentinel)
    narrow = Overlay.__new__(Overlay)
    narrow.ctx, narrow.region_wh, narrow.frame, narrow.ids, narrow.t_first = ctx, (60, 32), out.frame, out.ids, out.t_first
    for who, kw, want in ((out, dict(id_range=(0, 1)), INVALID_VALUE), (narrow, {}, BAD_NDRANGE), (out, dict(t_first=small), SIZE_MISMATCH)):
        assert who.call(labels, palette, c, raw=True, **kw) == want
        ctx.finish()
        assert np.array_equal(out.frame.pull(), c["frame_in"]) and np.array_equal(out.ids.pull(), sentinel)
        assert np.array_equal(out.t_first.pull().view(np.uint32), sentinel)
    for m in (labels, palette, small):
        m.release()
    out.release()


# ---- the layers above the C ABI

def _host_lib():
    u = C.c_uint
    return host_lib(
        clvr_host_render_slice=(C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]),
        clvr_host_render_projection=(C.c_void_p, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_float,
                                                  C.c_float, C.c_float]),
        clvr_host_grow_region=(None, [C.c_void_p, C.POINTER(u), u, C.c_int, C.c_int, C.c_int, C.c_void_p]),
        clvr_host_hold_mask=(None, [C.c_void_p]),
        clvr_host_label_components=(u, [C.c_void_p, C.c_int, C.c_int, C.c_int, u, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.c_void_p]),
        clvr_host_camera_direction=(None, [C.c_float, C.c_float, C.POINTER(C.c_float)]),
        clvr_host_overlay_slice=(C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, u, u, u, u]),
        clvr_host_overlay_camera=(C.c_void_p, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                               u, u, u, u]))


def test_host_mirror_overlays_equal_the_binding(gpu_ctx):
    """renderer::overlay_slice over render_slice's frame and overlay_camera over render_projection's, through libclvr_host.so, against
    the same calls of the binding on the regions the reference labels"""
    ctx = gpu_ctx
    dims, (W, H) = (48, 40, 36), (256, 128)
    vol = scene.phantom(48, dims=dims)
    env = scene.env_map(64, 32)
    ranks = lr.label(vol, 300, 32767)[0]
    seed = tuple(int(v) for v in np.argwhere(ranks == 1)[0][::-1])
    volume = ctx.image_from(vol)
    frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
    labels = ctx.buffer_from(ranks)
    mask = ctx.buffer_from(scene.mask_pack(ranks == 1))
    palette = ctx.buffer_from(scene.overlay_palette(20))
    L = _host_lib()
    h = L.clvr_host_create()

    def host_frame(ptr):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(1024, 2048, 4))[:H, :W].copy()

    try:
        L.clvr_host_load(h, vol.ctypes.data, dims[0], dims[1], dims[2], env.ctypes.data, 64, 32)
        result = (C.c_uint8 * 64)()
        L.clvr_host_grow_region(h, (C.c_uint * 3)(*seed), 1, 300, 32767, 0, result)
        L.clvr_host_hold_mask(h)
        n_comp, n_vox = C.c_ulonglong(), C.c_ulonglong()
        L.clvr_host_label_components(h, 300, 32767, 0, 8, C.byref(n_comp), C.byref(n_vox), (C.c_uint8 * (48 * 8))())
        assert n_comp.value == int(ranks.max()) and n_vox.value == int((ranks != 0).sum())
        # slices: the region mask (the grown component = rank 1), the held copy, the labelling with a rank filter
        for orientation, (name, position, n, step, source, flags, id_range) in enumerate((
                ("axial", 17.0, 1, 0.5, 0, BOTH, ALL_IDS), ("coronal", 20.25, 33, 0.37, 2, BOTH, (1, 2)), ("sagittal", 12.5, 16, 0.5, 1, ovr.OUTLINE, ALL_IDS))):
            L.clvr_host_render_slice(h, W, H, orientation, position, sr.MAX, n, step, 0.0, 2000.0, 0)
            host = host_frame(L.clvr_host_overlay_slice(h, W, H, source, orientation, position, n, step, flags, 96, 255, id_range[0], id_range[1]))
            plane = scene.slice_plane(dims, name, position, W, H, slab_samples=n, step=step)
            ctx.render_slice(frame, volume, *plane, W, H, mode=sr.MAX, slab_samples=n, step=step, window=(0.0, 2000.0))
            grey = frame.pull()
            region, kind = (labels, ovr.LABELS) if source == 2 else (mask, ovr.MASK)
            ctx.overlay_slice(frame, region, kind, dims, palette, *plane, W, H, slab_samples=n, step=step, flags=flags, id_range=id_range)
            mine = frame.pull()
            assert np.array_equal(host, mine), name
            words = ranks if source == 2 else (ranks == 1).astype(np.uint32)
            want = ovr.overlay(words, ovr.plane(*plane, n), (W, H), step, scene.overlay_palette(20), grey, flags, id_range=id_range)
            assert np.array_equal(mine, want[0]) and want[3]["outline"] > 20 and (mine != grey).any(axis=-1).sum() > 20, name
        # the camera of render_projection, over the renderer's whole frame: the view's centre is the frame's
        W, H = 2048, 1024
        whole = ctx.image([W, H], 4, np.uint8, (H, W, 4))
        pos, look = (C.c_float * 3)(*scene.default_camera(48)[0]), (C.c_float * 2)(0.9, 6.183)
        d = (C.c_float * 3)()
        L.clvr_host_camera_direction(look[0], look[1], d)
        L.clvr_host_render_projection(h, pos, look, W, H, 0, 0.0, 2000.0, 0.5)
        host = host_frame(L.clvr_host_overlay_camera(h, pos, look, W, H, 2, 0.5, BOTH, 96, 255, 1, 0xFFFFFFFF))
        ctx.render_projection(whole, volume, list(pos), list(d), W, H, mode=0, step=0.5, window=(0.0, 2000.0))
        grey = whole.pull()
        ctx.overlay_camera(whole, labels, ovr.LABELS, dims, palette, list(pos), list(d), W, H, step=0.5)
        mine = whole.pull()
        whole.release()
        assert np.array_equal(host, mine) and (mine != grey).any(axis=-1).sum() > 10000
    finally:
        L.clvr_host_destroy(h)
        for m in (frame, volume, labels, mask, palette):
            m.release()


def test_headless_show_overlays_instead_of_rewriting(tmp_path):
    dims, W, H = (64, 48, 40), 256, 128
    vol = scene.phantom(64, dims=dims)
    scene.write_nrrd(str(tmp_path / "v.nrrd"), vol)
    rng = np.random.default_rng(5)
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(rng.random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", str(W), str(H)]
    out = subprocess.run([exe, "--components=300,32767,show=both", "--slice=axial"] + files + [str(tmp_path / "p.ppm")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(s) for s in out.stdout.strip().splitlines()]
    ranks, _, info = lr.label(vol, 300, 32767)
    assert (lines[0]["mode"], lines[0]["n_components"], lines[0]["selected"]) == ("show", info["n_components"], [1, info["n_components"]])
    assert (lines[-1]["slice"], lines[-1]["overlay"], lines[-1]["frames"]) == ("axial", "both", 1)
    raw = open(tmp_path / "p.ppm", "rb").read()
    header = b"P6\n%d %d\n255\n" % (W, H)
    ppm = np.frombuffer(raw[len(header):], np.uint8).reshape(H, W, 3)[::-1]  # the PPM's first row is the frame's last
    plane = scene.slice_plane(dims, "axial", 19.5, W, H)
    grey = sr.slice_view(vol, *plane, (W, H), modes=(sr.MAX,), window_cw=(0.0, 4000.0))[0][sr.MAX][0]  # of the volume as loaded: not rewritten
    want = ovr.overlay(ranks, ovr.plane(*plane, 1), (W, H), 0.5, scene.overlay_palette(20), grey)
    assert np.array_equal(ppm, want[0][..., :3])
    coloured = (ppm[..., 0] != ppm[..., 1]) | (ppm[..., 1] != ppm[..., 2])
    assert want[3]["outline"] > 100 and want[3]["fill_only"] > 100 and coloured.sum() > 200 and (~coloured).sum() > 1000
    # a grown region on a camera view, outline only
    seed = np.argwhere(ranks == 1)[0][::-1]
    out = subprocess.run([exe, "--grow=%d,%d,%d,300,32767,show=outline" % tuple(seed), "--projection=max"] + files, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(s) for s in out.stdout.strip().splitlines()]
    assert lines[0]["mode"] == "show" and lines[0]["count"] == int((ranks == 1).sum()) and lines[-1]["overlay"] == "outline"
    for bad in ("--components=300,32767,show=both,keep", "--components=300,32767,fill=0,show", "--grow=1,1,1,0,5,show=thick", "--grow=1,1,1,0,5,remove,show"):
        assert subprocess.run([exe, bad, "--slice=axial"] + files, capture_output=True, text=True, timeout=120).returncode == 1, bad
    for view in ([], ["--mesh=300"]):  # show needs a slice or a camera view
        refused = subprocess.run([exe, "--components=300,32767,show"] + view + files, capture_output=True, text=True, timeout=120)
        assert refused.returncode == 1 and "show needs" in refused.stdout and "--components=LO,HI" in refused.stdout
