"""CPU checks of the overlay contract's restatement (tests/overlay_ref.py) and of what sits above the C ABI: the vectorised form against
the literal scalar loop, the blend's identities, the halo's origins against the slice reference's, the binding's names and struct
sizes, scene.overlay_palette, and -- with the reference alone -- the tally of every family tests/test_gpu_overlay.py compares on the
GPU, so that none of its comparisons can be empty.  The tests of the blend's identities, of the halo's origins and of words_of check
the reference and the test helpers against themselves: they say nothing about the library, whose coverage is the binding's and the
palette's tests here and tests/test_gpu_overlay.py."""
import ctypes as C
import os

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import overlay_ref as ovr
from tests import slice_ref as sr
from tests import test_gpu_overlay as go

F = np.float32


def test_ffi_names_the_values_of_the_header():
    assert (ffi.REGION_MASK, ffi.REGION_LABELS) == (ovr.MASK, ovr.LABELS) == (0, 1)
    assert (ffi.OVERLAY_FILL, ffi.OVERLAY_OUTLINE, ffi.OVERLAY_DENSE) == (ovr.FILL, ovr.OUTLINE, ovr.DENSE) == (1, 2, 4)
    assert "clwh_overlay_slice" in ffi.EXPORTED_SYMBOLS and "clwh_overlay_camera" in ffi.EXPORTED_SYMBOLS
    assert (C.sizeof(ffi.OverlayRegion), C.sizeof(ffi.OverlayPaint), C.sizeof(ffi.OverlaySliceDesc), C.sizeof(ffi.OverlayCameraDesc)) == (32, 40, 144, 128)
    assert (ffi.OverlaySliceDesc.region.offset, ffi.OverlaySliceDesc.paint.offset, ffi.OverlaySliceDesc.origin.offset) == (8, 40, 80)
    assert (ffi.OverlayCameraDesc.cam_pos.offset, ffi.OverlayCameraDesc.step.offset) == (80, 112)
    header = open(os.path.join(go.ROOT, "include", "clwh.h")).read()
    assert "CLWH_REGION_MASK = 0, CLWH_REGION_LABELS = 1" in header
    assert "CLWH_OVERLAY_FILL = 1," in header and "CLWH_OVERLAY_OUTLINE = 2," in header and "CLWH_OVERLAY_DENSE = 4 " in header
    assert "int clwh_overlay_slice(clwh_ctx *ctx, const clwh_overlay_slice_desc *desc);" in header
    assert "int clwh_overlay_camera(clwh_ctx *ctx, const clwh_overlay_camera_desc *desc);" in header


def test_overlay_palette():
    p = scene.overlay_palette(20)
    assert p.dtype == np.uint32 and p.shape == (20,) and len(set(p.tolist())) == 20 and np.all(p >> 24 == 255)
    assert p[0] == 230 | 25 << 8 | 75 << 16 | 255 << 24  # r in the lowest byte: the frame's byte order
    q = scene.overlay_palette(47)
    assert np.array_equal(q[:20], p) and np.array_equal(q[20:40], p) and np.array_equal(q[40:], p[:7])
    assert scene.overlay_palette(1).tolist() == [int(p[0])] and scene.overlay_palette(65536).shape == (65536,)
    # well separated: no two colours closer than 60 in rgb
    rgb = np.stack([p & 255, p >> 8 & 255, p >> 16 & 255], axis=1).astype(np.int64)
    d2 = ((rgb[:, None, :] - rgb[None, :, :]) ** 2).sum(axis=2) + np.eye(20, dtype=np.int64) * 10 ** 6
    assert d2.min() >= 60 ** 2, d2.min()
    for bad in (0, 65537, -1):
        with pytest.raises(ValueError):
            scene.overlay_palette(bad)


def test_blend_identities():
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, size=(4096, 4), dtype=np.uint8)
    col = rng.integers(0, 256, size=(4096, 4), dtype=np.uint8)
    assert np.array_equal(ovr.blend(px, col, np.zeros(4096, np.int64)), px)  # a = 0 keeps the bytes
    full = ovr.blend(px, col, np.full(4096, 255))
    assert np.array_equal(full[:, :3], col[:, :3]) and np.all(full[:, 3] == 255)  # a = 255 gives the colour, opaque
    for a in (1, 96, 128, 254):
        out = ovr.blend(px, col, np.full(4096, a)).astype(np.int64)
        lo, hi = np.minimum(px, col)[:, :3], np.maximum(px, col)[:, :3]
        assert np.all(out[:, :3] >= lo) and np.all(out[:, :3] <= hi) and np.all(out[:, 3] >= px[:, 3])
    # the overlay alpha of a pixel: A * alpha, rounded; A = 255 and alpha = 255 give 255, either 0 gives 0
    assert (255 * 255 + 127) // 255 == 255 and (0 * 255 + 127) // 255 == 0 and (255 * 96 + 127) // 255 == 96


def test_halo_origins_continue_the_slice_references():
    origin, du, dv, _ = go.oblique((64, 64, 64))
    w, h = 56, 40
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    assert np.array_equal(ovr.pixel_origins(origin, du, dv, xs.reshape(-1), ys.reshape(-1)), sr.pixel_origins(origin, du, dv, (w, h)))
    o = ovr.pixel_origins(origin, du, dv, np.array([-1, w]), np.array([-1, h]))
    assert np.array_equal(o[0], (origin + F(-1) * du) + F(-1) * dv) and np.array_equal(o[1], (origin + F(w) * du) + F(h) * dv)


def _sampled_pixels(case, count, seed):
    w, h = case["region_wh"]
    rng = np.random.default_rng(seed)
    pixels = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)}
    ids = go.reference_of(case)[1]
    ys, xs = np.nonzero(ids)
    for i in rng.permutation(len(xs))[:count]:  # pixels that show something ...
        pixels.add((int(xs[i]), int(ys[i])))
    for _ in range(count // 2):                 # ... and any others
        pixels.add((int(rng.integers(w)), int(rng.integers(h))))
    return sorted(pixels)


def _scalar_cases():
    phantom, odd, synthetic, edge = go.phantom_cases(), go.odd_cases(), go.synthetic_cases(), go.edge_cases()
    picked = [phantom[0], phantom[3], phantom[5], phantom[12], phantom[13], phantom[14], phantom[18]]
    picked += [odd[1], odd[6], odd[7], odd[9], odd[17], odd[24]]
    picked += [synthetic[1], synthetic[3], synthetic[5], synthetic[11], synthetic[-1]] + edge
    return picked


@pytest.mark.parametrize("index", range(21))
def test_scalar_loop_and_vectorised_form_agree(index):
    cases = _scalar_cases()
    assert len(cases) == 21
    c = cases[index]
    frame, ids, t_first, _ = go.reference_of(c)
    words = ovr.words_of(c["kind"], c["buffer"], c["dims"])
    shown = 0
    for x, y in _sampled_pixels(c, 10, index):
        px, ident, t = ovr.overlay_scalar(words, c["ray"], x, y, c["step"], c["palette"], c["frame_in"][y, x], c["flags"], c["fill_alpha"],
                                          c["outline_alpha"], c["id_range"])
        assert np.array_equal(frame[y, x], px) and ident == int(ids[y, x]), (x, y)
        assert np.array_equal(np.array(t, F).view(np.uint32), t_first[y, x].view(np.uint32)), (x, y)
        shown += ident != 0
    assert shown > 0 or not ids.any()


def test_words_of_ignores_a_masks_padding():
    rng = np.random.default_rng(9)
    for dims in ((70, 5, 3), (130, 4, 2), (5, 4, 3), (1, 1, 1), (64, 2, 2)):
        X, Y, Z = dims
        m = rng.integers(0, 2, size=(Z, Y, X)).astype(np.uint32)
        clean, dirty = go.buffer_words(ovr.MASK, m), go.buffer_words(ovr.MASK, m, garbage_seed=1)
        assert clean.size == dirty.size == scene.mask_words_per_row(X) * Y * Z
        assert (X % 64 == 0) == np.array_equal(clean, dirty)
        assert np.array_equal(ovr.words_of(ovr.MASK, dirty, dims), m) and np.array_equal(ovr.words_of(ovr.MASK, clean, dims), m)
    w = go.synthetic_words()
    assert np.array_equal(ovr.words_of(ovr.LABELS, go.buffer_words(ovr.LABELS, w), w.shape[::-1]), w) and int(w.max()) == 0xFFFFFFFF


ALL_BUT_HALO = [k for k in ovr.KINDS if k != "halo_only"]


def test_every_family_exercises_its_kinds():
    """the tallies test_gpu_overlay.py asserts after its GPU comparisons, here from the reference alone"""
    go.reference_tally(go.phantom_cases()).assert_kinds(ALL_BUT_HALO)
    go.reference_tally(go.odd_cases()).assert_kinds(("none", "empty", "first", "later", "outline", "fill_only", "skipped"))
    go.reference_tally(go.synthetic_cases() + go.edge_cases()).assert_kinds()
    # the kinds the issue names by where they come from
    edge = go.reference_tally(go.edge_cases())
    assert edge.counts["halo_only"] >= 30 and edge.counts["edge_plain"] >= 20, edge.counts
    close_ups = go.reference_tally(go.phantom_cases()[-4:])
    assert close_ups.counts["edge_plain"] >= 125, close_ups.counts
    assert go.reference_tally(go.phantom_cases()[3:4]).counts["rejected"] > 0
    wrap = go.reference_tally([c for c in go.phantom_cases() if c["ray"]["kind"] == "camera" and c["palette"].size == 1])
    assert wrap.counts["wrap"] > 0
    big = go.reference_tally([c for c in go.synthetic_cases() if c["id_range"][0] == 0x80000000])
    assert big.counts["first"] + big.counts["later"] > 0  # words >= 2^31 are drawn
    # slabs 1, 9 and 200 and both kinds of source appear in every family of planes
    for cases in (go.phantom_cases(), go.odd_cases()):
        assert {c["ray"]["n"] for c in cases if c["ray"]["kind"] == "plane"} >= {1, 9, 200}
        assert {c["kind"] for c in cases} == {ovr.MASK, ovr.LABELS} and {c["ray"]["kind"] for c in cases} == {"plane", "camera"}


def test_the_further_cases_show_what_they_are_about():
    c = go.tiling_case()
    stats = go.reference_of(c)[3]
    assert stats["outline"] > 50 and stats["fill_only"] > 50 and stats["later"] > 0
    ray = c["ray"]
    for v in (ray["origin"], ray["du"], ray["dv"]):
        assert np.array_equal(v * 8, np.round(v * 8))  # multiples of 1 / 8: the tiles' origins are exact
    assert sorted((x0, y0) for x0, y0, _, _ in go.TILES) == [(0, 0), (0, 16), (24, 0)]
    covered = np.zeros((40, 56), int)
    for x0, y0, w, h in go.TILES:
        assert w % 8 == 0 and h % 8 == 0
        covered[y0:y0 + h, x0:x0 + w] += 1
    assert np.all(covered == 1)
