"""-m "not gpu": this project's host-side mirrors against the REFERENCE's own code.

oracle/ref/Makefile compiles the reference's app/hdre_loader.cpp (with the stb_image.h it vendors), app/nrrd_loader.cpp
and common.hpp's Position3D into oracle/_ref/libref_hostio.so.  tests/golden/make_ref_hostio_golden.py fed that library
the files / angles made by the generators below and stored both the input files and what the reference returned for
them in tests/golden/ref_hostio.npz; the tests below feed this project's loaders the same stored files and require
identical bytes.  The reference tree is not needed to run them."""
import ctypes as C
import os

import numpy as np
import pytest

from cl_volume_renderer_amd import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_hostio.npz")

HDR_CASES = [(True, 64, 17), (False, 64, 17), (True, 5, 3), (True, 300, 9), (True, 1024, 4)]


@pytest.fixture(scope="module")
def ref():
    """{key: array}: the input files (`<case>.in`, raw bytes) and the reference's answers for them"""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def mine():
    from tests.test_host_mirror import _host

    L = _host()
    L.clvr_host_hdr_probe.restype = C.c_longlong
    L.clvr_host_hdr_probe.argtypes = [C.c_char_p, C.POINTER(C.c_uint), C.c_void_p, C.c_longlong]
    L.clvr_host_nrrd_load.restype = C.c_longlong
    L.clvr_host_nrrd_load.argtypes = [C.c_char_p, C.POINTER(C.c_uint), C.POINTER(C.c_float), C.c_void_p, C.c_longlong]
    return L


# ---- the inputs (tests/golden/make_ref_hostio_golden.py writes them with these functions)


def hdr_input(path, rle, w, h):
    rng = np.random.default_rng(w * 7 + h)
    rgb = (rng.random((h, w, 3), dtype=np.float32) ** 3 * 6.0).astype(np.float32)
    rgb[:, : w // 3] = rgb[:, :1]
    rgb[0, 0] = 0.0
    rgb[-1, -1] = [1e-6, 300.0, 1.0]  # tiny and over-range values
    scene.write_hdr(path, scene.float_to_rgbe(rgb), rle=rle)
    return w, h


def png_cases():
    from tests.test_host_mirror import PNG_CASES

    return PNG_CASES


def png_input(path, color, depth, interlace):
    """every PNG flavour of tests/test_host_mirror.py"""
    from tests.test_host_mirror import _png_bytes

    rng = np.random.default_rng(color * 100 + depth + interlace)
    w, h = 37, 19
    ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[color]
    palette = trns = None
    if color == 3:
        n_pal = 1 << depth
        palette = rng.integers(0, 256, (n_pal, 3)).astype(np.uint8)
        trns = rng.integers(0, 256, n_pal // 2).astype(np.uint8).tolist()
        img = rng.integers(0, n_pal, (h, w, 1))
    else:
        img = rng.integers(0, 1 << depth, (h, w, ch))
    if color == 0:
        trns = [0, int(img[3, 7, 0])] if depth <= 8 else [int(img[3, 7, 0]) >> 8, int(img[3, 7, 0]) & 255]
    if color == 2:
        k = img[2, 9].tolist()
        trns = [k[0] >> 8, k[0] & 255, k[1] >> 8, k[1] & 255, k[2] >> 8, k[2] & 255]
    open(path, "wb").write(_png_bytes(img, color, depth, interlace, palette, trns))
    return w, h


def nrrd_volume():
    rng = np.random.default_rng(11)
    return rng.integers(-2000, 4000, (9, 14, 23)).astype(np.int16)


def nrrd_input(path, gz):
    vol = nrrd_volume()
    scene.write_nrrd(path, vol, use_gzip=gz)
    return vol


def anisotropic_nrrd_input(path):
    vol = np.arange(4 * 3 * 5, dtype=np.int16).reshape(4, 3, 5)
    hdr = ("NRRD0004\n# comment\ntype: short\ndimension: 3\nsizes: 5 3 4\n"
           "space directions: (0.5,0,0) (0,0.75,0) (0,0,2.5)\nendian: little\nencoding: raw\n\n")
    open(path, "wb").write(hdr.encode() + vol.astype("<i2").tobytes())
    return vol


def camera_angles():
    rng = np.random.default_rng(2)
    return [(0.9, 6.183), (0.0, 0.0), (0.3, 6.1), (-1.2, 3.0)] + [tuple(rng.uniform(-7, 7, 2)) for _ in range(200)]


def _jpeg_scene(w, h, n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    planes = []
    for c in range(n):
        p = 128 + 90 * np.sin(xx / (5.0 + 3 * c) + c) * np.cos(yy / (7.0 - c)) + rng.normal(0, 12, (h, w))
        p[h // 3: h // 2, w // 4: w // 2] = 30 + 60 * c  # a hard edge
        planes.append(np.clip(p, 0, 255).astype(np.uint8))
    return planes


JPEG_CASES = [
    # name, (w, h), sampling per component, progressive, restart, table style, interleaved, extra
    ("grey", (37, 29), [(1, 1)], False, 0, 0, True, {}),
    ("444", (40, 24), [(1, 1)] * 3, False, 0, 1, True, {}),
    ("420", (53, 47), [(2, 2), (1, 1), (1, 1)], False, 0, 1, True, {}),
    ("422", (61, 18), [(2, 1), (1, 1), (1, 1)], False, 3, 0, True, {}),
    ("440", (19, 50), [(1, 2), (1, 1), (1, 1)], False, 0, 0, True, {}),
    ("411", (70, 20), [(4, 1), (1, 1), (1, 1)], False, 2, 1, True, {}),
    ("420_noninterleaved", (45, 33), [(2, 2), (1, 1), (1, 1)], False, 5, 0, False, {}),
    ("one_pixel_wide_chroma", (2, 9), [(2, 2), (1, 1), (1, 1)], False, 0, 0, True, {}),
    ("q16", (24, 24), [(1, 1)] * 3, False, 0, 0, True, {"scale": 8.0}),
    ("rgb_ids", (30, 22), [(1, 1)] * 3, False, 0, 0, True, {"ids": [ord("R"), ord("G"), ord("B")]}),
    ("adobe_rgb", (30, 22), [(1, 1)] * 3, False, 0, 0, True, {"adobe": 0}),
    ("adobe_ycc_with_jfif", (30, 22), [(2, 1), (1, 1), (1, 1)], False, 0, 0, True, {"adobe": 1, "jfif": True}),
    ("cmyk", (26, 21), [(1, 1)] * 4, False, 0, 0, True, {"adobe": 0}),
    ("ycck", (26, 21), [(2, 2), (1, 1), (1, 1), (2, 2)], False, 0, 1, True, {"adobe": 2}),
    ("prog_grey", (37, 29), [(1, 1)], True, 0, 0, True, {}),
    ("prog_420", (53, 47), [(2, 2), (1, 1), (1, 1)], True, 0, 1, True, {}),
    ("prog_444_restart", (41, 30), [(1, 1)] * 3, True, 4, 0, True, {}),
    ("prog_422_flat", (64, 40), [(2, 1), (1, 1), (1, 1)], True, 0, 1, True, {"flat": True}),
    ("prog_simple_script", (33, 33), [(2, 2), (1, 1), (1, 1)], True, 0, 0, True,
     {"script": [([0, 1, 2], 0, 0, 0, 0), ([0], 1, 63, 0, 0), ([1], 1, 63, 0, 0), ([2], 1, 63, 0, 0)]}),
]


def jpeg_input(path, case):
    from tests.jpeg_writer import Encoder, quant_table

    name, (w, h), samp, progressive, restart, style, interleaved, extra = case
    planes = _jpeg_scene(w, h, len(samp), len(name) + w)
    if extra.get("flat"):
        for p in planes:
            p[:, w // 2:] = p[0, 0]  # long runs of empty blocks: EOB runs
    scale = extra.get("scale", 0.6)
    markers = b""
    if extra.get("jfif"):
        markers += b"\xff\xe0" + (16).to_bytes(2, "big") + b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    if "adobe" in extra:
        markers += b"\xff\xee" + (14).to_bytes(2, "big") + b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([extra["adobe"]])
    enc = Encoder(planes, samp, [quant_table(scale), quant_table(scale * 1.7)], [0] + [1] * (len(samp) - 1),
                  progressive=progressive, restart=restart, style=style, markers=markers, ids=extra.get("ids"),
                  script=extra.get("script"))
    data = enc.encode_progressive() if progressive else enc.encode_baseline(interleaved)
    open(path, "wb").write(data)
    return w, h


# ---- golden keys


def hdr_key(rle, w, h):
    return "hdr_rle%d_%dx%d" % (rle, w, h)


def png_key(color, depth, interlace):
    return "png_c%d_d%d_i%d" % (color, depth, interlace)


def nrrd_key(gz):
    return "nrrd_gz%d" % gz


# ---- the tests


def _stored(ref, tmp_path, key, suffix):
    """the stored input file of case `key`, written back to disk for the loaders"""
    path = str(tmp_path / (key + suffix))
    open(path, "wb").write(ref[key + ".in"].tobytes())
    return path


def _mine_env(mine, path, w, h):
    out = np.zeros((h, w, 4), np.uint8)
    d = (C.c_uint * 2)()
    assert mine.clvr_host_hdr_probe(path.encode(), d, out.ctypes.data, out.nbytes) == out.nbytes
    assert (d[0], d[1]) == (w, h)
    return out


@pytest.mark.parametrize("rle,w,h", HDR_CASES)
def test_hdr_environment_maps_decode_like_the_reference(ref, mine, tmp_path, rle, w, h):
    """Radiance .hdr -> gamma-2.2 RGBA8 (app/hdre_loader.cpp:7-24 through stb_image): pins app/hdre_loader.cpp here"""
    key = hdr_key(rle, w, h)
    out_r = ref[key]
    assert out_r.shape == (h, w, 4)
    out_m = _mine_env(mine, _stored(ref, tmp_path, key, ".hdr"), w, h)
    assert np.array_equal(out_m, out_r)
    assert out_r[..., :3].std() > 10


def test_png_environment_maps_decode_like_the_reference(ref, mine, tmp_path):
    """every PNG flavour of tests/test_host_mirror.py through the reference's stb_image: pins app/png_reader.cpp"""
    for color, depth, interlace in png_cases():
        key = png_key(color, depth, interlace)
        out_r = ref[key]
        h, w = out_r.shape[:2]
        assert (w, h) == (37, 19)
        out_m = _mine_env(mine, _stored(ref, tmp_path, key, ".png"), w, h)
        assert np.array_equal(out_m, out_r), (color, depth, interlace)


def _mine_nrrd(mine, path, n):
    counts, sizes = (C.c_uint * 3)(), (C.c_float * 3)()
    out = np.zeros(n, np.int16)
    assert mine.clvr_host_nrrd_load(path.encode(), counts, sizes, out.ctypes.data, n) == n
    return tuple(counts), tuple(sizes), out


def _ref_nrrd(ref, key):
    return tuple(int(v) for v in ref[key + ".counts"]), tuple(float(v) for v in ref[key + ".sizes"]), ref[key + ".voxels"]


@pytest.mark.parametrize("gz", [True, False])
def test_nrrd_volumes_load_like_the_reference(ref, mine, tmp_path, gz):
    """app/nrrd_loader.cpp: counts, relative voxel sizes and every voxel"""
    vol = nrrd_volume()
    key = nrrd_key(gz)
    cr, sr, vr = _ref_nrrd(ref, key)
    cm, sm, vm = _mine_nrrd(mine, _stored(ref, tmp_path, key, ".nrrd"), vol.size)
    assert cr == cm == (23, 14, 9)
    assert sr == sm
    assert np.array_equal(vr, vm) and np.array_equal(vm, vol.reshape(-1))


def test_nrrd_anisotropic_header_and_the_reference_test_block(ref, mine, tmp_path):
    golden = os.path.join(ROOT, "tests", "golden", "sdf_testdata.nrrd")
    dims = scene.read_nrrd(golden).shape  # the reference's own test volume (tests/sdf/testdata.nrrd)
    n = int(np.prod(dims))
    cr, sr, vr = _ref_nrrd(ref, "nrrd_testdata")
    cm, sm, vm = _mine_nrrd(mine, golden, n)
    assert cr == cm == (dims[2], dims[1], dims[0]) and sr == sm and np.array_equal(vr, vm)
    # anisotropic spacing: voxel sizes are kept relative to x
    vol = anisotropic_nrrd_input(str(tmp_path / "a.nrrd"))
    cr, sr, vr = _ref_nrrd(ref, "nrrd_anisotropic")
    cm, sm, vm = _mine_nrrd(mine, _stored(ref, tmp_path, "nrrd_anisotropic", ".nrrd"), vol.size)
    assert cr == cm == (5, 3, 4)
    assert sr == sm and sr[0] == 1.0 and sr[1] == pytest.approx(1.5) and sr[2] == pytest.approx(5.0)
    assert np.array_equal(vr, vm)


def test_camera_direction_matches_position3d(ref, mine, orc):
    """Position3D(alpha, beta, 0, {1,0,0}) (app/common.hpp, renderer.cpp:140): the python helper, the oracle's
    orc_camera_direction and the C++ host mirror all give the reference's bits"""
    angles = camera_angles()
    wants = ref["camera_direction"]
    assert wants.shape == (len(angles), 3) and wants.dtype == np.float32
    mine.clvr_host_camera_direction.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float)]
    for (a, b), want in zip(angles, wants):
        a32, b32 = np.float32(a), np.float32(b)  # ui_state keeps the look angles as floats
        assert np.array_equal(scene.camera_direction(a32, b32), want), (a, b)
        got = (C.c_float * 3)()
        mine.clvr_host_camera_direction(a32, b32, got)
        assert np.array_equal(np.array(got[:], np.float32), want)
        o = (C.c_float * 3)()
        orc.lib().orc_camera_direction(float(a32), float(b32), o)
        assert np.array_equal(np.array(o[:], np.float32), want)


@pytest.mark.parametrize("case", JPEG_CASES, ids=[c[0] for c in JPEG_CASES])
def test_jpeg_environment_maps_decode_like_the_reference(ref, mine, tmp_path, case):
    """JPEG env maps (reference README.md:29) through app/jpeg_reader.cpp vs the reference's stb_image: baseline and
    progressive streams, every upsampling path, restart intervals, 16-bit quantisation tables, JFIF / Adobe colour
    handling (RGB, YCbCr, CMYK, YCCK) -- identical RGBA8 bytes."""
    name, (w, h) = case[0], case[1]
    key = "jpeg_" + name
    want = ref[key]
    assert want.shape == (h, w, 4)
    out = _mine_env(mine, _stored(ref, tmp_path, key, ".jpg"), w, h)
    assert np.array_equal(out, want), "first difference at %s" % (np.argwhere(out != want)[:3].tolist(),)
    assert want[..., :3].std() > 5 and (want[..., 3] == 255).all()
