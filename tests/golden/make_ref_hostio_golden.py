"""Generates tests/golden/ref_hostio.npz for tests/test_ref_hostio.py: the input files of every case (made by the
generators in that module) and what the REFERENCE's own loaders return for them -- oracle/_ref/libref_hostio.so, the
reference's app/hdre_loader.cpp + stb_image.h, app/nrrd_loader.cpp and common.hpp's Position3D, built by
oracle/ref/Makefile (`make -C oracle/ref REF=<reference tree>`).  Run from the repo root:
    python tests/golden/make_ref_hostio_golden.py
Keys: `<case>.in` the input file's bytes (uint8); `<case>` the RGBA8 an env-map load gave; `<case>.counts` / `.sizes` /
`.voxels` what an NRRD load gave; `camera_direction` Position3D's direction for every angle pair of camera_angles()."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_ref_hostio as t  # noqa: E402

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libref_hostio.so")
OUT = os.path.join(ROOT, "tests", "golden", "ref_hostio.npz")

L = C.CDLL(REF_LIB)
L.ref_env_load.restype = C.c_longlong
L.ref_env_load.argtypes = [C.c_char_p, C.POINTER(C.c_uint), C.c_void_p, C.c_longlong]
L.ref_nrrd_load.restype = C.c_longlong
L.ref_nrrd_load.argtypes = [C.c_char_p, C.POINTER(C.c_uint), C.POINTER(C.c_float), C.c_void_p, C.c_longlong]
L.ref_camera_direction.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_float)]

golden = {}


def env_in_child(path, w, h):
    """the reference's loader exits the process on a file it rejects, so every env map goes through it in a child"""
    code = ("import ctypes as C, numpy as np\n"
            "L = C.CDLL(%r)\n"
            "L.ref_env_load.restype = C.c_longlong\n"
            "L.ref_env_load.argtypes = [C.c_char_p, C.POINTER(C.c_uint), C.c_void_p, C.c_longlong]\n"
            "out = np.zeros((%d, %d, 4), np.uint8); d = (C.c_uint * 2)()\n"
            "n = L.ref_env_load(%r.encode(), d, out.ctypes.data, out.nbytes)\n"
            "assert n == out.nbytes and (d[0], d[1]) == (%d, %d), (n, d[0], d[1])\n"
            "np.save(%r, out)\n") % (REF_LIB, h, w, path, w, h, path + ".ref.npy")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "the reference's decoder rejected the test stream: " + r.stderr[-400:]
    return np.load(path + ".ref.npy")


def store_input(key, path):
    golden[key + ".in"] = np.frombuffer(open(path, "rb").read(), np.uint8)


def nrrd(key, path, n):
    counts, sizes = (C.c_uint * 3)(), (C.c_float * 3)()
    out = np.zeros(n, np.int16)
    assert L.ref_nrrd_load(path.encode(), counts, sizes, out.ctypes.data, n) == n
    golden[key + ".counts"] = np.array(counts[:], np.uint32)
    golden[key + ".sizes"] = np.array(sizes[:], np.float32)
    golden[key + ".voxels"] = out


with tempfile.TemporaryDirectory() as tmp:
    for rle, w, h in t.HDR_CASES:
        key = t.hdr_key(rle, w, h)
        p = os.path.join(tmp, key + ".hdr")
        t.hdr_input(p, rle, w, h)
        store_input(key, p)
        golden[key] = env_in_child(p, w, h)
    for color, depth, interlace in t.png_cases():
        key = t.png_key(color, depth, interlace)
        p = os.path.join(tmp, key + ".png")
        w, h = t.png_input(p, color, depth, interlace)
        store_input(key, p)
        golden[key] = env_in_child(p, w, h)
    for case in t.JPEG_CASES:
        key = "jpeg_" + case[0]
        p = os.path.join(tmp, key + ".jpg")
        w, h = t.jpeg_input(p, case)
        store_input(key, p)
        golden[key] = env_in_child(p, w, h)
    for gz in (True, False):
        key = t.nrrd_key(gz)
        p = os.path.join(tmp, key + ".nrrd")
        vol = t.nrrd_input(p, gz)
        store_input(key, p)
        nrrd(key, p, vol.size)
    p = os.path.join(tmp, "nrrd_anisotropic.nrrd")
    vol = t.anisotropic_nrrd_input(p)
    store_input("nrrd_anisotropic", p)
    nrrd("nrrd_anisotropic", p, vol.size)
    testdata = os.path.join(ROOT, "tests", "golden", "sdf_testdata.nrrd")
    from cl_volume_renderer_amd import scene

    nrrd("nrrd_testdata", testdata, scene.read_nrrd(testdata).size)
    dirs = []
    for a, b in t.camera_angles():
        want = (C.c_float * 3)()
        L.ref_camera_direction(float(np.float32(a)), float(np.float32(b)), want)
        dirs.append(want[:])
    golden["camera_direction"] = np.array(dirs, np.float32)

np.savez_compressed(OUT, **golden)
print(OUT, os.path.getsize(OUT), "bytes,", len(golden), "arrays")
