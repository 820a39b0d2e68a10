"""The C++ mirror of the thinning (renderer::thin_mask, renderer::mask_points over the C facade) and clvr_headless' skeleton item, on
the phantom's grown bone, against tests/thin_ref.py."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import scene
from tests import grow_ref as gr
from tests import thin_ref as tr
from tests.view_helpers import ROOT, host_lib

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _bone():
    vol = scene.phantom(48)
    adm = gr.admissible(vol, 500, 1200)
    z = vol.shape[0] // 2
    y, x = np.argwhere(adm[z])[0]
    seed = (int(x), int(y), int(z))
    bone, _ = gr.grow(vol, [seed], 500, 1200)
    assert bone.sum() > 1000
    return vol, seed, bone


def test_host_mirror_thins_and_lists():
    vol, seed, bone = _bone()
    n = 48
    env = scene.env_map(64, 32)
    L = host_lib(clvr_host_grow_region=(None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]),
                 clvr_host_thin_mask=(None, [C.c_void_p, C.c_int, C.c_uint, C.POINTER(C.c_ulonglong)]),
                 clvr_host_mask_points=(C.c_ulonglong, [C.c_void_p, C.c_void_p, C.c_ulonglong]))
    from cl_volume_renderer_amd import ffi

    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, n, n, n, env.ctypes.data, 64, 32)
        seeds = np.array(seed, np.uint32)
        for keep_ends, limit in ((1, 0), (0, 0), (1, 2)):
            grown = ffi.GrowResult()
            L.clvr_host_grow_region(h, seeds.ctypes.data, 1, 500, 1200, 0, C.byref(grown))
            assert grown.count == int(bone.sum())
            want, want_res = tr.thin(bone, tr.KEEP_ENDS if keep_ends else 0, None, limit)
            got_res = (C.c_ulonglong * 4)()
            L.clvr_host_thin_mask(h, keep_ends, limit, got_res)
            assert list(got_res) == [want_res[k] for k in ("count_in", "count_out", "deleted", "iterations")]
            want_points, _ = tr.points(want)
            assert L.clvr_host_mask_points(h, None, 0) == len(want_points) > 0
            got = np.zeros((len(want_points), 4), np.uint32)
            assert L.clvr_host_mask_points(h, got.ctypes.data, len(got)) == len(got)
            assert np.array_equal(got, want_points)
    finally:
        L.clvr_host_destroy(h)


def test_headless_skeleton_item(tmp_path):
    vol, seed, bone = _bone()
    Z, Y, X = vol.shape
    header = "NRRD0004\ntype: short\ndimension: 3\nsizes: %d %d %d\nendian: little\nencoding: raw\n\n" % (X, Y, Z)
    with open(tmp_path / "v.nrrd", "wb") as f:
        f.write(header.encode("ascii") + np.ascontiguousarray(vol, "<i2").tobytes())
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(np.random.default_rng(5).random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", "64", "64"]

    def run(*options):
        out = subprocess.run([exe] + list(options) + files + [str(tmp_path / "m.ply")], capture_output=True, text=True, timeout=120)
        return out.returncode, [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")], out.stderr

    for item, flags in (("skeleton", tr.KEEP_ENDS), ("skeleton=ends", tr.KEEP_ENDS), ("skeleton=kernel", 0)):
        code, lines, err = run("--grow=%d,%d,%d,500,1200,%s" % (seed + (item,)), "--mesh=-20000")
        assert code == 0, err
        want, res = tr.thin(bone, flags)
        what = tr.structure(want)
        line = [entry["skeleton"] for entry in lines if "skeleton" in entry]
        assert line == [{"mode": "kernel" if flags == 0 else "ends", "count_in": res["count_in"], "count_out": res["count_out"],
                         "iterations": res["iterations"], "ends": what["ends"], "junction_voxels": what["junction_voxels"]}]
        assert lines[0]["count"] == int(bone.sum())
    code, lines, err = run("--components=500,1200,largest=1,skeleton,show", "--slice=axial")
    assert code == 0, err
    assert [entry["skeleton"]["mode"] for entry in lines if "skeleton" in entry] == ["ends"]
    assert not any("skeleton" in entry for entry in run("--grow=%d,%d,%d,500,1200" % seed, "--mesh=-20000")[1])  # no item: no line
    for bad in ("skeleton=", "skeleton=x", "skeleton,skeleton", "skeleton=ends,skeleton=kernel"):
        assert run("--grow=%d,%d,%d,500,1200," % seed + bad)[0] == 1, bad
    assert run("--components=500,1200,skeleton=2")[0] == 1
