"""The C++ mirror of the volume filter (renderer::filter_volume, renderer::gaussian_weights over the C facade) and clvr_headless'
--filter option, on the small phantom, against tests/vfilter_ref.py and tests/grow_ref.py."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import grow_ref as gr
from tests import vfilter_ref as vr
from tests.view_helpers import ROOT, host_lib

pytestmark = pytest.mark.gpu

N = 48


@functools.lru_cache(maxsize=None)
def _case():
    """the phantom, its median, and a seed in the median's bone window"""
    vol = scene.phantom(N)
    med = vr.median(vol, (1, 1, 1))
    z = N // 2
    y, x = np.argwhere(gr.admissible(med, 500, 1200)[z])[0]
    return vol, med, (int(x), int(y), int(z))


def test_host_mirror_filters_the_volume():
    vol, med, seed = _case()
    env = scene.env_map(64, 32)
    L = host_lib(clvr_host_grow_region=(None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]),
                 clvr_host_set_voxel_sizes=(None, [C.c_void_p, C.POINTER(C.c_float)]),
                 clvr_host_filter_volume=(None, [C.c_void_p, C.c_int, C.POINTER(C.c_uint), C.c_double, C.c_int, C.c_void_p]))
    h = L.clvr_host_create()
    try:
        got = np.zeros_like(vol)

        def load():
            L.clvr_host_load(h, vol.ctypes.data, N, N, N, env.ctypes.data, 64, 32)

        def call(kind, radius, sigma=0.0, masked=0):
            r = (C.c_uint * 3)(*radius)
            L.clvr_host_filter_volume(h, kind, r, sigma, masked, got.ctypes.data)
            return list(r)

        load()
        call(ffi.FILTER_MEDIAN, (1, 1, 1))
        assert np.array_equal(got, med)
        grown = ffi.GrowResult()
        L.clvr_host_grow_region(h, np.array(seed, np.uint32).ctypes.data, 1, 500, 1200, 0, C.byref(grown))
        region, _ = gr.grow(med, [seed], 500, 1200)
        assert grown.count == int(region.sum()) > 1000
        # a second filter on the first one's result, only inside the grown region
        call(ffi.FILTER_MAX, (2, 0, 1), masked=1)
        assert np.array_equal(got, vr.filtered(med, vr.MAX, (2, 0, 1), None, region))
        # the Gaussian in millimetres on anisotropic voxels: the C++ weights are scene.gaussian_weights'
        load()
        sizes = (1.0, 1.0, 2.5)
        L.clvr_host_set_voxel_sizes(h, (C.c_float * 3)(*sizes))
        w = scene.gaussian_weights(1.5, sizes)
        assert call(ffi.FILTER_SMOOTH, (0, 0, 0), sigma=1.5) == [len(v) - 1 for v in w] == [5, 5, 2]
        assert np.array_equal(got, vr.smooth(vol, w))
    finally:
        L.clvr_host_destroy(h)


def test_headless_filter_option(tmp_path):
    vol, med, seed = _case()
    header = "NRRD0004\ntype: short\ndimension: 3\nsizes: %d %d %d\nendian: little\nencoding: raw\n\n" % (N, N, N)
    with open(tmp_path / "v.nrrd", "wb") as f:
        f.write(header.encode("ascii") + np.ascontiguousarray(vol, "<i2").tobytes())
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(np.random.default_rng(5).random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", "64", "64"]

    def run(*options):
        out = subprocess.run([exe] + list(options) + files + [str(tmp_path / "m.ply")], capture_output=True, text=True, timeout=120)
        return out.returncode, [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")], out.stderr

    grow = "--grow=%d,%d,%d,500,1200" % seed
    code, lines, err = run("--filter=median", grow, "--mesh=-20000")
    assert code == 0, err
    assert lines[0] == {"filter": {"kind": "median", "radius": [1, 1, 1]}}
    want, _ = gr.grow(med, [seed], 500, 1200)
    plain, _ = gr.grow(vol, [seed], 500, 1200)
    assert lines[1]["count"] == int(want.sum()) != int(plain.sum())
    # repeatable, applied in order
    code, lines, err = run("--filter=max=2", "--filter=median,2d", "--filter=gauss=0.8", grow, "--mesh=-20000")
    assert code == 0, err
    assert [e["filter"] for e in lines[:3]] == [{"kind": "max", "radius": [2, 2, 2]}, {"kind": "median", "radius": [1, 1, 0]},
                                                {"kind": "gauss", "radius": [3, 3, 3]}]
    chain = vr.smooth(vr.median(vr.extreme(vol, (2, 2, 2), vr.MAX), (1, 1, 0)), scene.gaussian_weights(0.8))
    assert lines[3]["count"] == int(gr.grow(chain, [seed], 500, 1200)[0].sum())
    assert not any("filter" in e for e in run(grow, "--mesh=-20000")[1])  # no option: no line
    for bad in ("--filter", "--filter=", "--filter=median,3d", "--filter=min=17", "--filter=max=-1", "--filter=gauss=", "--filter=gauss=x",
                "--filter=box=2", "--filters=median"):
        assert run(bad)[0] == 1, bad
