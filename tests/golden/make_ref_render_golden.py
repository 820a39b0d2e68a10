"""Generates tests/golden/ref_render.npz and tests/golden/ref_volume_kernels.npz for tests/test_ref_render.py and
tests/test_gpu_ref_render.py: what the REFERENCE's own OpenCL C kernels give for the cases of tests/test_ref_render.py --
oracle/_ref/libref_cl_default.so and libref_cl_gradient.so, the reference's utility*.cl, ray_marching.cl and pre-processing
kernels compiled for the host and linked with oracle/ref/ref_cl_shim.cpp by oracle/ref/Makefile
(`make -C oracle/ref REF=<reference tree>`).  Runs only where those libraries exist.  Run from the repo root:
    python tests/golden/make_ref_render_golden.py
Data only, in np.savez_compressed's format.  The inputs are regenerated from cl_volume_renderer_amd.scene by the cases' parameters; the fixture keeps their
SHA-256 (`<case>.inputs_sha`).  Keys of a render case: `.hit_index` the cache entry per pixel of the launch (-1: no hit),
`.entries` the distinct ones, `.contrib` / `.granted` [pass][hit pixel] the contribution the pixel added and whether its token
was granted, `.cache_rows` [pass][entry][4] the cache at `.entries` (zero elsewhere), `.contrib_sha` / `.cache_sha` /
`.frame_sha` [pass] SHA-256 of the whole arrays, `.frame_last` the raw frame after the last pass, `.exit_depths` [pass][3] the
paths that left the volume with i = 8, 9, 10.  Of an ambient-occlusion case: `.shade` [pass][pixel], `.cache_rows`
[pass][entry][2].  Of a volume `v<X>x<Y>x<Z>`: `.bilateral_noise`, `.bilateral_phantom_sha`, `.stats`, `.hist_bins` /
`.hist_counts` (the non-zero bins of tf_sort_values), `.clip<i>`, `.reset_zeroed`."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_cl_ffi  # noqa: E402
from tests import test_ref_render as t  # noqa: E402


class _RefVolumeKernels:
    bilateral_filter = staticmethod(ref_cl_ffi.bilateral_filter)
    fetch_stats = staticmethod(ref_cl_ffi.fetch_stats)
    apply_clip = staticmethod(ref_cl_ffi.apply_clip)

    @staticmethod
    def tf_sort_values(vol, w, h, *ranges):
        return ref_cl_ffi.tf_sort_values(vol, w, h, *ranges)[0]


def generate(orc):
    """({key: array} of ref_render.npz, {key: array} of ref_volume_kernels.npz); `orc` builds the SDFs (pinned by tests/golden/sdf_*)"""
    render, volume = {}, {}
    for case in t.RENDER_CASES:
        inputs = t.case_inputs(case, orc)
        vol, sdf, env = inputs[:3]
        sc = ref_cl_ffi.Scene(case["tf"], vol, sdf, env, case["frame"], case["launch"])
        sc.reset()
        render.update(t.record_render(case, inputs, sc, extra=lambda s: s.exit_depths.astype(np.int32)))
    for case in t.AO_CASES:
        inputs = t.case_inputs(case, orc)
        vol, sdf, env, _, pos, d, seeds = inputs
        light = ref_cl_ffi.Scene(case["tf"], vol, sdf, env, case["frame"], case["launch"])
        light.render(pos, d, seeds[0])  # compute_ao's primary march is compute_light's: the hit entries come from its token requests
        sc = ref_cl_ffi.Scene(case["tf"], vol, sdf, env, case["frame"], case["launch"])
        sc.reset()
        n_entries = sc.cache.size // 4

        def render_ao(p, dd, s, sc=sc, light=light):
            sc.render_ao(p, dd, s)
            assert not sc.shade[light.hit_index < 0].any()
            return sc.shade.copy()

        render.update(t.record_ao(case, inputs, render_ao, light.hit_index.copy(),
                                  lambda sc=sc, n=n_entries: sc.cache[: n * 2].reshape(-1, 2)))
        assert not sc.cache[n_entries * 2:].any()
    for dims in t.VOLUME_DIMS:
        volume.update(t.record_volume_kernels(dims, _RefVolumeKernels))
        sc = ref_cl_ffi.Scene("default", *t.case_inputs(t._case("reset", dims, "default", (0, 0, 0)), orc)[:3], (8, 8))
        sc.cache[:] = 0xABCD
        sc.reset()
        z = np.nonzero(sc.cache == 0)[0]
        assert z.size == z[-1] - z[0] + 1 and (sc.cache[z[-1] + 1:] == 0xABCD).all()
        volume["v%dx%dx%d.reset_zeroed" % dims] = np.array([z[0], z[-1] + 1], np.int64)
    return render, volume


def save(path, arrays):
    """np.savez_compressed with the members' time stamps fixed, so that the same arrays give the same file byte for byte"""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    from oracle import orc_ffi

    t0 = time.time()
    render, volume = generate(orc_ffi)
    counts = render["cap.cache_rows"][-1][:, 3]
    assert (counts == 256).any() and (counts < 256).any(), "the cap scene must hold voxels at the 256-token cap and below it"
    for path, arrays in ((t.GOLDEN_RENDER, render), (t.GOLDEN_VOLUME, volume)):
        save(path, arrays)
        print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
    print("generated in %.1f s" % (time.time() - t0))
