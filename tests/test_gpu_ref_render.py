"""-m gpu: the HIP path against what the REFERENCE's own kernels gave, directly -- not through the oracle.

tests/golden/ref_render.npz and ref_volume_kernels.npz hold the outputs of the reference's OpenCL C kernels compiled for the
host (oracle/ref/Makefile, tests/golden/make_ref_render_golden.py; the cases are those of tests/test_ref_render.py).  The
reference ran its work-items one after the other; what does not depend on that order is compared bit for bit: the hit entry
and the contribution of every pixel, the cache below the token cap and every count, the frame resolved from the stored
cache, compute_ao's cache, the pre-processing kernels.  Nothing here needs the reference tree or oracle/_ref/; the oracle only
builds the SDF (pinned by tests/golden/sdf_*) the scene marches through."""
import numpy as np
import pytest

from cl_volume_renderer_amd import ffi
from tests import test_ref_render as t
from tests.gpu_util import GpuScene
from tests.test_ref_render import ref, ref_volume  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

IDS = lambda cases: [c["name"] for c in cases]  # noqa: E731


def _scene(gpu_ctx, orc, ref, case):  # noqa: F811
    inputs = t.case_inputs(case, orc)
    vol, sdf, env, src, pos, d, seeds = inputs
    want_sha = ref[case["name"] + ".inputs_sha"]
    got_sha = np.stack([t.sha(vol), t.sha(sdf), t.sha(env), t.sha(pos), t.sha(d), t.sha(np.array(seeds, np.int64))])
    assert np.array_equal(got_sha, want_sha), "the scene is not the one the fixture was recorded on"
    g = GpuScene(gpu_ctx, vol, sdf, env, src, case["frame"], case["launch"])
    return g, pos, d, seeds, ffi.cache_len(*case["dims"]) // 4


@pytest.mark.parametrize("case", t.RENDER_CASES, ids=IDS(t.RENDER_CASES))
def test_hit_entry_and_contribution_per_pixel(gpu_ctx, orc, ref, case):  # noqa: F811
    """k_primary's hit entry of every pixel, and the sample every pixel contributes (image-space mode with contribution output:
    no token, every sample is kept) against what the reference's pixel added to its voxel, wherever its token was granted"""
    n = case["name"]
    g, pos, d, seeds, _ = _scene(gpu_ctx, orc, ref, case)
    hit = ref[n + ".hit_index"].astype(np.int64)
    passes = t.CONTRIB_PASSES if case["whole"] == "ends" else (0,)
    for k, p in enumerate(passes):
        g.render(pos, d, seeds[p], mode=ffi.ACCUM_IMAGE_SPACE, write_frame=False)
        assert np.array_equal(g.hit_index.pull(), hit)
        if case["whole"] != "ends":
            continue
        got = g.contrib.pull()[hit >= 0]
        granted = ref[n + ".granted"][k] == 1
        assert granted.sum() > 300
        assert np.array_equal(got[granted, :3], ref[n + ".contrib"][k][granted].astype(np.uint32))
        assert (got[:, 3] == 1).all()
    g.release()


@pytest.mark.parametrize("fused", [False, True], ids=["pass_per_launch", "fused"])
@pytest.mark.parametrize("case", t.RENDER_CASES, ids=IDS(t.RENDER_CASES))
def test_voxel_cache_after_the_passes(gpu_ctx, orc, ref, case, fused):  # noqa: F811
    """the reference's own accumulation: counts equal everywhere (min(requests, 256) in any order), entries below the 256-token
    cap bit for bit -- after every pass where the fixture holds every pass, after the last one for the fused launch"""
    n = case["name"]
    g, pos, d, seeds, n_entries = _scene(gpu_ctx, orc, ref, case)

    def check(p):
        got, want = g.cache.pull().reshape(-1, 4), t.full_cache(ref, n, n_entries, p)
        assert np.array_equal(got[:, 3], want[:, 3])
        below = want[:, 3] < 256
        assert np.array_equal(got[below], want[below])
        return below

    if fused:
        g.render(pos, d, None, seeds=seeds, debug=False)
        below = check(-1)
    else:
        for p, s in enumerate(seeds):
            g.render(pos, d, s, debug=False)
            if case["whole"] == "ends":
                check(p)
        below = check(-1)
    touched = ref[n + ".entries"]
    assert below[touched].any()  # (how many voxels each scene holds at the cap and below it: tests/test_ref_render.py)
    g.release()


@pytest.mark.parametrize("case", t.RENDER_CASES, ids=IDS(t.RENDER_CASES))
def test_frame_resolved_from_the_stored_cache(gpu_ctx, orc, ref, case):  # noqa: F811
    """k_resolve on the reference's final cache.  The reference's pixel reads its voxel right after its own add
    (ray_marching.cl:82-99), so in its raw frame the LAST pixel of every voxel, in launch order, shows the final cache: every
    pixel of that voxel must resolve to that colour; a pixel that hits nothing shows the environment map as stored."""
    n = case["name"]
    g, pos, d, seeds, n_entries = _scene(gpu_ctx, orc, ref, case)
    w, h = case["launch"]
    hit = ref[n + ".hit_index"].astype(np.int64)
    g.cache.push(t.full_cache(ref, n, n_entries).reshape(-1))
    g.kernel.render(frame=g.frame, volume=g.volume, sdf=g.sdf, env=g.env, buffer_volume=g.cache, cam_pos=pos, cam_dir=d, seed=0,
                    width=w, height=h, mode=ffi.ACCUM_VOXEL_CACHE, resolve_only=True, hit_index=g.hit_index)
    assert np.array_equal(g.hit_index.pull(), hit)
    frame = g.frame.pull()
    stored = ref[n + ".frame_last"]
    last_pixel = np.full(n_entries, -1, np.int64)
    is_hit = hit >= 0
    np.maximum.at(last_pixel, hit[is_hit], np.nonzero(is_hit)[0])
    want = stored[:h, :w].reshape(-1, 4).copy()
    want[is_hit] = want[last_pixel[hit[is_hit]]]
    assert np.array_equal(frame[:h, :w].reshape(-1, 4), want)
    assert len(np.unique(want[is_hit], axis=0)) > 20  # the frame is no flat colour
    if case["launch"] != case["frame"]:
        assert not frame[h:].any() and not frame[:, w:].any()
    g.release()


@pytest.mark.parametrize("case", t.AO_CASES, ids=IDS(t.AO_CASES))
def test_ambient_occlusion_cache(gpu_ctx, orc, ref, case):  # noqa: F811
    """k_ao: {samples, occluded} per voxel after every pass: sample counts equal everywhere, entries below the cap of 100 bit for bit
    (at the cap the reference's read-modify-write keeps whichever samples came first)"""
    n = case["name"]
    g, pos, d, seeds, n_entries = _scene(gpu_ctx, orc, ref, case)
    for p, s in enumerate(seeds):
        g.render(pos, d, s, shading=ffi.SHADE_AO)
        if p == 0:
            assert np.array_equal(g.hit_index.pull(), ref[n + ".hit_index"].astype(np.int64))
        pulled = g.cache.pull()
        got, want = pulled[: n_entries * 2].reshape(-1, 2), t.full_cache(ref, n, n_entries, p, channels=2)
        assert np.array_equal(got[:, 0], want[:, 0])
        below = want[:, 0] < 100
        assert np.array_equal(got[below], want[below])
        assert not pulled[n_entries * 2:].any()
    assert (below & (want[:, 0] > 0)).sum() > 50
    g.release()


def _ev(n, by=8):
    return (n + by - 1) // by * by


@pytest.mark.parametrize("dims", t.VOLUME_DIMS, ids=["%dx%dx%d" % d for d in t.VOLUME_DIMS])
def test_pre_processing_kernels(gpu_ctx, ref_volume, dims):  # noqa: F811
    """bilateral_filter, fetch_stats, tf_sort_values, apply_clip and buffer_reset through the generic launch"""
    n = "v%dx%dx%d" % dims
    X, Y, Z = dims
    phantom, noise = t.volume_case_inputs(dims)
    assert np.array_equal(np.stack([t.sha(phantom), t.sha(noise)]), ref_volume[n + ".inputs_sha"])
    G = [_ev(X), _ev(Y), _ev(Z)]
    mems, kernels = [], []

    def keep(m, into=mems):
        into.append(m)
        return m

    kb = keep(gpu_ctx.kernel("volume_filter.cl", "bilateral_filter"), kernels)
    for vol, key in ((noise, ".bilateral_noise"), (phantom, ".bilateral_phantom_sha")):
        src, dst = keep(gpu_ctx.image_from(vol)), keep(gpu_ctx.image([X, Y, Z], 1, np.int16, (Z, Y, X)))
        kb.launch(G, [4, 4, 4], src, dst)
        got = dst.pull()
        assert np.array_equal(t.sha(got) if key.endswith("_sha") else got, ref_volume[n + key])

    v = keep(gpu_ctx.image_from(phantom))
    stats = keep(gpu_ctx.buffer_from(np.array(t.STATS_INIT, np.int32)))
    ks = keep(gpu_ctx.kernel("reference_volume_figures.cl", "fetch_stats"), kernels)
    ks.launch(G, [4, 4, 4], v, stats)
    st = stats.pull()
    assert np.array_equal(st, ref_volume[n + ".stats"])

    W, H = t.HIST_WH
    bins = keep(gpu_ctx.buffer_from(np.zeros(W * H, np.uint32)))
    kh = keep(gpu_ctx.kernel("histogram.cl", "tf_sort_values"), kernels)
    kh.launch(G, [4, 4, 4], v, bins, np.uint32(W), np.uint32(H), float(st[0]), float(st[1]), float(st[2]), float(st[3]))
    want = np.zeros(W * H, np.uint32)
    want[ref_volume[n + ".hist_bins"]] = ref_volume[n + ".hist_counts"]
    assert np.array_equal(bins.pull().reshape(-1), want)

    kc = keep(gpu_ctx.kernel("reference_volume_clip.cl", "apply_clip"), kernels)
    for i, (start, length) in enumerate(t.CLIPS[dims]):
        dst = keep(gpu_ctx.image(list(length), 1, np.int16, (length[2], length[1], length[0])))
        b_start = keep(gpu_ctx.buffer_from(np.array(start, np.uint32)))
        b_len = keep(gpu_ctx.buffer_from(np.array(list(length) + [4], np.uint32)))
        kc.launch([_ev(k, 4) for k in length], [4, 4, 4], v, dst, b_start, b_len)
        assert np.array_equal(dst.pull(), ref_volume[n + ".clip%d" % i]), (start, length)

    first, end = (int(k) for k in ref_volume[n + ".reset_zeroed"])
    cache = keep(gpu_ctx.buffer_from(np.full(ffi.cache_len(X, Y, Z), 0xABCD, np.uint16)))
    gpu_ctx.buffer_reset(cache)
    assert first == 0 and not cache.pull()[:end].any()
    for m in mems:
        m.release()
    for k in kernels:
        k.release()
