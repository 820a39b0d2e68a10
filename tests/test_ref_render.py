"""-m "not gpu": the CPU oracle against the REFERENCE's own kernels, compiled from the reference's text.

oracle/ref/Makefile concatenates a transfer function, the reference's utility*.cl, ray_marching.cl and the pre-processing
kernels, compiles that unit for the host with clang -x cl and links it with oracle/ref/ref_cl_shim.cpp (the OpenCL built-ins as
DESIGN.md section 2 fixes them, and a serial driver) into oracle/_ref/libref_cl_<tf>.so.
tests/golden/make_ref_render_golden.py ran the cases below on those libraries and stored what they gave in
tests/golden/ref_render.npz and ref_volume_kernels.npz.  Here the oracle runs the same cases with one thread -- the driver's
order: rows outer, x inner -- and must give the stored bytes: hit entries, contributions, the cache after every pass and the
raw frame, cap regime included.  Where the libraries are present they run again and must give the stored bytes too, so the
fixtures cannot drift from their recipe.  Neither the reference tree nor oracle/_ref/ is needed for the rest.

record_render / record_ao / record_volume_kernels turn any backend's buffers into the fixture's arrays; the maker calls them
with the reference's library, the tests with the oracle."""
import hashlib
import os

import numpy as np
import pytest

from cl_volume_renderer_amd import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_RENDER = os.path.join(ROOT, "tests", "golden", "ref_render.npz")
GOLDEN_VOLUME = os.path.join(ROOT, "tests", "golden", "ref_volume_kernels.npz")

# ---- the cases ---------------------------------------------------------------------------------------------------------------
# pose: camera position; it looks at the volume's centre.  A SHA-256 of every pass's contributions, cache and frame is kept in any
# case; `whole` says what else: "ends" the cache rows of every pass and the contributions of the first and the last pass
# (CONTRIB_PASSES), "last" the cache rows of the last pass only (the 384 x 384 scene: anything more would not fit a fixture).
OUTSIDE = {(24, 24, 24): (-9.0, 20.0, -9.0), (20, 28, 17): (-9.0, 20.0, -9.0)}   # cut() runs for every pixel
INSIDE = {(24, 24, 24): (3.0, 19.0, 4.0), (20, 28, 17): (4.0, 20.0, 5.0)}        # in_volume: the ray starts at the camera


CONTRIB_PASSES = (0, -1)


def _case(name, dims, tf, pos, frame=(96, 64), launch=None, env=(64, 32), seeds=8, whole="ends"):
    return dict(name=name, dims=dims, tf=tf, pos=pos, frame=frame, launch=launch or frame, env=env, seeds=seeds, whole=whole)


RENDER_CASES = [
    _case("cube_default_outside", (24, 24, 24), "default", OUTSIDE[(24, 24, 24)]),
    _case("cube_gradient_inside", (24, 24, 24), "gradient", INSIDE[(24, 24, 24)]),
    _case("ragged_default_inside", (20, 28, 17), "default", INSIDE[(20, 28, 17)]),
    _case("ragged_gradient_outside", (20, 28, 17), "gradient", OUTSIDE[(20, 28, 17)]),
    _case("ragged_gradient_rect", (20, 28, 17), "gradient", INSIDE[(20, 28, 17)], launch=(40, 24)),  # launch smaller than the frame
    # dx == dy and the camera as far beyond the x face as beyond the y face: every ray of the middle row meets the box exactly on its
    # edge x == X, y == Y, where LIMITS' `<=` (utility_ray.cl:35) decides whether it cuts the volume at all
    _case("cube_default_edge_on", (24, 24, 24), "default", (32.0, 32.0, 12.0), seeds=2),
    # the scene of tests/test_gpu_exchange.py::test_exchange_of_two_emulated_ranks_against_the_oracle: voxels reach the 256-token cap
    _case("cap", (24, 24, 24), "default", (-9.0, 20.0, -9.0), frame=(384, 384), env=(128, 64), whole="last"),
]
AO_CASES = [
    # compute_ao on the ragged scene from so close that 24 passes on a tiny frame take some voxels to the cap of 100 samples
    _case("ao_ragged_gradient", (20, 28, 17), "gradient", INSIDE[(20, 28, 17)], frame=(48, 32), seeds=24),
    _case("ao_cube_default", (24, 24, 24), "default", OUTSIDE[(24, 24, 24)], frame=(48, 32)),  # every voxel stays below it
]
VOLUME_DIMS = [(70, 33, 45), (5, 4, 3), (2, 1, 1)]  # the ragged sizes of tests/test_gpu_volume_kernels.py
STATS_INIT = (2**31 - 1, -2**31, 2**31 - 1, -2**31, -2**31)  # app/reference_volume.cpp:23-28
HIST_WH = (500, 500)
CLIPS = {(70, 33, 45): [((5, 7, 3), (24, 20, 16)), ((60, 25, 40), (24, 20, 16)), ((3, 1, 2), (20, 12, 8))],
         (5, 4, 3): [((1, 1, 0), (3, 2, 3)), ((0, 0, 0), (5, 4, 3))], (2, 1, 1): [((1, 0, 0), (2, 1, 1))]}


def case_inputs(case, orc):
    """(volume, sdf, env, tf source, camera position, camera direction, seeds) -- all from scene.*; the fixture keeps their SHA-256"""
    dims = case["dims"]
    src = getattr(scene, "tf_%s_source" % case["tf"])()
    vol = scene.phantom(max(dims), dims=dims)
    sdf, _, _ = orc.sdf_build(vol, orc.parse_tf(src))
    env = scene.env_map(*case["env"])
    pos = np.array(case["pos"], np.float32)
    d = np.array(dims, np.float32) / np.float32(2) - pos
    d = (d / np.linalg.norm(d)).astype(np.float32)
    return vol, sdf, env, src, pos, d, scene.glibc_rand(case["seeds"])


def noise_volume(dims):
    """the volume of test_gpu_volume_kernels.py::test_bilateral_filter_noise: small differences, so most range weights are non-zero"""
    rng = np.random.default_rng(sum(dims))
    X, Y, Z = dims
    return (rng.integers(-6, 7, (Z, Y, X)) + rng.integers(-3, 4, (Z, 1, 1)) * 5).astype(np.int16)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


# ---- backend buffers -> fixture arrays ---------------------------------------------------------------------------------------


def record_render(case, inputs, sc, extra=None):
    """Runs the case's passes on `sc` (oracle.orc_ffi.Scene or oracle.ref_cl_ffi.Scene: .render, .cache, .frame, .hit_index,
    .contrib) and returns {key: array}.  `extra(sc)` may add per-pass arrays only one backend has."""
    vol, sdf, env, _, pos, d, seeds = inputs
    n, out = case["name"], {}
    out[n + ".inputs_sha"] = np.stack([sha(vol), sha(sdf), sha(env), sha(pos), sha(d), sha(np.array(seeds, np.int64))])
    per_pass = {k: [] for k in ("contrib_sha", "cache_sha", "frame_sha", "contrib", "granted", "cache_rows", "extra")}
    hit = entries = None
    for i, s in enumerate(seeds):
        sc.render(pos, d, s)
        if hit is None:
            hit = sc.hit_index.copy()
            assert hit.max() < 2**31
            entries = np.unique(hit[hit >= 0])
        assert np.array_equal(hit, sc.hit_index), "the primary hit does not depend on the seed"
        rows = sc.cache.reshape(-1, 4)
        rest = np.ones(rows.shape[0], bool)
        rest[entries] = False
        assert not rows[rest].any(), "only hit entries are ever written"
        assert sc.contrib.max() < 65536
        per_pass["contrib_sha"].append(sha(sc.contrib.astype(np.uint32)))
        per_pass["cache_sha"].append(sha(sc.cache))
        per_pass["frame_sha"].append(sha(sc.frame))
        if case["whole"] == "ends" or i == len(seeds) - 1:
            per_pass["cache_rows"].append(rows[entries].copy())
            if case["whole"] == "ends" and i in (0, len(seeds) - 1):
                per_pass["contrib"].append(sc.contrib[hit >= 0, :3].astype(np.uint16))
                per_pass["granted"].append(sc.contrib[hit >= 0, 3].astype(np.uint8))
        if extra:
            per_pass["extra"].append(extra(sc))
    out[n + ".hit_index"] = hit.astype(np.int32)
    out[n + ".entries"] = entries.astype(np.int32)
    out[n + ".frame_last"] = sc.frame.copy()
    for k, v in per_pass.items():
        if v and k != "extra":
            out[n + "." + k] = np.stack(v)
    if extra:
        out[n + ".exit_depths"] = np.stack(per_pass["extra"])
    return out


def record_ao(case, inputs, render_ao, hit_index, cache_of):
    """compute_ao pass by pass: `render_ao(pos, d, seed)` returns the launch's shade values (uint32 per pixel, 0 on a miss),
    `cache_of()` the 2-channel view {samples, occluded} of the cache"""
    vol, sdf, env, _, pos, d, seeds = inputs
    n, out = case["name"], {}
    entries = np.unique(hit_index[hit_index >= 0])
    shades, rows = [], []
    for s in seeds:
        shade = render_ao(pos, d, s)
        assert shade.max() <= 200
        shades.append(shade.astype(np.uint8))
        c = cache_of()
        rest = np.ones(c.shape[0], bool)
        rest[entries] = False
        assert not c[rest].any()
        rows.append(c[entries].copy())
    out[n + ".inputs_sha"] = np.stack([sha(vol), sha(sdf), sha(env), sha(pos), sha(d), sha(np.array(seeds, np.int64))])
    out[n + ".hit_index"] = hit_index.astype(np.int32)
    out[n + ".entries"] = entries.astype(np.int32)
    out[n + ".shade"] = np.stack(shades)
    out[n + ".cache_rows"] = np.stack(rows)
    return out


def volume_case_inputs(dims):
    return scene.phantom(max(dims), dims=dims), noise_volume(dims)


def record_volume_kernels(dims, k):
    """k: a namespace with bilateral_filter(vol), fetch_stats(vol, init), tf_sort_values(vol, w, h, 4 floats) -> frame,
    apply_clip(vol, start, length)"""
    phantom, noise = volume_case_inputs(dims)
    n, out = "v%dx%dx%d" % dims, {}
    out[n + ".inputs_sha"] = np.stack([sha(phantom), sha(noise)])
    out[n + ".bilateral_noise"] = k.bilateral_filter(noise)
    out[n + ".bilateral_phantom_sha"] = sha(k.bilateral_filter(phantom))
    st = np.asarray(k.fetch_stats(phantom, STATS_INIT), np.int32)
    out[n + ".stats"] = st
    frame = np.asarray(k.tf_sort_values(phantom, HIST_WH[0], HIST_WH[1], float(st[0]), float(st[1]), float(st[2]), float(st[3])))
    nz = np.nonzero(frame.reshape(-1))[0]
    out[n + ".hist_bins"] = nz.astype(np.int32)
    out[n + ".hist_counts"] = frame.reshape(-1)[nz].astype(np.uint32)
    for i, (start, length) in enumerate(CLIPS[dims]):
        out[n + ".clip%d" % i] = np.asarray(k.apply_clip(phantom, start, length), np.int16)
    return out


# ---- fixtures ----------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN_RENDER) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ref_volume():
    with np.load(GOLDEN_VOLUME) as z:
        return {k: z[k] for k in z.files}


def _same(got, want, prefix):
    keys = sorted(k for k in want if k.startswith(prefix + "."))
    assert keys, prefix
    for k in keys:
        if k in got:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert np.array_equal(got[k], want[k]), "%s: first difference at %s" % (k, np.argwhere(got[k] != want[k])[:3].tolist())
    return [k for k in keys if k not in got]


def full_cache(ref, name, n_entries, p=-1, channels=4):
    """the whole cache after pass p of a case, rebuilt from its stored rows (every other entry is zero)"""
    c = np.zeros((n_entries, channels), np.uint16)
    c[ref[name + ".entries"]] = ref[name + ".cache_rows"][p]
    return c


# ---- the tests ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", RENDER_CASES, ids=[c["name"] for c in RENDER_CASES])
def test_oracle_render_equals_the_compiled_reference(ref, orc, case):
    """orc_render with one thread == the reference's render kernel run serially: hit entry and contribution per pixel, cache after
    every pass, raw frame of every pass -- bit for bit, in and beyond the token cap"""
    inputs = case_inputs(case, orc)
    vol, sdf, env, src = inputs[:4]
    sc = orc.Scene(vol, sdf, env, orc.parse_tf(src), case["frame"], case["launch"], threads=1)
    got = record_render(case, inputs, sc)
    missing = _same(got, ref, case["name"])
    assert missing == [case["name"] + ".exit_depths"]  # the one thing only the shim's trace can tell


def test_render_fixture_exercises_every_branch(ref):
    """from the stored data alone: hit and miss pixels, paths that leave the volume at every bounce depth, voxels at and below the
    token cap, refused tokens, cut() and in_volume poses, a launch smaller than the frame"""
    for case in RENDER_CASES:
        n = case["name"]
        hit = ref[n + ".hit_index"]
        w, h = case["launch"]
        assert hit.shape == (w * h,)
        n_hit = int((hit >= 0).sum())
        frame = ref[n + ".frame_last"]
        env_pixels = int((frame[:h, :w, 3] == 200).sum())  # pixels that end in the environment map (ray_marching.cl:172-177, 188-193)
        assert n_hit > 300 and env_pixels > 100 and n_hit + env_pixels == w * h, (n, n_hit, env_pixels)
        assert (frame[:h, :w, 3][hit.reshape(h, w) >= 0] == 1).all()
        if case["launch"] != case["frame"]:
            assert not frame[h:].any() and not frame[:, w:].any()  # outside the launch rectangle nothing is written
        depths = ref[n + ".exit_depths"]
        assert depths.shape == (case["seeds"], 3) and (depths.sum(axis=0) > 50).all(), (n, depths.sum(axis=0))  # i = 8, 9, 10
        counts = ref[n + ".cache_rows"][-1][:, 3]
        assert (counts > 0).all()
        if case["whole"] == "ends":
            assert ref[n + ".contrib"].shape[0] == len(CONTRIB_PASSES) and ref[n + ".contrib"].any(axis=(1, 2)).all()
            assert len(np.unique(ref[n + ".contrib_sha"], axis=0)) == case["seeds"]  # every seed gives another sample
    edge_row = ref["cube_default_edge_on.hit_index"].reshape(64, 96)[32]
    assert (edge_row >= 0).sum() > 30  # rays that enter through the edge itself and hit
    counts = ref["cap.cache_rows"][-1][:, 3]
    assert counts.max() == 256 and 100 < int((counts == 256).sum()) and 100 < int((counts < 256).sum())
    rect = "ragged_gradient_rect"  # reaches the cap too; here the refused tokens are visible pixel by pixel
    assert (ref[rect + ".granted"][0] == 1).all() and 0 < int((ref[rect + ".granted"][-1] == 0).sum())
    counts = ref[rect + ".cache_rows"][-1][:, 3]
    assert counts.max() == 256 and (counts < 256).sum() > 30  # few voxels in so small a rectangle: 3 at the cap, 53 below it


@pytest.mark.parametrize("case", AO_CASES, ids=[c["name"] for c in AO_CASES])
def test_oracle_ao_equals_the_compiled_reference(ref, orc, case):
    """compute_ao (ray_marching.cl:104-149) through oracle/ref/ref_cl_driver.cl: the {samples, occluded} cache after every pass and
    the value every pixel is shaded with; the primary hit is the one of compute_light's fixture run"""
    inputs = case_inputs(case, orc)
    vol, sdf, env, src = inputs[:4]
    sc = orc.Scene(vol, sdf, env, orc.parse_tf(src), case["frame"], case["launch"], threads=1, shading=orc.SHADE_AO)
    n = case["name"]

    def render_ao(pos, d, s):
        sc.render(pos, d, s)
        assert np.array_equal(sc.hit_index, ref[n + ".hit_index"])
        return np.where(sc.hit_index >= 0, sc.frame[..., 0].reshape(-1), 0).astype(np.uint32)

    n_entries = sc.cache.size // 4
    got = record_ao(case, inputs, render_ao, ref[n + ".hit_index"].astype(np.int64), lambda: sc.cache[: n_entries * 2].reshape(-1, 2))
    assert not sc.cache[n_entries * 2:].any()
    assert _same(got, ref, n) == []
    samples = ref[n + ".cache_rows"][-1][:, 0]
    if n == "ao_ragged_gradient":
        assert samples.max() == 100 and (samples == 100).sum() > 10 and (samples < 100).sum() > 10  # at the cap of 100 and below it
    else:
        assert 0 < samples.max() < 100
    occluded = ref[n + ".cache_rows"][-1][:, 1]
    assert occluded.max() > 0 and (occluded < samples).any()
    assert (ref[n + ".hit_index"] >= 0).sum() > 100 and (ref[n + ".hit_index"] < 0).sum() > 100


class _OracleVolumeKernels:
    def __init__(self, orc):
        from oracle import orc_volume

        self.bilateral_filter = orc.bilateral_filter
        self.fetch_stats = orc_volume.fetch_stats
        self.tf_sort_values = orc_volume.tf_sort_values
        self.apply_clip = orc_volume.apply_clip


@pytest.mark.parametrize("dims", VOLUME_DIMS, ids=["%dx%dx%d" % d for d in VOLUME_DIMS])
def test_oracle_volume_kernels_equal_the_compiled_reference(ref_volume, orc, dims):
    """bilateral_filter, fetch_stats, tf_sort_values and apply_clip: orc_filter.c / orc_volume.py against the reference's kernels"""
    got = record_volume_kernels(dims, _OracleVolumeKernels(orc))
    assert _same(got, ref_volume, "v%dx%dx%d" % dims) == ["v%dx%dx%d.reset_zeroed" % dims]  # test_buffer_reset_zeroes_the_volume_grid
    if dims[0] > 8:
        assert len(ref_volume["v%dx%dx%d.hist_bins" % dims]) > 100


def test_buffer_reset_zeroes_the_volume_grid(ref_volume, orc):
    """buffer_reset.cl writes zeros to the entries of the volume's voxels: the first X*Y*Z entries (utility.cl:110) and nothing else"""
    for dims in VOLUME_DIMS:
        zeroed = ref_volume["v%dx%dx%d.reset_zeroed" % dims]
        assert zeroed.tolist() == [0, dims[0] * dims[1] * dims[2] * 4]  # [first, one past the last] ushort written
        assert orc.cache_len(*dims) >= zeroed[1]


def _libs_present():
    from oracle import ref_cl_ffi

    return ref_cl_ffi.available("default") and ref_cl_ffi.available("gradient")


@pytest.mark.skipif(not _libs_present(), reason="oracle/_ref/libref_cl_*.so not built (needs the reference tree at build time)")
def test_fixtures_follow_from_their_recipe(ref, ref_volume, orc):
    """the compiled reference run again gives the stored bytes (what tests/golden/make_ref_render_golden.py would write)"""
    from tests.golden import make_ref_render_golden as maker

    render, volume = maker.generate(orc)
    for got, want in ((render, ref), (volume, ref_volume)):
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
