"""The CPU half of tests/test_gpu_device_functions.py: what that file takes for granted is checked here, without a GPU.

1. The input sets really contain what they are meant to (pairs that tell a contracted sum from the contract's, denormal results,
   decider == 0, rays with two and three successful plane tests, ...).
2. The references are right: the oracle's array probes equal its one-record probes and, where the step is plain arithmetic, numpy's
   binary32 operations in the order written.
3. The rounding condition.  The exact environment route and the tone curve evaluate atan2 / asin / pow in binary64 and round once;
   the device library's binary64 functions are not glibc's, so the two agree after the rounding unless the binary64 value lies next
   to a point where the rounding changes.  A record closer than HARD_ULPS = 32 binary64 ulps to such a point is "hard" (32: OpenCL's
   loosest full-profile bound for the three functions, 16 ulp for pow, plus glibc's, doubled -- the ROCm device-library documents
   installed with the toolchain state no tighter bound for the binary64 functions, so OpenCL's is used); the GPU test demands
   only a neighbouring value there.  At most 1 record in 10^5 of any input set may be hard.  Measured (this file prints the
   figures): the 1 058 618 directions of every size have no hard record (smallest margin 403 ulps for atan2, 266 ulps for asin);
   of the 199 674 tone records exactly one is hard (mean 3263, 2 ulps), and no mean <= 255 comes closer than 75 932 ulps.
4. glibc's (float)f((double)x) is the correctly rounded binary32 value where it matters: against mpmath at 200 bits, for the records
   of every set with the smallest margins (a record with margin m is correctly rounded as soon as glibc's binary64 error is
   below m ulps, so the small margins are the ones at risk), a fixed random sample, and all 65536 tone means.
"""
import ctypes as C

import numpy as np
import pytest

from tests import device_function_inputs as dfi


# ---- 1. conditions on the inputs ---------------------------------------------------------------------------------------------
def test_arith_inputs_distinguish_a_contracted_sum_and_reach_denormal_results():
    a, b, names = dfi.arith_inputs()
    s = names["ordinary"]
    assert s.stop - s.start == 1 << 18
    assert np.all((np.abs(a[s]) >= 2.0 ** -20) & (np.abs(a[s]) <= 2.0 ** 20) & (np.abs(b[s]) >= 2.0 ** -20) & (np.abs(b[s]) <= 2.0 ** 20))
    share = dfi.contraction_shows(a[s], b[s]).mean()
    print("ordinary pairs whose a.x*b.x + a.y*b.y rounds differently when contracted: %.3f" % share)
    assert share >= 0.25
    want = dfi.floats(dfi.arith_reference(a, b))
    tiny = np.float32(2.0 ** -126)
    with np.errstate(invalid="ignore"):
        denormal = (np.abs(want) < tiny) & (want != 0)
    per_column = denormal.sum(axis=0)
    print("denormal results per output:", dict(zip(dfi.ARITH_NAMES, per_column.tolist())))
    assert all(per_column[k] >= 1000 for k in (0, 2, 7, 8, 9))        # quotient, dot3, cross3
    assert per_column[10] >= 1 and per_column[11] >= 1                 # the selects return a denormal operand
    sel = names["select pairs"]
    assert sel.stop - sel.start == 81
    patterns = dfi.bits(a[names["patterns"]])
    exponents = np.unique((patterns >> 23) & 0xFF)
    assert exponents.size == 256                                        # every exponent: denormals, infinities, NaNs among them


def test_hemisphere_inputs_hold_records_with_a_zero_decider(orc):
    d = dfi.hemisphere_inputs(orc)
    assert len(d["records"]) >= 1 << 18 and min(d["zero_found_per_axis"]) >= 16
    decider = orc.hemisphere_decider_n(d["normal"], d["seed"], d["gx"], d["gy"])
    assert int((decider == 0).sum()) >= 16 * 6
    assert (d["seed"] < 0).any() and d["gx"].max() >= 4000 and d["gy"].max() >= 2100
    assert set(np.unique(d["roughness"]).tolist()) == {0.0, 0.25, 1.0}
    zero = ~d["normal"].any(axis=1)
    assert zero.any() and np.isnan(d["normal"]).any()


@pytest.mark.parametrize("box", dfi.CUT_BOXES)
def test_cut_inputs_exercise_the_override_order_and_the_divisions_by_zero(orc, box):
    o, d = dfi.cut_inputs(box)
    assert len(o) >= 1 << 18
    ref, planes = dfi.cut_reference(orc, box, o, d)
    count = np.array([bin(v).count("1") for v in range(8)])[planes]
    print("box", box, "records with 0 / 1 / 2 / 3 successful plane tests:", np.bincount(count, minlength=4).tolist())
    assert (count == 2).sum() >= 100 and (count == 3).sum() >= 100 and (count == 0).sum() >= 100 and (count == 1).sum() >= 100
    zero_over_zero = ((o == 0) & (d == 0)).any(axis=1)
    assert zero_over_zero.sum() >= 100 and ((d == 0).sum(axis=1) == 2).sum() >= 100
    assert np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()
    dim = np.array(box, np.float32)
    on_face = ((o == 0) | (o == dim)).sum(axis=1)
    assert (on_face == 1).sum() >= 64 * 6 and (on_face == 2).sum() >= 64 * 12 and (on_face == 3).sum() >= 64 * 8


def test_ray_inputs_hold_the_degenerate_cameras(orc):
    d = dfi.ray_inputs()
    dirs = dfi.camera_directions()
    assert ((dirs[:, 0] == 0) & (dirs[:, 2] == 0)).sum() >= 6            # parallel to up: the cross product is 0
    length = np.sqrt((dirs.astype(np.float64) ** 2).sum(axis=1))
    assert (length < 1e-19).any() and (length > 1e19).any()
    got = dfi.floats(dfi.ray_reference(orc, d))
    assert np.isnan(got).all(axis=1).any() and not np.isnan(got).all()
    for w, h in dfi.FRAMES_SMALL:
        sel = (d["x_total"] == w) & (d["y_total"] == h)
        assert sel.sum() == w * h * len(dirs)


def test_taps_inputs_hold_irregular_positions():
    p = dfi.taps_inputs()
    want = dfi.taps_reference(p, *dfi.TAPS_DIMS)
    assert (want[:, 0] == 0).sum() >= 1000 and (want[:, 0] == 1).sum() >= 1 << 18
    assert np.isnan(p).any() and np.signbit(p[p == 0]).any() and p.shape[0] <= 1 << 22


# ---- 2. the references ---------------------------------------------------------------------------------------------------------
def _hash_numpy(seed):
    s = np.asarray(seed, np.uint32).copy()
    s = (s ^ np.uint32(61)) ^ (s >> np.uint32(16))
    s = s << np.uint32(3)
    s = s ^ (s >> np.uint32(4))
    s = (s.astype(np.uint64) * np.uint64(0xDEADBEEF) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return s ^ (s >> np.uint32(15))


def test_hash_probe_against_numpy_and_the_one_record_form(orc):
    seeds = dfi.hash_inputs()
    got = orc.hash_n(seeds)
    dfi.assert_same("orc_hash_n vs numpy", seeds[:, None], got, _hash_numpy(seeds), float_columns=False)
    for k in list(range(0, seeds.size, 9973)) + list(range(seeds.size - 5, seeds.size)):
        assert int(got[k]) == orc.lib().orc_hash(int(seeds[k]))


def _hemisphere_numpy(d):
    """utility_sampling.cl:25-50 in numpy: (reflective, plain), binary32 operations one at a time"""
    f = np.float32
    with np.errstate(all="ignore"):
        useed = (d["seed"].astype(np.int64) + (d["gx"].astype(np.int64) + 1) * (d["gy"].astype(np.int64) + 1)) & 0xFFFFFFFF
        draw = []
        for mul in (0x182205bd, 0xe8d052f3, 0xf1981dcf):
            r = _hash_numpy(((useed * mul) & 0xFFFFFFFF).astype(np.uint32)).view(np.int32)
            draw.append((np.fmod(r, np.int32(2048)) - np.int32(1024)).astype(f))     # C's remainder: the sign of the dividend
        direction = np.stack(draw, 1)
        n = d["normal"]

        def normalize(a):
            l = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
            return a / l[:, None]

        decider = (direction[:, 0] * n[:, 0] + direction[:, 1] * n[:, 1]) + direction[:, 2] * n[:, 2]
        plain = normalize(direction * decider[:, None])
        rough = d["roughness"][:, None]
        refl = normalize(n * (f(1) - rough) + plain * rough)
    assert refl.dtype == f and plain.dtype == f
    return np.concatenate([dfi.bits(refl), dfi.bits(plain)], axis=1)


def test_hemisphere_probes_against_numpy_and_the_one_record_forms(orc):
    d = dfi.hemisphere_inputs(orc)
    want = dfi.hemisphere_reference(orc, d)
    dfi.assert_same("orc_hemisphere_*_n vs numpy", d["records"], want, _hemisphere_numpy(d))
    out = (C.c_float * 3)()
    n = len(d["records"])
    for k in list(range(0, n, 4099)) + list(range(n - 300, n, 7)):
        nrm = (C.c_float * 3)(*[float(v) for v in d["normal"][k]])
        orc.lib().orc_hemisphere_reflective(nrm, int(d["seed"][k]), int(d["gx"][k]), int(d["gy"][k]), float(d["roughness"][k]), out)
        dfi.assert_same("orc_hemisphere_reflective one record", d["records"][k:k + 1], dfi.bits(np.array(out[:], np.float32)), want[k:k + 1, :3])
        orc.lib().orc_hemisphere_direction(nrm, int(d["seed"][k]), int(d["gx"][k]), int(d["gy"][k]), out)
        dfi.assert_same("orc_hemisphere_direction one record", d["records"][k:k + 1], dfi.bits(np.array(out[:], np.float32)), want[k:k + 1, 3:])


def test_ray_probe_against_numpy_and_the_one_record_form(orc):
    d = dfi.ray_inputs()
    want = dfi.ray_reference(orc, d)
    dfi.assert_same("orc_generate_ray_n vs numpy", d["records"], want, dfi.ray_numpy(d))
    out = (C.c_float * 3)()
    n = len(want)
    for k in range(0, n, 1009):
        o = (C.c_float * 3)(*[float(v) for v in d["origin"][k]])
        c = (C.c_float * 3)(*[float(v) for v in d["direction"][k]])
        orc.lib().orc_generate_ray(o, c, int(d["x"][k]), int(d["y"][k]), int(d["x_total"][k]), int(d["y_total"][k]), out)
        dfi.assert_same("orc_generate_ray one record", d["records"][k:k + 1], dfi.bits(np.array(out[:], np.float32)), want[k:k + 1])


@pytest.mark.parametrize("box", dfi.CUT_BOXES)
def test_cut_probe_against_numpy_and_the_one_record_form(orc, box):
    o, d = dfi.cut_inputs(box)
    rec = dfi.records(o, d)
    want, planes = dfi.cut_reference(orc, box, o, d)
    ref, ref_planes = dfi.cut_numpy(box, o, d)
    dfi.assert_same("orc_cut_n vs numpy", rec, want, ref, float_columns=[1, 2, 3])
    assert np.array_equal(planes, ref_planes)
    out = (C.c_float * 3)()
    n = len(o)
    for k in list(range(0, n, 2003)) + list(range(n - 10, n)):
        oo = (C.c_float * 3)(*[float(v) for v in o[k]])
        dd = (C.c_float * 3)(*[float(v) for v in d[k]])
        hit = orc.lib().orc_cut(box[0], box[1], box[2], oo, dd, out)
        one = np.concatenate([np.array([hit], np.uint32), dfi.bits(np.array(out[:], np.float32))])
        dfi.assert_same("orc_cut one record", rec[k:k + 1], one, want[k:k + 1], float_columns=[1, 2, 3])


@pytest.fixture(scope="module")
def env_host(tmp_path_factory):
    return dfi.EnvHost(tmp_path_factory.mktemp("envhost"))


@pytest.mark.parametrize("w,h", dfi.ENV_SIZES)
def test_env_probes_against_their_one_record_forms(orc, env_host, w, h):
    d = dfi.env_inputs(w, h)
    want = orc.env_texel_n(d, w, h)
    fast = env_host.texel_fast(d, w, h)
    approx = env_host.approx_bits(d[:, 0], d[:, 2], -d[:, 1])
    ij, out = (C.c_int32 * 2)(), (C.c_int * 2)()
    L = env_host.lib
    L.probe_env_texel_fast.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.probe_atan2_approx.restype = L.probe_asin_approx.restype = C.c_float
    L.probe_atan2_approx.argtypes, L.probe_asin_approx.argtypes = [C.c_float, C.c_float], [C.c_float]
    n = len(d)
    for k in list(range(0, 1 << 20, 5003)) + list(range(1 << 20, n, 37)) + list(range(n - 60, n)):
        v = [float(x) for x in d[k]]
        orc.lib().orc_env_texel((C.c_float * 3)(*v), w, h, ij)
        assert (ij[0], ij[1]) == tuple(want[k]), (k, v)
        ok = L.probe_env_texel_fast(v[0], v[1], v[2], w, h, out)
        assert (ok, out[0], out[1]) == tuple(fast[k]), (k, v)
        one = dfi.bits(np.array([L.probe_atan2_approx(v[0], v[2]), L.probe_asin_approx(-v[1])], np.float32))
        dfi.assert_same("approximations, one record", dfi.bits(d[k:k + 1]), one, approx[k:k + 1])
    # wherever the fast path decides, its texel is the exact contract's (tests/test_env_fast.py, here on every record)
    decided = fast[:, 0] == 1
    assert np.array_equal(fast[decided, 1:], want[decided])
    assert (want >= 0).all() and (want[:, 0] < w).all() and (want[:, 1] < h).all()
    print("%d x %d: %d records, %d undecided by the fast path" % (w, h, n, int((~decided).sum())))


def test_tone_probe_against_its_one_record_form_and_the_curve_taken_apart(orc):
    sums = dfi.tone_inputs()
    want = orc.tone_map_n(sums)
    out = (C.c_uint32 * 4)()
    n = len(sums)
    for k in list(range(0, n, 997)) + list(range(n - 600, n, 3)):
        orc.lib().orc_tone_map((C.c_uint32 * 4)(*[int(v) for v in sums[k]]), out)
        assert list(out) == want[k].tolist(), (k, sums[k])
    # tone_map == the byte of the rounded binary64 curve value, channel by channel (what the margin test reasons about)
    means = dfi.tone_means(sums)
    nonzero = sums[:, 3] != 0
    byte = orc.tone_byte_of_n(orc.tone_pow_n(means.ravel()).astype(np.float32)).reshape(-1, 3)
    assert np.array_equal(byte[nonzero], want[nonzero, :3]) and np.all(want[:, 3] == 1) and not want[~nonzero, :3].any()
    packed = orc.tone_rgba8_n(sums)
    assert np.array_equal(packed >> 24, np.ones(n, np.uint32)) and (want[:, 0] > 255).any()


def test_arith_reference_is_binary32_one_operation_at_a_time():
    """numpy is the definition of the arith probe; make sure it does not widen or fuse: a few results known by hand"""
    f = np.float32
    a = np.array([[1, 2.0 ** -12, 0], [3, 0, 0], [2.0 ** 12 + 1, 2.0 ** 12 + 1, 0], [1, 1, 1]], f)
    b = np.array([[1, 2.0 ** -12, 0], [7, 0, 0], [2.0 ** 12 + 1, -(2.0 ** 12), 1], [3, 3, 3]], f)
    r = dfi.floats(dfi.arith_reference(a, b))
    assert r[0, 2] == f(1)                                   # 1 + 2^-24 rounds to 1 (ties to even)
    assert r[1, 0] == f(0.42857143) and r[1, 1] == f(1.7320508)
    # (2^12+1)^2 = 2^24 + 2^13 + 1 rounds to 2^24 + 2^13; minus (2^12+1) 2^12 = 2^24 + 2^12 gives 2^12, a fused form 2^12 + 1
    assert r[2, 2] == f(2.0 ** 12)
    assert r[3, 2] == f(9) and r[3, 3] == f(1.7320508)


# ---- 3. the rounding condition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", dfi.ENV_SIZES)
def test_env_inputs_stay_clear_of_rounding_boundaries(orc, w, h):
    d = dfi.env_inputs(w, h)
    mt, mp, hard = dfi.env_margins(orc, d)
    n_random = 1 << 20
    print("%d x %d: %d records; smallest margin atan2 %.1f ulps, asin %.1f ulps (random directions: %.1f, %.1f); hard %d"
          % (w, h, len(d), mt.min(), mp.min(), mt[:n_random].min(), mp[:n_random].min(), int(hard.sum())))
    assert len(d) <= 1 << 22
    assert hard.sum() <= dfi.HARD_CAP * len(d)
    assert not hard[:n_random].any()
    # a record that is not hard has one allowed texel: the oracle's
    allowed = dfi.env_allowed_texels(orc, d, w, h)
    ij = orc.env_texel_n(d, w, h).astype(np.int64)
    want = ij[:, 1] * w + ij[:, 0]
    assert (allowed == want[:, None]).any(axis=1).all()


def test_tone_inputs_stay_clear_of_rounding_boundaries(orc):
    sums = dfi.tone_inputs()
    m, hard = dfi.tone_margins(orc, sums)
    r = np.arange(65536, dtype=np.uint32)
    mr = dfi.rounding_margin(orc.tone_pow_n(r))
    p = orc.tone_pow_n(r) * 255.0
    with np.errstate(all="ignore"):
        to_integer = np.abs(p - np.rint(p)) / np.spacing(np.abs(p))
    to_integer[p == np.rint(p)] = np.inf        # 0 and exact values: nothing to misround
    print("tone: %d records, %d hard; means r <= 255: smallest rounding margin %.1f ulps; r <= 65535: %.1f ulps, hard means %s; "
          "smallest distance of 255 p from an integer: %.1f ulps (r <= 255), %.1f ulps (r <= 65535)"
          % (len(sums), int(hard.sum()), mr[1:256].min(), mr[1:].min(), np.flatnonzero(mr < dfi.HARD_ULPS).tolist(),
             to_integer[:256].min(), to_integer.min()))
    assert len(sums) <= 1 << 22
    assert hard.sum() <= dfi.HARD_CAP * len(sums)
    assert not (mr[:256] < dfi.HARD_ULPS).any()
    allowed = dfi.tone_allowed_bytes(orc, sums)
    want = np.minimum(orc.tone_map_n(sums)[:, :3], 255)
    nonzero = sums[:, 3] != 0
    assert (allowed[nonzero] == want[nonzero, :, None]).any(axis=2).all()


# ---- 4. glibc's rounded results are the correctly rounded ones ---------------------------------------------------------------
def _correctly_rounded(mp, exact, got32):
    """got32 (binary32) is a nearest binary32 number to the mpmath value `exact`"""
    g = np.float32(got32)
    if np.isnan(g):
        return False
    d0 = abs(exact - mp.mpf(float(g)))
    for other in (np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(-np.inf))):
        if np.isfinite(other) and abs(exact - mp.mpf(float(other))) < d0:
            return False
    return True


def test_host_atan2_and_asin_round_correctly_where_it_is_closest(orc):
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.prec = 200
    rng = np.random.default_rng(3)
    checked = 0
    for w, h in dfi.ENV_SIZES:
        d = dfi.env_inputs(w, h)
        theta, phi = orc.env_angles_n(d)
        mt, mpg = dfi.rounding_margin(theta), dfi.rounding_margin(phi)
        first = (w, h) == dfi.ENV_SIZES[0]
        rows = np.arange(len(d)) if first else np.arange(1 << 20, len(d))   # the random directions are the same in every set
        pick_t = rows[np.argsort(mt[rows])[:1500 if first else 300]]
        pick_p = rows[np.argsort(mpg[rows])[:1500 if first else 300]]
        sample = rng.choice(rows, 500, replace=False)
        for k in np.unique(np.concatenate([pick_t, sample])):
            x, z = float(d[k, 0]), float(d[k, 2])
            if x == 0 and np.isfinite(z):
                # mpmath has no signed zero; IEEE 754 fixes these results: +-0 towards +z (or z = +0), +-pi towards -z (or z = -0)
                want = np.copysign(np.pi if np.signbit(z) else 0.0, x)
                assert theta[k] == want and np.signbit(theta[k]) == np.signbit(want), (k, d[k], theta[k])
            elif np.isfinite(theta[k]) and np.isfinite(x) and np.isfinite(z):
                assert _correctly_rounded(mp, mp.atan2(mp.mpf(x), mp.mpf(z)), theta[k]), (k, d[k], theta[k])
                checked += 1
        for k in np.unique(np.concatenate([pick_p, sample])):
            y = float(d[k, 1])
            if np.isfinite(phi[k]):
                assert _correctly_rounded(mp, mp.asin(mp.mpf(-y)), phi[k]), (k, d[k], phi[k])
                checked += 1
            else:
                assert not abs(y) <= 1      # NaN exactly where asin has no value
    print("checked %d angles against mpmath" % checked)
    assert checked > 4000


def test_host_tone_curve_rounds_correctly_for_every_mean(orc):
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.prec = 200
    sums = dfi.tone_inputs()
    means = np.unique(np.concatenate([np.arange(65536, dtype=np.uint32), dfi.tone_means(sums).ravel()]))
    p = orc.tone_pow_n(means)
    inv_gamma = mp.mpf(float(np.float32(1.0) / np.float32(1.77777777)))
    for r, v in zip(means.tolist(), p):
        base = float(np.float32(r) / np.float32(255.0) * np.float32(4.0))
        exact = mp.power(mp.mpf(base), inv_gamma) if r else mp.mpf(0)
        assert _correctly_rounded(mp, exact, v), (r, v)
