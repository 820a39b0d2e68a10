"""-m gpu: the render path's device functions one by one (clwh_debug_device_probe, csrc/probe_kernels.hip), by bits.

Every -m gpu parity test rests on DESIGN.md "Semantics": one binary32 operation at a time in the order written, no contraction,
correctly rounded division and sqrt, denormals kept, saturating conversions, atan2 / asin / pow in binary64 rounded once.  Whole
frames exercise that only at the values a few scenes produce, and a frame that differs does not say which function broke.  Here
each function of csrc/device_math.hpp, render_device.hpp and env_fast.hpp runs on the device over its edges (a camera parallel to
`up`, rays parallel to a face, origins on corners, decider == 0, the poles and the seam of the environment map, NaN and signed-zero
operands of the selects) and is compared with the oracle's probe of the same function -- for the plain arithmetic with numpy's
binary32 operations in the order written, for the certified fast path with the host build of the same header.

A signed zero must match in sign; two NaNs are equal (x86 and gfx950 produce different default NaN patterns).  The inputs, the
references and the rounding condition of the two routes through binary64 functions are tests/device_function_inputs.py's, checked
without a GPU by tests/test_device_function_inputs_cpu.py.  A failure names the probe, the first differing record and its words.
"""
import numpy as np
import pytest

from cl_volume_renderer_amd import ffi
from tests import device_function_inputs as dfi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env_host(tmp_path_factory):
    return dfi.EnvHost(tmp_path_factory.mktemp("envhost"))


def test_arith(gpu_ctx):
    """division, sqrtf, dot3's order, length3, normalize3, cross3 and the two selects: random bit patterns (every exponent, denormals,
    infinities, NaNs), pairs that round differently when contracted, denormal results, every ordered pair of special operands"""
    a, b, names = dfi.arith_inputs()
    rec = dfi.records(a, b)
    got = gpu_ctx.device_probe(ffi.PROBE_ARITH, rec)
    dfi.assert_same("arith", rec, got, dfi.arith_reference(a, b), names=dfi.ARITH_NAMES)


def test_hash(gpu_ctx, orc):
    seeds = dfi.hash_inputs()
    got = gpu_ctx.device_probe(ffi.PROBE_HASH, seeds)
    dfi.assert_same("hash", seeds[:, None], got, orc.hash_n(seeds), float_columns=False)


def test_hemisphere(gpu_ctx, orc):
    """hemisphere_reflective and hemisphere_direction: negative seeds, work-item ids up to 4096 x 2160, decider == 0 (the zero vector
    is normalised: NaN), a zero and a NaN normal"""
    d = dfi.hemisphere_inputs(orc)
    got = gpu_ctx.device_probe(ffi.PROBE_HEMISPHERE, d["records"])
    names = ["reflective.x", "reflective.y", "reflective.z", "direction.x", "direction.y", "direction.z"]
    dfi.assert_same("hemisphere", d["records"], got, dfi.hemisphere_reference(orc, d), names=names)


def test_ray(gpu_ctx, orc):
    """generate_ray: every pixel of 1 x 1, 2 x 3, 7 x 5, random pixels and the corners of 1920 x 1080 and 3840 x 2160; cameras along the
    axes, along +-up (the cross product is 0: NaN), within an ulp of up, and of length 1e-20 and 1e20"""
    d = dfi.ray_inputs()
    got = gpu_ctx.device_probe(ffi.PROBE_RAY, d["records"])
    dfi.assert_same("ray", d["records"], got, dfi.ray_reference(orc, d), names=["direction.x", "direction.y", "direction.z"])


@pytest.mark.parametrize("box", dfi.CUT_BOXES)
def test_cut(gpu_ctx, orc, box):
    """cut_box: origins inside, outside, on faces, edges and corners; direction components +0 and -0 (division by zero, 0 / 0); misses;
    two and three successful plane tests (later axes override)"""
    o, d = dfi.cut_inputs(box)
    rec = dfi.records(o, d)
    got = gpu_ctx.device_probe(ffi.PROBE_CUT, rec, params=(box[0], box[1], box[2], 0))
    want, _ = dfi.cut_reference(orc, box, o, d)
    dfi.assert_same("cut %s" % (box,), rec, got, want, float_columns=[1, 2, 3], names=["flag", "point.x", "point.y", "point.z"])


def test_env_approx(gpu_ctx, env_host):
    """atan2_approx and asin_approx: the device's bits are the host build's (what tests/test_env_fast.py measures on the CPU is what
    gfx950 computes: fmaf, division, sqrtf and copysignf agree)"""
    d = np.concatenate([dfi.env_inputs(*size)[(1 << 20) if k else 0:] for k, size in enumerate(dfi.ENV_SIZES)])
    y, x, v = d[:, 0], d[:, 2], -d[:, 1]
    rec = dfi.records(y, x, v)
    got = gpu_ctx.device_probe(ffi.PROBE_ENV_APPROX, rec)
    dfi.assert_same("env approx", rec, got, env_host.approx_bits(y, x, v), names=["atan2_approx", "asin_approx"])


@pytest.mark.parametrize("w,h", dfi.ENV_SIZES)
def test_env_fast(gpu_ctx, orc, env_host, w, h):
    """sample_environment_map_fast: (decided, texel) is the host build's; wherever decided, the texel is the exact oracle's"""
    d = dfi.env_inputs(w, h)
    rec = dfi.bits(d)
    got = gpu_ctx.device_probe(ffi.PROBE_ENV_FAST, rec, params=(w, h, 0, 0), aux=dfi.env_image(w, h))
    host = env_host.texel_fast(d, w, h)
    decided = host[:, 0] == 1
    index = (host[:, 2].astype(np.int64) * w + host[:, 1]).astype(np.uint32)
    want = np.stack([decided.astype(np.uint32), np.where(decided, index, np.uint32(0xFFFFFFFF))], axis=1)
    dfi.assert_same("env fast %d x %d vs the host build" % (w, h), rec, got, want, float_columns=False, names=["decided", "texel"])
    ij = orc.env_texel_n(d, w, h).astype(np.int64)
    exact = (ij[:, 1] * w + ij[:, 0]).astype(np.uint32)
    chosen = got[:, 0] == 1
    dfi.assert_same("env fast %d x %d vs the exact oracle" % (w, h), rec, got[:, 1], exact, float_columns=False, names=["texel"], skip=~chosen)


@pytest.mark.parametrize("w,h", dfi.ENV_SIZES)
def test_env_exact(gpu_ctx, orc, w, h):
    """sample_environment_map equals orc_env_texel on every record that is not hard; a hard record (its binary64 angle within 32 ulps
    of a binary32 rounding boundary: none in these sets, tests/test_device_function_inputs_cpu.py) must give the texel of one of
    the angle's two binary32 neighbours"""
    d = dfi.env_inputs(w, h)
    rec = dfi.bits(d)
    got = gpu_ctx.device_probe(ffi.PROBE_ENV_EXACT, rec, params=(w, h, 0, 0), aux=dfi.env_image(w, h))[:, 0]
    _, _, hard = dfi.env_margins(orc, d)
    assert hard.sum() <= dfi.HARD_CAP * len(d)
    ij = orc.env_texel_n(d, w, h).astype(np.int64)
    want = (ij[:, 1] * w + ij[:, 0]).astype(np.uint32)
    print("env exact %d x %d: %d records, %d hard" % (w, h, len(d), int(hard.sum())))
    dfi.assert_same("env exact %d x %d" % (w, h), rec, got, want, float_columns=False, names=["texel"], skip=hard)
    if hard.any():
        allowed = dfi.env_allowed_texels(orc, d[hard], w, h)
        ok = (allowed == got[hard].astype(np.int64)[:, None]).any(axis=1)
        assert ok.all(), ("env exact %d x %d, hard record" % (w, h), d[hard][~ok][0], got[hard][~ok][0], allowed[~ok][0])


def test_tone(gpu_ctx, orc):
    """tone_map_rgba8: every mean 0 .. 65535, every sum of counts 1, 2, 3, 7, 255, 256, count 0, sums near 2^32 - 1.  A hard record
    (a channel's binary64 curve value within 32 ulps of a binary32 rounding boundary: exactly one, mean 3263) must give the byte of
    one of the value's two binary32 neighbours"""
    sums = dfi.tone_inputs()
    got = gpu_ctx.device_probe(ffi.PROBE_TONE, sums)[:, 0]
    _, hard = dfi.tone_margins(orc, sums)
    assert hard.sum() <= dfi.HARD_CAP * len(sums)
    print("tone: %d records, %d hard" % (len(sums), int(hard.sum())))
    dfi.assert_same("tone", sums, got, orc.tone_rgba8_n(sums), float_columns=False, names=["rgba8"], skip=hard)
    allowed = dfi.tone_allowed_bytes(orc, sums[hard])
    for k, (word, rows) in enumerate(zip(got[hard].tolist(), allowed)):
        assert word >> 24 == 1, ("tone, hard record", sums[hard][k], hex(word))
        for c in range(3):
            assert (word >> (8 * c)) & 0xFF in rows[c].tolist(), ("tone, hard record", sums[hard][k], hex(word), rows.tolist())


def test_taps(gpu_ctx):
    """taps_are_voxel_neighbours and cache_entry_of: k + f around every integer that matters up to 2^23 - 1 (0.99999994 + 1 rounds to
    2), -0.0, NaN (converts to 0), random positions in [0, 2048)^3 whose entry needs 64 bits"""
    p = dfi.taps_inputs()
    X, Z = dfi.TAPS_DIMS
    rec = dfi.bits(p)
    got = gpu_ctx.device_probe(ffi.PROBE_TAPS, rec, params=(X, Z, 0, 0))
    want = dfi.taps_reference(p, X, Z)
    assert (want[:, 2] != 0).any()   # entries beyond 2^32
    dfi.assert_same("taps", rec, got, want, float_columns=False, names=["regular", "entry low", "entry high"])
