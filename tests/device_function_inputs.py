"""The input sets of the device-function probes (clwh_debug_device_probe), their references and the rounding margins.

Shared by tests/test_gpu_device_functions.py (device against reference, -m gpu) and tests/test_device_function_inputs_cpu.py
(conditions on the inputs and on the references themselves, no GPU).  Every set has a fixed seed; nothing here touches a GPU.

Comparison is by bits (a signed zero must match in sign) with one exception: two NaNs are equal whatever their payload, because
x86 and gfx950 produce different default NaN patterns.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARD_ULPS = 32.0        # binary64 ulps: OpenCL's loosest full-profile bound of atan2 / asin / pow (16, pow) plus glibc's, doubled
HARD_CAP = 1.0e-5       # at most this share of any input set may be hard
ENV_SIZES = [(4096, 2048), (64, 32), (1000, 333), (1, 1)]
CUT_BOXES = [(10, 10, 10), (512, 512, 512), (130, 20, 9)]
FRAMES_SMALL = [(1, 1), (2, 3), (7, 5)]
FRAMES_LARGE = [(1920, 1080), (3840, 2160)]
DENORMAL = np.array([0x00000001], np.uint32).view(np.float32)[0]   # the smallest one
SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, DENORMAL, -DENORMAL, np.inf, -np.inf, np.nan], np.float32)   # cl_min / cl_max operands


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def floats(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.float32)


def records(*columns):
    """uint32 [n][words]: the columns side by side; float32 columns travel as their bits, integer columns as their low 32 bits"""
    cols = []
    for c in columns:
        c = np.asarray(c)
        c = bits(c) if c.dtype == np.float32 else np.ascontiguousarray(c).astype(np.int64).astype(np.uint32)
        cols.append(c.reshape(c.shape[0], -1))
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def same_bits(got, want, float_columns=True):
    """bool [n][words]: equal as 32-bit words, or both NaN in a float column"""
    got, want = np.ascontiguousarray(got, np.uint32), np.ascontiguousarray(want, np.uint32)
    assert got.shape == want.shape, (got.shape, want.shape)
    eq = got == want
    if float_columns is not False:
        with np.errstate(invalid="ignore"):
            both_nan = np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32))
        if float_columns is not True:   # a list of the columns that hold floats
            mask = np.zeros(got.shape[-1], bool)
            mask[list(float_columns)] = True
            both_nan = both_nan & mask
        eq = eq | both_nan
    return eq


def assert_same(probe, inputs, got, want, float_columns=True, names=None, skip=None):
    """fails naming the probe, the first differing record, its input words and both results"""
    got = np.ascontiguousarray(got, np.uint32).reshape(len(inputs), -1)
    want = np.ascontiguousarray(want, np.uint32).reshape(len(inputs), -1)
    eq = same_bits(got, want, float_columns)
    if skip is not None:
        eq = eq | np.asarray(skip, bool)[:, None]
    if eq.all():
        return
    bad = np.flatnonzero(~eq.all(axis=1))
    k = int(bad[0])
    col = int(np.flatnonzero(~eq[k])[0])
    fmt = lambda row: " ".join("%08x" % int(v) for v in row)  # noqa: E731
    what = names[col] if names else "word %d" % col
    raise AssertionError("probe %s: %d of %d records differ; first: record %d, %s\n  in   %s\n  got  %s\n  want %s\n  as floats: in %s got %s want %s"
                         % (probe, bad.size, len(inputs), k, what, fmt(inputs[k]), fmt(got[k]), fmt(want[k]),
                            floats(inputs[k]), floats(got[k]), floats(want[k])))


# ---- arith ---------------------------------------------------------------------------------------------------------------------
def _ordinary(rng, shape):
    """|x| in 2^-20 .. 2^20, either sign, full random mantissas.  A vector's magnitude is uniform in the exponent over the whole
    range and its components lie within a factor 4 of it: the products of a sum a.x * b.x + a.y * b.y are then of comparable
    size, so that a product kept exact (a fused multiply-add) usually changes the sum's last bit."""
    scale = rng.uniform(-18.0, 18.0, (shape[0], 1))
    mag = np.exp2(scale + rng.uniform(-2.0, 2.0, shape))
    return (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def arith_inputs():
    """(a [n][3], b [n][3], slices by name)"""
    rng = np.random.default_rng(2024)
    parts, names = [], {}

    def add(name, a, b):
        a, b = np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)
        start = sum(len(p[0]) for p in parts)
        names[name] = slice(start, start + len(a))
        parts.append((a, b))

    n = 1 << 20
    pat = rng.integers(0, 2 ** 32, (2, n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)   # every exponent, denormals, inf, NaN
    add("patterns", pat[0], pat[1])
    m = 1 << 18
    add("ordinary", _ordinary(rng, (m, 3)), _ordinary(rng, (m, 3)))
    k = 1 << 12
    mant = lambda: rng.uniform(1.0, 2.0, (k, 3)) * rng.choice([-1.0, 1.0], (k, 3))  # noqa: E731
    add("denormal products", (mant() * 2.0 ** -70).astype(np.float32), (mant() * 2.0 ** -70).astype(np.float32))   # products ~ 2^-140
    add("denormal quotients", (mant() * 2.0 ** -100).astype(np.float32), (mant() * 2.0 ** 35).astype(np.float32))  # a.x / b.x ~ 2^-135
    den = rng.integers(1, 0x00800000, (2, k, 3), dtype=np.uint32) | (rng.integers(0, 2, (2, k, 3), dtype=np.uint32) << 31)
    add("denormal operands", den[0].view(np.float32), _ordinary(rng, (k, 3)))
    add("denormal both", den[0].view(np.float32), den[1].view(np.float32))
    pa, pb = np.meshgrid(SPECIALS, SPECIALS, indexing="ij")   # all ordered pairs in (a.x, b.x)
    ones = np.ones(pa.size, np.float32)
    add("select pairs", np.stack([pa.ravel(), ones, ones], 1), np.stack([pb.ravel(), ones, ones], 1))
    z, nz = np.float32(0.0), np.float32(-0.0)
    vec = [[z, z, z], [nz, nz, nz], [z, nz, z], [1e20, 1e20, 1e20], [-3e19, 2e19, 1e-20], [3.4e38, 0, 0], [1e-30, 1e-30, 1e-30],
           [1e-23, 0, 0], [0, -2e-23, 1e-23], [DENORMAL, 0, 0], [DENORMAL, -DENORMAL, DENORMAL], [1.5e-19, 1.5e-19, 1.5e-19],
           [1.9e19, 0, 0], [np.inf, 1, 1], [np.nan, 1, 1], [1, 0, 0], [0, -1, 0], [3, 4, 0]]
    add("normalize edges", np.array(vec, np.float32), np.array(vec[::-1], np.float32))
    a = np.concatenate([p[0] for p in parts])
    b = np.concatenate([p[1] for p in parts])
    return a, b, names


ARITH_NAMES = ["a.x / b.x", "sqrtf(a.x)", "dot3", "length3", "normalize3.x", "normalize3.y", "normalize3.z", "cross3.x", "cross3.y",
               "cross3.z", "cl_min", "cl_max"]


def arith_reference(a, b):
    """the definition: numpy binary32 operations, one at a time, in the order device_math.hpp writes them"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ax, ay, az, bx, by, bz = a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2]
    with np.errstate(all="ignore"):
        dot = lambda px, py, pz, qx, qy, qz: (px * qx + py * qy) + pz * qz  # noqa: E731
        length = np.sqrt(dot(ax, ay, az, ax, ay, az))
        out = [ax / bx, np.sqrt(ax), dot(ax, ay, az, bx, by, bz), length, ax / length, ay / length, az / length,
               ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx, np.where(bx < ax, bx, ax), np.where(ax < bx, bx, ax)]
    assert all(o.dtype == np.float32 for o in out)
    return np.stack([bits(o) for o in out], axis=1)


def contraction_shows(a, b):
    """bool [n]: a.x * b.x + a.y * b.y, evaluated with either product fused into the addition, differs from the contract's two
    roundings.  Binary64 holds a product of two binary32 numbers exactly; the sum of two of them is rounded to binary64 and then
    to binary32, which can differ from a single rounding only when the sum sits within 2^-29 of a binary32 tie."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    p, q = a64[:, 0] * b64[:, 0], a64[:, 1] * b64[:, 1]
    p32, q32 = p.astype(np.float32), q.astype(np.float32)
    contract = p32 + q32
    fused_q = (p32.astype(np.float64) + q).astype(np.float32)
    fused_p = (p + q32.astype(np.float64)).astype(np.float32)
    return (bits(contract) != bits(fused_q)) | (bits(contract) != bits(fused_p))


# ---- hash ----------------------------------------------------------------------------------------------------------------------
def hash_inputs():
    rng = np.random.default_rng(7)
    return np.concatenate([rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32),
                           np.array([0, 1, 61, 2 ** 31, 2 ** 32 - 1], np.uint32)])


# ---- hemisphere ----------------------------------------------------------------------------------------------------------------
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)


def hemisphere_inputs(orc):
    """dict of columns; `zero_decider`: the records (axis normals) whose decider the oracle finds to be 0"""
    rng = np.random.default_rng(31)
    n = 1 << 18
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm = nrm / np.sqrt((nrm * nrm).sum(axis=1, keepdims=True)).astype(np.float32)
    seed = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    gx, gy = rng.integers(0, 4096, n).astype(np.uint32), rng.integers(0, 2160, n).astype(np.uint32)
    rough = rng.choice(np.array([0.0, 0.25, 1.0], np.float32), n)
    parts = [(nrm, seed, gx, gy, rough)]
    # axis normals: decider == 0 when the drawn component along the axis is 0, one draw in 4096; search, keep 32 per axis
    m = 1 << 19
    zero_rows = []
    for k, axis in enumerate(AXES):
        s = rng.integers(-2 ** 31, 2 ** 31, m, dtype=np.int64).astype(np.int32)
        x, y = rng.integers(0, 4096, m).astype(np.uint32), rng.integers(0, 2160, m).astype(np.uint32)
        an = np.broadcast_to(axis, (m, 3))
        hit = np.flatnonzero(orc.hemisphere_decider_n(an, s, x, y) == 0.0)[:32]
        keep = np.concatenate([hit, np.arange(1024)])   # and ordinary draws on the same normal
        zero_rows.append(len(hit))
        parts.append((an[keep], s[keep], x[keep], y[keep], np.resize(np.array([0.0, 0.25, 1.0], np.float32), keep.size)))
    # a zero normal and a NaN normal, every roughness
    odd = np.array([[0, 0, 0], [-0.0, 0, -0.0], [np.nan, 0, 1], [np.nan, np.nan, np.nan], [np.inf, 0, 0]], np.float32)
    odd = np.repeat(odd, 48, axis=0)
    k = len(odd)
    parts.append((odd, rng.integers(-2 ** 31, 2 ** 31, k, dtype=np.int64).astype(np.int32), rng.integers(0, 4096, k).astype(np.uint32),
                  rng.integers(0, 2160, k).astype(np.uint32), np.resize(np.array([0.0, 0.25, 1.0], np.float32), k)))
    cols = [np.ascontiguousarray(np.concatenate([p[c] for p in parts])) for c in range(5)]
    d = dict(normal=cols[0], seed=cols[1], gx=cols[2], gy=cols[3], roughness=cols[4], zero_found_per_axis=zero_rows)
    d["records"] = records(d["gx"], d["gy"], d["normal"], d["seed"], d["roughness"])
    return d


def hemisphere_reference(orc, d):
    refl = orc.hemisphere_reflective_n(d["normal"], d["seed"], d["gx"], d["gy"], d["roughness"])
    plain = orc.hemisphere_direction_n(d["normal"], d["seed"], d["gx"], d["gy"])
    return np.concatenate([bits(refl), bits(plain)], axis=1)


# ---- ray -----------------------------------------------------------------------------------------------------------------------
def camera_directions():
    rng = np.random.default_rng(17)
    rand = rng.normal(size=(8, 3)).astype(np.float32)
    rand = rand / np.sqrt((rand * rand).sum(axis=1, keepdims=True)).astype(np.float32)
    one_below, one_above = np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))
    near_up = [[0, one_below, 0], [0, one_above, 0], [0, -one_below, 0], [DENORMAL, 1, 0], [0, 1, -DENORMAL], [DENORMAL, 1, DENORMAL],
               [2.0 ** -23, 1, 0], [0, -1, 2.0 ** -24], [1.2e-38, 1, 0]]
    up = [[0, 1, 0], [0, -1, 0], [-0.0, 1, -0.0], [0, 2.5, 0]]
    tiny, huge = rand[:4] * np.float32(1e-20), rand[4:] * np.float32(1e20)
    return np.concatenate([rand, AXES, np.array(up, np.float32), np.array(near_up, np.float32), tiny, huge]).astype(np.float32)


def ray_inputs():
    rng = np.random.default_rng(18)
    dirs = camera_directions()
    cols = []
    for w, h in FRAMES_SMALL:   # every pixel, every direction
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        px = np.stack([xx.ravel(), yy.ravel()], 1)
        k = np.repeat(np.arange(len(dirs)), len(px))
        p = np.tile(px, (len(dirs), 1))
        cols.append((dirs[k], p[:, 0], p[:, 1], np.full(len(k), w), np.full(len(k), h)))
    for w, h in FRAMES_LARGE:   # 2^16 random pixels, each with one of the directions; the four corners with every direction
        n = 1 << 16
        k = rng.integers(0, len(dirs), n)
        cols.append((dirs[k], rng.integers(0, w, n), rng.integers(0, h, n), np.full(n, w), np.full(n, h)))
        for cx, cy in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
            m = len(dirs)
            cols.append((dirs, np.full(m, cx), np.full(m, cy), np.full(m, w), np.full(m, h)))
    d = dict(direction=np.ascontiguousarray(np.concatenate([c[0] for c in cols])))
    for i, name in enumerate(("x", "y", "x_total", "y_total"), start=1):
        d[name] = np.concatenate([c[i] for c in cols]).astype(np.int32)
    d["origin"] = rng.uniform(-600, 600, d["direction"].shape).astype(np.float32)
    d["records"] = records(d["origin"], d["direction"], d["x"], d["y"], d["x_total"], d["y_total"])
    return d


def ray_reference(orc, d):
    return bits(orc.generate_ray_n(d["origin"], d["direction"], d["x"], d["y"], d["x_total"], d["y_total"]))


def ray_numpy(d):
    """utility_ray.cl:69-89 in numpy binary32, one operation at a time (tests the oracle's probe without a GPU)"""
    f = np.float32
    o = d["direction"].astype(f)
    with np.errstate(all="ignore"):
        def cross(a, b):
            return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

        def normalize(a):
            l = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
            return a / l[:, None]

        up = np.broadcast_to(np.array([0, 1, 0], f), o.shape)
        side = normalize(cross(up, o))
        cup = normalize(cross(o, side))
        cup = np.where((cup[:, 1] < 0)[:, None], -cup, cup)
        xt, yt = d["x_total"], d["y_total"]
        x_f = (d["x"] - xt // 2).astype(f)   # totals are positive: // is C's /
        y_f = (d["y"] - yt // 2).astype(f)
        aspect = xt.astype(f) / yt.astype(f)
        x_off = x_f / xt.astype(f) * aspect
        y_off = y_f / yt.astype(f)
        point = (o + side * x_off[:, None]) + cup * y_off[:, None]
        out = normalize(point)
    assert out.dtype == f
    return bits(out)


# ---- cut -----------------------------------------------------------------------------------------------------------------------
def cut_inputs(box):
    """(origin [n][3], direction [n][3]) for a box (X, Y, Z)"""
    rng = np.random.default_rng(1000 + box[0])
    dim = np.array(box, np.float32)
    f = np.float32

    def unit(n):
        v = rng.normal(size=(n, 3)).astype(f)
        return v / np.sqrt((v * v).sum(axis=1, keepdims=True)).astype(f)

    parts = []
    n = 1 << 18
    q = n // 4
    inside = (rng.uniform(0, 1, (q, 3)) * dim).astype(f)
    around = (rng.uniform(-1.0, 2.0, (3 * q, 3)) * dim).astype(f)    # one in 27 inside, the rest outside
    target = (rng.uniform(0, 1, (3 * q, 3)) * dim).astype(f)
    aimed = (target - around).astype(f)
    aimed = aimed / np.sqrt((aimed * aimed).sum(axis=1, keepdims=True)).astype(f)
    away = -aimed[: q]                                                # rays that miss: heading away from the box
    parts.append((inside, unit(q)))
    parts.append((around[:q], unit(q)))
    parts.append((around[q:2 * q], aimed[q:2 * q]))
    parts.append((around[2 * q:], np.concatenate([away[: q // 2], aimed[2 * q: 2 * q + (q - q // 2)]])))
    # origins exactly on each face, edge and corner: every component 0, dim or interior, not all interior; 64 directions each
    m = 64
    for code in range(26):   # digits 0: the component is 0, 1: it is the dimension, 2: interior; 26 = all interior is left out
        c = [(code // 3 ** k) % 3 for k in range(3)]
        o = (rng.uniform(0, 1, (m, 3)) * dim).astype(f)
        for k in range(3):
            if c[k] != 2:
                o[:, k] = 0.0 if c[k] == 0 else dim[k]
        centre = (dim * f(0.5) - o).astype(f)
        d = np.concatenate([unit(m // 2), (centre[: m // 2] + unit(m // 2) * dim * f(0.3)).astype(f)])
        parts.append((o, d))
    # directions with one and with two components equal to +0 and to -0; origins inside and outside
    for zeros in ([0], [1], [2], [0, 1], [0, 2], [1, 2]):
        for z in (f(0.0), f(-0.0)):
            d = unit(256)
            d[:, zeros] = z
            o = np.concatenate([(rng.uniform(0, 1, (128, 3)) * dim), (rng.uniform(-1, 2, (128, 3)) * dim)]).astype(f)
            parts.append((o, d))
            # the origin's component 0 (either sign) or dim where the direction's is 0: 0 / 0, and (dim - dim) / 0
            o2 = o.copy()
            o2[:64, zeros[0]] = 0.0
            o2[64:128, zeros[0]] = -0.0
            o2[128:192, zeros[0]] = dim[zeros[0]]
            o2[192:, zeros] = 0.0
            parts.append((o2, d.copy()))
    # rays along a face, along an edge, through two corners; NaN and infinite components
    odd_o = [[0, 0, 0], [0, 0, 0], dim, dim * f(0.5), [-1, -1, -1], [0, dim[1], 0], dim * f(0.5), dim * f(0.5), [np.nan, 1, 1], [1, 1, 1]]
    odd_d = [[1, 0, 0], dim, -dim, [0, 0, 0], [1, 1, 1], [1, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [0, 1, 0], [-0.0, -0.0, -0.0]]
    parts.append((np.array(odd_o, f), np.array(odd_d, f)))
    return (np.ascontiguousarray(np.concatenate([p[0] for p in parts]), f), np.ascontiguousarray(np.concatenate([p[1] for p in parts]), f))


def cut_reference(orc, box, origin, direction):
    """(uint32 [n][4]: flag, point bits; plane tests [n])"""
    hit, point, planes = orc.cut_n(box, origin, direction)
    return np.concatenate([hit.astype(np.uint32)[:, None], bits(point)], axis=1), planes


def cut_numpy(box, origin, direction):
    """utility_ray.cl:19-66 in numpy binary32, one operation at a time"""
    f = np.float32
    o, d = np.asarray(origin, f), np.asarray(direction, f)
    dim = [f(v) for v in box]
    with np.errstate(all="ignore"):
        def minimum_cut(k):
            a, b = (dim[k] - o[:, k]) / d[:, k], (-o[:, k]) / d[:, k]
            return np.where((a <= 0) | (b <= 0), f(0), np.where(b < a, b, a)).astype(f)

        def within(v, k):
            return (v <= dim[k]) & (v >= 0)

        c = [o + d * minimum_cut(k)[:, None] for k in range(3)]
        ok = [within(c[0][:, 1], 1) & within(c[0][:, 2], 2), within(c[1][:, 0], 0) & within(c[1][:, 2], 2),
              within(c[2][:, 0], 0) & within(c[2][:, 1], 1)]
        cp = np.zeros_like(o)
        for k in range(3):
            cp = np.where(ok[k][:, None], c[k], cp)
    flag = (ok[0] | ok[1] | ok[2]).astype(np.uint32)
    planes = ok[0].astype(np.int32) | (ok[1].astype(np.int32) << 1) | (ok[2].astype(np.int32) << 2)
    return np.concatenate([flag[:, None], bits(cp.astype(f))], axis=1), planes


# ---- environment map -----------------------------------------------------------------------------------------------------------
ENV_SPECIAL = np.array([[0, 1, 0], [0, -1, 0], [0, 0, -1], [-1e-9, 0, -1], [1e-9, 0, -1], [-0.0, 0.3, -1.0],
                        [0, 1.0000001, 0], [0, 0, 0], [np.nan, 0, 1]], np.float32)   # tests/test_env_fast.py's list
_ENV_RANDOM = None


def env_random_directions():
    global _ENV_RANDOM
    if _ENV_RANDOM is None:
        rng = np.random.default_rng(4096)
        d = rng.normal(size=(1 << 20, 3)).astype(np.float32)
        _ENV_RANDOM = d / np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
        _ENV_RANDOM.setflags(write=False)
    return _ENV_RANDOM


def env_inputs(w, h):
    """float32 [n][3]: the random unit directions, then the constructed ones of this size"""
    rng = np.random.default_rng(w)
    k = rng.integers(0, w, size=5000)
    ang = ((k / w) - 0.5) * 2 * np.pi
    columns = np.stack([np.sin(ang), rng.uniform(-0.9, 0.9, size=ang.size), np.cos(ang)], axis=1).astype(np.float32)
    j = rng.integers(0, h, size=5000)
    lat = ((j / h) - 0.5) * np.pi                     # asin(-d.y) on the boundary between rows j - 1 and j
    az = rng.uniform(-np.pi, np.pi, size=j.size)
    rows = np.stack([np.cos(lat) * np.sin(az), -np.sin(lat), np.cos(lat) * np.cos(az)], axis=1).astype(np.float32)
    one = np.float32(1)
    above = np.array([one + np.float32(s * 2.0 ** -23) for s in (1, 2, 3, 8)], np.float32)   # asin gives NaN
    small = rng.uniform(-1e-3, 1e-3, (16, 2)).astype(np.float32)
    beyond = np.stack([small[:, 0], np.tile(np.concatenate([above, -above]), 2), small[:, 1]], axis=1).astype(np.float32)
    seam = np.array([[0, 0, -1], [-0.0, 0, -1], [0, 0, 1], [-0.0, 0, 1], [1, 0, 0], [-1, 0, 0], [1, 0, -0.0], [DENORMAL, 0, -1],
                     [-DENORMAL, 0, -1], [0, 1, -0.0], [-0.0, -1, -0.0], [0, 0.99999994, 0], [0, -0.99999994, 0], [3, 0.5, -4],
                     [np.inf, 0, 1], [1, np.inf, 1], [1e-30, 1e-30, 1e-30]], np.float32)
    return np.ascontiguousarray(np.concatenate([env_random_directions(), columns, rows, ENV_SPECIAL, beyond, seam]), np.float32)


def env_image(w, h):
    """texel (i, j) holds j * w + i: the sampler returns the index it chose"""
    return np.arange(w * h, dtype=np.uint32)


def rounding_margin(v64):
    """distance of each binary64 value from the nearest point where rounding to binary32 changes (the midpoint of two neighbouring
    binary32 numbers), in binary64 ulps of the value; inf for NaN and infinities"""
    v = np.asarray(v64, np.float64)
    with np.errstate(all="ignore"):
        f = v.astype(np.float32)
        up, down = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
        mid_up = f.astype(np.float64) * 0.5 + up.astype(np.float64) * 0.5      # exact: halves of binary32 numbers, 25 bits
        mid_down = f.astype(np.float64) * 0.5 + down.astype(np.float64) * 0.5
        m = np.minimum(np.abs(v - mid_up), np.abs(v - mid_down)) / np.spacing(np.abs(v))
    m[~np.isfinite(v) | ~np.isfinite(m)] = np.inf
    return m


def bracket32(v64):
    """the binary32 neighbours of a binary64 value: (largest <= v, smallest >= v); equal when v is a binary32 number"""
    v = np.asarray(v64, np.float64)
    with np.errstate(all="ignore"):
        f = v.astype(np.float32)
        lo = np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f)
        hi = np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f)
    return lo.astype(np.float32), hi.astype(np.float32)


def env_margins(orc, d):
    """(margin of atan2, margin of asin, hard [n]) for directions d"""
    theta, phi = orc.env_angles_n(d)
    mt, mp = rounding_margin(theta), rounding_margin(phi)
    return mt, mp, (mt < HARD_ULPS) | (mp < HARD_ULPS)


def env_allowed_texels(orc, d, w, h):
    """int64 [n][4]: the texel indices of the binary32 neighbours of both binary64 angles (what a hard record may give)"""
    theta, phi = orc.env_angles_n(d)
    (tl, th), (pl, ph) = bracket32(theta), bracket32(phi)
    out = []
    for t in (tl, th):
        for p in (pl, ph):
            ij = orc.env_texel_of_angles_n(t, p, w, h).astype(np.int64)
            out.append(ij[:, 1] * w + ij[:, 0])
    return np.stack(out, axis=1)


class EnvHost:
    """the host build of csrc/env_fast.hpp (tests/csrc/env_fast_probe.cpp)"""

    def __init__(self, directory):
        so = os.path.join(str(directory), "env_probe.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "csrc", "env_fast_probe.cpp"), "-o", so])
        self.lib = C.CDLL(so)
        for name, args in (("probe_atan2_approx_n", [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]),
                           ("probe_asin_approx_n", [C.c_void_p, C.c_long, C.c_void_p]),
                           ("probe_env_texel_fast_n", [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p])):
            getattr(self.lib, name).argtypes = args
            getattr(self.lib, name).restype = None

    def approx_bits(self, y, x, v):
        """uint32 [n][2]: bits of atan2_approx(y, x) and asin_approx(v)"""
        y, x, v = (np.ascontiguousarray(a, np.float32) for a in (y, x, v))
        out = np.empty((2, y.size), np.uint32)
        self.lib.probe_atan2_approx_n(y.ctypes.data, x.ctypes.data, y.size, out[0].ctypes.data)
        self.lib.probe_asin_approx_n(v.ctypes.data, v.size, out[1].ctypes.data)
        return np.ascontiguousarray(out.T)

    def texel_fast(self, d, w, h):
        """int32 [n][3]: decided, i, j"""
        d = np.ascontiguousarray(d, np.float32)
        out = np.empty((len(d), 3), np.int32)
        self.lib.probe_env_texel_fast_n(d.ctypes.data, len(d), w, h, out.ctypes.data)
        return out


# ---- tone ----------------------------------------------------------------------------------------------------------------------
TONE_COUNTS = (1, 2, 3, 7, 255, 256)


def tone_inputs():
    """uint32 [n][4]: sum r, sum g, sum b, count"""
    rng = np.random.default_rng(99)
    r = np.arange(65536, dtype=np.uint32)
    parts = [np.stack([r, r, r, np.ones_like(r)], 1)]
    for count in TONE_COUNTS:
        sr = np.arange(255 * count + 1, dtype=np.uint32)
        parts.append(np.stack([sr, np.zeros_like(sr), np.zeros_like(sr), np.full_like(sr, count)], 1))
    zero = rng.integers(0, 2 ** 32, (64, 4), dtype=np.uint64).astype(np.uint32)
    zero[:, 3] = 0
    parts.append(zero)
    top = (2 ** 32 - 1 - np.arange(64, dtype=np.uint64)).astype(np.uint32)   # sums near 2^32 - 1
    for count in (1, 2, 255, 256, 65537, 0x01010101, 2 ** 32 - 1):
        c = np.full_like(top, count)
        parts.append(np.stack([top, top[::-1], rng.integers(0, 2 ** 32, 64, dtype=np.uint64).astype(np.uint32), c], 1))
    return np.ascontiguousarray(np.concatenate(parts))


def tone_means(sums):
    """uint32 [n][3]: the channel means the curve is applied to (count 0: none, reported as 0)"""
    s = np.asarray(sums, np.uint32)
    c = np.maximum(s[:, 3], 1)
    return np.where((s[:, 3] == 0)[:, None], 0, s[:, :3] // c[:, None]).astype(np.uint32)


def tone_margins(orc, sums):
    """(margin [n][3] of the curve's binary64 value per channel, hard [n])"""
    means = tone_means(sums)
    m = rounding_margin(orc.tone_pow_n(means.ravel())).reshape(means.shape)
    m[np.asarray(sums)[:, 3] == 0] = np.inf
    return m, (m < HARD_ULPS).any(axis=1)


def tone_allowed_bytes(orc, sums):
    """uint32 [n][3][2]: per channel the bytes of the two binary32 neighbours of the curve's binary64 value"""
    means = tone_means(sums)
    lo, hi = bracket32(orc.tone_pow_n(means.ravel()))
    b = np.stack([np.minimum(orc.tone_byte_of_n(lo), 255), np.minimum(orc.tone_byte_of_n(hi), 255)], axis=1)
    return b.reshape(means.shape[0], 3, 2)


# ---- taps ----------------------------------------------------------------------------------------------------------------------
TAPS_DIMS = (2048, 2048)   # X, Z of cache_entry_of


def taps_inputs():
    rng = np.random.default_rng(55)
    f = np.float32
    ks = [0, 1, 2, 255, 256, 511, 2047, 2 ** 23 - 1]
    below1 = np.nextafter(f(1), f(0))
    fr = [f(0), np.nextafter(below1, f(0)), below1, f(0.5), DENORMAL]
    vals = sorted({float(f(k) + x) for k in ks for x in fr} | {float(f(k)) for k in ks})
    # the sums k + f are rounded to binary32 here; the neighbours of each integer are what matters: add them explicitly
    near = [np.nextafter(f(k + 1), f(0)) for k in ks] + [np.nextafter(np.nextafter(f(k + 1), f(0)), f(0)) for k in ks]
    vals = np.array(sorted(set(vals) | {float(v) for v in near}), f)
    vals = np.concatenate([vals, np.array([-0.0, np.nan], f)])
    g = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(-1, 3)
    rand = rng.uniform(0, 2048, (1 << 18, 3)).astype(f)
    rand = np.minimum(rand, np.nextafter(f(2048), f(0)))   # uniform's upper end may round up to 2048
    return np.ascontiguousarray(np.concatenate([g, rand]), f)


def _f2i(v):
    """DESIGN.md "Semantics": truncate toward zero, saturate, NaN -> 0"""
    v = np.asarray(v, np.float32)
    out = np.zeros(v.shape, np.int64)
    ok = ~np.isnan(v)
    big, small = ok & (v >= 2147483648.0), ok & (v <= -2147483648.0)
    mid = ok & ~big & ~small
    out[big], out[small] = 2147483647, -2147483648
    out[mid] = np.trunc(v[mid].astype(np.float64)).astype(np.int64)
    return out


def taps_reference(p, X, Z):
    """uint32 [n][3]: the flag, and the cache entry (int64) as low and high word; numpy binary32 in the order written"""
    p = np.asarray(p, np.float32)
    one = np.float32(1)
    with np.errstate(all="ignore"):
        reg = np.ones(len(p), bool)
        for k in range(3):
            reg &= np.floor(p[:, k] + one) == np.floor(p[:, k]) + one
    x, y, z = _f2i(p[:, 0]), _f2i(p[:, 1]), _f2i(p[:, 2])
    e = (np.int64(X) * np.int64(Z) * y + np.int64(X) * z + x).astype(np.int64).view(np.uint64)
    return np.stack([reg.astype(np.uint32), (e & np.uint64(0xFFFFFFFF)).astype(np.uint32), (e >> np.uint64(32)).astype(np.uint32)], axis=1)
