"""The inputs of the SDF builders' event tests (tests/test_gpu_sdf_events.py): volumes, rule tables, their free-form twins for the
hiprtc classifier, shapes, the oracle's field per (volume, table) -- computed once and shared by every build variant -- and the
reference's host loop over the generic launch.  tests/test_sdf_event_cases_cpu.py asserts, without a GPU, that each input decides
events by what it is here for: the zero border texel, the gradient clause, the wrap of the float length converted to short.

Whether a voxel is an event, is_event_gen(value, (short)|gradient|), exists in several hand-written copies on the device (event_at in
sdf_device.hpp under three callers, k_sdfbit_events8 with its own neighbour loads, the compiled classifier of tf_jit.cpp); every one of
them is compared with the oracle (oracle/orc_sdf.c) on these inputs."""
import functools
import re

import numpy as np

from cl_volume_renderer_amd import scene
from oracle import orc_volume


# ---- volumes

def blobs(dims, seed):
    """random smooth blobs: fronts in every direction, seeds in all four parity classes, surfaces that meet the volume's faces"""
    rng = np.random.default_rng(seed)
    Z, Y, X = dims[2], dims[1], dims[0]
    z, y, x = np.mgrid[0:Z, 0:Y, 0:X].astype(np.float32)
    vol = np.full((Z, Y, X), -900.0, np.float32)
    for _ in range(5):
        c = rng.uniform(0, 1, 3) * np.array([X, Y, Z])
        r = rng.uniform(0.08, 0.3) * max(dims)
        vol = np.maximum(vol, 1000.0 - 60.0 * (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r))
    return np.ascontiguousarray(np.clip(vol, -1000, 1100).astype(np.int16))


def extremes(dims, seed):
    """the ends of the short range next to each other and next to values inside the tables' windows (700, 1100): central differences
    up to +-65535, lengths up to 113509 whose squares round in binary32 and whose conversion to short wraps, once or twice"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.choice([-32768, 32767, -32768, 32767, 0, 700, 1100], size=(Z, Y, X)).astype(np.int16))


# ---- rule tables and their free-form twins

TF_GRADIENT = scene.tf_gradient_source()   # value 500..1200, gradient in (100, 4000)
# `gradient < 40000` holds for every short: a voxel in the value window is an event exactly when the WRAPPED length exceeds 100 -- a
# conversion that saturates, or a comparison of the int, gives other events
TF_WRAP = scene.tf_rect_source([(600.0, 1200.0, 100.0, 40000.0, (0.2, 0.4, 0.6, 0.8))], stats=(-40000.0, 40000.0, 0.0, 120000.0))


def free_form_twin(rule_source):
    """the same function with its colour declared ahead of the `if` and every comparison in parentheses: outside the product's rule
    grammar, so it is compiled (tf_jit.cpp)"""
    cond = re.search(r"if\((.*)\)\n", rule_source).group(1)
    colour = re.search(r"tmp_color = (\{[\d,]+\});", rule_source).group(1)
    cond, n = re.subn(r"(value|gradient) (>=|<=|>|<) ([-+.\w]+)", r"(\1 \2 \3)", cond)
    assert n == 4 and rule_source.count("if(") == 1
    return ("inline bool is_event_gen(short value, short gradient, int4 *color){\n"
            "  int4 shade = %s;\n"
            "  if(%s) { *color = shade; return true; }\n"
            "  return false;\n}\n" % (colour, cond))


TABLES = {"gradient": TF_GRADIENT, "wrap": TF_WRAP}
FREE_FORM = {name: free_form_twin(source) for name, source in TABLES.items()}
ROUTES = {"rules": TABLES, "free_form": FREE_FORM}


def window_and_bounds(table):
    """((v_lo, v_hi), (g_lo, g_hi)) of the table's one rule, inclusive, as its text states them (not clamped to a short)"""
    num = r"([-+.\w]+)"
    m = re.search(r"value >= %s && value <= %s && gradient > %s && gradient < %s\)" % (num, num, num, num), TABLES[table])
    v_lo, v_hi, g_lo, g_hi = (int(float(t)) for t in m.groups())
    return (v_lo, v_hi), (g_lo + 1, g_hi - 1)


# ---- shapes (X, Y, Z)

PER_VOXEL_SHAPES = [(70, 33, 45), (65, 49, 17), (130, 3, 7), (2, 40, 40)]   # X % 8 != 0: k_sdfbit_events
PER_VOXEL_REGIONS_SHAPE = (130, 100, 40)                                    # the same with 3 x 3 x 3 regions of 64 x 48 x 16
EIGHT_VOXEL_SHAPES = [(72, 40, 56), (136, 100, 40)]                         # X % 8 == 0: k_sdfbit_events8
WIDE_ROW_SHAPE = (512, 17, 6)                                               # rows of 16 words: k_sdfbit_seed_rows16
BLOB_SHAPES = PER_VOXEL_SHAPES + [PER_VOXEL_REGIONS_SHAPE] + EIGHT_VOXEL_SHAPES + [WIDE_ROW_SHAPE]
EXTREME_SHAPES = [(37, 21, 13), (64, 8, 8), (24, 24, 24)]
RENDER_SHAPE = (72, 40, 56)   # `extremes` as the render path sees its classes: never k_repack's 16-byte path


def blob_seed(dims):
    return sum(dims) + (1 if dims == WIDE_ROW_SHAPE else 0)   # (as tests/test_gpu_sdf.py seeds them)


# (kind, dims, seed, table)
BLOB_CASES = [("blobs", dims, blob_seed(dims), "gradient") for dims in BLOB_SHAPES]
EXTREME_CASES = [("extremes", dims, sum(dims), "wrap") for dims in EXTREME_SHAPES]
CASES = BLOB_CASES + EXTREME_CASES
RENDER_CASE = ("extremes", RENDER_SHAPE, sum(RENDER_SHAPE), "wrap")
GENERIC_LAUNCH_CASES = [BLOB_CASES[0], EXTREME_CASES[0]]   # (70, 33, 45) and (37, 21, 13): the layer kernels one launch at a time


def case_id(case):
    kind, dims, seed, table = case
    return "%s-%dx%dx%d-%s" % (kind, dims[0], dims[1], dims[2], table)


@functools.lru_cache(maxsize=None)
def volume(kind, dims, seed):
    """the case's volume [z][y][x], made once; read-only, because every test of the session shares it"""
    vol = {"blobs": blobs, "extremes": extremes}[kind](dims, seed)
    vol.setflags(write=False)
    return vol


_ORACLE = {}


def oracle_sdf(orc, kind, dims, seed, table):
    """(field, launches) of the oracle under the RULE table `table` (a name of TABLES, or "default"), once per session"""
    key = (kind, dims, seed, table)
    if key not in _ORACLE:
        source = scene.tf_default_source() if table == "default" else TABLES[table]
        want, launches, _ = orc.sdf_build(volume(kind, dims, seed), orc.parse_tf(source))
        want.setflags(write=False)
        _ORACLE[key] = (want, launches)
    return _ORACLE[key]


# ---- the event test in numpy, independent of the oracle

def differences(vol, border):
    """central differences (gx, gy, gz), int32 [z][y][x], without the factor 1/2; outside the volume the border texel 0 ("zero": what
    read_imagei gives) or the nearest voxel ("edge")"""
    v = np.asarray(vol).astype(np.int32)
    p = np.pad(v, 1, mode="constant") if border == "zero" else np.pad(v, 1, mode="edge")
    return (p[1:-1, 1:-1, 2:] - p[1:-1, 1:-1, :-2], p[1:-1, 2:, 1:-1] - p[1:-1, :-2, 1:-1], p[2:, 1:-1, 1:-1] - p[:-2, 1:-1, 1:-1])


def length_int(gx, gy, gz):
    """(int) length(float3): binary32 products, summed (x + y) + z, correctly rounded square root, truncated"""
    fx, fy, fz = gx.astype(np.float32), gy.astype(np.float32), gz.astype(np.float32)
    return np.sqrt((fx * fx + fy * fy) + fz * fz, dtype=np.float32).astype(np.int32)


def events_of(vol, table, length=None, convert="wrap"):
    """the event set of a one-rule table from the int length per voxel: `convert` says how the int becomes the short that is compared
    ("wrap": the C conversion, "saturate", or "int": no conversion)"""
    if length is None:
        length = orc_volume.gradient_length_int(np.asarray(vol))
    (v_lo, v_hi), (g_lo, g_hi) = window_and_bounds(table)
    g = {"wrap": lambda a: a.astype(np.int16).astype(np.int32), "saturate": lambda a: np.clip(a, -32768, 32767), "int": lambda a: a}[convert](length)
    if convert != "int":
        g_hi = min(g_hi, 32767)   # a short is compared: every short is below 40000
    v = np.asarray(vol).astype(np.int32)
    return (v >= v_lo) & (v <= v_hi) & (g >= g_lo) & (g <= g_hi)


# ---- app/signed_distance_field.cpp:7-35 call by call over clwh_kernel_get / clwh_launch

def reference_host_loop(ctx, vol, code):
    """what the reference's unmodified host code does through the clw_* wrappers: create_base_image, then create_signed_distance_field
    layer by layer with the counter read back, on a global size rounded up to the local size's multiple (so it exceeds the volume).
    Returns (launches, the image the reference hands out [z][y][x])."""
    Z, Y, X = vol.shape
    v = ctx.image_from(np.ascontiguousarray(vol, np.int16))
    sdf = ctx.image([X, Y, Z], 1, np.int8, (Z, Y, X)); sdf.push(np.zeros((Z, Y, X), np.int8))
    pong = ctx.image([X, Y, Z], 1, np.int8, (Z, Y, X))
    max_it = min(max(X, Y, Z) // 2, 127)
    ev = lambda g, l: (g + l - 1) // l * l  # noqa: E731  evenness(), app/common.hpp:59-66
    gsz = [ev(X, 8), ev(Y, 8), ev(Z, 8)]
    base = ctx.kernel("signed_distance_field.cl", "create_base_image", code)
    base.launch(gsz, [4, 4, 4], v, sdf, pong, np.uint32(max_it))
    layer = ctx.kernel("signed_distance_field.cl", "create_signed_distance_field", code)
    counter = ctx.buffer(4, np.int32)
    ping_, pong_ = sdf, pong
    launches = 0
    for i in range(1, max_it + (max_it % 2) + 1 + 1):
        counter.push(np.zeros(1, np.int32))
        layer.launch(gsz, [4, 4, 4], ping_, pong_, np.uint32(i), counter, np.uint32(max_it))
        ping_, pong_ = pong_, ping_
        launches += 1
        if counter.pull()[0] == 0 and i % 2 == 1:
            break
    out = sdf.pull()
    for m in (v, sdf, pong, counter, base, layer):
        m.release()
    return launches, out
