"""The exact status every invalid call returns (include/clwh.h), one table per entry point.

Nothing here computes a picture: every call but the few marked "valid" is refused.  Two refusals come late by
design -- `resolve_only` without a frame is noticed after the camera's primary hits, and a transfer function
outside the rule grammar is refused by hiprtc -- so the scene is a real (tiny) one with a built SDF.
Descriptors with two faults pin which check comes first.
"""
import ctypes as C

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene

pytestmark = pytest.mark.gpu

INVALID_VALUE, UNKNOWN_KERNEL, TF_UNSUPPORTED, BAD_ARGS, BAD_NDRANGE, SIZE_MISMATCH = 1, 5, 6, 7, 8, 9
N, W, H = 16, 32, 16


def _status(call, *args, **kw):
    try:
        call(*args, **kw)
        return ffi.OK
    except ffi.ClwhError as e:
        return e.status


class _Objects:
    def __init__(self, ctx):
        self.ctx = ctx
        self.tf = scene.tf_default_source()
        self.volume = ctx.image_from(scene.phantom(N))
        self.sdf = ctx.image([N, N, N], 1, np.int8, (N, N, N))
        ctx.sdf_build(self.volume, self.tf, self.sdf)
        self.env = ctx.image_from(scene.env_map(16, 8).astype(np.uint8), channels=4)
        self.frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
        self.cache = ctx.buffer(ffi.cache_len(N, N, N) * 2, np.uint16)
        ctx.buffer_reset(self.cache)
        self.accum = ctx.buffer(ffi.accum_len(W, H, 1) * 16, np.float32)
        self.hit_index = ctx.buffer(W * H * 8, np.int64)
        self.contrib = ctx.buffer(W * H * 16, np.uint32)
        self.volume8 = ctx.image([8, 8, 8], 1, np.int16, (8, 8, 8))
        self.sdf8 = ctx.image([8, 8, 8], 1, np.int8, (8, 8, 8))
        self.tall = ctx.image([2, 65536, 1], 1, np.int16)   # does not fit the grid in y
        self.tall8 = ctx.image([2, 65536, 1], 1, np.int8)
        self.wide_env = ctx.image([32776, 1], 4, np.uint8)
        self.tiny = ctx.buffer(2, np.uint8)
        self.word = ctx.buffer(4, np.uint8)
        self.sixteen = ctx.buffer(16, np.int32)
        self.render = ctx.kernel("ray_marching.cl", "render", self.tf)
        self.pos, self.dir = scene.default_camera(N)

    def release(self):
        self.ctx.finish()
        for v in vars(self).values():
            if isinstance(v, (ffi.Mem, ffi.Kernel)):
                v.release()


@pytest.fixture(scope="module")
def o(gpu_ctx):
    objs = _Objects(gpu_ctx)
    yield objs
    objs.release()


def _handle(m):
    return m.h if m is not None else None


def _render_status(o, kernel="render", n_seeds=0, **kw):
    a = dict(frame=o.frame, volume=o.volume, sdf=o.sdf, env=o.env, buffer_volume=o.cache, accum=None, hit_index=None,
             contrib=None, width=W, height=H, accum_mode=ffi.ACCUM_VOXEL_CACHE, tile_rank=0, tile_world=1, write_frame=1,
             shading=ffi.SHADE_LIGHT, resolve_only=0, seed=1)
    a.update(kw)
    d = ffi.RenderDesc()
    for name in ("frame", "volume", "sdf", "env", "buffer_volume", "accum", "hit_index", "contrib"):
        setattr(d, name, _handle(a[name]))
    for name in ("width", "height", "accum_mode", "tile_rank", "tile_world", "write_frame", "shading", "resolve_only", "seed"):
        setattr(d, name, a[name])
    for q in range(3):
        d.cam_pos[q], d.cam_dir[q] = float(o.pos[q]), float(o.dir[q])
    d.n_seeds = n_seeds
    for q in range(min(max(n_seeds, 0), ffi.MAX_SEEDS)):
        d.seeds[q] = q + 1
    k = o.render if kernel == "render" else kernel
    return ffi.lib().clwh_render(_handle(k), C.byref(d))


IMG = ffi.ACCUM_IMAGE_SPACE
RENDER_CASES = [
    # one fault
    ("frame of the wrong kind", dict(frame="volume"), BAD_ARGS),
    ("volume of the wrong kind", dict(volume="sdf"), BAD_ARGS),
    ("sdf of the wrong kind", dict(sdf="volume"), BAD_ARGS),
    ("env of the wrong kind", dict(env="volume"), BAD_ARGS),
    ("env is a plain buffer", dict(env="cache"), BAD_ARGS),
    ("volume / sdf sizes differ", dict(sdf="sdf8"), SIZE_MISMATCH),
    ("width not a multiple of 8", dict(width=28), BAD_NDRANGE),
    ("height not a multiple of 8", dict(height=12), BAD_NDRANGE),
    ("empty launch", dict(width=0), BAD_NDRANGE),
    ("width above 65535", dict(width=65536), BAD_NDRANGE),
    ("height above 65535", dict(height=65536), BAD_NDRANGE),
    ("env wider than 32768", dict(env="wide_env"), INVALID_VALUE),
    ("rank outside world", dict(tile_rank=1), INVALID_VALUE),
    ("rank outside world of 2", dict(tile_rank=2, tile_world=2), INVALID_VALUE),
    ("negative rank", dict(tile_rank=-1), INVALID_VALUE),
    ("more seeds than CLWH_MAX_SEEDS", dict(n_seeds=ffi.MAX_SEEDS + 1), INVALID_VALUE),
    ("negative seed count", dict(n_seeds=-1), INVALID_VALUE),
    ("several seeds with contrib", dict(n_seeds=2, contrib="contrib"), BAD_ARGS),
    ("unknown shading", dict(shading=2), INVALID_VALUE),
    ("AO with image-space accumulation", dict(shading=ffi.SHADE_AO, accum_mode=IMG, accum="accum"), BAD_ARGS),
    ("unknown accumulation mode", dict(accum_mode=2), INVALID_VALUE),
    ("missing buffer_volume", dict(buffer_volume=None), BAD_ARGS),
    ("short buffer_volume", dict(buffer_volume="word"), BAD_ARGS),
    ("missing accum", dict(accum_mode=IMG), BAD_ARGS),
    ("short accum", dict(accum_mode=IMG, accum="sixteen"), BAD_ARGS),
    ("short hit_index", dict(hit_index="sixteen"), SIZE_MISMATCH),
    ("short contrib", dict(contrib="hit_index"), SIZE_MISMATCH),
    ("resolve_only without a frame", dict(frame=None, resolve_only=1), BAD_ARGS),
    ("no kernel", dict(kernel=None), INVALID_VALUE),
    # two faults: the earlier check wins
    ("wrong frame kind + size mismatch", dict(frame="volume", sdf="sdf8"), BAD_ARGS),
    ("size mismatch + bad width", dict(sdf="sdf8", width=28), SIZE_MISMATCH),
    ("bad width + rank outside world", dict(width=28, tile_rank=1), BAD_NDRANGE),
    ("bad width + missing buffer_volume", dict(width=28, buffer_volume=None), BAD_NDRANGE),
    ("rank outside world + several seeds with contrib", dict(tile_rank=1, n_seeds=2, contrib="contrib"), INVALID_VALUE),
    ("several seeds with contrib + unknown shading", dict(n_seeds=2, contrib="contrib", shading=2), BAD_ARGS),
    ("unknown shading + missing buffer_volume", dict(shading=2, buffer_volume=None), INVALID_VALUE),
    ("missing buffer_volume + short hit_index", dict(buffer_volume=None, hit_index="sixteen"), BAD_ARGS),
    ("unknown accumulation mode + short hit_index", dict(accum_mode=2, hit_index="sixteen"), INVALID_VALUE),
    ("short hit_index + resolve_only without a frame", dict(hit_index="sixteen", frame=None, resolve_only=1), SIZE_MISMATCH),
    ("AO with image-space accumulation + missing accum", dict(shading=ffi.SHADE_AO, accum_mode=IMG), BAD_ARGS),
]


@pytest.mark.parametrize("what,changes,expected", RENDER_CASES, ids=[c[0] for c in RENDER_CASES])
def test_render_status(o, what, changes, expected):
    kw = {k: (getattr(o, v) if isinstance(v, str) else v) for k, v in changes.items()}
    assert _render_status(o, **kw) == expected


def test_render_wrong_kernel_and_null_descriptor(o):
    empty = o.ctx.kernel("empty.cl", "empty")
    assert _render_status(o, kernel=empty) == INVALID_VALUE
    assert ffi.lib().clwh_render(o.render.h, None) == INVALID_VALUE
    empty.release()


def test_projection_status(o):
    """the branches tests/test_gpu_projection.py::test_argument_errors leaves out"""
    L = ffi.lib()

    def status(ctx=o.ctx.h, **kw):
        a = dict(frame=o.frame, volume=o.volume, width=W, height=H, mode=ffi.PROJ_MAX, flags=0, step=0.5, t_near=0.0,
                 t_far=float("inf"), window_center=0.0, window_width=1.0, values=None, t_extreme=None)
        a.update(kw)
        d = ffi.ProjectionDesc()
        for name in ("frame", "volume", "values", "t_extreme"):
            setattr(d, name, _handle(a[name]))
        for name in ("width", "height", "mode", "flags", "step", "t_near", "t_far", "window_center", "window_width"):
            setattr(d, name, a[name])
        for q in range(3):
            d.cam_pos[q], d.cam_dir[q] = float(o.pos[q]), float(o.dir[q])
        return L.clwh_render_projection(ctx, C.byref(d))

    assert status(ctx=None) == INVALID_VALUE
    assert L.clwh_render_projection(o.ctx.h, None) == INVALID_VALUE
    assert status(frame=None) == INVALID_VALUE and status(volume=None) == INVALID_VALUE
    assert status(flags=2) == INVALID_VALUE and status(flags=3) == INVALID_VALUE
    assert status(width=65536) == BAD_NDRANGE and status(height=65536) == BAD_NDRANGE
    # two faults
    assert status(mode=3, width=28) == INVALID_VALUE
    assert status(step=0.0, values=o.sixteen) == INVALID_VALUE
    assert status(width=28, values=o.sixteen) == BAD_NDRANGE
    assert status(width=2 * W, values=o.sixteen) == BAD_NDRANGE  # larger than the frame


def test_sdf_build_status(o):
    L, ctx = ffi.lib(), o.ctx

    def status(volume=o.volume, tf=o.tf, sdf=o.sdf, c=ctx.h):
        return L.clwh_sdf_build(c, _handle(volume), tf.encode() if tf is not None else None, _handle(sdf), None)

    assert status(c=None) == INVALID_VALUE
    assert status(volume=None) == INVALID_VALUE and status(sdf=None) == INVALID_VALUE and status(tf=None) == INVALID_VALUE
    assert status(volume=o.sdf) == BAD_ARGS and status(sdf=o.volume) == BAD_ARGS and status(sdf=o.cache) == BAD_ARGS
    assert status(sdf=o.sdf8) == SIZE_MISMATCH
    assert status(volume=o.tall, sdf=o.tall8) == INVALID_VALUE
    assert status(tf="this is neither a rule table nor C") == TF_UNSUPPORTED
    # two faults
    assert status(volume=o.sdf, sdf=o.sdf8) == BAD_ARGS
    assert status(volume=o.tall, sdf=o.sdf8) == SIZE_MISMATCH
    assert status(sdf=o.sdf8, tf="this is neither a rule table nor C") == SIZE_MISMATCH


def test_kernel_get_status(o):
    ctx = o.ctx
    assert _status(ctx.kernel, "no_such_file.cl", "render") == UNKNOWN_KERNEL
    assert _status(ctx.kernel, "ray_marching.cl", "no_such_entry", o.tf) == UNKNOWN_KERNEL
    assert _status(ctx.kernel, "histogram.cl", "fetch_stats") == UNKNOWN_KERNEL  # a known entry of another file
    assert _status(ctx.kernel, "ray_marching.cl", "render") == TF_UNSUPPORTED  # no prepended source
    assert _status(ctx.kernel, "signed_distance_field.cl", "create_base_image") == TF_UNSUPPORTED
    assert _status(ctx.kernel, "ray_marching.cl", "render", "this is neither a rule table nor C") == TF_UNSUPPORTED
    L, h = ffi.lib(), C.c_void_p()
    assert L.clwh_kernel_get(None, b"empty.cl", b"empty", b"", C.byref(h)) == INVALID_VALUE
    assert L.clwh_kernel_get(ctx.h, None, b"empty", b"", C.byref(h)) == INVALID_VALUE
    assert L.clwh_kernel_get(ctx.h, b"empty.cl", b"empty", b"", None) == INVALID_VALUE
    assert L.clwh_kernel_release(None) == INVALID_VALUE
    # valid: a directory prefix, a kernel that needs no source with and without one
    for file, entry, src in (("kernels/sub/empty.cl", "empty", ""), ("buffer_reset.cl", "buffer_reset", o.tf),
                             ("signed_distance_field.cl", "create_signed_distance_field", "")):
        k = ctx.kernel(file, entry, src)
        k.release()


LAUNCH_KERNELS = {
    "render": ("ray_marching.cl", "render"),
    "reset": ("buffer_reset.cl", "buffer_reset"),
    "stats": ("reference_volume_figures.cl", "fetch_stats"),
    "clip": ("reference_volume_clip.cl", "apply_clip"),
    "sort": ("histogram.cl", "tf_sort_values"),
    "flush": ("histogram.cl", "tf_flush_color_frame"),
    "filter": ("volume_filter.cl", "bilateral_filter"),
    "base": ("signed_distance_field.cl", "create_base_image"),
    "layer": ("signed_distance_field.cl", "create_signed_distance_field"),
    "empty": ("empty.cl", "empty"),
}
G, L1 = (W, H, 1), (8, 8, 1)
CAM = (1.0, 2.0, 3.0, 0.0, 0.0, 1.0)
# (kernel, arguments by name or value, expected); strings name members of _Objects
LAUNCH_CASES = [
    ("render", ("frame", "volume", "sdf", "env", "cache") + CAM, BAD_ARGS),                  # 11 arguments
    ("render", ("frame", "volume", "sdf", "env", "cache") + CAM + (1, 2), BAD_ARGS),         # 13 arguments
    ("render", ("frame", "volume", "sdf", "env", 5) + CAM + (1,), BAD_ARGS),                 # no memory object
    ("render", ("frame", "volume", "sdf", "env", "cache", 1) + CAM[1:] + (1,), BAD_ARGS),    # an integer as camera x
    ("render", ("frame", "volume", "sdf", "env", "cache") + CAM + (1.0,), BAD_ARGS),         # a float as seed
    ("render", ("frame", "volume", "sdf8", "env", "cache") + CAM + (1,), SIZE_MISMATCH),     # what clwh_render says
    ("render", ("volume", "volume", "sdf8", "env", "cache") + CAM + (1,), BAD_ARGS),
    ("reset", ("volume",), BAD_ARGS),
    ("reset", ("volume", 1), BAD_ARGS),
    ("reset", (1, "cache"), BAD_ARGS),
    ("stats", ("volume",), BAD_ARGS),
    ("stats", ("volume", 3), BAD_ARGS),
    ("stats", ("sdf", "sixteen"), BAD_ARGS),
    ("stats", ("volume", "word"), BAD_ARGS),
    ("stats", ("tall", "sixteen"), INVALID_VALUE),
    ("stats", ("tall", "word"), BAD_ARGS),
    ("clip", ("volume", "volume8", "sixteen"), BAD_ARGS),
    ("clip", ("volume", "volume8", "sixteen", 3), BAD_ARGS),
    ("clip", ("volume", "sdf8", "sixteen", "sixteen"), BAD_ARGS),
    ("clip", ("volume", "volume8", "word", "sixteen"), BAD_ARGS),
    ("clip", ("volume", "volume8", "sixteen", "word"), BAD_ARGS),
    ("clip", ("volume", "tall", "sixteen", "sixteen"), INVALID_VALUE),
    ("sort", ("volume", "hit_index", 8, 8, 0.0, 1.0, 0.0), BAD_ARGS),
    ("sort", ("volume", 1, 8, 8, 0.0, 1.0, 0.0, 1.0), BAD_ARGS),
    ("sort", ("volume", "hit_index", 8.0, 8, 0.0, 1.0, 0.0, 1.0), BAD_ARGS),
    ("sort", ("volume", "hit_index", 8, 8, 0, 1.0, 0.0, 1.0), BAD_ARGS),
    ("sort", ("sdf", "hit_index", 8, 8, 0.0, 1.0, 0.0, 1.0), BAD_ARGS),
    ("sort", ("volume", "hit_index", 0, 8, 0.0, 1.0, 0.0, 1.0), BAD_ARGS),
    ("sort", ("volume", "hit_index", 8, -1, 0.0, 1.0, 0.0, 1.0), BAD_ARGS),
    ("sort", ("volume", "sixteen", 8, 8, 0.0, 1.0, 0.0, 1.0), BAD_ARGS),
    ("sort", ("tall", "hit_index", 8, 8, 0.0, 1.0, 0.0, 1.0), INVALID_VALUE),
    ("flush", ("frame", "hit_index", "sixteen"), BAD_ARGS),
    ("flush", ("frame", "hit_index", 4, 4), BAD_ARGS),
    ("flush", ("frame", "hit_index", "sixteen", 1.0), BAD_ARGS),
    ("flush", ("volume", "hit_index", "sixteen", 4), BAD_ARGS),
    ("flush", ("frame", "sixteen", "sixteen", 4), SIZE_MISMATCH),
    ("flush", ("frame", "hit_index", "sixteen", -1), SIZE_MISMATCH),
    ("flush", ("frame", "hit_index", "sixteen", 5), SIZE_MISMATCH),
    ("flush", ("volume", "sixteen", "sixteen", 4), BAD_ARGS),
    ("filter", ("volume",), BAD_ARGS),
    ("filter", ("volume", 1), BAD_ARGS),
    ("filter", ("volume", "sdf"), BAD_ARGS),
    ("filter", ("volume", "volume"), BAD_ARGS),            # in place
    ("filter", ("volume", "volume8"), SIZE_MISMATCH),
    ("base", ("volume", "sdf", "sdf"), BAD_ARGS),
    ("base", ("volume", "sdf", 1, 8), BAD_ARGS),
    ("base", ("volume", "sdf", "sdf", 8.0), BAD_ARGS),
    ("base", ("sdf", "sdf", "sdf", 8), BAD_ARGS),
    ("base", ("volume", "volume", "sdf", 8), BAD_ARGS),
    ("base", ("volume", "sdf", "sdf8", 8), SIZE_MISMATCH),
    ("base", ("volume8", "sdf", "sdf", 8), SIZE_MISMATCH),
    ("base", ("tall", "tall8", "tall8", 8), INVALID_VALUE),
    ("base", ("sdf", "sdf", "sdf8", 8), BAD_ARGS),
    ("layer", ("sdf", "sdf", 1, "word"), BAD_ARGS),
    ("layer", ("sdf", "sdf", 1, 4, 8), BAD_ARGS),
    ("layer", ("sdf", 2, 1, "word", 8), BAD_ARGS),
    ("layer", ("sdf", "sdf", 1.0, "word", 8), BAD_ARGS),
    ("layer", ("sdf", "sdf", 1, "word", 8.0), BAD_ARGS),
    ("layer", ("volume", "sdf", 1, "word", 8), BAD_ARGS),
    ("layer", ("sdf", "sdf", 1, "tiny", 8), BAD_ARGS),
    ("layer", ("sdf", "sdf8", 1, "word", 8), SIZE_MISMATCH),
    ("layer", ("tall8", "tall8", 1, "word", 8), INVALID_VALUE),
    ("layer", ("sdf", "sdf8", 1, "tiny", 8), BAD_ARGS),
]


@pytest.fixture(scope="module")
def kernels(o):
    ks = {name: o.ctx.kernel(file, entry, o.tf if name in ("render", "base") else "") for name, (file, entry) in LAUNCH_KERNELS.items()}
    yield ks
    for k in ks.values():
        k.release()


@pytest.mark.parametrize("case", range(len(LAUNCH_CASES)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(LAUNCH_CASES)])
def test_launch_status(o, kernels, case):
    name, args, expected = LAUNCH_CASES[case]
    args = [getattr(o, a) if isinstance(a, str) else a for a in args]
    assert _status(kernels[name].launch, G, L1, *args) == expected


def test_launch_ndrange_status(o, kernels):
    for name, k in kernels.items():
        # clw_function.hpp:232-237, checked before the arguments of any kernel
        assert _status(k.launch, (30, H, 1), L1) == BAD_NDRANGE, name
        assert _status(k.launch, (4, H, 1), L1) == BAD_NDRANGE, name
        assert _status(k.launch, (W, H, 3), (8, 8, 2)) == BAD_NDRANGE, name
    lib, g = ffi.lib(), (C.c_size_t * 3)(W, H, 1)
    assert lib.clwh_launch(kernels["empty"].h, None, g, None, 0) == INVALID_VALUE
    assert lib.clwh_launch(kernels["empty"].h, g, None, None, 0) == INVALID_VALUE
    assert lib.clwh_launch(kernels["reset"].h, g, g, None, 2) == INVALID_VALUE
    assert lib.clwh_launch(None, g, g, None, 0) == INVALID_VALUE
    assert _status(kernels["empty"].launch, G, L1) == ffi.OK  # valid: launches nothing
    assert _status(kernels["empty"].launch, (W, 0, 0), (8, 0, 0)) == ffi.OK  # a zero extent counts as 1
    # the render kernel's launch size is the NDRange: what clwh_render says about it
    full = [o.frame, o.volume, o.sdf, o.env, o.cache] + list(CAM) + [1]
    assert _status(kernels["render"].launch, (28, 16, 1), (4, 8, 1), *full) == BAD_NDRANGE
    assert _status(kernels["render"].launch, (65536, 16, 1), (8, 8, 1), *full) == BAD_NDRANGE


def test_memory_object_status(o):
    ctx, L = o.ctx, ffi.lib()
    assert _status(ctx.image, [1, 8, 8], 1, np.int16) == INVALID_VALUE   # clw_image.hpp: width must exceed 1
    assert _status(ctx.image, [0, 8, 8], 1, np.int16) == INVALID_VALUE   # (an extent of 0 counts as 1)
    assert _status(ctx.image, [8, 8, 1], 3, np.uint8) == INVALID_VALUE
    assert _status(ctx.image, [8, 8, 1], 0, np.uint8) == INVALID_VALUE
    h, d = C.c_void_p(), (C.c_size_t * 3)(8, 8, 1)
    assert L.clwh_image_create(ctx.h, d, 1, 7, 0, C.byref(h)) == INVALID_VALUE  # no such element kind
    assert L.clwh_image_create(ctx.h, None, 1, ffi.ELEM_U8, 0, C.byref(h)) == INVALID_VALUE
    assert L.clwh_image_create(ctx.h, d, 3, 7, 0, C.byref(h)) == INVALID_VALUE
    assert L.clwh_image_wrap(ctx.h, o.cache.device_ptr, d, 1, 7, C.byref(h)) == INVALID_VALUE
    assert L.clwh_image_wrap(ctx.h, o.cache.device_ptr, d, 3, ffi.ELEM_U8, C.byref(h)) == INVALID_VALUE
    assert L.clwh_image_wrap(ctx.h, None, d, 1, ffi.ELEM_U8, C.byref(h)) == INVALID_VALUE
    assert L.clwh_mem_create(ctx.h, 0, 0, C.byref(h)) == INVALID_VALUE
    assert L.clwh_mem_wrap(ctx.h, None, 16, C.byref(h)) == INVALID_VALUE
    assert L.clwh_mem_wrap(ctx.h, o.cache.device_ptr, 0, C.byref(h)) == INVALID_VALUE
    host = np.zeros(32, np.uint8)
    for nbytes in (15, 17, 0):
        assert L.clwh_mem_push(ctx.h, o.sixteen.h, host.ctypes.data, nbytes) == SIZE_MISMATCH
        assert L.clwh_mem_pull(ctx.h, o.sixteen.h, host.ctypes.data, nbytes) == SIZE_MISMATCH
    assert L.clwh_mem_push(ctx.h, o.sixteen.h, None, 16) == INVALID_VALUE
    assert L.clwh_mem_pull(ctx.h, None, host.ctypes.data, 16) == INVALID_VALUE
    assert L.clwh_mem_push(None, o.sixteen.h, host.ctypes.data, 15) == INVALID_VALUE
    assert L.clwh_mem_release(None) == INVALID_VALUE and L.clwh_mem_mark_dirty(None) == INVALID_VALUE
    assert L.clwh_buffer_reset(ctx.h, None) == INVALID_VALUE


def test_resolve_and_context_status(o):
    ctx, L = o.ctx, ffi.lib()
    tiles = ctx.buffer(ffi.accum_len(W, H, 1) * 4, np.uint8)
    cam = (o.pos, o.dir)
    assert _status(ctx.accum_resolve, o.accum, 0, W, H, o.frame, o.env, *cam) == INVALID_VALUE
    assert _status(ctx.accum_resolve, o.accum, 1, W, H, o.volume, o.env, *cam) == BAD_ARGS
    assert _status(ctx.accum_resolve, o.accum, 1, W, H, o.frame, o.cache, *cam) == BAD_ARGS
    assert _status(ctx.accum_resolve, o.accum, 1, 28, H, o.frame, o.env, *cam) == BAD_NDRANGE
    assert _status(ctx.accum_resolve, o.sixteen, 1, W, H, o.frame, o.env, *cam) == SIZE_MISMATCH
    assert _status(ctx.accum_resolve, o.sixteen, 1, 28, H, o.volume, o.env, *cam) == BAD_ARGS
    assert _status(ctx.accum_resolve, o.sixteen, 1, 28, H, o.frame, o.env, *cam) == BAD_NDRANGE
    assert _status(ctx.accum_resolve_tiles, o.accum, 1, 1, W, H, tiles, o.env, *cam) == INVALID_VALUE
    assert _status(ctx.accum_resolve_tiles, o.accum, 0, 1, W, H, tiles, o.volume, *cam) == BAD_ARGS
    assert _status(ctx.accum_resolve_tiles, o.accum, 0, 1, W, 0, tiles, o.env, *cam) == BAD_NDRANGE
    assert _status(ctx.accum_resolve_tiles, o.accum, 0, 1, W, H, o.sixteen, o.env, *cam) == SIZE_MISMATCH
    assert _status(ctx.accum_resolve_tiles, o.sixteen, 0, 1, W, H, tiles, o.env, *cam) == SIZE_MISMATCH
    assert _status(ctx.frame_from_tiles, tiles, 0, W, H, o.frame) == INVALID_VALUE
    assert _status(ctx.frame_from_tiles, tiles, 1, W, H, o.volume) == BAD_ARGS
    assert _status(ctx.frame_from_tiles, tiles, 1, W, 12, o.frame) == BAD_NDRANGE
    assert _status(ctx.frame_from_tiles, o.sixteen, 1, W, H, o.frame) == SIZE_MISMATCH
    assert _status(ctx.frame_from_tiles, o.sixteen, 1, W, 12, o.volume) == BAD_ARGS
    tiles.release()
    ms, n = (C.c_float * 6)(), (C.c_int32 * 6)()
    assert L.clwh_ctx_timing_read_all(ctx.h, ms, n, 0) == INVALID_VALUE
    assert L.clwh_ctx_timing_read_all(None, ms, n, 6) == INVALID_VALUE
    assert L.clwh_ctx_timing_read(ctx.h, None, n) == INVALID_VALUE
    for f in (L.clwh_ctx_finish, L.clwh_ctx_destroy):
        assert f(None) == INVALID_VALUE
    assert L.clwh_ctx_set_timing(None, 1) == INVALID_VALUE and L.clwh_ctx_invalidate_derived(None, 7) == INVALID_VALUE
    assert L.clwh_ctx_acquire_from(None, None) == INVALID_VALUE and L.clwh_ctx_release_to(None, None) == INVALID_VALUE
    h = C.c_void_p()
    assert L.clwh_ctx_create(0, None) == INVALID_VALUE
    assert L.clwh_ctx_create(-1, C.byref(h)) == 2 and L.clwh_ctx_create(4096, C.byref(h)) == 2  # CLWH_ERR_NO_DEVICE


def test_device_probe_status(o):
    ctx, L = o.ctx, ffi.lib()
    probe = L.clwh_debug_device_probe
    p = (C.c_int32 * 4)(4, 4, 0, 0)
    big, n1 = o.cache.h, C.c_uint64(1)
    assert probe(None, ffi.PROBE_HASH, big, n1, big, None, p) == INVALID_VALUE
    assert probe(ctx.h, ffi.PROBE_HASH, None, n1, big, None, p) == INVALID_VALUE
    assert probe(ctx.h, ffi.PROBE_HASH, big, n1, None, None, p) == INVALID_VALUE
    assert probe(ctx.h, ffi.PROBE_HASH, big, n1, big, None, None) == INVALID_VALUE
    for which in (-1, len(ffi.PROBE_WORDS), 1 << 20):
        assert probe(ctx.h, which, big, n1, big, None, p) == INVALID_VALUE
    assert probe(ctx.h, -1, o.tiny.h, n1, o.tiny.h, None, p) == INVALID_VALUE          # the unknown probe comes before the sizes
    for which, (w_in, w_out) in enumerate(ffi.PROBE_WORDS):
        aux = big if which in (ffi.PROBE_ENV_EXACT, ffi.PROBE_ENV_FAST) else None
        n_in, n_out = C.c_uint64(16 // (4 * w_in) + 1), C.c_uint64(16 // (4 * w_out) + 1)  # one record more than 16 bytes hold
        assert probe(ctx.h, which, o.sixteen.h, n_in, big, aux, p) == SIZE_MISMATCH
        assert probe(ctx.h, which, big, n_out, o.sixteen.h, aux, p) == SIZE_MISMATCH
        assert probe(ctx.h, which, big, C.c_uint64(1 << 31), big, aux, p) == SIZE_MISMATCH
        assert probe(ctx.h, which, o.tiny.h, C.c_uint64(0), o.tiny.h, aux, p) == ffi.OK    # valid: no record
    for which in (ffi.PROBE_ENV_EXACT, ffi.PROBE_ENV_FAST):
        assert probe(ctx.h, which, big, n1, big, None, p) == INVALID_VALUE                  # the image is missing
        assert probe(ctx.h, which, big, n1, big, big, (C.c_int32 * 4)(0, 4, 0, 0)) == INVALID_VALUE
        assert probe(ctx.h, which, big, n1, big, big, (C.c_int32 * 4)(4, -1, 0, 0)) == INVALID_VALUE
        assert probe(ctx.h, which, big, n1, big, o.sixteen.h, (C.c_int32 * 4)(5, 1, 0, 0)) == SIZE_MISMATCH   # 5 texels in 16 bytes
        assert probe(ctx.h, which, big, n1, big, o.sixteen.h, (C.c_int32 * 4)(32768, 32768, 0, 0)) == SIZE_MISMATCH
        assert probe(ctx.h, which, o.tiny.h, n1, big, None, (C.c_int32 * 4)(0, 0, 0, 0)) == INVALID_VALUE     # before the sizes
    assert probe(ctx.h, ffi.PROBE_ENV_EXACT, o.sixteen.h, n1, o.word.h, o.sixteen.h, (C.c_int32 * 4)(2, 2, 0, 0)) == ffi.OK  # valid
    assert probe(ctx.h, ffi.PROBE_HASH, o.sixteen.h, n1, o.word.h, None, p) == ffi.OK   # valid: aux is not looked at
    ctx.finish()


def test_read_back_status(o):
    """clwh_debug_packed_scene and clwh_debug_view_data: on a context that has built nothing, then after one render / one projection
    / one isosurface of the 16^3 scene (8 bricks, 1 cell)"""
    L = ffi.lib()
    scene_arrays = (ffi.SCENE_HIT_RECORDS, ffi.SCENE_STEP_BYTES, ffi.SCENE_BRICK_MIN)
    view_arrays = (ffi.VIEW_BRICKS, ffi.VIEW_TABLE, ffi.VIEW_DILATED, ffi.VIEW_COARSE)
    info = (C.c_int32 * 4)()
    big = np.zeros(8 * 512 * 8, np.uint8)
    out, cap = big.ctypes.data_as(C.c_void_p), C.c_uint64(big.nbytes)
    ctx = ffi.Context(0)
    try:
        for entry, arrays in ((L.clwh_debug_packed_scene, scene_arrays), (L.clwh_debug_view_data, view_arrays)):
            for which in arrays:
                assert entry(ctx.h, which, None, C.c_uint64(0), info) == BAD_ARGS          # nothing built yet
                assert entry(ctx.h, which, out, cap, info) == BAD_ARGS
                assert entry(None, which, out, cap, info) == INVALID_VALUE
                assert entry(ctx.h, which, out, cap, None) == INVALID_VALUE
            for which in (-1, len(arrays), 1 << 20):
                assert entry(ctx.h, which, out, cap, info) == INVALID_VALUE                # the unknown array comes before the data
        assert not big.any()
        volume = ctx.image_from(scene.phantom(N))
        sdf = ctx.image([N, N, N], 1, np.int8, (N, N, N))
        ctx.sdf_build(volume, o.tf, sdf)
        env = ctx.image_from(scene.env_map(16, 8).astype(np.uint8), channels=4)
        frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))
        accum = ctx.buffer(ffi.accum_len(W, H, 1) * 16, np.float32)
        ctx.buffer_reset(accum)
        k = ctx.kernel("ray_marching.cl", "render", o.tf)
        k.render(frame=None, volume=volume, sdf=sdf, env=env, accum=accum, cam_pos=o.pos, cam_dir=o.dir, seed=1, width=W, height=H,
                 mode=ffi.ACCUM_IMAGE_SPACE, write_frame=False)
        packed = L.clwh_debug_packed_scene
        for which, nbytes in zip(scene_arrays, (8 * 512 * 8, 8 * 512, 8 * 4)):
            assert packed(ctx.h, which, None, C.c_uint64(0), info) == ffi.OK and tuple(info) == (2, 2, 2, 0)   # the shape alone
            assert packed(ctx.h, which, out, C.c_uint64(nbytes - 1), info) == SIZE_MISMATCH
            assert packed(ctx.h, which, out, C.c_uint64(0), info) == SIZE_MISMATCH
            assert packed(ctx.h, which, out, C.c_uint64(nbytes), info) == ffi.OK                             # valid
            assert packed(ctx.h, len(scene_arrays), out, C.c_uint64(0), info) == INVALID_VALUE               # before the size
        view = L.clwh_debug_view_data
        assert view(ctx.h, ffi.VIEW_BRICKS, None, C.c_uint64(0), info) == BAD_ARGS        # a render builds no view data
        ctx.render_projection(frame, volume, o.pos, o.dir, W, H)
        for which, nbytes in ((ffi.VIEW_BRICKS, 8 * 512 * 2), (ffi.VIEW_TABLE, 8 * 4)):
            assert view(ctx.h, which, None, C.c_uint64(0), info) == ffi.OK and tuple(info) == (2, 2, 2, 1)
            assert view(ctx.h, which, out, C.c_uint64(nbytes - 1), info) == SIZE_MISMATCH
            assert view(ctx.h, which, out, C.c_uint64(nbytes), info) == ffi.OK
        for which in (ffi.VIEW_DILATED, ffi.VIEW_COARSE):   # only the bricked copy exists: missing, whatever the capacity
            info[:] = [0, 0, 0, 0]
            assert view(ctx.h, which, None, C.c_uint64(0), info) == BAD_ARGS and tuple(info) == (2, 2, 2, 1)
            assert view(ctx.h, which, out, C.c_uint64(0), info) == BAD_ARGS and view(ctx.h, which, out, cap, info) == BAD_ARGS
        ctx.render_isosurface(frame, volume, o.pos, o.dir, W, H, 300.0)
        for which, nbytes in ((ffi.VIEW_DILATED, 8 * 4), (ffi.VIEW_COARSE, 4)):
            assert view(ctx.h, which, None, C.c_uint64(0), info) == ffi.OK
            assert view(ctx.h, which, out, C.c_uint64(nbytes - 1), info) == SIZE_MISMATCH
            assert view(ctx.h, which, out, C.c_uint64(nbytes), info) == ffi.OK
        ctx.invalidate_derived(scene=False, camera=False, projection=True)                # dropped again
        assert all(view(ctx.h, which, out, cap, info) == BAD_ARGS for which in view_arrays)
        ctx.finish()
        for m in (volume, sdf, env, frame, accum, k):
            m.release()
    finally:
        ctx.destroy()
