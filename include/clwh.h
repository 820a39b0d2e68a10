/*
 * clwh.h -- C ABI of libclwhip.so: the thin HIP shim that replaces the reference's
 * `opencl_wrapper` (clw_*) layer for the volumetric path-tracing hot path on MI355X (gfx950).
 *
 * Every entry point names the reference interface it replaces (paths relative to the reference
 * repository).  Conventions:
 *   - plain C: opaque handles, pointers and sizes; no exceptions, no callbacks;
 *   - every function returns an int status (CLWH_OK == 0); clwh_strerror() names it;
 *   - a handle is owned by whoever created it and is released explicitly; host pointers are
 *     only borrowed for the duration of a call;
 *   - one in-order HIP stream per context; push/pull are blocking like the reference's
 *     CL_TRUE transfers; launches are asynchronous and stream-ordered;
 *   - single host thread per context (the reference's ui::run loop).
 * The fail-hard convention of the reference (print + exit(1), clw_helper.hpp:293-309) lives in
 * the header-only C++ wrappers (include/clw_*.hpp), not in this ABI.
 */
#ifndef CLWH_H
#define CLWH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct clwh_ctx clwh_ctx;       /* replaces clw_context        (opencl_wrapper/include/clw_context.hpp:5-28) */
typedef struct clwh_mem clwh_mem;       /* replaces cl_mem of clw_vector / clw_image */
typedef struct clwh_kernel clwh_kernel; /* replaces cl_program + cl_kernel of clw_function */

enum clwh_status {
  CLWH_OK = 0,
  CLWH_ERR_INVALID_VALUE = 1,
  CLWH_ERR_NO_DEVICE = 2,
  CLWH_ERR_OUT_OF_MEMORY = 3,
  CLWH_ERR_HIP = 4,            /* a HIP runtime call failed; clwh_last_hip_error() has the code */
  CLWH_ERR_UNKNOWN_KERNEL = 5, /* (file, entry) is not one of the precompiled hot-path kernels */
  CLWH_ERR_TF_UNSUPPORTED = 6, /* the transfer-function source neither parses as rules nor compiles with hiprtc */
  CLWH_ERR_BAD_ARGS = 7,       /* wrong number / kind of kernel arguments */
  CLWH_ERR_BAD_NDRANGE = 8,    /* global not a multiple of local, zero size, ... */
  CLWH_ERR_SIZE_MISMATCH = 9,
  CLWH_ERR_INTERNAL_OVERFLOW = 10 /* a device-side work buffer overflowed; results of the last render are incomplete */
};

/* element kinds of an image channel: (signedness, sizeof) as clw_image picks them
 * (opencl_wrapper/include/clw_image.hpp:68-110) */
enum clwh_elem_kind {
  CLWH_ELEM_S8 = 0, CLWH_ELEM_S16 = 1, CLWH_ELEM_S32 = 2,
  CLWH_ELEM_U8 = 3, CLWH_ELEM_U16 = 4, CLWH_ELEM_U32 = 5,
  CLWH_ELEM_F32 = 6
};

enum clwh_mem_flags { CLWH_MEM_READ_WRITE = 0, CLWH_MEM_READ_ONLY = 1 };

/* ---- context: clw_context::clw_context / ~clw_context (opencl_wrapper/src/clw_context.cpp:38-83).
 * The reference takes platform[0]/device[0]; here the HIP device ordinal is explicit. */
int clwh_ctx_create(int device, clwh_ctx **out);
/* same, but enqueue on a stream the caller owns (e.g. PyTorch's current stream); NULL = default */
int clwh_ctx_create_on_stream(int device, void *hip_stream, clwh_ctx **out);
int clwh_ctx_destroy(clwh_ctx *ctx);
/* clFinish on the context's queue */
int clwh_ctx_finish(clwh_ctx *ctx);
void *clwh_ctx_stream(clwh_ctx *ctx);
int clwh_ctx_device(clwh_ctx *ctx);

/* ---- memory objects.
 * clwh_mem_create    replaces clCreateBuffer in clw_vector's ctor (clw_vector.hpp:14-33)
 * clwh_image_create  replaces clCreateImage in clw_image's ctor  (clw_image.hpp:18-137);
 *                    dims of 0 count as 1; 1-D/2-D/3-D follows from the dims
 * clwh_mem_wrap      adopts device memory the caller allocated (a torch tensor's data_ptr) or that another
 *                    clwh_mem -- of this or another context -- already names; never freed by the shim.  All objects
 *                    that name the same device pointer share ONE content version: a push, clwh_sdf_build or
 *                    clwh_mem_mark_dirty through any of them invalidates what every context derived from it
 * clwh_mem_push/pull replace the blocking clEnqueueWrite/Read{Buffer,Image}
 *                    (clw_vector.hpp:73-86, clw_image.hpp:202-216); `bytes` must equal the object size
 */
int clwh_mem_create(clwh_ctx *ctx, size_t bytes, int flags, clwh_mem **out);
int clwh_mem_wrap(clwh_ctx *ctx, void *device_ptr, size_t bytes, clwh_mem **out);
int clwh_image_create(clwh_ctx *ctx, const size_t dims[3], int channels, int elem_kind, int flags,
                      clwh_mem **out);
int clwh_image_wrap(clwh_ctx *ctx, void *device_ptr, const size_t dims[3], int channels,
                    int elem_kind, clwh_mem **out);
int clwh_mem_push(clwh_ctx *ctx, clwh_mem *mem, const void *host, size_t bytes);
int clwh_mem_pull(clwh_ctx *ctx, clwh_mem *mem, void *host, size_t bytes);
int clwh_mem_release(clwh_mem *mem);
/* page-lock / unlock a host buffer the caller keeps pushing from or pulling into (the host mirror of a clw_image,
 * e.g. the 8 MiB frame renderer::render_frame pulls after every pass, app/renderer.cpp:150): transfers then run as
 * one DMA instead of being staged through the runtime's bounce buffers.  Optional; never changes results. */
int clwh_host_register(void *host, size_t bytes);
int clwh_host_unregister(void *host);
void *clwh_mem_device_ptr(clwh_mem *mem);
size_t clwh_mem_size(clwh_mem *mem);
/* tell the shim that device code outside it rewrote the object (invalidates derived layouts) */
int clwh_mem_mark_dirty(clwh_mem *mem);

/* ---- kernels.
 * clwh_kernel_get replaces clw_function's ctor (clw_function.hpp:74-111): instead of flattening
 * `#clw_include_once`, prepending `prepend` and JIT-compiling, it looks (file, entry) up in the
 * registry of precompiled HIP kernels and parses `prepend` (the generated `is_event_gen` source,
 * app/ui.cpp:160-168) into a rule table that becomes a launch-time parameter; source outside the rule
 * grammar is compiled with hiprtc into a per-voxel classifier (csrc/tf_jit.cpp), so any `is_event_gen`
 * the reference's JIT would accept is accepted here too (up to 16 distinct colours).
 * Known pairs: ("ray_marching.cl","render"), ("signed_distance_field.cl","create_base_image"),
 * ("signed_distance_field.cl","create_signed_distance_field"), ("buffer_reset.cl","buffer_reset"),
 * ("empty.cl","empty"), and next to the hot path ("reference_volume_figures.cl","fetch_stats"),
 * ("reference_volume_clip.cl","apply_clip"), ("volume_filter.cl","bilateral_filter"),
 * ("histogram.cl","tf_sort_values"), ("histogram.cl","tf_flush_color_frame").
 */
int clwh_kernel_get(clwh_ctx *ctx, const char *file, const char *entry, const char *prepend,
                    clwh_kernel **out);
int clwh_kernel_release(clwh_kernel *k);

enum clwh_arg_kind { CLWH_ARG_MEM = 0, CLWH_ARG_I32 = 1, CLWH_ARG_U32 = 2, CLWH_ARG_F32 = 3,
                     CLWH_ARG_I64 = 4, CLWH_ARG_U64 = 5, CLWH_ARG_F64 = 6 };
typedef struct clwh_arg {
  int32_t kind;
  int32_t reserved;
  union {
    clwh_mem *mem;
    int32_t i32;
    uint32_t u32;
    float f32;
    int64_t i64;
    uint64_t u64;
    double f64;
  } v;
} clwh_arg;

/* clwh_launch replaces clw_function::execute (clw_function.hpp:217-244): zeros in global/local
 * count as 1; global must be a multiple of local (the reference asserts it); the argument list is
 * the reference kernel's own, in order (clSetKernelArg by position, clw_function.hpp:152-167). */
int clwh_launch(clwh_kernel *k, const size_t global[3], const size_t local[3], const clwh_arg *args,
                int nargs);

/* ---- hot-path entry points beyond the generic launch (used by the C++ host mirror and bench).
 *
 * clwh_render: one `render` pass = one sample per pixel (app/renderer.cpp:145-148 +
 * opencl_kernels/ray_marching.cl:152-199), with the options the MI355X design adds.
 */
enum clwh_accum_mode {
  CLWH_ACCUM_VOXEL_CACHE = 0, /* reference-exact world-space cache (utility.cl:20-54) */
  CLWH_ACCUM_IMAGE_SPACE = 1  /* per-pixel float4 {r,g,b,count}, no token cap (multi-GPU tiles) */
};
/* Which of the reference's two shading functions `render` runs.  ray_marching.cl:186 calls compute_light; compute_ao
 * (:104-149) is the alternate the authors kept in the file.  AO needs accum_mode CLWH_ACCUM_VOXEL_CACHE: it keeps
 * {samples, occluded} as 2 ushorts per voxel in buffer_volume (utility.cl:123-159; at least clwh_cache_len()/2
 * ushorts), capped at 100 samples per voxel.  compute_ao's return value has w == 0, which the reference's render()
 * would overpaint with the environment colour (:187-195); here an AO hit pixel resolves to {v, v, v, 1},
 * v = 2 * (100 - occluded), the value compute_ao returns. */
enum clwh_shading { CLWH_SHADE_LIGHT = 0, CLWH_SHADE_AO = 1 };
typedef struct clwh_render_desc {
  clwh_mem *frame;          /* RGBA8 2-D image; its dims are what get_image_width/height(frame) return */
  clwh_mem *volume;         /* S16 3-D image */
  clwh_mem *sdf;            /* S8 3-D image */
  clwh_mem *env;            /* RGBA8 2-D image */
  clwh_mem *buffer_volume;  /* voxel cache, clwh_cache_len() ushorts (mode 0) */
  float cam_pos[3];
  float cam_dir[3];
  int32_t seed;             /* the pass's random seed (renderer.cpp:142) when n_seeds == 0 */
  uint32_t width, height;   /* NDRange global size (multiples of 8) */
  int32_t accum_mode;
  clwh_mem *accum;          /* mode 1: float4 per pixel, tile-major (see clwh_accum_len) */
  int32_t tile_rank, tile_world; /* image-tile partition: 8x8 tiles, owner = (tx + ty) % world */
  int32_t write_frame;      /* 1: resolve the frame (deterministic, after all adds of the pass) */
  clwh_mem *hit_index;      /* optional int64 per pixel, row-major: cache entry or -1 (parity tests) */
  clwh_mem *contrib;        /* optional uint32[4] per pixel, row-major: r,g,b,granted (parity tests; one seed) */
  int32_t n_seeds;          /* > 0: render n_seeds passes (<= CLWH_MAX_SEEDS) in ONE launch, seeds[] below; the
                               result equals n_seeds consecutive single-seed calls (image-space mode always; voxel
                               cache mode while no voxel reaches the 256-token cap).  ceil(hit pixels / 64) x
                               n_seeds must stay below 2^24 (64 seeds: 16.7 M hit pixels), else
                               CLWH_ERR_INVALID_VALUE: use fewer seeds per launch */
  int32_t seeds[64];
  int32_t shading;          /* enum clwh_shading; 0 (zero-initialised descriptors) = compute_light */
  int32_t resolve_only;     /* 1: no pass; only resolve `frame` from buffer_volume / accum for this camera (the read-back
                               half of compute_light, ray_marching.cl:82-99) -- e.g. after the cache was updated by an
                               exchange between ranks */
} clwh_render_desc;
#define CLWH_MAX_SEEDS 64
int clwh_render(clwh_kernel *render_kernel, const clwh_render_desc *desc);

/* number of ushorts of a voxel cache for an X*Y*Z volume (the reference allocates X*Y*Z*4,
 * app/renderer.cpp:29-30, and can index one row past it, utility.cl:21 with utility_ray.cl:112-117;
 * the shim's kernels require the padded length) */
int64_t clwh_cache_len(uint32_t X, uint32_t Y, uint32_t Z);
/* number of float4 of a rank's tile-major accumulation buffer */
int64_t clwh_accum_len(uint32_t width, uint32_t height, int32_t tile_world);
/* resolve the RGBA8 frame from the tile-major accumulation buffers of all ranks laid back to back
 * (what the RCCL all-gather produces): hit pixels (count > 0) get ray_marching.cl:82-99 applied to
 * their sums; the others get the environment colour of their camera ray, alpha 200
 * (ray_marching.cl:172-178), which is why the camera and the env map are arguments. */
int clwh_accum_resolve(clwh_ctx *ctx, clwh_mem *accum_all_ranks, int32_t tile_world, uint32_t width,
                       uint32_t height, clwh_mem *frame_rgba8, clwh_mem *env, const float cam_pos[3],
                       const float cam_dir[3]);
/* The same resolve for several GPUs with a quarter of the exchange: a rank first resolves ITS tiles to RGBA8
 * (`tiles_rgba8`: clwh_accum_len(width, height, tile_world) 32-bit pixels, tile-major in the slot order of its accumulation
 * buffer), the ranks all-gather those 4-byte pixels instead of 16-byte sums, and clwh_frame_from_tiles puts all ranks' tiles,
 * laid back to back, into the row-major frame.  Pixel for pixel the result of clwh_accum_resolve (the resolve of
 * ray_marching.cl:82-99 / :172-178 is per pixel). */
int clwh_accum_resolve_tiles(clwh_ctx *ctx, clwh_mem *accum, int32_t tile_rank, int32_t tile_world, uint32_t width,
                             uint32_t height, clwh_mem *tiles_rgba8, clwh_mem *env, const float cam_pos[3],
                             const float cam_dir[3]);
int clwh_frame_from_tiles(clwh_ctx *ctx, clwh_mem *tiles_all_ranks, int32_t tile_world, uint32_t width, uint32_t height,
                          clwh_mem *frame_rgba8);
/* drop what the context derived from its inputs; the next clwh_render rebuilds it.  Needed only to time the
 * rebuild or to render "the first frame after a camera move" again (memory rewritten behind the shim's back
 * is what clwh_mem_mark_dirty is for).
 *   CLWH_DERIVED_SCENE   step bytes + hit records + exit-certificate table (function of volume, SDF, transfer
 *                        function: flush-time data).  There is ONE copy per device: contexts that render the same
 *                        (volume content, SDF content, transfer function) share it -- 9 bytes per voxel, 72 GiB at
 *                        2048^3 -- and it is freed when the last of them lets go.  Invalidating makes THIS context
 *                        rebuild; contexts already sharing the old copy keep it until their own inputs change.
 *   CLWH_DERIVED_CAMERA  primary hits (function of the camera and of the scene), per context
 *   CLWH_DERIVED_PROJECTION  the bricked int16 copy of the volume + per-brick {min, max} table that clwh_render_projection and
 *                        clwh_render_composite share, per context (ONE copy: 2 bytes per voxel + 4 per 8^3 brick), and with it the
 *                        prefix count over clwh_render_composite's colour/opacity table (4 bytes per entry) and the dilated
 *                        {min, max} tables that clwh_render_isosurface, clwh_render_slice and clwh_mesh_isosurface share (4 bytes
 *                        per brick and per 4^3 bricks): all are dropped */
enum clwh_derived { CLWH_DERIVED_SCENE = 1, CLWH_DERIVED_CAMERA = 2, CLWH_DERIVED_PROJECTION = 4 };
int clwh_ctx_invalidate_derived(clwh_ctx *ctx, int what);
/* which copy of the derived scene data the context renders from (after its last clwh_render): a process-wide unique id
 * of the content (0: none yet), its size in bytes, and how many contexts hold it right now */
int clwh_ctx_scene_info(clwh_ctx *ctx, uint64_t *scene_id, uint64_t *bytes, int32_t *holders);

/* ---- intensity projections: a view of the caller's S16 image without a transfer function (not in the reference).
 * For pixel (x, y) of the launched region the ray is the camera ray of clwh_render (generate_ray with the frame IMAGE's dims as totals):
 * origin o = cam_pos, normalised direction d.  Sample k >= 0 sits at t_k = (float)k * step, p_k = o + d * t_k (per component one float
 * multiply, then one float add), and is KEPT iff t_near <= t_k <= t_far and 0 <= p_k.c < dim_c on all three axes (NaN never; -0.0
 * counts as 0).  Its value is the voxel V[floor(p.z)][floor(p.y)][floor(p.x)] (x fastest).
 *   CLWH_PROJ_MAX   value = the largest kept value; t_extreme = t_k of the smallest k that attains it
 *   CLWH_PROJ_MIN   the same with the smallest kept value
 *   CLWH_PROJ_MEAN  value = (float)((double)sum / (double)count) with an int64 sum; t_extreme = NaN
 * A pixel without a kept sample has value = t_extreme = NaN and frame pixel (0, 0, 0, 0).  Otherwise, in float32 and in this order,
 * u = ((value - window_center) / window_width + 0.5f) * 255.0f + 0.5f, grey = (int)fminf(fmaxf(u, 0), 255), and the frame pixel is
 * (grey, grey, grey, 255).  CLWH_PROJ_DENSE reads every kept sample; without it MAX / MIN step over 8^3 bricks whose {min, max} cannot
 * change the result: same bytes, by the contract.
 * Errors: a NULL or wrong-kind handle, a bad mode or flags, a step that is not finite and > 0 (or so small that the camera's farthest
 * volume corner lies 2^29 steps away or more), a window that is not finite with window_width > 0, or a slab that is not
 * t_near <= t_far with t_near < +inf: CLWH_ERR_INVALID_VALUE.  A region that is empty, not a multiple of 8, larger than the frame or
 * than 65535: CLWH_ERR_BAD_NDRANGE.  An optional output smaller than 4 * width * height bytes: CLWH_ERR_SIZE_MISMATCH.
 * Asynchronous and ordered on the context's stream like clwh_render.  The first projection of a volume content builds the derived
 * data (CLWH_DERIVED_PROJECTION); a push, clwh_mem_mark_dirty or a rewrite through any clwh_mem of the same pointer rebuilds it. */
enum clwh_projection { CLWH_PROJ_MAX = 0, CLWH_PROJ_MIN = 1, CLWH_PROJ_MEAN = 2 };
enum clwh_projection_flags { CLWH_PROJ_DENSE = 1 };  /* no brick skipping: same result by contract; for tests and timing */
typedef struct clwh_projection_desc {
  clwh_mem *frame;            /* RGBA8 2-D image; its dims are generate_ray's totals (as clwh_render_desc.frame) */
  clwh_mem *volume;           /* S16 3-D image, 1 channel */
  float cam_pos[3], cam_dir[3];
  uint32_t width, height;     /* launched region: multiples of 8, <= frame dims, <= 65535 (same rule as clwh_render) */
  int32_t mode, flags;
  float step;                 /* h > 0, finite */
  float t_near, t_far;        /* slab along the ray; 0 and +INFINITY = whole volume */
  float window_center, window_width;  /* window_width > 0, finite */
  clwh_mem *values;           /* optional float32[height][width]: the projected value */
  clwh_mem *t_extreme;        /* optional float32[height][width] */
} clwh_projection_desc;
int clwh_render_projection(clwh_ctx *ctx, const clwh_projection_desc *desc);

/* ---- direct volume rendering: emission-absorption compositing of a ray's samples through a colour/opacity table, front to back, in
 * one launch (not in the reference).  Camera rays, step, t_near, t_far, the launched region and the meaning of KEPT sample are those
 * of clwh_render_projection, word for word: sample k >= 0 sits at t_k = (float)k * step, p_k = o + d * t_k (per component one float
 * multiply, then one float add), kept iff t_near <= t_k <= t_far and 0 <= p_k.c < dim_c on all three axes; its voxel is
 * v = V[floor(p.z)][floor(p.y)][floor(p.x)].
 * The table `lut` holds float32[lut_len][4] (r, g, b, a) on the device, 16-byte aligned, in at least 16 * lut_len bytes; lut_first is
 * the voxel value of entry 0, and a value's entry is i = min(max((int)v - lut_first, 0), lut_len - 1).  The table's contents are NOT
 * checked (that would need a device round trip); the arithmetic below defines the result for any bit pattern.
 * Per pixel, in float32, without contraction, with C = (0, 0, 0), A = 0, t_first = t_stop = NaN, for the kept samples in increasing k:
 *   1. (r, g, b, a) = lut[i].  If !(a > 0) (so also for NaN) the sample changes nothing; go to the next.
 *   2. With CLWH_COMP_SHADE only: gx = (float)(V(x+1,y,z) - V(x-1,y,z)), likewise gy, gz, the differences taken in int32 with each
 *      neighbour coordinate clamped to [0, dim-1]; l2 = (gx*gx + gy*gy) + gz*gz; if l2 > 0:
 *      c = fabsf((gx*d.x + gy*d.y) + gz*d.z) / sqrtf(l2), s = ambient + (1.0f - ambient) * fminf(c, 1.0f), else s = 1.0f; then
 *      r = r*s, g = g*s, b = b*s (sqrtf and / correctly rounded).  Two-sided headlight shading: the light is the camera ray.
 *   3. w = (1.0f - A) * a; C.c = C.c + w * c_c for r, g, b (one multiply, then one add); A = A + w.
 *   4. If t_first is NaN, t_first = t_k.  If A >= alpha_stop: t_stop = t_k and the ray ends; no later sample is read.
 * Outputs: frame pixel (q(C.r), q(C.g), q(C.b), q(A)) with q(x) = (int)fminf(fmaxf(x * 255.0f + 0.5f, 0.0f), 255.0f), where fmaxf and
 * fminf return the other operand for a NaN (premultiplied colour; a pixel without a contributing sample is (0, 0, 0, 0), as in the
 * projections).  Optional rgba (float32[height][width][4] = C.r, C.g, C.b, A; a NaN is stored as the quiet NaN 0x7FC00000, since
 * IEEE 754 leaves a NaN's sign and payload to the implementation), t_first, t_stop (float32[height][width]), all row-major over the
 * launched region.  Pixels of the frame outside the region are not touched.
 * A sample with !(a > 0) is a no-op by step 1, so without CLWH_COMP_DENSE the kernel steps over an 8^3 brick when no table entry in
 * [clamp(min - lut_first), clamp(max - lut_first)] has a > 0 (clamping is monotone, so every voxel of the brick maps into that
 * range): same bytes, by the contract.  Early termination (step 4) is part of the contract, not an optimisation: CLWH_COMP_DENSE
 * reads every kept sample up to t_stop.  No opacity correction for the step size: the caller scales the table.
 * Errors: a NULL or wrong-kind handle (lut NULL or not 16-byte aligned included), unknown flag bits, lut_len outside [1, 65536],
 * lut_first outside [-65536, 65535], !(alpha_stop > 0) (+inf is allowed: never stop early), ambient outside [0, 1] or NaN when
 * CLWH_COMP_SHADE is set, and every step / slab / camera-distance / volume-dims condition of clwh_render_projection:
 * CLWH_ERR_INVALID_VALUE (a zero-initialised descriptor is rejected: step == 0).  The region conditions of the projections:
 * CLWH_ERR_BAD_NDRANGE.  A lut smaller than 16 * lut_len bytes, rgba smaller than 16 * width * height or t_first / t_stop smaller than
 * 4 * width * height bytes: CLWH_ERR_SIZE_MISMATCH.
 * Asynchronous and ordered on the context's stream; no host wait.  The derived data (CLWH_DERIVED_PROJECTION) is the projections'
 * bricked copy of the volume, shared with them, plus a prefix count of "a > 0" over the table, keyed on the table's device pointer,
 * its shared content version and lut_len: a push, clwh_mem_mark_dirty or a write through another clwh_mem of the same pointer
 * rebuilds it. */
enum clwh_composite_flags {
  CLWH_COMP_DENSE = 1,  /* no brick skipping: same result by contract; for tests and timing */
  CLWH_COMP_SHADE = 2   /* step 2 */
};
typedef struct clwh_composite_desc {
  clwh_mem *frame;            /* RGBA8 2-D image; its dims are generate_ray's totals (as clwh_render_desc.frame) */
  clwh_mem *volume;           /* S16 3-D image, 1 channel */
  float cam_pos[3], cam_dir[3];
  uint32_t width, height;     /* launched region: multiples of 8, <= frame dims, <= 65535 */
  int32_t flags;
  float step;                 /* h > 0, finite */
  float t_near, t_far;        /* slab along the ray; 0 and +INFINITY = whole volume */
  clwh_mem *lut;              /* float32[lut_len][4] */
  int32_t lut_first, lut_len;
  float alpha_stop;           /* > 0; +INFINITY = never stop early */
  float ambient;              /* [0, 1]; read with CLWH_COMP_SHADE only */
  clwh_mem *rgba;             /* optional float32[height][width][4] */
  clwh_mem *t_first;          /* optional float32[height][width] */
  clwh_mem *t_stop;           /* optional float32[height][width] */
} clwh_composite_desc;
int clwh_render_composite(clwh_ctx *ctx, const clwh_composite_desc *desc);

/* ---- isosurface rendering: the first position along each camera ray where the TRILINEAR field of the volume reaches a value, shaded
 * by a two-sided headlight from the interpolated gradient, together with its depth and normal (not in the reference).  Camera rays,
 * step, t_near, t_far, the launched region and the meaning of KEPT sample are those of clwh_render_projection, word for word: sample
 * k >= 0 sits at t_k = (float)k * step, p_k = o + d * t_k (per component one float multiply, then one float add), kept iff
 * t_near <= t_k <= t_far and 0 <= p_k.c < dim_c on all three axes.
 * The field, in fixed point (so that the result does not depend on the order of evaluation and is exact without any float rule): for a
 * position p with 0 <= p.c < dim_c, per axis c
 *   q = p.c - 0.5f (voxel centres sit at integer + 0.5), f = floorf(q), i0 = (int)f, w = min((int)((q - f) * 256.0f), 255)
 * (float32, in this order; w is in [0, 255]); the axis' two corner coordinates are i0 and i0 + 1, each clamped to [0, dim_c - 1], with
 * the weights 256 - w and w.  S(p) = sum over the 8 corners of wx * wy * wz * V(corner), an exact integer: the interpolated value
 * times 2^24, |S| <= 2^39.  The threshold is T = (int64)floor((double)iso * 16777216.0) (exact).  A position is INSIDE iff S(p) >= T,
 * with CLWH_ISO_BELOW iff S(p) <= T.  No float comparison takes part in a hit decision.
 * Per pixel:
 *   1. k_hit = the smallest kept k with p_k inside.  None: the pixel is a MISS.
 *   2. Refinement, only if k_hit is not the ray's first kept sample (then k_hit - 1 is kept and outside): lo = t_{k_hit-1},
 *      hi = t_{k_hit}; `refine` times: m = lo + (hi - lo) * 0.5f, p = o + d * m; if p is inside then hi = m, else lo = m.  Float
 *      multiply and add are monotone, so lo <= m <= hi and every coordinate of p(m) lies between those of the two kept samples p_{k_hit-1}
 *      and p_{k_hit}: p(m) is inside the volume and S(p(m)) is defined.  t_hit = hi (= t_{k_hit} without refinement), p_hit = o + d * t_hit.
 *   3. Normal at p_hit, with p_hit's 8 (clamped) corners and weights: G_c = sum over the corners of wx * wy * wz * (V(corner + e_c) -
 *      V(corner - e_c)), each neighbour coordinate clamped to [0, dim_c - 1] again; an exact integer, |G_c| < 2^41.  g_c = (float)G_c
 *      with ONE rounding to nearest-even (every G_c is exact in binary64: (float)(double)G_c).  l2 = (gx*gx + gy*gy) + gz*gz.  If l2 > 0:
 *      n_c = g_c / sqrtf(l2), c = fabsf((gx*d.x + gy*d.y) + gz*d.z) / sqrtf(l2), s = ambient + (1.0f - ambient) * fminf(c, 1.0f)
 *      (float32, without contraction, sqrtf and / correctly rounded: the compositor's words); otherwise n = (0, 0, 0) and s = 1.0f.
 * Outputs: frame pixel (q(color[0]*s), q(color[1]*s), q(color[2]*s), 255) with clwh_render_composite's q; a miss is (0, 0, 0, 0);
 * pixels of the frame outside the region are not touched.  Optional t_hit (float32[height][width]; NaN for a miss) and normal
 * (float32[height][width][4] = n.x, n.y, n.z, (float)S(p_hit) * 2^-24, the (float) again one rounding of an integer that is exact in
 * binary64; every NaN is stored as 0x7FC00000, and a miss is four of them), row-major over the launched region.
 * CLWH_ISO_DENSE tests every kept sample up to the hit.  Without it the kernel steps over an 8^3 brick unread when the {min, max} of
 * the brick DILATED BY ONE VOXEL (clamped at the volume's faces) proves that no sample in it is inside: dmax * 2^24 < T, with
 * CLWH_ISO_BELOW dmin * 2^24 > T.  Proof: a sample whose voxel floor(p) = v lies in the brick has i0 in {v - 1, v} on every axis, so all
 * its clamped corners lie within one voxel of the brick, inside the dilated box; S is a combination of their values with non-negative
 * integer weights that sum to 2^24, so dmin * 2^24 <= S <= dmax * 2^24.  (A second table holds the same pair per cell of 4^3
 * bricks, the minimum and maximum over the cell's bricks; it bounds every brick of the cell and lets the walk leave a whole cell at
 * once.)  Same bytes as the dense walk, by the contract.
 * Errors: a NULL or wrong-kind handle, unknown flag bits, iso not finite or |iso| > 65536, refine outside [0, 24], ambient outside
 * [0, 1] or NaN, a colour component that is not finite, a camera position that is not finite, and every step / slab / camera-distance /
 * volume-dims condition of clwh_render_projection: CLWH_ERR_INVALID_VALUE (a zero-initialised descriptor is rejected: step == 0).  The
 * region conditions of the projections: CLWH_ERR_BAD_NDRANGE.  t_hit smaller than 4 * width * height bytes or normal smaller than
 * 16 * width * height: CLWH_ERR_SIZE_MISMATCH.
 * Asynchronous and ordered on the context's stream; no host wait.  The derived data (CLWH_DERIVED_PROJECTION) is the projections'
 * bricked copy of the volume, shared with them, plus the dilated {min, max} tables (4 bytes per brick and per cell of 4^3 bricks),
 * built by the first isosurface call of a volume content -- or by the first clwh_render_slice call that may skip, whichever comes
 * first -- and keyed like the copy: projections and composites never build them. */
enum clwh_isosurface_flags {
  CLWH_ISO_DENSE = 1,  /* no brick skipping: same result by contract; for tests and timing */
  CLWH_ISO_BELOW = 2   /* inside iff S <= T */
};
typedef struct clwh_isosurface_desc {
  clwh_mem *frame;            /* RGBA8 2-D image; its dims are generate_ray's totals (as clwh_render_desc.frame) */
  clwh_mem *volume;           /* S16 3-D image, 1 channel */
  float cam_pos[3], cam_dir[3];
  uint32_t width, height;     /* launched region: multiples of 8, <= frame dims, <= 65535 */
  int32_t flags;
  float step;                 /* h > 0, finite */
  float t_near, t_far;        /* slab along the ray; 0 and +INFINITY = whole volume */
  float iso;                  /* finite, |iso| <= 65536 */
  int32_t refine;             /* bisection steps between the last outside and the first inside sample, 0..24 */
  float color[3];             /* finite */
  float ambient;              /* [0, 1] */
  clwh_mem *t_hit;            /* optional float32[height][width] */
  clwh_mem *normal;           /* optional float32[height][width][4] */
} clwh_isosurface_desc;
int clwh_render_isosurface(clwh_ctx *ctx, const clwh_isosurface_desc *desc);

/* ---- oblique slices and thick slabs (multi-planar reformatting): the TRILINEAR field of the volume on a plane given in voxel
 * space, or its maximum / minimum / mean over `slab_samples` planes stacked along `normal` (not in the reference).  No camera: every
 * pixel owns a ray of its own, and all rays are parallel.
 * Rays.  For pixel (x, y) of the launched region, in float32 without contraction, per component c:
 *   o.c = (origin.c + (float)x * du.c) + (float)y * dv.c
 * Sample k, 0 <= k < slab_samples, sits at t_k = (float)k * step, p_k = o + normal * t_k (per component one float multiply, then one
 * float add), and is KEPT iff 0 <= p_k.c < dim_c on all three axes (NaN never; -0.0 counts as 0): the sample rule of
 * clwh_render_projection with a per-pixel origin, t_near = 0 and no t_far.  Float multiply and add are monotone in k, so the kept
 * samples of a ray -- and those inside any 8^3 brick -- are one contiguous range of k.
 * Value of a sample: S(p_k), the fixed-point trilinear field of clwh_render_isosurface, word for word: per axis q = p.c - 0.5f,
 * f = floorf(q), i0 = (int)f, w = min((int)((q - f) * 256.0f), 255); corners i0 and i0 + 1, each clamped to [0, dim_c - 1], with the
 * weights 256 - w and w; S = sum over the 8 corners of wx * wy * wz * V(corner), an exact integer, the interpolated value times 2^24,
 * |S| <= 2^39.
 * Per pixel:
 *   CLWH_SLICE_MAX   best = the largest kept S, k_ext = the smallest k that attains it.  value = (float)best * 2^-24, where (float)best
 *                    is ONE rounding to nearest-even of an integer that is exact in binary64 ((float)(double)best) and the scaling
 *                    by 2^-24 is exact.  t_extreme = (float)k_ext * step.
 *   CLWH_SLICE_MIN   the same with the smallest kept S
 *   CLWH_SLICE_MEAN  sum = the int64 sum of the kept S, count their number: value = (float)((double)sum / ((double)count *
 *                    16777216.0)); t_extreme = NaN.  |sum| <= 8192 * 2^39 = 2^52 is exact in binary64: hence slab_samples <= 8192.
 * A pixel without a kept sample has value = t_extreme = NaN and frame pixel (0, 0, 0, 0).  Every other pixel is windowed exactly as
 * the projections are: u = ((value - window_center) / window_width + 0.5f) * 255.0f + 0.5f, grey = (int)fminf(fmaxf(u, 0), 255),
 * frame pixel (grey, grey, grey, 255).  Pixels of the frame outside the region are not touched.  Optional values and t_extreme
 * (float32[height][width], row-major over the launched region); every NaN is stored as 0x7FC00000.
 * With slab_samples = 1 the result is the thin slice: value = (float)S(o) * 2^-24 in every mode, t_extreme = 0 (NaN for MEAN).
 * Skipping.  CLWH_SLICE_DENSE reads every kept sample.  Without it MAX may step over an 8^3 brick unread once a `best` exists and
 * dmax * 2^24 <= best, where dmax is the maximum of the brick DILATED BY ONE VOXEL (clamped at the volume's faces; the table of
 * clwh_render_isosurface); MIN likewise when dmin * 2^24 >= best.  Proof: a sample whose voxel floor(p) = v lies in the brick has i0 in
 * {v - 1, v} on every axis, so all its clamped corners lie within one voxel of the brick, inside the dilated box; S is a combination of
 * their values with non-negative integer weights that sum to 2^24, so dmin * 2^24 <= S <= dmax * 2^24.  Every sample of a skipped brick
 * therefore has S <= best (MAX) or S >= best (MIN); the samples are taken in increasing k, so such a sample comes after the one that
 * set `best`, and a sample that merely equals `best` changes neither `best` nor k_ext.  The pair of a cell of 4^3 bricks (minimum and
 * maximum over the cell's bricks) bounds every brick of the cell and may be used in the same way.  Same bytes as the dense walk, by the
 * contract.  MEAN reads every kept sample: the flag is accepted and changes nothing.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx or desc, a NULL or wrong-kind frame or volume; an unknown
 * mode or unknown flag bits; slab_samples outside [1, 8192]; a step that is not finite and > 0 (a zero-initialised descriptor is
 * rejected this way); a window that is not finite with window_width > 0; a component of origin, du, dv or normal that is not finite;
 * on any axis c, |origin.c| + (width - 1) * |du.c| + (height - 1) * |dv.c| + (slab_samples - 1) * step * |normal.c| >= 2^30, evaluated
 * in double (this keeps every coordinate finite and every float -> int conversion defined); volume dims beyond the projections' rule.
 * CLWH_ERR_BAD_NDRANGE: the region rules of the projections (empty, not a multiple of 8, larger than the frame or than 65535).
 * CLWH_ERR_SIZE_MISMATCH: values or t_extreme smaller than 4 * width * height bytes.
 * Asynchronous and ordered on the context's stream; no host wait.  The derived data (CLWH_DERIVED_PROJECTION) is the projections'
 * bricked copy of the volume, shared with them.  The dilated {min, max} tables are built by the first slice call that may skip (MAX or
 * MIN without CLWH_SLICE_DENSE) or by the first isosurface call of a volume content, whichever comes first, and are keyed like the
 * copy: a push, clwh_mem_mark_dirty or clwh_ctx_invalidate_derived rebuilds them. */
enum clwh_slice_mode { CLWH_SLICE_MAX = 0, CLWH_SLICE_MIN = 1, CLWH_SLICE_MEAN = 2 };
enum clwh_slice_flags { CLWH_SLICE_DENSE = 1 };  /* no brick skipping: same result by contract; for tests and timing */
typedef struct clwh_slice_desc {
  clwh_mem *frame;            /* RGBA8 2-D image */
  clwh_mem *volume;           /* S16 3-D image, 1 channel */
  float origin[3];            /* voxel-space position of pixel (0, 0), sample 0 */
  float du[3], dv[3];         /* voxel-space offset per pixel in x and in y */
  float normal[3];            /* slab direction; need not be unit; (0, 0, 0) allowed */
  uint32_t width, height;     /* launched region: multiples of 8, <= frame dims, <= 65535 */
  int32_t mode, flags;
  int32_t slab_samples;       /* 1 .. 8192; 1 = a thin slice */
  float step;                 /* > 0, finite */
  float window_center, window_width;  /* window_width > 0, finite */
  clwh_mem *values;           /* optional float32[height][width] */
  clwh_mem *t_extreme;        /* optional float32[height][width] */
} clwh_slice_desc;
int clwh_render_slice(clwh_ctx *ctx, const clwh_slice_desc *desc);

/* ---- the straightened curved planar reformat (CPR): the slice with a frame of its own per image row (not in the reference).  Image
 * row y is a line across a vessel at station y of a curve: `rows` holds, per row of the launched region, nine floats origin[3], du[3],
 * normal[3] in voxel space (scene.curve_frames / renderer::curve_frames make them from a centreline).
 * Rays.  For pixel (x, y) of the launched region, in float32 without contraction, per component c:
 *   o.c = origin_y.c + (float)x * du_y.c
 * (one multiply, then one add).  Sample k, 0 <= k < slab_samples, sits at p_k = o + normal_y * ((float)k * step).
 * From there on the text of clwh_render_slice applies word for word: the kept rule, S(p) and the three modes (CLWH_SLICE_MAX / MIN /
 * MEAN), the one rounding to float32, t_extreme, every NaN stored as 0x7FC00000, the pixel (0, 0, 0, 0) where no sample is kept, the
 * window, the pixels of the frame outside the region left untouched, and the skip rule with the dilated brick table and the table of
 * the cells of 4^3 bricks -- its proof is per ray and nowhere uses that the rays are parallel.  So
 *   pixel (x, y) of the curved view == pixel (x, 0) of clwh_render_slice with origin = origin_y, du = du_y, normal = normal_y,
 * byte for byte, in the frame, in values and in t_extreme (dv does not matter in a slice's row 0: (float)0 * dv adds +-0).
 * A row with origin outside the volume and du = normal = 0 keeps no sample: a transparent row (the padding rows of curve_frames).
 * Errors, in the slice's order of kinds.  CLWH_ERR_INVALID_VALUE: the slice's cases (ctx, desc, frame, volume, mode, flags,
 * slab_samples, step, window, volume dims); rows == NULL; a component of a row that is not finite; on any axis c of any row,
 * |origin.c| + (width - 1) * |du.c| + (slab_samples - 1) * step * |normal.c| >= 2^30, evaluated in double.  `rows` is read for `height`
 * rows before the region is checked, so it holds that many whenever it is not NULL.  CLWH_ERR_BAD_NDRANGE and CLWH_ERR_SIZE_MISMATCH
 * as in the slice.  Nothing is written on an error.
 * Asynchronous and ordered on the context's stream; no host wait.  The rows are validated on the host and copied through a page-locked
 * buffer of the context into a device buffer of the context, so the caller's array need not outlive the call; the next call that
 * stages rows (this one or clwh_curve_profile) waits for that copy's event only, and the device buffer is reused in stream order.
 * Derived data: the projections' bricked copy and the slice's dilated tables, built and invalidated exactly as for the slice. */
enum clwh_curved_flags { CLWH_CURVED_DENSE = 1 };  /* no brick skipping: same result by contract */
typedef struct clwh_curved_desc {
  clwh_mem *frame;            /* RGBA8 2-D image */
  clwh_mem *volume;           /* S16 3-D image, 1 channel */
  const float *rows;          /* HOST, float32[height][9]: per image row origin[3], du[3], normal[3], voxel space */
  uint32_t width, height;     /* launched region, the slice's rules */
  int32_t mode, flags;        /* CLWH_SLICE_MAX / MIN / MEAN; CLWH_CURVED_DENSE */
  int32_t slab_samples;       /* 1 .. 8192 */
  float step;                 /* > 0, finite */
  float window_center, window_width;
  clwh_mem *values, *t_extreme;   /* optional float32[height][width] */
} clwh_curved_desc;
int clwh_render_curved(clwh_ctx *ctx, const clwh_curved_desc *desc);

/* ---- the section profile of a mask along a curve: per station the cross-section of the mask in the plane the station's row spans,
 * as an exact integer record (not in the reference).  Integers and sets only.
 * Station y, 0 <= y < n_rows, has a grid of width x slab_samples samples p(x, k) = (origin_y + (float)x * du_y) + normal_y * ((float)k *
 * step), positioned as in clwh_render_curved.  A sample is SET iff it is kept (the slice's rule against `dims`) and bit ((int)p.x,
 * (int)p.y, (int)p.z) of the mask is set; the mask is in clwh_segment_grow's layout, and its padding bits are never read, whatever
 * they hold.  Without CLWH_PROFILE_CONNECTED the section is all set samples.  With it the section is the union of the 4-connected
 * components of set samples -- neighbours are (x +- 1, k) and (x, k +- 1) -- that contain a CENTRE sample: one of the up to four samples
 * {(width - 1) / 2, width / 2} x {(slab_samples - 1) / 2, slab_samples / 2} (integer division) that is set.  No centre sample set: the
 * section is empty.
 * Record: count = the size of the section; sum_x, sum_k = the sums of x and of k over it (at most 64 * 64 * 63); border = the number of
 * its samples with x in {0, width - 1} or k in {0, slab_samples - 1}: nonzero says the window cut the lumen.
 * Asynchronous and ordered on the context's stream; the rows are staged as in clwh_render_curved.
 * Errors.  CLWH_ERR_INVALID_VALUE: a NULL ctx or desc; a NULL, wrong-kind or misaligned mask (8 bytes) or records buffer (16 bytes);
 * rows == NULL; unknown flag bits; n_rows outside [1, 65535], width or slab_samples outside [1, 64]; a step that is not finite and > 0;
 * dims beyond clwh_segment_grow's limits; rows that are not finite or reach 2^30, as in clwh_render_curved.  CLWH_ERR_SIZE_MISMATCH: a
 * mask smaller than grow's size for `dims`, records smaller than 16 * n_rows bytes.  Nothing is written on an error. */
enum clwh_profile_flags { CLWH_PROFILE_CONNECTED = 1 };
typedef struct clwh_section_record { uint32_t count, sum_x, sum_k, border; } clwh_section_record;  /* 16 bytes */
typedef struct clwh_curve_profile_desc {
  clwh_mem *mask;             /* plain device buffer, grow's layout */
  uint32_t dims[3];           /* X, Y, Z of the mask */
  const float *rows;          /* HOST, float32[n_rows][9], as above */
  uint32_t n_rows;            /* 1 .. 65535, any number */
  uint32_t width;             /* 1 .. 64 samples across (x) */
  int32_t  slab_samples;      /* 1 .. 64 samples along normal (k) */
  float step;
  int32_t flags;
  clwh_mem *records;          /* plain device buffer, clwh_section_record[n_rows] */
} clwh_curve_profile_desc;
int clwh_curve_profile(clwh_ctx *ctx, const clwh_curve_profile_desc *desc);

/* ---- the isosurface as an indexed triangle mesh, by marching tetrahedra (not in the reference): the first output that is geometry, not
 * pixels.  Every decision is an integer comparison, so the result is defined bit for bit.
 * Grid.  Grid point P = (x, y, z), 0 <= P.c < dim_c, carries A(P) = (int64)V[z][y][x] << 24 and sits at the voxel's centre P + 0.5: the
 * voxel space of clwh_render_slice and of the trilinear field S, whose value at a voxel centre is exactly A(P).
 * T = (int64)floor((double)iso * 16777216.0), as for clwh_render_isosurface.  P is INSIDE iff A(P) >= T, with CLWH_MESH_BELOW iff
 * A(P) <= T.
 * Box.  The cells meshed are those with origin c, lo_k <= c.k < hi_k; box_lo / box_hi are given in grid points,
 * 0 <= lo_k <= hi_k <= dim_k - 1.  box_hi all zero means the whole volume, hi_k = dim_k - 1.  An axis with lo_k == hi_k gives the empty
 * mesh (0 vertices, 0 triangles, CLWH_OK).
 * Tetrahedra.  The corners of a cell are numbered by the mask m = dx | dy << 1 | dz << 2.  Every cell is cut into the six tetrahedra of
 * the Kuhn triangulation, one per permutation (a, b, c) of the axis bits {1, 2, 4}, in lexicographic order of (a, b); each has the
 * corners 0, a, a|b, 7 in this order.  All share the body diagonal, and the cut is the same in every cell, so neighbouring cells agree on
 * the diagonal of their common face.  Every edge of a tetrahedron runs from a grid point P to Q = P + d with d in {0,1}^3 \ {0}: seven
 * kinds of edge, dir = d.x | d.y << 1 | d.z << 2 in 1..7.
 * Vertices.  One per edge (P, dir) such that P and Q both lie in [lo, hi] on every axis (inclusive) and exactly one of P, Q is inside
 * (hence A(P) != A(Q)):
 *   key = ((P.z * Y + P.y) * X + P.x) * 8 + dir, a uint64
 *   w = (|T - A(P)| << 16) / |A(Q) - A(P)|, an int64 floor division, in [0, 65536]; always taken from the lower end P, so every
 *     tetrahedron and cell that shares the edge gets the same vertex
 *   position, per axis: F_c = P.c * 65536 + 32768 + (Q.c - P.c) * w as an integer, pos_c = (float)F_c * 2^-16: the conversion is ONE
 *     rounding to nearest-even, the scaling is exact
 *   normal: g_c(R) = V(R + e_c) - V(R - e_c) in int32, each neighbour coordinate clamped to [0, dim_c - 1] (the isosurface's central
 *     differences); G_c = (65536 - w) * g_c(P) + w * g_c(Q), an exact int64, |G_c| < 2^34; g_c = (float)G_c, one rounding;
 *     l2 = (gx*gx + gy*gy) + gz*gz; if l2 > 0: n_c = (-g_c) / sqrtf(l2), with CLWH_MESH_BELOW n_c = g_c / sqrtf(l2) (float32, without
 *     contraction, sqrtf and / correctly rounded: the compositor's words), so that the normal points to the outside; otherwise
 *     n = (0, 0, 0).
 * Triangles.  Let a tetrahedron's corners be at positions 0..3 in the order above.  0 or 4 of them inside: no triangle.  One inside a,
 * outside b < c < d: one triangle over the edges (a,b), (a,c), (a,d).  Three inside a < b < c, outside d: one triangle over (a,d),
 * (b,d), (c,d).  Two inside a < b, outside c < d: the quad (a,c), (a,d), (b,d), (b,c), split along (a,c)-(b,d) into q0 q1 q2 and
 * q0 q2 q3.  The winding is decided from the grid, never from vertex positions (which may coincide): with each vertex replaced by the
 * midpoint of its edge, m0, m1, m2, the triangle is emitted in the order for which ((m1 - m0) x (m2 - m0)) . (centroid of the outside
 * corners - centroid of the inside corners) > 0, otherwise with its last two vertices swapped: counter-clockwise seen from the
 * outside.  (The sign depends only on the tetrahedron and its 4-bit case.)  A triangle is three uint32 indices into the vertex array.
 * Triangles with coinciding positions are kept (w = 0 or 65536: a grid value equal to iso).
 * Order.  The order of vertices and of triangles is unspecified but deterministic: two calls with the same inputs give the same bytes,
 * and no order depends on the scheduling of the device.  Every vertex is referenced by at least one triangle.  The surface is left open
 * where it meets the box: no caps.
 * Buffers.  positions and normals (float32[capacity][3]), keys (uint64[capacity]) and triangles (uint32[capacity][3]) are plain device
 * buffers (clwh_mem_create, clwh_mem_wrap), all optional; positions and triangles come together, and normals and keys only with them.
 * The call always stores the true counts in *n_vertices and *n_triangles.  With every buffer NULL and both capacities 0 it only counts.
 * If a count exceeds its capacity, or 2^32 - 1, the call returns CLWH_ERR_SIZE_MISMATCH with the counts set and writes nothing to the
 * buffers: the caller allocates and calls again.
 * SYNCHRONOUS, unlike the views: the call is ordered on the context's stream, but it waits for the device -- once for the counts, once
 * more after filling -- and returns with the buffers written.  It is not a per-frame call.
 * Skipping.  Without CLWH_MESH_DENSE a brick of 8^3 grid points is visited only if its pair {dmin, dmax} over the brick DILATED BY ONE
 * VOXEL (the table of clwh_render_isosurface) allows a crossing: dmin * 2^24 < T <= dmax * 2^24, with CLWH_MESH_BELOW
 * dmin * 2^24 <= T < dmax * 2^24.  Proof: every edge owned by a grid point of the brick, and every corner of a cell whose origin lies in
 * the brick, is within one voxel of the brick; a crossing needs one end inside and one end outside, that is a value on either side of
 * T in the dilated box.  Same bytes as CLWH_MESH_DENSE, order included: the dense walk visits every brick and finds nothing in the others.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc, n_vertices or n_triangles; a NULL or wrong-kind
 * volume; unknown flag bits; iso not finite or |iso| > 65536; a box that breaks the rule above; a buffer that is an image; triangles
 * without positions or the reverse; normals or keys without positions; a capacity > 0 whose buffer (positions, triangles) is NULL;
 * volume dims beyond the projections' rule.  CLWH_ERR_SIZE_MISMATCH: a buffer smaller than its capacity times its element size (12,
 * 12, 8, 12 bytes), and the capacity rule above.  CLWH_ERR_OUT_OF_MEMORY: scratch that cannot be allocated.
 * The derived data (CLWH_DERIVED_PROJECTION) is the projections' bricked copy of the volume and, without CLWH_MESH_DENSE, the dilated
 * {min, max} tables, keyed and invalidated exactly as for clwh_render_isosurface.  The mesher's scratch (48 bytes per brick, and 2 KiB
 * per brick that has a vertex while a filling call runs) is kept with them and holds nothing between calls. */
enum clwh_mesh_flags {
  CLWH_MESH_DENSE = 1,  /* no brick skipping: same result by contract; for tests and timing */
  CLWH_MESH_BELOW = 2   /* inside iff A <= T */
};
typedef struct clwh_mesh_desc {
  clwh_mem *volume;           /* S16 3-D image, 1 channel */
  float iso;                  /* finite, |iso| <= 65536 */
  int32_t flags;
  uint32_t box_lo[3], box_hi[3];  /* grid points; box_hi all zero = the whole volume */
  clwh_mem *positions;        /* optional float32[vertex_capacity][3] */
  clwh_mem *normals;          /* optional float32[vertex_capacity][3] */
  clwh_mem *keys;             /* optional uint64[vertex_capacity] */
  clwh_mem *triangles;        /* optional uint32[triangle_capacity][3] */
  uint64_t vertex_capacity, triangle_capacity;
  uint64_t *n_vertices, *n_triangles;  /* host; required */
} clwh_mesh_desc;
int clwh_mesh_isosurface(clwh_ctx *ctx, const clwh_mesh_desc *desc);

/* ---- seeded region growing: the connected set of voxels inside a value window that hangs together with the seeds, as one bit per
 * voxel, with its statistics (not in the reference): the first operation that says "this structure, not that one".  Every decision is
 * an integer comparison and the result is a set, so it is defined bit for bit and does not depend on how the device schedules anything.
 * The volume is V[z][y][x], an S16 3-D image with one channel and dims X, Y, Z.
 * Admissible.  Voxel p is admissible iff lo <= V(p) <= hi (-32768 <= lo <= hi <= 32767) and box_lo.c <= p.c < box_hi.c on every axis.
 * The box is given in voxels, box_lo.c <= box_hi.c <= dim_c; box_hi all zero means the whole volume; an empty box gives the empty set
 * and CLWH_OK.
 * Neighbours.  Two voxels are neighbours iff they differ by 1 in exactly one coordinate (6-connectivity); with CLWH_GROW_26 iff they
 * differ by at most 1 in every coordinate and are not equal.  No clamping, no wrap-around: the border has no neighbours outside.
 * Seeds.  `seeds` is a HOST pointer to uint32[n_seeds][3] = (x, y, z), n_seeds <= 65536, duplicates allowed.  A seed that is not
 * admissible contributes nothing.  With CLWH_GROW_FROM_MASK every bit set in `mask` on entry whose voxel is admissible is a seed as
 * well (n_seeds may then be 0): growing in two steps with different windows, or continuing after an edit.  Without the flag the
 * contents of `mask` on entry are ignored.
 * Result.  R is the smallest set that contains the admissible seeds and, with each of its voxels, that voxel's admissible neighbours.
 * On return `mask` holds exactly R.
 * Mask layout.  One bit per voxel, rows x-fastest, in 32-bit words: words_per_row = 2 * ((X + 63) / 64) (even: a row is a run of
 * aligned 64-bit pairs); voxel (x, y, z) is bit x & 31 of word (z * Y + y) * words_per_row + (x >> 5).  Bits at x >= X and the padding
 * words are zero on return, whatever the buffer held on entry without CLWH_GROW_FROM_MASK.  `mask` is a plain device buffer
 * (clwh_mem_create, clwh_mem_wrap) whose device pointer is 8-byte aligned, of at least 4 * words_per_row * Y * Z bytes.
 * Statistics.  *result (HOST, required), all exact integers: count; bbox_lo / bbox_hi, the smallest box holding R, hi exclusive (all
 * zero when count == 0); sum of V over R; sum_sq of V * V over R; vmin / vmax over R (0 when count == 0); rounds, the number of rounds
 * the iteration took: informational, may differ between calls, not part of the contract.
 * SYNCHRONOUS, like clwh_mesh_isosurface: ordered on the context's stream, waits for the device, returns with mask and *result
 * written.  The number of launches depends on the data (a vessel tree has a geodesic depth in the thousands).  CLWH_GROW_DENSE
 * visits every tile of 64 x 16 x 16 voxels in every round instead of the worklist of tiles a neighbour's change woke: same bytes, by
 * the contract.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or result; a NULL or wrong-kind volume; a NULL
 * mask, a mask that is an image or whose device pointer is not 8-byte aligned; unknown flag bits; a window or a box that breaks the
 * rules above; n_seeds > 65536, n_seeds > 0 with NULL seeds, n_seeds == 0 without CLWH_GROW_FROM_MASK; a seed outside the volume;
 * volume dims beyond the projections' rule.  CLWH_ERR_SIZE_MISMATCH: a mask smaller than the layout needs.  CLWH_ERR_OUT_OF_MEMORY:
 * scratch that cannot be allocated.  Nothing is written to `mask` or *result on any of these.  (CLWH_ERR_INTERNAL_OVERFLOW: the iteration
 * passed its hard cap of X * Y * Z + 2 rounds, which no input can cause; the mask then holds a subset of R.)
 * The caller's volume image is read directly: no derived data is built or invalidated.  The scratch (one bit per voxel, four bytes per
 * tile, the copied seeds) is kept with the context and holds nothing between calls. */
enum clwh_grow_flags {
  CLWH_GROW_26 = 1,         /* 26-connectivity instead of 6 */
  CLWH_GROW_FROM_MASK = 2,  /* the admissible bits of `mask` on entry are seeds too */
  CLWH_GROW_DENSE = 4       /* every tile in every round: same result by contract; for tests and timing */
};
#define CLWH_GROW_MAX_SEEDS 65536
typedef struct clwh_grow_result {
  uint64_t count;
  uint32_t bbox_lo[3], bbox_hi[3];
  int64_t sum;
  uint64_t sum_sq;
  int32_t vmin, vmax;
  uint32_t rounds;
  uint32_t reserved;
} clwh_grow_result;
typedef struct clwh_grow_desc {
  clwh_mem *volume;           /* S16 3-D image, 1 channel */
  clwh_mem *mask;             /* plain device buffer in the mask layout */
  int32_t lo, hi;             /* the value window, both ends included */
  int32_t flags;
  uint32_t n_seeds;
  const uint32_t *seeds;      /* host; uint32[n_seeds][3] = x, y, z */
  uint32_t box_lo[3], box_hi[3];  /* voxels; box_hi all zero = the whole volume */
  clwh_grow_result *result;   /* host; required */
} clwh_grow_desc;
int clwh_segment_grow(clwh_ctx *ctx, const clwh_grow_desc *desc);

/* ---- a mask applied to a volume (not in the reference): out(p) = (bit(p) != invert) ? in(p) : fill for every voxel, with bit(p) read in
 * clwh_segment_grow's mask layout and invert = the flag CLWH_MASK_INVERT.  "Keep" with fill = -32768 followed by clwh_mesh_isosurface
 * or clwh_render_isosurface at the window's lower bound shows or meshes only the grown structure; CLWH_MASK_INVERT with the value of
 * air removes it.  volume_out may be volume_in, or another handle to the same pointer: the in-place case.
 * Asynchronous and ordered on the context's stream, like the views.  It counts as a rewrite of volume_out: the content version that
 * clwh_mem_push and clwh_mem_mark_dirty bump is bumped, so every derived data set keyed on that pointer (the bricked copy, the dilated
 * tables, the packed scene) rebuilds at its next use, in this context and in contexts that share the pointer.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx or desc; a NULL or wrong-kind volume_in or volume_out; a
 * NULL mask, a mask that is an image or whose device pointer is not 8-byte aligned; unknown flag bits; fill outside [-32768, 32767];
 * volume dims beyond the projections' rule.  CLWH_ERR_SIZE_MISMATCH: volumes of different dims; a mask smaller than the layout needs. */
enum clwh_apply_mask_flags { CLWH_MASK_INVERT = 1 };
typedef struct clwh_apply_mask_desc {
  clwh_mem *volume_in;        /* S16 3-D image, 1 channel */
  clwh_mem *volume_out;       /* the same dims; may name volume_in's memory */
  clwh_mem *mask;             /* plain device buffer in the mask layout */
  int32_t fill;               /* -32768 .. 32767 */
  int32_t flags;
} clwh_apply_mask_desc;
int clwh_volume_apply_mask(clwh_ctx *ctx, const clwh_apply_mask_desc *desc);

/* ---- volume filters (not in the reference): "denoise, then segment".  The median (the speckle remover that keeps edges), grey erosion
 * and dilation by a box, and a separable smoothing whose integer weights the caller derives from millimetres (scene.gaussian_weights),
 * over the int16 volume and into a volume, so every view, the mesher, the path tracer and every segmentation call read the result
 * unchanged.  Integers only: defined bit for bit.  The reference's bilateral_filter (clwh_launch) is a different filter and unchanged.
 * Neighbourhood and border.  V = volume_in (dims X, Y, Z); N(p) = the box of offsets |dx| <= rx, |dy| <= ry, |dz| <= rz, radius =
 * (rx, ry, rz).  Every tap is read at the coordinate CLAMPED to the volume per axis, V(clamp(x + dx, 0, X - 1), ...): the edge is
 * replicated.  (The reference's zero border would pull a -1000 HU air border towards 0.)
 * CLWH_FILTER_MEDIAN.  Every radius 0 or 1: n = 1, 3, 9 or 27 taps; (1, 1, 0) is the in-plane median for thick slices.  F(p) = element
 * (n - 1) / 2 of the sorted multiset of the n clamped taps; duplicates from clamping count as often as they occur.
 * CLWH_FILTER_MIN / CLWH_FILTER_MAX.  Every radius 0 .. CLWH_FILTER_MAX_RADIUS.  F(p) = the minimum / maximum over the clamped taps.
 * CLWH_FILTER_SMOOTH.  Every radius 0 .. CLWH_FILTER_MAX_RADIUS.  weights[c][k] (HOST, uint16[radius[c] + 1], copied before the call
 * returns) is the weight of the taps +-k along axis c, and weights[c][0] + 2 * sum over k >= 1 of weights[c][k] ==
 * CLWH_FILTER_WEIGHT_SUM exactly, per axis.  Three passes in the order x, y, z, each rounded to int16 on its own:
 *   T(p) = (sum over k of w[|k|] * S(clamp(p + k e_c)) + 2048) >> 12,
 * the sum in 32-bit signed arithmetic (|sum| <= 2^27), the shift arithmetic (floor).  T stays within the line's extremes (no clamp),
 * constant volumes pass through unchanged, and an axis of radius 0 (weights {4096}) is the identity.  The order of the passes and the
 * rounding per pass are part of the contract: another order or one rounding at the end give other bytes.
 * Output.  out(p) = F(p) where mask is NULL or its bit at p is set (clwh_segment_grow's mask layout, read only, padding ignored whatever
 * it holds); elsewhere out(p) = V(p).  F always reads the unfiltered V, also next to clear bits.  volume_out may be volume_in, or another
 * handle to the same pointer: the result is as if all of V had been read before anything was written.
 * Asynchronous and ordered on the context's stream, like clwh_volume_apply_mask, and a rewrite of volume_out in exactly its sense: the
 * same version bump.  Axes of radius 0 launch nothing; all radii 0 is a copy.  Scratch (at most two int16 copies of the volume) is kept
 * with the context and holds nothing between calls.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx or desc; a NULL or wrong-kind volume_in or volume_out; a
 * mask that is given and is an image or whose device pointer is not 8-byte aligned; an unknown kind; flags != 0; a radius above the
 * kind's limit; SMOOTH with a NULL weights[c] or a sum other than 4096 (weights of other kinds are ignored); volume dims beyond the
 * projections' rule.  CLWH_ERR_SIZE_MISMATCH: volumes of different dims; a mask smaller than the layout needs.
 * CLWH_ERR_OUT_OF_MEMORY: scratch that cannot be allocated.  Nothing is written and no version is bumped on any of these. */
enum clwh_filter_kind { CLWH_FILTER_MEDIAN = 0, CLWH_FILTER_MIN = 1, CLWH_FILTER_MAX = 2, CLWH_FILTER_SMOOTH = 3 };
#define CLWH_FILTER_MAX_RADIUS 16
#define CLWH_FILTER_WEIGHT_SUM 4096
typedef struct clwh_filter_desc {
  clwh_mem *volume_in;        /* S16 3-D image, 1 channel */
  clwh_mem *volume_out;       /* the same dims; may name volume_in's memory */
  clwh_mem *mask;             /* optional; grow's mask layout; read only */
  int32_t kind;               /* clwh_filter_kind */
  int32_t flags;              /* 0 */
  uint32_t radius[3];         /* rx, ry, rz in voxels */
  const uint16_t *weights[3]; /* host; SMOOTH only: weights[c] = uint16[radius[c] + 1], tap 0 first */
} clwh_filter_desc;
int clwh_volume_filter(clwh_ctx *ctx, const clwh_filter_desc *desc);

/* ---- connected-component labelling (not in the reference): ALL components of a value window at once, ranked largest first, where
 * clwh_segment_grow gives the one under the seeds.  "How many pieces", "keep the largest", "drop the specks below N voxels" are then a
 * table lookup and a rank interval.  Integers and sets only: defined bit for bit, independent of how the device schedules anything.
 * Admissible, neighbours.  Exactly clwh_segment_grow's: lo <= V(p) <= hi, inside the box (hi exclusive, box_hi all zero = the whole
 * volume, an empty box = nothing admissible and CLWH_OK); 6-connectivity, with CLWH_LABEL_26 26-connectivity.  With
 * CLWH_LABEL_FROM_MASK `mask` (grow's mask layout; read only, never written) is required and a voxel is admissible only if its bit
 * is set as well: a grown or edited mask split into its parts.  Without the flag `mask` is ignored.
 * Components and their order.  The components are the classes of the admissible voxels under the transitive closure of "neighbour".
 * A component's `first` voxel is its member with the smallest flat index (z * Y + y) * X + x.  Components are ranked 1, 2, ... by
 * descending voxel count, ties by ascending flat index of `first`: rank 1 is the largest, and "at least N voxels" is a prefix.
 * Outputs.  `labels`: a plain device buffer, 4-byte aligned, of at least 4 * X * Y * Z bytes, uint32 [z][y][x] without padding; on
 * return 0 for a voxel that is not admissible and the component's rank otherwise; every one of the X * Y * Z words is written.
 * `components` (optional) with component_capacity: a plain device buffer, 8-byte aligned, of clwh_label_component records (48 bytes);
 * records 0 .. min(n, capacity) - 1 are written, record k for rank k + 1 (bbox_hi exclusive, reserved = 0); records from n on are not
 * touched; a capacity below n is no error ("the 16 largest").  *result (HOST, required): n_components, n_voxels (the admissible
 * total); passes, the number of kernels launched: informational, not part of the contract.
 * Limits.  X * Y * Z <= 2^31 - 1: ranks and flat indices then fit 31 bits and a word of `labels` has a spare bit, which the call uses
 * while it runs (labels doubles as the union-find's memory: there is no second word per voxel).
 * SYNCHRONOUS, like clwh_segment_grow: ordered on the context's stream, returns with everything written.  The volume is read
 * directly; no derived data is built or invalidated.  The scratch is kept with the context and holds nothing between calls: one bit
 * per voxel, and 16 bytes per component plus the sort's work space (about as much again).
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or result; a NULL or wrong-kind volume; NULL
 * labels, labels that are an image or whose device pointer is not 4-byte aligned; components that are an image or not 8-byte aligned,
 * or NULL components with component_capacity > 0; CLWH_LABEL_FROM_MASK with a mask that breaks grow's rules (NULL, an image, not
 * 8-byte aligned); unknown flag bits; a window or a box that breaks grow's rules; volume dims beyond the projections' rule or
 * X * Y * Z > 2^31 - 1.  CLWH_ERR_SIZE_MISMATCH: labels smaller than 4 * X * Y * Z bytes, components smaller than 48 * capacity
 * bytes, a mask smaller than its layout.  CLWH_ERR_OUT_OF_MEMORY: scratch that cannot be allocated.  Nothing is written to labels,
 * components or *result on any of these. */
enum clwh_label_flags {
  CLWH_LABEL_26 = 1,        /* 26-connectivity instead of 6 */
  CLWH_LABEL_FROM_MASK = 2  /* admissible only where the bit of `mask` is set as well */
};
typedef struct clwh_label_component {
  uint64_t count;
  uint32_t first[3];                  /* x, y, z of the member with the smallest flat index */
  uint32_t bbox_lo[3], bbox_hi[3];    /* hi exclusive */
  uint32_t reserved;                  /* 0 */
} clwh_label_component;
typedef struct clwh_label_result {
  uint64_t n_components;
  uint64_t n_voxels;
  uint32_t passes;
  uint32_t reserved;
} clwh_label_result;
typedef struct clwh_label_desc {
  clwh_mem *volume;           /* S16 3-D image, 1 channel */
  clwh_mem *labels;           /* plain device buffer, uint32[Z][Y][X] */
  clwh_mem *components;       /* optional plain device buffer of clwh_label_component[component_capacity] */
  uint64_t component_capacity;
  clwh_mem *mask;             /* CLWH_LABEL_FROM_MASK: plain device buffer in the mask layout; read only */
  int32_t lo, hi;             /* the value window, both ends included */
  int32_t flags;
  uint32_t box_lo[3], box_hi[3];  /* voxels; box_hi all zero = the whole volume */
  clwh_label_result *result;  /* host; required */
} clwh_label_desc;
int clwh_segment_label(clwh_ctx *ctx, const clwh_label_desc *desc);

/* ---- a selection of components as a mask: bit(p) = (rank_lo <= labels(p) <= rank_hi), 1 <= rank_lo <= rank_hi, in
 * clwh_segment_grow's mask layout for dims = X, Y, Z, with the bits at x >= X and the padding words zero whatever the buffer held.
 * `labels` is what clwh_segment_label wrote (uint32 [z][y][x], a plain device buffer, 4-byte aligned).  The mask is what
 * clwh_volume_apply_mask and CLWH_GROW_FROM_MASK read.  Asynchronous and ordered on the context's stream, like clwh_volume_apply_mask.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx or desc; NULL labels, labels that are an image or not
 * 4-byte aligned; a NULL mask, a mask that is an image or not 8-byte aligned; a dim of 0, dims beyond the projections' rule or
 * X * Y * Z > 2^31 - 1; rank_lo == 0 or rank_lo > rank_hi.  CLWH_ERR_SIZE_MISMATCH: labels smaller than 4 * X * Y * Z bytes, a mask
 * smaller than the layout needs. */
typedef struct clwh_labels_to_mask_desc {
  clwh_mem *labels;
  clwh_mem *mask;
  uint32_t dims[3];           /* X, Y, Z of the labelled volume */
  uint32_t rank_lo, rank_hi;  /* both ends included */
} clwh_labels_to_mask_desc;
int clwh_labels_to_mask(clwh_ctx *ctx, const clwh_labels_to_mask_desc *desc);

/* ---- the exact squared distance map of a mask (not in the reference): "how far is every voxel from this structure", "how deep inside
 * it am I".  The squared Euclidean distance between voxel centres with an integer weight per axis is an integer, so the map, every
 * threshold of it and the morphology below are defined bit for bit.
 * Sites.  S = the voxels of the volume (dims = X, Y, Z) whose bit in `mask` (clwh_segment_grow's mask layout; read only) is set; with
 * CLWH_DIST_TO_CLEAR the voxels of the volume whose bit is clear.  Voxels outside the volume do not exist: they are neither set nor
 * clear.  Bits at x >= X and the padding words of `mask` are ignored, whatever they hold.
 * Distance.  D(p) = min over q in S of wx (p.x - q.x)^2 + wy (p.y - q.y)^2 + wz (p.z - q.z)^2; CLWH_DIST_NONE if S is empty.
 * Weights.  wx, wy, wz >= 1 and wx (X - 1)^2 + wy (Y - 1)^2 + wz (Z - 1)^2 <= 2^32 - 2 (computed in 64 bits): every finite D fits a
 * uint32 and never equals CLWH_DIST_NONE.  (49, 49, 625) are voxels of 0.7 x 0.7 x 2.5 mm in units of 0.01 mm^2; (1, 1, 1) is voxels.
 * Output.  `dist`: a plain device buffer, 4-byte aligned, uint32 [Z][Y][X] without padding; dist(p) = D(p) if D(p) <= cap, else
 * CLWH_DIST_NONE (cap = CLWH_DIST_NONE: no cap).  All X * Y * Z words are written and nothing behind them.  A cap lets the kernels look
 * no farther than sqrt(cap / w) along an axis: same bytes, by the contract.
 * Limits.  Those of clwh_labels_to_mask: no dim of 0, dims within the projections' rule, X * Y * Z <= 2^31 - 1.
 * Asynchronous and ordered on the context's stream, like clwh_volume_apply_mask; no host result, no derived data.  Scratch: two maps of
 * 4 * X * Y * Z bytes each, 1 GiB together at 512^3 (a pass along an axis reads one buffer and writes another, so that a line of any
 * length takes the same path, and keeps a stack of as many words), kept with the context like grow's; it holds nothing between calls.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx or desc; a mask that breaks grow's rules (NULL, an image,
 * not 8-byte aligned); a NULL dist, a dist that is an image or not 4-byte aligned; unknown flag bits; dims that break the limits; a
 * weight of 0 or weights beyond the bound.  CLWH_ERR_SIZE_MISMATCH: a mask smaller than its layout, dist smaller than 4 * X * Y * Z
 * bytes.  CLWH_ERR_OUT_OF_MEMORY: scratch that cannot be allocated.  Nothing is written on any of these. */
#define CLWH_DIST_NONE 0xFFFFFFFFu
enum clwh_distance_flags { CLWH_DIST_TO_CLEAR = 1 };
typedef struct clwh_distance_desc {
  clwh_mem *mask;             /* plain device buffer in the mask layout; read only */
  clwh_mem *dist;             /* plain device buffer, uint32[Z][Y][X] */
  uint32_t dims[3];           /* X, Y, Z */
  uint32_t weight[3];         /* wx, wy, wz >= 1 */
  uint32_t cap;               /* CLWH_DIST_NONE = no cap */
  int32_t flags;
} clwh_distance_desc;
int clwh_mask_distance(clwh_ctx *ctx, const clwh_distance_desc *desc);

/* ---- dilation, erosion, opening and closing of a mask by a ball (not in the reference): "this lesion plus 5 mm", "peel one
 * millimetre off", "close the pinholes", "break the thin bridge".  The ball is { d : wx d.x^2 + wy d.y^2 + wz d.z^2 <= radius_sq }:
 * anisotropic through the weights, in their unit.  With D_set and D_clear clwh_mask_distance's maps of M = mask_in without and with
 * CLWH_DIST_TO_CLEAR, and CLWH_DIST_NONE counting as farther than any radius_sq (0xFFFFFFFF included):
 * DILATE(M) = { p : D_set(p) <= radius_sq };  ERODE(M) = { p in M : D_clear(p) > radius_sq };  OPEN = DILATE(ERODE(M));
 * CLOSE = ERODE(DILATE(M)), both steps with the same ball.
 * The volume's border does not erode: voxels outside the volume are not clear (they do not exist), so a structure that the scan box
 * cuts through keeps its cut face, a full mask erodes to itself, and CLOSE has no artefacts along the border.
 * Output.  On return mask_out holds exactly that set, the bits at x >= X and the padding words zero whatever the buffers held;
 * radius_sq = 0 therefore copies M with clean padding.  mask_out may name mask_in's memory.  Any radius_sq is allowed.
 * Asynchronous and ordered on the context's stream; limits and the weights' rule as for clwh_mask_distance.  The comparison is made
 * in the last pass of the distance transform (every pass capped at radius_sq), so no finished map is written.  Scratch, kept with the
 * context: two intermediate maps of 4 bytes per voxel each (1 GiB together at 512^3) and, for OPEN and CLOSE, one mask.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx or desc; mask_in or mask_out that breaks grow's rules;
 * an op outside 0 .. 3; flags != 0; dims that break the limits; a weight of 0 or weights beyond the bound.  CLWH_ERR_SIZE_MISMATCH: a
 * mask smaller than its layout.  CLWH_ERR_OUT_OF_MEMORY: scratch that cannot be allocated.  Nothing is written on any of these. */
enum clwh_morph_op { CLWH_MORPH_DILATE = 0, CLWH_MORPH_ERODE = 1, CLWH_MORPH_OPEN = 2, CLWH_MORPH_CLOSE = 3 };
typedef struct clwh_morph_desc {
  clwh_mem *mask_in;          /* plain device buffer in the mask layout */
  clwh_mem *mask_out;         /* the same layout; may name mask_in's memory */
  uint32_t dims[3];           /* X, Y, Z */
  uint32_t weight[3];         /* wx, wy, wz >= 1 */
  uint32_t radius_sq;         /* in the weights' unit; any value */
  int32_t op;                 /* clwh_morph_op */
  int32_t flags;              /* 0 */
} clwh_morph_desc;
int clwh_mask_morph(clwh_ctx *ctx, const clwh_morph_desc *desc);

/* ---- mask algebra on the device (not in the reference): out = a AND b, a OR b, a XOR b, a AND NOT b, or NOT a, for masks of dims =
 * X, Y, Z in clwh_segment_grow's layout.  CLWH_MASK_NOT ignores b, which may then be NULL; the complement is taken within the volume.
 * Bits at x >= X and the padding words of a and b are ignored and those of out are zero on return.  out may name a's or b's memory.
 * One kernel; asynchronous and ordered on the context's stream.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx or desc; a, out or (except for CLWH_MASK_NOT) b that
 * breaks grow's rules for a mask (NULL, an image, not 8-byte aligned); an op outside 0 .. 4; a dim of 0, dims beyond the projections'
 * rule or X * Y * Z > 2^31 - 1.  CLWH_ERR_SIZE_MISMATCH: a mask smaller than the layout needs.  Nothing is written on any of these. */
enum clwh_mask_op { CLWH_MASK_AND = 0, CLWH_MASK_OR = 1, CLWH_MASK_XOR = 2, CLWH_MASK_ANDNOT = 3, CLWH_MASK_NOT = 4 };
typedef struct clwh_mask_combine_desc {
  clwh_mem *a;
  clwh_mem *b;                /* ignored by CLWH_MASK_NOT, may then be NULL */
  clwh_mem *out;              /* may name a's or b's memory */
  uint32_t dims[3];           /* X, Y, Z */
  int32_t op;                 /* clwh_mask_op */
} clwh_mask_combine_desc;
int clwh_mask_combine(clwh_ctx *ctx, const clwh_mask_combine_desc *desc);

/* ---- topology-preserving thinning of a mask (not in the reference): the skeleton of a structure -- "the whole vessel tree, every
 * branch and fork", "is this a ring or a blob" -- where clwh_mask_morph erodes without regard to topology and clwh_cost_trace needs
 * both ends named.  The mask is peeled layer by layer, and no voxel is deleted whose removal would change the number of parts,
 * cavities or tunnels.  Integers and sets only: defined bit for bit, independent of how the device schedules anything.
 * Conventions.  M = the voxels of the volume (dims = X, Y, Z) whose bit in mask_in (clwh_segment_grow's mask layout) is set; bits at
 * x >= X and the padding words are ignored on entry and zero on return.  Object voxels are 26-connected, background voxels
 * 6-connected.  EVERYTHING OUTSIDE THE VOLUME IS BACKGROUND -- unlike clwh_mask_morph, whose border does not erode: a structure that
 * the scan box cuts through is peeled from its cut face too.
 * Simple.  Take the 26 neighbours of p as a set N (outside = clear).  p is simple iff (a) N is not empty and is one 26-connected
 * component, adjacency taken inside the 3 x 3 x 3 block without its centre, and (b) among the CLEAR positions of the 18-neighbourhood
 * (offsets with |dx| + |dy| + |dz| <= 2) at least one is a face neighbour, and all clear face neighbours lie in one component under
 * 6-adjacency within that 18-neighbourhood.
 * Iteration i = 1, 2, ...  On M as it stands at the start of the iteration: B = the voxels of M with a clear or outside face
 * neighbour; E = the voxels of M with exactly one set 26-neighbour (with CLWH_THIN_KEEP_ENDS; otherwise empty); C = B \ E \ anchors.
 * Then eight sub-passes s = 0 .. 7 in this order, s = (x & 1) | (y & 1) << 1 | (z & 1) << 2: every voxel of C with parity s that is
 * still set and is simple in the current M is deleted, all of them at once (two voxels of one parity are never 26-neighbours, so no
 * order inside a sub-pass matters).  The call stops after the first iteration that deletes nothing, or after max_iterations
 * (0 = no limit).
 * Result (HOST, required), all exact and functions of the input alone: count_in = |M| on entry, count_out on return, deleted =
 * count_in - count_out, iterations = the number of iterations run, the final empty one included.
 * Buffers.  mask_out may name mask_in's memory; otherwise mask_in is read only.  `anchors` (optional, the same layout, read only) names
 * voxels that are never deleted; its bits outside M mean nothing.  It must not overlap mask_out unless mask_out is mask_in.
 * SYNCHRONOUS, like clwh_segment_grow: ordered on the context's stream, returns with mask_out and *result written.  Per iteration one
 * kernel finds C and lists the tiles of 64 x 16 x 16 voxels that hold a candidate, and one kernel per sub-pass works the listed tiles;
 * the host reads the counters every four iterations.  CLWH_THIN_DENSE visits every tile: same bytes, by the contract.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or result; mask_in, mask_out or (when given) anchors
 * that breaks grow's rules for a mask (NULL, an image, not 8-byte aligned); unknown flag bits; a dim of 0, dims beyond the projections'
 * rule or X * Y * Z > 2^31 - 1.  CLWH_ERR_SIZE_MISMATCH: a mask smaller than the layout needs.  CLWH_ERR_OUT_OF_MEMORY: scratch that
 * cannot be allocated.  Nothing is written on any of these.  (CLWH_ERR_INTERNAL_OVERFLOW: the loop passed its hard cap of
 * count_in + 1 iterations, which no input can cause: every iteration but the last deletes a voxel.)
 * The scratch (one bit per voxel for C, eight bytes per tile, the counters) is kept with the context and holds nothing between calls. */
enum clwh_thin_flags {
  CLWH_THIN_KEEP_ENDS = 1,  /* curve skeleton: a voxel with exactly one set 26-neighbour at the start of an iteration stays */
  CLWH_THIN_DENSE = 2       /* every tile in every sub-pass: same result by contract; for tests and timing */
};
typedef struct clwh_thin_result {
  uint64_t count_in, count_out, deleted;
  uint32_t iterations;
  uint32_t reserved;
} clwh_thin_result;
typedef struct clwh_thin_desc {
  clwh_mem *mask_in;          /* plain device buffer in the mask layout */
  clwh_mem *mask_out;         /* the same layout; may name mask_in's memory */
  clwh_mem *anchors;          /* optional, the same layout; read only */
  uint32_t dims[3];           /* X, Y, Z */
  int32_t flags;              /* clwh_thin_flags */
  uint32_t max_iterations;    /* 0 = until nothing is deleted */
  uint32_t reserved;          /* 0 */
  clwh_thin_result *result;   /* host; required */
} clwh_thin_desc;
int clwh_mask_thin(clwh_ctx *ctx, const clwh_thin_desc *desc);

/* ---- the set voxels of a mask as a list (not in the reference): what turns a thin mask into something the host can walk.  The voxels
 * of the volume (dims = X, Y, Z) whose bit in `mask` (grow's layout; read only; bits at x >= X and padding words ignored) is set, in
 * ascending flat index (z * Y + y) * X + x.  Point k is uint32[4] = x, y, z, n26 in `points`, n26 = the number of set 26-neighbours
 * (outside the volume = clear); with `map` (uint32 [Z][Y][X], for instance clwh_mask_distance's depth) values[k] = map at that voxel.
 * Counting and filling follow clwh_mesh_isosurface: *n_points (HOST, required) always receives the true count; with points NULL and
 * capacity 0 the call only counts; a count above `capacity` returns CLWH_ERR_SIZE_MISMATCH with the count set and writes nothing to
 * the buffers.  No atomics: per-word counts, rocprim::exclusive_scan, one lane per word -- the order is fixed.  SYNCHRONOUS.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or n_points; a mask that breaks grow's rules;
 * points, map or values that is an image or not 4-byte aligned; map without values or values without map; values without points; a
 * capacity > 0 with NULL points; flags != 0; dims as for clwh_mask_thin.  CLWH_ERR_SIZE_MISMATCH: a mask smaller than its layout, a map
 * smaller than 4 * X * Y * Z bytes, points smaller than 16 * capacity or values smaller than 4 * capacity bytes; the capacity rule
 * above.  CLWH_ERR_OUT_OF_MEMORY: scratch that cannot be allocated (eight bytes per 64-bit word of the mask, kept with the context). */
typedef struct clwh_mask_points_desc {
  clwh_mem *mask;             /* plain device buffer in the mask layout; read only */
  clwh_mem *points;           /* optional uint32[capacity][4] = x, y, z, n26 */
  clwh_mem *map;              /* optional uint32[Z][Y][X] to sample; read only */
  clwh_mem *values;           /* uint32[capacity]; with map only */
  uint32_t dims[3];           /* X, Y, Z */
  int32_t flags;              /* 0 */
  uint64_t capacity;
  uint64_t *n_points;         /* host; required */
} clwh_mask_points_desc;
int clwh_mask_points(clwh_ctx *ctx, const clwh_mask_points_desc *desc);

/* ---- geodesic distance maps and nearest-seed territories inside a mask (not in the reference): shortest paths THROUGH a mask from a set
 * of labelled seeds, giving every voxel a distance and the id of its nearest seed.  "These two bones touch: give me each one" is erode,
 * label, and this call with the pieces as seeds; "how far along this vessel" is this call with one seed.  Integers and sets only:
 * defined bit for bit, independent of how the device schedules anything.
 * Domain.  dims = X, Y, Z.  D = the voxels of the volume whose bit in `domain` (clwh_segment_grow's mask layout; read only) is set.
 * Bits at x >= X and the padding words are ignored, whatever they hold.
 * Steps and costs.  Neighbours are clwh_segment_grow's: 6, or 26 with CLWH_GEO_26; no clamping, no wrap-around.  A step that changes
 * one coordinate costs weight_face[axis]; with CLWH_GEO_26 a step that changes two costs weight_edge[k], k the axis that does NOT
 * change (0: y and z change, 1: x and z, 2: x and y), and a step that changes all three costs weight_corner.  Every weight in use is
 * an integer in 1 .. 65535; edge and corner weights are ignored without CLWH_GEO_26.  No triangle inequality is demanded.  A path is
 * a sequence of voxels of D, each a neighbour of the one before; its length is the sum of its steps' costs.
 * Seeds.  `seeds` is a HOST pointer to uint32[n_seeds][4] = (x, y, z, id), n_seeds <= CLWH_GROW_MAX_SEEDS, id >= 1; duplicates and
 * several ids on one voxel are allowed; a seed outside D contributes nothing.  With CLWH_GEO_FROM_LABELS every voxel of D whose word
 * in `seed_labels` (uint32 [Z][Y][X], a plain device buffer, 4-byte aligned) is nonzero is a seed with that word as its id as well;
 * n_seeds may then be 0.  Without the flag n_seeds == 0 is an error and seed_labels is ignored.
 * Result.  For p in D: dist(p) = the smallest length of a path from any seed to p (a seed's own voxel: 0); label(p) = the smallest id
 * among the seeds that attain it.  cap <= 0xFFFF0000 limits the distance (CLWH_DIST_NONE means 0xFFFF0000; any other value above
 * 0xFFFF0000 is an error): with weights <= 65535 no sum then overflows 32 bits, and a voxel whose distance exceeds the cap counts as
 * not reached.  Voxels not in D, and voxels of D that no seed reaches within the cap, get dist = CLWH_DIST_NONE and label = 0.
 * Outputs.  `dist` and `labels`: plain device buffers, 4-byte aligned, uint32 [Z][Y][X] without padding; all X * Y * Z words are
 * written and nothing behind them.  Either may be NULL, not both.  `labels` may name seed_labels' memory (in place).  *result (HOST,
 * required): reached, the number of voxels with a finite distance; max_dist, the largest of them (0 when nothing is reached); rounds:
 * informational, may differ between calls, not part of the contract.
 * CLWH_GEO_DENSE visits every tile of 16 x 16 x 8 voxels in every round instead of the worklist: same bytes, by the contract.
 * Limits.  Those of clwh_labels_to_mask: no dim of 0, dims within the projections' rule, X * Y * Z <= 2^31 - 1.
 * SYNCHRONOUS, like clwh_segment_grow (the host reads the round counters): ordered on the context's stream, returns with everything
 * written.  No derived data is built or invalidated.  Scratch, kept with the context, holds nothing between calls: the packed 64-bit
 * keys, 8 * X * Y * Z bytes (1 GiB at 512^3, what clwh_mask_distance keeps), 8 bytes per tile, and the copied seeds.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or result; a domain that breaks grow's rules for
 * a mask (NULL, an image, not 8-byte aligned); dist and labels both NULL, one of them an image or not 4-byte aligned;
 * CLWH_GEO_FROM_LABELS with a NULL, image or misaligned seed_labels; unknown flag bits; dims that break the limits; a weight in use
 * of 0 or above 65535; a cap above 0xFFFF0000 other than CLWH_DIST_NONE; n_seeds > CLWH_GROW_MAX_SEEDS, n_seeds > 0 with NULL
 * seeds, n_seeds == 0 without CLWH_GEO_FROM_LABELS; a seed outside the volume or with id 0.  CLWH_ERR_SIZE_MISMATCH: a domain smaller
 * than its layout; dist, labels or (with the flag) seed_labels smaller than 4 * X * Y * Z bytes.  CLWH_ERR_OUT_OF_MEMORY: scratch that
 * cannot be allocated.  Nothing is written on any of these.  (CLWH_ERR_INTERNAL_OVERFLOW: the iteration passed its hard cap of
 * X * Y * Z + 2 rounds, which no input can cause: a shortest path crosses fewer tile faces than it has voxels.) */
enum clwh_geodesic_flags {
  CLWH_GEO_26 = 1,           /* 26-connectivity instead of 6 */
  CLWH_GEO_FROM_LABELS = 2,  /* the nonzero words of seed_labels inside D are seeds too */
  CLWH_GEO_DENSE = 4         /* every tile in every round: same result by contract; for tests and timing */
};
#define CLWH_GEO_CAP_MAX 0xFFFF0000u
typedef struct clwh_geodesic_result {
  uint64_t reached;
  uint32_t max_dist;
  uint32_t rounds;
} clwh_geodesic_result;
typedef struct clwh_geodesic_desc {
  clwh_mem *domain;           /* plain device buffer in the mask layout; read only */
  clwh_mem *seed_labels;      /* CLWH_GEO_FROM_LABELS: plain device buffer, uint32[Z][Y][X] */
  clwh_mem *dist;             /* optional plain device buffer, uint32[Z][Y][X] */
  clwh_mem *labels;           /* optional, the same; may name seed_labels' memory */
  uint32_t dims[3];           /* X, Y, Z */
  uint32_t weight_face[3];    /* the step along x, y, z */
  uint32_t weight_edge[3];    /* CLWH_GEO_26: the step that leaves x, y, z unchanged */
  uint32_t weight_corner;     /* CLWH_GEO_26 */
  uint32_t cap;               /* CLWH_DIST_NONE = 0xFFFF0000 */
  int32_t flags;
  uint32_t n_seeds;
  const uint32_t *seeds;      /* host; uint32[n_seeds][4] = x, y, z, id */
  clwh_geodesic_result *result;  /* host; required */
} clwh_geodesic_desc;
int clwh_mask_geodesic(clwh_ctx *ctx, const clwh_geodesic_desc *desc);

/* ---- the path behind a geodesic distance: from `target` back to a seed along a shortest path.  `dist` is a map written by
 * clwh_mask_geodesic, `labels` (optional) the labelling written with it; dims, weights and CLWH_GEO_26 as in that call.
 * Definition.  The path starts at the target.  From p with dist(p) > 0 the next point is p + dir for the first direction that
 * qualifies, the directions running in the order (dz, dy, dx) ascending with dx fastest and those that are not neighbours under the
 * connectivity skipped: p + dir lies inside the volume, dist(p + dir) != CLWH_DIST_NONE, dist(p + dir) + w(dir) == dist(p), and, if
 * labels is given, labels(p + dir) == labels(p).  Such a direction always exists for a map of clwh_mask_geodesic.  The path ends at the
 * first point with dist == 0.
 * Output.  `points`: a plain device buffer, 4-byte aligned, uint32[capacity][3] = (x, y, z), target first; *n_points (HOST, required)
 * is the true count and min(n_points, capacity) points are written; points may be NULL when capacity is 0.  A target with
 * dist == CLWH_DIST_NONE gives n_points = 0 and CLWH_OK.  SYNCHRONOUS; one wave walks the path.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or n_points; a NULL dist, a dist that is an image
 * or not 4-byte aligned; labels or points that are an image or misaligned, NULL points with capacity > 0; flag bits other than
 * CLWH_GEO_26; dims that break clwh_mask_geodesic's limits; a weight in use of 0 or above 65535; a target outside the volume.
 * CLWH_ERR_SIZE_MISMATCH: dist or labels smaller than 4 * X * Y * Z bytes, points smaller than 12 * capacity bytes.  Nothing is
 * written on any of these.  A map that is not clwh_mask_geodesic's, where no direction qualifies at a point with dist > 0, ends the
 * path there: the points up to it and *n_points are written and the call returns CLWH_ERR_INVALID_VALUE.  It never loops: every step
 * strictly lowers dist. */
typedef struct clwh_geodesic_trace_desc {
  clwh_mem *dist;             /* plain device buffer, uint32[Z][Y][X] */
  clwh_mem *labels;           /* optional, the same */
  clwh_mem *points;           /* plain device buffer, uint32[capacity][3] */
  uint64_t capacity;
  uint32_t dims[3];           /* X, Y, Z */
  uint32_t weight_face[3];
  uint32_t weight_edge[3];
  uint32_t weight_corner;
  int32_t flags;              /* CLWH_GEO_26 or 0 */
  uint32_t target[3];         /* x, y, z */
  uint64_t *n_points;         /* host; required */
} clwh_geodesic_trace_desc;
int clwh_geodesic_trace(clwh_ctx *ctx, const clwh_geodesic_trace_desc *desc);

/* ---- geodesic distance maps through a cost field (not in the reference): clwh_mask_geodesic with a step cost that depends on the voxel,
 * not only on the direction.  A shortest path through a tube hugs the inner wall of every bend; with a cost that is low in the middle
 * of the structure and high at its wall (clwh_cost_from_field over clwh_mask_distance's depth map) the path is the centreline, the
 * curve to measure a vessel's length along.  With a cost from the gradient, territories meet on the image's edges while the paths on
 * both sides are of similar length (the cost is a SUM; clwh_watershed divides by the edges alone); with a cost from
 * the value and no domain, a path follows a bright vessel that nobody has segmented.  Integers and sets only: defined bit for bit,
 * independent of how the device schedules anything.
 * Cost.  `cost`: a plain device buffer, 2-byte aligned, uint16 [Z][Y][X] without padding, at least 2 * X * Y * Z bytes; read only.
 * Domain.  D = { p : cost(p) >= 1 and (domain == NULL or p's bit in `domain` is set) }: a cost of 0 is a wall.  `domain` is optional
 * (NULL = the whole volume), in clwh_segment_grow's mask layout, read only; bits at x >= X and the padding words are ignored.
 * Steps.  Neighbours, directions and the flags CLWH_GEO_26, CLWH_GEO_FROM_LABELS and CLWH_GEO_DENSE are clwh_mask_geodesic's.  The step
 * from q to its neighbour p costs mult(direction) * cost(p): the direction's multiplier (mult_face[axis], mult_edge[k], mult_corner,
 * indexed like that call's weights) times the cost of the voxel ENTERED.  Every multiplier in use is an integer in 1 .. 255; edge and
 * corner multipliers are ignored without CLWH_GEO_26.  A step costs at most 255 * 65535 < 2^24.  The length is not symmetric: a
 * path pays for every voxel but its first, its reverse for every voxel but its last.
 * Seeds, result, outputs, limits, scratch: exactly clwh_mask_geodesic's (seeds on the HOST as (x, y, z, id), id >= 1, at most
 * CLWH_GROW_MAX_SEEDS; a seed outside D contributes nothing; dist(p) = the smallest length of a path from any seed to p, 0 at a seed's
 * own voxel whatever its cost; label(p) = the smallest id among the seeds that attain it; CLWH_DIST_NONE and 0 outside D and where no
 * seed reaches within the cap; either output may be NULL, not both; labels may name seed_labels' memory; all X * Y * Z words of an
 * output are written and nothing behind them; *result as there).  SYNCHRONOUS.
 * The cap.  cap <= CLWH_COST_CAP_MAX = 0xFF000000 (CLWH_DIST_NONE means that maximum; any other value above it is an error): with
 * steps below 2^24 no sum of real operands wraps 32 bits, and a voxel whose distance exceeds the cap counts as not reached.  LARGE
 * COSTS OVER LONG PATHS CAN EXCEED THE CAP: a path of more than 256 steps of 255 * 65535 passes it.  Scaling the cost so that the longest
 * path of interest stays below 0xFF000000 is the caller's job; result->max_dist and result->reached tell whether it did.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or result; a cost that is NULL, an image or not
 * 2-byte aligned; a domain that is given and breaks grow's rules for a mask (an image, not 8-byte aligned); dist and labels both NULL,
 * one of them an image or not 4-byte aligned; CLWH_GEO_FROM_LABELS with a NULL, image or misaligned seed_labels; unknown flag bits;
 * dims that break the limits; a multiplier in use of 0 or above 255; a cap above 0xFF000000 other than CLWH_DIST_NONE; n_seeds >
 * CLWH_GROW_MAX_SEEDS, n_seeds > 0 with NULL seeds, n_seeds == 0 without CLWH_GEO_FROM_LABELS; a seed outside the volume or with id 0.
 * CLWH_ERR_SIZE_MISMATCH: a cost smaller than 2 * X * Y * Z bytes; a domain smaller than its layout; dist, labels or (with the flag)
 * seed_labels smaller than 4 * X * Y * Z bytes.  CLWH_ERR_OUT_OF_MEMORY: scratch that cannot be allocated.  Nothing is written on any
 * of these.  (CLWH_ERR_INTERNAL_OVERFLOW: the iteration passed its hard cap of X * Y * Z + 2 rounds, which no input can cause: every
 * step cost is positive, so a shortest path visits no voxel twice and crosses fewer tile faces than it has voxels.) */
#define CLWH_COST_CAP_MAX 0xFF000000u
typedef struct clwh_cost_geodesic_desc {
  clwh_mem *cost;             /* plain device buffer, uint16[Z][Y][X]; read only; 0 = wall */
  clwh_mem *domain;           /* optional plain device buffer in the mask layout; read only */
  clwh_mem *seed_labels;      /* CLWH_GEO_FROM_LABELS: plain device buffer, uint32[Z][Y][X] */
  clwh_mem *dist;             /* optional plain device buffer, uint32[Z][Y][X] */
  clwh_mem *labels;           /* optional, the same; may name seed_labels' memory */
  uint32_t dims[3];           /* X, Y, Z */
  uint32_t mult_face[3];      /* the step along x, y, z: 1 .. 255 */
  uint32_t mult_edge[3];      /* CLWH_GEO_26: the step that leaves x, y, z unchanged */
  uint32_t mult_corner;       /* CLWH_GEO_26 */
  uint32_t cap;               /* CLWH_DIST_NONE = CLWH_COST_CAP_MAX */
  int32_t flags;              /* clwh_geodesic_flags */
  uint32_t n_seeds;
  const uint32_t *seeds;      /* host; uint32[n_seeds][4] = x, y, z, id */
  clwh_geodesic_result *result;  /* host; required */
} clwh_cost_geodesic_desc;
int clwh_cost_geodesic(clwh_ctx *ctx, const clwh_cost_geodesic_desc *desc);

/* ---- the path behind a cost geodesic's distance: clwh_geodesic_trace with the cost field.  `dist` is a map written by
 * clwh_cost_geodesic, `labels` (optional) the labelling written with it; cost, dims, multipliers and CLWH_GEO_26 as in that call.
 * Definition.  The path starts at the target.  From p with dist(p) > 0 the next point is p + dir for the first direction that
 * qualifies, in clwh_geodesic_trace's order ((dz, dy, dx) ascending with dx fastest, non-neighbours skipped): p + dir lies inside the
 * volume, dist(p + dir) != CLWH_DIST_NONE, dist(p + dir) + mult(dir) * cost(p) == dist(p) -- cost(p) is the cost of the voxel the
 * forward path entered, the current one -- and, if labels is given, labels(p + dir) == labels(p).  Such a direction always exists for
 * a map of clwh_cost_geodesic.  The path ends at the first point with dist == 0.
 * Output, the unreached target (n_points = 0, CLWH_OK) and SYNCHRONOUS as in clwh_geodesic_trace.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or n_points; a NULL cost, a cost that is an image
 * or not 2-byte aligned; a NULL dist, a dist that is an image or not 4-byte aligned; labels or points that are an image or misaligned,
 * NULL points with capacity > 0; flag bits other than CLWH_GEO_26; dims that break clwh_mask_geodesic's limits; a multiplier in use
 * of 0 or above 255; a target outside the volume.  CLWH_ERR_SIZE_MISMATCH: a cost smaller than 2 * X * Y * Z bytes, dist or labels
 * smaller than 4 * X * Y * Z bytes, points smaller than 12 * capacity bytes.  Nothing is written on any of these.  Maps that are not
 * clwh_cost_geodesic's, where at a point with dist > 0 the cost is 0 or no direction qualifies, end the path there: the points up to
 * it and *n_points are written and the call returns CLWH_ERR_INVALID_VALUE.  It never loops: every step strictly lowers dist. */
typedef struct clwh_cost_trace_desc {
  clwh_mem *cost;             /* plain device buffer, uint16[Z][Y][X] */
  clwh_mem *dist;             /* plain device buffer, uint32[Z][Y][X] */
  clwh_mem *labels;           /* optional, the same */
  clwh_mem *points;           /* plain device buffer, uint32[capacity][3] */
  uint64_t capacity;
  uint32_t dims[3];           /* X, Y, Z */
  uint32_t mult_face[3];
  uint32_t mult_edge[3];
  uint32_t mult_corner;
  int32_t flags;              /* CLWH_GEO_26 or 0 */
  uint32_t target[3];         /* x, y, z */
  uint64_t *n_points;         /* host; required */
} clwh_cost_trace_desc;
int clwh_cost_trace(clwh_ctx *ctx, const clwh_cost_trace_desc *desc);

/* ---- a cost field from a table (not in the reference): the one place a cost is made on the device.
 *   cost(p) = table[index(p)], or 0 where `domain` is given and p's bit is clear;
 *   index(p) = clamp((s(p) - lo) >> shift, 0, n - 1), in 64-bit signed arithmetic, the clamp below 0 taken before the shift (s < lo
 *   gives entry 0 whatever lo is).
 * `table` is a HOST pointer to uint16[n], 1 <= n <= 65536, copied before the call returns; lo is any int64; shift <= 40.
 * The sources of s, dims = X, Y, Z:
 *   CLWH_COST_SRC_U32       `source` is a plain device buffer, 4-byte aligned, uint32 [Z][Y][X] (a distance map, any words); s = the
 *                           word, CLWH_DIST_NONE included as the number it is, so it clamps to the last entry unless lo says otherwise;
 *   CLWH_COST_SRC_VALUE     `source` is the volume V (an S16 3-D image with one channel, whose dims must equal `dims`); s = V(p);
 *   CLWH_COST_SRC_GRADIENT  the same image; s = gx^2 + gy^2 + gz^2 with gx = V(min(x + 1, X - 1), y, z) - V(max(x - 1, 0), y, z) and
 *                           likewise gy, gz: unscaled central differences, one-sided at the border; up to 3 * 65535^2.
 * Output.  `cost`: a plain device buffer, 2-byte aligned, uint16 [Z][Y][X]; all X * Y * Z entries are written and nothing behind them.
 * `domain`: optional, clwh_segment_grow's mask layout, read only.  Limits: those of clwh_labels_to_mask.  Asynchronous and ordered on
 * the context's stream, like clwh_mask_distance; one kernel, a lane per voxel; the scratch is the table's copy.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or table; an unknown source kind; a source that is
 * NULL or of the wrong kind for it (for CLWH_COST_SRC_U32 an image or not 4-byte aligned; for the others anything but an S16 3-D
 * image with one channel); a cost that is NULL, an image or not 2-byte aligned; a domain that is given and breaks grow's rules; flags
 * other than 0; n outside 1 .. 65536; shift above 40; dims that break the limits or differ from the image's.
 * CLWH_ERR_SIZE_MISMATCH: a uint32 source smaller than 4 * X * Y * Z bytes, a cost smaller than 2 * X * Y * Z bytes, a domain smaller
 * than its layout.  CLWH_ERR_OUT_OF_MEMORY: scratch that cannot be allocated.  Nothing is written on any of these. */
enum clwh_cost_source { CLWH_COST_SRC_U32 = 0, CLWH_COST_SRC_VALUE = 1, CLWH_COST_SRC_GRADIENT = 2 };
typedef struct clwh_cost_field_desc {
  clwh_mem *source;           /* uint32[Z][Y][X] plain device buffer, or the S16 volume image */
  clwh_mem *domain;           /* optional plain device buffer in the mask layout; read only */
  clwh_mem *cost;             /* plain device buffer, uint16[Z][Y][X] */
  const uint16_t *table;      /* host; uint16[n] */
  int64_t lo;
  uint32_t dims[3];           /* X, Y, Z */
  uint32_t n;                 /* 1 .. 65536 */
  uint32_t shift;             /* 0 .. 40 */
  int32_t kind;               /* clwh_cost_source */
  int32_t flags;              /* 0 */
} clwh_cost_field_desc;
int clwh_cost_from_field(clwh_ctx *ctx, const clwh_cost_field_desc *desc);

/* ---- seeded watershed of a cost field (not in the reference): every seed floods its basin, and two floods meet on the ridge between
 * them, however far either seed lies from it.  clwh_cost_geodesic SUMS the cost along a path, so a seed 3 voxels from a ridge of cost
 * 20 spills over it before a seed 40 voxels away across a basin of cost 1 gets there; the watershed takes the MAXIMUM along the path,
 * the height of the lowest pass, and the border lies on the ridge.  With a cost from the gradient (clwh_cost_from_field,
 * CLWH_COST_SRC_GRADIENT) one click in each organ divides the image along the edges between them.  Integers and sets only: defined
 * bit for bit, in two stages, so that the answer is a function of the input alone.
 * Cost, domain.  `cost` and `domain` are clwh_cost_geodesic's: a plain device buffer, 2-byte aligned, uint16 [Z][Y][X] without padding,
 * read only; an optional mask in clwh_segment_grow's layout, read only, bits at x >= X and the padding words ignored.
 * D = { p : cost(p) >= 1 and (domain == NULL or p's bit in `domain` is set) }: a cost of 0 is a wall.
 * Neighbours, seeds, flags.  clwh_mask_geodesic's: 6 neighbours, or 26 with CLWH_GEO_26; seeds on the HOST as (x, y, z, id), id >= 1,
 * at most CLWH_GROW_MAX_SEEDS, and/or with CLWH_GEO_FROM_LABELS every voxel of D whose word in seed_labels is not 0, with that word as
 * its id; several ids on one voxel are allowed; a seed outside D contributes nothing.  CLWH_GEO_DENSE: same bytes, by the contract.
 * Stage 1, the level.  A state is a pair (M, L), ordered lexicographically.  A path in D from a seed starts with (0, 0) at the seed's
 * own voxel, whatever its cost; stepping into p with c = cost(p) turns (M, L) into (c, 0) if c > M and into (M, min(L + 1,
 * plateau_cap)) otherwise.  ML(p) = the smallest state over all paths in D from any seed to p.  M is the height of the lowest pass from a
 * seed to p; L counts the steps since that height was reached and saturates at plateau_cap (0 .. 65534): it divides a plateau by the
 * distance from where the flood entered it, where without it a flat region would go whole to the smallest id.  plateau_cap = 0 is the
 * pure max-cost watershed.  A voxel whose M would exceed level_cap (0 .. 65535) counts as not reached.  The step is monotone in the
 * state and never lowers it, so the minimum over paths is also the least fixpoint of the relaxation.
 * Stage 2, the label.  Between neighbours q, p in D that are both reached, q -> p is an edge iff the step from ML(q) into p gives
 * exactly ML(p).  label(p) = the smallest id of any seed from whose voxel p can be reached along edges (a seed on s reaches s).  Every
 * reached voxel has such a seed: on a path s = p0 .. pn that attains ML(p), let j be the last index with ML(pj) < ML(p); the step from
 * ML(pj) into pj+1 lies between ML(pj+1) = ML(p) and the path's own state there, which is at most ML(p), so it is an edge, and so is
 * every later step, between voxels whose state is ML(p) already; by induction on the state pj is reached from a seed.  No step gives
 * (0, 0), so no edge enters a seed's voxel: it keeps the smallest of its own ids.  With L saturated the edges can form cycles; the
 * definition does not mind.
 * Outputs.  labels: uint32 [Z][Y][X], 0 outside D and where the voxel is not reached; it may name seed_labels' memory.  level: uint32
 * [Z][Y][X] = M << 16 | L, CLWH_DIST_NONE outside D and where the voxel is not reached (plateau_cap <= 65534 keeps the two apart).
 * Either may be NULL, not both.  All X * Y * Z words of an output are written and nothing behind them.  *result (host, required):
 * reached, the number of voxels with a state; max_level, the largest M among them (0 when nothing is reached); rounds: of both stages
 * together, informational, not part of the contract.  Without `labels` stage 2 is not run.
 * Limits, ordering, scratch.  clwh_mask_geodesic's limits.  SYNCHRONOUS, ordered on the context's stream, returns with everything
 * written.  The scratch is that call's 8 * X * Y * Z bytes, reused as two uint32 arrays, its worklist with a second word per tile, and
 * the copied seeds.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or result; a cost that is NULL, an image or not
 * 2-byte aligned; a domain that is given and breaks grow's rules for a mask (an image, not 8-byte aligned); level and labels both NULL,
 * one of them an image or not 4-byte aligned; CLWH_GEO_FROM_LABELS with a NULL, image or misaligned seed_labels; unknown flag bits;
 * dims that break the limits; plateau_cap > 65534; level_cap > 65535; n_seeds > CLWH_GROW_MAX_SEEDS, n_seeds > 0 with NULL seeds,
 * n_seeds == 0 without CLWH_GEO_FROM_LABELS; a seed outside the volume or with id 0.  CLWH_ERR_SIZE_MISMATCH: a cost smaller than
 * 2 * X * Y * Z bytes; a domain smaller than its layout; level, labels or (with the flag) seed_labels smaller than 4 * X * Y * Z bytes.
 * CLWH_ERR_OUT_OF_MEMORY: scratch that cannot be allocated.  Nothing is written on any of these.  (CLWH_ERR_INTERNAL_OVERFLOW: a stage
 * passed its hard cap of X * Y * Z + 2 rounds, which no input can cause: cutting a loop out of a path never raises its state, so every
 * ML is attained by a path that visits no voxel twice and crosses fewer tile faces than the volume has voxels; the same holds for the
 * chain of edges behind a label.) */
#define CLWH_WATERSHED_PLATEAU_MAX 65534u
#define CLWH_WATERSHED_LEVEL_MAX 65535u
typedef struct clwh_watershed_result {
  uint64_t reached;
  uint32_t max_level;
  uint32_t rounds;
} clwh_watershed_result;
typedef struct clwh_watershed_desc {
  clwh_mem *cost;             /* plain device buffer, uint16[Z][Y][X]; read only; 0 = wall */
  clwh_mem *domain;           /* optional plain device buffer in the mask layout; read only */
  clwh_mem *seed_labels;      /* CLWH_GEO_FROM_LABELS: plain device buffer, uint32[Z][Y][X] */
  clwh_mem *level;            /* optional plain device buffer, uint32[Z][Y][X] = M << 16 | L */
  clwh_mem *labels;           /* optional, the same; may name seed_labels' memory */
  uint32_t dims[3];           /* X, Y, Z */
  uint32_t plateau_cap;       /* 0 .. 65534 */
  uint32_t level_cap;         /* 0 .. 65535 */
  int32_t flags;              /* clwh_geodesic_flags */
  uint32_t n_seeds;
  const uint32_t *seeds;      /* host; uint32[n_seeds][4] = x, y, z, id */
  clwh_watershed_result *result;  /* host; required */
} clwh_watershed_desc;
int clwh_watershed(clwh_ctx *ctx, const clwh_watershed_desc *desc);

/* ---- measuring a region (not in the reference): once a mask has been grown, dilated, closed, intersected or selected from a
 * labelling, "how many voxels is this now, what is its mean density, where is it, how large is its surface" -- on the device, as exact
 * integers.  A region is a set R of voxels of the volume V[z][y][x] (an S16 3-D image with one channel; the dims come from it).  The
 * record of R, every field an exact integer:
 *   count, sum (of V over R), sum_sq (of V * V), vmin, vmax (0 when count == 0);
 *   sum_pos[c] = the sum of p.c over R, the centroid's numerators (voxel centres are at p + 0.5);
 *   bbox_lo, bbox_hi (hi exclusive; all zero when count == 0);
 *   faces[c] = the number of pairs (p, p + e_c), both inside the volume, of which exactly one is in R;
 *   border_faces[c] = #{p in R : p.c == 0} + #{p in R : p.c == dim_c - 1}, so a voxel with dim_c == 1 counts twice.
 * The empty region has the all-zero record.  faces and border_faces are kept apart for the reason clwh_mask_morph gives: the outside of
 * the volume is not clear, so whether the face a scan box cuts through a structure counts as surface is the caller's choice.  The face
 * area over-estimates a smooth surface (by about 1.5 times for a sphere: it measures the staircase); clwh_mesh_isosurface is the other
 * measure.
 * Limits.  Those of clwh_labels_to_mask: no dim of 0, dims within the projections' rule, X * Y * Z <= 2^31 - 1.  Under them every
 * field fits: count < 2^31, |sum| <= 2^15 * count < 2^46, sum_sq <= 2^30 * count < 2^61, sum_pos[c] <= (dim_c - 1) * count
 * < 2^47 while no dim exceeds 2^16 (and below 2^62 for any dims the limits allow), faces[c] < X * Y * Z < 2^31, border_faces[c] <=
 * 2 * count < 2^32. */
typedef struct clwh_region_stats {   /* 104 bytes */
  uint64_t count;
  int64_t sum;                       /* of V over the region */
  uint64_t sum_sq;                   /* of V * V */
  int32_t vmin, vmax;                /* 0 when count == 0 */
  uint64_t sum_pos[3];               /* of p.x, p.y, p.z */
  uint32_t bbox_lo[3], bbox_hi[3];   /* hi exclusive; all zero when count == 0 */
  uint32_t faces[3];
  uint32_t border_faces[3];
} clwh_region_stats;

/* clwh_mask_statistics: the record of R = the set bits of `mask` (clwh_segment_grow's mask layout; read only; bits at x >= X and the
 * padding words are ignored whatever they hold), and optionally the histogram of V over R: `hist`, a plain device buffer, 8-byte
 * aligned, of uint64[n_bins]; bin b counts the region's voxels with hist_lo + b * bin_width <= V < hist_lo + (b + 1) * bin_width
 * (in 64-bit arithmetic), -32768 <= hist_lo <= 32767, bin_width >= 1, 1 <= n_bins <= 65536; all n_bins words are written and nothing
 * behind them; result->hist_below and hist_above count the region's voxels under and over the range (both 0 without `hist`), so that
 * sum(hist) + hist_below + hist_above == count.  Without `hist`, n_bins must be 0 (hist_lo and bin_width are then ignored).
 * SYNCHRONOUS, like clwh_segment_grow: ordered on the context's stream, returns with *result (HOST, required) and hist written.  The
 * volume is read directly; no derived data is built or invalidated.  One pass over mask and volume; the scratch (one record) is kept
 * with the context.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx, desc or result; a NULL or wrong-kind volume; a mask that
 * breaks grow's rules (NULL, an image, not 8-byte aligned); flags other than 0; a hist that is an image or not 8-byte aligned; with a
 * hist, n_bins outside 1 .. 65536, bin_width < 1 or hist_lo outside [-32768, 32767]; without one, n_bins != 0; dims that break the
 * limits.  CLWH_ERR_SIZE_MISMATCH: a mask smaller than its layout, a hist smaller than 8 * n_bins bytes.  CLWH_ERR_OUT_OF_MEMORY:
 * scratch that cannot be allocated.  Nothing is written on any of these. */
typedef struct clwh_mask_stats_result {
  clwh_region_stats stats;
  uint64_t hist_below, hist_above;
} clwh_mask_stats_result;
typedef struct clwh_mask_stats_desc {
  clwh_mem *volume;           /* S16 3-D image, 1 channel */
  clwh_mem *mask;             /* plain device buffer in the mask layout; read only */
  clwh_mem *hist;             /* optional plain device buffer of uint64[n_bins] */
  int32_t hist_lo;            /* -32768 .. 32767 */
  int32_t bin_width;          /* >= 1 */
  int32_t n_bins;             /* 1 .. 65536; 0 without hist */
  int32_t flags;              /* 0 */
  clwh_mask_stats_result *result;  /* host; required */
} clwh_mask_stats_desc;
int clwh_mask_statistics(clwh_ctx *ctx, const clwh_mask_stats_desc *desc);

/* clwh_label_statistics: one record per rank.  `labels`: uint32 [z][y][x], a plain device buffer, 4-byte aligned, of at least
 * 4 * X * Y * Z bytes: what clwh_segment_label wrote, or ANY words the caller made.  `stats`: a plain device buffer, 8-byte aligned, of
 * clwh_region_stats[capacity], 1 <= capacity <= 2^24.  Record k is the record of R_k = { p : labels(p) == k + 1 }; ALL capacity records
 * are written, absent ranks get the all-zero record, and nothing behind them is touched.  Label 0 and labels above capacity belong to
 * no region; for the faces of their neighbours they still count as "not in R_k".  Nothing assumes that a region is connected or that
 * different ranks do not touch: a face between ranks a != b counts for both.  "Which of these 40 pieces is calcified, and where is
 * each" is this call after clwh_segment_label.
 * Asynchronous and ordered on the context's stream, like clwh_labels_to_mask; no host result, no scratch.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx or desc; a NULL or wrong-kind volume; NULL labels, labels
 * that are an image or not 4-byte aligned; NULL stats, stats that are an image or not 8-byte aligned; capacity outside 1 .. 2^24; flags
 * other than 0; dims that break the limits.  CLWH_ERR_SIZE_MISMATCH: labels smaller than 4 * X * Y * Z bytes, stats smaller than
 * 104 * capacity bytes.  Nothing is written on any of these. */
typedef struct clwh_label_stats_desc {
  clwh_mem *volume;           /* S16 3-D image, 1 channel */
  clwh_mem *labels;           /* plain device buffer, uint32[Z][Y][X] */
  clwh_mem *stats;            /* plain device buffer of clwh_region_stats[capacity] */
  uint64_t capacity;          /* 1 .. 2^24 */
  int32_t flags;              /* 0 */
  int32_t reserved;           /* ignored */
} clwh_label_stats_desc;
int clwh_label_statistics(clwh_ctx *ctx, const clwh_label_stats_desc *desc);

/* ---- overlays (not in the reference): a mask or a labelling drawn as coloured, half-transparent areas with an outline over the frame
 * a view has just written -- on a slice (clwh_overlay_slice) or in a camera view (clwh_overlay_camera) -- and the id under every
 * pixel (picking).  A view over buffers the library already produces: no volume is read, rewritten or rebuilt.  Integers and float
 * comparisons only: defined bit for bit.
 * Region.  `region.buffer` is a plain device buffer for dims = X, Y, Z, of one of two kinds:
 *   CLWH_REGION_MASK    clwh_segment_grow's mask layout (8-byte aligned); word(v) = 1 where the bit of voxel v is set, else 0.  Bits
 *                       at x >= X and the padding words are ignored, whatever they hold.
 *   CLWH_REGION_LABELS  uint32 [z][y][x] (4-byte aligned): what clwh_segment_label wrote, or ANY words of the caller's, words
 *                       >= 2^31 included; word(v) = the word.
 * With the filter 1 <= id_lo <= id_hi, id(v) = word(v) if id_lo <= word(v) <= id_hi, else 0.  Limits as clwh_labels_to_mask's: no dim
 * of 0, dims within the projections' rule, X * Y * Z <= 2^31 - 1.
 * Rays.  A ray and its kept samples are defined for EVERY integer pixel (x, y), also outside the launched region:
 *   clwh_overlay_slice   clwh_render_slice's: o = (origin + (float)x * du) + (float)y * dv, p_k = o + normal * ((float)k * step) for
 *                        0 <= k < slab_samples (1 .. 8192), kept iff 0 <= p_k.c < dim_c on all three axes.
 *   clwh_overlay_camera  clwh_render_projection's: generate_ray with the frame IMAGE's dims as totals, o = cam_pos (finite, as
 *                        clwh_render_composite demands), p_k = o + d * ((float)k * step), kept iff t_near <= t_k <= t_far and inside.
 * A kept sample lies in voxel v = ((int)p.x, (int)p.y, (int)p.z).  ID(x, y) = id(v) of the smallest kept k whose id is not 0, K(x, y)
 * that k; ID = 0 if there is no kept sample or every kept sample has id 0.
 * Outputs, written for the pixels of the launched region only.  ids (optional): uint32[height][width] = ID.  t_first (optional):
 * float32[height][width] = (float)K * step, 0x7FC00000 where ID == 0.
 * Frame.  `palette`: a plain device buffer (4-byte aligned) of n_colours (1 .. 65536) packed RGBA8 words, bytes in the frame's
 * order; the colour of a pixel is (r, g, b, A) = palette[(ID - 1) % n_colours].  A pixel with ID != 0 is an OUTLINE pixel iff one of
 * ID(x - 1, y), ID(x + 1, y), ID(x, y - 1), ID(x, y + 1) differs from ID(x, y) -- by the ray formula also at x = -1, x = width,
 * y = -1, y = height, so the edge of the launched region is no boundary and tiling a frame into regions changes no byte; a neighbour
 * without a kept sample has ID 0, so a structure cut by the volume's face is outlined there.  The overlay alpha a of a pixel, all
 * divisions integer: with CLWH_OVERLAY_OUTLINE on an outline pixel a = (A * outline_alpha + 127) / 255; else with CLWH_OVERLAY_FILL
 * on a pixel with ID != 0 a = (A * fill_alpha + 127) / 255; else the pixel is not touched.  Then for c in r, g, b
 * out.c = (in.c * (255 - a) + col.c * a + 127) / 255 and out.alpha = in.alpha + ((255 - in.alpha) * a + 127) / 255; a == 0 leaves
 * the same bytes.  With neither flag the frame is not written at all: the call only produces ids and t_first.  Pixels outside the
 * region are never touched.
 * Skipping.  CLWH_OVERLAY_DENSE reads every kept sample up to the first hit.  Without it an 8^3 brick or a cell of 4^3 bricks may be
 * stepped over unread iff no voxel in it has a nonzero id: the table that says so is built per call from the region (the caller's
 * buffers carry no content version).  Same bytes as the dense walk, by the contract.  As built, clwh_overlay_camera skips and
 * clwh_overlay_slice walks densely (a slab is too short for the table to pay: DESIGN.md); the flag is accepted by both.
 * Errors, tested in this order of kinds.  CLWH_ERR_INVALID_VALUE: a NULL ctx or desc; a NULL or wrong-kind frame; a NULL region
 * buffer or palette, one that is an image or misaligned (8 bytes for a mask, 4 for labels and the palette); ids or t_first that are
 * images; an unknown kind or unknown flag bits; id_lo == 0 or id_lo > id_hi; n_colours outside 1 .. 65536; fill_alpha or
 * outline_alpha above 255; dims beyond the limits; for the slice call clwh_render_slice's conditions on slab_samples, step, origin,
 * du, dv and normal, its 2^30 bound taken with width and height in place of width - 1 and height - 1 (the halo is evaluated); for
 * the camera call clwh_render_composite's conditions on step, t_near, t_far and cam_pos.  CLWH_ERR_BAD_NDRANGE: the region rules of the
 * projections.  CLWH_ERR_SIZE_MISMATCH: a region buffer smaller than its layout, a palette smaller than 4 * n_colours bytes, ids or
 * t_first smaller than 4 * width * height bytes.  Nothing is written on any of these.
 * Asynchronous and ordered on the context's stream; no derived data of any volume is built or invalidated.  The scratch (8 bytes per
 * pixel of the region and its halo, 4 bytes per brick and per cell) is kept with the context and holds nothing between calls.  No
 * host wait except when the scratch grows: a call with a larger region or more bricks than any before it on the context allocates,
 * and waits for the stream's work on the smaller scratch before it frees that (like grow's scratch). */
enum clwh_region_kind { CLWH_REGION_MASK = 0, CLWH_REGION_LABELS = 1 };
enum clwh_overlay_flags {
  CLWH_OVERLAY_FILL = 1,     /* blend the colour over every pixel with ID != 0 */
  CLWH_OVERLAY_OUTLINE = 2,  /* ... and with outline_alpha over the outline pixels */
  CLWH_OVERLAY_DENSE = 4     /* no brick skipping: same result by contract; for tests and timing */
};
typedef struct clwh_overlay_region {
  clwh_mem *buffer;           /* plain device buffer of the given kind */
  int32_t kind;               /* clwh_region_kind */
  uint32_t dims[3];           /* X, Y, Z */
  uint32_t id_lo, id_hi;      /* both ends included; 1 <= id_lo <= id_hi */
} clwh_overlay_region;
typedef struct clwh_overlay_paint {
  clwh_mem *palette;          /* plain device buffer of n_colours RGBA8 words */
  uint32_t n_colours;         /* 1 .. 65536 */
  int32_t flags;              /* clwh_overlay_flags */
  uint32_t fill_alpha, outline_alpha;  /* 0 .. 255 */
  clwh_mem *ids;              /* optional uint32[height][width] */
  clwh_mem *t_first;          /* optional float32[height][width] */
} clwh_overlay_paint;
typedef struct clwh_overlay_slice_desc {
  clwh_mem *frame;            /* RGBA8 2-D image, drawn onto */
  clwh_overlay_region region;
  clwh_overlay_paint paint;
  float origin[3], du[3], dv[3], normal[3];  /* as clwh_slice_desc */
  uint32_t width, height;     /* launched region: multiples of 8, <= frame dims, <= 65535 */
  int32_t slab_samples;       /* 1 .. 8192 */
  float step;                 /* > 0, finite */
} clwh_overlay_slice_desc;
typedef struct clwh_overlay_camera_desc {
  clwh_mem *frame;            /* RGBA8 2-D image, drawn onto; its dims are generate_ray's totals */
  clwh_overlay_region region;
  clwh_overlay_paint paint;
  float cam_pos[3], cam_dir[3];
  uint32_t width, height;
  float step;                 /* h > 0, finite */
  float t_near, t_far;        /* 0 and +INFINITY = whole volume */
  int32_t reserved;           /* ignored */
} clwh_overlay_camera_desc;
int clwh_overlay_slice(clwh_ctx *ctx, const clwh_overlay_slice_desc *desc);
int clwh_overlay_camera(clwh_ctx *ctx, const clwh_overlay_camera_desc *desc);

/* clwh_sdf_build replaces the host loop of signed_distance_field::signed_distance_field
 * (app/signed_distance_field.cpp:7-35): base image + all propagation layers, no host round trip
 * per layer.  `sdf` is an S8 3-D image of the volume's dims.  n_launches (optional) receives the
 * number of create_signed_distance_field layers the reference's loop would have run. */
int clwh_sdf_build(clwh_ctx *ctx, clwh_mem *volume, const char *tf_source, clwh_mem *sdf,
                   int32_t *n_launches);

/* buffer_reset.cl:3-13 / app/renderer.cpp:32-35 */
int clwh_buffer_reset(clwh_ctx *ctx, clwh_mem *buffer_volume);

/* ---- the reference's world-space accumulation fed with contributions computed elsewhere (the pixels of other
 * ranks): utility.cl:20-54 (token + add) with the 256-token rule of ray_marching.cl:28,39 applied to the GLOBAL
 * count ("reference-exact voxel-cache mode").  The reference hands a voxel's tokens to whichever
 * work-items reach the atomic first; across GPUs the exchange fixes one legal outcome of that race instead: the
 * contributions to a voxel are taken in the order the caller lists them -- (rank, pixel) -- while the voxel's count
 * is below 256 and dropped afterwards, so every rank that applies the same list to its replica of buffer_volume ends
 * with the same bytes, equal to the single-GPU cache while the count stays below the cap.
 *   clwh_cache_exchange_plan         once per camera.  entries: int64[n] on the device, the cache entry (what
 *                                    clwh_render_desc.hit_index reports) of every contributing pixel of every rank
 *                                    in (rank, pixel) order; entries outside the cache are ignored.  Blocking
 *                                    (one stable sort).
 *   clwh_cache_apply_contributions   once per pass.  rgb: int32[n][rgb_stride] on the device, the pass's contribution
 *                                    of each listed pixel (clwh_render_desc.contrib rows, gathered), same order.
 *                                    One kernel on the context's stream, no host round trip. */
typedef struct clwh_exchange_plan clwh_exchange_plan;
int clwh_cache_exchange_plan(clwh_ctx *ctx, clwh_mem *entries, uint64_t n, clwh_exchange_plan **out);
int clwh_cache_apply_contributions(clwh_ctx *ctx, clwh_exchange_plan *plan, clwh_mem *buffer_volume, clwh_mem *rgb,
                                   int32_t rgb_stride);
int clwh_cache_exchange_plan_release(clwh_exchange_plan *plan);

/* ---- display hand-off without a host readback.
 * Replaces clw_foreign_memory::acquire / release (opencl_wrapper/include/clw_foreign_memory.hpp:40-46:
 * clEnqueueAcquireGLObjects / clEnqueueReleaseGLObjects on a cl_mem made from a GL texture).  The frame the
 * render kernels write is any device memory adopted with clwh_image_wrap -- the pointer a graphics-interop
 * mapping (hipGraphicsResourceGetMappedPointer on a registered GL buffer) or another framework's allocator hands
 * out -- so the frame never crosses PCIe.  Ordering between the context's stream and the consumer's stream is
 * by HIP events, no host synchronisation:
 *   clwh_ctx_acquire_from(ctx, s)  work queued on the context's stream after this call waits for everything
 *                                  queued on stream `s` so far (the display has finished with the previous frame)
 *   clwh_ctx_release_to(ctx, s)    work queued on stream `s` after this call waits for everything queued on the
 *                                  context's stream so far (the frame is complete before the display reads it)
 * `s` is a hipStream_t (NULL = the default stream). */
int clwh_ctx_acquire_from(clwh_ctx *ctx, void *hip_stream);
int clwh_ctx_release_to(clwh_ctx *ctx, void *hip_stream);

/* ---- transfer function: the parsed form of the generated `is_event_gen` source */
#define CLWH_TF_MAX_RULES 16
typedef struct clwh_tf_rule {
  int32_t v_lo, v_hi;   /* value    in [v_lo, v_hi] */
  int32_t g_lo, g_hi;   /* gradient in [g_lo, g_hi] when use_gradient */
  int32_t use_gradient;
  int32_t writes_color;
  int32_t terminal;
  int32_t color[4];
} clwh_tf_rule;
typedef struct clwh_tf {
  int32_t n;
  clwh_tf_rule rules[CLWH_TF_MAX_RULES];
} clwh_tf;
int clwh_tf_parse(const char *source, clwh_tf *out);

/* ---- diagnostics */
/* self-test of the library's float -> integer conversions (DESIGN.md "Semantics": truncate, saturate, NaN -> 0), which the kernels
 * perform with single hardware instructions: converts n floats on the device both ways -- the instruction and the definition
 * written out -- into int32 / uint32 arrays of 2 n elements each ([0, n): instruction, [n, 2n): definition) */
int clwh_debug_float_conversions(clwh_ctx *ctx, clwh_mem *floats_in, uint64_t n, clwh_mem *i32_out, clwh_mem *u32_out);
/* self-test of the wave-wide minimum k_repack takes over a sub-brick's 64 voxels for the exit-certificate table (cross-lane DPP
 * operations): n (a multiple of 64) values, one wave per 64; u32_out[0, n/64) = that minimum, [n/64, 2n/64) = the same by a shuffle loop */
int clwh_debug_wave_min(clwh_ctx *ctx, clwh_mem *u32_in, uint64_t n, clwh_mem *u32_out);
/* the render path's device functions one by one (csrc/device_math.hpp, render_device.hpp, env_fast.hpp), so that a test can say which
 * function differs from the contract of DESIGN.md "Semantics" and at which input: one lane per record calls the function(s) `which`
 * names, unchanged, on the record's words.  `in` holds n records of 32-bit words, `out` receives n records; floats travel as their bits.
 *   which        in (words)                                     out (words)
 *   ARITH        a.x a.y a.z b.x b.y b.z                        a.x / b.x, sqrtf(a.x), dot3(a, b), length3(a), normalize3(a) [3],
 *                                                               cross3(a, b) [3], cl_min(a.x, b.x), cl_max(a.x, b.x)
 *   HASH         seed                                           hash_u32(seed)
 *   HEMISPHERE   gx gy normal[3] seed roughness                 hemisphere_reflective [3], hemisphere_direction [3]
 *   RAY          origin[3] direction[3] x y x_total y_total     generate_ray(...).direction [3]
 *   CUT          origin[3] direction[3]                         cut_box's flag, cut point [3]; box = (float)params[0..2]
 *   ENV_EXACT    d[3]                                           sample_environment_map(aux, w, h, d); w = params[0], h = params[1]
 *   ENV_FAST     d[3]                                           sample_environment_map_fast: decided (0 / 1), texel (0xFFFFFFFF when not)
 *   ENV_APPROX   y x v                                          atan2_approx(y, x), asin_approx(v)
 *   TONE         sr sg sb count                                 tone_map_rgba8
 *   TAPS         p[3]                                           taps_are_voxel_neighbours(p), cache_entry_of(params[0], params[1], p) as
 *                                                               int64: low word, high word
 *   HULL         k (uint32), scale, v[3]                        hull_direction(k)[3], hull_cell(scale * hull_direction(k)), hull_cell(v):
 *                                                               the hull table's directions and the octahedral cell a vector falls in
 * `aux` is read by the two ENV probes only (null otherwise): an environment image of w * h words, row-major; a caller that stores
 * j * w + i in texel (i, j) reads back the texel the sampler chose.  CLWH_ERR_INVALID_VALUE: a null ctx / in / out / params, an unknown
 * `which`, an ENV probe without aux or with w < 1 or h < 1; CLWH_ERR_SIZE_MISMATCH: n >= 2^31, or `in`, `out` or `aux` shorter than
 * the records (the image); n == 0 does nothing */
enum clwh_probe {
  CLWH_PROBE_ARITH = 0,
  CLWH_PROBE_HASH = 1,
  CLWH_PROBE_HEMISPHERE = 2,
  CLWH_PROBE_RAY = 3,
  CLWH_PROBE_CUT = 4,
  CLWH_PROBE_ENV_EXACT = 5,
  CLWH_PROBE_ENV_FAST = 6,
  CLWH_PROBE_ENV_APPROX = 7,
  CLWH_PROBE_TONE = 8,
  CLWH_PROBE_TAPS = 9,
  CLWH_PROBE_HULL = 10,
  CLWH_PROBE_COUNT = 11
};
int clwh_debug_device_probe(clwh_ctx *ctx, int32_t which, clwh_mem *in, uint64_t n, clwh_mem *out, clwh_mem *aux, const int32_t params[4]);
/* the exit-certificate table of the derived scene data the context rendered from last: info_out = {cells along x, y, z,
 * log2 of a cell's edge in voxels}; host_out (may be null: the shape alone) receives 8 bytes per cell, x fastest, byte o = the entry
 * of direction octant o = [d.x < 0] | [d.y < 0] << 1 | [d.z < 0] << 2: 1..127 = the box towards the octant's corner is free and this is
 * its smallest step value; 0x80 | g = it is not, and g (saturating at 127) cells along the octant's diagonal is the nearest cell
 * whose box is free or that lies outside the volume.  CLWH_ERR_BAD_ARGS: the context holds no scene data */
int clwh_debug_macro_table(clwh_ctx *ctx, void *host_out, uint64_t capacity, int32_t info_out[4]);
/* the arrays k_repack derives from (volume, SDF, transfer function), as the context rendered from them last, raw and in brick order
 * (DESIGN.md 2): info_out = {bricks along x, y, z, 0}; host_out (may be null: the shape alone) receives the array `which` names.
 * Voxel (x, y, z) has slot (((z >> 3) * NBY + (y >> 3)) * NBX + (x >> 3)) * 512 + inner, inner = (z & 4) << 6 | (y & 4) << 5 |
 * (x & 4) << 4 | (z & 3) << 4 | (y & 3) << 2 | (x & 3); a brick's slots beyond the volume are padding.
 *   HIT_RECORDS  two uint32 per slot: word 0 = gx[16:0] | gy[14:0] << 17, word 1 = gy[16:15] | gz[16:0] << 2 | class << 19 (gx, gy, gz:
 *                the voxel's central differences, border 0; class: 1 + index of its first matching rule, 0: none).  Written per 4^3
 *                sub-brick (64 consecutive slots), and only where a voxel of the sub-brick may be an event under some gradient;
 *                the other sub-bricks hold whatever the memory held before and no march reads them
 *   STEP_BYTES   one byte per slot: bit 7 = class != 0, bits 0-6 = max(sdf, 0); padding 0
 *   BRICK_MIN    one uint32 per brick: the smallest free value of its real voxels (0: the voxel may be an event or sdf <= 0, else sdf)
 * CLWH_ERR_INVALID_VALUE: a null ctx / info_out, an unknown `which`; CLWH_ERR_BAD_ARGS: the context holds no scene data;
 * CLWH_ERR_SIZE_MISMATCH: `capacity` is short */
enum clwh_scene_array { CLWH_SCENE_HIT_RECORDS = 0, CLWH_SCENE_STEP_BYTES = 1, CLWH_SCENE_BRICK_MIN = 2 };
int clwh_debug_packed_scene(clwh_ctx *ctx, int32_t which, void *host_out, uint64_t capacity, int32_t info_out[4]);
/* the data the views derive from the volume (projections, compositing, isosurface, slices, the mesher), as the context's last view
 * call left them, raw: info_out = {bricks along x, y, z, cells of 4^3 bricks}; host_out (may be null: the shape alone) receives
 *   BRICKS   int16 per slot, the brick order above, padding 0
 *   TABLE    uint32 per brick: (uint16)min | (uint16)max << 16 over its real voxels
 *   DILATED  the same pair over the brick grown by one voxel, clamped at the volume's faces
 *   COARSE   the same pair per cell of 4^3 bricks over its bricks' DILATED pairs; cells x fastest, ceil(bricks / 4) per axis
 * CLWH_ERR_INVALID_VALUE: a null ctx / info_out, an unknown `which`; CLWH_ERR_BAD_ARGS: the context holds no view data, or DILATED /
 * COARSE is asked for and no call that skips by them (isosurface, slice MAX / MIN, mesher) has built them for the current BRICKS --
 * info_out is filled all the same, nothing is copied; CLWH_ERR_SIZE_MISMATCH: `capacity` is short */
enum clwh_view_array { CLWH_VIEW_BRICKS = 0, CLWH_VIEW_TABLE = 1, CLWH_VIEW_DILATED = 2, CLWH_VIEW_COARSE = 3 };
int clwh_debug_view_data(clwh_ctx *ctx, int32_t which, void *host_out, uint64_t capacity, int32_t info_out[4]);
/* the start-certificate table of the derived scene data the context rendered from last: info_out = {X, Y, Z,
 * 1 if the table was built else 0}; host_out (may be null: the shape alone) receives one byte per voxel, x fastest: bit o is set when
 * no voxel of the box from this voxel (inclusive) to the volume corner direction octant o heads for may be an event.  Nothing is
 * written when the table was not built.  CLWH_ERR_BAD_ARGS: the context holds no scene data */
int clwh_debug_start_table(clwh_ctx *ctx, void *host_out, uint64_t capacity, int32_t info_out[4]);
/* the smallest min |direction component| with which a start certificate is granted in a volume of X x Y x Z voxels (a multiple of
 * 1/64; 2: never) */
int clwh_debug_start_cert_dmin(int32_t X, int32_t Y, int32_t Z, float *dmin_out);
/* the hit records of the camera the context rendered last: *n_hits_out = their number; host_out (may be null: the count alone) receives
 * 64 bytes per hit: float origin[3], direction[3], normal[3]; uint32 colour; int64 cache entry; uint32 x | y << 16, pixel slot,
 * start-certificate byte, 0.  CLWH_ERR_BAD_ARGS: no camera yet */
int clwh_debug_hit_records(clwh_ctx *ctx, void *host_out, uint64_t capacity, uint32_t *n_hits_out);
/* the hull-certificate table of the derived scene data the context rendered from last: info_out = {cells of the
 * octahedral grid along one axis, planes, 0, 1 if the table was built else 0}; host_out (may be null: the shape alone) receives four
 * floats per plane k = j * grid + i: the unit normal n_k (the octahedral decode of the centre of cell (i, j)) and h_k, above the largest
 * n_k . c over the eight corners c of every event voxel by the slack clwh_debug_hull_cert_bound names, within 2^-9; +inf: no plane.
 * Nothing is written when the table was not built.  CLWH_ERR_BAD_ARGS: the context holds no scene data */
int clwh_debug_hull_table(clwh_ctx *ctx, void *host_out, uint64_t capacity, int32_t info_out[4]);
/* out[0]: the smallest direction . n_k with which a hull certificate is granted in a volume of X x Y x Z voxels (a multiple of 1/64;
 * 2: never); out[1]: the slack every h_k of the table includes */
int clwh_debug_hull_cert_bound(int32_t X, int32_t Y, int32_t Z, float out[2]);
/* per hit of the camera the context rendered last (the order of clwh_debug_hit_records), one uint32: 0 = no plane of the hull table has
 * the hit's start point P = (origin + direction) + 2 normal in front of it (or there is no table); else bits 0-12 = 1 + the plane's
 * index, bits 16-31 = n_k . P - h_k in 1/256 voxels, rounded down, saturating.  CLWH_ERR_BAD_ARGS: no camera yet */
int clwh_debug_hull_codes(clwh_ctx *ctx, void *host_out, uint64_t capacity, uint32_t *n_hits_out);
/* the second word per hit, same order: 0 = the start point has a NaN or no plane of the search lies within D
 * voxels of it, else 1 + the plane's index in bits 0-12 and, in bits 16-23, the signed margin n_k . P - h_k in 1/scale voxels, rounded
 * down, two's complement, clamped to 127.  All zero without a table or under CLWH_TUNE_HULL_DEFER=0. */
int clwh_debug_hull_planes(clwh_ctx *ctx, void *host_out, uint64_t capacity, uint32_t *n_hits_out);
/* out = {the smallest direction . n_k with which a march that has got in front of its plane within J literal steps is granted in a
 * volume of X x Y x Z voxels (2: never), J, D (voxels), scale} */
int clwh_debug_hull_defer_bound(int32_t X, int32_t Y, int32_t Z, float out[4]);
/* tilted planes: out = {the same bound over 70 - 5 - J steps with the J that armed marches get when the rule is on
 * (2: never), that J, the longest path P a tilted plane may ask a march to count, the margin the tilt aims above the bound, the target
 * t, t / sqrt(1 - t^2)} */
int clwh_debug_hull_tilt_bound(int32_t X, int32_t Y, int32_t Z, float out[6]);
/* the hull table's h_k alone (4096 floats), as k_bounce's tilted-plane test reads them; info_out = {grid, planes, 0, 1 if the scene has
 * the table}.  host_out NULL: the size alone */
int clwh_debug_hull_h(clwh_ctx *ctx, void *host_out, uint64_t capacity, int32_t info_out[4]);
const char *clwh_strerror(int status);
int clwh_last_hip_error(void);
const char *clwh_version(void);
/* per-context timing of the dominant kernel of clwh_render: when enabled, every clwh_render records
 * a HIP event pair on the context's stream around that kernel (no host sync per pass);
 * clwh_ctx_timing_read waits for them, returns the summed duration and launch count, and resets. */
int clwh_ctx_set_timing(clwh_ctx *ctx, int enabled);
int clwh_ctx_timing_read(clwh_ctx *ctx, float *total_ms, int32_t *launches);
/* the same per kernel of the render path: ms[k] / launches[k] for k < n, k = enum clwh_timer (HIP events on the
 * context's stream around each launch; what bench.py's per-kernel roofline is computed from) */
enum clwh_timer {
  CLWH_TIMER_BOUNCE = 0,   /* k_bounce (the dominant kernel; what clwh_ctx_timing_read returns) */
  CLWH_TIMER_PRIMARY = 1,  /* k_primary */
  CLWH_TIMER_FIXUP = 2,    /* k_env_fixup + k_commit */
  CLWH_TIMER_RESOLVE = 3,  /* k_resolve / k_accum_resolve */
  CLWH_TIMER_REPACK = 4,   /* k_repack */
  CLWH_TIMER_AO = 5,       /* k_ao */
  CLWH_TIMER_COUNT = 6
};
int clwh_ctx_timing_read_all(clwh_ctx *ctx, float *ms, int32_t *launches, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* CLWH_H */
