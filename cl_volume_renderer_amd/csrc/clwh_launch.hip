// clwh_launch.hip -- clwh_kernel_get / clwh_launch: the reference's kernels found by their (file, entry) names and launched with
// the reference kernels' own argument lists, by position.  One function per kernel; the pre-processing kernels they launch are in
// volume_kernels.hip and sdf_layer_kernels.hip, the render kernel goes through clwh_render.
#include <cmath>
#include <cstring>
#include <new>

#include "clwh_host.hpp"

using namespace clvr;

// ---- arguments by position
struct Args {
  const clwh_arg *v;
  int n;
  bool is_mem(int i) const { return v[i].kind == CLWH_ARG_MEM && v[i].v.mem != nullptr; }
  clwh_mem *mem(int i) const { return v[i].v.mem; }
  // `count` arguments, the first `mems` of them memory objects
  bool shaped(int count, int mems) const {
    if (n != count) return false;
    for (int i = 0; i < mems; ++i)
      if (!is_mem(i)) return false;
    return true;
  }
  bool f32(int i, float &o) const {
    if (v[i].kind == CLWH_ARG_F32) { o = v[i].v.f32; return true; }
    if (v[i].kind == CLWH_ARG_F64) { o = (float)v[i].v.f64; return true; }
    return false;
  }
  bool i32(int i, int32_t &o) const {
    switch (v[i].kind) {
      case CLWH_ARG_I32: o = v[i].v.i32; return true;
      case CLWH_ARG_U32: o = (int32_t)v[i].v.u32; return true;
      case CLWH_ARG_I64: o = (int32_t)v[i].v.i64; return true;
      case CLWH_ARG_U64: o = (int32_t)v[i].v.u64; return true;
      default: return false;
    }
  }
};

static const int16_t *s16(const clwh_mem *m) { return (const int16_t *)m->dptr; }
static int dim(const clwh_mem *m, int q) { return (int)m->dims[q]; }

static int k_empty(clwh_kernel *, const size_t *, const Args &) { return CLWH_OK; }

// render(frame, volume, sdf, env, buffer_volume, 6 x float, int seed)  ray_marching.cl:152
static int k_render(clwh_kernel *k, const size_t g[3], const Args &a) {
  if (!a.shaped(12, 5)) return CLWH_ERR_BAD_ARGS;
  clwh_render_desc d;
  std::memset(&d, 0, sizeof d);
  d.frame = a.mem(0);
  d.volume = a.mem(1);
  d.sdf = a.mem(2);
  d.env = a.mem(3);
  d.buffer_volume = a.mem(4);
  for (int q = 0; q < 3; ++q)
    if (!a.f32(5 + q, d.cam_pos[q]) || !a.f32(8 + q, d.cam_dir[q])) return CLWH_ERR_BAD_ARGS;
  if (!a.i32(11, d.seed)) return CLWH_ERR_BAD_ARGS;
  d.width = (uint32_t)g[0];
  d.height = (uint32_t)g[1];
  d.accum_mode = CLWH_ACCUM_VOXEL_CACHE;
  d.tile_rank = 0;
  d.tile_world = 1;
  d.write_frame = 1;
  return clwh_render(k, &d);
}

// buffer_reset(volume, buffer_volume)  buffer_reset.cl:3
static int k_buffer_reset(clwh_kernel *k, const size_t *, const Args &a) {
  if (!a.shaped(2, 2)) return CLWH_ERR_BAD_ARGS;
  return clwh_buffer_reset(k->ctx, a.mem(1));
}

// fetch_stats(volume, int stats[5])  reference_volume_figures.cl:10
static int k_fetch_stats(clwh_kernel *k, const size_t *, const Args &a) {
  if (!a.shaped(2, 2)) return CLWH_ERR_BAD_ARGS;
  clwh_mem *v = a.mem(0), *st = a.mem(1);
  if (!is_image(v, 3, 1, CLWH_ELEM_S16) || st->bytes < 4 * sizeof(int32_t)) return CLWH_ERR_BAD_ARGS;
  if (!fits_grid_yz(v)) return CLWH_ERR_INVALID_VALUE;
  HIP_TRY(launch_fetch_stats(s16(v), dim(v, 0), dim(v, 1), dim(v, 2), (int32_t *)st->dptr, k->ctx->stream));
  touch(st);
  return CLWH_OK;
}

// tf_sort_values(volume, uint* frame, int width, int height, float min_v, max_v, min_g, max_g)  histogram.cl:4
static int k_tf_sort_values(clwh_kernel *k, const size_t *, const Args &a) {
  if (!a.shaped(8, 2)) return CLWH_ERR_BAD_ARGS;
  clwh_mem *v = a.mem(0), *fr = a.mem(1);
  int32_t w, h;
  float f[4];
  if (!a.i32(2, w) || !a.i32(3, h)) return CLWH_ERR_BAD_ARGS;
  for (int q = 0; q < 4; ++q)
    if (!a.f32(4 + q, f[q])) return CLWH_ERR_BAD_ARGS;
  if (!is_image(v, 3, 1, CLWH_ELEM_S16) || w <= 0 || h <= 0 || fr->bytes < (size_t)w * (size_t)h * 4u) return CLWH_ERR_BAD_ARGS;
  if (!fits_grid_yz(v)) return CLWH_ERR_INVALID_VALUE;
  HIP_TRY(launch_tf_sort_values(s16(v), dim(v, 0), dim(v, 1), dim(v, 2), (uint32_t *)fr->dptr, w, h, f[0], f[1], f[2], f[3], k->ctx->stream));
  touch(fr);
  return CLWH_OK;
}

// tf_flush_color_frame(image2d color_frame, int* frame, int* lookup, int lookup_len)  histogram.cl:34
static int k_tf_flush_color_frame(clwh_kernel *k, const size_t *, const Args &a) {
  if (!a.shaped(4, 3)) return CLWH_ERR_BAD_ARGS;
  clwh_mem *cf = a.mem(0), *fr = a.mem(1), *lk = a.mem(2);
  int32_t len;
  if (!a.i32(3, len) || !is_image(cf, 2, 4, CLWH_ELEM_U8)) return CLWH_ERR_BAD_ARGS;
  const size_t fw = cf->dims[0], fh = cf->dims[1];
  if (fr->bytes < fw * fh * 4u || len < 0 || lk->bytes < (size_t)len * 4u) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(launch_tf_flush_color_frame((uint32_t *)cf->dptr, (int)fw, (int)fh, (const int32_t *)fr->dptr,
                                      (const int32_t *)lk->dptr, len, k->ctx->stream));
  touch(cf);
  return CLWH_OK;
}

// the 13 x 17 tap weights of the bilateral filter, built on first use
static int ensure_bilateral_weights(clwh_ctx *ctx) {
  if (ctx->bilateral_weights.ptr) return CLWH_OK;
  // utility_filter.cl:43-44,53-55: w = exp(-r2/(2 sigma_s^2) - d^2/(2 sigma_r^2)), float operands, the
  // exponential evaluated in binary64 and rounded once.  d >= 16 must already round to zero.
  const float sigmas = 0.6f, sigmar = 1.0f;
  float host[13 * 17];
  for (int r2 = 0; r2 < 13; ++r2)
    for (int d = 0; d < 17; ++d) {
      const float posd = ((float)r2) / (2 * sigmas * sigmas);
      const float cold = ((float)(d * d)) / (2 * sigmar * sigmar);
      host[r2 * 17 + d] = (float)std::exp((double)(-posd - cold));
    }
  for (int r2 = 0; r2 < 13; ++r2)
    if (host[r2 * 17 + 16] != 0.0f) return CLWH_ERR_INTERNAL_OVERFLOW;
  CLWH_TRY(ctx->bilateral_weights.reserve(ctx->stream, sizeof host));
  HIP_TRY(hipMemcpy(ctx->bilateral_weights.ptr, host, sizeof host, hipMemcpyHostToDevice));
  return CLWH_OK;
}

// bilateral_filter(reference_volume, buffer)  volume_filter.cl:5
static int k_bilateral_filter(clwh_kernel *k, const size_t *, const Args &a) {
  if (!a.shaped(2, 2)) return CLWH_ERR_BAD_ARGS;
  clwh_mem *src = a.mem(0), *dst = a.mem(1);
  if (!is_image(src, 3, 1, CLWH_ELEM_S16) || !is_image(dst, 3, 1, CLWH_ELEM_S16)) return CLWH_ERR_BAD_ARGS;
  if (src->dptr == dst->dptr) return CLWH_ERR_BAD_ARGS;  // a stencil cannot run in place
  if (!same_dims(src, dst)) return CLWH_ERR_SIZE_MISMATCH;  // the reference writes to src's coordinates
  if (src->dims[0] > 0x7fffffffu || src->dims[1] > 8u * 65535u || src->dims[2] > 8u * 65535u) return CLWH_ERR_INVALID_VALUE;
  CLWH_TRY(ensure_bilateral_weights(k->ctx));
  HIP_TRY(launch_bilateral_filter(s16(src), dim(src, 0), dim(src, 1), dim(src, 2), (int16_t *)dst->dptr,
                                  k->ctx->bilateral_weights.as<float>(), k->ctx->stream));
  touch(dst);
  return CLWH_OK;
}

// apply_clip(original, clipped, uint start[3], uint len[4])  reference_volume_clip.cl:4
static int k_apply_clip(clwh_kernel *k, const size_t *, const Args &a) {
  if (!a.shaped(4, 4)) return CLWH_ERR_BAD_ARGS;
  clwh_mem *src = a.mem(0), *dst = a.mem(1), *start = a.mem(2), *len = a.mem(3);
  if (!is_image(src, 3, 1, CLWH_ELEM_S16) || !is_image(dst, 3, 1, CLWH_ELEM_S16) || start->bytes < 12 || len->bytes < 12)
    return CLWH_ERR_BAD_ARGS;
  if (!fits_grid_yz(dst)) return CLWH_ERR_INVALID_VALUE;
  HIP_TRY(launch_apply_clip(s16(src), dim(src, 0), dim(src, 1), dim(src, 2), (int16_t *)dst->dptr, dim(dst, 0), dim(dst, 1), dim(dst, 2),
                            (const uint32_t *)start->dptr, (const uint32_t *)len->dptr, k->ctx->stream));
  touch(dst);
  return CLWH_OK;
}

// create_base_image(volume, ping, pong, uint max_iterations)  signed_distance_field.cl:6
static int k_sdf_base(clwh_kernel *k, const size_t *, const Args &a) {
  if (!a.shaped(4, 3) || !k->has_tf) return CLWH_ERR_BAD_ARGS;
  clwh_mem *v = a.mem(0), *ping = a.mem(1), *pong = a.mem(2);
  SdfArgs s;
  std::memset(&s, 0, sizeof s);
  if (!a.i32(3, s.max_iterations)) return CLWH_ERR_BAD_ARGS;
  if (!is_image(v, 3, 1, CLWH_ELEM_S16) || !is_image(ping, 3, 1, CLWH_ELEM_S8) || !is_image(pong, 3, 1, CLWH_ELEM_S8))
    return CLWH_ERR_BAD_ARGS;
  if (!same_dims(v, ping) || !same_dims(v, pong)) return CLWH_ERR_SIZE_MISMATCH;
  if (!fits_grid_yz(v)) return CLWH_ERR_INVALID_VALUE;
  s.volume = s16(v);
  s.X = dim(v, 0); s.Y = dim(v, 1); s.Z = dim(v, 2);
  s.ping = (int8_t *)ping->dptr;
  s.pong = (int8_t *)pong->dptr;
  CLWH_TRY(kernel_tf(k, v, s.tf, &s.cls_in));
  HIP_TRY(launch_sdf_base(s, k->ctx->stream));
  touch(ping);
  touch(pong);
  return CLWH_OK;
}

// create_signed_distance_field(in, out, int iteration, int* add_buffer, int max_iterations)
static int k_sdf_layer(clwh_kernel *k, const size_t *, const Args &a) {
  if (!a.shaped(5, 2) || !a.is_mem(3)) return CLWH_ERR_BAD_ARGS;
  clwh_mem *in = a.mem(0), *out = a.mem(1), *counter = a.mem(3);
  SdfArgs s;
  std::memset(&s, 0, sizeof s);
  if (!a.i32(2, s.iteration) || !a.i32(4, s.max_iterations)) return CLWH_ERR_BAD_ARGS;
  if (!is_image(in, 3, 1, CLWH_ELEM_S8) || !is_image(out, 3, 1, CLWH_ELEM_S8) || counter->bytes < 4) return CLWH_ERR_BAD_ARGS;
  if (!same_dims(in, out)) return CLWH_ERR_SIZE_MISMATCH;
  if (!fits_grid_yz(in)) return CLWH_ERR_INVALID_VALUE;
  s.X = dim(in, 0); s.Y = dim(in, 1); s.Z = dim(in, 2);
  s.ping = (int8_t *)in->dptr;
  s.pong = (int8_t *)out->dptr;
  s.counter_out = (int32_t *)counter->dptr;
  HIP_TRY(launch_sdf_layer(s, k->ctx->stream));
  touch(out);
  touch(counter);
  return CLWH_OK;
}

// ---- the registry: the reference's (file, entry) names, whether the kernel needs the transfer-function source prepended
struct KernelEntry {
  const char *file, *entry;
  int id;
  bool needs_tf;
  int (*launch)(clwh_kernel *k, const size_t global[3], const Args &args);
};
static const KernelEntry kKernels[] = {
    {"ray_marching.cl", "render", CLWH_K_RENDER, true, k_render},
    {"signed_distance_field.cl", "create_base_image", CLWH_K_SDF_BASE, true, k_sdf_base},
    {"signed_distance_field.cl", "create_signed_distance_field", CLWH_K_SDF_LAYER, false, k_sdf_layer},
    {"buffer_reset.cl", "buffer_reset", CLWH_K_BUFFER_RESET, false, k_buffer_reset},
    {"empty.cl", "empty", CLWH_K_EMPTY, false, k_empty},
    {"reference_volume_figures.cl", "fetch_stats", CLWH_K_FETCH_STATS, false, k_fetch_stats},
    {"reference_volume_clip.cl", "apply_clip", CLWH_K_APPLY_CLIP, false, k_apply_clip},
    {"histogram.cl", "tf_sort_values", CLWH_K_TF_SORT_VALUES, false, k_tf_sort_values},
    {"histogram.cl", "tf_flush_color_frame", CLWH_K_TF_FLUSH_COLOR_FRAME, false, k_tf_flush_color_frame},
    {"volume_filter.cl", "bilateral_filter", CLWH_K_BILATERAL_FILTER, false, k_bilateral_filter},
};

static void normalise3(const size_t in[3], size_t out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = (in && in[k]) ? in[k] : 1;
}

extern "C" {

int clwh_kernel_get(clwh_ctx *ctx, const char *file, const char *entry, const char *prepend, clwh_kernel **out) {
  if (!ctx || !file || !entry || !out) return CLWH_ERR_INVALID_VALUE;
  *out = nullptr;
  // the reference passes paths relative to KERNEL_DIR; accept a directory prefix
  const char *base = std::strrchr(file, '/');
  base = base ? base + 1 : file;
  const KernelEntry *found = nullptr;
  for (const KernelEntry &e : kKernels)
    if (!found && !std::strcmp(base, e.file) && !std::strcmp(entry, e.entry)) found = &e;
  if (!found) return CLWH_ERR_UNKNOWN_KERNEL;
  clwh_kernel *k = new (std::nothrow) clwh_kernel();
  if (!k) return CLWH_ERR_OUT_OF_MEMORY;
  k->ctx = ctx;
  k->id = found->id;
  int rc = CLWH_OK;
  if (found->needs_tf) {
    if (!prepend || prepend[0] == '\0') {
      rc = CLWH_ERR_TF_UNSUPPORTED;  // the reference would fail to compile: is_event_gen is undeclared
    } else {
      rc = clwh_tf_parse(prepend, &k->tf);
      if (rc == CLWH_ERR_TF_UNSUPPORTED) rc = jit_for_source(ctx, prepend, k->jit);  // general fallback: hiprtc
      k->has_tf = rc == CLWH_OK;
    }
  }
  if (rc != CLWH_OK) {
    delete k;
    return rc;
  }
  *out = k;
  return CLWH_OK;
}

int clwh_kernel_release(clwh_kernel *k) {
  if (!k) return CLWH_ERR_INVALID_VALUE;
  delete k;
  return CLWH_OK;
}

int clwh_launch(clwh_kernel *k, const size_t global_in[3], const size_t local_in[3], const clwh_arg *args, int nargs) {
  if (!k || !global_in || !local_in || (nargs > 0 && !args)) return CLWH_ERR_INVALID_VALUE;
  size_t g[3], l[3];
  normalise3(global_in, g);
  normalise3(local_in, l);
  for (int q = 0; q < 3; ++q)
    if (g[q] < l[q] || (g[q] % l[q]) != 0) return CLWH_ERR_BAD_NDRANGE;  // clw_function.hpp:232-237
  HIP_TRY(hipSetDevice(k->ctx->device));
  for (const KernelEntry &e : kKernels)
    if (e.id == k->id) return e.launch(k, g, Args{args, nargs});
  return CLWH_ERR_UNKNOWN_KERNEL;
}

}  // extern "C"
