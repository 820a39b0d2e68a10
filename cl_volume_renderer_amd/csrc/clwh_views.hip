// clwh_views.hip -- the image views of the volume on the host: clwh_render_projection (intensity projections), clwh_render_composite
// (compositing through a colour/opacity table), clwh_render_isosurface (the isosurface of the trilinear field) and clwh_render_slice
// (its oblique slices and slabs).  All read the same bricked copy of the volume (ensure_projection_data), as does the mesher
// (clwh_mesh.hip).  The kernels are in projection_kernels.hip, composite_kernels.hip, isosurface_kernels.hip and slice_kernels.hip.
// Next to the slice clwh_render_curved, the slice with a frame per image row, and clwh_curve_profile, which measures a mask's
// cross-sections along the same rows (curved_kernels.hip).
// Behind them clwh_overlay_slice and clwh_overlay_camera, which draw a mask or a labelling over a frame one of them has written, with
// the slice's or the projection's rays (overlay_kernels.hip); they read no volume.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

// the volume in brick order + the per-brick {min, max} table, rebuilt when the key (device pointer, shared content version, dims)
// changes -- the dims are part of it, so two wraps of one pointer with permuted dims never share a layout
int clvr::ensure_projection_data(clwh_ctx *ctx, const clwh_mem *volume, ViewVolume &v) {
  ProjectionData &p = ctx->proj;
  v.X = (int32_t)volume->dims[0]; v.Y = (int32_t)volume->dims[1]; v.Z = (int32_t)volume->dims[2];
  v.NBX = (v.X + 7) / 8; v.NBY = (v.Y + 7) / 8; v.NBZ = (v.Z + 7) / 8;
  v.CNX = (v.NBX + 3) / 4; v.CNY = (v.NBY + 3) / 4;
  const size_t n_bricks = (size_t)v.NBX * v.NBY * v.NBZ;
  const size_t off_table = n_bricks * 512u * sizeof(int16_t);
  const size_t bytes = off_table + n_bricks * sizeof(uint32_t);
  const bool same = p.valid && p.vol == volume->dptr && p.vol_ver == volume->version() &&
                    p.dims[0] == volume->dims[0] && p.dims[1] == volume->dims[1] && p.dims[2] == volume->dims[2];
  if (!same) {
    p.valid = p.dilated_valid = false;  // (the dilated table is derived from this copy)
    CLWH_TRY(p.data.reserve(ctx->stream, bytes));
    ProjRepackArgs r;
    r.volume = (const int16_t *)volume->dptr;
    r.X = v.X; r.Y = v.Y; r.Z = v.Z;
    r.NBX = v.NBX; r.NBY = v.NBY; r.NBZ = v.NBZ;
    r.bricks = p.data.as<int16_t>();
    r.table = reinterpret_cast<uint32_t *>(p.data.as<uint8_t>() + off_table);
    HIP_TRY(launch_proj_repack(r, ctx->stream));
    p.valid = true;
    p.vol = volume->dptr;
    p.vol_ver = volume->version();
    for (int q = 0; q < 3; ++q) p.dims[q] = volume->dims[q];
  }
  v.bricks = p.data.as<int16_t>();
  v.table = reinterpret_cast<const uint32_t *>(p.data.as<uint8_t>() + off_table);
  return CLWH_OK;
}

// the {min, max} table of the bricks dilated by one voxel and, behind it, of the cells of 4^3 bricks, built from the bricked copy
// (which ensure_projection_data has just made current: a rebuild of the copy has cleared dilated_valid) by the first call of a
// volume content that may skip by it
int clvr::ensure_dilated_table(clwh_ctx *ctx, ViewVolume &v) {
  ProjectionData &p = ctx->proj;
  const size_t n_bricks = (size_t)v.NBX * v.NBY * v.NBZ, n_cells = (size_t)v.CNX * v.CNY * ((v.NBZ + 3) / 4);
  if (!p.dilated_valid) {
    CLWH_TRY(p.dilated.reserve(ctx->stream, (n_bricks + n_cells) * sizeof(uint32_t)));
    HIP_TRY(launch_iso_dilate(v, p.dilated.as<uint32_t>(), ctx->stream));
    p.dilated_valid = true;
  }
  v.dilated = p.dilated.as<uint32_t>();
  v.coarse = v.dilated + n_bricks;
  return CLWH_OK;
}

// ---- what the entry points check alike, by the status a failure returns: every CLWH_ERR_INVALID_VALUE condition of an entry point is
// decided before any CLWH_ERR_BAD_NDRANGE condition, and those before any CLWH_ERR_SIZE_MISMATCH

// (value) the frame and the volume are images of the kinds the views read and write
static bool view_images_ok(const clwh_mem *frame, const clwh_mem *volume) {
  return is_image(frame, 2, 4, CLWH_ELEM_U8) && is_image(volume, 3, 1, CLWH_ELEM_S16) && dims_fit_int32(volume);
}
// (ndrange) the launched region: whole tiles, 16-bit, inside the frame
static bool view_region_ok(const clwh_mem *frame, uint32_t width, uint32_t height) {
  return launch_size_ok(width, height) && width <= 65535u && height <= 65535u && width <= frame->dims[0] && height <= frame->dims[1];
}
// (size) an optional output holds `bytes`
static bool holds(const clwh_mem *m, size_t bytes) { return !m || m->bytes >= bytes; }

// distance from the camera to the farthest corner of the volume's box (infinite for an infinite camera)
static double farthest_corner(const size_t dims[3], const float cam_pos[3]) {
  double far = 0.0;
  for (int c = 0; c < 8; ++c) {
    double s2 = 0.0;
    for (int q = 0; q < 3; ++q) {
      const double corner = (c >> q) & 1 ? (double)dims[q] : 0.0;
      s2 += (corner - (double)cam_pos[q]) * (corner - (double)cam_pos[q]);
    }
    far = std::max(far, std::sqrt(s2));
  }
  return far;
}
// (value) the camera and the march.  Every kept sample lies in the volume's box, at most `far` from the camera: k < 2^30 once
// far / step < 2^29 (|d| = 1 within float rounding), which bounds the kernels' 32-bit sample indices (ViewCamera::k_cap); false for an
// infinite camera.  std::max in farthest_corner drops a NaN distance, so a NaN camera position passes that test: the compositor and
// the isosurface refuse it by name (finite_camera), the projections accept it and find no kept sample (include/clwh.h).
static bool view_march_ok(const size_t dims[3], const float cam_pos[3], float step, float t_near, float t_far, bool finite_camera) {
  if (!(std::isfinite(step) && step > 0.0f)) return false;
  if (!(t_near <= t_far) || t_near == INFINITY) return false;  // (false for NaN)
  if (finite_camera && !(std::isfinite(cam_pos[0]) && std::isfinite(cam_pos[1]) && std::isfinite(cam_pos[2]))) return false;
  return farthest_corner(dims, cam_pos) / (double)step < 536870912.0;
}

static ViewFrame view_frame(const clwh_mem *frame, uint32_t width, uint32_t height) {
  ViewFrame f;
  f.frame = (uint32_t *)frame->dptr;
  f.frame_w = (int32_t)frame->dims[0];
  f.frame_h = (int32_t)frame->dims[1];
  f.launch_w = (int32_t)width;
  f.launch_h = (int32_t)height;
  f.tiles_x = f.launch_w / 8;
  f.num_tiles = f.tiles_x * (f.launch_h / 8);
  return f;
}
static ViewCamera view_camera(const float cam_pos[3], const float cam_dir[3], float step, float t_near, float t_far) {
  ViewCamera c;
  for (int q = 0; q < 3; ++q) {
    c.cam_pos[q] = cam_pos[q];
    c.cam_dir[q] = cam_dir[q];
  }
  c.step = step;
  c.t_near = t_near;
  c.t_far = t_far;
  c.k_cap = 1 << 30;
  return c;
}
template <class T>
static T *optional_output(const clwh_mem *m) { return m ? (T *)m->dptr : nullptr; }

extern "C" int clwh_render_projection(clwh_ctx *ctx, const clwh_projection_desc *d) {
  if (!ctx || !d || !view_images_ok(d->frame, d->volume)) return CLWH_ERR_INVALID_VALUE;
  if (d->mode != CLWH_PROJ_MAX && d->mode != CLWH_PROJ_MIN && d->mode != CLWH_PROJ_MEAN) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~CLWH_PROJ_DENSE) != 0) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->window_center) && std::isfinite(d->window_width) && d->window_width > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  if (!view_march_ok(d->volume->dims, d->cam_pos, d->step, d->t_near, d->t_far, /*finite_camera=*/false)) return CLWH_ERR_INVALID_VALUE;
  if (!view_region_ok(d->frame, d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  const size_t out_bytes = (size_t)d->width * d->height * sizeof(float);
  if (!holds(d->values, out_bytes) || !holds(d->t_extreme, out_bytes)) return CLWH_ERR_SIZE_MISMATCH;

  ProjArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a.vol));
  a.fr = view_frame(d->frame, d->width, d->height);
  a.cam = view_camera(d->cam_pos, d->cam_dir, d->step, d->t_near, d->t_far);
  a.window_center = d->window_center;
  a.window_width = d->window_width;
  a.values = optional_output<float>(d->values);
  a.t_extreme = optional_output<float>(d->t_extreme);
  HIP_TRY(launch_projection(a, d->mode, (d->flags & CLWH_PROJ_DENSE) != 0, ctx->stream));
  return CLWH_OK;
}

// the prefix count of "a > 0" over the table, rebuilt when the key (device pointer, shared content version, length) changes
static int ensure_lut_prefix(clwh_ctx *ctx, const clwh_mem *lut, int32_t lut_len, CompArgs &a) {
  ProjectionData &p = ctx->proj;
  const bool same = p.lut_valid && p.lut == lut->dptr && p.lut_ver == lut->version() && p.lut_len == lut_len;
  if (!same) {
    p.lut_valid = false;
    CLWH_TRY(p.lut_prefix.reserve(ctx->stream, (size_t)lut_len * sizeof(uint32_t)));
    HIP_TRY(launch_comp_prefix((const float4 *)lut->dptr, lut_len, p.lut_prefix.as<uint32_t>(), ctx->stream));
    p.lut_valid = true;
    p.lut = lut->dptr;
    p.lut_ver = lut->version();
    p.lut_len = lut_len;
  }
  a.prefix = p.lut_prefix.as<uint32_t>();
  return CLWH_OK;
}

extern "C" int clwh_render_composite(clwh_ctx *ctx, const clwh_composite_desc *d) {
  if (!ctx || !d || !view_images_ok(d->frame, d->volume)) return CLWH_ERR_INVALID_VALUE;
  if (!d->lut || !d->lut->dptr || (reinterpret_cast<uintptr_t>(d->lut->dptr) & 15u) != 0u) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_COMP_DENSE | CLWH_COMP_SHADE)) != 0) return CLWH_ERR_INVALID_VALUE;
  if (d->lut_len < 1 || d->lut_len > 65536 || d->lut_first < -65536 || d->lut_first > 65535) return CLWH_ERR_INVALID_VALUE;
  if (!(d->alpha_stop > 0.0f)) return CLWH_ERR_INVALID_VALUE;  // (false for NaN; +inf never stops early)
  const bool shade = (d->flags & CLWH_COMP_SHADE) != 0;
  if (shade && !(d->ambient >= 0.0f && d->ambient <= 1.0f)) return CLWH_ERR_INVALID_VALUE;
  if (!view_march_ok(d->volume->dims, d->cam_pos, d->step, d->t_near, d->t_far, /*finite_camera=*/true)) return CLWH_ERR_INVALID_VALUE;
  if (!view_region_ok(d->frame, d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  if (d->lut->bytes < (size_t)d->lut_len * 16u) return CLWH_ERR_SIZE_MISMATCH;
  const size_t out_bytes = (size_t)d->width * d->height * sizeof(float);
  if (!holds(d->rgba, 4u * out_bytes) || !holds(d->t_first, out_bytes) || !holds(d->t_stop, out_bytes)) return CLWH_ERR_SIZE_MISMATCH;

  CompArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a.vol));
  CLWH_TRY(ensure_lut_prefix(ctx, d->lut, d->lut_len, a));
  a.fr = view_frame(d->frame, d->width, d->height);
  a.cam = view_camera(d->cam_pos, d->cam_dir, d->step, d->t_near, d->t_far);
  a.lut = (const float4 *)d->lut->dptr;
  a.lut_first = d->lut_first;
  a.lut_len = d->lut_len;
  a.alpha_stop = d->alpha_stop;
  a.ambient = d->ambient;
  a.rgba = optional_output<float4>(d->rgba);
  a.t_first = optional_output<float>(d->t_first);
  a.t_stop = optional_output<float>(d->t_stop);
  HIP_TRY(launch_composite(a, shade, (d->flags & CLWH_COMP_DENSE) != 0, ctx->stream));
  return CLWH_OK;
}

extern "C" int clwh_render_isosurface(clwh_ctx *ctx, const clwh_isosurface_desc *d) {
  if (!ctx || !d || !view_images_ok(d->frame, d->volume)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_ISO_DENSE | CLWH_ISO_BELOW)) != 0) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->iso) && std::fabs(d->iso) <= 65536.0f)) return CLWH_ERR_INVALID_VALUE;
  if (d->refine < 0 || d->refine > 24) return CLWH_ERR_INVALID_VALUE;
  if (!(d->ambient >= 0.0f && d->ambient <= 1.0f)) return CLWH_ERR_INVALID_VALUE;  // (false for NaN)
  if (!(std::isfinite(d->color[0]) && std::isfinite(d->color[1]) && std::isfinite(d->color[2]))) return CLWH_ERR_INVALID_VALUE;
  if (!view_march_ok(d->volume->dims, d->cam_pos, d->step, d->t_near, d->t_far, /*finite_camera=*/true)) return CLWH_ERR_INVALID_VALUE;
  if (!view_region_ok(d->frame, d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  const size_t out_bytes = (size_t)d->width * d->height * sizeof(float);
  if (!holds(d->t_hit, out_bytes) || !holds(d->normal, 4u * out_bytes)) return CLWH_ERR_SIZE_MISMATCH;

  IsoArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a.vol));
  CLWH_TRY(ensure_dilated_table(ctx, a.vol));
  const bool dense = (d->flags & CLWH_ISO_DENSE) != 0, below = (d->flags & CLWH_ISO_BELOW) != 0;
  a.fr = view_frame(d->frame, d->width, d->height);
  a.cam = view_camera(d->cam_pos, d->cam_dir, d->step, d->t_near, d->t_far);
  for (int q = 0; q < 3; ++q) a.color[q] = d->color[q];
  // T = floor(iso * 2^24): the product is exact in binary64 (24 significant bits, |.| <= 2^40)
  a.threshold = (int64_t)std::floor((double)d->iso * 16777216.0);
  // dmax * 2^24 < T  <=>  dmax < ceil(T / 2^24);  dmin * 2^24 > T  <=>  dmin > floor(T / 2^24)  (>> of a negative int64 is arithmetic)
  a.skip_bound = below ? (int32_t)(a.threshold >> 24) : (int32_t)(-((-a.threshold) >> 24));
  a.refine = d->refine;
  a.ambient = d->ambient;
  a.t_hit = optional_output<float>(d->t_hit);
  a.normal = optional_output<float4>(d->normal);
  HIP_TRY(launch_isosurface(a, below, dense, ctx->stream));
  return CLWH_OK;
}

extern "C" int clwh_render_slice(clwh_ctx *ctx, const clwh_slice_desc *d) {
  if (!ctx || !d || !view_images_ok(d->frame, d->volume)) return CLWH_ERR_INVALID_VALUE;
  if (d->mode != CLWH_SLICE_MAX && d->mode != CLWH_SLICE_MIN && d->mode != CLWH_SLICE_MEAN) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~CLWH_SLICE_DENSE) != 0) return CLWH_ERR_INVALID_VALUE;
  if (d->slab_samples < 1 || d->slab_samples > 8192) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->step) && d->step > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->window_center) && std::isfinite(d->window_width) && d->window_width > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  for (int q = 0; q < 3; ++q) {
    if (!(std::isfinite(d->origin[q]) && std::isfinite(d->du[q]) && std::isfinite(d->dv[q]) && std::isfinite(d->normal[q]))) return CLWH_ERR_INVALID_VALUE;
    // how far any sample of the region can lie from 0 on this axis: below 2^30 every coordinate is finite and converts to int32
    const double reach = std::fabs((double)d->origin[q]) + (d->width ? (double)d->width - 1.0 : 0.0) * std::fabs((double)d->du[q]) +
                         (d->height ? (double)d->height - 1.0 : 0.0) * std::fabs((double)d->dv[q]) +
                         (double)(d->slab_samples - 1) * (double)d->step * std::fabs((double)d->normal[q]);
    if (!(reach < 1073741824.0)) return CLWH_ERR_INVALID_VALUE;
  }
  if (!view_region_ok(d->frame, d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  const size_t out_bytes = (size_t)d->width * d->height * sizeof(float);
  if (!holds(d->values, out_bytes) || !holds(d->t_extreme, out_bytes)) return CLWH_ERR_SIZE_MISMATCH;

  SliceArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a.vol));
  const bool dense = (d->flags & CLWH_SLICE_DENSE) != 0 || d->mode == CLWH_SLICE_MEAN;  // MEAN reads every kept sample
  if (!dense) CLWH_TRY(ensure_dilated_table(ctx, a.vol));
  a.use_coarse = ctx->tune.slice_coarse;
  a.fr = view_frame(d->frame, d->width, d->height);
  for (int q = 0; q < 3; ++q) {
    a.origin[q] = d->origin[q];
    a.du[q] = d->du[q];
    a.dv[q] = d->dv[q];
    a.normal[q] = d->normal[q];
  }
  a.step = d->step;
  a.window_center = d->window_center;
  a.window_width = d->window_width;
  a.slab_samples = d->slab_samples;
  a.values = optional_output<float>(d->values);
  a.t_extreme = optional_output<float>(d->t_extreme);
  HIP_TRY(launch_slice(a, d->mode, dense, ctx->stream));
  return CLWH_OK;
}

// ---- the curved reformat and the section profile along a curve (curved_kernels.hip)
static_assert(sizeof(clwh_curved_desc) == 72 && sizeof(clwh_curve_profile_desc) == 64 && sizeof(clwh_section_record) == 16,
              "the curve descriptors' layout (ffi.py states it again)");

// (value) n rows of origin[3], du[3], normal[3]: every component finite, and on every axis how far any sample of a row of `width`
// pixels and `slab_samples` samples can lie from 0 stays below 2^30 (the slice's reach without a dv)
static bool curve_rows_ok(const float *rows, size_t n, uint32_t width, int32_t slab_samples, float step) {
  const double across = width ? (double)width - 1.0 : 0.0, along = (double)(slab_samples - 1) * (double)step;
  for (size_t y = 0; y < n; ++y) {
    const float *r = rows + y * 9u;
    for (int q = 0; q < 3; ++q) {
      if (!(std::isfinite(r[q]) && std::isfinite(r[3 + q]) && std::isfinite(r[6 + q]))) return false;
      const double reach = std::fabs((double)r[q]) + across * std::fabs((double)r[3 + q]) + along * std::fabs((double)r[6 + q]);
      if (!(reach < 1073741824.0)) return false;
    }
  }
  return true;
}
// the rows into the context's device buffer through its page-locked copy; nobody waits for the stream (CurveScratch)
static int stage_curve_rows(clwh_ctx *ctx, const float *rows, size_t n, const float **device_rows) {
  CurveScratch &s = ctx->curve;
  const size_t bytes = n * 9u * sizeof(float);
  CLWH_TRY(s.rows.reserve(ctx->stream, bytes));
  CLWH_TRY(s.copied.ensure(hipEventDisableTiming));
  if (s.in_flight) HIP_TRY(hipEventSynchronize(s.copied.ev));  // the previous call's copy has left the page-locked rows
  s.in_flight = false;
  if (s.host_bytes < bytes) {
    if (s.host) HIP_TRY(hipHostFree(s.host));
    s.host = nullptr;
    s.host_bytes = 0;
    HIP_TRY(hipHostMalloc((void **)&s.host, bytes, hipHostMallocDefault));
    s.host_bytes = bytes;
  }
  std::memcpy(s.host, rows, bytes);
  HIP_TRY(hipMemcpyAsync(s.rows.ptr, s.host, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipEventRecord(s.copied.ev, ctx->stream));
  s.in_flight = true;
  *device_rows = s.rows.as<float>();
  return CLWH_OK;
}

extern "C" int clwh_render_curved(clwh_ctx *ctx, const clwh_curved_desc *d) {
  if (!ctx || !d || !view_images_ok(d->frame, d->volume) || !d->rows) return CLWH_ERR_INVALID_VALUE;
  if (d->mode != CLWH_SLICE_MAX && d->mode != CLWH_SLICE_MIN && d->mode != CLWH_SLICE_MEAN) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~CLWH_CURVED_DENSE) != 0) return CLWH_ERR_INVALID_VALUE;
  if (d->slab_samples < 1 || d->slab_samples > 8192) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->step) && d->step > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->window_center) && std::isfinite(d->window_width) && d->window_width > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  if (!curve_rows_ok(d->rows, d->height, d->width, d->slab_samples, d->step)) return CLWH_ERR_INVALID_VALUE;
  if (!view_region_ok(d->frame, d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  const size_t out_bytes = (size_t)d->width * d->height * sizeof(float);
  if (!holds(d->values, out_bytes) || !holds(d->t_extreme, out_bytes)) return CLWH_ERR_SIZE_MISMATCH;

  CurvedArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a.vol));
  const bool dense = (d->flags & CLWH_CURVED_DENSE) != 0 || d->mode == CLWH_SLICE_MEAN;  // MEAN reads every kept sample
  if (!dense) CLWH_TRY(ensure_dilated_table(ctx, a.vol));
  CLWH_TRY(stage_curve_rows(ctx, d->rows, d->height, &a.rows));
  a.use_coarse = ctx->tune.slice_coarse;
  a.fr = view_frame(d->frame, d->width, d->height);
  a.step = d->step;
  a.window_center = d->window_center;
  a.window_width = d->window_width;
  a.slab_samples = d->slab_samples;
  a.values = optional_output<float>(d->values);
  a.t_extreme = optional_output<float>(d->t_extreme);
  HIP_TRY(launch_curved(a, d->mode, dense, ctx->stream));
  return CLWH_OK;
}

extern "C" int clwh_curve_profile(clwh_ctx *ctx, const clwh_curve_profile_desc *d) {
  if (!ctx || !d || !mask_ok(d->mask) || !d->rows) return CLWH_ERR_INVALID_VALUE;
  if (!is_plain_buffer(d->records) || ((uintptr_t)d->records->dptr & 15u) != 0u) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~CLWH_PROFILE_CONNECTED) != 0) return CLWH_ERR_INVALID_VALUE;
  if (d->n_rows < 1u || d->n_rows > 65535u || d->width < 1u || d->width > 64u) return CLWH_ERR_INVALID_VALUE;
  if (d->slab_samples < 1 || d->slab_samples > 64) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->step) && d->step > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  if (!curve_rows_ok(d->rows, d->n_rows, d->width, d->slab_samples, d->step)) return CLWH_ERR_INVALID_VALUE;
  if (!mask_fits(X, Y, Z, d->mask)) return CLWH_ERR_SIZE_MISMATCH;
  if (d->records->bytes / sizeof(clwh_section_record) < (size_t)d->n_rows) return CLWH_ERR_SIZE_MISMATCH;

  CurveProfileArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(stage_curve_rows(ctx, d->rows, d->n_rows, &a.rows));
  a.mask = (const unsigned long long *)d->mask->dptr;
  a.X = (int32_t)X;
  a.Y = (int32_t)Y;
  a.Z = (int32_t)Z;
  a.W64 = (int32_t)mask_w64(X);
  a.n_rows = d->n_rows;
  a.width = (int32_t)d->width;
  a.slab_samples = d->slab_samples;
  a.step = d->step;
  a.records = (uint32_t *)d->records->dptr;
  HIP_TRY(launch_curve_profile(a, (d->flags & CLWH_PROFILE_CONNECTED) != 0, ctx->stream));
  return CLWH_OK;
}

// ---- overlays of a mask or a labelling on a frame one of the views above has written (overlay_kernels.hip)
static_assert(sizeof(clwh_overlay_region) == 32 && sizeof(clwh_overlay_paint) == 40 && sizeof(clwh_overlay_slice_desc) == 144 &&
                  sizeof(clwh_overlay_camera_desc) == 128, "the overlay descriptors' layout (ffi.py states it again)");

// (value) what both overlay calls demand of the frame, the region and the paint
static bool overlay_values_ok(const clwh_mem *frame, const clwh_overlay_region &r, const clwh_overlay_paint &p) {
  if (!is_image(frame, 2, 4, CLWH_ELEM_U8)) return false;
  if (r.kind != CLWH_REGION_MASK && r.kind != CLWH_REGION_LABELS) return false;
  if (!is_plain_buffer(r.buffer) || ((uintptr_t)r.buffer->dptr & (r.kind == CLWH_REGION_MASK ? 7u : 3u)) != 0u) return false;
  if (!is_plain_buffer(p.palette) || ((uintptr_t)p.palette->dptr & 3u) != 0u) return false;
  if ((p.ids && !is_plain_buffer(p.ids)) || (p.t_first && !is_plain_buffer(p.t_first))) return false;
  if ((p.flags & ~(CLWH_OVERLAY_FILL | CLWH_OVERLAY_OUTLINE | CLWH_OVERLAY_DENSE)) != 0) return false;
  if (r.id_lo == 0u || r.id_lo > r.id_hi) return false;
  if (p.n_colours < 1u || p.n_colours > 65536u || p.fill_alpha > 255u || p.outline_alpha > 255u) return false;
  // clwh_labels_to_mask's limits: X * Y * Z <= 2^31 - 1, by division (the product may not fit)
  const uint64_t X = r.dims[0], Y = r.dims[1], Z = r.dims[2];
  if (X == 0 || Y == 0 || Z == 0 || X > 0x7FFFFFFFu || Y > 0x7FFFFFFFu || Z > 0x7FFFFFFFu) return false;
  return X * Y <= 0x7FFFFFFFull && Z <= 0x7FFFFFFFull / (X * Y);
}
// (size) the region's buffer holds its layout, the palette its colours, the outputs the launched region
static bool overlay_sizes_ok(const clwh_overlay_region &r, const clwh_overlay_paint &p, uint32_t width, uint32_t height) {
  const uint64_t X = r.dims[0], Y = r.dims[1], Z = r.dims[2];
  if (r.kind == CLWH_REGION_MASK ? r.buffer->bytes / (((X + 63u) / 64u) * 8u) < Y * Z : r.buffer->bytes / 4u < X * Y * Z) return false;
  if (p.palette->bytes < (size_t)p.n_colours * 4u) return false;
  const size_t out_bytes = (size_t)width * height * 4u;
  return holds(p.ids, out_bytes) && holds(p.t_first, out_bytes);
}

// what the two calls share once their checks have passed: a.cam or the plane and a.step are set
static int overlay_run(clwh_ctx *ctx, OverlayArgs &a, const clwh_mem *frame, const clwh_overlay_region &r, const clwh_overlay_paint &p,
                       uint32_t width, uint32_t height, bool camera) {
  HIP_TRY(hipSetDevice(ctx->device));
  ViewVolume &v = a.vol;
  v.X = (int32_t)r.dims[0]; v.Y = (int32_t)r.dims[1]; v.Z = (int32_t)r.dims[2];
  v.NBX = (v.X + 7) / 8; v.NBY = (v.Y + 7) / 8; v.NBZ = (v.Z + 7) / 8;
  v.CNX = (v.NBX + 3) / 4; v.CNY = (v.NBY + 3) / 4;
  a.fr = view_frame(frame, width, height);
  a.kind = r.kind;
  if (r.kind == CLWH_REGION_MASK) a.mask = (const unsigned long long *)r.buffer->dptr;
  else a.labels = (const uint32_t *)r.buffer->dptr;
  a.W64 = (v.X + 63) / 64;
  a.id_lo = r.id_lo;
  a.id_hi = r.id_hi;
  a.palette = (const uint32_t *)p.palette->dptr;
  a.n_colours = p.n_colours;
  a.flags = p.flags;
  a.fill_alpha = p.fill_alpha;
  a.outline_alpha = p.outline_alpha;
  a.ids = optional_output<uint32_t>(p.ids);
  a.t_first = optional_output<float>(p.t_first);
  OverlayScratch &s = ctx->overlay;
  CLWH_TRY(s.pixel_ids.reserve(ctx->stream, ((size_t)width + 2u) * ((size_t)height + 2u) * sizeof(uint2)));
  a.pixel_ids = s.pixel_ids.as<uint2>();
  // the camera's rays step over empty bricks; the plane's walk densely: a slab is short, and the table, which has to be built per call
  // (a caller's buffer has no content version), cost more than it saved in every slab timed
  const bool skip = camera && (p.flags & CLWH_OVERLAY_DENSE) == 0;
  if (skip) {
    const size_t n_bricks = (size_t)v.NBX * v.NBY * v.NBZ, n_cells = (size_t)v.CNX * v.CNY * ((v.NBZ + 3) / 4);
    CLWH_TRY(s.occupancy.reserve(ctx->stream, (n_bricks + n_cells) * sizeof(uint32_t)));
    uint32_t *bricks = s.occupancy.as<uint32_t>();
    HIP_TRY(launch_region_occupancy(a, bricks, bricks + n_bricks, n_cells, ctx->stream));
    a.occ_bricks = bricks;
    a.occ_cells = bricks + n_bricks;
  }
  HIP_TRY(launch_overlay(a, camera, skip, ctx->stream));
  return CLWH_OK;
}

extern "C" int clwh_overlay_slice(clwh_ctx *ctx, const clwh_overlay_slice_desc *d) {
  if (!ctx || !d || !overlay_values_ok(d->frame, d->region, d->paint)) return CLWH_ERR_INVALID_VALUE;
  if (d->slab_samples < 1 || d->slab_samples > 8192) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->step) && d->step > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  for (int q = 0; q < 3; ++q) {
    if (!(std::isfinite(d->origin[q]) && std::isfinite(d->du[q]) && std::isfinite(d->dv[q]) && std::isfinite(d->normal[q]))) return CLWH_ERR_INVALID_VALUE;
    // clwh_render_slice's reach with the halo's pixels -1, width and height: below 2^30 every coordinate converts to int32
    const double reach = std::fabs((double)d->origin[q]) + (double)d->width * std::fabs((double)d->du[q]) +
                         (double)d->height * std::fabs((double)d->dv[q]) +
                         (double)(d->slab_samples - 1) * (double)d->step * std::fabs((double)d->normal[q]);
    if (!(reach < 1073741824.0)) return CLWH_ERR_INVALID_VALUE;
  }
  if (!view_region_ok(d->frame, d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  if (!overlay_sizes_ok(d->region, d->paint, d->width, d->height)) return CLWH_ERR_SIZE_MISMATCH;

  OverlayArgs a;
  std::memset(&a, 0, sizeof a);
  for (int q = 0; q < 3; ++q) {
    a.origin[q] = d->origin[q];
    a.du[q] = d->du[q];
    a.dv[q] = d->dv[q];
    a.normal[q] = d->normal[q];
  }
  a.step = d->step;
  a.slab_samples = d->slab_samples;
  return overlay_run(ctx, a, d->frame, d->region, d->paint, d->width, d->height, /*camera=*/false);
}

extern "C" int clwh_overlay_camera(clwh_ctx *ctx, const clwh_overlay_camera_desc *d) {
  if (!ctx || !d || !overlay_values_ok(d->frame, d->region, d->paint)) return CLWH_ERR_INVALID_VALUE;
  const size_t dims[3] = {d->region.dims[0], d->region.dims[1], d->region.dims[2]};
  if (!view_march_ok(dims, d->cam_pos, d->step, d->t_near, d->t_far, /*finite_camera=*/true)) return CLWH_ERR_INVALID_VALUE;
  if (!view_region_ok(d->frame, d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  if (!overlay_sizes_ok(d->region, d->paint, d->width, d->height)) return CLWH_ERR_SIZE_MISMATCH;

  OverlayArgs a;
  std::memset(&a, 0, sizeof a);
  a.cam = view_camera(d->cam_pos, d->cam_dir, d->step, d->t_near, d->t_far);
  a.step = d->step;
  return overlay_run(ctx, a, d->frame, d->region, d->paint, d->width, d->height, /*camera=*/true);
}
