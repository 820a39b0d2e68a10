// clwh_projection.hip -- clwh_render_projection, clwh_render_composite, clwh_render_isosurface, clwh_render_slice and
// clwh_mesh_isosurface on the host: intensity projections of the volume, compositing through a colour/opacity table, the isosurface of
// the trilinear field, its oblique slices and slabs, and the isosurface as a triangle mesh.  All read the same bricked copy of the
// volume (ensure_projection_data).  The kernels are in projection_kernels.hip, composite_kernels.hip, isosurface_kernels.hip,
// slice_kernels.hip and mesh_kernels.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

// the volume in brick order + the per-brick {min, max} table, rebuilt when the key (device pointer, shared content version, dims)
// changes -- the dims are part of it, so two wraps of one pointer with permuted dims never share a layout
template <class Args>
static int ensure_projection_data(clwh_ctx *ctx, const clwh_mem *volume, Args &a) {
  ProjectionData &p = ctx->proj;
  const int X = (int)volume->dims[0], Y = (int)volume->dims[1], Z = (int)volume->dims[2];
  const int NBX = (X + 7) / 8, NBY = (Y + 7) / 8, NBZ = (Z + 7) / 8;
  const size_t n_bricks = (size_t)NBX * NBY * NBZ;
  const size_t off_table = n_bricks * 512u * sizeof(int16_t);
  const size_t bytes = off_table + n_bricks * sizeof(uint32_t);
  const bool same = p.valid && p.vol == volume->dptr && p.vol_ver == volume->version() &&
                    p.dims[0] == volume->dims[0] && p.dims[1] == volume->dims[1] && p.dims[2] == volume->dims[2];
  if (!same) {
    p.valid = p.dilated_valid = false;  // (the dilated table is derived from this copy)
    CLWH_TRY(p.data.reserve(ctx->stream, bytes));
    ProjRepackArgs r;
    r.volume = (const int16_t *)volume->dptr;
    r.X = X; r.Y = Y; r.Z = Z;
    r.NBX = NBX; r.NBY = NBY; r.NBZ = NBZ;
    r.bricks = p.data.as<int16_t>();
    r.table = reinterpret_cast<uint32_t *>(p.data.as<uint8_t>() + off_table);
    HIP_TRY(launch_proj_repack(r, ctx->stream));
    p.valid = true;
    p.vol = volume->dptr;
    p.vol_ver = volume->version();
    for (int q = 0; q < 3; ++q) p.dims[q] = volume->dims[q];
  }
  a.bricks = p.data.as<int16_t>();
  a.table = reinterpret_cast<const uint32_t *>(p.data.as<uint8_t>() + off_table);
  a.X = X; a.Y = Y; a.Z = Z;
  a.NBX = NBX; a.NBY = NBY;
  return CLWH_OK;
}

// distance from the camera to the farthest corner of the volume's box (infinite for an infinite camera)
static double farthest_corner(const clwh_mem *volume, const float cam_pos[3]) {
  double far = 0.0;
  for (int c = 0; c < 8; ++c) {
    double s2 = 0.0;
    for (int q = 0; q < 3; ++q) {
      const double corner = (c >> q) & 1 ? (double)volume->dims[q] : 0.0;
      s2 += (corner - (double)cam_pos[q]) * (corner - (double)cam_pos[q]);
    }
    far = std::max(far, std::sqrt(s2));
  }
  return far;
}

extern "C" int clwh_render_projection(clwh_ctx *ctx, const clwh_projection_desc *d) {
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!is_image(d->frame, 2, 4, CLWH_ELEM_U8) || !is_image(d->volume, 3, 1, CLWH_ELEM_S16)) return CLWH_ERR_INVALID_VALUE;
  if (d->mode != CLWH_PROJ_MAX && d->mode != CLWH_PROJ_MIN && d->mode != CLWH_PROJ_MEAN) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~CLWH_PROJ_DENSE) != 0) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->step) && d->step > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->window_center) && std::isfinite(d->window_width) && d->window_width > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  if (!(d->t_near <= d->t_far) || d->t_near == INFINITY) return CLWH_ERR_INVALID_VALUE;  // (false for NaN)
  if (!dims_fit_int32(d->volume)) return CLWH_ERR_INVALID_VALUE;
  // every kept sample lies in the volume's box, at most `far` from the camera: k < 2^30 once far / step < 2^29 (|d| = 1 within
  // float rounding), which bounds the kernels' 32-bit sample indices (ProjArgs::k_cap)
  if (!(farthest_corner(d->volume, d->cam_pos) / (double)d->step < 536870912.0)) return CLWH_ERR_INVALID_VALUE;  // (false for an infinite camera)
  if (!launch_size_ok(d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  if (d->width > 65535u || d->height > 65535u) return CLWH_ERR_BAD_NDRANGE;
  if (d->width > d->frame->dims[0] || d->height > d->frame->dims[1]) return CLWH_ERR_BAD_NDRANGE;
  const size_t out_bytes = (size_t)d->width * d->height * sizeof(float);
  if ((d->values && d->values->bytes < out_bytes) || (d->t_extreme && d->t_extreme->bytes < out_bytes)) return CLWH_ERR_SIZE_MISMATCH;

  ProjArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a));
  a.frame = (uint32_t *)d->frame->dptr;
  a.frame_w = (int32_t)d->frame->dims[0];
  a.frame_h = (int32_t)d->frame->dims[1];
  a.launch_w = (int32_t)d->width;
  a.launch_h = (int32_t)d->height;
  a.tiles_x = a.launch_w / 8;
  a.num_tiles = a.tiles_x * (a.launch_h / 8);
  for (int q = 0; q < 3; ++q) {
    a.cam_pos[q] = d->cam_pos[q];
    a.cam_dir[q] = d->cam_dir[q];
  }
  a.step = d->step;
  a.t_near = d->t_near;
  a.t_far = d->t_far;
  a.window_center = d->window_center;
  a.window_width = d->window_width;
  a.k_cap = 1 << 30;
  a.values = d->values ? (float *)d->values->dptr : nullptr;
  a.t_extreme = d->t_extreme ? (float *)d->t_extreme->dptr : nullptr;
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
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!is_image(d->frame, 2, 4, CLWH_ELEM_U8) || !is_image(d->volume, 3, 1, CLWH_ELEM_S16)) return CLWH_ERR_INVALID_VALUE;
  if (!d->lut || !d->lut->dptr || (reinterpret_cast<uintptr_t>(d->lut->dptr) & 15u) != 0u) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_COMP_DENSE | CLWH_COMP_SHADE)) != 0) return CLWH_ERR_INVALID_VALUE;
  if (d->lut_len < 1 || d->lut_len > 65536 || d->lut_first < -65536 || d->lut_first > 65535) return CLWH_ERR_INVALID_VALUE;
  if (!(d->alpha_stop > 0.0f)) return CLWH_ERR_INVALID_VALUE;  // (false for NaN; +inf never stops early)
  const bool shade = (d->flags & CLWH_COMP_SHADE) != 0;
  if (shade && !(d->ambient >= 0.0f && d->ambient <= 1.0f)) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->step) && d->step > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  if (!(d->t_near <= d->t_far) || d->t_near == INFINITY) return CLWH_ERR_INVALID_VALUE;  // (false for NaN)
  if (!dims_fit_int32(d->volume)) return CLWH_ERR_INVALID_VALUE;
  // (std::max in farthest_corner drops a NaN distance, so a camera that is not finite is refused by name)
  if (!(std::isfinite(d->cam_pos[0]) && std::isfinite(d->cam_pos[1]) && std::isfinite(d->cam_pos[2]))) return CLWH_ERR_INVALID_VALUE;
  if (!(farthest_corner(d->volume, d->cam_pos) / (double)d->step < 536870912.0)) return CLWH_ERR_INVALID_VALUE;  // as the projections
  if (!launch_size_ok(d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  if (d->width > 65535u || d->height > 65535u) return CLWH_ERR_BAD_NDRANGE;
  if (d->width > d->frame->dims[0] || d->height > d->frame->dims[1]) return CLWH_ERR_BAD_NDRANGE;
  if (d->lut->bytes < (size_t)d->lut_len * 16u) return CLWH_ERR_SIZE_MISMATCH;
  const size_t out_bytes = (size_t)d->width * d->height * sizeof(float);
  if (d->rgba && d->rgba->bytes < 4u * out_bytes) return CLWH_ERR_SIZE_MISMATCH;
  if ((d->t_first && d->t_first->bytes < out_bytes) || (d->t_stop && d->t_stop->bytes < out_bytes)) return CLWH_ERR_SIZE_MISMATCH;

  CompArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a));
  CLWH_TRY(ensure_lut_prefix(ctx, d->lut, d->lut_len, a));
  a.frame = (uint32_t *)d->frame->dptr;
  a.frame_w = (int32_t)d->frame->dims[0];
  a.frame_h = (int32_t)d->frame->dims[1];
  a.launch_w = (int32_t)d->width;
  a.launch_h = (int32_t)d->height;
  a.tiles_x = a.launch_w / 8;
  a.num_tiles = a.tiles_x * (a.launch_h / 8);
  for (int q = 0; q < 3; ++q) {
    a.cam_pos[q] = d->cam_pos[q];
    a.cam_dir[q] = d->cam_dir[q];
  }
  a.step = d->step;
  a.t_near = d->t_near;
  a.t_far = d->t_far;
  a.k_cap = 1 << 30;
  a.lut = (const float4 *)d->lut->dptr;
  a.lut_first = d->lut_first;
  a.lut_len = d->lut_len;
  a.alpha_stop = d->alpha_stop;
  a.ambient = d->ambient;
  a.rgba = d->rgba ? (float4 *)d->rgba->dptr : nullptr;
  a.t_first = d->t_first ? (float *)d->t_first->dptr : nullptr;
  a.t_stop = d->t_stop ? (float *)d->t_stop->dptr : nullptr;
  HIP_TRY(launch_composite(a, shade, (d->flags & CLWH_COMP_DENSE) != 0, ctx->stream));
  return CLWH_OK;
}

// the {min, max} table of the bricks dilated by one voxel and, behind it, of the cells of 4^3 bricks, built from the bricked copy
// (which ensure_projection_data has just made current: a rebuild of the copy has cleared dilated_valid) by the first isosurface
// call of a volume content, or the first slice call that may skip
template <class Args>
static int ensure_dilated_table(clwh_ctx *ctx, Args &a) {
  ProjectionData &p = ctx->proj;
  if (!p.dilated_valid) {
    const int NBZ = (a.Z + 7) / 8;
    const size_t n_bricks = (size_t)a.NBX * a.NBY * NBZ, n_cells = (size_t)((a.NBX + 3) / 4) * ((a.NBY + 3) / 4) * ((NBZ + 3) / 4);
    CLWH_TRY(p.dilated.reserve(ctx->stream, (n_bricks + n_cells) * sizeof(uint32_t)));
    HIP_TRY(launch_iso_dilate(a.bricks, a.X, a.Y, a.Z, a.NBX, a.NBY, NBZ, p.dilated.as<uint32_t>(), ctx->stream));
    p.dilated_valid = true;
  }
  a.dilated = p.dilated.as<uint32_t>();
  a.coarse = a.dilated + (size_t)a.NBX * a.NBY * ((a.Z + 7) / 8);
  a.CNX = (a.NBX + 3) / 4;
  a.CNY = (a.NBY + 3) / 4;
  return CLWH_OK;
}

extern "C" int clwh_render_isosurface(clwh_ctx *ctx, const clwh_isosurface_desc *d) {
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!is_image(d->frame, 2, 4, CLWH_ELEM_U8) || !is_image(d->volume, 3, 1, CLWH_ELEM_S16)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_ISO_DENSE | CLWH_ISO_BELOW)) != 0) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->iso) && std::fabs(d->iso) <= 65536.0f)) return CLWH_ERR_INVALID_VALUE;
  if (d->refine < 0 || d->refine > 24) return CLWH_ERR_INVALID_VALUE;
  if (!(d->ambient >= 0.0f && d->ambient <= 1.0f)) return CLWH_ERR_INVALID_VALUE;  // (false for NaN)
  if (!(std::isfinite(d->color[0]) && std::isfinite(d->color[1]) && std::isfinite(d->color[2]))) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->step) && d->step > 0.0f)) return CLWH_ERR_INVALID_VALUE;
  if (!(d->t_near <= d->t_far) || d->t_near == INFINITY) return CLWH_ERR_INVALID_VALUE;  // (false for NaN)
  if (!dims_fit_int32(d->volume)) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->cam_pos[0]) && std::isfinite(d->cam_pos[1]) && std::isfinite(d->cam_pos[2]))) return CLWH_ERR_INVALID_VALUE;  // as the compositor
  if (!(farthest_corner(d->volume, d->cam_pos) / (double)d->step < 536870912.0)) return CLWH_ERR_INVALID_VALUE;  // as the projections
  if (!launch_size_ok(d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  if (d->width > 65535u || d->height > 65535u) return CLWH_ERR_BAD_NDRANGE;
  if (d->width > d->frame->dims[0] || d->height > d->frame->dims[1]) return CLWH_ERR_BAD_NDRANGE;
  const size_t out_bytes = (size_t)d->width * d->height * sizeof(float);
  if ((d->t_hit && d->t_hit->bytes < out_bytes) || (d->normal && d->normal->bytes < 4u * out_bytes)) return CLWH_ERR_SIZE_MISMATCH;

  IsoArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a));
  CLWH_TRY(ensure_dilated_table(ctx, a));
  const bool dense = (d->flags & CLWH_ISO_DENSE) != 0, below = (d->flags & CLWH_ISO_BELOW) != 0;
  a.frame = (uint32_t *)d->frame->dptr;
  a.frame_w = (int32_t)d->frame->dims[0];
  a.frame_h = (int32_t)d->frame->dims[1];
  a.launch_w = (int32_t)d->width;
  a.launch_h = (int32_t)d->height;
  a.tiles_x = a.launch_w / 8;
  a.num_tiles = a.tiles_x * (a.launch_h / 8);
  for (int q = 0; q < 3; ++q) {
    a.cam_pos[q] = d->cam_pos[q];
    a.cam_dir[q] = d->cam_dir[q];
    a.color[q] = d->color[q];
  }
  a.step = d->step;
  a.t_near = d->t_near;
  a.t_far = d->t_far;
  a.k_cap = 1 << 30;
  // T = floor(iso * 2^24): the product is exact in binary64 (24 significant bits, |.| <= 2^40)
  a.threshold = (int64_t)std::floor((double)d->iso * 16777216.0);
  // dmax * 2^24 < T  <=>  dmax < ceil(T / 2^24);  dmin * 2^24 > T  <=>  dmin > floor(T / 2^24)  (>> of a negative int64 is arithmetic)
  a.skip_bound = below ? (int32_t)(a.threshold >> 24) : (int32_t)(-((-a.threshold) >> 24));
  a.refine = d->refine;
  a.ambient = d->ambient;
  a.t_hit = d->t_hit ? (float *)d->t_hit->dptr : nullptr;
  a.normal = d->normal ? (float4 *)d->normal->dptr : nullptr;
  HIP_TRY(launch_isosurface(a, below, dense, ctx->stream));
  return CLWH_OK;
}

extern "C" int clwh_render_slice(clwh_ctx *ctx, const clwh_slice_desc *d) {
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!is_image(d->frame, 2, 4, CLWH_ELEM_U8) || !is_image(d->volume, 3, 1, CLWH_ELEM_S16)) return CLWH_ERR_INVALID_VALUE;
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
  if (!dims_fit_int32(d->volume)) return CLWH_ERR_INVALID_VALUE;
  if (!launch_size_ok(d->width, d->height)) return CLWH_ERR_BAD_NDRANGE;
  if (d->width > 65535u || d->height > 65535u) return CLWH_ERR_BAD_NDRANGE;
  if (d->width > d->frame->dims[0] || d->height > d->frame->dims[1]) return CLWH_ERR_BAD_NDRANGE;
  const size_t out_bytes = (size_t)d->width * d->height * sizeof(float);
  if ((d->values && d->values->bytes < out_bytes) || (d->t_extreme && d->t_extreme->bytes < out_bytes)) return CLWH_ERR_SIZE_MISMATCH;

  SliceArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a));
  const bool dense = (d->flags & CLWH_SLICE_DENSE) != 0 || d->mode == CLWH_SLICE_MEAN;  // MEAN reads every kept sample
  if (!dense) CLWH_TRY(ensure_dilated_table(ctx, a));
  a.use_coarse = ctx->tune.slice_coarse;
  a.frame = (uint32_t *)d->frame->dptr;
  a.frame_w = (int32_t)d->frame->dims[0];
  a.frame_h = (int32_t)d->frame->dims[1];
  a.launch_w = (int32_t)d->width;
  a.launch_h = (int32_t)d->height;
  a.tiles_x = a.launch_w / 8;
  a.num_tiles = a.tiles_x * (a.launch_h / 8);
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
  a.values = d->values ? (float *)d->values->dptr : nullptr;
  a.t_extreme = d->t_extreme ? (float *)d->t_extreme->dptr : nullptr;
  HIP_TRY(launch_slice(a, d->mode, dense, ctx->stream));
  return CLWH_OK;
}

// an output of the mesher: a plain device buffer (clwh_mem_create / clwh_mem_wrap), not an image
static bool is_plain_buffer(const clwh_mem *m) { return m && m->dptr && !m->is_image; }

extern "C" int clwh_mesh_isosurface(clwh_ctx *ctx, const clwh_mesh_desc *d) {
  if (!ctx || !d || !d->n_vertices || !d->n_triangles) return CLWH_ERR_INVALID_VALUE;
  if (!is_image(d->volume, 3, 1, CLWH_ELEM_S16)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_MESH_DENSE | CLWH_MESH_BELOW)) != 0) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->iso) && std::fabs(d->iso) <= 65536.0f)) return CLWH_ERR_INVALID_VALUE;
  const bool whole = (d->box_hi[0] | d->box_hi[1] | d->box_hi[2]) == 0u;
  uint64_t lo[3], hi[3];
  for (int q = 0; q < 3; ++q) {
    if (d->volume->dims[q] == 0) return CLWH_ERR_INVALID_VALUE;
    lo[q] = d->box_lo[q];
    hi[q] = whole ? (uint64_t)d->volume->dims[q] - 1u : (uint64_t)d->box_hi[q];
    if (!(lo[q] <= hi[q] && hi[q] <= (uint64_t)d->volume->dims[q] - 1u)) return CLWH_ERR_INVALID_VALUE;
  }
  const clwh_mem *outs[4] = {d->positions, d->normals, d->keys, d->triangles};
  for (const clwh_mem *m : outs)
    if (m && !is_plain_buffer(m)) return CLWH_ERR_INVALID_VALUE;
  if ((d->positions != nullptr) != (d->triangles != nullptr)) return CLWH_ERR_INVALID_VALUE;
  if ((d->normals || d->keys) && !d->positions) return CLWH_ERR_INVALID_VALUE;  // they accompany the positions
  if ((d->vertex_capacity > 0 && !d->positions) || (d->triangle_capacity > 0 && !d->triangles)) return CLWH_ERR_INVALID_VALUE;
  if (!dims_fit_int32(d->volume)) return CLWH_ERR_INVALID_VALUE;
  // (compared by division: capacity * element size may not fit 64 bits)
  if (d->positions && d->vertex_capacity > d->positions->bytes / 12u) return CLWH_ERR_SIZE_MISMATCH;
  if (d->normals && d->vertex_capacity > d->normals->bytes / 12u) return CLWH_ERR_SIZE_MISMATCH;
  if (d->keys && d->vertex_capacity > d->keys->bytes / 8u) return CLWH_ERR_SIZE_MISMATCH;
  if (d->triangles && d->triangle_capacity > d->triangles->bytes / 12u) return CLWH_ERR_SIZE_MISMATCH;

  *d->n_vertices = *d->n_triangles = 0;
  if (lo[0] == hi[0] || lo[1] == hi[1] || lo[2] == hi[2]) return CLWH_OK;  // no cell: the empty mesh

  MeshArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a));
  a.below = (d->flags & CLWH_MESH_BELOW) != 0;
  a.skip = (d->flags & CLWH_MESH_DENSE) == 0;
  if (a.skip) CLWH_TRY(ensure_dilated_table(ctx, a));
  a.n_bricks = (uint64_t)a.NBX * (uint64_t)a.NBY * (uint64_t)((a.Z + 7) / 8);
  for (int q = 0; q < 3; ++q) {
    a.lo[q] = (int32_t)lo[q];
    a.hi[q] = (int32_t)hi[q];
  }
  // T = floor(iso * 2^24), exact in binary64; V << 24 >= T  <=>  V >= ceil(T / 2^24), V << 24 <= T  <=>  V <= floor(T / 2^24)
  a.threshold = (int64_t)std::floor((double)d->iso * 16777216.0);
  a.in_bound = a.below ? (int32_t)(a.threshold >> 24) : (int32_t)(-((-a.threshold) >> 24));

  // the mesher's scratch, kept beside the copy: per brick {vertices, triangles, has a vertex} and their scans, rocPRIM's work space,
  // and (for a filling call) the point table of the bricks that have a vertex
  ProjectionData &p = ctx->proj;
  const size_t n1 = (size_t)a.n_bricks + 1u;
  CLWH_TRY(p.mesh_counts.reserve(ctx->stream, 6u * n1 * sizeof(uint64_t)));
  a.counts = p.mesh_counts.as<uint64_t>();
  uint64_t *bases = a.counts + 3u * n1;
  a.bases = bases;
  size_t temp_bytes = 0;
  HIP_TRY(launch_mesh_scan(nullptr, temp_bytes, a.counts, bases, n1, ctx->stream));
  CLWH_TRY(p.mesh_temp.reserve(ctx->stream, std::max(temp_bytes, (size_t)16)));
  HIP_TRY(launch_mesh_count(a, ctx->stream));
  for (size_t c = 0; c < 3u; ++c) HIP_TRY(launch_mesh_scan(p.mesh_temp.ptr, temp_bytes, a.counts + c * n1, bases + c * n1, n1, ctx->stream));
  uint64_t totals[3] = {0, 0, 0};  // vertices, triangles, bricks with a vertex
  for (size_t c = 0; c < 3u; ++c)
    HIP_TRY(hipMemcpyAsync(&totals[c], bases + c * n1 + (n1 - 1u), sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // the one wait for the counts
  *d->n_vertices = totals[0];
  *d->n_triangles = totals[1];
  if (totals[0] > 0xFFFFFFFFull || totals[1] > 0xFFFFFFFFull) return CLWH_ERR_SIZE_MISMATCH;  // indices are 32-bit
  if (!d->positions) return CLWH_OK;  // a counting call
  if (totals[0] > d->vertex_capacity || totals[1] > d->triangle_capacity) return CLWH_ERR_SIZE_MISMATCH;
  if (totals[0] == 0) return CLWH_OK;  // (no vertex: no triangle)
  CLWH_TRY(p.mesh_points.reserve(ctx->stream, ((size_t)totals[2] + 1u) * 512u * sizeof(uint32_t)));  // (one spare slot: see k_mesh_triangles)
  a.points = p.mesh_points.as<uint32_t>();
  a.positions = (float *)d->positions->dptr;
  a.normals = d->normals ? (float *)d->normals->dptr : nullptr;
  a.keys = d->keys ? (uint64_t *)d->keys->dptr : nullptr;
  a.triangles = (uint32_t *)d->triangles->dptr;
  HIP_TRY(launch_mesh_fill(a, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous by contract: the buffers are written when the call returns
  return CLWH_OK;
}
