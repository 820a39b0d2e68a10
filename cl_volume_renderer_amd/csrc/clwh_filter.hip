// clwh_filter.hip -- clwh_volume_filter on the host: the argument checks in the header's order, the scratch and the route of the passes
// through it.  The kernels are in filter_kernels.hip.
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

static_assert(sizeof(clwh_filter_desc) == 72, "the descriptor as the Python binding lays it out");

extern "C" int clwh_volume_filter(clwh_ctx *ctx, const clwh_filter_desc *d) {
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!volume_ok(d->volume_in) || !volume_ok(d->volume_out)) return CLWH_ERR_INVALID_VALUE;
  if (d->mask && !mask_ok(d->mask)) return CLWH_ERR_INVALID_VALUE;
  if (d->kind < CLWH_FILTER_MEDIAN || d->kind > CLWH_FILTER_SMOOTH) return CLWH_ERR_INVALID_VALUE;
  if (d->flags != 0) return CLWH_ERR_INVALID_VALUE;
  const uint32_t limit = d->kind == CLWH_FILTER_MEDIAN ? 1u : (uint32_t)CLWH_FILTER_MAX_RADIUS;
  for (int c = 0; c < 3; ++c)
    if (d->radius[c] > limit) return CLWH_ERR_INVALID_VALUE;
  if (d->kind == CLWH_FILTER_SMOOTH)
    for (int c = 0; c < 3; ++c) {
      if (!d->weights[c]) return CLWH_ERR_INVALID_VALUE;
      uint32_t sum = d->weights[c][0];
      for (uint32_t k = 1; k <= d->radius[c]; ++k) sum += 2u * d->weights[c][k];
      if (sum != (uint32_t)CLWH_FILTER_WEIGHT_SUM) return CLWH_ERR_INVALID_VALUE;
    }
  if (!dims_fit_int32(d->volume_in) || !dims_fit_int32(d->volume_out)) return CLWH_ERR_INVALID_VALUE;
  if (!same_dims(d->volume_in, d->volume_out)) return CLWH_ERR_SIZE_MISMATCH;
  const clwh_mem *in = d->volume_in;
  if (d->mask && !mask_fits(in->dims[0], in->dims[1], in->dims[2], d->mask)) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  const int16_t *V = (const int16_t *)in->dptr;
  int16_t *out = (int16_t *)d->volume_out->dptr;
  const bool in_place = (const void *)V == (const void *)out;
  const size_t bytes = in->dims[0] * in->dims[1] * in->dims[2] * sizeof(int16_t);
  int axes[3], n_pass = 0;  // the axes that are filtered, in the contract's order
  for (int c = 0; c < 3; ++c)
    if (d->radius[c] != 0u) axes[n_pass++] = c;

  FilterArgs a;
  std::memset(&a, 0, sizeof a);
  a.X = (int32_t)in->dims[0];
  a.Y = (int32_t)in->dims[1];
  a.Z = (int32_t)in->dims[2];
  a.W64 = (int32_t)mask_w64(in->dims[0]);
  const auto wide = [&](const void *p) { return (int32_t)(((uintptr_t)p & 15u) == 0u && (a.X % 8) == 0); };
  FilterScratch &g = ctx->filter;

  if (n_pass == 0) {  // F = V: a copy, whatever the mask holds
    if (!in_place) HIP_TRY(hipMemcpyAsync(out, V, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  } else if (d->kind == CLWH_FILTER_MEDIAN) {
    if (in_place) {  // the taps and the mask's clear voxels come from a copy
      CLWH_TRY(g.a.reserve(ctx->stream, bytes));
      HIP_TRY(hipMemcpyAsync(g.a.ptr, V, bytes, hipMemcpyDeviceToDevice, ctx->stream));
      V = g.a.as<int16_t>();
    }
    a.src = a.orig = V;
    a.dst = out;
    a.mask = d->mask ? (const uint8_t *)d->mask->dptr : nullptr;
    a.wide_src = wide(a.src);
    HIP_TRY(launch_filter_median(a, (int)d->radius[0], (int)d->radius[1], (int)d->radius[2], ctx->stream));
  } else {
    // V -> (A ->) (B ->) out, so that no pass has src == dst: one pass in place writes A and A is copied; two or three passes never
    // write V before the last, which reads of V only the voxel it writes (the mask's clear bits)
    const bool via_copy = n_pass == 1 && in_place;
    if (n_pass >= 2 || via_copy) CLWH_TRY(g.a.reserve(ctx->stream, bytes));
    if (n_pass == 3) CLWH_TRY(g.b.reserve(ctx->stream, bytes));
    a.orig = V;
    a.mask = d->mask ? (const uint8_t *)d->mask->dptr : nullptr;
    const uint8_t *mask = a.mask;
    const int16_t *src = V;
    for (int p = 0; p < n_pass; ++p) {
      const bool last = p == n_pass - 1;
      int16_t *dst = last ? (via_copy ? g.a.as<int16_t>() : out) : (p == 0 ? g.a.as<int16_t>() : g.b.as<int16_t>());
      a.src = src;
      a.dst = dst;
      a.mask = last ? mask : nullptr;  // the select and the read of V(p) in the last pass only
      a.axis = axes[p];
      a.r = (int32_t)d->radius[axes[p]];
      a.wide_src = wide(a.src);
      a.wide_dst = wide(a.dst);
      a.wide_orig = wide(a.orig);
      if (d->kind == CLWH_FILTER_SMOOTH)
        for (int32_t k = 0; k <= a.r; ++k) a.w[k] = d->weights[axes[p]][k];  // (by value in the launch: copied before the call returns)
      HIP_TRY(launch_filter_line(a, d->kind, ctx->stream));
      src = dst;
    }
    if (via_copy) HIP_TRY(hipMemcpyAsync(out, g.a.ptr, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  }
  touch(d->volume_out);  // a rewrite: what any context derived from this pointer is rebuilt at its next use
  return CLWH_OK;
}
