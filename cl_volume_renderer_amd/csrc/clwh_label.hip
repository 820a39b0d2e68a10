// clwh_label.hip -- clwh_segment_label and clwh_labels_to_mask on the host: the argument checks in the header's order, the scratch, and
// the one read of the device's counts between the union-find and the sort.  The kernels are in label_kernels.hip.
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

static_assert(sizeof(clwh_label_component) == 48 && sizeof(LabelRecord) == 48, "the table's record is 48 bytes");

extern "C" int clwh_segment_label(clwh_ctx *ctx, const clwh_label_desc *d) {
  if (!ctx || !d || !d->result) return CLWH_ERR_INVALID_VALUE;
  if (!volume_ok(d->volume)) return CLWH_ERR_INVALID_VALUE;
  if (!words_ok(d->labels)) return CLWH_ERR_INVALID_VALUE;
  if (d->components ? !mask_ok(d->components) : d->component_capacity > 0) return CLWH_ERR_INVALID_VALUE;  // (a mask's rule: plain, 8-byte aligned)
  const bool from_mask = (d->flags & CLWH_LABEL_FROM_MASK) != 0;
  if (from_mask && !mask_ok(d->mask)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_LABEL_26 | CLWH_LABEL_FROM_MASK)) != 0) return CLWH_ERR_INVALID_VALUE;
  const clwh_mem *vol = d->volume;
  ResolvedBox box;
  if (!resolve_window_and_box(d->lo, d->hi, d->box_lo, d->box_hi, vol, box)) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = vol->dims[0], Y = vol->dims[1], Z = vol->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  const uint64_t voxels = X * Y * Z;
  if (d->labels->bytes / 4u < voxels) return CLWH_ERR_SIZE_MISMATCH;
  if (d->components && d->components->bytes / sizeof(clwh_label_component) < d->component_capacity) return CLWH_ERR_SIZE_MISMATCH;
  if (from_mask && !mask_fits(X, Y, Z, d->mask)) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  clwh_label_result out;
  std::memset(&out, 0, sizeof out);
  if (box.empty) {
    CLWH_TRY(clear_and_wait(ctx, d->labels->dptr, voxels * 4u));
    *d->result = out;
    return CLWH_OK;
  }

  LabelScratch &g = ctx->label;
  const size_t W64 = mask_w64(X);
  CLWH_TRY(g.admissible.reserve(ctx->stream, W64 * 8u * Y * Z));
  CLWH_TRY(g.counters.reserve(ctx->stream, 64));
  CLWH_TRY(g.host.ensure());

  LabelArgs a;
  std::memset(&a, 0, sizeof a);
  a.volume = (const int16_t *)vol->dptr;
  a.mask = from_mask ? (const unsigned long long *)d->mask->dptr : nullptr;
  a.adm = g.admissible.as<unsigned long long>();
  a.labels = (uint32_t *)d->labels->dptr;
  a.X = (int32_t)X;
  a.Y = (int32_t)Y;
  a.Z = (int32_t)Z;
  a.W64 = (int32_t)W64;
  a.lo = d->lo;
  a.hi = d->hi;
  for (int q = 0; q < 3; ++q) {
    a.box_lo[q] = (int32_t)box.lo[q];
    a.box_hi[q] = (int32_t)box.hi[q];
  }
  a.conn26 = (d->flags & CLWH_LABEL_26) != 0;
  a.counters = g.counters.as<unsigned long long>();

  HIP_TRY(hipMemsetAsync(a.counters, 0, 64, ctx->stream));
  HIP_TRY(launch_label_classes(a, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.host.ptr, a.counters, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // the one wait in the middle: the sort's buffers are sized by the number of components
  uint64_t counts[2];
  std::memcpy(counts, g.host.ptr, sizeof counts);
  out.n_components = counts[0];
  out.n_voxels = counts[1];
  out.passes = 4;
  if (counts[0] == 0) {
    CLWH_TRY(clear_and_wait(ctx, d->labels->dptr, voxels * 4u));
    *d->result = out;
    return CLWH_OK;
  }

  a.n_roots = (uint32_t)counts[0];
  a.n_records = d->components ? (uint32_t)(d->component_capacity < counts[0] ? d->component_capacity : counts[0]) : 0u;
  a.records = d->components ? (LabelRecord *)d->components->dptr : nullptr;
  CLWH_TRY(g.keys.reserve(ctx->stream, 2u * (size_t)a.n_roots * sizeof(unsigned long long)));
  a.keys_in = g.keys.as<unsigned long long>();
  a.keys_out = a.keys_in + a.n_roots;
  size_t temp_bytes = 0;
  HIP_TRY(launch_label_sort(nullptr, temp_bytes, a, ctx->stream));
  CLWH_TRY(g.temp.reserve(ctx->stream, temp_bytes ? temp_bytes : 16));
  HIP_TRY(launch_label_keys(a, ctx->stream));
  HIP_TRY(launch_label_sort(g.temp.ptr, temp_bytes, a, ctx->stream));
  HIP_TRY(launch_label_ranks(a, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous by contract
  out.passes = 10;  // (the sort's own launches not counted)
  *d->result = out;
  return CLWH_OK;
}

extern "C" int clwh_labels_to_mask(clwh_ctx *ctx, const clwh_labels_to_mask_desc *d) {
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!words_ok(d->labels)) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->mask)) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  if (d->rank_lo == 0u || d->rank_lo > d->rank_hi) return CLWH_ERR_INVALID_VALUE;
  if (d->labels->bytes / 4u < X * Y * Z) return CLWH_ERR_SIZE_MISMATCH;
  if (!mask_fits(X, Y, Z, d->mask)) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(launch_labels_to_mask((const uint32_t *)d->labels->dptr, (unsigned long long *)d->mask->dptr, (int32_t)X, (int32_t)Y, (int32_t)Z,
                                (int32_t)mask_w64(X), d->rank_lo, d->rank_hi, ctx->stream));
  return CLWH_OK;
}
