// clwh_region_stats.hip -- clwh_mask_statistics and clwh_label_statistics on the host: the argument checks in the header's order, the
// scratch, and the three launches (identities, sums, final form).  The kernels are in region_stats_kernels.hip.
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

static_assert(sizeof(clwh_region_stats) == 104 && sizeof(clwh_mask_stats_result) == 120 && sizeof(clwh_mask_stats_desc) == 48 &&
                  sizeof(clwh_label_stats_desc) == 40,
              "the record and the descriptors as the Python binding lays them out");

extern "C" int clwh_mask_statistics(clwh_ctx *ctx, const clwh_mask_stats_desc *d) {
  if (!ctx || !d || !d->result) return CLWH_ERR_INVALID_VALUE;
  if (!volume_ok(d->volume)) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->mask)) return CLWH_ERR_INVALID_VALUE;
  if (d->flags != 0) return CLWH_ERR_INVALID_VALUE;
  if (d->hist) {
    if (!mask_ok(d->hist)) return CLWH_ERR_INVALID_VALUE;  // a plain buffer of 64-bit words, like a mask
    if (d->n_bins < 1 || d->n_bins > 65536 || d->bin_width < 1 || d->hist_lo < -32768 || d->hist_lo > 32767) return CLWH_ERR_INVALID_VALUE;
  } else if (d->n_bins != 0) {
    return CLWH_ERR_INVALID_VALUE;
  }
  const clwh_mem *vol = d->volume;
  if (!voxels_fit_31_bits(vol->dims[0], vol->dims[1], vol->dims[2])) return CLWH_ERR_INVALID_VALUE;
  if (!mask_fits(vol->dims[0], vol->dims[1], vol->dims[2], d->mask)) return CLWH_ERR_SIZE_MISMATCH;
  if (d->hist && d->hist->bytes / 8u < (size_t)d->n_bins) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  // scratch: the record, behind it {hist_below, hist_above}
  CLWH_TRY(ctx->region_stats.result.reserve(ctx->stream, sizeof(clwh_mask_stats_result)));
  clwh_mask_stats_result *dev = ctx->region_stats.result.as<clwh_mask_stats_result>();

  MaskStatsArgs a;
  std::memset(&a, 0, sizeof a);
  a.volume = (const int16_t *)vol->dptr;
  a.mask = (const uint8_t *)d->mask->dptr;
  a.X = (int32_t)vol->dims[0];
  a.Y = (int32_t)vol->dims[1];
  a.Z = (int32_t)vol->dims[2];
  a.W64 = (int32_t)mask_w64(vol->dims[0]);
  a.result = &dev->stats;
  a.tails = reinterpret_cast<unsigned long long *>(&dev->hist_below);
  if (d->hist) {
    a.hist = (unsigned long long *)d->hist->dptr;
    a.hist_lo = d->hist_lo;
    a.bin_width = (uint32_t)d->bin_width;
    a.n_bins = (uint32_t)d->n_bins;
    HIP_TRY(hipMemsetAsync(a.hist, 0, (size_t)d->n_bins * 8u, ctx->stream));
  }
  HIP_TRY(hipMemsetAsync(a.tails, 0, 16u, ctx->stream));
  HIP_TRY(launch_stats_init(a.result, 1u, ctx->stream));
  HIP_TRY(launch_mask_stats(a, ctx->stream));
  HIP_TRY(launch_stats_finish(a.result, 1u, ctx->stream));
  clwh_mask_stats_result out;
  HIP_TRY(hipMemcpyAsync(&out, dev, sizeof out, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous by contract
  *d->result = out;
  return CLWH_OK;
}

extern "C" int clwh_label_statistics(clwh_ctx *ctx, const clwh_label_stats_desc *d) {
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!volume_ok(d->volume)) return CLWH_ERR_INVALID_VALUE;
  if (!words_ok(d->labels)) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->stats)) return CLWH_ERR_INVALID_VALUE;  // a plain buffer, 8-byte aligned
  if (d->capacity < 1u || d->capacity > (1ull << 24)) return CLWH_ERR_INVALID_VALUE;
  if (d->flags != 0) return CLWH_ERR_INVALID_VALUE;
  const clwh_mem *vol = d->volume;
  if (!voxels_fit_31_bits(vol->dims[0], vol->dims[1], vol->dims[2])) return CLWH_ERR_INVALID_VALUE;
  const size_t voxels = vol->dims[0] * vol->dims[1] * vol->dims[2];
  if (d->labels->bytes / 4u < voxels) return CLWH_ERR_SIZE_MISMATCH;
  if (d->stats->bytes / sizeof(clwh_region_stats) < d->capacity) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  LabelStatsArgs a;
  std::memset(&a, 0, sizeof a);
  a.volume = (const int16_t *)vol->dptr;
  a.labels = (const uint32_t *)d->labels->dptr;
  a.X = (int32_t)vol->dims[0];
  a.Y = (int32_t)vol->dims[1];
  a.Z = (int32_t)vol->dims[2];
  a.capacity = (uint32_t)d->capacity;
  a.stats = (clwh_region_stats *)d->stats->dptr;
  a.mode = ctx->tune.label_stats;
  HIP_TRY(launch_stats_init(a.stats, a.capacity, ctx->stream));
  HIP_TRY(launch_label_stats(a, ctx->stream));
  HIP_TRY(launch_stats_finish(a.stats, a.capacity, ctx->stream));
  return CLWH_OK;
}
