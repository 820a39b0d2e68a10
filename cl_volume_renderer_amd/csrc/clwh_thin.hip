// clwh_thin.hip -- clwh_mask_thin and clwh_mask_points on the host: the argument checks in the header's order, the scratch, the batches of
// iterations and the counting call.  The kernels are in thin_kernels.hip.
#include <algorithm>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

static_assert(sizeof(clwh_thin_desc) == 56 && sizeof(clwh_thin_result) == 32 && sizeof(clwh_mask_points_desc) == 64,
              "the descriptors as the Python binding lays them out");
static_assert(2 + 2 * kThinBatch <= 2 * kGrowBatch, "the counters fit the worklist's line and the pinned one");

extern "C" int clwh_mask_thin(clwh_ctx *ctx, const clwh_thin_desc *d) {
  if (!ctx || !d || !d->result) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->mask_in) || !mask_ok(d->mask_out)) return CLWH_ERR_INVALID_VALUE;
  if (d->anchors && !mask_ok(d->anchors)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_THIN_KEEP_ENDS | CLWH_THIN_DENSE)) != 0) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  if (!mask_fits(X, Y, Z, d->mask_in) || !mask_fits(X, Y, Z, d->mask_out)) return CLWH_ERR_SIZE_MISMATCH;
  if (d->anchors && !mask_fits(X, Y, Z, d->anchors)) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  const size_t W64 = mask_w64(X), mask_bytes = W64 * 8u * (size_t)(Y * Z);
  ThinScratch &g = ctx->thin;
  TileWork tiles;
  std::memset(&tiles, 0, sizeof tiles);
  tiles.TX = (int32_t)W64;
  tiles.TY = (int32_t)((Y + 15u) / 16u);
  tiles.TZ = (int32_t)((Z + 15u) / 16u);  // (TX * TY * TZ is below 2^31: a tile holds a voxel)
  void *unused;
  CLWH_TRY(g.candidates.reserve(ctx->stream, mask_bytes));
  CLWH_TRY(tile_work_begin(ctx, g.work, tiles, 0, 0, &unused));  // (clears the stamps)
  ThinArgs a;
  std::memset(&a, 0, sizeof a);
  a.mask = (unsigned long long *)d->mask_out->dptr;
  a.anchors = d->anchors ? (const unsigned long long *)d->anchors->dptr : nullptr;
  a.cand = g.candidates.as<unsigned long long>();
  a.stamps = tiles.stamps;
  a.list = tiles.list;
  a.counters = tiles.counters;
  a.X = (int32_t)X;
  a.Y = (int32_t)Y;
  a.Z = (int32_t)Z;
  a.W64 = (int32_t)W64;
  a.TX = tiles.TX;
  a.TY = tiles.TY;
  a.TZ = tiles.TZ;
  a.dense = (d->flags & CLWH_THIN_DENSE) != 0;
  a.keep_ends = (d->flags & CLWH_THIN_KEEP_ENDS) != 0;

  constexpr size_t kWords = 2u + 2u * (size_t)kThinBatch;
  HIP_TRY(hipMemsetAsync(a.counters, 0, 2u * sizeof(uint32_t), ctx->stream));
  HIP_TRY(launch_thin_begin(a, (const unsigned long long *)d->mask_in->dptr, ctx->stream));

  // Every iteration but the last deletes a voxel: at most count_in + 1 of them.  A batch that turns out to be longer than the thinning
  // costs its idle iterations one word read per block.
  uint64_t iterations = 0, deleted = 0, count_in = 0;
  for (bool done = false; !done;) {
    uint64_t batch = (uint64_t)kThinBatch;
    if (d->max_iterations != 0u) batch = std::min<uint64_t>(batch, (uint64_t)d->max_iterations - iterations);
    HIP_TRY(hipMemsetAsync(a.counters + 2, 0, (kWords - 2u) * sizeof(uint32_t), ctx->stream));
    for (uint64_t slot = 0; slot < batch; ++slot) HIP_TRY(launch_thin_iteration(a, (uint32_t)(iterations + slot + 1u), (int)slot, ctx->stream));
    HIP_TRY(hipMemcpyAsync(g.work.host.ptr, a.counters, kWords * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t *h = g.work.host.ptr;
    count_in = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    for (uint64_t slot = 0; slot < batch && !done; ++slot) {
      ++iterations;
      deleted += h[3u + 2u * slot];
      done = h[3u + 2u * slot] == 0u || iterations == (uint64_t)d->max_iterations;
    }
    if (!done && iterations >= count_in + 1u) return CLWH_ERR_INTERNAL_OVERFLOW;
  }
  clwh_thin_result out;
  std::memset(&out, 0, sizeof out);
  out.count_in = count_in;
  out.deleted = deleted;
  out.count_out = count_in - deleted;
  out.iterations = (uint32_t)iterations;
  *d->result = out;
  return CLWH_OK;
}

extern "C" int clwh_mask_points(clwh_ctx *ctx, const clwh_mask_points_desc *d) {
  if (!ctx || !d || !d->n_points) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->mask)) return CLWH_ERR_INVALID_VALUE;
  const clwh_mem *words[3] = {d->points, d->map, d->values};
  for (const clwh_mem *m : words)
    if (m && !words_ok(m)) return CLWH_ERR_INVALID_VALUE;
  if ((d->map != nullptr) != (d->values != nullptr)) return CLWH_ERR_INVALID_VALUE;
  if (d->values && !d->points) return CLWH_ERR_INVALID_VALUE;
  if (d->capacity > 0 && !d->points) return CLWH_ERR_INVALID_VALUE;
  if (d->flags != 0) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  const size_t voxels = (size_t)(X * Y * Z);
  if (!mask_fits(X, Y, Z, d->mask)) return CLWH_ERR_SIZE_MISMATCH;
  if (d->map && d->map->bytes / 4u < voxels) return CLWH_ERR_SIZE_MISMATCH;
  // (compared by division: capacity * element size may not fit 64 bits)
  if (d->points && d->capacity > d->points->bytes / 16u) return CLWH_ERR_SIZE_MISMATCH;
  if (d->values && d->capacity > d->values->bytes / 4u) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  ThinScratch &g = ctx->thin;
  PointsArgs a;
  std::memset(&a, 0, sizeof a);
  a.mask = (const unsigned long long *)d->mask->dptr;
  a.X = (int32_t)X;
  a.Y = (int32_t)Y;
  a.Z = (int32_t)Z;
  a.W64 = (int32_t)mask_w64(X);
  const size_t n1 = mask_w64(X) * (size_t)(Y * Z) + 1u;  // the words, and one more whose base is the total (below 2^32: so is X * Y * Z)
  CLWH_TRY(g.counts.reserve(ctx->stream, 2u * n1 * sizeof(uint32_t)));
  a.counts = g.counts.as<uint32_t>();
  a.bases = a.counts + n1;
  size_t temp_bytes = 0;
  HIP_TRY(launch_points_scan(nullptr, temp_bytes, a.counts, a.bases, n1, ctx->stream));
  CLWH_TRY(g.temp.reserve(ctx->stream, std::max(temp_bytes, (size_t)16)));
  HIP_TRY(launch_points_count(a, ctx->stream));
  HIP_TRY(launch_points_scan(g.temp.ptr, temp_bytes, a.counts, a.bases, n1, ctx->stream));
  uint32_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, a.bases + (n1 - 1u), sizeof total, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // the one wait for the count
  *d->n_points = total;
  if (!d->points) return CLWH_OK;  // a counting call
  if (total > d->capacity) return CLWH_ERR_SIZE_MISMATCH;
  if (total == 0u) return CLWH_OK;
  a.points = (uint32_t *)d->points->dptr;
  a.map = d->map ? (const uint32_t *)d->map->dptr : nullptr;
  a.values = d->values ? (uint32_t *)d->values->dptr : nullptr;
  HIP_TRY(launch_points_fill(a, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous by contract: the buffers are written when the call returns
  return CLWH_OK;
}
