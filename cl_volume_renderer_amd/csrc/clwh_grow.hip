// clwh_grow.hip -- clwh_segment_grow and clwh_volume_apply_mask on the host: the argument checks in the header's order, the scratch, and
// the rounds of the tiles' worklist.  The kernels are in grow_kernels.hip.
#include <algorithm>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

extern "C" int clwh_segment_grow(clwh_ctx *ctx, const clwh_grow_desc *d) {
  if (!ctx || !d || !d->result) return CLWH_ERR_INVALID_VALUE;
  if (!volume_ok(d->volume)) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->mask)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_GROW_26 | CLWH_GROW_FROM_MASK | CLWH_GROW_DENSE)) != 0) return CLWH_ERR_INVALID_VALUE;
  const clwh_mem *vol = d->volume;
  ResolvedBox box;
  if (!resolve_window_and_box(d->lo, d->hi, d->box_lo, d->box_hi, vol, box)) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds > CLWH_GROW_MAX_SEEDS || (d->n_seeds > 0 && !d->seeds)) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds == 0 && !(d->flags & CLWH_GROW_FROM_MASK)) return CLWH_ERR_INVALID_VALUE;
  for (uint32_t i = 0; i < d->n_seeds; ++i)
    for (int q = 0; q < 3; ++q)
      if ((uint64_t)d->seeds[3u * i + (uint32_t)q] >= (uint64_t)vol->dims[q]) return CLWH_ERR_INVALID_VALUE;
  if (!dims_fit_int32(vol)) return CLWH_ERR_INVALID_VALUE;
  const size_t W64 = mask_w64(vol->dims[0]), TX = W64, TY = (vol->dims[1] + 15u) / 16u, TZ = (vol->dims[2] + 15u) / 16u;
  if (TY * TZ > 0x7FFFFFFFu / TX) return CLWH_ERR_INVALID_VALUE;  // tiles are numbered in 32 bits
  if (!mask_fits(vol->dims[0], vol->dims[1], vol->dims[2], d->mask)) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  const size_t mask_bytes = W64 * 8u * vol->dims[1] * vol->dims[2];
  clwh_grow_result out;
  std::memset(&out, 0, sizeof out);
  if (box.empty) {  // the empty set
    CLWH_TRY(clear_and_wait(ctx, d->mask->dptr, mask_bytes));
    *d->result = out;
    return CLWH_OK;
  }

  // scratch: A; the tiles' worklist with the reduction's result behind it; the seeds
  GrowScratch &g = ctx->grow;
  GrowArgs a;
  std::memset(&a, 0, sizeof a);
  a.tiles.TX = (int32_t)TX;
  a.tiles.TY = (int32_t)TY;
  a.tiles.TZ = (int32_t)TZ;
  a.tiles.dense = (d->flags & CLWH_GROW_DENSE) != 0;
  CLWH_TRY(g.admissible.reserve(ctx->stream, mask_bytes));
  CLWH_TRY(tile_work_begin(ctx, g.work, a.tiles, (size_t)d->n_seeds * 12u, sizeof(GrowDeviceResult), (void **)&a.result));
  a.volume = (const int16_t *)vol->dptr;
  a.mask = (unsigned long long *)d->mask->dptr;
  a.adm = g.admissible.as<unsigned long long>();
  a.X = (int32_t)vol->dims[0];
  a.Y = (int32_t)vol->dims[1];
  a.Z = (int32_t)vol->dims[2];
  a.W64 = (int32_t)W64;
  a.lo = d->lo;
  a.hi = d->hi;
  for (int q = 0; q < 3; ++q) {
    a.box_lo[q] = (int32_t)box.lo[q];
    a.box_hi[q] = (int32_t)box.hi[q];
  }
  a.conn26 = (d->flags & CLWH_GROW_26) != 0;
  a.from_mask = (d->flags & CLWH_GROW_FROM_MASK) != 0;
  a.seeds = g.work.seeds.as<uint32_t>();
  a.n_seeds = d->n_seeds;

  GrowDeviceResult start;
  std::memset(&start, 0, sizeof start);
  start.vmin = INT32_MAX;
  start.vmax = INT32_MIN;
  start.lo[0] = start.lo[1] = start.lo[2] = 0xFFFFFFFFu;
  HIP_TRY(hipMemcpyAsync(a.result, &start, sizeof start, hipMemcpyHostToDevice, ctx->stream));
  if (d->n_seeds > 0) HIP_TRY(hipMemcpyAsync(g.work.seeds.ptr, d->seeds, (size_t)d->n_seeds * 12u, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(launch_grow_admissible(a, ctx->stream));
  HIP_TRY(launch_grow_seeds(a, ctx->stream));

  // Every round that lists a tile sets a bit or leaves the next list empty, so at most count + 2 rounds list one.
  // (X * Y * Z fits: the mask, one bit per voxel, fits the buffer)
  const uint64_t cap = std::min<uint64_t>((uint64_t)vol->dims[0] * vol->dims[1] * vol->dims[2] + 2u, 0xFFFFFF00u);
  uint64_t rounds;
  CLWH_TRY(tile_work_run(ctx, g.work, a.tiles, cap, [&](uint32_t round, int slot) { return launch_grow_round(a, round, slot, ctx->stream); }, &rounds));

  HIP_TRY(launch_grow_reduce(a, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.work.host.ptr, a.result, sizeof(GrowDeviceResult), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous by contract: the mask is written when the call returns
  GrowDeviceResult r;
  std::memcpy(&r, g.work.host.ptr, sizeof r);
  out.rounds = (uint32_t)rounds;
  if (r.count != 0ull) {
    out.count = r.count;
    out.sum = (int64_t)r.sum;
    out.sum_sq = r.sum_sq;
    out.vmin = r.vmin;
    out.vmax = r.vmax;
    for (int q = 0; q < 3; ++q) {
      out.bbox_lo[q] = r.lo[q];
      out.bbox_hi[q] = r.hi[q] + 1u;
    }
  }
  *d->result = out;
  return CLWH_OK;
}

extern "C" int clwh_volume_apply_mask(clwh_ctx *ctx, const clwh_apply_mask_desc *d) {
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!volume_ok(d->volume_in) || !volume_ok(d->volume_out)) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->mask)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~CLWH_MASK_INVERT) != 0) return CLWH_ERR_INVALID_VALUE;
  if (d->fill < -32768 || d->fill > 32767) return CLWH_ERR_INVALID_VALUE;
  if (!dims_fit_int32(d->volume_in) || !dims_fit_int32(d->volume_out)) return CLWH_ERR_INVALID_VALUE;
  if (!same_dims(d->volume_in, d->volume_out)) return CLWH_ERR_SIZE_MISMATCH;
  const clwh_mem *in = d->volume_in;
  if (!mask_fits(in->dims[0], in->dims[1], in->dims[2], d->mask)) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(launch_apply_mask((const int16_t *)in->dptr, (int16_t *)d->volume_out->dptr, (const unsigned long long *)d->mask->dptr,
                            (int32_t)in->dims[0], (int32_t)in->dims[1], (int32_t)in->dims[2], (int32_t)mask_w64(in->dims[0]), d->fill,
                            (d->flags & CLWH_MASK_INVERT) != 0, ctx->stream));
  touch(d->volume_out);  // a rewrite: what any context derived from this pointer is rebuilt at its next use
  return CLWH_OK;
}
