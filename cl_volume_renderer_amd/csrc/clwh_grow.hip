// clwh_grow.hip -- clwh_segment_grow and clwh_volume_apply_mask on the host: the argument checks in the header's order, the scratch, and
// the loop that enqueues rounds until a round lists no tile.  The kernels are in grow_kernels.hip.
#include <algorithm>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

// a mask handle the kernels can use: a plain device buffer whose rows are aligned 64-bit words
static bool mask_ok(const clwh_mem *m) { return is_plain_buffer(m) && ((uintptr_t)m->dptr & 7u) == 0u; }
static bool volume_ok(const clwh_mem *m) {
  return is_image(m, 3, 1, CLWH_ELEM_S16) && m->dptr && m->dims[0] != 0 && m->dims[1] != 0 && m->dims[2] != 0;
}
// 64-bit words per row; whether the buffer holds the whole mask (dims below 2^31 each; compared by division: the product may not fit)
static size_t mask_w64(const clwh_mem *volume) { return (volume->dims[0] + 63u) / 64u; }
static bool mask_fits(const clwh_mem *volume, const clwh_mem *mask) {
  return mask->bytes / (mask_w64(volume) * 8u) >= volume->dims[1] * volume->dims[2];
}

extern "C" int clwh_segment_grow(clwh_ctx *ctx, const clwh_grow_desc *d) {
  if (!ctx || !d || !d->result) return CLWH_ERR_INVALID_VALUE;
  if (!volume_ok(d->volume)) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->mask)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_GROW_26 | CLWH_GROW_FROM_MASK | CLWH_GROW_DENSE)) != 0) return CLWH_ERR_INVALID_VALUE;
  if (!(d->lo >= -32768 && d->lo <= d->hi && d->hi <= 32767)) return CLWH_ERR_INVALID_VALUE;
  const clwh_mem *vol = d->volume;
  const bool whole = (d->box_hi[0] | d->box_hi[1] | d->box_hi[2]) == 0u;
  uint64_t lo[3], hi[3];
  for (int q = 0; q < 3; ++q) {
    lo[q] = d->box_lo[q];
    hi[q] = whole ? (uint64_t)vol->dims[q] : (uint64_t)d->box_hi[q];
    if (!(lo[q] <= hi[q] && hi[q] <= (uint64_t)vol->dims[q])) return CLWH_ERR_INVALID_VALUE;
  }
  if (d->n_seeds > CLWH_GROW_MAX_SEEDS || (d->n_seeds > 0 && !d->seeds)) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds == 0 && !(d->flags & CLWH_GROW_FROM_MASK)) return CLWH_ERR_INVALID_VALUE;
  for (uint32_t i = 0; i < d->n_seeds; ++i)
    for (int q = 0; q < 3; ++q)
      if ((uint64_t)d->seeds[3u * i + (uint32_t)q] >= (uint64_t)vol->dims[q]) return CLWH_ERR_INVALID_VALUE;
  if (!dims_fit_int32(vol)) return CLWH_ERR_INVALID_VALUE;
  const size_t W64 = mask_w64(vol), TX = W64, TY = (vol->dims[1] + 15u) / 16u, TZ = (vol->dims[2] + 15u) / 16u;
  if (TY * TZ > 0x7FFFFFFFu / TX) return CLWH_ERR_INVALID_VALUE;  // tiles are numbered in 32 bits
  if (!mask_fits(vol, d->mask)) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  const size_t mask_bytes = W64 * 8u * vol->dims[1] * vol->dims[2], n_tiles = TX * TY * TZ;
  clwh_grow_result out;
  std::memset(&out, 0, sizeof out);
  if (lo[0] == hi[0] || lo[1] == hi[1] || lo[2] == hi[2]) {  // nothing is admissible: the empty set
    HIP_TRY(hipMemsetAsync(d->mask->dptr, 0, mask_bytes, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *d->result = out;
    return CLWH_OK;
  }

  // scratch: A; stamps | list | counters | result (the counters on a 64-byte line of their own); the seeds
  GrowScratch &g = ctx->grow;
  const size_t tile_words = (n_tiles + 15u) & ~(size_t)15u;
  CLWH_TRY(g.admissible.reserve(ctx->stream, mask_bytes));
  CLWH_TRY(g.tiles.reserve(ctx->stream, (2u * tile_words + 2u * (size_t)kGrowBatch) * sizeof(uint32_t) + sizeof(GrowDeviceResult)));
  CLWH_TRY(g.seeds.reserve(ctx->stream, std::max<size_t>((size_t)d->n_seeds * 12u, 16u)));
  CLWH_TRY(g.host.ensure());

  GrowArgs a;
  std::memset(&a, 0, sizeof a);
  a.volume = (const int16_t *)vol->dptr;
  a.mask = (unsigned long long *)d->mask->dptr;
  a.adm = g.admissible.as<unsigned long long>();
  a.X = (int32_t)vol->dims[0];
  a.Y = (int32_t)vol->dims[1];
  a.Z = (int32_t)vol->dims[2];
  a.W64 = (int32_t)W64;
  a.TX = (int32_t)TX;
  a.TY = (int32_t)TY;
  a.TZ = (int32_t)TZ;
  a.lo = d->lo;
  a.hi = d->hi;
  for (int q = 0; q < 3; ++q) {
    a.box_lo[q] = (int32_t)lo[q];
    a.box_hi[q] = (int32_t)hi[q];
  }
  a.conn26 = (d->flags & CLWH_GROW_26) != 0;
  a.from_mask = (d->flags & CLWH_GROW_FROM_MASK) != 0;
  a.dense = (d->flags & CLWH_GROW_DENSE) != 0;
  a.stamps = g.tiles.as<uint32_t>();
  a.list = a.stamps + tile_words;
  a.counters = a.list + tile_words;
  a.result = reinterpret_cast<GrowDeviceResult *>(a.counters + 2 * kGrowBatch);
  a.seeds = g.seeds.as<uint32_t>();
  a.n_seeds = d->n_seeds;

  GrowDeviceResult start;
  std::memset(&start, 0, sizeof start);
  start.vmin = INT32_MAX;
  start.vmax = INT32_MIN;
  start.lo[0] = start.lo[1] = start.lo[2] = 0xFFFFFFFFu;
  HIP_TRY(hipMemsetAsync(a.stamps, 0, tile_words * sizeof(uint32_t), ctx->stream));
  HIP_TRY(hipMemcpyAsync(a.result, &start, sizeof start, hipMemcpyHostToDevice, ctx->stream));
  if (d->n_seeds > 0) HIP_TRY(hipMemcpyAsync(g.seeds.ptr, d->seeds, (size_t)d->n_seeds * 12u, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(launch_grow_admissible(a, ctx->stream));
  HIP_TRY(launch_grow_seeds(a, ctx->stream));

  // Rounds, eight to a batch: the pinned line holds eight {listed, ticket} pairs, and a batch that turns out to be longer than the
  // search costs its empty rounds one word read per block.  Every round that lists a tile sets a bit or leaves the next list empty, so
  // at most count + 2 rounds list one; the cap only keeps a defect from spinning.
  // (X * Y * Z fits: the mask, one bit per voxel, fits the buffer)
  const uint64_t cap = std::min<uint64_t>((uint64_t)vol->dims[0] * vol->dims[1] * vol->dims[2] + 2u, 0xFFFFFF00u);
  uint64_t rounds = 0;
  for (uint32_t round = 1;; round += (uint32_t)kGrowBatch) {
    HIP_TRY(hipMemsetAsync(a.counters, 0, 2u * (size_t)kGrowBatch * sizeof(uint32_t), ctx->stream));
    for (int slot = 0; slot < kGrowBatch; ++slot) HIP_TRY(launch_grow_round(a, round + (uint32_t)slot, slot, ctx->stream));
    HIP_TRY(hipMemcpyAsync(g.host.ptr, a.counters, 2u * (size_t)kGrowBatch * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int slot = 0; slot < kGrowBatch; ++slot) rounds += g.host.ptr[2 * slot] != 0u;
    if (g.host.ptr[2 * (kGrowBatch - 1)] == 0u) break;  // the batch's last round listed nothing: converged
    if (rounds >= cap) return CLWH_ERR_INTERNAL_OVERFLOW;
  }

  HIP_TRY(launch_grow_reduce(a, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.host.ptr, a.result, sizeof(GrowDeviceResult), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous by contract: the mask is written when the call returns
  GrowDeviceResult r;
  std::memcpy(&r, g.host.ptr, sizeof r);
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
  if (!mask_fits(d->volume_in, d->mask)) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  const clwh_mem *in = d->volume_in;
  HIP_TRY(launch_apply_mask((const int16_t *)in->dptr, (int16_t *)d->volume_out->dptr, (const unsigned long long *)d->mask->dptr,
                            (int32_t)in->dims[0], (int32_t)in->dims[1], (int32_t)in->dims[2], (int32_t)mask_w64(in), d->fill,
                            (d->flags & CLWH_MASK_INVERT) != 0, ctx->stream));
  touch(d->volume_out);  // a rewrite: what any context derived from this pointer is rebuilt at its next use
  return CLWH_OK;
}
