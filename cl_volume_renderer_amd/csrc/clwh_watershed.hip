// clwh_watershed.hip -- clwh_watershed on the host: the argument checks in the header's order, the scratch (the geodesic's keys as two
// uint32 arrays, its worklist with a second set of stamps behind the result) and the rounds of the two phases.  The kernels are in
// watershed_kernels.hip.
#include <algorithm>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

static_assert(sizeof(clwh_watershed_desc) == 88 && sizeof(clwh_watershed_result) == 16, "the descriptor as the Python binding lays it out");

// a cost field: a plain device buffer of 16-bit entries
static bool cost_ok(const clwh_mem *m) { return is_plain_buffer(m) && ((uintptr_t)m->dptr & 1u) == 0u; }

constexpr int kGeoTile[3] = {kGeoTileX, kGeoTileY, kGeoTileZ};

extern "C" int clwh_watershed(clwh_ctx *ctx, const clwh_watershed_desc *d) {
  if (!ctx || !d || !d->result) return CLWH_ERR_INVALID_VALUE;
  if (!cost_ok(d->cost)) return CLWH_ERR_INVALID_VALUE;
  if (d->domain && !mask_ok(d->domain)) return CLWH_ERR_INVALID_VALUE;
  if (!d->level && !d->labels) return CLWH_ERR_INVALID_VALUE;
  if ((d->level && !words_ok(d->level)) || (d->labels && !words_ok(d->labels))) return CLWH_ERR_INVALID_VALUE;
  const bool from_labels = (d->flags & CLWH_GEO_FROM_LABELS) != 0, conn26 = (d->flags & CLWH_GEO_26) != 0;
  if (from_labels && !words_ok(d->seed_labels)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_GEO_26 | CLWH_GEO_FROM_LABELS | CLWH_GEO_DENSE)) != 0) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  if (d->plateau_cap > CLWH_WATERSHED_PLATEAU_MAX) return CLWH_ERR_INVALID_VALUE;
  if (d->level_cap > CLWH_WATERSHED_LEVEL_MAX) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds > CLWH_GROW_MAX_SEEDS || (d->n_seeds > 0 && !d->seeds)) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds == 0 && !from_labels) return CLWH_ERR_INVALID_VALUE;
  for (uint32_t i = 0; i < d->n_seeds; ++i) {
    for (int q = 0; q < 3; ++q)
      if (d->seeds[4u * i + (uint32_t)q] >= d->dims[q]) return CLWH_ERR_INVALID_VALUE;
    if (d->seeds[4u * i + 3u] == 0u) return CLWH_ERR_INVALID_VALUE;
  }
  const size_t voxels = (size_t)(X * Y * Z);
  if (d->cost->bytes / 2u < voxels) return CLWH_ERR_SIZE_MISMATCH;
  if (d->domain && !mask_fits(X, Y, Z, d->domain)) return CLWH_ERR_SIZE_MISMATCH;
  if ((d->level && d->level->bytes / 4u < voxels) || (d->labels && d->labels->bytes / 4u < voxels)) return CLWH_ERR_SIZE_MISMATCH;
  if (from_labels && d->seed_labels->bytes / 4u < voxels) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  const size_t TX = (d->dims[0] + kGeoTile[0] - 1u) / kGeoTile[0], TY = (d->dims[1] + kGeoTile[1] - 1u) / kGeoTile[1],
               TZ = (d->dims[2] + kGeoTile[2] - 1u) / kGeoTile[2];  // (TX * TY * TZ is below 2^31: a tile holds a voxel)

  // scratch: the geodesic's -- the keys' 8 bytes per voxel as the states and the working labels; the tiles' worklist with the result and
  // phase 2's stamps behind it; the seeds
  GeodesicScratch &g = ctx->geodesic;
  WsArgs a;
  std::memset(&a, 0, sizeof a);
  a.tiles.TX = (int32_t)TX;
  a.tiles.TY = (int32_t)TY;
  a.tiles.TZ = (int32_t)TZ;
  a.tiles.dense = (d->flags & CLWH_GEO_DENSE) != 0;
  const size_t tile_words = (TX * TY * TZ + 15u) & ~(size_t)15u;
  CLWH_TRY(g.keys.reserve(ctx->stream, voxels * 8u));
  CLWH_TRY(tile_work_begin(ctx, g.work, a.tiles, (size_t)d->n_seeds * 16u, sizeof(WsDeviceResult) + tile_words * sizeof(uint32_t), (void **)&a.result));
  a.stamps_level = a.tiles.stamps;
  a.stamps_label = (uint32_t *)(a.result + 1);
  a.cost = (const uint16_t *)d->cost->dptr;
  a.domain = d->domain ? (const uint8_t *)d->domain->dptr : nullptr;
  a.seed_labels = from_labels ? (const uint32_t *)d->seed_labels->dptr : nullptr;
  a.state = g.keys.as<uint32_t>();
  a.wlab = a.state + voxels;
  a.level = d->level ? (uint32_t *)d->level->dptr : nullptr;
  a.labels = d->labels ? (uint32_t *)d->labels->dptr : nullptr;
  a.X = (int32_t)d->dims[0];
  a.Y = (int32_t)d->dims[1];
  a.Z = (int32_t)d->dims[2];
  a.W64 = (int32_t)mask_w64(X);
  a.plateau_cap = d->plateau_cap;
  a.level_cap = d->level_cap;
  a.conn26 = conn26;
  a.seeds = g.work.seeds.as<uint32_t>();
  a.n_seeds = d->n_seeds;

  HIP_TRY(hipMemsetAsync(a.result, 0, sizeof(WsDeviceResult) + tile_words * sizeof(uint32_t), ctx->stream));
  if (d->n_seeds > 0) HIP_TRY(hipMemcpyAsync(g.work.seeds.ptr, d->seeds, (size_t)d->n_seeds * 16u, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(launch_ws_init(a, ctx->stream));

  // Per phase the geodesic's bound: what a voxel's answer rests on (a path that attains its state; a chain of edges from its seed) can be
  // taken to visit no voxel twice, so it crosses fewer tile faces than the volume has voxels: X * Y * Z + 2 rounds suffice.
  const uint64_t cap = std::min<uint64_t>((uint64_t)voxels + 2u, 0xFFFFFF00u);
  uint64_t rounds_level, rounds_label = 0;
  CLWH_TRY(tile_work_run(ctx, g.work, a.tiles, cap, [&](uint32_t round, int slot) { return launch_ws_level_round(a, round, slot, ctx->stream); }, &rounds_level));
  if (a.labels) {  // every state is final: the labels, from the seeds' tiles again (nobody asked: the levels need no phase 2)
    a.tiles.stamps = a.stamps_label;
    CLWH_TRY(tile_work_run(ctx, g.work, a.tiles, cap, [&](uint32_t round, int slot) { return launch_ws_label_round(a, round, slot, ctx->stream); }, &rounds_label));
  }

  HIP_TRY(launch_ws_finish(a, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.work.host.ptr, a.result, sizeof(WsDeviceResult), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous by contract: the maps are written when the call returns
  WsDeviceResult r;
  std::memcpy(&r, g.work.host.ptr, sizeof r);
  clwh_watershed_result out;
  out.reached = r.reached;
  out.max_level = r.max_level;
  out.rounds = (uint32_t)(rounds_level + rounds_label);
  *d->result = out;
  return CLWH_OK;
}
