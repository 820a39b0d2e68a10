// clwh_geodesic.hip -- clwh_mask_geodesic and clwh_geodesic_trace on the host: the argument checks in the header's order, the scratch,
// and the loop that enqueues rounds until a round lists no tile (clwh_grow.hip's).  The kernels are in geodesic_kernels.hip.
#include <algorithm>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

static_assert(sizeof(clwh_geodesic_desc) == 104 && sizeof(clwh_geodesic_trace_desc) == 96 && sizeof(clwh_geodesic_result) == 16,
              "the descriptors as the Python binding lays them out");

// grow's rules for a mask and its size, label's for a buffer of words and for the dims (clwh_grow.hip, clwh_label.hip)
static bool mask_ok(const clwh_mem *m) { return is_plain_buffer(m) && ((uintptr_t)m->dptr & 7u) == 0u; }
static bool words_ok(const clwh_mem *m) { return is_plain_buffer(m) && ((uintptr_t)m->dptr & 3u) == 0u; }
static bool dims_ok(const uint32_t *dims) {
  const uint64_t X = dims[0], Y = dims[1], Z = dims[2];
  if (X == 0 || Y == 0 || Z == 0 || X > 0x7FFFFFFFu || Y > 0x7FFFFFFFu || Z > 0x7FFFFFFFu) return false;
  return X * Y <= 0x7FFFFFFFull && Z <= 0x7FFFFFFFull / (X * Y);  // X * Y * Z <= 2^31 - 1, by division: the product may not fit
}
static bool mask_fits(const uint32_t *dims, const clwh_mem *mask) {
  return mask->bytes / ((((uint64_t)dims[0] + 63u) / 64u) * 8u) >= (uint64_t)dims[1] * dims[2];
}
static bool weight_ok(uint32_t w) { return w >= 1u && w <= 65535u; }
static bool weights_ok(const uint32_t *face, const uint32_t *edge, uint32_t corner, bool conn26) {
  for (int q = 0; q < 3; ++q)
    if (!weight_ok(face[q]) || (conn26 && !weight_ok(edge[q]))) return false;
  return !conn26 || weight_ok(corner);
}

constexpr int kGeoTile[3] = {kGeoTileX, kGeoTileY, kGeoTileZ};

extern "C" int clwh_mask_geodesic(clwh_ctx *ctx, const clwh_geodesic_desc *d) {
  if (!ctx || !d || !d->result) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->domain)) return CLWH_ERR_INVALID_VALUE;
  if (!d->dist && !d->labels) return CLWH_ERR_INVALID_VALUE;
  if ((d->dist && !words_ok(d->dist)) || (d->labels && !words_ok(d->labels))) return CLWH_ERR_INVALID_VALUE;
  const bool from_labels = (d->flags & CLWH_GEO_FROM_LABELS) != 0, conn26 = (d->flags & CLWH_GEO_26) != 0;
  if (from_labels && !words_ok(d->seed_labels)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_GEO_26 | CLWH_GEO_FROM_LABELS | CLWH_GEO_DENSE)) != 0) return CLWH_ERR_INVALID_VALUE;
  if (!dims_ok(d->dims)) return CLWH_ERR_INVALID_VALUE;
  if (!weights_ok(d->weight_face, d->weight_edge, d->weight_corner, conn26)) return CLWH_ERR_INVALID_VALUE;
  if (d->cap > CLWH_GEO_CAP_MAX && d->cap != CLWH_DIST_NONE) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds > CLWH_GROW_MAX_SEEDS || (d->n_seeds > 0 && !d->seeds)) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds == 0 && !from_labels) return CLWH_ERR_INVALID_VALUE;
  for (uint32_t i = 0; i < d->n_seeds; ++i) {
    for (int q = 0; q < 3; ++q)
      if (d->seeds[4u * i + (uint32_t)q] >= d->dims[q]) return CLWH_ERR_INVALID_VALUE;
    if (d->seeds[4u * i + 3u] == 0u) return CLWH_ERR_INVALID_VALUE;
  }
  const size_t voxels = (size_t)d->dims[0] * d->dims[1] * d->dims[2];
  if (!mask_fits(d->dims, d->domain)) return CLWH_ERR_SIZE_MISMATCH;
  if ((d->dist && d->dist->bytes / 4u < voxels) || (d->labels && d->labels->bytes / 4u < voxels)) return CLWH_ERR_SIZE_MISMATCH;
  if (from_labels && d->seed_labels->bytes / 4u < voxels) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  const size_t TX = (d->dims[0] + kGeoTile[0] - 1u) / kGeoTile[0], TY = (d->dims[1] + kGeoTile[1] - 1u) / kGeoTile[1],
               TZ = (d->dims[2] + kGeoTile[2] - 1u) / kGeoTile[2], n_tiles = TX * TY * TZ;  // (below 2^31: a tile holds a voxel)

  // scratch: the keys; stamps | list | counters | result (the counters on a 64-byte line of their own); the seeds
  GeodesicScratch &g = ctx->geodesic;
  const size_t tile_words = (n_tiles + 15u) & ~(size_t)15u;
  CLWH_TRY(g.keys.reserve(ctx->stream, voxels * 8u));
  CLWH_TRY(g.tiles.reserve(ctx->stream, (2u * tile_words + 2u * (size_t)kGrowBatch) * sizeof(uint32_t) + sizeof(GeoDeviceResult)));
  CLWH_TRY(g.seeds.reserve(ctx->stream, std::max<size_t>((size_t)d->n_seeds * 16u, 16u)));
  CLWH_TRY(g.host.ensure());

  GeoArgs a;
  std::memset(&a, 0, sizeof a);
  a.domain = (const uint8_t *)d->domain->dptr;
  a.seed_labels = from_labels ? (const uint32_t *)d->seed_labels->dptr : nullptr;
  a.keys = g.keys.as<unsigned long long>();
  a.dist = d->dist ? (uint32_t *)d->dist->dptr : nullptr;
  a.labels = d->labels ? (uint32_t *)d->labels->dptr : nullptr;
  a.X = (int32_t)d->dims[0];
  a.Y = (int32_t)d->dims[1];
  a.Z = (int32_t)d->dims[2];
  a.W64 = (int32_t)((d->dims[0] + 63u) / 64u);
  a.TX = (int32_t)TX;
  a.TY = (int32_t)TY;
  a.TZ = (int32_t)TZ;
  for (int q = 0; q < 3; ++q) {
    a.w_face[q] = d->weight_face[q];
    a.w_edge[q] = d->weight_edge[q];
  }
  a.w_corner = d->weight_corner;
  a.cap = d->cap == CLWH_DIST_NONE ? CLWH_GEO_CAP_MAX : d->cap;
  a.conn26 = conn26;
  a.dense = (d->flags & CLWH_GEO_DENSE) != 0;
  a.stamps = g.tiles.as<uint32_t>();
  a.list = a.stamps + tile_words;
  a.counters = a.list + tile_words;
  a.result = reinterpret_cast<GeoDeviceResult *>(a.counters + 2 * kGrowBatch);
  a.seeds = g.seeds.as<uint32_t>();
  a.n_seeds = d->n_seeds;

  HIP_TRY(hipMemsetAsync(a.stamps, 0, tile_words * sizeof(uint32_t), ctx->stream));
  HIP_TRY(hipMemsetAsync(a.result, 0, sizeof(GeoDeviceResult), ctx->stream));
  if (d->n_seeds > 0) HIP_TRY(hipMemcpyAsync(g.seeds.ptr, d->seeds, (size_t)d->n_seeds * 16u, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(launch_geo_init(a, ctx->stream));

  // Rounds, eight to a batch, as in clwh_segment_grow.  After round r every voxel with a shortest path that crosses fewer than r tile
  // faces holds its final key, and a shortest path visits no voxel twice: X * Y * Z + 2 rounds suffice, the cap only keeps a defect
  // from spinning.
  const uint64_t cap = std::min<uint64_t>((uint64_t)voxels + 2u, 0xFFFFFF00u);
  uint64_t rounds = 0;
  for (uint32_t round = 1;; round += (uint32_t)kGrowBatch) {
    HIP_TRY(hipMemsetAsync(a.counters, 0, 2u * (size_t)kGrowBatch * sizeof(uint32_t), ctx->stream));
    for (int slot = 0; slot < kGrowBatch; ++slot) HIP_TRY(launch_geo_round(a, round + (uint32_t)slot, slot, ctx->stream));
    HIP_TRY(hipMemcpyAsync(g.host.ptr, a.counters, 2u * (size_t)kGrowBatch * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int slot = 0; slot < kGrowBatch; ++slot) rounds += g.host.ptr[2 * slot] != 0u;
    if (g.host.ptr[2 * (kGrowBatch - 1)] == 0u) break;  // the batch's last round listed nothing: converged
    if (rounds >= cap) return CLWH_ERR_INTERNAL_OVERFLOW;
  }

  HIP_TRY(launch_geo_finish(a, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.host.ptr, a.result, sizeof(GeoDeviceResult), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous by contract: the maps are written when the call returns
  GeoDeviceResult r;
  std::memcpy(&r, g.host.ptr, sizeof r);
  clwh_geodesic_result out;
  out.reached = r.reached;
  out.max_dist = r.max_dist;
  out.rounds = (uint32_t)rounds;
  *d->result = out;
  return CLWH_OK;
}

extern "C" int clwh_geodesic_trace(clwh_ctx *ctx, const clwh_geodesic_trace_desc *d) {
  if (!ctx || !d || !d->n_points) return CLWH_ERR_INVALID_VALUE;
  if (!words_ok(d->dist)) return CLWH_ERR_INVALID_VALUE;
  if (d->labels && !words_ok(d->labels)) return CLWH_ERR_INVALID_VALUE;
  if (d->points ? !words_ok(d->points) : d->capacity > 0) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~CLWH_GEO_26) != 0) return CLWH_ERR_INVALID_VALUE;
  if (!dims_ok(d->dims)) return CLWH_ERR_INVALID_VALUE;
  const bool conn26 = (d->flags & CLWH_GEO_26) != 0;
  if (!weights_ok(d->weight_face, d->weight_edge, d->weight_corner, conn26)) return CLWH_ERR_INVALID_VALUE;
  for (int q = 0; q < 3; ++q)
    if (d->target[q] >= d->dims[q]) return CLWH_ERR_INVALID_VALUE;
  const size_t voxels = (size_t)d->dims[0] * d->dims[1] * d->dims[2];
  if (d->dist->bytes / 4u < voxels || (d->labels && d->labels->bytes / 4u < voxels)) return CLWH_ERR_SIZE_MISMATCH;
  if (d->points && d->points->bytes / 12u < d->capacity) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  GeodesicScratch &g = ctx->geodesic;
  CLWH_TRY(g.trace.reserve(ctx->stream, sizeof(GeoTraceResult)));
  CLWH_TRY(g.host.ensure());
  GeoTraceArgs a;
  std::memset(&a, 0, sizeof a);
  a.dist = (const uint32_t *)d->dist->dptr;
  a.labels = d->labels ? (const uint32_t *)d->labels->dptr : nullptr;
  a.points = d->points ? (uint32_t *)d->points->dptr : nullptr;
  a.capacity = d->capacity;
  a.X = (int32_t)d->dims[0];
  a.Y = (int32_t)d->dims[1];
  a.Z = (int32_t)d->dims[2];
  for (int q = 0; q < 3; ++q) {
    a.target[q] = (int32_t)d->target[q];
    a.w_face[q] = d->weight_face[q];
    a.w_edge[q] = d->weight_edge[q];
  }
  a.w_corner = d->weight_corner;
  a.conn26 = conn26;
  a.result = g.trace.as<GeoTraceResult>();
  HIP_TRY(launch_geo_trace(a, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.host.ptr, a.result, sizeof(GeoTraceResult), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  GeoTraceResult r;
  std::memcpy(&r, g.host.ptr, sizeof r);
  *d->n_points = r.n_points;
  return r.broken ? CLWH_ERR_INVALID_VALUE : CLWH_OK;
}
