// clwh_geodesic.hip -- clwh_mask_geodesic and clwh_geodesic_trace on the host: the argument checks in the header's order, the scratch,
// and the rounds of the tiles' worklist.  The kernels are in geodesic_kernels.hip.
#include <algorithm>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

static_assert(sizeof(clwh_geodesic_desc) == 104 && sizeof(clwh_geodesic_trace_desc) == 96 && sizeof(clwh_geodesic_result) == 16,
              "the descriptors as the Python binding lays them out");

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
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  if (!weights_ok(d->weight_face, d->weight_edge, d->weight_corner, conn26)) return CLWH_ERR_INVALID_VALUE;
  if (d->cap > CLWH_GEO_CAP_MAX && d->cap != CLWH_DIST_NONE) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds > CLWH_GROW_MAX_SEEDS || (d->n_seeds > 0 && !d->seeds)) return CLWH_ERR_INVALID_VALUE;
  if (d->n_seeds == 0 && !from_labels) return CLWH_ERR_INVALID_VALUE;
  for (uint32_t i = 0; i < d->n_seeds; ++i) {
    for (int q = 0; q < 3; ++q)
      if (d->seeds[4u * i + (uint32_t)q] >= d->dims[q]) return CLWH_ERR_INVALID_VALUE;
    if (d->seeds[4u * i + 3u] == 0u) return CLWH_ERR_INVALID_VALUE;
  }
  const size_t voxels = (size_t)(X * Y * Z);
  if (!mask_fits(X, Y, Z, d->domain)) return CLWH_ERR_SIZE_MISMATCH;
  if ((d->dist && d->dist->bytes / 4u < voxels) || (d->labels && d->labels->bytes / 4u < voxels)) return CLWH_ERR_SIZE_MISMATCH;
  if (from_labels && d->seed_labels->bytes / 4u < voxels) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  const size_t TX = (d->dims[0] + kGeoTile[0] - 1u) / kGeoTile[0], TY = (d->dims[1] + kGeoTile[1] - 1u) / kGeoTile[1],
               TZ = (d->dims[2] + kGeoTile[2] - 1u) / kGeoTile[2];  // (TX * TY * TZ is below 2^31: a tile holds a voxel)

  // scratch: the keys; the tiles' worklist with the result behind it; the seeds
  GeodesicScratch &g = ctx->geodesic;
  GeoArgs a;
  std::memset(&a, 0, sizeof a);
  a.tiles.TX = (int32_t)TX;
  a.tiles.TY = (int32_t)TY;
  a.tiles.TZ = (int32_t)TZ;
  a.tiles.dense = (d->flags & CLWH_GEO_DENSE) != 0;
  CLWH_TRY(g.keys.reserve(ctx->stream, voxels * 8u));
  CLWH_TRY(tile_work_begin(ctx, g.work, a.tiles, (size_t)d->n_seeds * 16u, sizeof(GeoDeviceResult), (void **)&a.result));
  a.domain = (const uint8_t *)d->domain->dptr;
  a.seed_labels = from_labels ? (const uint32_t *)d->seed_labels->dptr : nullptr;
  a.keys = g.keys.as<unsigned long long>();
  a.dist = d->dist ? (uint32_t *)d->dist->dptr : nullptr;
  a.labels = d->labels ? (uint32_t *)d->labels->dptr : nullptr;
  a.X = (int32_t)d->dims[0];
  a.Y = (int32_t)d->dims[1];
  a.Z = (int32_t)d->dims[2];
  a.W64 = (int32_t)mask_w64(X);
  for (int q = 0; q < 3; ++q) {
    a.w_face[q] = d->weight_face[q];
    a.w_edge[q] = d->weight_edge[q];
  }
  a.w_corner = d->weight_corner;
  a.cap = d->cap == CLWH_DIST_NONE ? CLWH_GEO_CAP_MAX : d->cap;
  a.conn26 = conn26;
  a.seeds = g.work.seeds.as<uint32_t>();
  a.n_seeds = d->n_seeds;

  HIP_TRY(hipMemsetAsync(a.result, 0, sizeof(GeoDeviceResult), ctx->stream));
  if (d->n_seeds > 0) HIP_TRY(hipMemcpyAsync(g.work.seeds.ptr, d->seeds, (size_t)d->n_seeds * 16u, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(launch_geo_init(a, ctx->stream));

  // After round r every voxel with a shortest path that crosses fewer than r tile faces holds its final key, and a shortest path
  // visits no voxel twice: X * Y * Z + 2 rounds suffice.
  const uint64_t cap = std::min<uint64_t>((uint64_t)voxels + 2u, 0xFFFFFF00u);
  uint64_t rounds;
  CLWH_TRY(tile_work_run(ctx, g.work, a.tiles, cap, [&](uint32_t round, int slot) { return launch_geo_round(a, round, slot, ctx->stream); }, &rounds));

  HIP_TRY(launch_geo_finish(a, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.work.host.ptr, a.result, sizeof(GeoDeviceResult), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous by contract: the maps are written when the call returns
  GeoDeviceResult r;
  std::memcpy(&r, g.work.host.ptr, sizeof r);
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
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  const bool conn26 = (d->flags & CLWH_GEO_26) != 0;
  if (!weights_ok(d->weight_face, d->weight_edge, d->weight_corner, conn26)) return CLWH_ERR_INVALID_VALUE;
  for (int q = 0; q < 3; ++q)
    if (d->target[q] >= d->dims[q]) return CLWH_ERR_INVALID_VALUE;
  const size_t voxels = (size_t)(X * Y * Z);
  if (d->dist->bytes / 4u < voxels || (d->labels && d->labels->bytes / 4u < voxels)) return CLWH_ERR_SIZE_MISMATCH;
  if (d->points && d->points->bytes / 12u < d->capacity) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  GeodesicScratch &g = ctx->geodesic;
  CLWH_TRY(g.trace.reserve(ctx->stream, sizeof(GeoTraceResult)));
  CLWH_TRY(g.work.host.ensure());
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
  HIP_TRY(hipMemcpyAsync(g.work.host.ptr, a.result, sizeof(GeoTraceResult), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  GeoTraceResult r;
  std::memcpy(&r, g.work.host.ptr, sizeof r);
  *d->n_points = r.n_points;
  return r.broken ? CLWH_ERR_INVALID_VALUE : CLWH_OK;
}
