// clwh_costpath.hip -- clwh_cost_geodesic, clwh_cost_trace and clwh_cost_from_field on the host: the argument checks in the header's
// order, the scratch (the geodesic's keys and worklist; the table's copy), and the rounds of the tiles' worklist.  The kernels are in
// costpath_kernels.hip; the finish kernel is the geodesic's.
#include <algorithm>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

static_assert(sizeof(clwh_cost_geodesic_desc) == 112 && sizeof(clwh_cost_trace_desc) == 104 && sizeof(clwh_cost_field_desc) == 72,
              "the descriptors as the Python binding lays them out");

// a cost field: a plain device buffer of 16-bit entries
static bool cost_ok(const clwh_mem *m) { return is_plain_buffer(m) && ((uintptr_t)m->dptr & 1u) == 0u; }
static bool mult_ok(uint32_t m) { return m >= 1u && m <= 255u; }
static bool mults_ok(const uint32_t *face, const uint32_t *edge, uint32_t corner, bool conn26) {
  for (int q = 0; q < 3; ++q)
    if (!mult_ok(face[q]) || (conn26 && !mult_ok(edge[q]))) return false;
  return !conn26 || mult_ok(corner);
}

constexpr int kGeoTile[3] = {kGeoTileX, kGeoTileY, kGeoTileZ};

extern "C" int clwh_cost_geodesic(clwh_ctx *ctx, const clwh_cost_geodesic_desc *d) {
  if (!ctx || !d || !d->result) return CLWH_ERR_INVALID_VALUE;
  if (!cost_ok(d->cost)) return CLWH_ERR_INVALID_VALUE;
  if (d->domain && !mask_ok(d->domain)) return CLWH_ERR_INVALID_VALUE;
  if (!d->dist && !d->labels) return CLWH_ERR_INVALID_VALUE;
  if ((d->dist && !words_ok(d->dist)) || (d->labels && !words_ok(d->labels))) return CLWH_ERR_INVALID_VALUE;
  const bool from_labels = (d->flags & CLWH_GEO_FROM_LABELS) != 0, conn26 = (d->flags & CLWH_GEO_26) != 0;
  if (from_labels && !words_ok(d->seed_labels)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_GEO_26 | CLWH_GEO_FROM_LABELS | CLWH_GEO_DENSE)) != 0) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  if (!mults_ok(d->mult_face, d->mult_edge, d->mult_corner, conn26)) return CLWH_ERR_INVALID_VALUE;
  if (d->cap > CLWH_COST_CAP_MAX && d->cap != CLWH_DIST_NONE) return CLWH_ERR_INVALID_VALUE;
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
  if ((d->dist && d->dist->bytes / 4u < voxels) || (d->labels && d->labels->bytes / 4u < voxels)) return CLWH_ERR_SIZE_MISMATCH;
  if (from_labels && d->seed_labels->bytes / 4u < voxels) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  const size_t TX = (d->dims[0] + kGeoTile[0] - 1u) / kGeoTile[0], TY = (d->dims[1] + kGeoTile[1] - 1u) / kGeoTile[1],
               TZ = (d->dims[2] + kGeoTile[2] - 1u) / kGeoTile[2];  // (TX * TY * TZ is below 2^31: a tile holds a voxel)

  // scratch: the geodesic's -- the keys; the tiles' worklist with the result behind it; the seeds
  GeodesicScratch &g = ctx->geodesic;
  CostArgs c;
  std::memset(&c, 0, sizeof c);
  GeoArgs &a = c.g;
  a.tiles.TX = (int32_t)TX;
  a.tiles.TY = (int32_t)TY;
  a.tiles.TZ = (int32_t)TZ;
  a.tiles.dense = (d->flags & CLWH_GEO_DENSE) != 0;
  CLWH_TRY(g.keys.reserve(ctx->stream, voxels * 8u));
  CLWH_TRY(tile_work_begin(ctx, g.work, a.tiles, (size_t)d->n_seeds * 16u, sizeof(GeoDeviceResult), (void **)&a.result));
  c.cost = (const uint16_t *)d->cost->dptr;
  a.domain = d->domain ? (const uint8_t *)d->domain->dptr : nullptr;
  a.seed_labels = from_labels ? (const uint32_t *)d->seed_labels->dptr : nullptr;
  a.keys = g.keys.as<unsigned long long>();
  a.dist = d->dist ? (uint32_t *)d->dist->dptr : nullptr;
  a.labels = d->labels ? (uint32_t *)d->labels->dptr : nullptr;
  a.X = (int32_t)d->dims[0];
  a.Y = (int32_t)d->dims[1];
  a.Z = (int32_t)d->dims[2];
  a.W64 = (int32_t)mask_w64(X);
  for (int q = 0; q < 3; ++q) {
    a.w_face[q] = d->mult_face[q];
    a.w_edge[q] = conn26 ? d->mult_edge[q] : 0u;
  }
  a.w_corner = conn26 ? d->mult_corner : 0u;
  a.cap = d->cap == CLWH_DIST_NONE ? CLWH_COST_CAP_MAX : d->cap;
  a.conn26 = conn26;
  a.seeds = g.work.seeds.as<uint32_t>();
  a.n_seeds = d->n_seeds;

  HIP_TRY(hipMemsetAsync(a.result, 0, sizeof(GeoDeviceResult), ctx->stream));
  if (d->n_seeds > 0) HIP_TRY(hipMemcpyAsync(g.work.seeds.ptr, d->seeds, (size_t)d->n_seeds * 16u, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(launch_cost_init(c, ctx->stream));

  // After round r every voxel with a shortest path that crosses fewer than r tile faces holds its final key, and a shortest path
  // visits no voxel twice, every step cost being positive: X * Y * Z + 2 rounds suffice.
  const uint64_t cap = std::min<uint64_t>((uint64_t)voxels + 2u, 0xFFFFFF00u);
  uint64_t rounds;
  CLWH_TRY(tile_work_run(ctx, g.work, a.tiles, cap, [&](uint32_t round, int slot) { return launch_cost_round(c, round, slot, ctx->stream); }, &rounds));

  HIP_TRY(launch_geo_finish(a, ctx->stream));  // the keys split into the maps: nothing there depends on the cost
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

extern "C" int clwh_cost_trace(clwh_ctx *ctx, const clwh_cost_trace_desc *d) {
  if (!ctx || !d || !d->n_points) return CLWH_ERR_INVALID_VALUE;
  if (!cost_ok(d->cost)) return CLWH_ERR_INVALID_VALUE;
  if (!words_ok(d->dist)) return CLWH_ERR_INVALID_VALUE;
  if (d->labels && !words_ok(d->labels)) return CLWH_ERR_INVALID_VALUE;
  if (d->points ? !words_ok(d->points) : d->capacity > 0) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~CLWH_GEO_26) != 0) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  const bool conn26 = (d->flags & CLWH_GEO_26) != 0;
  if (!mults_ok(d->mult_face, d->mult_edge, d->mult_corner, conn26)) return CLWH_ERR_INVALID_VALUE;
  for (int q = 0; q < 3; ++q)
    if (d->target[q] >= d->dims[q]) return CLWH_ERR_INVALID_VALUE;
  const size_t voxels = (size_t)(X * Y * Z);
  if (d->cost->bytes / 2u < voxels) return CLWH_ERR_SIZE_MISMATCH;
  if (d->dist->bytes / 4u < voxels || (d->labels && d->labels->bytes / 4u < voxels)) return CLWH_ERR_SIZE_MISMATCH;
  if (d->points && d->points->bytes / 12u < d->capacity) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  GeodesicScratch &g = ctx->geodesic;
  CLWH_TRY(g.trace.reserve(ctx->stream, sizeof(GeoTraceResult)));
  CLWH_TRY(g.work.host.ensure());
  CostTraceArgs c;
  std::memset(&c, 0, sizeof c);
  GeoTraceArgs &a = c.g;
  c.cost = (const uint16_t *)d->cost->dptr;
  a.dist = (const uint32_t *)d->dist->dptr;
  a.labels = d->labels ? (const uint32_t *)d->labels->dptr : nullptr;
  a.points = d->points ? (uint32_t *)d->points->dptr : nullptr;
  a.capacity = d->capacity;
  a.X = (int32_t)d->dims[0];
  a.Y = (int32_t)d->dims[1];
  a.Z = (int32_t)d->dims[2];
  for (int q = 0; q < 3; ++q) {
    a.target[q] = (int32_t)d->target[q];
    a.w_face[q] = d->mult_face[q];
    a.w_edge[q] = conn26 ? d->mult_edge[q] : 0u;
  }
  a.w_corner = conn26 ? d->mult_corner : 0u;
  a.conn26 = conn26;
  a.result = g.trace.as<GeoTraceResult>();
  HIP_TRY(launch_cost_trace(c, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.work.host.ptr, a.result, sizeof(GeoTraceResult), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  GeoTraceResult r;
  std::memcpy(&r, g.work.host.ptr, sizeof r);
  *d->n_points = r.n_points;
  return r.broken ? CLWH_ERR_INVALID_VALUE : CLWH_OK;
}

extern "C" int clwh_cost_from_field(clwh_ctx *ctx, const clwh_cost_field_desc *d) {
  if (!ctx || !d || !d->table) return CLWH_ERR_INVALID_VALUE;
  if (d->kind != CLWH_COST_SRC_U32 && d->kind != CLWH_COST_SRC_VALUE && d->kind != CLWH_COST_SRC_GRADIENT) return CLWH_ERR_INVALID_VALUE;
  const bool from_words = d->kind == CLWH_COST_SRC_U32;
  if (from_words ? !words_ok(d->source) : !volume_ok(d->source)) return CLWH_ERR_INVALID_VALUE;
  if (!cost_ok(d->cost)) return CLWH_ERR_INVALID_VALUE;
  if (d->domain && !mask_ok(d->domain)) return CLWH_ERR_INVALID_VALUE;
  if (d->flags != 0) return CLWH_ERR_INVALID_VALUE;
  if (d->n < 1u || d->n > 65536u || d->shift > 40u) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  if (!from_words && (d->source->dims[0] != X || d->source->dims[1] != Y || d->source->dims[2] != Z)) return CLWH_ERR_INVALID_VALUE;
  const size_t voxels = (size_t)(X * Y * Z);
  if (from_words && d->source->bytes / 4u < voxels) return CLWH_ERR_SIZE_MISMATCH;
  if (d->cost->bytes / 2u < voxels) return CLWH_ERR_SIZE_MISMATCH;
  if (d->domain && !mask_fits(X, Y, Z, d->domain)) return CLWH_ERR_SIZE_MISMATCH;

  HIP_TRY(hipSetDevice(ctx->device));
  CostScratch &s = ctx->cost;
  constexpr size_t kTableBytes = 65536u * sizeof(uint16_t);
  CLWH_TRY(s.table.reserve(ctx->stream, kTableBytes));
  if (!s.host) HIP_TRY(hipHostMalloc((void **)&s.host, kTableBytes, hipHostMallocDefault));
  CLWH_TRY(s.copied.ensure(hipEventDisableTiming));
  if (s.in_flight) HIP_TRY(hipEventSynchronize(s.copied.ev));  // the previous call's copy has left the page-locked table
  s.in_flight = false;
  std::memcpy(s.host, d->table, (size_t)d->n * sizeof(uint16_t));
  HIP_TRY(hipMemcpyAsync(s.table.ptr, s.host, (size_t)d->n * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipEventRecord(s.copied.ev, ctx->stream));
  s.in_flight = true;

  CostFieldArgs a;
  std::memset(&a, 0, sizeof a);
  a.words = from_words ? (const uint32_t *)d->source->dptr : nullptr;
  a.volume = from_words ? nullptr : (const int16_t *)d->source->dptr;
  a.domain = d->domain ? (const uint8_t *)d->domain->dptr : nullptr;
  a.table = s.table.as<uint16_t>();
  a.cost = (uint16_t *)d->cost->dptr;
  a.lo = (long long)d->lo;
  a.X = (int32_t)d->dims[0];
  a.Y = (int32_t)d->dims[1];
  a.Z = (int32_t)d->dims[2];
  a.W64 = (int32_t)mask_w64(X);
  a.n = d->n;
  a.shift = d->shift;
  a.kind = d->kind;
  HIP_TRY(launch_cost_field(a, ctx->stream));
  return CLWH_OK;
}
