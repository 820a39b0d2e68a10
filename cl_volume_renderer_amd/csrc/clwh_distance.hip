// clwh_distance.hip -- clwh_mask_distance, clwh_mask_morph and clwh_mask_combine on the host: the argument checks in the header's
// order, the scratch, and the three passes of the separable transform.  The kernels are in distance_kernels.hip.
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

static_assert(sizeof(clwh_distance_desc) == 48 && sizeof(clwh_morph_desc) == 56 && sizeof(clwh_mask_combine_desc) == 40,
              "the descriptors as the Python binding lays them out");

// wx (X - 1)^2 + wy (Y - 1)^2 + wz (Z - 1)^2 <= 2^32 - 2 and no weight of 0; each term by division, the products may not fit
static bool weights_ok(const uint32_t *dims, const uint32_t *weight) {
  const uint64_t bound = 0xFFFFFFFEull;
  uint64_t sum = 0;
  for (int q = 0; q < 3; ++q) {
    if (weight[q] == 0u) return false;
    const uint64_t e = (uint64_t)(dims[q] - 1u) * (dims[q] - 1u);
    if (e != 0u && weight[q] > bound / e) return false;
    sum += weight[q] * e;
  }
  return sum <= bound;
}
static DistArgs dist_args(const uint32_t *dims, const uint32_t *weight, uint32_t cap) {
  DistArgs a;
  std::memset(&a, 0, sizeof a);
  a.X = (int32_t)dims[0];
  a.Y = (int32_t)dims[1];
  a.Z = (int32_t)dims[2];
  a.W64 = (int32_t)mask_w64(dims[0]);
  for (int q = 0; q < 3; ++q) a.weight[q] = weight[q];
  a.cap = cap == CLWH_DIST_NONE ? ~0ull : (unsigned long long)cap;
  return a;
}

// Which of the two line passes writes the map: the search outward from each voxel costs up to sqrt(cap / w) steps per voxel, the two
// linear scans cost the line's length whatever the data.  Measured at 512^3 the scans won every case, by ten
// times without a cap and still with a cap of 8 voxels; CLWH_TUNE_DIST_LINES=search is there to time one against the other.  Same
// bytes either way.  (The morphology keeps the search: its caps are a few voxels and its last pass writes bits, not a map.)
static bool lines_by_scan(const clwh_ctx *ctx) { return ctx->tune.dist_lines != 2; }

extern "C" int clwh_mask_distance(clwh_ctx *ctx, const clwh_distance_desc *d) {
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->mask)) return CLWH_ERR_INVALID_VALUE;
  if (!words_ok(d->dist)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~CLWH_DIST_TO_CLEAR) != 0) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  if (!weights_ok(d->dims, d->weight)) return CLWH_ERR_INVALID_VALUE;
  const size_t voxels = (size_t)(X * Y * Z);
  if (!mask_fits(X, Y, Z, d->mask)) return CLWH_ERR_SIZE_MISMATCH;
  if (d->dist->bytes / 4u < voxels) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  const DistArgs a = dist_args(d->dims, d->weight, d->cap);
  const bool scan_y = lines_by_scan(ctx), scan_z = scan_y;
  CLWH_TRY(ctx->distance.map_a.reserve(ctx->stream, voxels * 4u));
  if (scan_y) CLWH_TRY(ctx->distance.map_b.reserve(ctx->stream, voxels * 4u));

  // rows -> dist, along y -> scratch, along z -> dist
  uint32_t *out = (uint32_t *)d->dist->dptr, *tmp = ctx->distance.map_a.as<uint32_t>(), *stack = ctx->distance.map_b.as<uint32_t>();
  HIP_TRY(launch_dist_rows(a, (const unsigned long long *)d->mask->dptr, out, (d->flags & CLWH_DIST_TO_CLEAR) != 0, ctx->stream));
  HIP_TRY(scan_y ? launch_dist_lines_scan(a, out, tmp, stack, 0, ctx->stream) : launch_dist_lines(a, out, tmp, 0, ctx->stream));
  HIP_TRY(scan_z ? launch_dist_lines_scan(a, tmp, out, stack, 1, ctx->stream) : launch_dist_lines(a, tmp, out, 1, ctx->stream));
  return CLWH_OK;
}

// one step: out = { D_set <= cap } or, eroding, { D_clear > cap }; the maps stay in the scratch
static int morph_step(clwh_ctx *ctx, const DistArgs &a, const unsigned long long *in, unsigned long long *out, bool erode) {
  uint32_t *m0 = ctx->distance.map_a.as<uint32_t>(), *m1 = ctx->distance.map_b.as<uint32_t>();
  HIP_TRY(launch_dist_rows(a, in, m0, erode, ctx->stream));
  HIP_TRY(launch_dist_lines(a, m0, m1, 0, ctx->stream));
  HIP_TRY(launch_dist_lines_bits(a, m1, out, erode, ctx->stream));
  return CLWH_OK;
}

extern "C" int clwh_mask_morph(clwh_ctx *ctx, const clwh_morph_desc *d) {
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->mask_in) || !mask_ok(d->mask_out)) return CLWH_ERR_INVALID_VALUE;
  if (d->op < CLWH_MORPH_DILATE || d->op > CLWH_MORPH_CLOSE) return CLWH_ERR_INVALID_VALUE;
  if (d->flags != 0) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  if (!weights_ok(d->dims, d->weight)) return CLWH_ERR_INVALID_VALUE;
  if (!mask_fits(X, Y, Z, d->mask_in) || !mask_fits(X, Y, Z, d->mask_out)) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t voxels = (size_t)(X * Y * Z);
  const bool two_steps = d->op == CLWH_MORPH_OPEN || d->op == CLWH_MORPH_CLOSE;
  DistanceScratch &g = ctx->distance;
  CLWH_TRY(g.map_a.reserve(ctx->stream, voxels * 4u));
  CLWH_TRY(g.map_b.reserve(ctx->stream, voxels * 4u));
  if (two_steps) CLWH_TRY(g.bits.reserve(ctx->stream, mask_w64(X) * 8u * (size_t)(Y * Z)));

  // NONE is farther than any radius: a radius_sq of 0xFFFFFFFF asks for every finite distance, which is what "no cap" computes
  const DistArgs a = dist_args(d->dims, d->weight, d->radius_sq);
  const unsigned long long *in = (const unsigned long long *)d->mask_in->dptr;
  unsigned long long *out = (unsigned long long *)d->mask_out->dptr, *mid = g.bits.as<unsigned long long>();
  switch (d->op) {
    case CLWH_MORPH_DILATE: return morph_step(ctx, a, in, out, false);
    case CLWH_MORPH_ERODE: return morph_step(ctx, a, in, out, true);
    case CLWH_MORPH_OPEN:
      CLWH_TRY(morph_step(ctx, a, in, mid, true));
      return morph_step(ctx, a, mid, out, false);
    default:
      CLWH_TRY(morph_step(ctx, a, in, mid, false));
      return morph_step(ctx, a, mid, out, true);
  }
}

extern "C" int clwh_mask_combine(clwh_ctx *ctx, const clwh_mask_combine_desc *d) {
  if (!ctx || !d) return CLWH_ERR_INVALID_VALUE;
  if (!mask_ok(d->a) || !mask_ok(d->out)) return CLWH_ERR_INVALID_VALUE;
  if (d->op < CLWH_MASK_AND || d->op > CLWH_MASK_NOT) return CLWH_ERR_INVALID_VALUE;
  const bool binary = d->op != CLWH_MASK_NOT;
  if (binary && !mask_ok(d->b)) return CLWH_ERR_INVALID_VALUE;
  const uint64_t X = d->dims[0], Y = d->dims[1], Z = d->dims[2];
  if (!voxels_fit_31_bits(X, Y, Z)) return CLWH_ERR_INVALID_VALUE;
  if (!mask_fits(X, Y, Z, d->a) || !mask_fits(X, Y, Z, d->out) || (binary && !mask_fits(X, Y, Z, d->b))) return CLWH_ERR_SIZE_MISMATCH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(launch_mask_combine((const unsigned long long *)d->a->dptr, binary ? (const unsigned long long *)d->b->dptr : nullptr,
                              (unsigned long long *)d->out->dptr, (int32_t)d->dims[0], (int32_t)d->dims[1], (int32_t)d->dims[2],
                              (int32_t)mask_w64(X), d->op, ctx->stream));
  return CLWH_OK;
}
