// clwh_sdf.hip -- clwh_sdf_build on the host: the signed distance field of (volume, transfer function) in one call.
// The kernels are in sdf_front_kernels.hip, sdf_bits_kernels.hip and sdf_bits_layers_kernels.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

static int sdf_max_iterations(const clwh_mem *v) {
  size_t m = std::max(v->dims[0], std::max(v->dims[1], v->dims[2])) / 2;  // signed_distance_field.cpp:11
  return (int)std::min<size_t>(m, 127);
}

// the per-layer counts, once the stream has produced them
static int read_settled(clwh_ctx *ctx, std::vector<int32_t> &settled) {
  HIP_TRY(hipMemcpyAsync(settled.data(), ctx->sdf.counters.ptr, settled.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CLWH_OK;
}

// the byte front: one launch per layer over the active 8x8x8 tiles (sdf_front_kernels.hip); CLWH_TUNE_SDF=front
static int sdf_build_front(clwh_ctx *ctx, SdfArgs &b, std::vector<int32_t> &settled) {
  const int X = b.X, Y = b.Y, Z = b.Z;
  const int TX = (X + 7) / 8, TY = (Y + 7) / 8, TZ = (Z + 7) / 8;
  const size_t n_tiles = (size_t)TX * TY * TZ;
  CLWH_TRY(ctx->sdf.flags.reserve(ctx->stream, 4 * n_tiles));
  uint8_t *all_flags = ctx->sdf.flags.as<uint8_t>();
  HIP_TRY(hipMemsetAsync(all_flags, 0, 4 * n_tiles, ctx->stream));
  uint8_t *flags[3] = {all_flags, all_flags + n_tiles, all_flags + 2 * n_tiles};
  HIP_TRY(launch_sdf_base_front(b, flags[1], TX, TY, ctx->stream));  // layer 1 reads flags[1 % 3]

  SdfFrontArgs a;
  std::memset(&a, 0, sizeof a);
  a.sdf = b.ping;
  a.X = X; a.Y = Y; a.Z = Z;
  a.TX = TX; a.TY = TY; a.TZ = TZ;
  a.max_iterations = b.max_iterations;
  a.counters = b.counters;
  a.tile_done = all_flags + 3 * n_tiles;

  // layers that can still settle a voxel: i + 1 < max_iterations; the host looks at the per-layer
  // counts every kSdfLayersPerCheck launches and stops once a layer settled nothing (nothing can change after it)
  constexpr int kSdfLayersPerCheck = 32;  // measured 16 / 32 / 64 / 128: 5.31 / 5.21 / 5.14 / 5.19 ms for the 512^3 build
  const int last_layer = a.max_iterations - 2;
  int i = 1;
  bool quiet = false;
  while (i <= last_layer && !quiet) {
    const int chunk_end = std::min(last_layer, i + kSdfLayersPerCheck - 1);
    for (; i <= chunk_end; ++i) {
      a.iteration = i;
      a.flags_cur = flags[i % 3];
      a.flags_next = flags[(i + 1) % 3];
      a.flags_clear = flags[(i + 2) % 3];
      HIP_TRY(launch_sdf_front(a, ctx->stream));
    }
    CLWH_TRY(read_settled(ctx, settled));
    for (int j = 1; j < i; ++j)
      if (settled[j] == 0) quiet = true;
  }
  if (i <= 1) return read_settled(ctx, settled);  // no layer ran (max_iterations <= 2): still need the base counts
  return CLWH_OK;
}

#ifdef CLVR_SDFBIT_TIMING
static int print_sdfbit_timing(const clwh_ctx *ctx) {
  unsigned long long tm[8];
  HIP_TRY(hipMemcpy(tm, ctx->sdf.timing.ptr, sizeof tm, hipMemcpyDeviceToHost));
  const double n = tm[0] ? (double)tm[0] : 1.0;
  std::fprintf(stderr, "sdfbit timing: %llu regions (%llu interior); per region, us: fetch %.2f load %.2f steps %.2f store+values %.2f tail %.2f\n", tm[0], tm[6],
               tm[1] / n / 100.0, tm[2] / n / 100.0, tm[3] / n / 100.0, tm[4] / n / 100.0, tm[5] / n / 100.0);
  return CLWH_OK;
}
#endif

// CLWH_DEBUG_SDFBIT: regions each launch worked on
static int print_sdfbit_regions(const SdfBitArgs &a, const uint32_t *queue, int n_launches, size_t n_blocks) {
  std::vector<uint32_t> q(2 * (size_t)(n_launches + 1));
  HIP_TRY(hipMemcpy(q.data(), queue, q.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::fprintf(stderr, "sdfbit: %zu regions of 64 x 48 x %d voxels, active per launch:", n_blocks, a.core_z);
  for (int l = 0; l < n_launches; ++l) std::fprintf(stderr, " %u", q[2 * l]);
  std::fprintf(stderr, "\n");
  return CLWH_OK;
}

// the bit-parallel build: event bits -> seeds + base image -> eight layers per launch on one bit per voxel (sdf_bits_kernels.hip, sdf_bits_layers_kernels.hip)
static int sdf_build_bits(clwh_ctx *ctx, SdfArgs &b, std::vector<int32_t> &settled) {
  const int X = b.X, Y = b.Y, Z = b.Z;
  SdfBitArgs a;
  std::memset(&a, 0, sizeof a);
  a.X = X; a.Y = Y; a.Z = Z;
  a.WP = 2 * ((X + 63) / 64);
  const int waves = ctx->tune.sdfbit_waves;
  sdfbit_block_grid(X, Y, Z, waves, &a.BX, &a.BY, &a.BZ, &a.core_z);
  const size_t words = (size_t)a.WP * (size_t)Y * (size_t)Z;
  const size_t n_blocks = (size_t)a.BX * a.BY * a.BZ;
  if (n_blocks >= (1ull << 31)) return CLWH_ERR_INVALID_VALUE;
  // a voxel D corner moves from the nearest seed settles to D + 1 while D + 1 < max_iterations: max_iterations - 2 layers
  const int total = b.max_iterations - 2;
  const int n_launches = total > 0 ? (total + 7) / 8 : 0;
  // scratch: event bits (x-fastest rows), two reached-set buffers (tiled by region, padded to whole regions), the list of active
  // blocks, per-launch {count, head}, the regions' states and wake stamps
  const size_t tiled = n_blocks * (size_t)(2 * 48 * a.core_z);
  const size_t small = (n_blocks + 2 * (size_t)(n_launches + 1) + 1) & ~(size_t)1;  // even: the planes behind it take 8-byte atomics
  const size_t scratch_words = words + 2 * tiled + small + 7 * tiled;  // ... and the seven bit planes of the layer index
  CLWH_TRY(ctx->sdf.bits.reserve(ctx->stream, scratch_words * sizeof(uint32_t) + 2 * n_blocks));
  uint32_t *bits = ctx->sdf.bits.as<uint32_t>();
  uint32_t *ev = bits, *reached[2] = {bits + words, bits + words + tiled};  // words and tiled are even: 8-byte aligned
  uint32_t *list = bits + words + 2 * tiled, *queue = list + n_blocks;
  a.planes = bits + words + 2 * tiled + small;
  a.plane_words = tiled;
  HIP_TRY(hipMemsetAsync(a.planes, 0, 7 * tiled * sizeof(uint32_t), ctx->stream));
  a.sdf = b.ping;
  a.ev = ev;
  a.list = list;
  a.state = reinterpret_cast<uint8_t *>(bits + scratch_words);
  a.wake = a.state + n_blocks;
  a.presence = b.counters;
  HIP_TRY(hipMemsetAsync(reached[0], 0, 2 * tiled * sizeof(uint32_t), ctx->stream));  // rows nobody ever writes (beyond the volume, never reached) read as empty in both buffers
  HIP_TRY(hipMemsetAsync(queue, 0, 2 * (size_t)(n_launches + 1) * sizeof(uint32_t), ctx->stream));
  HIP_TRY(hipMemsetAsync(a.wake, 0, n_blocks, ctx->stream));
  HIP_TRY(launch_sdfbit_events(b, ev, a.WP, ctx->stream));
  a.r_out = reached[0];
  HIP_TRY(launch_sdfbit_seed(a, ctx->stream));
  a.r_in = reached[0];
  HIP_TRY(launch_sdfbit_state(a, ctx->stream));
#ifdef CLVR_SDFBIT_TIMING
  CLWH_TRY(ctx->sdf.timing.reserve(ctx->stream, 8 * sizeof(unsigned long long)));
  a.timing = ctx->sdf.timing.as<unsigned long long>();
  HIP_TRY(hipMemsetAsync(a.timing, 0, 8 * sizeof(unsigned long long), ctx->stream));
#endif
  int t = 0;
  for (int r0 = 0; r0 < total; r0 += 8, ++t) {
    a.r0 = r0;
    a.launch = t;
    a.steps = std::min(8, total - r0);
    a.r_in = reached[t & 1];
    a.r_out = reached[(t + 1) & 1];
    a.list_count = queue + 2 * t;
    a.list_head = queue + 2 * t + 1;
    const bool rec_lds = waves == 8 && ctx->tune.sdfbit_rec_lds != 0;
    HIP_TRY(launch_sdfbit_layers(a, waves, (unsigned)ctx->tune.sdfbit_grid * (waves == 16 ? 1u : (rec_lds ? 3u : 2u)) / 2u, rec_lds, ctx->stream));
  }
  // the values, once: the reached set after the last launch is the one it wrote (regions complete earlier are complete in both)
  HIP_TRY(launch_sdfbit_expand(a, reached[t & 1], b.max_iterations, ctx->stream));
  CLWH_TRY(read_settled(ctx, settled));
#ifdef CLVR_SDFBIT_TIMING
  CLWH_TRY(print_sdfbit_timing(ctx));
#endif
  if (std::getenv("CLWH_DEBUG_SDFBIT")) return print_sdfbit_regions(a, queue, n_launches, n_blocks);
  return CLWH_OK;
}

// what the reference's host loop would have run (app/signed_distance_field.cpp:22-32): its counter at
// layer i counts the voxels holding i plus those settling to i+1 (< max); it stops at the first odd
// layer whose counter is zero, or at the bound
static int reference_launches(const std::vector<int32_t> &settled, int max_iterations) {
  const int kSlots = (int)settled.size();
  const int bound = max_iterations + (max_iterations % 2) + 1;
  for (int j = 1; j <= bound; ++j) {
    const int64_t holding = (j == 1) ? settled[0] : (j - 1 < kSlots ? settled[j - 1] : 0);
    const int64_t settling = j < kSlots ? settled[j] : 0;
    const bool holding_counts = j < max_iterations;  // a voxel holding j is rewritten only while j < max
    if ((j & 1) && (holding_counts ? holding : 0) + settling == 0) return j;
  }
  return bound;
}

extern "C" int clwh_sdf_build(clwh_ctx *ctx, clwh_mem *volume, const char *tf_source, clwh_mem *sdf, int32_t *n_launches) {
  if (!ctx || !volume || !tf_source || !sdf) return CLWH_ERR_INVALID_VALUE;
  if (!is_image(volume, 3, 1, CLWH_ELEM_S16) || !is_image(sdf, 3, 1, CLWH_ELEM_S8)) return CLWH_ERR_BAD_ARGS;
  if (!same_dims(volume, sdf)) return CLWH_ERR_SIZE_MISMATCH;
  if (!fits_grid_yz(volume)) return CLWH_ERR_INVALID_VALUE;
  HIP_TRY(hipSetDevice(ctx->device));
  SdfArgs b;
  std::memset(&b, 0, sizeof b);
  clwh_tf tf;
  int rc = clwh_tf_parse(tf_source, &tf);
  if (rc == CLWH_OK) {
    tf_to_dev(tf, b.tf);
  } else if (rc == CLWH_ERR_TF_UNSUPPORTED) {
    std::shared_ptr<JitTf> jit;
    rc = jit_for_source(ctx, tf_source, jit);
    if (rc == CLWH_OK) rc = ensure_classes(ctx, jit, volume, b.tf, &b.cls_in);
  }
  if (rc != CLWH_OK) return rc;

  constexpr int kSlots = 160;
  CLWH_TRY(ctx->sdf.counters.reserve(ctx->stream, kSlots * sizeof(int32_t)));
  HIP_TRY(hipMemsetAsync(ctx->sdf.counters.ptr, 0, kSlots * sizeof(int32_t), ctx->stream));
  std::vector<int32_t> settled(kSlots, 0);
  b.volume = (const int16_t *)volume->dptr;
  b.X = (int)volume->dims[0]; b.Y = (int)volume->dims[1]; b.Z = (int)volume->dims[2];
  b.ping = (int8_t *)sdf->dptr;
  b.max_iterations = sdf_max_iterations(volume);
  b.counters = ctx->sdf.counters.as<int32_t>();  // [0] != 0: some |v| == 1
  CLWH_TRY(ctx->tune.sdf_front ? sdf_build_front(ctx, b, settled) : sdf_build_bits(ctx, b, settled));
  if (n_launches) *n_launches = reference_launches(settled, b.max_iterations);
  touch(sdf);
  return CLWH_OK;
}
