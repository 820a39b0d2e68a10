// sdf_bits_kernels.hip -- the bit-parallel fused signed-distance-field build (clwh_sdf_build, default), gfx950: its fixed passes (event bits,
// seeds, region states, the expansion to bytes); the layers in between are in sdf_bits_layers_kernels.hip.  The layer iteration is a
// breadth-first search over the "8 clamped corner neighbours" graph (sdf_front_kernels.hip): with D(v) = the number of corner moves from v to the nearest
// non-homogeneous voxel, the converged image holds sign * min(D + 1, max_iterations), and a voxel only settles
// while D + 1 < max_iterations.  The search front does not need the byte image at all: the set
// R_r = {v : D(v) <= r} is ONE BIT per voxel (x-fastest rows of 32-bit words), and one layer is
//   R_{r+1} = R_r | shift_x(+-1, clamped)( R_r(y-1,z-1) | R_r(y+1,z-1) | R_r(y-1,z+1) | R_r(y+1,z+1) )   (rows clamped)
// -- a dozen word operations for 128 voxels.  A block keeps a 128 x 32 x 32 voxel region of R (its 64 x 16 x 16 core and a
// halo of 8 rows / 32 bits) in 16 KB of LDS and runs EIGHT layers on it before anything returns to memory: information
// travels one voxel per layer, so after 8 layers the core is exact although the halo's rim is not.  125 dependent
// launches become 16, none of them with a host round trip; blocks whose core is complete, or whose 27-neighbourhood
// holds no reached voxel yet, leave after reading a few state bytes.  A voxel's value is written once, in the launch
// in which its bit appears (layer index recorded bit-sliced per core word), with the sign of its event bit.
// Bit-exact against the oracle / the reference's golden vector like the byte front it replaces (tests/test_gpu_sdf.py).
#include "mask_device.hpp"  // load8
#include "sdf_device.hpp"

namespace clvr {

// event bit of every voxel: one wave = 64 voxels along x = two words
template <bool USE_GRAD>
__global__ __launch_bounds__(256) void k_sdfbit_events(const SdfArgs a, uint32_t *__restrict__ ev, int32_t WP) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y, z = blockIdx.z;
  const VolumeIntLinear v{a.volume, a.X, a.Y, a.Z};
  bool e = false;
  if (x < a.X) e = event_at<USE_GRAD>(v, a.tf, a.cls_in, x, y, z);
  const unsigned long long m = __ballot(e);
  if ((threadIdx.x & 63u) == 0u) {
    const int w = x >> 5;  // x is a multiple of 64 here
    if (w < WP) {
      uint32_t *row = ev + ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)WP;
      row[w] = (uint32_t)m;
      row[w + 1] = (uint32_t)(m >> 32);  // WP is even
    }
  }
}

// the same for rule tables on rows of a multiple of 8 voxels: a lane classifies the 8 voxels of one 16-byte load (with `gradient`
// rules: plus the four neighbouring rows' loads) and writes their byte of the bit image (387 -> 57 us at 512^3 without
// gradient rules: the per-voxel kernel was issue-bound)
template <bool USE_GRAD>
__global__ __launch_bounds__(256) void k_sdfbit_events8(const SdfArgs a, uint8_t *__restrict__ ev_bytes, int32_t WP) {
  size_t row;
  uint32_t unit;
  const size_t n_rows = (size_t)a.Y * (size_t)a.Z;
  if (!sdfbit_row_unit((uint32_t)WP * 4u, n_rows, row, unit)) return;
  const int x0 = (int)unit * 8;
  uint32_t bits = 0u;
  if (x0 < a.X) {  // X is a multiple of 8: all eight voxels exist
    const int16_t *own = a.volume + row * (size_t)a.X + (size_t)x0;
    int value[8], gradient[8];
    load8(own, value);
#pragma unroll
    for (int h = 0; h < 8; ++h) gradient[h] = 0;
    if (USE_GRAD) {
      // utility_filter.cl:2-35 at the voxel: central differences of the six neighbours (border texel 0), the float length
      // converted to short (signed_distance_field.cl:13-20) -- event_at<true> for eight voxels of one row
      const int z = (int)(row / (size_t)a.Y), y = (int)(row - (size_t)z * (size_t)a.Y);
      int ym[8], yp[8], zm[8], zp[8];
#pragma unroll
      for (int h = 0; h < 8; ++h) ym[h] = yp[h] = zm[h] = zp[h] = 0;
      if (y > 0) load8(own - a.X, ym);
      if (y + 1 < a.Y) load8(own + a.X, yp);
      if (z > 0) load8(own - (size_t)a.X * (size_t)a.Y, zm);
      if (z + 1 < a.Z) load8(own + (size_t)a.X * (size_t)a.Y, zp);
      const int left = x0 > 0 ? (int)own[-1] : 0, right = x0 + 8 < a.X ? (int)own[8] : 0;
#pragma unroll
      for (int h = 0; h < 8; ++h) {
        const float dx = (float)((h < 7 ? value[h < 7 ? h + 1 : 7] : right) - (h > 0 ? value[h > 0 ? h - 1 : 0] : left));
        const float dy = (float)(yp[h] - ym[h]);
        const float dz = (float)(zp[h] - zm[h]);
        gradient[h] = (int)(short)f2i(sqrtf((dx * dx + dy * dy) + dz * dz));
      }
    }
    // tf_eval for the eight voxels at once, the rule (one scalar load of its bounds) in the outer loop: the first matching
    // rule decides, a terminal rule that does not match decides "no event" (render_device.hpp: tf_eval)
    uint32_t undecided = 0xFFu;
    for (int k = 0; k < a.tf.n && undecided; ++k) {
      const int lo = a.tf.rules[k].v_lo, hi = a.tf.rules[k].v_hi, g_lo = a.tf.rules[k].g_lo, g_hi = a.tf.rules[k].g_hi;
      const bool use_g = USE_GRAD && (a.tf.rules[k].flags & TF_USE_GRADIENT);
      uint32_t m = 0u;
#pragma unroll
      for (int h = 0; h < 8; ++h) {
        bool hit = value[h] >= lo && value[h] <= hi;
        if (use_g) hit = hit && gradient[h] >= g_lo && gradient[h] <= g_hi;
        m |= hit ? (1u << h) : 0u;
      }
      bits |= m & undecided;
      undecided &= ~m;
      if (a.tf.rules[k].flags & TF_TERMINAL) undecided = 0u;
    }
  }
  ev_bytes[row * (size_t)WP * 4u + unit] = (uint8_t)bits;
}

// The reached-set buffers are TILED by region: tile (bx, by, bz) = the region's core, 48 * core_z rows of two words, row (cy, cz) at
// ((cz * 48 + cy) * 2): the rows a wave of k_sdfbit_layers loads / stores (64 lanes = 64 consecutive y) are contiguous 8-byte pairs.
// (In the x-fastest layout of the event bits the same rows lie 64 bytes apart at 512^3: every lane its own cache line, and the
// address unit, not the layers, set the pace of a region.)  Tiles are padded to full size; rows beyond the volume stay zero.
struct SdfBitTiles {
  int32_t BX, BY, core_z;
  __device__ __forceinline__ size_t tile_words() const { return (size_t)2 * 48u * (size_t)core_z; }
  __device__ __forceinline__ size_t word(int w, int y, int z) const {
    const int bx = w >> 1, by = y / 48, cy = y - by * 48, bz = z / core_z, cz = z - bz * core_z;
    return (((size_t)bz * BY + by) * BX + bx) * tile_words() + (size_t)((cz * 48 + cy) * 2 + (w & 1));
  }
};

// non-homogeneous voxels (create_base_image: some clamped corner neighbour's event flag differs) = the seeds R_0
__device__ __forceinline__ void sdfbit_seed_word(const uint32_t *__restrict__ ev, uint32_t *__restrict__ r0, int32_t X, int32_t Y, int32_t Z, int32_t WP,
                                                 int32_t *presence, const SdfBitTiles &tiles, int w, int y, int z) {
  const size_t rowi = (size_t)z * (size_t)Y + (size_t)y;
  const int x_lo = w * 32;
  uint32_t valid = 0u;
  if (x_lo < X) valid = (X - x_lo >= 32) ? 0xFFFFFFFFu : ((1u << (X - x_lo)) - 1u);
  const uint32_t lastbit = (((X - 1) >> 5) == w) ? (1u << ((X - 1) & 31)) : 0u;
  const uint32_t firstbit = (w == 0) ? 1u : 0u;
  const uint32_t own = ev[rowi * (size_t)WP + w];
  uint32_t differs = 0u;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int ny = corner_step(y, c & 1, Y), nz = corner_step(z, c & 2, Z);
    const uint32_t *row = ev + ((size_t)nz * Y + ny) * (size_t)WP;
    const uint32_t cur = row[w], prev = w > 0 ? row[w - 1] : 0u, next = w + 1 < WP ? row[w + 1] : 0u;
    const uint32_t left = ((cur << 1) | (prev >> 31)) | (cur & firstbit);   // value at clamp(x - 1)
    const uint32_t right = ((cur >> 1) | (next << 31)) | (cur & lastbit);   // value at clamp(x + 1)
    differs |= (left ^ own) | (right ^ own);
  }
  differs &= valid;
  r0[tiles.word(w, y, z)] = differs;
  if (differs) presence[0] = 1;  // non-zero marker, plain store (see k_sdf_base_front)
}
__global__ __launch_bounds__(256) void k_sdfbit_seed(const uint32_t *__restrict__ ev, uint32_t *__restrict__ r0, int32_t X, int32_t Y,
                                                      int32_t Z, int32_t WP, int32_t *presence, SdfBitTiles tiles) {
  size_t rowi;
  uint32_t unit;
  if (!sdfbit_row_unit((uint32_t)WP, (size_t)Y * (size_t)Z, rowi, unit)) return;
  const int z = (int)(rowi / (size_t)Y), y = (int)(rowi - (size_t)z * (size_t)Y);
  sdfbit_seed_word(ev, r0, X, Y, Z, WP, presence, tiles, (int)unit, y, z);
}
// rows of a multiple of WPB words (16, 32 or 64 lanes along x): a block takes sixteen consecutive rows, so that every 128-byte line of the
// tiled image is written whole by one block (see k_sdfbit_expand16_rows16)
template <int WPB>
__global__ __launch_bounds__(16 * WPB) void k_sdfbit_seed_rows16(const uint32_t *__restrict__ ev, uint32_t *__restrict__ r0, int32_t X, int32_t Y,
                                                                 int32_t Z, int32_t WP, int32_t *presence, SdfBitTiles tiles) {
  const int w = (int)blockIdx.x * WPB + (int)(threadIdx.x % (unsigned)WPB), y = (int)blockIdx.y * 16 + (int)(threadIdx.x / (unsigned)WPB);
  if (y >= Y) return;
  sdfbit_seed_word(ev, r0, X, Y, Z, WP, presence, tiles, w, y, (int)blockIdx.z);
}

// The values, once: bit planes of the layer index + the final reached set + the event bits -> one signed byte per voxel.
// A seed (reached, index 0) holds +-1, a voxel reached by layer `index` holds +-(index + 1), an unreached one +-max_iterations
// (create_base_image's values for the first and the last, signed_distance_field.cl:40-53; the sign is the event class).
__global__ __launch_bounds__(256) void k_sdfbit_expand(const uint32_t *__restrict__ ev, const uint32_t *__restrict__ reached, const uint32_t *__restrict__ planes,
                                                        size_t plane_words, int8_t *__restrict__ sdf, int32_t X, int32_t Y, int32_t Z, int32_t WP,
                                                        int32_t max_iterations, SdfBitTiles tiles) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y, z = blockIdx.z;
  if (x >= X) return;
  const size_t roww = ((size_t)z * Y + y) * (size_t)WP + (size_t)(x >> 5), tw = tiles.word(x >> 5, y, z);
  const uint32_t sh = (uint32_t)(x & 31);
  const uint32_t e = (ev[roww] >> sh) & 1u, r = (reached[tw] >> sh) & 1u;
  uint32_t index = 0u;
  if (r) {
#pragma unroll
    for (int p = 0; p < 7; ++p) index |= ((planes[(size_t)p * plane_words + tw] >> sh) & 1u) << p;
  }
  const int val = r ? (int)index + 1 : max_iterations;
  sdf[((size_t)z * Y + y) * (size_t)X + (size_t)x] = (int8_t)(e ? -val : val);
}

// the same, sixteen voxels (one 16-byte store) per lane: rows of a multiple of 16 voxels
__device__ __forceinline__ void sdfbit_expand16_voxels(const uint32_t *__restrict__ ev, const uint32_t *__restrict__ reached, const uint32_t *__restrict__ planes,
                                                       size_t plane_words, int8_t *__restrict__ sdf, int32_t X, int32_t WP, int32_t max_iterations,
                                                       const SdfBitTiles &tiles, int x0, int y, int z, size_t row) {
  const uint32_t b1 = 0x01010101u;
  const size_t tw = tiles.word(x0 >> 5, y, z);
  const uint32_t sh = (uint32_t)(x0 & 31);
  const uint32_t e16 = (ev[row * (size_t)WP + (size_t)(x0 >> 5)] >> sh) & 0xFFFFu, r16 = (reached[tw] >> sh) & 0xFFFFu;
  uint32_t p16[7];
#pragma unroll
  for (int p = 0; p < 7; ++p) p16[p] = 0u;
  if (r16 != 0u) {  // nothing reached here (the far field beyond 126 layers, empty volumes): no plane is read
#pragma unroll
    for (int p = 0; p < 7; ++p) p16[p] = (planes[(size_t)p * plane_words + tw] >> sh) & 0xFFFFu;
  }
  uint32_t out[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    auto spread = [&](uint32_t bits16) { return __umul24((bits16 >> (4 * q)) & 0xFu, 0x204081u) & b1; };  // four bits -> the low bit of four bytes
    auto bytes_ff = [](uint32_t ones) { return (ones << 8) - ones; };                                        // 0 / 1 per byte -> 0x00 / 0xFF
    uint32_t idx = 0u;
#pragma unroll
    for (int p = 0; p < 7; ++p) idx += spread(p16[p]) << p;                                                  // <= 127 per byte
    const uint32_t rb = bytes_ff(spread(r16)), eb = spread(e16);
    const uint32_t val = ((idx + b1) & rb) | (((uint32_t)max_iterations * b1) & ~rb);                        // reached: index + 1 (<= 128 - 1); else max
    out[q] = (val ^ bytes_ff(eb)) + eb;                                                                      // two's complement per byte where the voxel is an event
  }
  *reinterpret_cast<uint4 *>(sdf + row * (size_t)X + (size_t)x0) = uint4{out[0], out[1], out[2], out[3]};
}
__global__ __launch_bounds__(256) void k_sdfbit_expand16(const uint32_t *__restrict__ ev, const uint32_t *__restrict__ reached, const uint32_t *__restrict__ planes,
                                                          size_t plane_words, int8_t *__restrict__ sdf, int32_t X, int32_t Y, int32_t Z, int32_t WP,
                                                          int32_t max_iterations, SdfBitTiles tiles) {
  size_t row;
  uint32_t unit;
  if (!sdfbit_row_unit((uint32_t)(X / 16), (size_t)Y * (size_t)Z, row, unit)) return;
  const int z = (int)(row / (size_t)Y), y = (int)(row - (size_t)z * (size_t)Y);
  sdfbit_expand16_voxels(ev, reached, planes, plane_words, sdf, X, WP, max_iterations, tiles, (int)unit * 16, y, z, row);
}
// Rows of a multiple of 16 * UPB voxels (UPB = 32 or 64 lanes along x): a block takes UPB * 16 voxels of SIXTEEN consecutive rows -- the rows
// whose words share a 128-byte line in the tiled bit images (a tile keeps its 48 rows' word pairs contiguous).  With one or two rows per
// block eight consecutive blocks -- on eight XCDs -- each fetched every line of the planes: 32 GB read for 9 GB of bit images at 2048^3.
template <int UPB>
__global__ __launch_bounds__(16 * UPB) void k_sdfbit_expand16_rows16(const uint32_t *__restrict__ ev, const uint32_t *__restrict__ reached,
                                                                     const uint32_t *__restrict__ planes, size_t plane_words, int8_t *__restrict__ sdf,
                                                                     int32_t X, int32_t Y, int32_t Z, int32_t WP, int32_t max_iterations, SdfBitTiles tiles) {
  const int u = (int)(threadIdx.x % (unsigned)UPB), r = (int)(threadIdx.x / (unsigned)UPB);
  const int x0 = ((int)blockIdx.x * UPB + u) * 16, y = (int)blockIdx.y * 16 + r, z = (int)blockIdx.z;
  if (y >= Y) return;  // (x0 < X: X is a multiple of 16 * UPB)
  sdfbit_expand16_voxels(ev, reached, planes, plane_words, sdf, X, WP, max_iterations, tiles, x0, y, z, (size_t)z * (size_t)Y + (size_t)y);
}

__global__ __launch_bounds__(64) void k_sdfbit_state(const SdfBitArgs a) {
  const int b = blockIdx.x;
  const int bx = b % a.BX, by = (b / a.BX) % a.BY, bz = b / (a.BX * a.BY);
  const unsigned lane = threadIdx.x;
  bool any = false, all = true;
  uint32_t orx[2] = {0u, 0u};
  int y0 = 255, y1 = -1, z0 = 255, z1 = -1;
  for (int r = (int)lane; r < kBitCoreY * a.core_z; r += 64) {
    const int cy = r % kBitCoreY, cz = r / kBitCoreY;
    const int gy = by * kBitCoreY + cy, gz = bz * a.core_z + cz;
    if (gy >= a.Y || gz >= a.Z) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gw = 2 * bx + j, x_lo = gw * 32;
      if (gw >= a.WP || x_lo >= a.X) continue;
      const uint32_t valid = (a.X - x_lo >= 32) ? 0xFFFFFFFFu : ((1u << (a.X - x_lo)) - 1u);
      const uint32_t wv = a.r_in[(size_t)b * (size_t)(2 * kBitCoreY * a.core_z) + (size_t)(r * 2 + j)];
      any |= wv != 0u;
      all &= wv == valid;
      orx[j] |= wv;
      if (wv) { y0 = min(y0, cy); y1 = max(y1, cy); z0 = min(z0, cz); z1 = max(z1, cz); }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    orx[0] |= (uint32_t)__shfl_xor((int)orx[0], off); orx[1] |= (uint32_t)__shfl_xor((int)orx[1], off);
    y0 = min(y0, __shfl_xor(y0, off)); y1 = max(y1, __shfl_xor(y1, off));
    z0 = min(z0, __shfl_xor(z0, off)); z1 = max(z1, __shfl_xor(z1, off));
  }
  const bool w_any = __ballot(any) != 0ull, w_all = __ballot(!all) == 0ull;
  if (lane == 0u) a.state[b] = w_all ? 2 : (w_any ? 1 : 0);
  if (w_any) {
    const unsigned long long orx64 = (unsigned long long)orx[0] | ((unsigned long long)orx[1] << 32);
    sdfbit_wake_neighbours(a, bx, by, bz, __ffsll((long long)orx64) - 1, 63 - __clzll((long long)orx64), y0, y1, z0, z1, lane, 1);  // launch 0
  }
}

void sdfbit_block_grid(int X, int Y, int Z, int waves, int32_t *BX, int32_t *BY, int32_t *BZ, int32_t *core_z) {
  *core_z = kBitRows * waves - 2 * kBitHalo;
  *BX = (X + 63) / 64;
  *BY = (Y + kBitCoreY - 1) / kBitCoreY;
  *BZ = (Z + *core_z - 1) / *core_z;
}

hipError_t launch_sdfbit_events(const SdfArgs &a, uint32_t *ev, int32_t WP, hipStream_t s) {
  if (!a.cls_in && (a.X % 8) == 0)
    hipLaunchKernelGGL(a.tf.uses_gradient ? k_sdfbit_events8<true> : k_sdfbit_events8<false>, sdfbit_row_grid((uint32_t)WP * 4u, (size_t)a.Y * (size_t)a.Z),
                       dim3(256), 0, s, a, (uint8_t *)ev, WP);
  else
    hipLaunchKernelGGL(a.tf.uses_gradient ? k_sdfbit_events<true> : k_sdfbit_events<false>, dim3(((unsigned)a.X + 255u) / 256u, (unsigned)a.Y, (unsigned)a.Z),
                       dim3(256), 0, s, a, ev, WP);
  return hipGetLastError();
}

template <int WPB>
static void seed_rows16(const SdfBitArgs &a, const SdfBitTiles &tiles, hipStream_t s) {
  hipLaunchKernelGGL(k_sdfbit_seed_rows16<WPB>, dim3((unsigned)a.WP / WPB, ((unsigned)a.Y + 15u) / 16u, (unsigned)a.Z), dim3(16 * WPB), 0, s, a.ev, a.r_out, a.X,
                     a.Y, a.Z, a.WP, a.presence, tiles);
}
hipError_t launch_sdfbit_seed(const SdfBitArgs &a, hipStream_t s) {
  const size_t n_rows = (size_t)a.Y * (size_t)a.Z;
  const SdfBitTiles tiles{a.BX, a.BY, a.core_z};
  if ((a.WP % 64) == 0) seed_rows16<64>(a, tiles, s);
  else if ((a.WP % 32) == 0) seed_rows16<32>(a, tiles, s);
  else if ((a.WP % 16) == 0) seed_rows16<16>(a, tiles, s);
  else
    hipLaunchKernelGGL(k_sdfbit_seed, sdfbit_row_grid((uint32_t)a.WP, n_rows), dim3(256), 0, s, a.ev, a.r_out, a.X, a.Y, a.Z, a.WP, a.presence, tiles);
  return hipGetLastError();
}

template <int UPB>
static void expand_rows16(const SdfBitArgs &a, const uint32_t *reached, int32_t max_iterations, const SdfBitTiles &tiles, hipStream_t s) {
  hipLaunchKernelGGL(k_sdfbit_expand16_rows16<UPB>, dim3((unsigned)(a.X / (16 * UPB)), ((unsigned)a.Y + 15u) / 16u, (unsigned)a.Z), dim3(16 * UPB), 0, s, a.ev,
                     reached, (const uint32_t *)a.planes, a.plane_words, a.sdf, a.X, a.Y, a.Z, a.WP, max_iterations, tiles);
}
hipError_t launch_sdfbit_expand(const SdfBitArgs &a, const uint32_t *reached, int32_t max_iterations, hipStream_t s) {
  const size_t n_rows = (size_t)a.Y * (size_t)a.Z;
  const SdfBitTiles tiles{a.BX, a.BY, a.core_z};
  if ((a.X % 1024) == 0 && max_iterations >= 1) expand_rows16<64>(a, reached, max_iterations, tiles, s);
  else if ((a.X % 512) == 0 && max_iterations >= 1) expand_rows16<32>(a, reached, max_iterations, tiles, s);
  else if ((a.X % 16) == 0 && max_iterations >= 1)
    hipLaunchKernelGGL(k_sdfbit_expand16, sdfbit_row_grid((uint32_t)(a.X / 16), n_rows), dim3(256), 0, s, a.ev, reached, (const uint32_t *)a.planes,
                       a.plane_words, a.sdf, a.X, a.Y, a.Z, a.WP, max_iterations, tiles);
  else
    hipLaunchKernelGGL(k_sdfbit_expand, dim3(((unsigned)a.X + 255u) / 256u, (unsigned)a.Y, (unsigned)a.Z), dim3(256), 0, s, a.ev, reached,
                       (const uint32_t *)a.planes, a.plane_words, a.sdf, a.X, a.Y, a.Z, a.WP, max_iterations, tiles);
  return hipGetLastError();
}

hipError_t launch_sdfbit_state(const SdfBitArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_sdfbit_state, dim3((unsigned)(a.BX * a.BY * a.BZ)), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
