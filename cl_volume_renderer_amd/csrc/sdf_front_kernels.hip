// sdf_front_kernels.hip -- the byte front, the first fused signed-distance-field build (CLWH_TUNE_SDF=front; the default is the
// bit-parallel build of sdf_bits_kernels.hip), gfx950.
//
// The layer iteration is a breadth-first distance transform over the
// "8 corner neighbours" graph -- a homogeneous voxel settles at layer i to +-(i+1) exactly when a corner
// neighbour holds +-i (signed_distance_field.cl:56-112; its neighbourhood is sign-uniform by
// construction of the base image).  Only voxels next to the layer-i front can change at layer i, so
// the fused build works IN PLACE on the caller's SDF image and visits only the 8x8x8 tiles whose
// 27-neighbourhood changed in the previous layer.  Reading a neighbour that another wave settles
// concurrently is harmless: it moves from +-max to +-(i+1), both > i, and signs never change, so the
// "min |neighbour| == i" test sees the same answer either way.  The result is the fixed point the
// reference's ping/pong loop converges to (both of its buffers hold every settled voxel).
#include "sdf_device.hpp"

namespace clvr {

// base image for the fused build: same values as k_sdf_base into ONE buffer, plus the layer-1 tile flags
// A block classifies a 32 x 8 x 4 box of voxels: the event flag of every voxel of the box and of its one-voxel
// halo (clamped to the volume, signed_distance_field.cl:17-31) is evaluated ONCE into LDS -- 2040 evaluations for
// 1024 voxels instead of nine per voxel -- and the homogeneity test reads the eight corner flags from there.
constexpr int kBaseX = 32, kBaseY = 8, kBaseZ = 4;
constexpr int kBaseRX = kBaseX + 2, kBaseRY = kBaseY + 2, kBaseRZ = kBaseZ + 2;
template <bool USE_GRAD>
__global__ __launch_bounds__(256) void k_sdf_base_front(const SdfArgs a, uint8_t *flags, int32_t TX, int32_t TY) {
  __shared__ uint8_t ev[kBaseRZ][kBaseRY][kBaseRX];
  __shared__ int any_one;
  const int x0 = blockIdx.x * kBaseX, y0 = blockIdx.y * kBaseY, z0 = blockIdx.z * kBaseZ;
  const VolumeIntLinear v{a.volume, a.X, a.Y, a.Z};
  if (threadIdx.x == 0) any_one = 0;
  for (int i = threadIdx.x; i < kBaseRX * kBaseRY * kBaseRZ; i += 256) {
    const int rx = i % kBaseRX, ry = (i / kBaseRX) % kBaseRY, rz = i / (kBaseRX * kBaseRY);
    const int gx = min(max(x0 - 1 + rx, 0), a.X - 1), gy = min(max(y0 - 1 + ry, 0), a.Y - 1), gz = min(max(z0 - 1 + rz, 0), a.Z - 1);
    ev[rz][ry][rx] = event_at<USE_GRAD>(v, a.tf, a.cls_in, gx, gy, gz) ? 1 : 0;
  }
  __syncthreads();
  bool block_has_one = false;
  for (int i = threadIdx.x; i < kBaseX * kBaseY * kBaseZ; i += 256) {
    const int lx = i % kBaseX, ly = (i / kBaseX) % kBaseY, lz = i / (kBaseX * kBaseY);
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    if (x >= a.X || y >= a.Y || z >= a.Z) continue;
    const unsigned e = ev[lz + 1][ly + 1][lx + 1];
    bool homogenous = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      // the halo cell of a voxel on the volume's face holds the clamped neighbour's flag
      const int3 n = corner_neighbour(c, x, y, z, a.X, a.Y, a.Z);
      const int nx = n.x - x0 + 1, ny = n.y - y0 + 1, nz = n.z - z0 + 1;
      homogenous &= (ev[nz][ny][nx] == e);
    }
    int r = e ? -1 : 1;
    if (homogenous) r *= a.max_iterations;
    a.ping[((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x] = (int8_t)r;
    if (r == 1 || r == -1) {
      // layer 1 must visit every tile that holds a corner neighbour of a |v| == 1 voxel (idempotent byte stores)
      block_has_one = true;
      const size_t own = ((size_t)(z >> 3) * TY + (size_t)(y >> 3)) * TX + (size_t)(x >> 3);
      flags[own] = 1;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int3 n = corner_neighbour(c, x, y, z, a.X, a.Y, a.Z);
        const size_t t = ((size_t)(n.z >> 3) * TY + (size_t)(n.y >> 3)) * TX + (size_t)(n.x >> 3);
        if (t != own) flags[t] = 1;
      }
    }
  }
  // only zero / non-zero of the counts is ever needed (loop termination), so plain stores replace the
  // same-address atomics that would serialise at one L2 channel
  if (block_has_one) any_one = 1;
  __syncthreads();
  if (threadIdx.x == 0 && any_one) a.counters[0] = 1;
}

// one wave tests the block's tiles, four waves process the active ones
constexpr unsigned kFrontTilesPerBlock = 32;  // measured 16 / 32 / 64 / 256 consecutive tiles per block: 6.96 / 6.61 / 8.26 / 14.3 ms for the 512^3 build
constexpr int kRowStride = 16, kSliceStride = 160;  // LDS image of a tile + halo: rows of 16 bytes [x0-4, x0+12)
constexpr unsigned kFrontWaves = 4;  // waves per block sharing the block's list of active tiles
__global__ __launch_bounds__(64 * kFrontWaves) void k_sdf_front(const SdfFrontArgs a) {
  __shared__ uint32_t s_list[kFrontTilesPerBlock];
  __shared__ uint32_t s_count;
  __shared__ __attribute__((aligned(16))) int8_t s_region[kFrontWaves][10 * kSliceStride];
  const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t n_tiles = (uint32_t)a.TX * (uint32_t)a.TY * (uint32_t)a.TZ;
  if (tid == 0) s_count = 0u;
  __syncthreads();

  // which of this block's tiles can change in this layer?  A block owns CONSECUTIVE tiles (one row of tiles at
  // 512^3): their flag reads are coalesced and neighbouring tiles share halo rows in L1 / L2.  Spreading a block's
  // tiles over the volume for balance (the first version) cost 13 ms against 8 ms for the whole 512^3 build.
  if (wave == 0u) {
    const uint32_t tile = lane < kFrontTilesPerBlock ? blockIdx.x * kFrontTilesPerBlock + lane : n_tiles;
    bool active = false;
    if (tile < n_tiles) {
      a.flags_clear[tile] = 0;
      // flagged by whoever settled a voxel next to (or inside) this tile -- unless every voxel of the tile
      // is settled already (the front has passed): such a tile can never change again
      active = a.flags_cur[tile] != 0 && a.tile_done[tile] == 0;
    }
    const unsigned long long am = __ballot(active);
    if (active) s_list[__builtin_amdgcn_mbcnt_hi((unsigned)(am >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)am, 0u))] = tile;
    if (lane == 0u) s_count = (uint32_t)__popcll(am);
  }
  __syncthreads();
  const uint32_t n_active = s_count;
  const int it = a.iteration;
  const bool rows_aligned = (a.X & 3) == 0;

  for (uint32_t k0 = 0; k0 < n_active; k0 += kFrontWaves) {
    const uint32_t k = k0 + wave;
    const bool have = k < n_active;
    int x0 = 0, y0 = 0, z0 = 0;
    uint32_t t = 0u;
    if (have) {
      t = s_list[k];
      x0 = (int)(t % (uint32_t)a.TX) * 8;
      y0 = (int)((t / (uint32_t)a.TX) % (uint32_t)a.TY) * 8;
      z0 = (int)(t / ((uint32_t)a.TX * (uint32_t)a.TY)) * 8;
      // tile + 1-voxel halo, neighbour coordinates clamped to the volume (signed_distance_field.cl:72)
      const bool wide = rows_aligned && x0 >= 4 && x0 + 12 <= a.X;  // one aligned 16-byte load per row
      for (unsigned r = lane; r < 100u; r += 64u) {
        const int rz = (int)(r / 10u), ry = (int)(r % 10u);
        const int gz = min(max(z0 - 1 + rz, 0), a.Z - 1), gy = min(max(y0 - 1 + ry, 0), a.Y - 1);
        const int8_t *row = a.sdf + ((size_t)gz * (size_t)a.Y + (size_t)gy) * (size_t)a.X;
        int8_t *dst = &s_region[wave][rz * kSliceStride + ry * kRowStride];
        if (wide) {
          // 16 bytes [x0-4, x0+12): the source is only 4-byte aligned (x0 - 4 = 4 mod 8), so four dword loads
          const uint32_t *src = reinterpret_cast<const uint32_t *>(row + x0 - 4);
          uint4 v;
          v.x = src[0]; v.y = src[1]; v.z = src[2]; v.w = src[3];
          *reinterpret_cast<uint4 *>(dst) = v;
        } else {
          // bytes 0..2 and 13..15 of the row are never neighbours of an own voxel, but the packed-byte test below
          // classifies whole dwords: keep them in the value range (an arbitrary 0x80 would carry into byte 3)
          *reinterpret_cast<uint4 *>(dst) = uint4{0u, 0u, 0u, 0u};
#pragma unroll
          for (int rx = 0; rx < 10; ++rx) dst[3 + rx] = row[min(max(x0 - 1 + rx, 0), a.X - 1)];
        }
      }
    }
    // every wave works on its own s_region slice: only the wave's own LDS writes must be visible to its reads
    // (LDS operations of one wave execute in order), so a wave-level fence replaces the block barrier
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int settled = 0;
    bool open_voxels = false;  // does this lane still hold a voxel that may settle in a later layer?
    unsigned face_mask = 0u;  // which faces of the tile this lane's settled voxels lie on: -x +x -y +y -z +z
    if (have) {
      const int ly = (int)(lane & 7u), lz = (int)(lane >> 3);
      const int y = y0 + ly, z = z0 + lz;
      if (y < a.Y && z < a.Z) {
        // A lane owns the 8 voxels of one x-row of the tile.  The reference's test (signed_distance_field.cl:56-112)
        //   |v| > it  and  the 8 corner neighbours all have one sign (zeros allowed)  and  their smallest |value| == it
        // is evaluated for the 8 voxels at once on packed bytes: the four neighbouring rows (y+-1, z+-1) are read as four
        // 16-byte LDS words, each byte is classified with carry-free SWAR arithmetic (all magnitudes are <= 127, so adding
        // 0x7F / subtracting from 0x80 | x never crosses a byte), the per-row flags are AND / OR-ed over the four rows, and
        // a voxel's corner neighbours are the flag bytes one to the left and one to the right of its own byte.  The first
        // version read 72 single bytes per lane and spent ~550 VALU instructions per row of 8 voxels; the layers of the 512^3
        // build were bound by exactly that arithmetic (profiles/r02_sdf_front_variants_negative_results.txt).
        const uint32_t b1 = 0x01010101u, b80 = 0x80808080u, b7f = 0x7F7F7F7Fu;
        const uint32_t itb = (uint32_t)it * b1, itp1b = (uint32_t)(it + 1) * b1, itp2b = (uint32_t)(it + 2) * b1;
        const int8_t *own_row = &s_region[wave][(lz + 1) * kSliceStride + (ly + 1) * kRowStride];
        uint32_t all_ne[4] = {~0u, ~0u, ~0u, ~0u}, all_ge[4] = {~0u, ~0u, ~0u, ~0u}, any_neg[4] = {0u, 0u, 0u, 0u},
                 any_pos[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint4 row = *reinterpret_cast<const uint4 *>(own_row + ((q & 1) ? kRowStride : -kRowStride) +
                                                             ((q & 2) ? kSliceStride : -kSliceStride));
          const uint32_t w[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const uint32_t sgn = (w[d] >> 7) & b1;
            const uint32_t mag = (w[d] ^ ((sgn << 8) - sgn)) + sgn;  // |byte| per byte
            all_ne[d] &= (mag ^ itb) + b7f;                          // bit 7: |byte| != it
            all_ge[d] &= (mag | b80) - itb;                          // bit 7: |byte| >= it
            any_neg[d] |= w[d];                                      // bit 7: byte < 0
            any_pos[d] |= (mag + b7f) & ~w[d];                       // bit 7: byte > 0
          }
        }
        // flags of the bytes left (x - 1) and right (x + 1) of the own bytes 4..11, i.e. of dwords 1 and 2
        auto left = [](const uint32_t *f, int d) { return (f[d] << 8) | (f[d - 1] >> 24); };
        auto right = [](const uint32_t *f, int d) { return (f[d] >> 8) | (f[d + 1] << 24); };
        const uint32_t *own_words = reinterpret_cast<const uint32_t *>(own_row + 4);  // 4-byte aligned: two dword reads
        const uint32_t own[2] = {own_words[0], own_words[1]};
        uint32_t settle[2], opened[2], fresh[2];
        const bool can_settle = it + 1 < a.max_iterations;  // the reference only writes values below max_iterations
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int d = h + 1;
          const uint32_t sgn = (own[h] >> 7) & b1, neg_mask = (sgn << 8) - sgn;
          const uint32_t mag = (own[h] ^ neg_mask) + sgn;
          const uint32_t unsettled = (mag | b80) - itp1b;                                   // |v| > it
          const uint32_t eq_any = ~(left(all_ne, d) & right(all_ne, d));                    // some corner neighbour holds it
          const uint32_t ge_all = left(all_ge, d) & right(all_ge, d);                       // none holds less (or zero)
          const uint32_t mixed = (left(any_neg, d) | right(any_neg, d)) & (left(any_pos, d) | right(any_pos, d));
          // voxels beyond the volume's x extent (last tile of a row when X is not a multiple of 8) do not exist
          uint32_t valid = b80;
          if (x0 + 8 > a.X) {
            valid = 0u;
#pragma unroll
            for (int bx = 0; bx < 4; ++bx)
              if (x0 + h * 4 + bx < a.X) valid |= 0x80u << (8 * bx);
          }
          settle[h] = can_settle ? (unsettled & eq_any & ge_all & ~mixed & valid) : 0u;
          opened[h] = ((mag | b80) - itp2b) & ~settle[h] & valid;                           // |v| > it + 1 and not settled now
          const uint32_t sel = settle[h] >> 7, sel_mask = (sel << 8) - sel;
          fresh[h] = (own[h] & ~sel_mask) | (((itp1b ^ neg_mask) + sgn) & sel_mask);        // +-(it + 1) with the voxel's sign
        }
        settled = __popc(settle[0]) + __popc(settle[1]);
        open_voxels = (opened[0] | opened[1]) != 0u;
        if (settled) {
          int8_t *out = a.sdf + ((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x0;
          if (rows_aligned && x0 + 8 <= a.X) {
            if (settle[0]) *reinterpret_cast<uint32_t *>(out) = fresh[0];
            if (settle[1]) *reinterpret_cast<uint32_t *>(out + 4) = fresh[1];
          } else {
#pragma unroll
            for (int lx = 0; lx < 8; ++lx)
              if ((settle[lx >> 2] >> (8 * (lx & 3) + 7)) & 1u) out[lx] = (int8_t)(fresh[lx >> 2] >> (8 * (lx & 3)));
          }
          face_mask = ((settle[0] >> 7) & 1u) | ((settle[1] >> 31) ? 2u : 0u) | (ly == 0 ? 4u : 0u) | (ly == 7 ? 8u : 0u) |
                      (lz == 0 ? 16u : 0u) | (lz == 7 ? 32u : 0u);
        }
      }
    }
    if (have && __ballot(open_voxels) == 0ull && lane == 0u) a.tile_done[t] = 1;
    // per wave: count, and flag every tile that holds a corner neighbour of a voxel settled here: the
    // tile itself and the (up to 26) neighbours its settled boundary voxels touch
    const unsigned long long sm = __ballot(settled > 0);
    if (have && sm != 0ull) {
      int total = settled;
      unsigned touch = face_mask;
      for (int off = 32; off > 0; off >>= 1) {
        total += __shfl_xor(total, off);
        touch |= (unsigned)__shfl_xor((int)touch, off);
      }
      if (lane == 0u && total > 0) a.counters[it] = 1;  // non-zero marker (see k_sdf_base_front)
      if (lane < 27u) {
        const int dx = (int)(lane % 3u) - 1, dy = (int)((lane / 3u) % 3u) - 1, dz = (int)(lane / 9u) - 1;
        const bool ok_x = dx == 0 || (touch & (dx < 0 ? 1u : 2u)), ok_y = dy == 0 || (touch & (dy < 0 ? 4u : 8u)),
                   ok_z = dz == 0 || (touch & (dz < 0 ? 16u : 32u));
        const int nx = x0 / 8 + dx, ny = y0 / 8 + dy, nz = z0 / 8 + dz;
        if (ok_x && ok_y && ok_z && nx >= 0 && ny >= 0 && nz >= 0 && nx < a.TX && ny < a.TY && nz < a.TZ)
          a.flags_next[((size_t)nz * a.TY + ny) * a.TX + nx] = 1;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the region is overwritten by the wave's next tile
    __builtin_amdgcn_wave_barrier();
  }
}

hipError_t launch_sdf_base_front(const SdfArgs &a, uint8_t *flags, int32_t TX, int32_t TY, hipStream_t s) {
  const dim3 grid(((unsigned)a.X + kBaseX - 1u) / kBaseX, ((unsigned)a.Y + kBaseY - 1u) / kBaseY, ((unsigned)a.Z + kBaseZ - 1u) / kBaseZ);
  hipLaunchKernelGGL(a.tf.uses_gradient ? k_sdf_base_front<true> : k_sdf_base_front<false>, grid, dim3(256), 0, s, a, flags, TX, TY);
  return hipGetLastError();
}

hipError_t launch_sdf_front(const SdfFrontArgs &a, hipStream_t s) {
  const uint32_t n_tiles = (uint32_t)a.TX * (uint32_t)a.TY * (uint32_t)a.TZ;
  hipLaunchKernelGGL(k_sdf_front, dim3((n_tiles + kFrontTilesPerBlock - 1u) / kFrontTilesPerBlock), dim3(64 * kFrontWaves), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
