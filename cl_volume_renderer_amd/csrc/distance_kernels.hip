// distance_kernels.hip -- the exact squared Euclidean distance map of a mask (clwh_mask_distance), the ball morphology thresholded
// from it (clwh_mask_morph) and mask algebra (clwh_mask_combine), gfx950.  Masks are grow's bit rows: W64 64-bit words per row.
// The transform is separable:  D(p) = min_z' [ wz dz^2 + min_y' [ wy dy^2 + min_x' wx dx^2 ] ].
//   k_dist_rows        f1(x, y, z) = wx * g^2, g the distance along x to the nearest site of the row, straight from the bits: inside
//                      the voxel's own word by count-leading / count-trailing zeros, across words by a wave-wide look at 64 words a time
//   k_dist_lines_scan  one axis (y, then z): out(j) = min_i f(i) + w (j - i)^2 on every line by two linear scans, src -> dst (two
//                      buffers: a pass never reads what it writes, whatever the line's length): the map's passes
//   k_dist_lines<0>    the same pass by a search outward from every voxel: the morphology's pass along y (and the map's under
//                      CLWH_TUNE_DIST_LINES=search)
//   k_dist_lines<1>    ... and the morphology's last pass: the map is not written, the comparison with radius_sq is, as one 64-bit
//                      word of the mask per wave
//   k_mask_combine     a word of out from a word of a and b
// In the search, the envelope of the parabolas is found outward from i = j: candidates at distance k cost at least w k^2 because
// f >= 0, so the search ends as soon as w k^2 >= the running best (or > cap): exact, no stack, sqrt(D / w) steps per voxel.  A lane
// is one voxel, a wave 64 consecutive x, so every load and store of a step is one coalesced 256-byte row.
// Integers only.  A finite value is at most 2^32 - 2 (the weights' rule), NONE = 2^32 - 1 is "no site (within cap)"; NONE is widened
// to an infinity of 64 bits before anything is added to it, and every sum and product is 64-bit.
#include "mask_device.hpp"

namespace clvr {

namespace {

using u64 = unsigned long long;
constexpr u64 kInf = ~0ull;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr u64 kMaxFinite = 0xFFFFFFFEull;

// word i of a row's sites: the mask's word (complemented for "distance to clear"), without the bits at x >= X
__device__ __forceinline__ u64 site_word(const u64 *__restrict__ row, int32_t i, int32_t W64, int32_t X, int32_t flip) {
  u64 v = row[i];
  if (flip) v = ~v;
  if (i == W64 - 1 && (X & 63) != 0) v &= (1ull << (X & 63)) - 1ull;
  return v;
}

}  // namespace

// a thread per voxel of the padded row (W64 * 64), a wave per 64-bit word
__global__ __launch_bounds__(256) void k_dist_rows(const u64 *__restrict__ mask, uint32_t *__restrict__ out, int32_t X, size_t rows,
                                                   int32_t W64, int32_t flip, u64 wx, u64 cap) {
  const size_t padded = (size_t)W64 * 64u, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= padded * rows) return;  // (whole waves: padded is a multiple of 64)
  const size_t r = id / padded;
  const int32_t x = (int32_t)(id - r * padded), w = x >> 6, b = x & 63, lane = (int32_t)(threadIdx.x & 63u);
  const u64 *row = mask + r * (size_t)W64;
  const u64 own = site_word(row, w, W64, X, flip);

  // the nearest word with a site before and behind this one, 64 words a look; a word k places away is at least 64 (k - 1) + 1 voxels
  // from every lane, so the look ends where that is beyond cap
  int32_t wl = -1, wr = -1;
  for (int32_t base = w - 1; base >= 0; base -= 64) {
    const u64 reach = (u64)(w - 1 - base) * 64u + 1u;
    if (wx * reach * reach > cap) break;
    const int32_t i = base - lane;
    const u64 v = i >= 0 ? site_word(row, i, W64, X, flip) : 0ull;
    const u64 found = __ballot(v != 0ull);
    if (found != 0ull) {
      wl = base - (int32_t)__builtin_ctzll(found);
      break;
    }
  }
  for (int32_t base = w + 1; base < W64; base += 64) {
    const u64 reach = (u64)(base - w - 1) * 64u + 1u;
    if (wx * reach * reach > cap) break;
    const int32_t i = base + lane;
    const u64 v = i < W64 ? site_word(row, i, W64, X, flip) : 0ull;
    const u64 found = __ballot(v != 0ull);
    if (found != 0ull) {
      wr = base + (int32_t)__builtin_ctzll(found);
      break;
    }
  }

  u64 g = kInf;
  const u64 below = own & (~0ull >> (63 - b)), above = own >> b;  // sites at or before x, at or behind x
  if (below != 0ull) g = (u64)(b - (63 - (int32_t)__builtin_clzll(below)));
  else if (wl >= 0) g = (u64)(x - (wl * 64 + 63 - (int32_t)__builtin_clzll(site_word(row, wl, W64, X, flip))));
  u64 g2 = kInf;
  if (above != 0ull) g2 = (u64)__builtin_ctzll(above);
  else if (wr >= 0) g2 = (u64)(wr * 64 + (int32_t)__builtin_ctzll(site_word(row, wr, W64, X, flip)) - x);
  g = g < g2 ? g : g2;
  if (x >= X) return;
  const u64 d = g == kInf ? kInf : wx * g * g;  // g <= X - 1: at most 2^32 - 2
  out[r * (size_t)X + (size_t)x] = d <= cap && d <= kMaxFinite ? (uint32_t)d : kNone;
}

// One axis.  A thread per voxel of the padded row; the line of voxel (x, j) is src[base + i * stride], i = 0 .. n - 1.
// BITS: bit(x) = inside != (value <= cap) for x < X, written as the wave's word of `bits` (clean padding); else dst = value or NONE.
template <bool BITS>
__global__ __launch_bounds__(256) void k_dist_lines(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, u64 *__restrict__ bits,
                                                    int32_t X, int32_t Y, size_t rows, int32_t W64, int32_t along_z, u64 w, u64 cap,
                                                    int32_t invert) {
  const size_t padded = (size_t)W64 * 64u, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= padded * rows) return;  // (whole waves)
  const size_t r = id / padded;
  const int32_t x = (int32_t)(id - r * padded);
  bool within = false;
  uint32_t value = kNone;
  if (x < X) {
    const size_t z = r / (size_t)Y, y = r - z * (size_t)Y;
    const int64_t j = along_z ? (int64_t)z : (int64_t)y, n = along_z ? (int64_t)(rows / (size_t)Y) : (int64_t)Y;
    const int64_t stride = along_z ? (int64_t)X * Y : (int64_t)X;
    const uint32_t *p = src + r * (size_t)X + (size_t)x;
    const uint32_t f = *p;
    u64 best = f == kNone ? kInf : (u64)f;
    const u64 stop = cap == kInf ? kInf : cap + 1u;  // nothing at w k^2 > cap can count
    for (int64_t k = 1;; ++k) {
      const u64 wk = w * (u64)k * (u64)k;  // k <= n - 1: at most 2^32 - 2
      if (wk >= (best < stop ? best : stop)) break;
      const bool lo = j - k >= 0, hi = j + k < n;
      if (!lo && !hi) break;
      if (lo) {
        const uint32_t v = p[-k * stride];
        if (v != kNone && (u64)v + wk < best) best = (u64)v + wk;
      }
      if (hi) {
        const uint32_t v = p[k * stride];
        if (v != kNone && (u64)v + wk < best) best = (u64)v + wk;
      }
    }
    within = best <= cap && best <= kMaxFinite;
    value = within ? (uint32_t)best : kNone;
    if (!BITS) dst[r * (size_t)X + (size_t)x] = value;
  }
  if (BITS) {
    const u64 word = __ballot(x < X && within != (invert != 0));
    if ((threadIdx.x & 63u) == 0u) bits[id >> 6] = word;
  }
}

// The same pass by Meijster's two linear scans, a thread per LINE (lanes are 64 consecutive x, so a step's loads of src are
// coalesced): the first scan keeps the stack of the parabolas that own a stretch of the lower envelope, (s, t) = (the parabola's
// index, the first position it owns); the second walks back and reads the envelope off.  O(n) per line whatever the data.  A
// parabola with f = NONE owns nothing and is never pushed.  All of it in signed 64 bits: values below 2^34, Sep's numerator below 2^35.
//   parabola i is at or below parabola u > i at x  <=>  x <= Sep(i, u) = floor((f(u) - f(i) + w (u^2 - i^2)) / (2 w (u - i)))
// The stack lives in two maps laid out like the volume, slot q of a line at the line's voxel q: `stack_s`, and dst itself for t --
// dst's words are dead until the second scan writes them, and that scan writes voxel u only when every slot above it is popped
// (t grows with the slot, so slot q has t >= q, and the top is in registers before its own word is overwritten).  dst != src.
__global__ __launch_bounds__(256) void k_dist_lines_scan(const uint32_t *__restrict__ src, uint32_t *dst, uint32_t *__restrict__ stack_s,
                                                         int32_t X, int32_t Y, int32_t Z, int32_t W64, int32_t along_z, long long w,
                                                         u64 cap) {
  const size_t padded = (size_t)W64 * 64u, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  const size_t lines = along_z ? (size_t)Y : (size_t)Z;  // per x
  if (id >= padded * lines) return;
  const size_t o = id / padded;
  const int32_t x = (int32_t)(id - o * padded);
  if (x >= X) return;
  const long long n = along_z ? Z : Y;
  const size_t stride = along_z ? (size_t)X * (size_t)Y : (size_t)X;
  const size_t base = (along_z ? o * (size_t)X : o * (size_t)X * (size_t)Y) + (size_t)x;
  long long q = -1, si = 0, ti = 0, gi = 0;  // the stack's height - 1 and its top: index, first position owned, f(index)
  for (long long u = 0; u < n; ++u) {
    const uint32_t word = src[base + (size_t)u * stride];
    if (word == kNone) continue;
    const long long gu = (long long)word;
    while (q >= 0) {  // the top owns nothing any more if u is below it where its stretch begins
      const long long a = ti - si, b = ti - u;
      if (gi + w * a * a <= gu + w * b * b) break;
      if (--q >= 0) {
        si = (long long)stack_s[base + (size_t)q * stride];
        ti = (long long)dst[base + (size_t)q * stride];
        gi = (long long)src[base + (size_t)si * stride];
      }
    }
    long long first = 0;
    if (q >= 0) {
      const long long num = gu - gi + w * (u * u - si * si), den = 2 * w * (u - si);
      first = (num >= 0 ? num / den : -((-num + den - 1) / den)) + 1;  // floor, + 1
      if (first >= n) continue;  // u is nowhere below the envelope inside the line
    }
    ++q;
    si = u;
    ti = first;
    gi = gu;
    stack_s[base + (size_t)q * stride] = (uint32_t)u;
    dst[base + (size_t)q * stride] = (uint32_t)first;
  }
  for (long long u = n - 1; u >= 0; --u) {
    u64 value = kInf;
    if (q >= 0) value = (u64)(gi + w * (u - si) * (u - si));
    const bool pop = q >= 0 && u == ti;
    if (pop && --q >= 0) {  // (the new top is read before this voxel's word, which may be its slot's neighbour but never its slot)
      si = (long long)stack_s[base + (size_t)q * stride];
      ti = (long long)dst[base + (size_t)q * stride];
      gi = (long long)src[base + (size_t)si * stride];
    }
    dst[base + (size_t)u * stride] = value <= cap && value <= kMaxFinite ? (uint32_t)value : kNone;
  }
}

// op: CLWH_MASK_AND .. CLWH_MASK_NOT; a thread per 64-bit word; out may be a or b (a thread reads its words before it writes)
__global__ __launch_bounds__(256) void k_mask_combine(const u64 *a, const u64 *b, u64 *out, int32_t X, size_t words, int32_t W64, int32_t op) {
  const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= words) return;
  const u64 va = a[id], vb = op == CLWH_MASK_NOT ? 0ull : b[id];
  u64 v;
  switch (op) {
    case CLWH_MASK_AND: v = va & vb; break;
    case CLWH_MASK_OR: v = va | vb; break;
    case CLWH_MASK_XOR: v = va ^ vb; break;
    case CLWH_MASK_ANDNOT: v = va & ~vb; break;
    default: v = ~va; break;
  }
  if ((X & 63) != 0 && id % (size_t)W64 == (size_t)(W64 - 1)) v &= (1ull << (X & 63)) - 1ull;
  out[id] = v;
}

hipError_t launch_dist_rows(const DistArgs &a, const unsigned long long *mask, uint32_t *out, int32_t flip, hipStream_t s) {
  const size_t rows = (size_t)a.Y * (size_t)a.Z;
  hipLaunchKernelGGL(k_dist_rows, dim3(blocks_for(rows * (size_t)a.W64 * 64u)), dim3(256), 0, s, mask, out, a.X, rows, a.W64, flip,
                     (u64)a.weight[0], a.cap);
  return hipGetLastError();
}

hipError_t launch_dist_lines(const DistArgs &a, const uint32_t *src, uint32_t *dst, int32_t along_z, hipStream_t s) {
  const size_t rows = (size_t)a.Y * (size_t)a.Z;
  hipLaunchKernelGGL(k_dist_lines<false>, dim3(blocks_for(rows * (size_t)a.W64 * 64u)), dim3(256), 0, s, src, dst, (u64 *)nullptr, a.X, a.Y,
                     rows, a.W64, along_z, (u64)a.weight[along_z ? 2 : 1], a.cap, 0);
  return hipGetLastError();
}

hipError_t launch_dist_lines_scan(const DistArgs &a, const uint32_t *src, uint32_t *dst, uint32_t *stack, int32_t along_z, hipStream_t s) {
  const size_t lines = along_z ? (size_t)a.Y : (size_t)a.Z;
  hipLaunchKernelGGL(k_dist_lines_scan, dim3(blocks_for(lines * (size_t)a.W64 * 64u)), dim3(256), 0, s, src, dst, stack, a.X, a.Y, a.Z, a.W64,
                     along_z, (long long)a.weight[along_z ? 2 : 1], a.cap);
  return hipGetLastError();
}

hipError_t launch_dist_lines_bits(const DistArgs &a, const uint32_t *src, unsigned long long *bits, int32_t invert, hipStream_t s) {
  const size_t rows = (size_t)a.Y * (size_t)a.Z;
  hipLaunchKernelGGL(k_dist_lines<true>, dim3(blocks_for(rows * (size_t)a.W64 * 64u)), dim3(256), 0, s, src, (uint32_t *)nullptr, bits, a.X,
                     a.Y, rows, a.W64, 1, (u64)a.weight[2], a.cap, invert);
  return hipGetLastError();
}

hipError_t launch_mask_combine(const unsigned long long *a, const unsigned long long *b, unsigned long long *out, int32_t X, int32_t Y,
                               int32_t Z, int32_t W64, int32_t op, hipStream_t s) {
  const size_t words = (size_t)W64 * (size_t)Y * (size_t)Z;
  hipLaunchKernelGGL(k_mask_combine, dim3(blocks_for(words)), dim3(256), 0, s, a, b, out, X, words, W64, op);
  return hipGetLastError();
}

}  // namespace clvr
