// region_stats_kernels.hip -- the exact statistics of a mask's region and of every rank of a labelling (clwh_mask_statistics,
// clwh_label_statistics; host side clwh_region_stats.hip).  Integers only: sums, extremes and counts commute, so the order in which
// lanes, waves and blocks add their parts does not show in the result.  A record is accumulated in the layout of clwh_region_stats with
// the extremes and bbox_lo at their identities and bbox_hi inclusive (k_stats_init), and brought into its final form by k_stats_finish.
#include "mask_device.hpp"

namespace clvr {

namespace {

using u64 = unsigned long long;

// clwh_region_stats as the atomics see it
struct RegionRec {
  u64 count, sum, sum_sq;  // sum: int64 in two's complement
  int32_t vmin, vmax;
  u64 pos[3];
  uint32_t lo[3], hi[3];   // hi inclusive until k_stats_finish
  uint32_t faces[3], border[3];
};
static_assert(sizeof(RegionRec) == sizeof(clwh_region_stats) && sizeof(RegionRec) == 104, "one layout");

// what a lane, a wave or a block holds of one region: a block sees fewer than 2^31 voxels, so its counts fit 32 bits
struct Partial {
  uint32_t count;
  long long sum;
  u64 sum_sq;
  int32_t vmin, vmax;
  u64 pos[3];
  uint32_t lo[3], hi[3];
  uint32_t faces[3], border[3];
};

__device__ __forceinline__ void partial_reset(Partial &p) {
  p.count = 0u;
  p.sum = 0;
  p.sum_sq = 0ull;
  p.vmin = 0x7fffffff;
  p.vmax = -0x7fffffff - 1;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    p.pos[q] = 0ull;
    p.lo[q] = 0xFFFFFFFFu;
    p.hi[q] = 0u;
    p.faces[q] = 0u;
    p.border[q] = 0u;
  }
}

// a part into its record in memory: vector atomics, only for the fields that change
__device__ __forceinline__ void global_add(RegionRec *r, const Partial &p) {
  if (p.count) {
    atomicAdd(&r->count, (u64)p.count);
    atomicAdd(&r->sum, (u64)p.sum);
    atomicAdd(&r->sum_sq, p.sum_sq);
    atomicMin(&r->vmin, p.vmin);
    atomicMax(&r->vmax, p.vmax);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (p.pos[q]) atomicAdd(&r->pos[q], p.pos[q]);
      atomicMin(&r->lo[q], p.lo[q]);
      atomicMax(&r->hi[q], p.hi[q]);
      if (p.border[q]) atomicAdd(&r->border[q], p.border[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (p.faces[q]) atomicAdd(&r->faces[q], p.faces[q]);
}

__device__ __forceinline__ uint32_t shfl_u32(uint32_t v, int off) { return (uint32_t)__shfl_xor((int)v, off); }

__device__ __forceinline__ void wave_reduce(Partial &p) {
  for (int off = 32; off > 0; off >>= 1) {
    p.count += shfl_u32(p.count, off);
    p.sum += __shfl_xor(p.sum, off);
    p.sum_sq += __shfl_xor(p.sum_sq, off);
    p.vmin = min(p.vmin, __shfl_xor(p.vmin, off));
    p.vmax = max(p.vmax, __shfl_xor(p.vmax, off));
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      p.pos[q] += __shfl_xor(p.pos[q], off);
      p.lo[q] = min(p.lo[q], shfl_u32(p.lo[q], off));
      p.hi[q] = max(p.hi[q], shfl_u32(p.hi[q], off));
      p.faces[q] += shfl_u32(p.faces[q], off);
      p.border[q] += shfl_u32(p.border[q], off);
    }
  }
}

__device__ __forceinline__ void partial_merge(Partial &s, const Partial &p) {
  s.count += p.count;
  s.sum += p.sum;
  s.sum_sq += p.sum_sq;
  s.vmin = min(s.vmin, p.vmin);
  s.vmax = max(s.vmax, p.vmax);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    s.pos[q] += p.pos[q];
    s.lo[q] = min(s.lo[q], p.lo[q]);
    s.hi[q] = max(s.hi[q], p.hi[q]);
    s.faces[q] += p.faces[q];
    s.border[q] += p.border[q];
  }
}

// ---- the mask path: k_grow_reduce's walk (a lane takes a byte of the mask, 8 voxels, in a grid-stride loop) with the positions, the
// faces from the bits alone, and the histogram in k_tf_sort_values' LDS hash (its slot count was measured there)
constexpr int kHistSlotsLog2 = 12, kHistSlots = 1 << kHistSlotsLog2;

template <bool ROWS8, bool HIST>
__global__ __launch_bounds__(256) void k_mask_stats(const MaskStatsArgs a) {
  __shared__ int s_key[HIST ? kHistSlots : 1];
  __shared__ uint32_t s_cnt[HIST ? kHistSlots : 1];
  if (HIST) {
    for (int i = (int)threadIdx.x; i < kHistSlots; i += 256) {
      s_key[i] = -1;
      s_cnt[i] = 0u;
    }
    __syncthreads();
  }
  // open addressing, keys never leave once set, counts by LDS atomics; a bin that finds its probe window taken goes to memory directly
  auto hist_add = [&](int bin, uint32_t c) {
    unsigned slot = ((unsigned)bin * 2654435761u) >> (32 - kHistSlotsLog2);
    for (int probe = 0; probe < 4; ++probe) {
      int k = s_key[slot];
      if (k == -1) {
        const int old = atomicCAS(&s_key[slot], -1, bin);
        k = old == -1 ? bin : old;
      }
      if (k == bin) {
        atomicAdd(&s_cnt[slot], c);
        return;
      }
      slot = (slot + 1u) & (unsigned)(kHistSlots - 1);
    }
    atomicAdd(&a.hist[bin], (u64)c);
  };

  const size_t bytes_per_row = (size_t)a.W64 * 8u, total = bytes_per_row * (size_t)a.Y * (size_t)a.Z;
  const uint32_t X = (uint32_t)a.X, Y = (uint32_t)a.Y, Z = (uint32_t)a.Z;
  Partial s;
  partial_reset(s);
  uint32_t below = 0u, above = 0u;
  for (size_t id = (size_t)blockIdx.x * 256u + threadIdx.x; id < total; id += (size_t)gridDim.x * 256u) {
    const size_t row = id / bytes_per_row;
    const uint32_t x0 = (uint32_t)(id - row * bytes_per_row) * 8u;
    if (x0 >= X) continue;  // a padding byte: whatever it holds
    const uint32_t rem = X - x0, valid = rem >= 8u ? 0xFFu : ((1u << rem) - 1u);
    const uint32_t z = (uint32_t)(row / (size_t)Y), y = (uint32_t)(row - (size_t)z * (size_t)Y);
    const uint32_t m = (uint32_t)a.mask[id] & valid;
    // faces: the bits against themselves shifted by one (bit 0 of the next byte carried in), against row y + 1 and against row z + 1
    const uint32_t next = rem > 8u ? ((uint32_t)a.mask[id + 1u] & 1u) : 0u;
    const uint32_t pairs = rem > 8u ? 0xFFu : (valid >> 1);  // bit h: voxel x0 + h + 1 exists
    const uint32_t m9 = m | (next << 8);
    s.faces[0] += (uint32_t)__popc((m9 ^ (m9 >> 1)) & pairs);
    if (y + 1u < Y) s.faces[1] += (uint32_t)__popc(m ^ ((uint32_t)a.mask[id + bytes_per_row] & valid));
    if (z + 1u < Z) s.faces[2] += (uint32_t)__popc(m ^ ((uint32_t)a.mask[id + bytes_per_row * (size_t)Y] & valid));
    if (!m) continue;
    const int16_t *p = a.volume + row * (size_t)X + (size_t)x0;
    int v[8];
    if (ROWS8) {
      load8(p, v);
    } else {
#pragma unroll
      for (int h = 0; h < 8; ++h) v[h] = ((m >> h) & 1u) ? (int)p[h] : 0;
    }
    int run_bin = -1;
    uint32_t run_count = 0u, offsets = 0u;
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      if (!((m >> h) & 1u)) continue;
      offsets += (uint32_t)h;
      s.sum += v[h];
      s.sum_sq += (u64)((long long)v[h] * (long long)v[h]);
      s.vmin = min(s.vmin, v[h]);
      s.vmax = max(s.vmax, v[h]);
      if (HIST) {
        const int d = v[h] - a.hist_lo;  // both within int16: no overflow
        if (d < 0) {
          ++below;
        } else {
          const uint32_t b = a.bin_width == 1u ? (uint32_t)d : (uint32_t)d / a.bin_width;
          if (b >= a.n_bins) {
            ++above;
          } else {
            if ((int)b != run_bin) {  // neighbouring voxels mostly share a bin: one table update per run
              if (run_count) hist_add(run_bin, run_count);
              run_bin = (int)b;
              run_count = 0u;
            }
            ++run_count;
          }
        }
      }
    }
    if (HIST && run_count) hist_add(run_bin, run_count);
    const uint32_t c = (uint32_t)__popc(m);
    s.count += c;
    s.pos[0] += (u64)c * x0 + offsets;
    s.pos[1] += (u64)c * y;
    s.pos[2] += (u64)c * z;
    s.lo[0] = min(s.lo[0], x0 + (uint32_t)(__ffs((int)m) - 1));
    s.hi[0] = max(s.hi[0], x0 + (uint32_t)(31 - __clz((int)m)));
    s.lo[1] = min(s.lo[1], y);
    s.hi[1] = max(s.hi[1], y);
    s.lo[2] = min(s.lo[2], z);
    s.hi[2] = max(s.hi[2], z);
    s.border[0] += (x0 == 0u ? (m & 1u) : 0u) + (rem <= 8u ? ((m >> (rem - 1u)) & 1u) : 0u);
    s.border[1] += c * ((y == 0u ? 1u : 0u) + (y + 1u == Y ? 1u : 0u));
    s.border[2] += c * ((z == 0u ? 1u : 0u) + (z + 1u == Z ? 1u : 0u));
  }

  wave_reduce(s);
  if (HIST) {
    for (int off = 32; off > 0; off >>= 1) {
      below += shfl_u32(below, off);
      above += shfl_u32(above, off);
    }
  }
  __shared__ Partial part[4];
  __shared__ uint32_t tails[4][2];
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
    part[wave] = s;
    tails[wave][0] = below;
    tails[wave][1] = above;
  }
  __syncthreads();  // (also: every count of the block's histogram is in LDS)
  if (HIST) {
    for (int i = (int)threadIdx.x; i < kHistSlots; i += 256)
      if (s_key[i] >= 0 && s_cnt[i] != 0u) atomicAdd(&a.hist[s_key[i]], (u64)s_cnt[i]);
  }
  if (threadIdx.x != 0u) return;
  Partial sum = part[0];
  for (int w = 1; w < 4; ++w) partial_merge(sum, part[w]);
  global_add(reinterpret_cast<RegionRec *>(a.result), sum);
  if (HIST) {
    const uint32_t lo = tails[0][0] + tails[1][0] + tails[2][0] + tails[3][0], hi = tails[0][1] + tails[1][1] + tails[2][1] + tails[3][1];
    if (lo) atomicAdd(&a.tails[0], (u64)lo);
    if (hi) atomicAdd(&a.tails[1], (u64)hi);
  }
}

// ---- the label path.  A lane takes eight consecutive voxels of a row and keeps ONE part in registers for as long as the valid ranks it
// meets stay the same, across its whole grid-stride walk (rank 0 and ranks above the capacity are dropped as they are read and do not
// end it): with one rank that owns the volume a lane adds to shared words once, at the end.  A part that ends goes into the block's LDS
// hash of whole records (kLabelSlots of them, 27 KB: four blocks per CU); when the table is three quarters full the block
// writes it out and starts afresh, so millions of small ranks pass through it and the large ones between them stay resident.  A rank
// that finds its probe window taken goes to memory directly.  Faces go to the voxel's own record: it compares its rank with all six
// neighbours (a neighbour outside the volume is replaced by the voxel's own rank: no face), so a part never touches a second record.
constexpr int kLabelSlotsLog2 = 8, kLabelSlots = 1 << kLabelSlotsLog2;
struct LabelTable {
  uint32_t key[kLabelSlots];  // the rank, 0: free
  uint32_t count[kLabelSlots];
  u64 sum[kLabelSlots], sum_sq[kLabelSlots], pos[3][kLabelSlots];
  int32_t vmin[kLabelSlots], vmax[kLabelSlots];
  uint32_t lo[3][kLabelSlots], hi[3][kLabelSlots], faces[3][kLabelSlots], border[3][kLabelSlots];
  uint32_t used;
};

__device__ __forceinline__ void table_reset(LabelTable &t, int i) {
  t.key[i] = 0u;
  t.count[i] = 0u;
  t.sum[i] = 0ull;
  t.sum_sq[i] = 0ull;
  t.vmin[i] = 0x7fffffff;
  t.vmax[i] = -0x7fffffff - 1;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    t.pos[q][i] = 0ull;
    t.lo[q][i] = 0xFFFFFFFFu;
    t.hi[q][i] = 0u;
    t.faces[q][i] = 0u;
    t.border[q][i] = 0u;
  }
}

__device__ __forceinline__ void table_add(LabelTable &t, uint32_t rank, const Partial &p, RegionRec *stats, bool direct) {
  if (direct) {  // (the experiment without the table: CLWH_TUNE_LABEL_STATS=direct)
    global_add(&stats[rank - 1u], p);
    return;
  }
  unsigned slot = (rank * 2654435761u) >> (32 - kLabelSlotsLog2);
  for (int probe = 0; probe < 8; ++probe) {
    uint32_t k = t.key[slot];
    if (k == 0u) {
      const uint32_t old = atomicCAS(&t.key[slot], 0u, rank);
      if (old == 0u) atomicAdd(&t.used, 1u);
      k = old == 0u ? rank : old;
    }
    if (k == rank) {
      atomicAdd(&t.count[slot], p.count);
      atomicAdd(&t.sum[slot], (u64)p.sum);
      atomicAdd(&t.sum_sq[slot], p.sum_sq);
      atomicMin(&t.vmin[slot], p.vmin);
      atomicMax(&t.vmax[slot], p.vmax);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (p.pos[q]) atomicAdd(&t.pos[q][slot], p.pos[q]);
        atomicMin(&t.lo[q][slot], p.lo[q]);
        atomicMax(&t.hi[q][slot], p.hi[q]);
        if (p.faces[q]) atomicAdd(&t.faces[q][slot], p.faces[q]);
        if (p.border[q]) atomicAdd(&t.border[q][slot], p.border[q]);
      }
      return;
    }
    slot = (slot + 1u) & (unsigned)(kLabelSlots - 1);
  }
  global_add(&stats[rank - 1u], p);
}

// every thread of the block: the table into memory, and empty again
__device__ __forceinline__ void table_flush(LabelTable &t, RegionRec *stats) {
  __syncthreads();
  for (int i = (int)threadIdx.x; i < kLabelSlots; i += 256) {
    const uint32_t rank = t.key[i];
    if (rank == 0u) continue;
    Partial p;
    p.count = t.count[i];
    p.sum = (long long)t.sum[i];
    p.sum_sq = t.sum_sq[i];
    p.vmin = t.vmin[i];
    p.vmax = t.vmax[i];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      p.pos[q] = t.pos[q][i];
      p.lo[q] = t.lo[q][i];
      p.hi[q] = t.hi[q][i];
      p.faces[q] = t.faces[q][i];
      p.border[q] = t.border[q][i];
    }
    global_add(&stats[rank - 1u], p);
    table_reset(t, i);
  }
  if (threadIdx.x == 0u) t.used = 0u;
  __syncthreads();
}

// eight words of a row: two 16-byte loads, or one by one with `own` where the row has ended
template <bool ROWS8>
__device__ __forceinline__ void labels_load8(const uint32_t *p, uint32_t rem, uint32_t (&w)[8]) {
  if (ROWS8) {
    const uint4 lo = reinterpret_cast<const uint4 *>(p)[0], hi = reinterpret_cast<const uint4 *>(p)[1];
    w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
    w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
  } else {
#pragma unroll
    for (int h = 0; h < 8; ++h) w[h] = (uint32_t)h < rem ? p[h] : 0u;
  }
}

template <bool ROWS8>
__global__ __launch_bounds__(256) void k_label_stats(const LabelStatsArgs a) {
  __shared__ LabelTable t;
  RegionRec *const stats = reinterpret_cast<RegionRec *>(a.stats);
  for (int i = (int)threadIdx.x; i < kLabelSlots; i += 256) table_reset(t, i);
  if (threadIdx.x == 0u) t.used = 0u;
  __syncthreads();

  const uint32_t X = (uint32_t)a.X, Y = (uint32_t)a.Y, Z = (uint32_t)a.Z, cap = a.capacity;
  const size_t per_row = ((size_t)X + 7u) / 8u, n_items = per_row * (size_t)Y * (size_t)Z, slice = (size_t)X * (size_t)Y;
  Partial cur;
  partial_reset(cur);
  uint32_t cur_rank = 0u;
  const bool direct = a.mode == 2, per_item = a.mode == 1;
  for (size_t base = (size_t)blockIdx.x * 256u; base < n_items; base += (size_t)gridDim.x * 256u) {  // (the same trips for every thread)
    if (__syncthreads_or(t.used > (uint32_t)(kLabelSlots * 3 / 4))) table_flush(t, stats);
    const size_t item = base + threadIdx.x;
    if (item >= n_items) continue;
    const size_t row = item / per_row;
    const uint32_t x0 = (uint32_t)(item - row * per_row) * 8u, rem = X - x0;
    const uint32_t z = (uint32_t)(row / (size_t)Y), y = (uint32_t)(row - (size_t)z * (size_t)Y);
    const size_t at = row * (size_t)X + (size_t)x0;
    uint32_t own[8];
    labels_load8<ROWS8>(a.labels + at, rem, own);
    bool any = false;
#pragma unroll
    for (int h = 0; h < 8; ++h) any = any || (own[h] - 1u < cap);
    if (!any) continue;

    int v[8];
    if (ROWS8) {
      load8(a.volume + at, v);
    } else {
#pragma unroll
      for (int h = 0; h < 8; ++h) v[h] = (uint32_t)h < rem ? (int)a.volume[at + (size_t)h] : 0;
    }
    // the neighbours' ranks; where the volume ends, the voxel's own (no face)
    uint32_t ym[8], yp[8], zm[8], zp[8];
    if (y > 0u) {
      labels_load8<ROWS8>(a.labels + at - (size_t)X, rem, ym);
    } else {
#pragma unroll
      for (int h = 0; h < 8; ++h) ym[h] = own[h];
    }
    if (y + 1u < Y) {
      labels_load8<ROWS8>(a.labels + at + (size_t)X, rem, yp);
    } else {
#pragma unroll
      for (int h = 0; h < 8; ++h) yp[h] = own[h];
    }
    if (z > 0u) {
      labels_load8<ROWS8>(a.labels + at - slice, rem, zm);
    } else {
#pragma unroll
      for (int h = 0; h < 8; ++h) zm[h] = own[h];
    }
    if (z + 1u < Z) {
      labels_load8<ROWS8>(a.labels + at + slice, rem, zp);
    } else {
#pragma unroll
      for (int h = 0; h < 8; ++h) zp[h] = own[h];
    }
    const uint32_t before = x0 > 0u ? a.labels[at - 1u] : own[0];
    const uint32_t after = rem > 8u ? a.labels[at + 8u] : own[7];  // (own[7] is only compared where voxel x0 + 7 exists)

#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const uint32_t rank = own[h], x = x0 + (uint32_t)h;
      if ((uint32_t)h >= rem || rank - 1u >= cap) continue;
      if (rank != cur_rank) {
        if (cur_rank) table_add(t, cur_rank, cur, stats, direct);
        cur_rank = rank;
        partial_reset(cur);
      }
      const uint32_t xm = h > 0 ? own[h > 0 ? h - 1 : 0] : before;
      const uint32_t xp = (uint32_t)h + 1u >= rem ? rank : (h < 7 ? own[h < 7 ? h + 1 : 7] : after);
      ++cur.count;
      cur.sum += v[h];
      cur.sum_sq += (u64)((long long)v[h] * (long long)v[h]);
      cur.vmin = min(cur.vmin, v[h]);
      cur.vmax = max(cur.vmax, v[h]);
      cur.pos[0] += x;
      cur.pos[1] += y;
      cur.pos[2] += z;
      cur.lo[0] = min(cur.lo[0], x);
      cur.hi[0] = max(cur.hi[0], x);
      cur.lo[1] = min(cur.lo[1], y);
      cur.hi[1] = max(cur.hi[1], y);
      cur.lo[2] = min(cur.lo[2], z);
      cur.hi[2] = max(cur.hi[2], z);
      cur.faces[0] += (xm != rank ? 1u : 0u) + (xp != rank ? 1u : 0u);
      cur.faces[1] += (ym[h] != rank ? 1u : 0u) + (yp[h] != rank ? 1u : 0u);
      cur.faces[2] += (zm[h] != rank ? 1u : 0u) + (zp[h] != rank ? 1u : 0u);
      cur.border[0] += (x == 0u ? 1u : 0u) + (x + 1u == X ? 1u : 0u);
      cur.border[1] += (y == 0u ? 1u : 0u) + (y + 1u == Y ? 1u : 0u);
      cur.border[2] += (z == 0u ? 1u : 0u) + (z + 1u == Z ? 1u : 0u);
    }
    if (per_item && cur_rank) {  // (the experiment without the part that outlives its eight voxels: CLWH_TUNE_LABEL_STATS=item)
      table_add(t, cur_rank, cur, stats, direct);
      cur_rank = 0u;
    }
  }
  if (cur_rank) table_add(t, cur_rank, cur, stats, direct);
  table_flush(t, stats);
}

// ---- records before and after the sums: the identities; then the empty record for a region without voxels, bbox_hi exclusive
__global__ __launch_bounds__(256) void k_stats_init(RegionRec *stats, uint32_t n) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  RegionRec r;
  r.count = r.sum = r.sum_sq = 0ull;
  r.vmin = 0x7fffffff;
  r.vmax = -0x7fffffff - 1;
  for (int q = 0; q < 3; ++q) {
    r.pos[q] = 0ull;
    r.lo[q] = 0xFFFFFFFFu;
    r.hi[q] = r.faces[q] = r.border[q] = 0u;
  }
  stats[k] = r;
}

__global__ __launch_bounds__(256) void k_stats_finish(RegionRec *stats, uint32_t n) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  RegionRec *r = &stats[k];
  if (r->count == 0ull) {  // (faces and border faces of no voxels are 0 already)
    r->vmin = r->vmax = 0;
    for (int q = 0; q < 3; ++q) r->lo[q] = 0u;
  } else {
    for (int q = 0; q < 3; ++q) r->hi[q] += 1u;
  }
}

}  // namespace

hipError_t launch_stats_init(clwh_region_stats *stats, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_stats_init, dim3(blocks_for(n)), dim3(256), 0, s, reinterpret_cast<RegionRec *>(stats), n);
  return hipGetLastError();
}

hipError_t launch_stats_finish(clwh_region_stats *stats, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_stats_finish, dim3(blocks_for(n)), dim3(256), 0, s, reinterpret_cast<RegionRec *>(stats), n);
  return hipGetLastError();
}

hipError_t launch_mask_stats(const MaskStatsArgs &a, hipStream_t s) {
  const size_t bytes = (size_t)a.Y * (size_t)a.Z * (size_t)a.W64 * 8u;
  const unsigned need = blocks_for(bytes), grid = need < 2048u ? need : 2048u;
  const bool rows8 = rows_of_8(a.volume, a.X);
  auto kernel = a.hist ? (rows8 ? k_mask_stats<true, true> : k_mask_stats<false, true>) : (rows8 ? k_mask_stats<true, false> : k_mask_stats<false, false>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_label_stats(const LabelStatsArgs &a, hipStream_t s) {
  const size_t items = (((size_t)a.X + 7u) / 8u) * (size_t)a.Y * (size_t)a.Z;
  // four blocks per CU hold their tables (27 KB each); a grid of that size walks the volume
  const unsigned need = blocks_for(items), grid = need < 1024u ? need : 1024u;
  const bool rows8 = rows_of_8(a.volume, a.X) && aligned16(a.labels);
  hipLaunchKernelGGL(rows8 ? k_label_stats<true> : k_label_stats<false>, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
