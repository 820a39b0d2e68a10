// label_kernels.hip -- connected-component labelling (clwh_segment_label) and rank selections (clwh_labels_to_mask), gfx950.
// The unit of work is a RUN: a maximal stretch of set bits inside one 64-bit word of the admissible image A (grow's bit rows: W64 words
// per row).  A run is named by the flat index of its first voxel, and that voxel's word of the caller's `labels` buffer is the run's
// parent word; the other words of `labels` are not read before the last kernel writes all of them.  So the union-find needs no memory
// of its own, and CT data (long runs) has an order of magnitude fewer units than voxels.
//   k_label_admissible(8)  A = window & box (& the caller's mask, read only)
//   k_label_init           parent(run) = run
//   k_label_merge          every run is united with the runs it touches in the word before it and in the earlier rows (1 + 2 rows under
//                          6-connectivity, 1 + 4 under 26): neighbourhood is symmetric, so looking back finds every pair once
//   k_label_flatten        parent(run) = root(run); roots and admissible voxels are counted          -> the host reads both
//   k_label_keys           root -> FLAG | slot, keys[slot] = ~0 << 32 | first
//   k_label_count          keys[slot of the run's root] -= length << 32, added up per wave first
//   (rocprim::radix_sort_keys: ascending (~count << 32 | first) = descending count, ties by ascending first)
//   k_label_rank           root of sorted place k -> FLAG | k + 1; the table's record k: count, first, an empty box
//   k_label_resolve        every other run -> FLAG | rank (read from its root); the boxes of the ranks the table holds
//   k_label_write          every voxel's word: its run's rank, or 0
// Union-find with the smaller index as the root: parent(p) <= p always, a root is its own parent, and the only store to a parent word
// while runs are united is  old = atomicMin(&parent[a], b)  with b < a.  If old == a the root a now hangs below b.  Otherwise somebody
// else linked a first (old < a); whether the minimum replaced that link (b < old) or not, uniting `old` with b restores what was lost
// and establishes what was asked, so the loop goes on with (old, b): the closure of {links} + {pairs still being united} never
// shrinks.  max(a, b) falls with every retry, so a unite ends; parents are read with agent-scope atomic loads, and a stale word is an
// older link of the same chain or "a is a root", which the atomicMin answers with the true word.  The classes are those of the
// neighbour relation whatever the order of blocks, a class's root is its smallest run start = its `first` voxel, and everything after
// the flatten is sums, minima, maxima and a sort of distinct keys: the bytes do not depend on the schedule.
#include <rocprim/device/device_radix_sort.hpp>

#include "mask_device.hpp"

namespace clvr {

namespace {

typedef unsigned long long u64;
constexpr uint32_t kFlag = 0x80000000u;  // flat indices and ranks are below 2^31 (the host refuses larger volumes)

__device__ __forceinline__ uint32_t parent_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t find_root(const uint32_t *parent, uint32_t p) {
  for (;;) {
    const uint32_t q = parent_load(parent + p);
    if (q == p) return p;
    p = q;
  }
}
__device__ __forceinline__ void unite(uint32_t *parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

// the first bit of the run of `b` that holds bit t
__device__ __forceinline__ int run_start(u64 b, int t) {
  const u64 zeros_below = ~b & ((1ull << t) - 1ull);
  return zeros_below ? 64 - __builtin_clzll(zeros_below) : 0;
}
// the run of `b` that starts at bit s, as a mask
__device__ __forceinline__ u64 run_from(u64 b, int s) {
  const u64 zeros_above = ~b & (~0ull << s);
  const u64 below_end = zeros_above ? ((1ull << __builtin_ctzll(zeros_above)) - 1ull) : ~0ull;
  return below_end & (~0ull << s);
}

struct LabelWord {
  size_t w;        // the word's index in A
  uint32_t base;   // the flat index of its bit 0
  int tx, y, z;
};
__device__ __forceinline__ bool label_word(const LabelArgs &a, LabelWord &o) {
  const size_t total = (size_t)a.W64 * (size_t)a.Y * (size_t)a.Z;
  o.w = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (o.w >= total) return false;
  const size_t row = o.w / (size_t)a.W64;
  o.tx = (int)(o.w - row * (size_t)a.W64);
  o.z = (int)(row / (size_t)a.Y);
  o.y = (int)(row - (size_t)o.z * (size_t)a.Y);
  o.base = (uint32_t)(row * (size_t)a.X + (size_t)o.tx * 64u);
  return true;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off));
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
  return v;
}

}  // namespace

// A, ANDed with the caller's mask if there is one.  Rows of a multiple of 8 voxels: a lane owns one byte of A (admissible_byte).
__global__ __launch_bounds__(256) void k_label_admissible8(const LabelArgs a) {
  const size_t total = (size_t)a.W64 * 8u * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total) return;
  int x0, y, z;
  uint32_t bits = admissible_byte(a, id, x0, y, z);
  if (bits != 0u && a.mask) bits &= (uint32_t)reinterpret_cast<const uint8_t *>(a.mask)[id];
  reinterpret_cast<uint8_t *>(a.adm)[id] = (uint8_t)bits;
}

// the same for any row length or alignment: a thread per voxel of the padded row, a wave per 64-bit word (admissible_voxel)
__global__ __launch_bounds__(256) void k_label_admissible(const LabelArgs a) {
  const size_t total = (size_t)a.W64 * 64u * (size_t)a.Y * (size_t)a.Z, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total) return;  // (whole waves: `total` and a wave's first id are multiples of 64)
  int x, y, z;
  u64 bits = __ballot(admissible_voxel(a, id, x, y, z));
  if ((threadIdx.x & 63u) == 0u) {
    if (a.mask) bits &= a.mask[id >> 6];
    a.adm[id >> 6] = bits;
  }
}

// every run is its own root
__global__ __launch_bounds__(256) void k_label_init(const LabelArgs a) {
  LabelWord o;
  if (!label_word(a, o)) return;
  const u64 m = a.adm[o.w];
  for (u64 starts = m & ~(m << 1); starts; starts &= starts - 1ull) {
    const uint32_t p = o.base + (uint32_t)__builtin_ctzll(starts);
    a.labels[p] = p;
  }
}

namespace {

// run `mine` (the mask `run` of its word) against the words (left, mid, right) of one earlier row; nbase: the flat index of mid's bit 0
template <bool CONN26>
__device__ __forceinline__ void unite_with_row(uint32_t *parent, uint32_t mine, u64 run, u64 left, u64 mid, u64 right, uint32_t nbase) {
  const u64 reach = CONN26 ? (run | (run << 1) | (run >> 1)) : run;
  for (u64 o = mid & reach; o;) {
    const int s = run_start(mid, __builtin_ctzll(o));
    unite(parent, mine, nbase + (uint32_t)s);
    o &= ~run_from(mid, s);
  }
  if (CONN26) {
    if ((run & 1ull) && (left >> 63)) unite(parent, mine, nbase - 64u + (uint32_t)run_start(left, 63));
    if ((run >> 63) && (right & 1ull)) unite(parent, mine, nbase + 64u);
  }
}

}  // namespace

template <bool CONN26>
__global__ __launch_bounds__(256) void k_label_merge(const LabelArgs a) {
  LabelWord o;
  if (!label_word(a, o)) return;
  const u64 m = a.adm[o.w];
  if (!m) return;
  uint32_t *parent = a.labels;
  if ((m & 1ull) && o.tx > 0) {  // the run that goes on from the word before
    const u64 before = a.adm[o.w - 1u];
    if (before >> 63) unite(parent, o.base, o.base - 64u + (uint32_t)run_start(before, 63));
  }
  // the earlier rows: (y - 1, z), (y, z - 1) and under 26 (y - 1, z - 1), (y + 1, z - 1)
  const int dy[4] = {-1, 0, -1, 1}, dz[4] = {0, -1, -1, -1};
#pragma unroll
  for (int q = 0; q < (CONN26 ? 4 : 2); ++q) {
    const int ny = o.y + dy[q], nz = o.z + dz[q];
    if (ny < 0 || ny >= a.Y || nz < 0) continue;
    const size_t nrow = (size_t)nz * (size_t)a.Y + (size_t)ny;
    const u64 *words = a.adm + nrow * (size_t)a.W64 + (size_t)o.tx;
    const u64 mid = words[0];
    const u64 left = (CONN26 && o.tx > 0) ? words[-1] : 0ull;
    const u64 right = (CONN26 && o.tx + 1 < a.W64) ? words[1] : 0ull;
    if (!(mid | (left >> 63) | (right & 1ull))) continue;
    const uint32_t nbase = (uint32_t)(nrow * (size_t)a.X + (size_t)o.tx * 64u);
    for (u64 starts = m & ~(m << 1); starts; starts &= starts - 1ull) {
      const int s = __builtin_ctzll(starts);
      unite_with_row<CONN26>(parent, o.base + (uint32_t)s, run_from(m, s), left, mid, right, nbase);
    }
  }
}

// behind a kernel boundary: every link is visible.  parent(run) = its root; counters[0] += roots, counters[1] += admissible voxels
__global__ __launch_bounds__(256) void k_label_flatten(const LabelArgs a) {
  LabelWord o;
  const bool live = label_word(a, o);
  const u64 m = live ? a.adm[o.w] : 0ull;
  uint32_t roots = 0u;
  for (u64 starts = m & ~(m << 1); starts; starts &= starts - 1ull) {
    const uint32_t p = o.base + (uint32_t)__builtin_ctzll(starts);
    const uint32_t r = find_root(a.labels, p);  // (a word another lane flattens meanwhile holds an ancestor either way)
    if (r == p) ++roots;
    else __hip_atomic_store(a.labels + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  roots = wave_sum(roots);
  const uint32_t voxels = wave_sum((uint32_t)__popcll(m));
  if ((threadIdx.x & 63u) == 0u && voxels) {
    if (roots) atomicAdd(&a.counters[0], (u64)roots);
    atomicAdd(&a.counters[1], (u64)voxels);
  }
}

// a slot per root, taken per wave: root -> FLAG | slot, and the slot's key with a count of zero
__global__ __launch_bounds__(256) void k_label_keys(const LabelArgs a) {
  LabelWord o;
  const bool live = label_word(a, o);
  const u64 m = live ? a.adm[o.w] : 0ull;
  u64 roots = 0ull;
  for (u64 starts = m & ~(m << 1); starts; starts &= starts - 1ull) {
    const int s = __builtin_ctzll(starts);
    if (a.labels[o.base + (uint32_t)s] == o.base + (uint32_t)s) roots |= 1ull << s;
  }
  const uint32_t mine = (uint32_t)__popcll(roots);
  uint32_t before = mine;  // the inclusive scan over the wave's lanes
  const unsigned lane = threadIdx.x & 63u;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = (uint32_t)__shfl_up((int)before, off);
    if (lane >= (unsigned)off) before += v;
  }
  const uint32_t total = (uint32_t)__shfl((int)before, 63);
  if (!total) return;
  uint32_t slot = 0u;
  if (lane == 0u) slot = (uint32_t)atomicAdd(&a.counters[2], (u64)total);
  slot = (uint32_t)__shfl((int)slot, 0) + before - mine;
  for (; roots; roots &= roots - 1ull) {
    const uint32_t p = o.base + (uint32_t)__builtin_ctzll(roots);
    a.labels[p] = kFlag | slot;
    a.keys_in[slot] = (0xFFFFFFFFull << 32) | (u64)p;
    ++slot;
  }
}

namespace {
// the slot (k_label_count) or rank (k_label_resolve) of the run that starts at p: its own word if it is a root, else its root's
__device__ __forceinline__ uint32_t label_of_run(const uint32_t *labels, uint32_t p) {
  const uint32_t v = labels[p];
  return ((v & kFlag) ? v : labels[v]) & ~kFlag;
}
}  // namespace

// counts.  The lanes of a wave take their words' runs in step; the runs of a step that belong to the same class as the first of them
// are added up in the wave and cost one atomic, then the same for the first of the rest, three times; what is left costs one atomic
// each.  A class that fills the volume costs an atomic per wave and step, also where specks lie between its runs
__global__ __launch_bounds__(256) void k_label_count(const LabelArgs a) {
  LabelWord o;
  const bool live = label_word(a, o);
  const u64 m = live ? a.adm[o.w] : 0ull;
  u64 starts = m & ~(m << 1);
  const unsigned lane = threadIdx.x & 63u;
  for (;;) {
    const u64 active = __ballot(starts != 0ull);
    if (!active) break;
    uint32_t slot = 0xFFFFFFFFu, len = 0u;
    if (starts) {
      const int s = __builtin_ctzll(starts);
      starts &= starts - 1ull;
      slot = label_of_run(a.labels, o.base + (uint32_t)s);
      len = (uint32_t)__popcll(run_from(m, s));
    }
    // up to three classes per step are added up in the wave: the class of the first lane still waiting, each time
    bool waiting = len != 0u;
    for (int turn = 0; turn < 3; ++turn) {
      const u64 todo = __ballot(waiting);
      if (!todo) break;  // (the same for every lane)
      const int leader = __builtin_ctzll(todo);
      const uint32_t lead_slot = (uint32_t)__shfl((int)slot, leader);
      const bool with_leader = waiting && slot == lead_slot;
      const uint32_t sum = wave_sum(with_leader ? len : 0u);
      if (lane == (unsigned)leader) atomicAdd(&a.keys_in[slot], (0ull - (u64)sum) << 32);
      if (with_leader) waiting = false;
    }
    if (waiting) atomicAdd(&a.keys_in[slot], (0ull - (u64)len) << 32);
  }
}

// sorted place k is rank k + 1
__global__ __launch_bounds__(256) void k_label_rank(const LabelArgs a) {
  const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= (size_t)a.n_roots) return;
  const u64 key = a.keys_out[k];
  const uint32_t first = (uint32_t)key, count = ~(uint32_t)(key >> 32);
  a.labels[first] = kFlag | (uint32_t)(k + 1u);
  if (k < (size_t)a.n_records) {
    LabelRecord r;
    r.count = (u64)count;
    r.first[0] = first % (uint32_t)a.X;
    r.first[1] = (first / (uint32_t)a.X) % (uint32_t)a.Y;
    r.first[2] = first / ((uint32_t)a.X * (uint32_t)a.Y);
    for (int q = 0; q < 3; ++q) {
      r.lo[q] = 0xFFFFFFFFu;
      r.hi[q] = 0u;
    }
    r.reserved = 0u;
    a.records[k] = r;
  }
}

namespace {
// a bound that has long been reached is not sent again: one load instead of an atomic on a word the whole grid shares
__device__ __forceinline__ void box_min(uint32_t *word, uint32_t v) {
  if (v < parent_load(word)) __hip_atomic_fetch_min(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void box_max(uint32_t *word, uint32_t v) {
  if (v > parent_load(word)) __hip_atomic_fetch_max(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
}  // namespace

// every run that is no root takes FLAG | rank from its root (the roots have theirs and are only read here); the runs of the ranks the
// table holds widen their record's box, reduced per wave like the counts
__global__ __launch_bounds__(256) void k_label_resolve(const LabelArgs a) {
  LabelWord o;
  const bool live = label_word(a, o);
  const u64 m = live ? a.adm[o.w] : 0ull;
  u64 starts = m & ~(m << 1);
  const unsigned lane = threadIdx.x & 63u;
  for (;;) {
    const u64 active = __ballot(starts != 0ull);
    if (!active) break;
    uint32_t rank = 0u, x_lo = 0xFFFFFFFFu, x_hi = 0u;
    if (starts) {
      const int s = __builtin_ctzll(starts);
      starts &= starts - 1ull;
      const uint32_t p = o.base + (uint32_t)s;
      const uint32_t v = a.labels[p];
      if (v & kFlag) {
        rank = v & ~kFlag;
      } else {
        const uint32_t r = a.labels[v];
        a.labels[p] = r;
        rank = r & ~kFlag;
      }
      x_lo = (uint32_t)(o.tx * 64 + s);
      x_hi = x_lo + (uint32_t)__popcll(run_from(m, s));
    }
    if (a.n_records != 0u) {  // (the same for every lane)
      const int leader = __builtin_ctzll(active);
      const uint32_t lead_rank = (uint32_t)__shfl((int)rank, leader);
      const bool with_leader = rank == lead_rank, leads = lane == (unsigned)leader;
      const uint32_t y = (uint32_t)o.y, z = (uint32_t)o.z;
      uint32_t lo[3], hi[3];
      lo[0] = wave_min(with_leader ? x_lo : 0xFFFFFFFFu);
      hi[0] = wave_max(with_leader ? x_hi : 0u);
      lo[1] = wave_min(with_leader ? y : 0xFFFFFFFFu);
      hi[1] = wave_max(with_leader ? y + 1u : 0u);
      lo[2] = wave_min(with_leader ? z : 0xFFFFFFFFu);
      hi[2] = wave_max(with_leader ? z + 1u : 0u);
      if (!leads) lo[0] = x_lo, hi[0] = x_hi, lo[1] = y, hi[1] = y + 1u, lo[2] = z, hi[2] = z + 1u;
      if (rank != 0u && rank <= a.n_records && (leads || !with_leader)) {
        LabelRecord *r = a.records + (rank - 1u);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          box_min(&r->lo[q], lo[q]);
          box_max(&r->hi[q], hi[q]);
        }
      }
    }
  }
}

// every word of labels: a thread per voxel of the padded row, a wave per word of A.  The word of a run's first voxel holds FLAG | rank
// until its own lane stores the rank there: either reads as the rank
__global__ __launch_bounds__(256) void k_label_write(const LabelArgs a) {
  const size_t padded = (size_t)a.W64 * 64u, total = padded * (size_t)a.Y * (size_t)a.Z;
  const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= total) return;
  const size_t row = id / padded;
  const int x = (int)(id - row * padded);
  if (x >= a.X) return;
  const u64 m = a.adm[id >> 6];
  const int bit = x & 63;
  const size_t p = row * (size_t)a.X + (size_t)x;
  uint32_t rank = 0u;
  if ((m >> bit) & 1ull) rank = a.labels[p - (size_t)(bit - run_start(m, bit))] & ~kFlag;
  a.labels[p] = rank;
}

// mask bit = rank_lo <= label <= rank_hi.  Rows of a multiple of 8 labels at a 16-byte aligned buffer: a lane makes one byte of the mask
// from two 16-byte loads; the bytes at x >= X are the padding and become zero
__global__ __launch_bounds__(256) void k_labels_to_mask(const uint32_t *__restrict__ labels, uint8_t *mask, int32_t X, size_t rows, int32_t W64,
                                                        uint32_t rank_lo, uint32_t rank_hi) {
  const size_t bytes_per_row = (size_t)W64 * 8u, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= bytes_per_row * rows) return;
  const size_t row = id / bytes_per_row;
  const int x0 = (int)(id - row * bytes_per_row) * 8;
  uint32_t bits = 0u;
  if (x0 < X) {
    const uint4 *p = reinterpret_cast<const uint4 *>(labels + row * (size_t)X + (size_t)x0);
    const uint4 q0 = p[0], q1 = p[1];
    const uint32_t v[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
    for (int h = 0; h < 8; ++h) bits |= (v[h] - rank_lo <= rank_hi - rank_lo) ? (1u << h) : 0u;
  }
  mask[id] = (uint8_t)bits;
}
// any row length or alignment: a thread per label of the padded row, a wave per 64-bit word
__global__ __launch_bounds__(256) void k_labels_to_mask_ragged(const uint32_t *__restrict__ labels, unsigned long long *mask, int32_t X, size_t rows,
                                                               int32_t W64, uint32_t rank_lo, uint32_t rank_hi) {
  const size_t padded = (size_t)W64 * 64u, id = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (id >= padded * rows) return;
  const size_t row = id / padded;
  const int x = (int)(id - row * padded);
  const bool in = x < X && (labels[row * (size_t)X + (size_t)x] - rank_lo <= rank_hi - rank_lo);
  const u64 bits = __ballot(in);
  if ((threadIdx.x & 63u) == 0u) mask[id >> 6] = bits;
}

namespace {
inline size_t label_words(const LabelArgs &a) { return (size_t)a.W64 * (size_t)a.Y * (size_t)a.Z; }
}  // namespace

// A, the runs, their unions, the flatten with its two counts
hipError_t launch_label_classes(const LabelArgs &a, hipStream_t s) {
  const size_t words = label_words(a);
  if (rows_of_8(a.volume, a.X)) hipLaunchKernelGGL(k_label_admissible8, dim3(blocks_for(words * 8u)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_label_admissible, dim3(blocks_for(words * 64u)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_label_init, dim3(blocks_for(words)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(a.conn26 ? k_label_merge<true> : k_label_merge<false>, dim3(blocks_for(words)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_label_flatten, dim3(blocks_for(words)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// temp == nullptr: only temp_bytes is set
hipError_t launch_label_sort(void *temp, size_t &temp_bytes, const LabelArgs &a, hipStream_t s) {
  return rocprim::radix_sort_keys(temp, temp_bytes, a.keys_in, a.keys_out, (size_t)a.n_roots, 0u, 64u, s);
}

// the keys and their counts (before the sort); the ranks, the table and every word of labels (after it)
hipError_t launch_label_keys(const LabelArgs &a, hipStream_t s) {
  const size_t words = label_words(a);
  hipLaunchKernelGGL(k_label_keys, dim3(blocks_for(words)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_label_count, dim3(blocks_for(words)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_label_ranks(const LabelArgs &a, hipStream_t s) {
  const size_t words = label_words(a);
  hipLaunchKernelGGL(k_label_rank, dim3(blocks_for(a.n_roots)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_label_resolve, dim3(blocks_for(words)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_label_write, dim3(blocks_for(words * 64u)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_labels_to_mask(const uint32_t *labels, unsigned long long *mask, int32_t X, int32_t Y, int32_t Z, int32_t W64, uint32_t rank_lo,
                                 uint32_t rank_hi, hipStream_t s) {
  const size_t rows = (size_t)Y * (size_t)Z;
  if (rows_of_8(labels, X))
    hipLaunchKernelGGL(k_labels_to_mask, dim3(blocks_for(rows * (size_t)W64 * 8u)), dim3(256), 0, s, labels, (uint8_t *)mask, X, rows, W64, rank_lo, rank_hi);
  else
    hipLaunchKernelGGL(k_labels_to_mask_ragged, dim3(blocks_for(rows * (size_t)W64 * 64u)), dim3(256), 0, s, labels, mask, X, rows, W64, rank_lo, rank_hi);
  return hipGetLastError();
}

}  // namespace clvr
