// bounce_device.hpp -- what the kernels of the `render` pass share around k_bounce / k_bounce2: small wave helpers, the lane states, the
// end of a sample (finish_item, k_env_fixup's too), the fix-up record, the exit certificate's look-up, scheduling statistics.
#pragma once
#include "render_device.hpp"

namespace clvr {

__device__ __forceinline__ VolumePacked make_volume(const RenderArgs &a) {
  return VolumePacked{a.grec, a.stepb, a.volume_lin, a.sdf_lin, a.X, a.Y, a.Z, a.NBX, a.NBY};
}

// n / d and n % d for n, d < 2^24 through the float reciprocal (a 32-bit integer division is ~35 VALU instructions)
__device__ __forceinline__ uint32_t udivmod24(uint32_t n, uint32_t d, uint32_t &rem) {
  // n < 2^24 and d < 2^24 convert exactly; the estimate's relative error is below 2^-22, so for the quotients met
  // here (below 2^20, or d a power of two) it is off by at most one either way
  uint32_t q = (uint32_t)((float)n * __builtin_amdgcn_rcpf((float)d));
  uint32_t qd;
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(qd) : "v"(q), "v"(d));
  int32_t r = (int32_t)(n - qd);
  if (r < 0) { q -= 1u; r += (int32_t)d; }
  if (r >= (int32_t)d) { q += 1u; r -= (int32_t)d; }
  rem = (uint32_t)r;
  return q;
}

// A wave-uniform value, pinned to a scalar register.  What the vector unit computed or loaded (a division's reciprocal, a word of global
// memory) stays in a vector register otherwise, uniform or not, and every branch on it becomes an exec-mask branch.
__device__ __forceinline__ uint32_t scalar_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// number of set bits of `mask` below this lane
__device__ __forceinline__ unsigned prefix_count(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
__device__ __forceinline__ unsigned lane_id() { return prefix_count(~0ull); }

// The state of a ray in k_bounce / k_bounce2, one register: ST_IDLE (no item), ST_MARCH, ST_CERT (parked for an exit-certificate attempt),
// or ST_EVENT + the pending event.
enum : int { ST_IDLE = 0, ST_MARCH = 1, ST_CERT = 2, ST_EVENT = 8 };
enum : int { EV_START = 3,              // start distribution ray `o` from the primary hit (a freshly fetched item: o = 1)
             EV_HIT_COLOR_PENDING = 4,  // a Hit whose rule colour is still to be fetched (classify_step DEFER_COLOR)
             EV_CHECK = 5 };            // the new position has no voxel: left the volume, or one of the rare in-between cases?
constexpr int kCertNever = 255;         // no step is this long

// What a Hit's colour needs of its rule, staged in LDS once per block: entry k = {rule k writes a colour, that colour}.  The kernel
// argument segment answers the same question with two loads, one after the other, behind the hit record's.
__device__ __forceinline__ void stage_rule_colors(uint2 *rule_color, const TfDev &tf) {
  if (threadIdx.x < (unsigned)CLWH_TF_MAX_RULES) {
    const bool used = (int)threadIdx.x < tf.n;
    const TfRuleDev &rule = tf.rules[used ? threadIdx.x : 0u];
    rule_color[threadIdx.x] = used ? uint2{rule.flags & TF_WRITES_COLOR, rule.color} : uint2{0u, 0u};
  }
}
// hit_gradient_and_color (render_device.hpp) with the rule's colour from that table: LDS reads behind the record's load
template <int SMALL = 0>
__device__ __forceinline__ f3 hit_gradient_and_color(const VolumePacked &v, const uint2 *rule_color, f3 pos, bool want_color, uint32_t &color) {
  const bool regular = hit_record_serves(v, pos);
  if (regular || want_color) {
    const uint2 r = v.template hit_record<SMALL>(pos.x, pos.y, pos.z);  // either condition implies pos is inside the volume
    if (want_color) {
      const uint2 rule = rule_color[VolumePacked::hit_class(r) - 1u];
      if (rule.x != 0u) color = rule.y;
    }
    if (regular) {
      int gx, gy, gz;
      VolumePacked::hit_gradient(r, gx, gy, gz);
      return f3{(float)gx, (float)gy, (float)gz};
    }
  }
  return gradient_literal(v, pos);
}

// Image-space accumulation of one launch: a sample adds r | g<<16 | b<<32 | 1<<48 to its HIT's 64-bit
// delta with ONE atomic (a launch has at most 64 seeds and a contribution is at most 255, so no field can
// carry); k_commit then folds the deltas into the caller's float4 buffer with plain read-modify-writes.
// Four float atomics per sample were a quarter of the kernel's L2-missing requests.
template <int MODE>
__device__ __forceinline__ void finish_item(const RenderArgs &a, int64_t entry, uint32_t hit, uint32_t gx, uint32_t gy,
                                            uint32_t bv_r, uint32_t bv_g, uint32_t bv_b) {
  // ray_marching.cl:75-76: halve (dist_count = 2), then add
  const uint32_t cr = (bv_r / 2u) & 0xFFFFu, cg = (bv_g / 2u) & 0xFFFFu, cb = (bv_b / 2u) & 0xFFFFu;
  if (MODE == CLWH_ACCUM_VOXEL_CACHE && a.grants == nullptr) {
    cache_add(a.cache, entry, cr, cg, cb, 0u);
  } else {
    const unsigned long long packed = (unsigned long long)cr | ((unsigned long long)cg << 16) |
                                      ((unsigned long long)cb << 32) | (1ull << 48);
    atomicAdd(a.delta + hit, packed);
  }
  if (a.contrib_out) {
    uint32_t *q = a.contrib_out + ((size_t)gy * (size_t)a.launch_w + gx) * 4;
    q[0] = cr; q[1] = cg; q[2] = cb; q[3] = 1u;
  }
}

// Environment lookups use the certified fast path (env_fast.hpp).  A lookup that cannot be certified
// (about one in a thousand) does not stall the lane: the sample's pending term {atten*energy, factor,
// direction} goes into a fix-up record, the lane walks the rest of the sample as usual, and the tiny
// k_env_fixup launch that follows evaluates the exact binary64 lookup and finishes the arithmetic in
// the reference's order.  Every sample is accumulated exactly once, by one of the two kernels.
constexpr int kFixupDwords = 32;  // one record = 128 B: header[4] bv_before[3] n_pending[1] 2 x {P[3] factor dir[3]}

// Exit certificates.  A march that ends in Exit_volume contributes through its DIRECTION only (ray_marching.cl:54-62
// samples the environment with current_ray.direction): where it leaves the volume is never used.  So when it can be
// PROVEN that a march will leave the volume without a Hit within the steps it has left, its remaining steps -- far-field
// fetches, one 128-byte line each, for a position nobody needs -- are skipped and the Exit event is raised at once; the
// result is bit-identical.  The proof is one table lookup: the ray's coordinates are monotone, so the rest of its path
// lies in the box between its macro cell (16^3 voxels) and the volume corner its direction octant heads for, and the
// table (k_macro_table .. k_macro_bounds) holds, per cell and octant, the smallest SDF value of that box if it is
// free: no voxel that could be an event (a Hit needs one) and SDF values of at least kCertMinStep.  The ray's distance to the face it
// leaves through, divided by that minimum, bounds the steps the march still takes; the bound must fit the march's budget (a march that ran out of steps would continue as the NEXT march,
// with another weight, ray_marching.cl:52-73).  tools/exit_certificate.py measured the idea on the oracle first: every
// exiting ray gets its certificate at some point, 5 of the 30 step fetches per item disappear (all far field), and not
// one certificate in millions was wrong.
// `away`: after a refusal, the path length the march has to cover before a look-up can succeed ((g - 1) cells, k_macro_hints); 0 when
// the table does not say (the box is free but the budget too small, or one of the rare directions)
__device__ __forceinline__ bool certify_exit(const RenderArgs &a, f3 p, f3 d, int budget, int &away) {
  // the position has a voxel or sits on the far face: 0 <= p <= dim (or -0.0)
  const unsigned cx = min((unsigned)(int)p.x >> a.macro_shift, (unsigned)a.MNX - 1u), cy = min((unsigned)(int)p.y >> a.macro_shift, (unsigned)a.MNY - 1u),
                 cz = min((unsigned)(int)p.z >> a.macro_shift, (unsigned)a.MNZ - 1u);
  const unsigned octant = (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
  const int entry = a.macro[(((cz * (unsigned)a.MNY + cy) * (unsigned)a.MNX + cx) << 3) | octant];  // (at most 2^22 entries)
  const bool refused = (entry & (int)kCertRefused) != 0;
  const int box_min = refused ? 0 : entry;
  away = refused ? ((entry & 0x7F) - 1) << a.macro_shift : 0;
  // One kind of position is outside the reasoning below: a coordinate that landed exactly ON the far face (== dimension: not exited,
  // utility_ray.cl:112-117) reads the border SDF 0 and advances 0.5 |d| per step; with a direction component too small to move that
  // coordinate (0.5 x 2^-10 is above half an ulp of every dimension below 2^13) the reference can crawl along the face and even run
  // out of its 70 steps.  Such directions get no certificate and march literally; for all others the next step leaves (the 5).
  const float dmin = fminf(fminf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
  const float dsum = d.x + d.y + d.z;  // NaN direction: the position turns NaN and never leaves
  // Every step inside the box is max(sdf, 0.5) >= box_min long and the direction has unit length, so after (budget - 5) steps the march has
  // travelled T = (budget - 5) * box_min along the ray (an integer below 2^14: exact) and has passed the face of an axis as soon as
  // T * |d_axis| >= its distance to that face -- one axis is enough; the 5 steps kept back cover the roundings of the march, of these three
  // products, and the strictness of exited_volume.  (Round 3 first took the smallest (face - p) / d over the axes: three reciprocals,
  // quarter-rate instructions, for the same decision.)
  const float T = (float)((budget - 5) * box_min);
  const float fx = d.x < 0.0f ? p.x : (float)a.X - p.x, fy = d.y < 0.0f ? p.y : (float)a.Y - p.y, fz = d.z < 0.0f ? p.z : (float)a.Z - p.z;
  const bool leaves = T * fabsf(d.x) >= fx || T * fabsf(d.y) >= fy || T * fabsf(d.z) >= fz;
  return box_min != 0 && budget > 5 && leaves && dmin >= 0.0009765625f && dsum == dsum;
}
// Start certificates: `mask` is the byte of the first leg's start voxel in the "free from here" table (k_start_*, scene_kernels.hip), `d`
// the leg's direction, `dmin_needed` start_cert_dmin (clwh_internal.hpp).  Octants as above; a NaN direction never leaves.
__device__ __forceinline__ bool start_certificate(uint32_t mask, f3 d, float dmin_needed) {
  const unsigned octant = (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
  const float dmin = fminf(fminf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
  const float dsum = d.x + d.y + d.z;
  return ((mask >> octant) & 1u) != 0u && dmin >= dmin_needed && dsum == dsum;
}
// Hull certificates: direction k of the support table (k_hull_*, scene_kernels.hip), the centre of cell (k % 64, k / 64) of an octahedral
// grid.  The unnormalised components are multiples of 1/64 below 2 and the sum of their squares a multiple of 2^-12 below 4: every
// operation before the reciprocal square root is exact in binary32 whether or not it is contracted, so the table's builder, k_primary
// and k_bounce get the same bits (v_rsq_f32 leaves the length within 2^-22 of 1: kHullSlack).
__device__ __forceinline__ f3 hull_direction(unsigned k) {
  static_assert(kHullGrid == 64, "cell centres are odd multiples of 1/64");
  const float u = (float)(2 * (int)(k & 63u) - 63) * 0.015625f, v = (float)(2 * (int)((k >> 6) & 63u) - 63) * 0.015625f;
  const float z = (1.0f - fabsf(u)) - fabsf(v);
  const float x = z >= 0.0f ? u : copysignf(1.0f - fabsf(v), u), y = z >= 0.0f ? v : copysignf(1.0f - fabsf(u), v);
  const float r = __builtin_amdgcn_rsqf((x * x + y * y) + z * z);
  return f3{x * r, y * r, z * r};
}
// The octahedral cell a vector of any length falls in: hull_direction's inverse on its cell centres (the reciprocal and the products
// are off by an ulp, the centres lie half a cell from every border).  k_bounce's tilted planes pick their plane with it;
// ANY cell is a safe answer -- only the yield depends on it -- but it must be a cell: fmaxf / fminf drop a NaN, so a NaN lands in cell 0.
__device__ __forceinline__ unsigned hull_cell(f3 n) {
  static_assert(kHullGrid == 64, "cell (i, j) covers u in [i / 32 - 1, (i + 1) / 32 - 1)");
  const float r = __builtin_amdgcn_rcpf((fabsf(n.x) + fabsf(n.y)) + fabsf(n.z));
  const float x = n.x * r, y = n.y * r;
  const float u = n.z >= 0.0f ? x : copysignf(1.0f - fabsf(y), x), v = n.z >= 0.0f ? y : copysignf(1.0f - fabsf(x), y);
  const int i = (int)fminf(fmaxf(floorf(u * 32.0f + 32.0f), 0.0f), 63.0f), j = (int)fminf(fmaxf(floorf(v * 32.0f + 32.0f), 0.0f), 63.0f);
  return (unsigned)(j * 64 + i);
}
// (the test itself: k_bounce's opening half.  The far-face crawl and NaN directions as in certify_exit.)
__device__ __forceinline__ bool certify_exit(const RenderArgs &a, f3 p, f3 d, int budget) {
  int away;
  return certify_exit(a, p, d, budget, away);
}

// ---- what k_bounce and k_bounce2 share word for word: the LDS index tables, the home queue and the scheduling statistics
// SMALL == 2: the per-axis index terms are read from LDS (packed_volume.hpp); the block's `threads` threads fill the tables
template <int SMALL>
__device__ __forceinline__ void index_tables_to_lds(VolumePacked &vol, const RenderArgs &a, int threads) {
  extern __shared__ uint32_t lds_parts[];
  if (SMALL == 2) {
    vol.parts = lds_parts;
    vol.parts_y0 = a.X;
    vol.parts_z0 = a.X + a.Y;
    for (int k = (int)threadIdx.x; k < a.X + a.Y + a.Z; k += threads)
      lds_parts[k] = k < a.X ? vol.part_x<1>((unsigned)k) : (k < a.X + a.Y ? vol.part_y<1>((unsigned)(k - a.X)) : vol.part_z<1>((unsigned)(k - a.X - a.Y)));
  }
}
// the unit queue a wave serves first
__device__ __forceinline__ unsigned home_queue_of(const RenderArgs &a, unsigned waves_per_block) {
  // HW_REG_XCC_ID (id 20), bits [3:0]: the XCD this wave runs on
  unsigned home_queue = (unsigned)__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;
  if (a.unit_affinity == 1) home_queue = (blockIdx.x * waves_per_block + (threadIdx.x >> 6)) & 7u;
  if (a.unit_affinity == 2) home_queue = 0u;
  return home_queue;
}

// Scheduling statistics of a launch (-DCLVR_BOUNCE_STATS, experiment builds: clwh_render.hip prints them).  A wave counts in
// registers and lane 0 adds the sums to the CTR_* slots when the wave ends.  In a product build the struct is empty and so is every
// method, ballots included.
// -DCLVR_BOUNCE_STATS also VERIFIES k_bounce's start certificates: a granted first leg is marched literally all the same and counted as
// wrong unless it ends in Exit.  -DCLVR_BOUNCE_STATS=2 takes them as the product build does (its counts are the product build's).
#ifdef CLVR_BOUNCE_STATS
constexpr bool kBounceStats = true;
constexpr bool kStartCertVerify = (CLVR_BOUNCE_STATS + 0) != 2;
#else
constexpr bool kBounceStats = false;
constexpr bool kStartCertVerify = false;
#endif
template <bool ON> struct BounceStatsT;
template <> struct BounceStatsT<false> {
  __device__ void step(int) {}
  __device__ void cert_begin(int, int) {}
  __device__ void cert_end(int, int) {}
  __device__ void closing_half(int) {}
  __device__ void event_phase(int) {}
  __device__ void refill(uint32_t) {}
  __device__ void fresh_items(int, int) {}
  __device__ void swap_point() {}
  __device__ void start_cert(bool, bool) {}
  __device__ void hull_cert(bool, bool, bool) {}
  __device__ void hull_more(bool, bool, bool, bool) {}
  __device__ void hull_fired(bool, bool) {}
  __device__ void hull_tilt(bool, bool, bool, bool, bool) {}
  __device__ void hull_late(bool) {}
  __device__ void march_end(uint32_t *, int) {}
  template <bool TWO_RAYS> __device__ void flush(uint32_t *) {}
};
template <> struct BounceStatsT<true> {
  uint32_t step_iters = 0, step_lanes = 0, event_phases = 0, event_lanes = 0, refills = 0, refill_lanes = 0;
  uint32_t ev_kind[4] = {0, 0, 0, 0};
  uint32_t cert_phases = 0, cert_lanes = 0, cert_granted = 0;
  uint32_t step_idle = 0;  // idle lanes, summed over the step iterations
  uint32_t swaps = 0;      // k_bounce2's swap points
  uint32_t closing = 0, marching_before = 0;  // lanes of this pass's closing half; marching lanes before this certificate phase
  // a step iteration
  __device__ __forceinline__ void step(int st) {
    step_iters += 1; step_lanes += (uint32_t)__popcll(__ballot(st == ST_MARCH));
    step_idle += (uint32_t)__popcll(__ballot(st == ST_IDLE));
  }
  // a certificate phase of `n_cert` lanes, before and after the look-ups
  __device__ __forceinline__ void cert_begin(int st, int n_cert) {
    cert_phases += 1; cert_lanes += (uint32_t)n_cert;
    marching_before = (uint32_t)__popcll(__ballot(st == ST_MARCH));
  }
  __device__ __forceinline__ void cert_end(int st, int n_cert) { cert_granted += (uint32_t)(n_cert - (__popcll(__ballot(st == ST_MARCH)) - (int)marching_before)); }
  // k_bounce: the closing half of an event phase
  __device__ __forceinline__ void closing_half(int st) {
    closing = (uint32_t)__popcll(__ballot(st >= ST_EVENT));
    event_lanes += closing;
    ev_kind[1] += (uint32_t)__popcll(__ballot(st == ST_EVENT + EV_EXIT || st == ST_EVENT + EV_CHECK));
    ev_kind[2] += (uint32_t)__popcll(__ballot(st == ST_EVENT + EV_HIT || st == ST_EVENT + EV_HIT_COLOR_PENDING));
    ev_kind[3] += (uint32_t)__popcll(__ballot(st == ST_EVENT + EV_NONE));
  }
  // k_bounce2: its one-piece event phase
  __device__ __forceinline__ void event_phase(int st) {
    if (__ballot(st >= ST_EVENT) != 0ull) { event_phases += 1; event_lanes += (uint32_t)__popcll(__ballot(st >= ST_EVENT)); }
  }
  __device__ __forceinline__ void refill(uint32_t count) { refills += 1; refill_lanes += count; }
  // k_bounce, before the opening half: a fresh item's start counts as an event of this phase (as when it was served from its parked state)
  __device__ __forceinline__ void fresh_items(int st, int o) {
    const uint32_t n_fresh = (uint32_t)__popcll(__ballot(st == ST_EVENT + EV_START && o == 1));
    ev_kind[0] += n_fresh; event_lanes += n_fresh;
    if (closing + n_fresh != 0u) event_phases += 1;  // one phase, two halves
  }
  __device__ __forceinline__ void swap_point() { swaps += 1; }
  // k_bounce's start certificates; kStartCertVerify: a granted first leg is marched literally all the same, and when its march
  // ends (closing half, any lane on its own) it counts as WRONG unless it ended in Exit -- a Hit, or 70 steps without an event
  uint32_t start_tried = 0, start_granted = 0;
  bool start_open = false;  // this lane's current march holds a start certificate
  __device__ __forceinline__ void start_cert(bool tried, bool granted) {
    start_tried += (uint32_t)__popcll(__ballot(tried)); start_granted += (uint32_t)__popcll(__ballot(granted));
    start_open = start_open || granted;
  }
  // hull certificates, verified the same way; `both`: the octant proof grants the leg as well
  uint32_t hull_tried = 0, hull_granted = 0, hull_both = 0;
  bool hull_open = false;
  __device__ __forceinline__ void hull_cert(bool tried, bool granted, bool both) {
    hull_tried += (uint32_t)__popcll(__ballot(tried)); hull_granted += (uint32_t)__popcll(__ballot(granted));
    hull_both += (uint32_t)__popcll(__ballot(both));
    hull_open = hull_open || granted;
  }
  // item 13's classes, verified the same way: 0 first legs granted after a few literal steps, 1 rebounds granted at once, 2 rebounds
  // granted after a few literal steps; per class tried (deferred: armed) and granted (deferred: got in front within kHullDeferSteps)
  uint32_t more_tried[3] = {0, 0, 0}, more_granted[3] = {0, 0, 0};
  int more_open = -1;  // this lane's current march holds a certificate of that class
  __device__ __forceinline__ void hull_more(bool rebound_tried, bool rebound_granted, bool armed, bool first_leg) {
    more_tried[0] += (uint32_t)__popcll(__ballot(armed && first_leg)); more_tried[2] += (uint32_t)__popcll(__ballot(armed && !first_leg));
    more_tried[1] += (uint32_t)__popcll(__ballot(rebound_tried)); more_granted[1] += (uint32_t)__popcll(__ballot(rebound_granted));
    if (rebound_granted) more_open = 1;
  }
  __device__ __forceinline__ void hull_fired(bool fired_any, bool first_leg) {
    const bool fired = fired_any && !tilt_armed, tilted = fired_any && tilt_armed;  // whose arming it was
    more_granted[0] += (uint32_t)__popcll(__ballot(fired && first_leg)); more_granted[2] += (uint32_t)__popcll(__ballot(fired && !first_leg));
    if (fired) more_open = first_leg ? 0 : 2;
    tilt_granted[1] += (uint32_t)__popcll(__ballot(tilted && first_leg)); tilt_granted[3] += (uint32_t)__popcll(__ballot(tilted && !first_leg));
    if (tilted) tilt_open = first_leg ? 1 : 3;
  }
  // item 14's classes, verified the same way: 0 first legs granted at once by a tilted plane, 1 first legs granted after a few literal
  // steps, 2 / 3 the same for rebounds; `starts`: the lane starts a march in this opening half (armed by the tilted plane or not)
  uint32_t tilt_tried[4] = {0, 0, 0, 0}, tilt_granted[4] = {0, 0, 0, 0}, tilt_late = 0;
  int tilt_open = -1;
  bool tilt_armed = false;  // this lane's current march was armed by a tilted plane
  __device__ __forceinline__ void hull_tilt(bool tried, bool granted, bool armed, bool starts, bool first_leg) {
    tilt_tried[0] += (uint32_t)__popcll(__ballot(tried && first_leg)); tilt_tried[2] += (uint32_t)__popcll(__ballot(tried && !first_leg));
    tilt_granted[0] += (uint32_t)__popcll(__ballot(granted && first_leg)); tilt_granted[2] += (uint32_t)__popcll(__ballot(granted && !first_leg));
    tilt_tried[1] += (uint32_t)__popcll(__ballot(armed && first_leg)); tilt_tried[3] += (uint32_t)__popcll(__ballot(armed && !first_leg));
    if (granted) tilt_open = first_leg ? 0 : 2;
    if (starts) tilt_armed = armed;
  }
  __device__ __forceinline__ void hull_late(bool late) { tilt_late += (uint32_t)__popcll(__ballot(late)); }
  __device__ __forceinline__ void march_end(uint32_t *counters, int ev) {
    if (start_open && ev != EV_EXIT) atomicAdd(&counters[CTR_START_WRONG], 1u);
    if (hull_open && ev != EV_EXIT) atomicAdd(&counters[CTR_HULL_WRONG], 1u);
    if (more_open >= 0 && ev != EV_EXIT) atomicAdd(&counters[CTR_HULL_DEFER + 3 * more_open + 2], 1u);
    if (tilt_open >= 0 && ev != EV_EXIT) atomicAdd(&counters[CTR_HULL_TILT + 3 * tilt_open + 2], 1u);
    start_open = false;
    hull_open = false;
    more_open = -1;
    tilt_open = -1;
  }
  // lane 0 of a wave that ends
  template <bool TWO_RAYS> __device__ __forceinline__ void flush(uint32_t *counters) {
    atomicAdd(&counters[CTR_STEP_ITERS], step_iters); atomicAdd(&counters[CTR_STEP_LANES], step_lanes);
    atomicAdd(&counters[CTR_EVENT_PHASES], event_phases); atomicAdd(&counters[CTR_EVENT_LANES], event_lanes);
    atomicAdd(&counters[CTR_REFILLS], refills); atomicAdd(&counters[CTR_REFILL_LANES], refill_lanes);
    if (TWO_RAYS) { atomicAdd(&counters[CTR_SWAPS], swaps); return; }
    for (int k = 0; k < 4; ++k) atomicAdd(&counters[CTR_EV_KIND + k], ev_kind[k]);
    atomicAdd(&counters[CTR_CERT_PHASES], cert_phases); atomicAdd(&counters[CTR_CERT_LANES], cert_lanes);
    atomicAdd(&counters[CTR_CERT_GRANTED], cert_granted); atomicAdd(&counters[CTR_STEP_IDLE], step_idle);
    atomicAdd(&counters[CTR_START_TRIED], start_tried); atomicAdd(&counters[CTR_START_GRANTED], start_granted);
    atomicAdd(&counters[CTR_HULL_TRIED], hull_tried); atomicAdd(&counters[CTR_HULL_GRANTED], hull_granted); atomicAdd(&counters[CTR_HULL_BOTH], hull_both);
    for (int k = 0; k < 3; ++k) { atomicAdd(&counters[CTR_HULL_DEFER + 3 * k], more_tried[k]); atomicAdd(&counters[CTR_HULL_DEFER + 3 * k + 1], more_granted[k]); }
    for (int k = 0; k < 4; ++k) { atomicAdd(&counters[CTR_HULL_TILT + 3 * k], tilt_tried[k]); atomicAdd(&counters[CTR_HULL_TILT + 3 * k + 1], tilt_granted[k]); }
    atomicAdd(&counters[CTR_HULL_TILT + 12], tilt_late);
  }
};
using BounceStats = BounceStatsT<kBounceStats>;

}  // namespace clvr
