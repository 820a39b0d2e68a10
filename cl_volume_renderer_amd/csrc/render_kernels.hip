// render_kernels.hip -- the `render` pass for gfx950, organised for wave64 hardware: its overview, k_bounce and launch_bounce.
//
// The reference runs one work-item per pixel through the whole path (ray_marching.cl:152-199):
// camera ray -> box entry -> primary march -> on a Hit, two distribution rays of up to three
// marches each -> accumulate -> read the accumulator back.  On a 64-wide wave that shape wastes the
// machine twice: only a fraction of the pixels hit anything, and the lanes that do walk paths of
// very different lengths.  Here the pass is split where the divergence is:
//
//   k_repack   (when volume / SDF / TF changed)  bricked step bytes + hit records (packed_volume.hpp);      scene_kernels.hip
//                                                k_macro_*: the exit-certificate table
//                                                k_start_*: the start-certificate table (a byte per voxel)
//                                                k_hull_*: the hull-certificate table (support of the event voxels in 4096 directions)
//   k_primary  (when the camera changed)         one lane per pixel: ray, box entry, primary march;         primary_kernels.hip
//                                                hits are compacted into 64-byte records with a
//                                                wave ballot + prefix (one atomic per wave);
//                                                misses keep their environment colour
//                                                a hit carries the start-certificate byte of the voxel
//                                                its distribution rays start from
//                                                and, beside its record, the plane of the hull table that
//                                                start point lies furthest in front of (or least behind)
//   k_bounce   (every launch, 1..64 seeds)       persistent waves pull (hit, seed) items from eight         this file
//                                                work queues; each lane runs the sample's two               (k_bounce2, two rays per
//                                                distribution rays as a small state machine; idle           lane: bounce_two_rays.hpp)
//                                                lanes are refilled by ballot/prefix compaction once
//                                                enough of them are idle; march steps and event
//                                                handling run in separate wave-wide phases
//   k_env_fixup / k_commit                       exact environment lookups the fast path could not          accumulate_kernels.hip
//                                                certify; per-hit sums -> float4 accumulator
//   k_resolve  (when a frame is wanted)          read the accumulator AFTER the pass (deterministic;        accumulate_kernels.hip
//                                                one legal outcome of the reference's race, SURVEY
//                                                fact 4), tone curve, RGBA8
//   k_ao       (shading = CLWH_SHADE_AO)         compute_ao (ray_marching.cl:104-149) per primary hit       primary_kernels.hip
//
// bounce_device.hpp: what these kernels share (lane states, finish_item, the fix-up record, certify_exit, scheduling statistics).
//
// The primary march does not depend on the pass's seed, so its result is kept while camera, volume,
// SDF and transfer function stay the same; per sample, every float operation is the one the reference
// kernel performs, in the same order (device_math.hpp), only scheduled differently.
#include <algorithm>

#include "bounce_two_rays.hpp"

namespace clvr {

#ifndef CLVR_CERT_PHASE_MIN_LANES
#define CLVR_CERT_PHASE_MIN_LANES 16
#endif
constexpr int kCertPhaseMinLanes = CLVR_CERT_PHASE_MIN_LANES;  // certificates are looked up once this many lanes of a wave wait for one
#ifndef CLVR_BOUNCE_WAVES_PER_SIMD
// Waves per SIMD.  With the event-only state in LDS (`cold` below) every variant of the kernel needs 64 registers or fewer, so
// the register file allows eight; LDS (22 KB per 256-thread block at 512^3: the cold state, the index tables, div255) allows seven
// blocks per CU.  Measured on the 64-pass launch, 6 / 7 / 8 (8 with 512-thread blocks) -> 4.27 / 4.14 / 4.22 ms
// (profiles/r02_sweep_k_bounce_lds_state.txt); before that change the kernel held 80 registers + 9 spilled and ran six.
#define CLVR_BOUNCE_WAVES_PER_SIMD 7
#endif
#ifndef CLVR_BOUNCE_THREADS
#define CLVR_BOUNCE_THREADS 256
#endif
constexpr int kBounceThreads = CLVR_BOUNCE_THREADS;  // the waves of a block share the LDS index tables

// k_bounce: ray_marching.cl:39-77 for every (hit, seed) item.
//
// Lane state machine.  MARCH lanes take march steps; a lane that reaches an event (Hit / Exit /
// 70 steps) parks in EVENT until the wave runs its event phase; IDLE lanes have no item.  The event
// phase has two halves with the refill between them, so a lane whose sample ends takes its next
// item and starts it in the same phase (k_bounce2 still parks fresh items through a step run).
//
// UNITS picks the refill (see there): true, a wave reserves whole units of 64 items and decodes a unit once on scalar operands -- fewer
// wave instructions and atomics, more L2-missing lines: long launches of tables without `gradient` rules, which are bound by VALU
// issue as much as by memory; false, every refill takes the queue's next n_idle items and each lane decodes its own -- launches that
// run at the line rate of their misses (`gradient` tables) and short launches, a chain of dependent waits.
template <bool USE_GRAD, int MODE, bool SMALL_VOLUME, bool UNITS>
__global__ __launch_bounds__(kBounceThreads, CLVR_BOUNCE_WAVES_PER_SIMD) void k_bounce(const RenderArgs a) {
  constexpr int SMALL = SMALL_VOLUME ? 2 : 0;  // 2: the per-axis index terms are read from LDS (packed_volume.hpp)
  VolumePacked vol = make_volume(a);
  index_tables_to_lds<SMALL>(vol, a, kBounceThreads);
  // c / 255.0f for the 256 possible colour bytes (a correctly rounded division is ~10 VALU instructions, the
  // kernel is VALU-issue bound, and every bounce needs four of them): one LDS read instead
  __shared__ float div255[256];
  if (threadIdx.x < 256u) div255[threadIdx.x] = (float)threadIdx.x / 255.0f;
  // {writes a colour, the colour} of every rule: a Hit found through its step byte reads its colour here, from LDS behind its hit
  // record, instead of the rule's flags and then its colour from the argument segment -- two more memory waits, one after the other,
  // in every opening half with such a Hit (128 bytes: the block still fits seven times into a CU's LDS at 512^3)
  __shared__ uint2 rule_color[CLWH_TF_MAX_RULES];
  stage_rule_colors(rule_color, a.tf);
  __syncthreads();
  // the hit count of this camera: a kernel argument, or still only on the device (single-pass launches, clwh_render)
  const uint32_t n_hits_arg = a.n_hits_on_device ? a.counters[CTR_HITS] : a.n_hits;
  const uint32_t n_hits = UNITS ? scalar_u32(n_hits_arg) : n_hits_arg;
  const uint32_t n_chunks = (n_hits + 63u) >> 6;
  const unsigned lane = lane_id();
  const unsigned home_queue_xcd = home_queue_of(a, (unsigned)(kBounceThreads / 64));
  const uint32_t home_queue = UNITS ? scalar_u32(home_queue_xcd % (unsigned)a.unit_queues) : home_queue_xcd;
  unsigned queue_dry_lane0 = 0u;  // !UNITS: bit q: queue q is known to be empty (lane 0's copy is the one that matters)
  bool exhausted = false;         // wave-uniform: the queues have no more items (UNITS: a copy of W_EXHAUSTED)
  // UNITS: the wave's place in the unit queues (see the refill) is wave-uniform and the refill works on it in scalar registers.  Between
  // two refills that state lives in lanes of ONE vector register (as the scalar registers the compiler spills do): the refill reads
  // it into scalar registers and writes it back, and the step loop and the event phase carry no scalar of it.
  enum : int { W_UNIT_H,      // the current unit: the hit its next item names,
               W_UNIT_LEFT,   // that many of its 64 items are left (0: the wave holds no unit),
               W_UNIT_SEED,   // its seed
               W_UNIT_S,      // and the seed's index (voxel-cache launches: the grants count seeds)
               W_TICKET_Q,    // the queue of the ticket below, kNoTicket: none is out
               W_QUEUE_DRY,   // bit q: queue q is known to be empty
               W_EXHAUSTED }; // every queue is dry and the wave holds no unit
  constexpr uint32_t kNoTicket = 0xFFu;
  uint32_t wave_state = lane == (unsigned)W_TICKET_Q ? kNoTicket : 0u;
#define WAVE_GET(k) ((uint32_t)__builtin_amdgcn_readlane((int)wave_state, (k)))
#define WAVE_SET(k, v) asm("v_writelane_b32 %0, %1, %2" : "+v"(wave_state) : "s"(scalar_u32(v)), "n"(k))
  // The ticket: lane 0's answer to an atomicAdd(head of queue W_TICKET_Q, 64), asked for but not yet looked at.  With `ahead` it is
  // asked when the unit before it becomes current, a step run or more before it is wanted; without, in the refill that wants it.
  uint32_t ticket = 0u;
  const bool ahead = a.unit_ahead != 0;
  // The sample.  What only the event phase needs lives in LDS, one dword per lane and field (a conflict-free
  // ds_read/ds_write each): the registers decide how many waves a SIMD holds, and with one dependent fetch per step it
  // is the number of waves in flight that sets the pace.
  enum : int { C_START_X, C_START_Y, C_START_Z,  // hit origin + hit direction: where both distribution rays start from
               C_NORMAL_X, C_NORMAL_Y, C_NORMAL_Z,
               C_ENTRY_LO,
               C_ENTRY_HI,  // bits 0-7: the entry's (a stored entry is -1, -2 or below 2^34: bit 7 is its sign); bits 8-20: the hit's hull-certificate code;
                            // bits 24-31: the hit's start-certificate byte.  With deferred hull grants (hull_defer below: the scene has a hull
                            // table, so no axis is longer than 2^11 and an entry is -1, -2 or below 2^33) the entry's keep bits 0-2, bit 2 its
                            // sign; the code moves to bits 3-15 and bits 16-23 hold the signed margin of the hit's plane in 1/16 voxels
               C_PIXEL, C_HIT, C_SEED,
               C_FIX,  // (fix + 2) << 2 | npend; fix: fix-up record of the sample (-1: none, -2: dropped, the buffer overflowed),
                       // npend: pending environment terms written to it
               C_BV_R, C_BV_G, C_BV_B, C_FIELDS };
  __shared__ uint32_t cold[C_FIELDS][kBounceThreads];
#define COLD(f) cold[f][threadIdx.x]
#define COLD_ENTRY_HI() ((uint32_t)((int32_t)(COLD(C_ENTRY_HI) << (32 - entry_hi_bits)) >> (32 - entry_hi_bits)))
  // path state; energies and colour carry over from distribution ray 1 into ray 2 (SURVEY "hard parts")
  Ray ray{{0, 0, 0}, {0, 0, 0}};
  float atten = 0.0f, r_energy = 0.0f, g_energy = 0.0f, b_energy = 0.0f;
  uint32_t color = 0u;
  int o = 0, i = 0;
  // scheduling state
  int st = ST_IDLE;        // ST_IDLE / ST_MARCH / ST_CERT / ST_EVENT + event
  int sd = 0;              // SDF value for the next step of a MARCH lane
  // steps this march may still take (0..70) in bits 24-30; below them kCertReady - (the path length the march still has to cover
  // before its next certificate look-up can succeed, see certify_exit): one add per step moves both, `no steps left` is one
  // unsigned compare, and the march may ask again once bit 23 is set.  (The distance is at most 126 cells, a march covers at most
  // 70 x 127 voxels: neither field reaches its neighbour.)
  // Bit 31, kArmed: the march waits for a deferred hull grant (opening half); its low field then counts down the path after which
  // its position is in front of the hit's plane, and the certificate phase grants it without a look-up.
  uint32_t march = 0u;
  constexpr uint32_t kOneStep = 1u << 24, kCertReady = 1u << 23, kArmed = 1u << 31;
  const bool cert_hint = a.cert_hint != 0;
  const int cert_min_lanes = a.cert_min_lanes;
  // a lane asks for an exit certificate when its next step is at least this long (wave-uniform)
  const int cert_at = a.cert_min_step != 0 ? a.cert_min_step : kCertNever;
  // first legs ask the hit's start-certificate byte: long launches only (launch_bounce); tables with `gradient` rules have no such table
  const bool start_cert = !USE_GRAD && a.cert_min_step != 0;
  const bool hull_cert = start_cert && a.hull_codes != nullptr;  // ... and the hit's hull-certificate code
  // ... and marches that start behind the hit's plane, or from a secondary hit, ask it too (CLWH_TUNE_HULL_DEFER=0: no)
  const bool hull_defer = hull_cert && a.hull_planes != nullptr;
  const int entry_hi_bits = hull_defer ? 3 : 8;  // C_ENTRY_HI's layout (wave-uniform)
  const uint32_t *hull_words = hull_defer ? a.hull_planes : a.hull_codes;  // the word per hit the refill reads
  // ... and a march that the hit's plane neither grants nor arms asks the plane tilted towards its own direction (CLWH_TUNE_HULL_TILT=0: no)
  const bool hull_tilt = hull_defer && a.hull_h != nullptr;
  // an armed lane's grant fires while it has at least this budget left: two constants and the flag -- J as a kernel argument, one more
  // scalar live across the step loop, gave every instance a private segment
  constexpr uint32_t kFireDefer = (uint32_t)(70 - kHullDeferSteps) * kOneStep, kFireTilt = (uint32_t)(70 - kHullTiltSteps) * kOneStep;
  BounceStats stats;

  // One pass of the loop: step run, closing half of the event phase, refill, opening half.  (First pass: no lane marches and no
  // lane has an event, so only the refill and the opening half do anything.)
  for (;;) {
    // ---- step phase: MARCH lanes step until fewer than kStepPhaseMinLanes are still marching -----
    if (__ballot(st == ST_MARCH) != 0ull) {
      do {
        stats.step(st);
        if (st == ST_MARCH) {
          // sd is an integer in 0..127: fmaxf is cl_max here
          ray.origin = ray.origin + ray.direction * fmaxf((float)sd, 0.5f);
          march += (uint32_t)sd - kOneStep;
          if (!USE_GRAD) {
            // Has the new position a voxel?  +0 <= coordinate < dimension is ONE unsigned compare of the float's bits per axis
            // (negative values, -0.0 and NaN all have larger patterns than any dimension).  Whatever fails it -- nearly always
            // a ray that left the volume; else the far face, NaN or -0.0 -- is sorted out exactly in the event phase (EV_CHECK),
            // at the event phase's price instead of eight more compares in every iteration of this loop.
            const bool has_voxel = __float_as_uint(ray.origin.x) < __float_as_uint((float)a.X) &&
                                   __float_as_uint(ray.origin.y) < __float_as_uint((float)a.Y) &&
                                   __float_as_uint(ray.origin.z) < __float_as_uint((float)a.Z);
            if (has_voxel) {
              // the step byte says everything a table without `gradient` rules needs (classify_step's last case)
              const unsigned q = vol.template step_marched<SMALL>(ray.origin.x, ray.origin.y, ray.origin.z);
              sd = (int)(q & 0x7Fu);
              if (q & 0x80u) st = ST_EVENT + EV_HIT_COLOR_PENDING;
              else if ((march & ~kArmed) < kOneStep) st = ST_EVENT + EV_NONE;
              // far from every surface: can the rest of this march be proven to exit?  (An armed lane asks as soon as it has covered its
              // path, however short its next step: its flag is larger than every threshold.)
              else if (((march & kArmed) | (uint32_t)sd) >= (uint32_t)cert_at && (march & kCertReady)) st = ST_CERT;
            } else {
              st = ST_EVENT + EV_CHECK;
            }
          } else if (exited_volume(vol, ray.origin)) {
            st = ST_EVENT + EV_EXIT;
          } else {
            int next_sd;
            bool pending = false;
            const bool is_hit = classify_step<USE_GRAD, SMALL, true>(vol, a.tf, ray.origin, color, next_sd, &pending);
            if (is_hit) {
              st = ST_EVENT + (pending ? EV_HIT_COLOR_PENDING : EV_HIT);
            } else if (march < kOneStep) {
              st = ST_EVENT + EV_NONE;
            } else {
              sd = next_sd;
              if (sd >= cert_at && (march & kCertReady)) st = ST_CERT;
            }
          }
        }
        // ---- exit certificates, inside the step loop: lanes park until enough of them wait (or nobody marches), one table
        // lookup each (certify_exit), and go back to marching or on to their Exit event; the loop, and with it the lane
        // count of the event phase, is the same as without certificates
        const int n_cert = __popcll(__ballot(st == ST_CERT));
        if (n_cert != 0 && (n_cert >= cert_min_lanes || __popcll(__ballot(st == ST_MARCH)) < a.step_min_lanes)) {
          stats.cert_begin(st, n_cert);
          // deferred hull grant: the lane has covered the path that puts it in front of its plane; with at most J (kHullDeferSteps, with
          // tilted planes kHullTiltSteps)
          // steps taken the theorem holds from here (hull_defer_delta0, clwh_internal.hpp) -- no look-up.  Later than that it is a march
          // like any other; with tilted planes (three times as many lanes are armed, 7.25 M instead of 2.3 M per configs[1] launch, and
          // 1.17 M of them get there late: profiles/bounce_hull_tilt_counters.txt) one whose next step is too short to ask the table
          // goes back to marching without a look-up.
          const bool was_armed = !USE_GRAD && st == ST_CERT && (march & kArmed) != 0u;
          const bool fired = was_armed && (march & ~kArmed) >= (hull_tilt ? kFireTilt : kFireDefer);
          const bool late = hull_tilt && was_armed && !fired && sd < cert_at;
          stats.hull_fired(fired, i == 8);
          stats.hull_late(late);
          if (st == ST_CERT) {
            if (!USE_GRAD) march &= ~kArmed;  // (no lane of a USE_GRAD instance is ever armed)
            int away;
            if (fired && !kStartCertVerify) {
              st = ST_EVENT + EV_EXIT;
            } else if (late) {
              st = ST_MARCH;  // (bit 23 stays set: it asks at its next step that is long enough)
            } else if (certify_exit(a, ray.origin, ray.direction, (int)(march >> 24), away)) {
              st = ST_EVENT + EV_EXIT;  // the march WOULD end in Exit_volume; only its direction matters from here on
            } else {
              // it tries again at its next step that is long enough (trying less often -- only once the step has doubled, or grown by
              // half -- left more lines to fetch than the look-ups cost: 4.03 / 3.92 / 3.91 ms), but not before it has covered the
              // distance the refusing entry names (CLWH_TUNE_CERT_HINT=0: at once, as before the table had hints)
              march = (march & ~(kOneStep - 1u)) | (kCertReady - (uint32_t)(cert_hint ? away : 0));
              st = ST_MARCH;
            }
          }
          stats.cert_end(st, n_cert);
        }
      } while (__popcll(__ballot(st == ST_MARCH)) >= a.step_min_lanes);
    }

    // ---- event phase, closing half: every parked lane handles its event, up to the end of its sample -----
    // What the lane does next is left in `st` for the opening half: ST_EVENT + EV_START (start distribution ray `o` from the
    // primary hit), + EV_HIT / EV_HIT_COLOR_PENDING (bounce from this hit; with i > 10 its bounced ray is not marched and ray
    // `o` starts instead), + EV_NONE (march on); ST_IDLE when the sample has ended.  No vector crosses the refill between the halves.
    stats.closing_half(st);
    if (st >= ST_EVENT) {
      int ev = st - ST_EVENT;
      if (ev == EV_CHECK) {
        // The step loop's quick test found no voxel at the new position: the reference's own tests, in its order
        // (utility_ray.cl:157-168: exited? event? out of steps?).  Nearly always the ray has left the volume.  The rare march
        // that goes on -- a position exactly on the far face, NaN, -0.0 -- is finished right here, step by literal step: sent
        // back to the step loop it would come here again after every step (a NaN position has no voxel ever), and in a short
        // launch the seventy event phases of one such ray were the tail of the whole launch (0.30 -> 0.44 ms per pass).
        for (;;) {
          if (exited_volume(vol, ray.origin)) { ev = EV_EXIT; break; }
          int next_sd;
          bool pending = false;
          if (classify_step<USE_GRAD, SMALL, true>(vol, a.tf, ray.origin, color, next_sd, &pending)) {
            ev = pending ? EV_HIT_COLOR_PENDING : EV_HIT;
            break;
          }
          if ((march & ~kArmed) < kOneStep) { ev = EV_NONE; break; }
          ray.origin = ray.origin + ray.direction * fmaxf((float)next_sd, 0.5f);
          march -= kOneStep;
        }
      }
      stats.march_end(a.counters, ev);
      bool ended = false;  // distribution ray `o` has ended: the next one starts from the primary hit, or the sample is complete

      if (ev == EV_EXIT) {
        // ray_marching.cl:54-62: left the volume -> environment light ends this distribution ray
        // i is 8, 9 or 10 here (it starts at 8 and a path ends once it exceeds 10); the quotients are folded at compile time
        const float factor = i == 8 ? 8.0f / 8.0f : (i == 9 ? 8.0f / 9.0f : (i == 10 ? 8.0f / 10.0f : 8.0f / (float)i));
        const float p_r = atten * r_energy, p_g = atten * g_energy, p_b = atten * b_energy;
        uint32_t light = 0u;
        const uint32_t fix_word = COLD(C_FIX);
        int fix = (int)(fix_word >> 2) - 2, npend = (int)(fix_word & 3u);
        bool certain = (fix == -1) && sample_environment_map_fast(a.env, a.env_w, a.env_h, ray.direction, light);
        if (certain) {
          // uint += float: promote, add, truncate back
          COLD(C_BV_R) = f2u((float)COLD(C_BV_R) + p_r * (float)(light & 255u) * factor / 1.0f);
          COLD(C_BV_G) = f2u((float)COLD(C_BV_G) + p_g * (float)((light >> 8) & 255u) * factor / 1.0f);
          COLD(C_BV_B) = f2u((float)COLD(C_BV_B) + p_b * (float)((light >> 16) & 255u) * factor / 1.0f);
        } else {
          if (fix == -1) {
            // first undecided lookup of this sample: open a fix-up record
            const uint32_t slot = atomicAdd(&a.counters[CTR_FIXUPS], 1u);
            if (slot < a.fixup_capacity) {
              fix = (int)slot;
              uint32_t *rec = a.fixups + (size_t)slot * kFixupDwords;
              rec[0] = COLD(C_HIT);
              rec[1] = COLD(C_ENTRY_LO);
              rec[2] = COLD_ENTRY_HI();
              rec[3] = COLD(C_PIXEL);
              rec[4] = COLD(C_BV_R); rec[5] = COLD(C_BV_G); rec[6] = COLD(C_BV_B);
            } else {
              a.sticky_flags[0] = 1u;  // reported by the host as an error; the sample is dropped
              fix = -2;
            }
          }
          if (fix >= 0) {
            uint32_t *e = a.fixups + (size_t)fix * kFixupDwords + 8 + 7 * npend;
            e[0] = __float_as_uint(p_r); e[1] = __float_as_uint(p_g); e[2] = __float_as_uint(p_b);
            e[3] = __float_as_uint(factor);
            e[4] = __float_as_uint(ray.direction.x); e[5] = __float_as_uint(ray.direction.y);
            e[6] = __float_as_uint(ray.direction.z);
            npend += 1;
          }
          COLD(C_FIX) = ((uint32_t)(fix + 2) << 2) | (uint32_t)npend;
        }
        o += 1;
        ev = EV_START;
        ended = true;
      } else if (ev == EV_HIT || ev == EV_HIT_COLOR_PENDING) {
        // ray_marching.cl:63-72: secondary hit; the bounce itself is the opening half's.  i > 10: third march of this
        // distribution ray, see there
        i += 1;
        if (i > 10) {
          o += 1;
          ended = true;
        }
      } else if (ev == EV_NONE) {
        // 70 steps without an event: the next march continues from where this one stopped
        i += 1;
        if (i > 10) {
          o += 1;
          ev = EV_START;
          ended = true;
        }
      }

      if (ended && o > 2) {
        const int fix = (int)(COLD(C_FIX) >> 2) - 2;
        if (fix == -1)
          finish_item<MODE>(a, (int64_t)(((uint64_t)COLD_ENTRY_HI() << 32) | (uint64_t)COLD(C_ENTRY_LO)), COLD(C_HIT), COLD(C_PIXEL) & 0xFFFFu,
                            COLD(C_PIXEL) >> 16, COLD(C_BV_R), COLD(C_BV_G), COLD(C_BV_B));
        else if (fix >= 0) a.fixups[(size_t)fix * kFixupDwords + 7] = COLD(C_FIX) & 3u;  // k_env_fixup finishes it
        st = ST_IDLE;
      } else {
        st = ST_EVENT + ev;
      }
    }

    // ---- refill, between the two halves of the event phase: idle lanes pull consecutive items of the unit queues ----
    // (ballots and shuffles: all 64 lanes pass here.)  A lane whose sample has just ended in the closing half takes its next
    // item now and starts it in the opening half of the same pass; it never sits out a step run without a ray.
    // An item is (hit, seed); 64 consecutive items of a queue are one unit = (chunk of 64 consecutive hits,
    // seed).  Units are dealt to eight queues by chunk number; a wave serves the queue of the XCD it runs on
    // first (so the seeds of one chunk -- thousands of rays leaving the same few voxels -- meet in ONE L2)
    // and steals from the other queues when its own is dry.  Two forms (UNITS; launch_bounce picks).  The dealing by
    // refill, second below: as soon as `refill_min_lanes` lanes are idle they take the queue's next n_idle items with one
    // atomic and every lane decodes its own.  Whole units, first below: a wave reserves WHOLE units, one atomicAdd(head, 64)
    // each (every head is a multiple of 64), and decodes a unit once, on scalar operands: chunk -> first hit, seed
    // index -> seed.  As soon as `refill_min_lanes` lanes are idle they take the next items of the wave's unit --
    // h = unit_h + rank, no division and no per-lane seed load -- and, where that unit ends, go on in the next one
    // in the same refill, so a wave does not drain down to its slowest sample before it gets new work.  A refill
    // that stays inside its unit (three in four on the headline) waits once, for the hit records and hull words,
    // which are issued together; one that uses its unit up waits for the atomic's answer first.  With `ahead`
    // (CLWH_TUNE_UNIT_AHEAD=1; off: launch_bounce) the unit after the current one is asked for when the current one
    // starts and that wait goes too.  Placement only affects speed.
    const unsigned long long idle_mask = __ballot(st == ST_IDLE);
    const uint32_t n_idle = (uint32_t)__popcll(idle_mask);
    if (UNITS) exhausted = WAVE_GET(W_EXHAUSTED) != 0u;
    if (!exhausted && n_idle >= (uint32_t)a.refill_min_lanes) {
      if constexpr (UNITS) {
        uint32_t ask_ahead = kNoTicket;  // the queue to ask for the unit after the one this refill makes current: asked below, behind the hit records
        // every head sits on its own 128-byte line: same-address atomics serialise at one L2 channel
        auto ask_ticket = [&](uint32_t q, uint32_t &answer) {
          // (the empty statement hides that the lane number never changes: the compiler would split the loops below into a copy for
          // lane 0 and one for the rest, and everything in them would sit in vector registers behind exec masks)
          uint32_t asker = lane;
          asm volatile("" : "+v"(asker));
          if (asker == 0u) answer = atomicAdd(&a.counters[CTR_QUEUE_STRIDE * (q + 1u)], 64u);
        };
        const uint32_t NQ = (uint32_t)a.unit_queues, S = (uint32_t)a.n_seeds, G = (uint32_t)a.unit_group;
        const uint32_t KB = (uint32_t)a.unit_block_log2, n_blocks = (n_chunks + (1u << KB) - 1u) >> KB;
        uint32_t unit_h = WAVE_GET(W_UNIT_H), unit_left = WAVE_GET(W_UNIT_LEFT), unit_seed = WAVE_GET(W_UNIT_SEED);
        uint32_t unit_s = MODE == CLWH_ACCUM_VOXEL_CACHE ? WAVE_GET(W_UNIT_S) : 0u;
        uint32_t ticket_q = WAVE_GET(W_TICKET_Q), queue_dry = WAVE_GET(W_QUEUE_DRY);
        const uint32_t rank = st == ST_IDLE ? prefix_count(idle_mask) : 64u;  // this idle lane's place among the idle ones
        uint32_t taken = 0u;                                                  // items handed out in this refill (wave-uniform)
        uint32_t h = 0xFFFFFFFFu, s = 0u, seed = 0u;                          // this lane's item; 2^32 - 1: none
        // blocks of 2^unit_block_log2 consecutive chunks are dealt round-robin to the queues (a block past the
        // last chunk is padding: its items name hits that do not exist and are skipped)
        auto chunks_of = [&](uint32_t q) { return scalar_u32((n_blocks + NQ - 1u - q) / NQ) << KB; };
        for (;;) {  // at most two rounds: a fresh unit has 64 items
          while (unit_left == 0u) {
            // the next unit becomes the current one
            uint32_t q = ticket_q, answer = ticket;
            ticket_q = kNoTicket;
            if (q == kNoTicket) {
              // no ticket out (on demand; a queue ran dry; the tail of a queue): ask the first queue, from home on, not known to be dry,
              // and wait for the answer
              for (uint32_t tries = 0; tries < NQ && q == kNoTicket; ++tries) {
                const uint32_t t = home_queue + tries - (home_queue + tries >= NQ ? NQ : 0u);
                if (chunks_of(t) != 0u && ((queue_dry >> t) & 1u) == 0u) q = t;
              }
              if (q == kNoTicket) break;  // every queue is dry
              ask_ticket(q, answer);
            }
            const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)answer, 0) >> 6;  // the unit's number in its queue
            const uint32_t chunks_q = chunks_of(q), units_q = chunks_q * S;
            ask_ahead = kNoTicket;
            if (p >= units_q) {
              queue_dry |= 1u << q;  // remembered: never asked again
              continue;
            }
            if (p + 1u >= units_q) queue_dry |= 1u << q;
            else if (ahead) ask_ahead = q;
            // queue order: groups of `unit_group` chunks, inside a group seed-major -- the seeds of a chunk are
            // `unit_group` units apart (their accumulation atomics do not collide) yet close enough to find
            // each other's voxels still in L2
            const uint32_t g = scalar_u32(p / (G * S)), r = p - g * (G * S);
            const uint32_t in_group = min(G, chunks_q - g * G);  // the last group may be short
            const uint32_t s_u = scalar_u32(r / in_group), ch = g * G + (r - s_u * in_group);
            const uint32_t chunk = ((q + NQ * (ch >> KB)) << KB) + (ch & ((1u << KB) - 1u));
            if (chunk >= n_chunks) continue;  // padding
            unit_h = chunk * 64u;
            unit_left = 64u;
            unit_s = s_u;
            unit_seed = (uint32_t)a.seeds[s_u];
          }
          if (unit_left == 0u) {
            exhausted = true;  // every queue is dry and the wave holds no unit
            break;
          }
          const uint32_t take = min(n_idle - taken, unit_left);
          if (rank - taken < take) {  // (a lane served in the first round: rank < taken, the difference wraps)
            h = unit_h + (rank - taken);
            s = unit_s;
            seed = unit_seed;
          }
          unit_h += take;
          unit_left -= take;
          taken += take;
          if (taken == n_idle) break;
        }
        WAVE_SET(W_UNIT_H, unit_h); WAVE_SET(W_UNIT_LEFT, unit_left); WAVE_SET(W_UNIT_SEED, unit_seed);
        if (MODE == CLWH_ACCUM_VOXEL_CACHE) WAVE_SET(W_UNIT_S, unit_s);
        WAVE_SET(W_TICKET_Q, ask_ahead != kNoTicket ? ask_ahead : ticket_q); WAVE_SET(W_QUEUE_DRY, queue_dry); WAVE_SET(W_EXHAUSTED, exhausted ? 1u : 0u);
        stats.refill(taken);
        if (h < n_hits) {  // (an item of the last chunk may name a hit past the last one: skipped)
          const uint4 *src = reinterpret_cast<const uint4 *>(&a.hits[h]);
          const uint4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
          const uint32_t plane = hull_cert ? hull_words[h] : 0u;  // (one layout or the other: wave-uniform masks and shift)
          const f3 hit_origin = f3{__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z)};
          const f3 hit_direction = f3{__uint_as_float(q0.w), __uint_as_float(q1.x), __uint_as_float(q1.y)};
          const f3 start = hit_origin + hit_direction;  // ray_bounce_fake_reflectance's origin (utility_ray.cl:100-103)
          color = q2.y;
          const int64_t entry = (int64_t)(((uint64_t)q2.w << 32) | (uint64_t)q2.z);
          bool granted = true;
          if (MODE == CLWH_ACCUM_VOXEL_CACHE)
            granted = a.grants ? s < a.grants[h] : (entry >= 0 && cache_take_token(a.cache, entry, 256u));
          if (granted) {
            COLD(C_START_X) = __float_as_uint(start.x); COLD(C_START_Y) = __float_as_uint(start.y); COLD(C_START_Z) = __float_as_uint(start.z);
            COLD(C_NORMAL_X) = q1.z; COLD(C_NORMAL_Y) = q1.w; COLD(C_NORMAL_Z) = q2.x;
            COLD(C_ENTRY_LO) = q2.z;
            COLD(C_ENTRY_HI) = (q2.w & ((1u << entry_hi_bits) - 1u)) | ((plane & 0x1FFFu) << entry_hi_bits) | (plane & (hull_defer ? 0x00FF0000u : 0u)) | (q3.z << 24);
            COLD(C_PIXEL) = q3.x;
            COLD(C_HIT) = h;
            COLD(C_SEED) = seed;
            COLD(C_FIX) = (uint32_t)(-1 + 2) << 2;
            COLD(C_BV_R) = 0u; COLD(C_BV_G) = 0u; COLD(C_BV_B) = 0u;
            r_energy = div255[color & 255u];
            g_energy = div255[(color >> 8) & 255u];
            b_energy = div255[(color >> 16) & 255u];
            o = 1;
            st = ST_EVENT + EV_START;  // ready to bounce from its primary hit
          } else if (a.contrib_out) {
            uint32_t *q = a.contrib_out + ((size_t)(q3.x >> 16) * (size_t)a.launch_w + (q3.x & 0xFFFFu)) * 4;
            q[0] = 0u; q[1] = 0u; q[2] = 0u; q[3] = 0u;
          }
        }
        // the ticket for the unit after the one that has just become current: nobody looks at the answer before the next refill that
        // uses up a unit, a step run or more from here
        if (ask_ahead != kNoTicket) ask_ticket(ask_ahead, ticket);
      } else {
        // every refill takes the next n_idle items of a queue with one atomic, and each lane decodes its own item
        const uint32_t NQ = (uint32_t)a.unit_queues, S = (uint32_t)a.n_seeds, G = (uint32_t)a.unit_group;
        const uint32_t KB = (uint32_t)a.unit_block_log2, n_blocks = (n_chunks + (1u << KB) - 1u) >> KB;
        uint32_t base = 0u, count = 0u, q_sel = 0u;
        if (lane == 0u) {
          for (uint32_t tries = 0; tries < NQ && count == 0u; ++tries) {
            const uint32_t q = (home_queue + tries) % NQ;
            // blocks of 2^unit_block_log2 consecutive chunks are dealt round-robin to the queues (a block past the
            // last chunk is padding: its items name hits that do not exist and are skipped)
            const uint32_t blocks_q = (n_blocks + NQ - 1u - q) / NQ;
            const uint32_t chunks_q = blocks_q << KB;
            if (chunks_q == 0u || ((queue_dry_lane0 >> q) & 1u)) continue;
            const uint32_t total = chunks_q * S * 64u;
            // every head sits on its own 128-byte line: same-address atomics serialise at one L2 channel
            const uint32_t p = atomicAdd(&a.counters[CTR_QUEUE_STRIDE * (q + 1u)], n_idle);
            if (p + n_idle >= total) queue_dry_lane0 |= 1u << q;  // remembered: never asked again
            if (p < total) {
              base = p;
              count = min(n_idle, total - p);
              q_sel = q;
            }
          }
        }
        base = __shfl(base, 0);
        count = __shfl(count, 0);
        q_sel = __shfl(q_sel, 0);
        stats.refill(count);
        if (count == 0u) {
          exhausted = true;  // every queue is dry
        } else if (st == ST_IDLE) {
          const uint32_t rank = (uint32_t)__popcll(idle_mask & ((1ull << lane) - 1ull));
          if (rank < count) {
            const uint32_t item = base + rank, p = item >> 6;
            // queue order: groups of `unit_group` chunks, inside a group seed-major (as above)
            // (units per queue stay below 2^24: launch_bounce checks)
            const uint32_t chunks_q = ((n_blocks + NQ - 1u - q_sel) / NQ) << KB;  // wave-uniform: scalar
            uint32_t r, c_in;
            const uint32_t g = udivmod24(p, G * S, r);
            const uint32_t in_group = min(G, chunks_q - g * G);  // the last group may be short
            const uint32_t s = udivmod24(r, in_group, c_in), ch = g * G + c_in;
            const uint32_t chunk = ((q_sel + NQ * (ch >> KB)) << KB) + (ch & ((1u << KB) - 1u));
            const uint32_t h = chunk * 64u + (item & 63u);
            if (h < n_hits) {  // (an item of the last chunk may name a hit past the last one: skipped)
              const uint4 *src = reinterpret_cast<const uint4 *>(&a.hits[h]);
              const uint4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
              const f3 hit_origin = f3{__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z)};
              const f3 hit_direction = f3{__uint_as_float(q0.w), __uint_as_float(q1.x), __uint_as_float(q1.y)};
              const f3 start = hit_origin + hit_direction;  // ray_bounce_fake_reflectance's origin (utility_ray.cl:100-103)
              color = q2.y;
              const int64_t entry = (int64_t)(((uint64_t)q2.w << 32) | (uint64_t)q2.z);
              bool granted = true;
              if (MODE == CLWH_ACCUM_VOXEL_CACHE)
                granted = a.grants ? s < a.grants[h] : (entry >= 0 && cache_take_token(a.cache, entry, 256u));
              if (granted) {
                COLD(C_START_X) = __float_as_uint(start.x); COLD(C_START_Y) = __float_as_uint(start.y); COLD(C_START_Z) = __float_as_uint(start.z);
                COLD(C_NORMAL_X) = q1.z; COLD(C_NORMAL_Y) = q1.w; COLD(C_NORMAL_Z) = q2.x;
                COLD(C_ENTRY_LO) = q2.z;
                const uint32_t plane = hull_cert ? hull_words[h] : 0u;  // (one layout or the other: wave-uniform masks and shift)
                COLD(C_ENTRY_HI) = (q2.w & ((1u << entry_hi_bits) - 1u)) | ((plane & 0x1FFFu) << entry_hi_bits) | (plane & (hull_defer ? 0x00FF0000u : 0u)) | (q3.z << 24);
                COLD(C_PIXEL) = q3.x;
                COLD(C_HIT) = h;
                COLD(C_SEED) = (uint32_t)a.seeds[s];
                COLD(C_FIX) = (uint32_t)(-1 + 2) << 2;
                COLD(C_BV_R) = 0u; COLD(C_BV_G) = 0u; COLD(C_BV_B) = 0u;
                r_energy = div255[color & 255u];
                g_energy = div255[(color >> 8) & 255u];
                b_energy = div255[(color >> 16) & 255u];
                o = 1;
                st = ST_EVENT + EV_START;  // ready to bounce from its primary hit
              } else if (a.contrib_out) {
                uint32_t *q = a.contrib_out + ((size_t)(q3.x >> 16) * (size_t)a.launch_w + (q3.x & 0xFFFFu)) * 4;
                q[0] = 0u; q[1] = 0u; q[2] = 0u; q[3] = 0u;
              }
            }
          }
        }
      }
    }
    stats.fresh_items(st, o);
    if (__ballot(st != ST_IDLE) == 0ull) {
      if (exhausted && lane == 0u) stats.flush<false>(a.counters);
      if (exhausted) break;  // nothing in flight and nothing left to fetch
      continue;              // every fetched sample was refused its token (or was padding): fetch again (no lane marches, no lane has an event)
    }

    // ---- event phase, opening half: the bounce is one shared block, then the march's first SDF read ---------
    bool sc_tried = false, sc_granted = false;  // this lane's first leg asked for / holds a start certificate
    bool hc_tried = false, hc_granted = false;  // ... a hull certificate
    bool rb_tried = false, rb_granted = false;  // this lane's rebound from a secondary hit asked for / holds a hull certificate
    uint32_t armed_path = 0u;                   // != 0: this lane's march may be granted once it has covered this path (deferred grant)
    bool tl_tried = false, tl_granted = false, tl_armed = false;  // this lane's march asked a tilted plane / holds its certificate / is armed by it
    bool started = false;                       // this lane starts a march in this half (statistics)
    if (st >= ST_EVENT) {
      const int ev = st - ST_EVENT;
      bool start_path = (ev == EV_START);  // begin distribution ray `o` from the primary hit
      bool bounce = false, from_hit = false;
      f3 bn{0, 0, 0}, bstart{0, 0, 0};  // the bounce's normal and its origin + direction
      int bseed = 0;                    // its seed, less the sample's

      if (ev == EV_HIT || ev == EV_HIT_COLOR_PENDING) {
        // ray_marching.cl:63-72: secondary hit -> bounce around the local normal, attenuate; the rule colour (still
        // pending when the Hit came through the step byte) and the gradient arrive in one 8-byte load; the colour is rule_color's
        bn = -normalize3(hit_gradient_and_color<SMALL>(vol, rule_color, ray.origin, ev == EV_HIT_COLOR_PENDING, color));
        bstart = ray.origin + ray.direction;
        bseed = o + i - 1;  // (the closing half has counted this march already)
        bounce = true;
        from_hit = true;
        if (i > 10) {
          // third march of this distribution ray: the reference still multiplies the energies (they
          // carry into the next distribution ray) but its bounced ray is never marched
          r_energy *= div255[color & 255u];
          g_energy *= div255[(color >> 8) & 255u];
          b_energy *= div255[(color >> 16) & 255u];
          bounce = false;
          start_path = true;
        }
      }

      if (start_path) {
        // ray_marching.cl:48: bounce from the primary hit around the primary normal
        bn = f3{__uint_as_float(COLD(C_NORMAL_X)), __uint_as_float(COLD(C_NORMAL_Y)), __uint_as_float(COLD(C_NORMAL_Z))};
        bstart = f3{__uint_as_float(COLD(C_START_X)), __uint_as_float(COLD(C_START_Y)), __uint_as_float(COLD(C_START_Z))};
        bseed = o;
        bounce = true;
        from_hit = false;
      }

      if (bounce) {
        // ray_bounce_fake_reflectance, then origin += normal*2 (ray_marching.cl:48-50 / :65-67)
        const float roughness = div255[color >> 24];
        const uint32_t pixel = COLD(C_PIXEL);
        Ray nr;
        nr.direction = hemisphere_reflective(pixel & 0xFFFFu, pixel >> 16, bn, (int)COLD(C_SEED) + bseed, roughness);
        nr.origin = bstart + bn * 2.0f;
        const float d = fabsf(dot3(nr.direction, bn));
        if (from_hit) {
          atten *= d;
          r_energy *= div255[color & 255u];
          g_energy *= div255[(color >> 8) & 255u];
          b_energy *= div255[(color >> 16) & 255u];
        } else {
          atten = d;
          i = 8;
          if (start_cert) {
            // Start certificate.  All first legs of a hit start from the same point, whose voxel k_primary has looked up in the
            // "free from here" table (k_start_*, scene_kernels.hip): bit `octant` says that the box from that voxel to the volume
            // corner this direction heads for holds no voxel that may be an event.  The march's coordinates are monotone, so it can
            // only end in Exit_volume or run out of steps, and start_cert_dmin (clwh_internal.hpp) is the smallest direction
            // component with which it provably leaves within its 70 steps.  Like every exit certificate it ends the march at once:
            // only the direction is used from here on, and not one step byte is fetched.
            sc_tried = true;
            const uint32_t word = COLD(C_ENTRY_HI);
            sc_granted = start_certificate(word >> 24, nr.direction, a.start_cert_dmin);
          }
        }
        // Hull certificate.  k_primary has found a plane {x : n_k . x = h_k} with every corner of every event voxel behind it
        // (k_hull_*, scene_kernels.hip); a march that starts in front of it with direction . n_k >= hull_cert_delta0
        // (clwh_internal.hpp: the proof) moves away from every event voxel linearly with its path, the steps grow with that
        // distance, and it provably leaves within its 70 steps.  The proof that fits a leg leaving a convex surface, where the
        // octant's box nearly always holds the object.  First legs start at the point P the plane was chosen for; with hull_defer a
        // rebound from a secondary hit asks the same plane with its own margin, m_P + n_k . (start - P), and a march that starts up to
        // kHullDeferDeficit behind the plane is armed: it is granted in the certificate phase once it has got in front.
        if (hull_cert && (hull_defer || !from_hit)) {
          const uint32_t word = COLD(C_ENTRY_HI);
          const uint32_t code = (word >> entry_hi_bits) & 0x1FFFu;
          const f3 n = hull_direction(code - 1u);
          const float dn = dot3(nr.direction, n);
          const f3 dir = nr.direction;
          const bool dir_ok = fminf(fminf(fabsf(dir.x), fabsf(dir.y)), fabsf(dir.z)) >= 0.0009765625f && (dir.x + dir.y) + dir.z == (dir.x + dir.y) + dir.z;
          float m = hull_defer ? (float)((int32_t)(word << 8) >> 24) * (1.0f / (float)kHullMarginScale) : 0.0f;
          if (from_hit) {
            const f3 p = f3{__uint_as_float(COLD(C_START_X)), __uint_as_float(COLD(C_START_Y)), __uint_as_float(COLD(C_START_Z))} +
                         f3{__uint_as_float(COLD(C_NORMAL_X)), __uint_as_float(COLD(C_NORMAL_Y)), __uint_as_float(COLD(C_NORMAL_Z))} * 2.0f;
            m = m + dot3(n, f3{nr.origin.x - p.x, nr.origin.y - p.y, nr.origin.z - p.z});
          }
          const bool tried = code != 0u, granted = tried && dir_ok && m >= 0.0f && dn >= a.hull_delta0;
          if (from_hit) { rb_tried = tried; rb_granted = granted; }
          else { hc_tried = tried && m >= 0.0f; hc_granted = granted; }
          if (tried && dir_ok && !sc_granted && m < 0.0f && m >= -kHullDeferDeficit && dn >= a.hull_defer_delta0)
            armed_path = (uint32_t)ceilf(-m * __builtin_amdgcn_rcpf(dn) * (1.0f + 0x1p-19f));  // at least -m / dn, at most 8 x 64 + 1
          // Tilted plane (clwh_internal.hpp: the proof).  What the hit's own plane neither grants nor arms asks the plane of the same table
          // whose normal is n_k (a hit without a word: the bounce's normal) turned towards the direction of travel just far enough that
          // direction . n' reaches the target: found in closed form, its h_k' read from the 16 KB copy of the table's fourth column.
          if (hull_tilt && dir_ok && !granted && !sc_granted && armed_path == 0u) {
            const f3 n0{tried ? n.x : bn.x, tried ? n.y : bn.y, tried ? n.z : bn.z};
            const float c = dot3(dir, n0);
            const float lambda = c >= a.hull_tilt_target ? 0.0f : a.hull_tilt_gain * __builtin_amdgcn_sqrtf(fmaxf(1.0f - c * c, 0.0f)) - c;
            const unsigned k2 = hull_cell(f3{n0.x + lambda * dir.x, n0.y + lambda * dir.y, n0.z + lambda * dir.z});
            const f3 n2 = hull_direction(k2);
            const float dn2 = dot3(dir, n2), m2 = dot3(n2, nr.origin) - a.hull_h[k2];
            tl_tried = true;
            if (m2 >= 0.0f && dn2 >= a.hull_delta0) {
              tl_granted = true;
            } else if (m2 < 0.0f && dn2 >= a.hull_defer_delta0) {
              const float need = ceilf(-m2 * __builtin_amdgcn_rcpf(dn2) * (1.0f + 0x1p-19f));  // at least -m2 / dn2 (+inf: a table without events)
              if (need <= (float)kHullTiltPath) { armed_path = (uint32_t)need; tl_armed = true; }
            }
          }
        }
        ray = nr;
      }

      if ((sc_granted || hc_granted || rb_granted || tl_granted) && !kStartCertVerify) {
        st = ST_EVENT + EV_EXIT;  // the next closing half takes it from here
      } else {
        // start (or continue) a march: its first SDF read is at trunc(origin) (utility_ray.cl:148-150)
        sd = (int)(vol.template step_i<SMALL>(f2i(ray.origin.x), f2i(ray.origin.y), f2i(ray.origin.z)) & 0x7Fu);
        march = 70u * kOneStep + kCertReady;
        if (armed_path != 0u) march = kArmed + 70u * kOneStep + kCertReady - armed_path;
        st = ST_MARCH;
        started = true;
      }
    }
    stats.start_cert(sc_tried, sc_granted);
    stats.hull_cert(hc_tried, hc_granted, hc_granted && sc_granted);
    stats.hull_more(rb_tried, rb_granted, armed_path != 0u && !tl_armed && st == ST_MARCH, i == 8);
    stats.hull_tilt(tl_tried, tl_granted, tl_armed && st == ST_MARCH, started, i == 8);
  }
#undef COLD_ENTRY_HI
#undef COLD
#undef WAVE_SET
#undef WAVE_GET
}

hipError_t launch_bounce(const RenderArgs &a_in, hipStream_t s) {
  RenderArgs a = a_in;
  const uint64_t total = (uint64_t)a.n_hits * (uint64_t)a.n_seeds;
  if (total == 0) return hipSuccess;
  // persistent grid: enough waves to fill the chip (256 CUs x 32 waves), never more than the work
  const uint64_t waves_needed = (total + 63u) / 64u;
  constexpr unsigned wpb = (unsigned)kBounceThreads / 64u;  // waves per block; bounce_max_blocks counts 256-thread blocks
  // (two frame jobs in flight on two streams share the chip: a rank's share of a multi-GPU job -- a few million items -- runs 9 % (4 ranks)
  // to 18 % (8 ranks) faster when each launch takes half the grid, CLWH_TUNE_BLOCKS=1024, which bench.py sets for such runs; alone on the
  // GPU the same launch is 20-30 % slower on half the grid, so the default stays the full chip: profiles/r02_emulate_rank_grid_sweep.txt)
  const unsigned blocks = (unsigned)std::min<uint64_t>((waves_needed + wpb - 1u) / wpb, ((uint64_t)a.bounce_max_blocks * 4u + wpb - 1u) / wpb);
  const dim3 grid(blocks), block(kBounceThreads);
  // Scheduling thresholds (0 = automatic).  A launch with only a few units per wave (one or a few passes) is
  // bound by its longest dependent chain: every wave steps its samples to completion and refills when empty.
  // A long launch is bound by VALU issue: lanes refill at 16 idle and the march phase ends at 16 marching lanes.
  // Measured crossover on the headline scene: between 4 and 8 passes per launch = about 6 units per wave
  // (round-1 sweep, git history: profiles/r01_tune_refill_step_thresholds.txt; re-swept in profiles/r02_tune_k_bounce_knobs.txt).
  // (with the hit count still on the device n_hits is the pixel count, an upper bound; the class follows the estimate: the last
  // camera's count with slack, clwh_render)
  const uint64_t waves_likely = ((uint64_t)a.n_hits_estimate * (uint64_t)a.n_seeds + 63u) / 64u;
  const bool long_launch = a.force_long_launch || waves_likely >= 6u * (uint64_t)blocks * wpb;
  if (a.step_min_lanes <= 0) a.step_min_lanes = long_launch ? 16 : 1;
  if (a.refill_min_lanes <= 0) a.refill_min_lanes = long_launch ? 16 : 64;
  // certificates: a long launch looks them up once 16 lanes of a wave wait for one (8: 4.32, 16: 4.25, 4: 4.42 ms); a short launch
  // is bound by its longest chain of dependent fetches, where the look-up is one more of them: 0.263 ms per pass without, 0.277 with
  a.cert_min_lanes = kCertPhaseMinLanes;
  if (!long_launch) a.cert_min_step = 0;
  if (!bounce_queues_fit(a.n_hits, a.unit_block_log2, a.n_seeds)) return hipErrorInvalidValue;
  // The refill's form (k_bounce's UNITS).  Whole units per wave cost L2-missing lines (+5.7 % on the headline: a wave owns a unit for
  // about four refills, so a wider stretch of the queue is in flight and the seeds of a chunk share fewer lines) and save wave
  // instructions (-4.5 %) and three atomics in four.  The long launch of a table without `gradient` rules gains 2 % by that; the launch
  // of a `gradient` table runs at the line rate of its misses and lost 6 %, and the short launch, a chain of dependent waits, lost 2 %
  // to atomic -> scalar decode -> seed -> hit records in a row: both keep the dealing by refill.  So does a volume
  // beyond the 32-bit step offsets (`small` below; 2048^3): its launch runs at the line rate too, and whole units were measured at
  // 512^3 only.
  // A unit is asked for when a wave needs one.  Reserving the next unit a pass ahead (CLWH_TUNE_UNIT_AHEAD=1) was measured slower on
  // the headline, 2.682 -> 2.704 ms: it stays a knob, off, that nothing but the tests and that A/B turns on.
  a.unit_ahead = a.unit_ahead > 0 ? 1 : 0;
  const bool g = a.tf.uses_gradient != 0;
  // fewer than 2^23 bricks (up to ~1600^3): every step byte has a 32-bit offset -> the march's 32-bit addressing, with
  // the index terms of the three axes in LDS tables
  const bool small = (uint64_t)a.NBX * (uint64_t)a.NBY * (uint64_t)((a.Z + 7) / 8) < (1ull << 23) &&
                     a.X + a.Y + a.Z <= VolumePacked::kPartsMaxEntries;
  const bool units = long_launch && !g && small;
  const size_t lds_parts_bytes = small ? (size_t)(a.X + a.Y + a.Z) * sizeof(uint32_t) : 0u;
  // CLWH_TUNE_BOUNCE_RAYS=2: long launches run k_bounce2 (two rays per lane; hit index and seed index share a dword: 2^26 hits)
  const bool two_rays = a.bounce_rays == 2 && long_launch && a.n_hits < (1u << 26) && kBounceThreads == 256;
  if (two_rays) a.fixup_capacity = std::min<uint32_t>(a.fixup_capacity, (1u << 27) - 4u);
#define CLVR_LAUNCH_BOUNCE(G, M)                                                                    \
  do {                                                                                              \
    if (two_rays) {                                                                                 \
      if (small) hipLaunchKernelGGL((k_bounce2<G, M, true>), grid, block, lds_parts_bytes, s, a);  \
      else hipLaunchKernelGGL((k_bounce2<G, M, false>), grid, block, 0, s, a);                     \
    } else if (units) {                                                                             \
      hipLaunchKernelGGL((k_bounce<false, M, true, true>), grid, block, lds_parts_bytes, s, a);    \
    } else if (small) hipLaunchKernelGGL((k_bounce<G, M, true, false>), grid, block, lds_parts_bytes, s, a); \
    else hipLaunchKernelGGL((k_bounce<G, M, false, false>), grid, block, 0, s, a);                 \
  } while (0)
  if (a.mode == CLWH_ACCUM_VOXEL_CACHE) {
    if (g) CLVR_LAUNCH_BOUNCE(true, CLWH_ACCUM_VOXEL_CACHE);
    else CLVR_LAUNCH_BOUNCE(false, CLWH_ACCUM_VOXEL_CACHE);
  } else {
    if (g) CLVR_LAUNCH_BOUNCE(true, CLWH_ACCUM_IMAGE_SPACE);
    else CLVR_LAUNCH_BOUNCE(false, CLWH_ACCUM_IMAGE_SPACE);
  }
#undef CLVR_LAUNCH_BOUNCE
  return hipGetLastError();
}

}  // namespace clvr
