// tile_work_device.hpp -- the tile worklist that the searches in rounds share on the device (grow_kernels.hip, geodesic_kernels.hip).
//   The protocol.  The volume is cut into tiles, tile (tx, ty, tz) at (tz * TY + ty) * TX + tx, and a block of 256 threads owns the
//   tile it works on.  A tile's stamp is the number of the round (1, 2, ...) in which it is to be visited, so stamps are cleared once
//   per call and never between rounds.  Whoever puts something into a tile before the rounds stamps it 1.  A round is k_tile_list, which
//   appends every tile stamped for this round to the list (so a tile is listed once per round, however many neighbours stamped it, and
//   only its owner stores to it during the round), and the caller's round kernel: a persistent grid whose blocks take the listed tiles
//   by ticket (tile_take), work each to its local fixpoint, and stamp for round + 1 the neighbouring tiles that can see what changed
//   (tile_wake); those are read again behind the kernel boundary.  Round 1 counts everything a tile holds as changed: it was stored by
//   other kernels, and nobody has looked at it from the other side of a tile face yet.  When a round lists no tile every tile is at
//   its local fixpoint with the halo it would read now.  Why the halo may be read while its owner stores to it is the round kernel's
//   own proof, at the head of its file.
//   counters[2 * slot] is the number of tiles listed for the round in batch slot `slot`, counters[2 * slot + 1] its ticket.
#pragma once

#include "mask_device.hpp"

namespace clvr {

namespace {

struct TileShared {  // a round kernel's __shared__ state of the worklist
  uint32_t ticket, wake;
};

// The block's next tile of the round's n listed ones, false when they are all taken.  Two barriers: every thread calls it.
__device__ __forceinline__ bool tile_take(const TileWork &w, uint32_t n, int slot, TileShared &sh, int &tx, int &ty, int &tz) {
  __syncthreads();  // the previous tile's last reads of sh and of the kernel's own shared arrays
  if (threadIdx.x == 0u) {
    sh.ticket = atomicAdd(&w.counters[2 * slot + 1], 1u);
    sh.wake = 0u;
  }
  __syncthreads();
  const uint32_t ticket = sh.ticket;
  if (ticket >= n) return false;
  const uint32_t tile = w.dense ? ticket : w.list[ticket];  // dense: the ticket is the tile
  tx = (int)(tile % (uint32_t)w.TX);
  ty = (int)((tile / (uint32_t)w.TX) % (uint32_t)w.TY);
  tz = (int)(tile / (uint32_t)(w.TX * w.TY));
  return true;
}

// The neighbouring tiles that what this block changed can be seen from are visited in the next round.  A thread with `fresh` says
// where its change lies: at_x[0] / at_x[2] whether it touches the tile's low / high face along x (at_x[1] is true), the same for y
// and z.  One barrier: every thread calls it.
template <bool CONN26>
__device__ __forceinline__ void tile_wake(const TileWork &w, uint32_t round, TileShared &sh, int tx, int ty, int tz, bool fresh,
                                          const bool (&at_x)[3], const bool (&at_y)[3], const bool (&at_z)[3]) {
  if (fresh) {
    uint32_t wake = 0u;
#pragma unroll
    for (int q = 0; q < 27; ++q) {
      const int dx = q % 3, dy = (q / 3) % 3, dz = q / 9;
      const int moved = (dx != 1) + (dy != 1) + (dz != 1);
      if (moved == 0 || (!CONN26 && moved != 1)) continue;  // an edge or corner neighbour is adjacent only under 26-connectivity
      if (at_x[dx] && at_y[dy] && at_z[dz]) wake |= 1u << q;
    }
    if (wake) atomicOr(&sh.wake, wake);
  }
  __syncthreads();
  const unsigned t = threadIdx.x;
  if (t < 27u && ((sh.wake >> t) & 1u)) {
    const int nx = tx + (int)(t % 3u) - 1, ny = ty + (int)((t / 3u) % 3u) - 1, nz = tz + (int)(t / 9u) - 1;
    if (nx >= 0 && nx < w.TX && ny >= 0 && ny < w.TY && nz >= 0 && nz < w.TZ) w.stamps[((size_t)nz * w.TY + ny) * w.TX + nx] = round + 1u;
  }
}

// One round: the list, then the caller's round kernel on a persistent grid of at most grid_cap blocks (fewer tiles need fewer blocks)
template <class Args>
inline hipError_t launch_tile_round(void (*k_round)(Args, uint32_t, int), unsigned grid_cap, const Args &a, uint32_t round, int slot,
                                    hipStream_t s) {
  enqueue_tile_list(a.tiles, round, slot, s);
  const size_t n_tiles = (size_t)a.tiles.TX * (size_t)a.tiles.TY * (size_t)a.tiles.TZ;
  hipLaunchKernelGGL(k_round, dim3((unsigned)(n_tiles < grid_cap ? n_tiles : grid_cap)), dim3(256), 0, s, a, round, slot);
  return hipGetLastError();
}

}  // namespace

}  // namespace clvr
