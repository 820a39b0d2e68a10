// tile_work_kernels.hip -- the list kernel of the tile worklist (tile_work_device.hpp has the protocol), gfx950.
#include "tile_work_device.hpp"

namespace clvr {

// the tiles stamped for `round` into the list of counter slot `slot`; dense: one stamped tile lists them all (the round kernel then takes
// the ticket itself for the tile).  A round behind an empty one has nothing to list.
__global__ __launch_bounds__(256) void k_tile_list(const TileWork w, uint32_t round, int slot) {
  if (slot > 0 && w.counters[2 * (slot - 1)] == 0u) return;
  const uint32_t n_tiles = (uint32_t)(w.TX * w.TY * w.TZ), i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_tiles || w.stamps[i] != round) return;
  if (w.dense) w.counters[2 * slot] = n_tiles;  // (the same value from every writer)
  else w.list[atomicAdd(&w.counters[2 * slot], 1u)] = i;
}

void enqueue_tile_list(const TileWork &w, uint32_t round, int slot, hipStream_t s) {
  hipLaunchKernelGGL(k_tile_list, dim3(blocks_for((size_t)w.TX * (size_t)w.TY * (size_t)w.TZ)), dim3(256), 0, s, w, round, slot);
}

}  // namespace clvr
