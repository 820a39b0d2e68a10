// mesh_kernels.hip -- the isosurface of the volume's grid as an indexed triangle mesh by marching tetrahedra (clwh_mesh_isosurface).
// Every decision is an integer comparison on the grid values A(P) = V(P) << 24 against T = floor(iso * 2^24), every vertex is a function
// of its edge (P, dir) alone and taken from the edge's lower end, so the result can be tested bit for bit (include/clwh.h).  The bricked
// int16 copy of the volume and the dilated {min, max} table are the views' (k_proj_repack, k_iso_dilate).
//
// One 512-thread block per 8^3 brick, thread = grid point of the brick, x fastest.  Every kernel stages the 9^3 grid values the brick's
// points and cells need in LDS and classifies its point the same way (mesh_classify), so the three agree on every count:
//
//   k_mesh_count     per brick {vertices, triangles, "has a vertex"}.  Without CLWH_MESH_DENSE a brick whose dilated pair has no value
//                    on one side of T returns zeros unread; a brick outside the box always does.
//   (the three columns are scanned by rocprim::exclusive_scan; the totals go to the host, the one wait)
//   k_mesh_vertices  a brick with vertices writes them at base + rank (rank: block-local scan, grid point x fastest, then dir
//                    ascending) and leaves per grid point "edge mask | rank << 8" in the brick's slot of the point table.
//   k_mesh_triangles a brick with triangles writes them at base + rank (cell x fastest, tetrahedron, triangle).  The index of the
//                    vertex on edge (P', dir') is base[brick(P')] + rank[P'] + popcount(mask[P'] below dir'), read from the point table:
//                    no search, no atomics, so no order depends on which wave runs first.
//
// The point table has one slot of 512 words per brick WITH a vertex, not per brick: the count pass needs no table, so the scan can hand
// out the slots.  That is why vertices and triangles are two launches (a cell's triangle may name a vertex of the next brick, which
// must have been ranked before): the 9^3 stage is repeated, the table stays small, and the dense walk gives the same bytes in the
// same order because an unvisited brick and a visited one without a crossing both count zero.
#include <rocprim/device/device_scan.hpp>

#include "view_device.hpp"

namespace clvr {

// the six tetrahedra of the Kuhn triangulation: corners 0, a, a|b, 7 for the permutations (a, b, c) of {1, 2, 4}, (a, b) ascending
// (three bits per tetrahedron, so that no lookup indexes registers)
__device__ __forceinline__ uint32_t mesh_tet_a(int tet) { return ((1u | 1u << 3 | 2u << 6 | 2u << 9 | 4u << 12 | 4u << 15) >> (3 * tet)) & 7u; }
__device__ __forceinline__ uint32_t mesh_tet_ab(int tet) { return ((3u | 5u << 3 | 3u << 6 | 6u << 9 | 5u << 12 | 6u << 15) >> (3 * tet)) & 7u; }
// triangles of a tetrahedron by its 4-bit case (bit p: corner at position p inside).  Bits 0-1: the number of triangles; triangle k at
// bits 2 + 12 k, its vertex j at 4 bits from there: lo | hi << 2, the edge between the corners at positions lo < hi.  The winding is
// the contract's (counter-clockwise seen from outside, decided on the edge midpoints); it depends on the parity of the permutation
// only, so there are two rows: [0] for tetrahedra 0, 3, 4 and [1] for 1, 2, 5.
__device__ const uint32_t k_mesh_cases[2][16] = {
    {0x0000000u, 0x0003211u, 0x0002751u, 0x2763722u, 0x0003a61u, 0x3a53392u, 0x2393b52u, 0x0003b71u, 0x00037b1u, 0x3793a12u, 0x3b12792u,
     0x00027a1u, 0x3363662u, 0x0003651u, 0x0002311u, 0x0000000u},
    {0x0000000u, 0x0002311u, 0x0003651u, 0x3663362u, 0x00027a1u, 0x2793b12u, 0x3a13792u, 0x00037b1u, 0x0003b71u, 0x3b52392u, 0x3393a52u,
     0x0003a61u, 0x3722762u, 0x0002751u, 0x0003211u, 0x0000000u}};
__device__ __forceinline__ uint32_t mesh_case_word(int tet, uint32_t c4) { return k_mesh_cases[(0x26 >> tet) & 1][c4]; }

__device__ __forceinline__ bool mesh_inside(const MeshArgs &a, int v) { return a.below ? v <= a.in_bound : v >= a.in_bound; }

// can the brick own a crossing edge or a cell with a triangle?  (uniform over the block)
__device__ __forceinline__ bool mesh_brick_active(const MeshArgs &a, size_t brick, int bx, int by, int bz) {
  // its grid points [8 b, 8 b + 7] meet the box [lo, hi] on every axis
  if (bx * 8 > a.hi[0] || bx * 8 + 7 < a.lo[0] || by * 8 > a.hi[1] || by * 8 + 7 < a.lo[1] || bz * 8 > a.hi[2] || bz * 8 + 7 < a.lo[2]) return false;
  if (a.skip) {  // a crossing needs a value inside and a value outside within one voxel of the brick
    const uint32_t mm = a.vol.dilated[brick];
    const int dmin = table_min(mm), dmax = table_max(mm);
    return a.below ? (dmin <= a.in_bound && dmax > a.in_bound) : (dmin < a.in_bound && dmax >= a.in_bound);
  }
  return true;
}

// the 9^3 grid values at and one past the brick's points, [z][y][x]; rows of 9 words put a wave's 8 x 8 points on addresses i + 9 j,
// all different modulo 32 but for the last row (2-way there)
__device__ __forceinline__ void mesh_stage(const MeshArgs &a, int bx, int by, int bz, int *s_val) {
  for (unsigned i = threadIdx.x; i < 729u; i += 512u) {
    const int x = bx * 8 + (int)(i % 9u), y = by * 8 + (int)((i / 9u) % 9u), z = bz * 8 + (int)(i / 81u);
    int v = 0;  // past the volume: never an end of an edge of the box (hi <= dim - 1)
    if (x < a.vol.X && y < a.vol.Y && z < a.vol.Z) v = a.vol.bricks[VolumePacked::record_index(x, y, z, a.vol.NBX, a.vol.NBY)];
    s_val[i] = v;
  }
  __syncthreads();
}

struct MeshPoint {
  int x, y, z;
  uint32_t in8;    // bit m: the corner P + m is inside (meaningful where the corner is in the box)
  uint32_t edges;  // bit dir - 1: the edge (P, dir) has a vertex
  bool cell;       // P is the origin of a meshed cell
};

__device__ __forceinline__ MeshPoint mesh_classify(const MeshArgs &a, int bx, int by, int bz, const int *s_val) {
  const int i = (int)(threadIdx.x & 7u), j = (int)((threadIdx.x >> 3) & 7u), k = (int)(threadIdx.x >> 6);
  MeshPoint p;
  p.x = bx * 8 + i;
  p.y = by * 8 + j;
  p.z = bz * 8 + k;
  const bool p_ok = p.x >= a.lo[0] && p.x <= a.hi[0] && p.y >= a.lo[1] && p.y <= a.hi[1] && p.z >= a.lo[2] && p.z <= a.hi[2];
  const uint32_t ax = (p.x < a.hi[0] ? 1u : 0u) | (p.y < a.hi[1] ? 2u : 0u) | (p.z < a.hi[2] ? 4u : 0u);  // axes with P + e in the box
  p.in8 = 0u;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int v = s_val[((k + (m >> 2)) * 9 + (j + ((m >> 1) & 1))) * 9 + (i + (m & 1))];
    p.in8 |= (mesh_inside(a, v) ? 1u : 0u) << m;
  }
  p.edges = 0u;
  p.cell = p_ok && ax == 7u;
  if (p_ok) {
    const uint32_t differs = (p.in8 & 1u) ? ~p.in8 : p.in8;  // bit m: corner m on the other side than P
#pragma unroll
    for (uint32_t dir = 1; dir < 8; ++dir)
      if ((dir & ~ax) == 0u && ((differs >> dir) & 1u)) p.edges |= 1u << (dir - 1u);
  }
  return p;
}

__device__ __forceinline__ uint32_t mesh_tet_case(uint32_t in8, int tet) {
  return (in8 & 1u) | (((in8 >> mesh_tet_a(tet)) & 1u) << 1) | (((in8 >> mesh_tet_ab(tet)) & 1u) << 2) | (((in8 >> 7) & 1u) << 3);
}
__device__ __forceinline__ uint32_t mesh_cell_triangles(const MeshPoint &p) {
  if (!p.cell) return 0u;
  uint32_t n = 0u;
#pragma unroll
  for (int t = 0; t < 6; ++t) {  // 1 or 3 corners inside: one triangle; 2: two (the table's bits 0-1, without the load)
    const uint32_t inside = (uint32_t)__popc(mesh_tet_case(p.in8, t));
    n += inside == 2u ? 2u : (inside & 1u);
  }
  return n;
}

// exclusive prefix of v over the block's 512 threads in thread order, and the block's total
__device__ __forceinline__ uint32_t mesh_block_scan(uint32_t v, uint32_t *s_wave, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)inc, off);
    if (lane >= (uint32_t)off) inc += o;
  }
  if (lane == 63u) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = 0u;
  total = 0u;
#pragma unroll
  for (uint32_t w = 0; w < 8u; ++w) {
    const uint32_t s = s_wave[w];
    before += w < wave ? s : 0u;
    total += s;
  }
  return before + inc - v;
}

__device__ __forceinline__ void mesh_brick_coords(const MeshArgs &a, size_t brick, int &bx, int &by, int &bz) {
  bx = (int)(brick % (size_t)a.vol.NBX);
  by = (int)((brick / (size_t)a.vol.NBX) % (size_t)a.vol.NBY);
  bz = (int)(brick / ((size_t)a.vol.NBX * (size_t)a.vol.NBY));
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_mesh_count(const MeshArgs a) {
  __shared__ int s_val[729];
  __shared__ uint32_t s_wave[8];
  const size_t brick = blockIdx.x, n1 = a.n_bricks + 1u;
  int bx, by, bz;
  mesh_brick_coords(a, brick, bx, by, bz);
  uint32_t total = 0u;
  if (mesh_brick_active(a, brick, bx, by, bz)) {
    mesh_stage(a, bx, by, bz, s_val);
    const MeshPoint p = mesh_classify(a, bx, by, bz, s_val);
    // vertices <= 3584 and triangles <= 6144 per brick: one scan of 16 + 16 bits carries both
    (void)mesh_block_scan((uint32_t)__popc(p.edges) | (mesh_cell_triangles(p) << 16), s_wave, total);
  }
  if (threadIdx.x == 0u) {
    a.counts[brick] = total & 0xFFFFu;
    a.counts[n1 + brick] = total >> 16;
    a.counts[2u * n1 + brick] = (total & 0xFFFFu) ? 1u : 0u;
    if (brick == 0u) a.counts[a.n_bricks] = a.counts[n1 + a.n_bricks] = a.counts[2u * n1 + a.n_bricks] = 0u;  // the scans' last element: the totals
  }
}

__global__ __launch_bounds__(512) void k_mesh_vertices(const MeshArgs a) {
  __shared__ int s_val[729];
  __shared__ uint32_t s_wave[8];
  const size_t brick = blockIdx.x, n1 = a.n_bricks + 1u;
  const uint64_t base = a.bases[brick];
  if (a.bases[brick + 1u] == base) return;  // no vertex (uniform)
  int bx, by, bz;
  mesh_brick_coords(a, brick, bx, by, bz);
  mesh_stage(a, bx, by, bz, s_val);
  const MeshPoint p = mesh_classify(a, bx, by, bz, s_val);
  uint32_t total;
  const uint32_t rank = mesh_block_scan((uint32_t)__popc(p.edges), s_wave, total);
  a.points[(size_t)a.bases[2u * n1 + brick] * 512u + threadIdx.x] = p.edges | (rank << 8);
  if (!a.positions) return;

  const int i = (int)(threadIdx.x & 7u), j = (int)((threadIdx.x >> 3) & 7u), k = (int)(threadIdx.x >> 6);
  const long long AP = (long long)s_val[(k * 9 + j) * 9 + i] << 24;
  uint64_t o = base + rank;
  for (uint32_t rest = p.edges; rest != 0u; rest &= rest - 1u, ++o) {
    const int dir = __ffs((int)rest);  // bit dir - 1
    const int dx = dir & 1, dy = (dir >> 1) & 1, dz = dir >> 2;
    const long long AQ = (long long)s_val[((k + dz) * 9 + (j + dy)) * 9 + (i + dx)] << 24;
    const long long num = a.threshold > AP ? a.threshold - AP : AP - a.threshold, den = AQ > AP ? AQ - AP : AP - AQ;  // num <= den, den > 0
    const long long w = (num << 16) / den;
    const long long Fx = (long long)p.x * 65536 + 32768 + dx * w, Fy = (long long)p.y * 65536 + 32768 + dy * w, Fz = (long long)p.z * 65536 + 32768 + dz * w;
    // F < 2^48 is exact in binary64: one rounding; the scaling by 2^-16 is exact
    a.positions[3u * o + 0u] = (float)(double)Fx * 1.52587890625e-05f;
    a.positions[3u * o + 1u] = (float)(double)Fy * 1.52587890625e-05f;
    a.positions[3u * o + 2u] = (float)(double)Fz * 1.52587890625e-05f;
    if (a.keys) a.keys[o] = (((uint64_t)p.z * (uint64_t)a.vol.Y + (uint64_t)p.y) * (uint64_t)a.vol.X + (uint64_t)p.x) * 8u + (uint64_t)dir;
    if (a.normals) {
      int px, py, pz, qx, qy, qz;
      central_difference(a.vol, p.x, p.y, p.z, px, py, pz);  // g_c(R): the isosurface's
      central_difference(a.vol, p.x + dx, p.y + dy, p.z + dz, qx, qy, qz);
      const long long Gx = (65536 - w) * px + w * qx, Gy = (65536 - w) * py + w * qy, Gz = (65536 - w) * pz + w * qz;
      const float gx = (float)(double)Gx, gy = (float)(double)Gy, gz = (float)(double)Gz;
      const float l2 = length2(gx, gy, gz);
      float nx = 0.0f, ny = 0.0f, nz = 0.0f;
      if (l2 > 0.0f) {
        const float len = sqrtf(l2);
        nx = (a.below ? gx : -gx) / len;
        ny = (a.below ? gy : -gy) / len;
        nz = (a.below ? gz : -gz) / len;
      }
      a.normals[3u * o + 0u] = nx;
      a.normals[3u * o + 1u] = ny;
      a.normals[3u * o + 2u] = nz;
    }
  }
}

__global__ __launch_bounds__(512) void k_mesh_triangles(const MeshArgs a) {
  __shared__ int s_val[729];
  __shared__ uint32_t s_wave[8];
  const size_t brick = blockIdx.x, n1 = a.n_bricks + 1u;
  const uint64_t base = a.bases[n1 + brick];
  if (a.bases[n1 + brick + 1u] == base) return;  // no triangle (uniform)
  int bx, by, bz;
  mesh_brick_coords(a, brick, bx, by, bz);
  mesh_stage(a, bx, by, bz, s_val);
  const MeshPoint p = mesh_classify(a, bx, by, bz, s_val);
  uint32_t total;
  uint64_t o = base + mesh_block_scan(mesh_cell_triangles(p), s_wave, total);
  if (!p.cell) return;
  for (int t = 0; t < 6; ++t) {
    const uint32_t corners = mesh_tet_a(t) << 3 | mesh_tet_ab(t) << 6 | 7u << 9;  // the corner at position q: bits 3 q
    uint32_t word = mesh_case_word(t, mesh_tet_case(p.in8, t));
    const uint32_t n = word & 3u;
    word >>= 2;
    for (uint32_t tri = 0; tri < n; ++tri, ++o) {
      for (uint32_t v = 0; v < 3u; ++v, word >>= 4) {
        const uint32_t lo = (corners >> (3u * (word & 3u))) & 7u, dir = ((corners >> (3u * ((word >> 2) & 3u))) & 7u) ^ lo;  // the edge's lower end P' = P + lo owns it
        const int x = p.x + (int)(lo & 1u), y = p.y + (int)((lo >> 1) & 1u), z = p.z + (int)(lo >> 2);
        const size_t owner = brick_index(a.vol, x >> 3, y >> 3, z >> 3);
        const uint32_t rec = a.points[(size_t)a.bases[2u * n1 + owner] * 512u + (size_t)(((z & 7) * 8 + (y & 7)) * 8 + (x & 7))];
        a.triangles[3u * o + v] = (uint32_t)(a.bases[owner] + (uint64_t)(rec >> 8) + (uint64_t)__popc(rec & ((1u << (dir - 1u)) - 1u)));
      }
    }
  }
}

hipError_t launch_mesh_count(const MeshArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_mesh_count, dim3((unsigned)a.n_bricks), dim3(512), 0, s, a);
  return hipGetLastError();
}

// temp == nullptr: only temp_bytes is set
hipError_t launch_mesh_scan(void *temp, size_t &temp_bytes, const uint64_t *counts, uint64_t *bases, size_t n, hipStream_t s) {
  return rocprim::exclusive_scan(temp, temp_bytes, counts, bases, (uint64_t)0, n, rocprim::plus<uint64_t>(), s);
}

hipError_t launch_mesh_fill(const MeshArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_mesh_vertices, dim3((unsigned)a.n_bricks), dim3(512), 0, s, a);
  if (a.triangles) hipLaunchKernelGGL(k_mesh_triangles, dim3((unsigned)a.n_bricks), dim3(512), 0, s, a);
  return hipGetLastError();
}

}  // namespace clvr
