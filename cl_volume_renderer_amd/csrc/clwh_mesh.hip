// clwh_mesh.hip -- clwh_mesh_isosurface on the host: the isosurface of the volume's grid as an indexed triangle mesh, over the views'
// bricked copy of the volume and dilated table (clwh_views.hip: ensure_projection_data, ensure_dilated_table).  The kernels are in
// mesh_kernels.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "clwh_host.hpp"

using namespace clvr;

extern "C" int clwh_mesh_isosurface(clwh_ctx *ctx, const clwh_mesh_desc *d) {
  if (!ctx || !d || !d->n_vertices || !d->n_triangles) return CLWH_ERR_INVALID_VALUE;
  if (!is_image(d->volume, 3, 1, CLWH_ELEM_S16)) return CLWH_ERR_INVALID_VALUE;
  if ((d->flags & ~(CLWH_MESH_DENSE | CLWH_MESH_BELOW)) != 0) return CLWH_ERR_INVALID_VALUE;
  if (!(std::isfinite(d->iso) && std::fabs(d->iso) <= 65536.0f)) return CLWH_ERR_INVALID_VALUE;
  const bool whole = (d->box_hi[0] | d->box_hi[1] | d->box_hi[2]) == 0u;
  uint64_t lo[3], hi[3];
  for (int q = 0; q < 3; ++q) {
    if (d->volume->dims[q] == 0) return CLWH_ERR_INVALID_VALUE;
    lo[q] = d->box_lo[q];
    hi[q] = whole ? (uint64_t)d->volume->dims[q] - 1u : (uint64_t)d->box_hi[q];
    if (!(lo[q] <= hi[q] && hi[q] <= (uint64_t)d->volume->dims[q] - 1u)) return CLWH_ERR_INVALID_VALUE;
  }
  const clwh_mem *outs[4] = {d->positions, d->normals, d->keys, d->triangles};
  for (const clwh_mem *m : outs)
    if (m && !is_plain_buffer(m)) return CLWH_ERR_INVALID_VALUE;
  if ((d->positions != nullptr) != (d->triangles != nullptr)) return CLWH_ERR_INVALID_VALUE;
  if ((d->normals || d->keys) && !d->positions) return CLWH_ERR_INVALID_VALUE;  // they accompany the positions
  if ((d->vertex_capacity > 0 && !d->positions) || (d->triangle_capacity > 0 && !d->triangles)) return CLWH_ERR_INVALID_VALUE;
  if (!dims_fit_int32(d->volume)) return CLWH_ERR_INVALID_VALUE;
  // (compared by division: capacity * element size may not fit 64 bits)
  if (d->positions && d->vertex_capacity > d->positions->bytes / 12u) return CLWH_ERR_SIZE_MISMATCH;
  if (d->normals && d->vertex_capacity > d->normals->bytes / 12u) return CLWH_ERR_SIZE_MISMATCH;
  if (d->keys && d->vertex_capacity > d->keys->bytes / 8u) return CLWH_ERR_SIZE_MISMATCH;
  if (d->triangles && d->triangle_capacity > d->triangles->bytes / 12u) return CLWH_ERR_SIZE_MISMATCH;

  *d->n_vertices = *d->n_triangles = 0;
  if (lo[0] == hi[0] || lo[1] == hi[1] || lo[2] == hi[2]) return CLWH_OK;  // no cell: the empty mesh

  MeshArgs a;
  std::memset(&a, 0, sizeof a);
  HIP_TRY(hipSetDevice(ctx->device));
  CLWH_TRY(ensure_projection_data(ctx, d->volume, a.vol));
  a.below = (d->flags & CLWH_MESH_BELOW) != 0;
  a.skip = (d->flags & CLWH_MESH_DENSE) == 0;
  if (a.skip) CLWH_TRY(ensure_dilated_table(ctx, a.vol));
  a.n_bricks = (uint64_t)a.vol.NBX * (uint64_t)a.vol.NBY * (uint64_t)a.vol.NBZ;
  for (int q = 0; q < 3; ++q) {
    a.lo[q] = (int32_t)lo[q];
    a.hi[q] = (int32_t)hi[q];
  }
  // T = floor(iso * 2^24), exact in binary64; V << 24 >= T  <=>  V >= ceil(T / 2^24), V << 24 <= T  <=>  V <= floor(T / 2^24)
  a.threshold = (int64_t)std::floor((double)d->iso * 16777216.0);
  a.in_bound = a.below ? (int32_t)(a.threshold >> 24) : (int32_t)(-((-a.threshold) >> 24));

  // the mesher's scratch, kept beside the copy: per brick {vertices, triangles, has a vertex} and their scans, rocPRIM's work space,
  // and (for a filling call) the point table of the bricks that have a vertex
  ProjectionData &p = ctx->proj;
  const size_t n1 = (size_t)a.n_bricks + 1u;
  CLWH_TRY(p.mesh_counts.reserve(ctx->stream, 6u * n1 * sizeof(uint64_t)));
  a.counts = p.mesh_counts.as<uint64_t>();
  uint64_t *bases = a.counts + 3u * n1;
  a.bases = bases;
  size_t temp_bytes = 0;
  HIP_TRY(launch_mesh_scan(nullptr, temp_bytes, a.counts, bases, n1, ctx->stream));
  CLWH_TRY(p.mesh_temp.reserve(ctx->stream, std::max(temp_bytes, (size_t)16)));
  HIP_TRY(launch_mesh_count(a, ctx->stream));
  for (size_t c = 0; c < 3u; ++c) HIP_TRY(launch_mesh_scan(p.mesh_temp.ptr, temp_bytes, a.counts + c * n1, bases + c * n1, n1, ctx->stream));
  uint64_t totals[3] = {0, 0, 0};  // vertices, triangles, bricks with a vertex
  for (size_t c = 0; c < 3u; ++c)
    HIP_TRY(hipMemcpyAsync(&totals[c], bases + c * n1 + (n1 - 1u), sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // the one wait for the counts
  *d->n_vertices = totals[0];
  *d->n_triangles = totals[1];
  if (totals[0] > 0xFFFFFFFFull || totals[1] > 0xFFFFFFFFull) return CLWH_ERR_SIZE_MISMATCH;  // indices are 32-bit
  if (!d->positions) return CLWH_OK;  // a counting call
  if (totals[0] > d->vertex_capacity || totals[1] > d->triangle_capacity) return CLWH_ERR_SIZE_MISMATCH;
  if (totals[0] == 0) return CLWH_OK;  // (no vertex: no triangle)
  CLWH_TRY(p.mesh_points.reserve(ctx->stream, ((size_t)totals[2] + 1u) * 512u * sizeof(uint32_t)));  // (one spare slot: see k_mesh_triangles)
  a.points = p.mesh_points.as<uint32_t>();
  a.positions = (float *)d->positions->dptr;
  a.normals = d->normals ? (float *)d->normals->dptr : nullptr;
  a.keys = d->keys ? (uint64_t *)d->keys->dptr : nullptr;
  a.triangles = (uint32_t *)d->triangles->dptr;
  HIP_TRY(launch_mesh_fill(a, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous by contract: the buffers are written when the call returns
  return CLWH_OK;
}
