// Nearest point on a triangle mesh within a radius over a uniform cell grid (not
// in the reference): ucsa_triangle_cell_counts, ucsa_triangle_cell_pairs and
// ucsa_nearest_triangle.  The contract is stated in include/ucsa_hip.h;
// tests/surface_numpy.py restates it as plain brute force (nearest_triangle) and
// models this file's traversal (nearest_triangle_grid, the same float32
// expressions), and the outputs match the brute force byte for byte: the result
// does not depend on the cell size, the origin or the order of the queries.
//
// k_tri_counts     a lane per face: per axis the cells [pg_cell(min corner),
//                  pg_cell(max corner)]; the count is the product of the three
//                  range lengths, 0 for a face with a corner index outside
//                  [0, nv) or a non-finite corner.
// k_tri_pairs      a lane per face: the (linear cell, face) pairs of that box in
//                  x, y, z order at first[f] ...: fixed positions, no atomics.
// k_nearest_tri    a lane per query: the ring walk of cell_grid.h (pg_walk) over
//                  records of three float4 per (cell, face) pair, sorted by cell
//                  with faces ascending inside a cell: a cell's candidates are
//                  contiguous 16-byte loads and no index is chased.  A face
//                  registered in several cells is evaluated more than once; the
//                  result is a minimum over a set and does not change.
//
// The closest point of a face (tg_closest) and the state of a query's walk
// (FaceWalk) live in tri_closest.h, which mesh_sdf.hip shares.
//
// Why the cut is safe (docs/DESIGN_NOTEBOOK.md, section NT): a face none of
// whose cells was visited has all three corners beyond one cut wall (monotone
// cell assignment, as for points); its closest point is a combination of the
// corners with weights v, w in [0, 1], w <= fl(1 - v), so it lies beyond the
// wall too, up to thirteen and a half roundings of coordinates no larger than
// |o| + |top| + |q| on that axis.  The gap is shortened by S = 2^-19 of that sum
// (32 roundings) and its square compared with B * (1 + 2^-20).
// k_tri_pairs' loops are bounded by the grid's dims and by n_pairs; no atomics,
// no LDS, no waiting on another thread.
#include "tri_closest.h"

namespace {

// the face's box of cells on one axis (finite corners)
__device__ __forceinline__ void tg_range(float a, float b, float c, float o, float cell,
                                         uint32_t dim, uint32_t& c0, uint32_t& c1) {
  const float mn = fminf(fminf(a, b), c), mx = fmaxf(fmaxf(a, b), c);
  c0 = pg_cell((mn - o) / cell, dim);
  c1 = pg_cell((mx - o) / cell, dim);
}

__global__ void __launch_bounds__(PG_THREADS) k_tri_counts(const float* __restrict__ verts,
                                                           uint32_t nv,
                                                           const int32_t* __restrict__ faces,
                                                           uint32_t nf, GridArgs g,
                                                           int32_t* __restrict__ counts) {
  const uint32_t f = blockIdx.x * PG_THREADS + threadIdx.x;
  if (f >= nf) return;
  const Corners c = tg_corners(verts, nv, faces, f);
  uint32_t n = 0;
  if (c.ok) {
    uint32_t x0, x1, y0, y1, z0, z1;
    tg_range(c.ax, c.bx, c.cx, g.o[0], g.cell, g.d[0], x0, x1);
    tg_range(c.ay, c.by, c.cy, g.o[1], g.cell, g.d[1], y0, y1);
    tg_range(c.az, c.bz, c.cz, g.o[2], g.cell, g.d[2], z0, z1);
    n = (x1 - x0 + 1u) * (y1 - y0 + 1u) * (z1 - z0 + 1u);  // <= cells <= 2^24
  }
  counts[f] = (int32_t)n;
}

__global__ void __launch_bounds__(PG_THREADS) k_tri_pairs(const float* __restrict__ verts,
                                                          uint32_t nv,
                                                          const int32_t* __restrict__ faces,
                                                          uint32_t nf, GridArgs g,
                                                          const int32_t* __restrict__ first,
                                                          uint32_t n_pairs,
                                                          int32_t* __restrict__ keys,
                                                          int32_t* __restrict__ pair_face) {
  const uint32_t f = blockIdx.x * PG_THREADS + threadIdx.x;
  if (f >= nf) return;
  const Corners c = tg_corners(verts, nv, faces, f);
  if (!c.ok) return;
  const int32_t at = first[f];
  if (at < 0) return;
  uint32_t x0, x1, y0, y1, z0, z1;
  tg_range(c.ax, c.bx, c.cx, g.o[0], g.cell, g.d[0], x0, x1);
  tg_range(c.ay, c.by, c.cy, g.o[1], g.cell, g.d[1], y0, y1);
  tg_range(c.az, c.bz, c.cz, g.o[2], g.cell, g.d[2], z0, z1);
  uint32_t k = (uint32_t)at;  // at most 2^24 steps from at < 2^31: no wrap
  for (uint32_t x = x0; x <= x1; ++x)
    for (uint32_t y = y0; y <= y1; ++y)
      for (uint32_t z = z0; z <= z1; ++z, ++k) {
        if (k >= n_pairs) return;  // a `first` that is not the scan of the counts
        keys[k] = (int32_t)((x * g.d[1] + y) * g.d[2] + z);
        pair_face[k] = (int32_t)f;
      }
}

__global__ void __launch_bounds__(PG_THREADS) k_tri_no_match(uint32_t nq,
                                                             int32_t* __restrict__ face,
                                                             float* __restrict__ dist2,
                                                             float* __restrict__ bary) {
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;
  if (i >= nq) return;
  face[i] = -1;
  dist2[i] = INFINITY;
  bary[3ull * i] = 0.0f;
  bary[3ull * i + 1u] = 0.0f;
  bary[3ull * i + 2u] = 0.0f;
}

__global__ void __launch_bounds__(PG_THREADS) k_nearest_tri(const float4* __restrict__ rec,
                                                            const int32_t* __restrict__ offsets,
                                                            uint32_t n, GridArgs g,
                                                            const float* __restrict__ queries,
                                                            const int32_t* __restrict__ q_order,
                                                            uint32_t nq, float limit2,
                                                            int32_t* __restrict__ face,
                                                            float* __restrict__ dist2,
                                                            float* __restrict__ bary) {
  const uint32_t t = blockIdx.x * PG_THREADS + threadIdx.x;
  if (t >= nq) return;
  const uint32_t qi = q_order ? (uint32_t)q_order[t] : t;
  if (qi >= nq) return;  // a malformed order writes nothing outside the outputs
  FaceWalk w;
  w.rec = rec;
  w.qx = queries[3ull * qi];
  w.qy = queries[3ull * qi + 1u];
  w.qz = queries[3ull * qi + 2u];
  w.best = limit2;
  w.bidx = PG_NONE;
  w.v = 0.0f;
  w.w = 0.0f;
  pg_walk(offsets, n, g, TG_KS, limit2, w);
  const bool hit = w.bidx != PG_NONE;
  face[qi] = hit ? (int32_t)w.bidx : -1;
  dist2[qi] = hit ? w.best : INFINITY;
  bary[3ull * qi] = hit ? (1.0f - w.v) - w.w : 0.0f;
  bary[3ull * qi + 1u] = hit ? w.v : 0.0f;
  bary[3ull * qi + 2u] = hit ? w.w : 0.0f;
}

// the arguments the two build kernels share: -> 0 or the offending argument's index + 1
int tg_mesh_args(uint32_t nv, uint32_t nf, const float* origin, float cell, const uint32_t* dims,
                 GridArgs& g) {
  if (nv > 0x7FFFFFFFu) return 2;
  if (nf > 0x7FFFFFFFu) return 4;
  const int bad = pg_grid_args(origin, cell, dims, g);
  return bad ? 4 + bad : 0;  // origin 4, cell 5, dims 6
}

}  // namespace

extern "C" int32_t ucsa_triangle_cell_counts(const float* verts, uint32_t nv, const int32_t* faces,
                                             uint32_t nf, const float* origin, float cell,
                                             const uint32_t* dims, int32_t* counts, void* stream) {
  GridArgs g;
  const int bad = tg_mesh_args(nv, nf, origin, cell, dims, g);
  UCSA_CHECK_ARG(bad == 0, bad - 1);
  if (nf == 0) return 0;
  UCSA_CHECK_ARG(nv == 0 || verts, 0);
  UCSA_CHECK_ARG(faces, 2);
  UCSA_CHECK_ARG(counts, 7);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_tri_counts, dim3(ucsa_div_up(nf, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, verts, nv, faces, nf, g, counts);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_triangle_cell_pairs(const float* verts, uint32_t nv, const int32_t* faces,
                                            uint32_t nf, const float* origin, float cell,
                                            const uint32_t* dims, const int32_t* first,
                                            uint32_t n_pairs, int32_t* keys, int32_t* pair_face,
                                            void* stream) {
  GridArgs g;
  const int bad = tg_mesh_args(nv, nf, origin, cell, dims, g);
  UCSA_CHECK_ARG(bad == 0, bad - 1);
  UCSA_CHECK_ARG(n_pairs <= 0x7FFFFFFFu, 8);
  if (nf == 0 || n_pairs == 0) return 0;
  UCSA_CHECK_ARG(nv == 0 || verts, 0);
  UCSA_CHECK_ARG(faces, 2);
  UCSA_CHECK_ARG(first, 7);
  UCSA_CHECK_ARG(keys, 9);
  UCSA_CHECK_ARG(pair_face, 10);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_tri_pairs, dim3(ucsa_div_up(nf, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, verts, nv, faces, nf, g, first, n_pairs, keys, pair_face);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_nearest_triangle(const float* records, const int32_t* offsets,
                                         uint32_t n_pairs, const float* origin, float cell,
                                         const uint32_t* dims, const float* queries,
                                         const int32_t* q_order, uint32_t nq, float max_dist,
                                         int32_t* face, float* dist2, float* bary, void* stream) {
  GridArgs g;
  float limit2;
  const void* outs[] = {face, dist2, bary};
  const int32_t st = pg_search_args(records, offsets, n_pairs, origin, cell, dims, queries, nq,
                                    max_dist, outs, 3, g, limit2);
  if (st != 0 || nq == 0) return st;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ucsa_div_up(nq, PG_THREADS));
  UCSA_CLEAR_ERR();
  if (n_pairs == 0)
    hipLaunchKernelGGL(k_tri_no_match, grid, dim3(PG_THREADS), 0, s, nq, face, dist2, bary);
  else
    hipLaunchKernelGGL(k_nearest_tri, grid, dim3(PG_THREADS), 0, s, (const float4*)records,
                       offsets, n_pairs, g, queries, q_order, nq, limit2, face, dist2, bary);
  return ucsa_launch_status();
}
