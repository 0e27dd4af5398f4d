// Nearest point within a radius over a uniform cell grid (not in the
// reference): ucsa_point_cell_keys and ucsa_nearest_point.  The contract is
// stated in include/ucsa_hip.h; tests/nearest_numpy.py restates it as plain
// brute force (nearest_point) and models this file's traversal
// (nearest_point_grid, the same float32 expressions), and the outputs match the
// brute force byte for byte: the result does not depend on the cell size, the
// origin or the order of the queries.
//
// k_cell_keys      a lane per point: t = (p - origin) / cell, clamped as a float
//                  into [0, dim - 1] before it becomes an integer; the key is
//                  the linear cell index (x * ny + y) * nz + z, or the number of
//                  cells for a non-finite point (and, without clamping, for a
//                  point outside the grid): that key sorts last and no walk
//                  reaches it.
// k_nearest        a lane per query: the ring walk of cell_grid.h (pg_walk) over
//                  the sorted points, one float4 each (x, y, z and the bits of
//                  the original index).  A candidate's d2 = (dx*dx + dy*dy) +
//                  dz*dz with dx = q.x - p.x ... replaces the best one if it is
//                  smaller, or equal with a smaller index.
//
// Why the cut is safe (docs/DESIGN_NOTEBOOK.md, section NN, has the derivation):
//   * cell assignment: floor(clamp(fl(fl(p - o) / cell))) is monotone in p.  A
//     point in a cell of index >= m (m >= 1) has fl(fl(p - o) / cell) >= m, so
//     p - o >= m * cell * (1 - 2u) (u = 2^-24), whatever side of the nominal wall
//     rounding put it; likewise below a wall.  The query's own cell plays no
//     part in the bound, only its position.
//   * the wall o + m * cell, the gap to it and d2 are each computed with a
//     relative error of a few u in terms of |o|, |o + dims * cell| and |q|.  The
//     gap is shortened by S = K * (|o| + |top| + |q|) and its square compared
//     with B * (1 + K), K = 2^-20 = 16u: an unvisited point's float32 d2 is then
//     strictly above B, so neither a closer point nor a tie with a smaller index
//     is lost.
// No atomics, no LDS, no waiting on another thread.
#include "cell_grid.h"

namespace {

__global__ void __launch_bounds__(PG_THREADS) k_cell_keys(const float* __restrict__ pts, uint32_t n,
                                                          GridArgs g, uint32_t clamp,
                                                          int32_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;
  if (i >= n) return;
  const float x = pts[3ull * i], y = pts[3ull * i + 1u], z = pts[3ull * i + 2u];
  const float tx = (x - g.o[0]) / g.cell, ty = (y - g.o[1]) / g.cell, tz = (z - g.o[2]) / g.cell;
  bool ok = pg_finite3(x, y, z);
  if (!clamp)
    ok = ok && tx >= 0.0f && tx < (float)g.d[0] && ty >= 0.0f && ty < (float)g.d[1] &&
         tz >= 0.0f && tz < (float)g.d[2];
  const uint32_t key = (pg_cell(tx, g.d[0]) * g.d[1] + pg_cell(ty, g.d[1])) * g.d[2] +
                       pg_cell(tz, g.d[2]);
  keys[i] = (int32_t)(ok ? key : g.d[0] * g.d[1] * g.d[2]);
}

__global__ void __launch_bounds__(PG_THREADS) k_no_match(uint32_t nq, int32_t* __restrict__ index,
                                                         float* __restrict__ dist2) {
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;
  if (i >= nq) return;
  index[i] = -1;
  dist2[i] = INFINITY;
}

// the state of one query's walk (cell_grid.h)
struct PointWalk {
  const float4* __restrict__ sp;
  float qx, qy, qz;
  float best;     // B = min(best d2, max_dist^2)
  uint32_t bidx;  // PG_NONE: no match yet
  __device__ __forceinline__ void score(uint32_t k) {
    const float4 p = sp[k];
    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const uint32_t j = __float_as_uint(p.w);
    if (d2 < best || (d2 == best && j < bidx)) {
      best = d2;
      bidx = j;
    }
  }
};

__global__ void __launch_bounds__(PG_THREADS) k_nearest(const float4* __restrict__ sp,
                                                        const int32_t* __restrict__ offsets,
                                                        uint32_t n, GridArgs g,
                                                        const float* __restrict__ queries,
                                                        const int32_t* __restrict__ q_order,
                                                        uint32_t nq, float limit2,
                                                        int32_t* __restrict__ index,
                                                        float* __restrict__ dist2) {
  const uint32_t t = blockIdx.x * PG_THREADS + threadIdx.x;
  if (t >= nq) return;
  const uint32_t qi = q_order ? (uint32_t)q_order[t] : t;
  if (qi >= nq) return;  // a malformed order writes nothing outside the outputs
  PointWalk w;
  w.sp = sp;
  w.qx = queries[3ull * qi];
  w.qy = queries[3ull * qi + 1u];
  w.qz = queries[3ull * qi + 2u];
  w.best = limit2;
  w.bidx = PG_NONE;
  pg_walk(offsets, n, g, PG_K, limit2, w);
  const bool hit = w.bidx != PG_NONE;
  index[qi] = hit ? (int32_t)w.bidx : -1;
  dist2[qi] = hit ? w.best : INFINITY;
}

}  // namespace

extern "C" int32_t ucsa_point_cell_keys(const float* points, uint32_t n, const float* origin,
                                        float cell, const uint32_t* dims, uint32_t clamp,
                                        int32_t* keys, void* stream) {
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFu, 1);
  GridArgs g;
  const int bad = pg_grid_args(origin, cell, dims, g);
  UCSA_CHECK_ARG(bad != 1, 2);
  UCSA_CHECK_ARG(bad != 2, 3);
  UCSA_CHECK_ARG(bad != 3, 4);
  UCSA_CHECK_ARG(clamp <= 1u, 5);
  if (n == 0) return 0;
  UCSA_CHECK_ARG(points, 0);
  UCSA_CHECK_ARG(keys, 6);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_cell_keys, dim3(ucsa_div_up(n, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, points, n, g, clamp, keys);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_nearest_point(const float* sorted_points, const int32_t* offsets,
                                      uint32_t n, const float* origin, float cell,
                                      const uint32_t* dims, const float* queries,
                                      const int32_t* q_order, uint32_t nq, float max_dist,
                                      int32_t* index, float* dist2, void* stream) {
  GridArgs g;
  float limit2;
  const void* outs[] = {index, dist2};
  const int32_t st = pg_search_args(sorted_points, offsets, n, origin, cell, dims, queries, nq,
                                    max_dist, outs, 2, g, limit2);
  if (st != 0 || nq == 0) return st;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ucsa_div_up(nq, PG_THREADS));
  UCSA_CLEAR_ERR();
  if (n == 0)
    hipLaunchKernelGGL(k_no_match, grid, dim3(PG_THREADS), 0, s, nq, index, dist2);
  else
    hipLaunchKernelGGL(k_nearest, grid, dim3(PG_THREADS), 0, s, (const float4*)sorted_points,
                       offsets, n, g, queries, q_order, nq, limit2, index, dist2);
  return ucsa_launch_status();
}
