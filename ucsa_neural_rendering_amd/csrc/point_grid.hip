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
// k_nearest        a lane per query.  Rings r = 0, 1, ... of cells around the
//                  query's clamped cell, clipped to per-axis limits [lo, hi]
//                  that start at the grid.  Along z the cells of a row are
//                  consecutive in the sorted order, so a run of cells costs two
//                  offset reads.  After each ring the six slabs of unvisited
//                  cells (beyond the ring, on each side of each axis) are
//                  tested: a slab whose near wall is farther from the query
//                  than B = min(best d2, max_dist^2) -- strictly, and with the
//                  margins below -- is cut off by moving that limit in; the
//                  walk ends when no slab is left.
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
//   * a comparison with a NaN is false: no cut, more walking, the same result.
// Every loop is bounded by the grid's dims; offsets are clamped into [0, n]; no
// atomics, no LDS, no waiting on another thread.
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

struct Walk {
  float qx, qy, qz;
  float best;     // B = min(best d2, max_dist^2)
  uint32_t bidx;  // PG_NONE: no match yet
};

// the candidates of the cells lin0 .. lin1 of one row (consecutive in the sorted order)
__device__ __forceinline__ void pg_run(const float4* __restrict__ sp,
                                       const int32_t* __restrict__ offsets, uint32_t n,
                                       uint32_t lin0, uint32_t lin1, Walk& w) {
  int32_t b = offsets[lin0], e = offsets[lin1 + 1u];
  b = b < 0 ? 0 : b;
  e = e > (int32_t)n ? (int32_t)n : e;
  for (int32_t k = b; k < e; ++k) {  // 0 <= k < n
    const float4 p = sp[k];
    const float dx = w.qx - p.x, dy = w.qy - p.y, dz = w.qz - p.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const uint32_t j = __float_as_uint(p.w);
    if (d2 < w.best || (d2 == w.best && j < w.bidx)) {
      w.best = d2;
      w.bidx = j;
    }
  }
}

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
  Walk w;
  w.qx = queries[3ull * qi];
  w.qy = queries[3ull * qi + 1u];
  w.qz = queries[3ull * qi + 2u];
  w.best = limit2;
  w.bidx = PG_NONE;
  const int32_t nx = (int32_t)g.d[0], ny = (int32_t)g.d[1], nz = (int32_t)g.d[2];
  const float h = g.cell;
  // the box's far corner and the slack of every wall distance, per axis
  const float topx = g.o[0] + (float)g.d[0] * h, topy = g.o[1] + (float)g.d[1] * h,
              topz = g.o[2] + (float)g.d[2] * h;
  const float Sx = PG_K * ((fabsf(g.o[0]) + fabsf(topx)) + fabsf(w.qx));
  const float Sy = PG_K * ((fabsf(g.o[1]) + fabsf(topy)) + fabsf(w.qy));
  const float Sz = PG_K * ((fabsf(g.o[2]) + fabsf(topz)) + fabsf(w.qz));
  bool walk = pg_finite3(w.qx, w.qy, w.qz);
  if (walk) {
    // farther than max_dist from the box that holds the points: no ring at all
    const float ex = fmaxf(fmaxf(g.o[0] - w.qx, w.qx - topx) - Sx, 0.0f);
    const float ey = fmaxf(fmaxf(g.o[1] - w.qy, w.qy - topy) - Sy, 0.0f);
    const float ez = fmaxf(fmaxf(g.o[2] - w.qz, w.qz - topz) - Sz, 0.0f);
    const float out2 = (ex * ex + ey * ey) + ez * ez;
    walk = !(out2 > limit2 * PG_ONE_PLUS_K);
  }
  if (walk) {
    const int32_t cx = (int32_t)pg_cell((w.qx - g.o[0]) / h, g.d[0]);
    const int32_t cy = (int32_t)pg_cell((w.qy - g.o[1]) / h, g.d[1]);
    const int32_t cz = (int32_t)pg_cell((w.qz - g.o[2]) / h, g.d[2]);
    int32_t lox = 0, loy = 0, loz = 0, hix = nx - 1, hiy = ny - 1, hiz = nz - 1;
    // r grows by one per pass and a slab exists only while cx + r + 1 <= hix or
    // cx - r - 1 >= lox (and so on): at most max(nx, ny, nz) passes
    for (int32_t r = 0;; ++r) {
      const int32_t x0 = max(cx - r, lox), x1 = min(cx + r, hix);
      const int32_t y0 = max(cy - r, loy), y1 = min(cy + r, hiy);
      const int32_t z0 = max(cz - r, loz), z1 = min(cz + r, hiz);
      for (int32_t x = x0; x <= x1; ++x) {
        const bool xedge = x == cx - r || x == cx + r;
        for (int32_t y = y0; y <= y1; ++y) {
          const uint32_t row = (uint32_t)(x * ny + y) * (uint32_t)nz;
          if (xedge || y == cy - r || y == cy + r) {
            if (z0 <= z1) pg_run(sp, offsets, n, row + (uint32_t)z0, row + (uint32_t)z1, w);
          } else {  // r >= 1 here: the two caps of the column
            if (cz - r >= loz) pg_run(sp, offsets, n, row + (uint32_t)(cz - r), row + (uint32_t)(cz - r), w);
            if (cz + r <= hiz) pg_run(sp, offsets, n, row + (uint32_t)(cz + r), row + (uint32_t)(cz + r), w);
          }
        }
      }
      const float bk = w.best * PG_ONE_PLUS_K;
      bool left = false;
      if (cx + r + 1 <= hix) {
        if (pg_cut(g.o[0], h, w.qx, Sx, bk, cx + r + 1, true)) hix = cx + r; else left = true;
      }
      if (cx - r - 1 >= lox) {
        if (pg_cut(g.o[0], h, w.qx, Sx, bk, cx - r, false)) lox = cx - r; else left = true;
      }
      if (cy + r + 1 <= hiy) {
        if (pg_cut(g.o[1], h, w.qy, Sy, bk, cy + r + 1, true)) hiy = cy + r; else left = true;
      }
      if (cy - r - 1 >= loy) {
        if (pg_cut(g.o[1], h, w.qy, Sy, bk, cy - r, false)) loy = cy - r; else left = true;
      }
      if (cz + r + 1 <= hiz) {
        if (pg_cut(g.o[2], h, w.qz, Sz, bk, cz + r + 1, true)) hiz = cz + r; else left = true;
      }
      if (cz - r - 1 >= loz) {
        if (pg_cut(g.o[2], h, w.qz, Sz, bk, cz - r, false)) loz = cz - r; else left = true;
      }
      if (!left) break;
    }
  }
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
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFu, 2);
  GridArgs g;
  const int bad = pg_grid_args(origin, cell, dims, g);
  UCSA_CHECK_ARG(bad != 1, 3);
  UCSA_CHECK_ARG(bad != 2, 4);
  UCSA_CHECK_ARG(bad != 3, 5);
  UCSA_CHECK_ARG(nq <= 0x7FFFFFFFu, 8);
  const float limit2 = max_dist * max_dist;
  UCSA_CHECK_ARG(max_dist > 0.0f && pg_host_finite(max_dist) && pg_host_finite(limit2), 9);
  if (nq == 0) return 0;
  UCSA_CHECK_ARG(queries, 6);
  UCSA_CHECK_ARG(index, 10);
  UCSA_CHECK_ARG(dist2, 11);
  UCSA_CHECK_ARG(n == 0 || sorted_points, 0);
  UCSA_CHECK_ARG(n == 0 || offsets, 1);
  UCSA_CHECK_ARG(n == 0 || ((uintptr_t)sorted_points & 15u) == 0, 0);
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
