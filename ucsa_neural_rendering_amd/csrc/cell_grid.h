// The uniform cell grid shared by point_grid.hip, triangle_grid.hip and
// mesh_simplify.hip: the grid's arguments and their checks, the cell of a
// coordinate, and the ring walk of the two radius searches (pg_walk) with the
// arguments their entry points share.  The arithmetic is restated once in
// tests/nearest_numpy.py (cell_coords and ring_walk, which both models call) and
// must stay as it is there: both searches promise numpy's float32 bits.
#pragma once
#include "ucsa_common.h"

namespace {

constexpr uint32_t PG_THREADS = 256;
constexpr uint32_t PG_MAX_CELLS = 1u << 24;
constexpr float PG_K = 9.5367431640625e-07f;           // 2^-20
constexpr float PG_ONE_PLUS_K = 1.00000095367431640625f;  // 1 + 2^-20
constexpr uint32_t PG_NONE = 0xFFFFFFFFu;

struct GridArgs {
  float o[3];
  float cell;
  uint32_t d[3];
};

__device__ __forceinline__ bool pg_finite3(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z);
}

// the clamp comes before the conversion: the float is in [0, dim - 1] <= 2^24
__device__ __forceinline__ uint32_t pg_cell(float t, uint32_t dim) {
  const float c = fminf(fmaxf(t, 0.0f), (float)(dim - 1u));  // fmaxf(NaN, 0) = 0
  return (uint32_t)floorf(c);
}

// one side of one axis after ring r: is there a slab, and can it be cut?
// `wall_cell` is the index whose low wall bounds the slab (the slab's first cell
// on the far side, the cell after the slab's last on the near side).
__device__ __forceinline__ bool pg_cut(float o, float cell, float q, float S, float bk,
                                       int32_t wall_cell, bool far_side) {
  const float wall = o + (float)wall_cell * cell;
  const float gap = (far_side ? wall - q : q - wall) - S;
  return gap > 0.0f && gap * gap > bk;
}

// the candidates of the cells lin0 .. lin1 of one row (consecutive in the sorted order)
template <class State>
__device__ __forceinline__ void pg_run(const int32_t* __restrict__ offsets, uint32_t n,
                                       uint32_t lin0, uint32_t lin1, State& w) {
  int32_t b = offsets[lin0], e = offsets[lin1 + 1u];
  b = b < 0 ? 0 : b;
  e = e > (int32_t)n ? (int32_t)n : e;
  for (int32_t k = b; k < e; ++k) w.score((uint32_t)k);  // 0 <= k < n
}

// The ring walk of one query.  `w` is the query's state: its position qx, qy,
// qz, best = B = min(best d2, max_dist^2) (limit2 on entry), bidx (PG_NONE on
// entry) and score(k), which holds the candidate at sorted position k < n
// against (best, bidx).  Rings r = 0, 1, ... of cells around the query's clamped
// cell, clipped to per-axis limits [lo, hi] that start at the grid.  Along z the
// cells of a row are consecutive in the sorted order, so a run of cells costs
// two offset reads.  After each ring the six slabs of unvisited cells (beyond
// the ring, on each side of each axis) are tested: a slab whose near wall is
// farther from the query than B -- strictly, the gap shortened by
// S = ks * (|o| + |top| + |q|) and its square compared with B * (1 + 2^-20) -- is
// cut off by moving that limit in; the walk ends when no slab is left.  `ks` is
// the search's slack (PG_K for points, twice that for faces); why its cut is
// safe is argued at the head of each search's file.  A comparison with a NaN is
// false: no cut, more walking, the same result.  Every loop is bounded by the
// grid's dims; offsets are clamped into [0, n].
template <class State>
__device__ __forceinline__ void pg_walk(const int32_t* __restrict__ offsets, uint32_t n,
                                        const GridArgs& g, float ks, float limit2, State& w) {
  const int32_t nx = (int32_t)g.d[0], ny = (int32_t)g.d[1], nz = (int32_t)g.d[2];
  const float h = g.cell;
  // the box's far corner and the slack of every wall distance, per axis
  const float topx = g.o[0] + (float)g.d[0] * h, topy = g.o[1] + (float)g.d[1] * h,
              topz = g.o[2] + (float)g.d[2] * h;
  const float Sx = ks * ((fabsf(g.o[0]) + fabsf(topx)) + fabsf(w.qx));
  const float Sy = ks * ((fabsf(g.o[1]) + fabsf(topy)) + fabsf(w.qy));
  const float Sz = ks * ((fabsf(g.o[2]) + fabsf(topz)) + fabsf(w.qz));
  bool walk = pg_finite3(w.qx, w.qy, w.qz);
  if (walk) {
    // farther than max_dist from the box that holds the candidates: no ring at all
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
            if (z0 <= z1) pg_run(offsets, n, row + (uint32_t)z0, row + (uint32_t)z1, w);
          } else {  // r >= 1 here: the two caps of the column
            if (cz - r >= loz) pg_run(offsets, n, row + (uint32_t)(cz - r), row + (uint32_t)(cz - r), w);
            if (cz + r <= hiz) pg_run(offsets, n, row + (uint32_t)(cz + r), row + (uint32_t)(cz + r), w);
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
}

// host side (the device overloads of isfinite are not visible to a host function)
inline bool pg_host_finite(float v) { return v - v == 0.0f; }

// origin finite, cell > 0 and finite, dims in 1..max_dim (<= 2^24) each with at
// most max_cells cells, and the box's far corner finite: -> 0, or the index
// (1..3) of the offending one.  The defaults are those of a grid with an offset
// per cell.
inline int pg_grid_args(const float* origin, float cell, const uint32_t* dims, GridArgs& g,
                        uint32_t max_dim = PG_MAX_CELLS, uint64_t max_cells = PG_MAX_CELLS) {
  if (!origin || !(pg_host_finite(origin[0]) && pg_host_finite(origin[1]) && pg_host_finite(origin[2]))) return 1;
  if (!(cell > 0.0f) || !pg_host_finite(cell)) return 2;
  if (!dims) return 3;
  for (int a = 0; a < 3; ++a)
    if (dims[a] == 0 || dims[a] > max_dim) return 3;
  if ((uint64_t)dims[0] * dims[1] > max_cells ||  // no wrap under either caller's limits
      (uint64_t)dims[0] * dims[1] * dims[2] > max_cells)
    return 3;
  for (int a = 0; a < 3; ++a) {
    g.o[a] = origin[a];
    g.d[a] = dims[a];
    if (!pg_host_finite(origin[a] + (float)dims[a] * cell)) return 2;
  }
  g.cell = cell;
  return 0;
}

// The arguments ucsa_nearest_point and ucsa_nearest_triangle share, at the
// positions both give them: n (2), the grid (3..5), nq (8), max_dist (9), and
// once there is a query the queries (6), the `n_outs` outputs (10 ...), the
// records (0: present and 16-byte aligned) and the offsets (1).  -> 0 with `g`
// and `limit2` filled, or the error code of the first offending argument.
inline int32_t pg_search_args(const float* records, const int32_t* offsets, uint32_t n,
                              const float* origin, float cell, const uint32_t* dims,
                              const float* queries, uint32_t nq, float max_dist,
                              const void* const* outs, int n_outs, GridArgs& g, float& limit2) {
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFu, 2);
  const int bad = pg_grid_args(origin, cell, dims, g);
  UCSA_CHECK_ARG(bad != 1, 3);
  UCSA_CHECK_ARG(bad != 2, 4);
  UCSA_CHECK_ARG(bad != 3, 5);
  UCSA_CHECK_ARG(nq <= 0x7FFFFFFFu, 8);
  limit2 = max_dist * max_dist;
  UCSA_CHECK_ARG(max_dist > 0.0f && pg_host_finite(max_dist) && pg_host_finite(limit2), 9);
  if (nq == 0) return 0;
  UCSA_CHECK_ARG(queries, 6);
  for (int i = 0; i < n_outs; ++i) UCSA_CHECK_ARG(outs[i], 10 + i);
  UCSA_CHECK_ARG(n == 0 || records, 0);
  UCSA_CHECK_ARG(n == 0 || offsets, 1);
  UCSA_CHECK_ARG(n == 0 || ((uintptr_t)records & 15u) == 0, 0);
  return 0;
}

}  // namespace
