// The uniform cell grid shared by point_grid.hip and triangle_grid.hip: the
// grid's arguments and their checks, the cell of a coordinate, and the test that
// cuts a slab of unvisited cells off a ring walk.  The arithmetic is restated in
// tests/nearest_numpy.py (cell_coords, the stop rule) and must stay as it is
// there: both searches promise numpy's float32 bits.
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

// host side (the device overloads of isfinite are not visible to a host function)
inline bool pg_host_finite(float v) { return v - v == 0.0f; }

// origin finite, cell > 0 and finite, dims >= 1 with at most 2^24 cells, and the
// box's far corner finite: -> 0, or the index (1..3) of the offending one
inline int pg_grid_args(const float* origin, float cell, const uint32_t* dims, GridArgs& g) {
  if (!origin || !(pg_host_finite(origin[0]) && pg_host_finite(origin[1]) && pg_host_finite(origin[2]))) return 1;
  if (!(cell > 0.0f) || !pg_host_finite(cell)) return 2;
  if (!dims || dims[0] == 0 || dims[1] == 0 || dims[2] == 0) return 3;
  if ((uint64_t)dims[0] * dims[1] > PG_MAX_CELLS ||
      (uint64_t)dims[0] * dims[1] * dims[2] > PG_MAX_CELLS)
    return 3;
  for (int a = 0; a < 3; ++a) {
    g.o[a] = origin[a];
    g.d[a] = dims[a];
    if (!pg_host_finite(origin[a] + (float)dims[a] * cell)) return 2;
  }
  g.cell = cell;
  return 0;
}

}  // namespace
