// The sample of a TSDF volume at a moved point, shared by the ICP steps against a
// volume (mesh_register.hip: k_tsdf_icp_sums, k_tsdf_icp_sums_batch) and the
// scores of many hypotheses (tsdf_score.hip: k_tsdf_score), with the lattice's
// arguments and their checks.  The expressions are those of the contracts in
// include/ucsa_hip.h (the ray-caster's trilinear value and gradient), restated
// in tests/tsdf_register_numpy.py: every kernel that calls tsdf_sample promises
// the same float32 bits.
#pragma once
#include <cmath>

#include "ucsa_common.h"

namespace {

struct TsdfLattice {
  uint32_t n[3];
  float o[3], h[3];
};

// The lattice arguments every entry point takes first, in the order of their
// argument indices: the index 0..6 of the first that fails, or -1; fills L.
inline int tsdf_lattice_args(const float* tsdf, const float* weight, uint32_t nx, uint32_t ny,
                             uint32_t nz, const float* origin3, const float* spacing3,
                             TsdfLattice& L) {
  if (!tsdf) return 0;
  if (!weight) return 1;
  if (!(nx >= 2 && ny >= 1 && nz >= 1 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull)) return 2;
  if (!(ny >= 2)) return 3;
  if (!(nz >= 2)) return 4;
  if (!(origin3 && std::isfinite(origin3[0]) && std::isfinite(origin3[1]) &&
        std::isfinite(origin3[2])))
    return 5;
  if (!spacing3) return 6;
  for (int a = 0; a < 3; ++a)
    if (!(spacing3[a] > 0.0f && std::isfinite(spacing3[a]))) return 6;
  L.n[0] = nx, L.n[1] = ny, L.n[2] = nz;
  for (int a = 0; a < 3; ++a) L.o[a] = origin3[a], L.h[a] = spacing3[a];
  return -1;
}

__device__ __forceinline__ float tsdf_lerp(float x, float y, float f) { return x + f * (y - x); }

struct TsdfSample {
  float q[3];     // the moved point
  float F;        // the trilinear value
  float G[3];     // its gradient per scene unit, not normalised
  float ln;       // the gradient's length
  bool observed;  // inside the lattice, all eight corners with weight >= min_weight
};

// The point (x, y, z) moved by the twelve floats T of [R | t], its cell of the
// lattice, the cell's eight weights and eight values, the trilinear value F, the
// gradient and its length.  LOAD_BYTES is the gather's flavour: 4, sixteen 4-byte
// loads; 8, eight 8-byte loads, the corners k = 0, 1 being neighbours in memory
// (4-byte aligned, which a global load takes).  Either way every load of the
// gather is issued before the first use.  A caller that does not use G and ln
// (k_tsdf_score) pays nothing for them: the function is inlined and they are dead.
//
// Why every index is in range (the one statement of it; the kernels refer
// here).  No float is converted to an integer and no index is formed before
// `inside` holds, that is 0 <= g_a <= n_a - 1 on every axis; a NaN fails both
// comparisons, so a lane without a point passes NaN coordinates, is outside
// every lattice and loads nothing.  Then fl_a = min(floor(g_a), n_a - 2) is an
// integer in [0, n_a - 2] (tsdf_lattice_args checks n_a >= 2), so the cell's far
// corner c_a + 1 <= n_a - 1 is a lattice point; its linear index is at most
// nx*ny*nz - 1 <= 2^31 - 2 (checked there too), so the uint32 products do not
// wrap; an 8-byte load at a corner with k = 0 ends with the corner at k = 1,
// inside the array.
template <int LOAD_BYTES>
__device__ __forceinline__ TsdfSample tsdf_sample(const float* __restrict__ tsdf,
                                                  const float* __restrict__ weight,
                                                  const TsdfLattice& L,
                                                  const float* __restrict__ T, float x, float y,
                                                  float z, float min_weight) {
  static_assert(LOAD_BYTES == 4 || LOAD_BYTES == 8, "4-byte loads or 8-byte pairs");
  TsdfSample s;
  s.q[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  s.q[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  s.q[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
  float g[3];
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g[a] = (s.q[a] - L.o[a]) / L.h[a];
    inside = inside && g[a] >= 0.0f && g[a] <= (float)(L.n[a] - 1u);
  }
  float f[3] = {0.0f, 0.0f, 0.0f};
  float w[8], v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) w[c] = v[c] = 0.0f;
  if (inside) {
    uint32_t c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float fl = fminf(floorf(g[a]), (float)(L.n[a] - 2u));
      c[a] = (uint32_t)fl;
      f[a] = g[a] - fl;
    }
    const uint32_t sj = L.n[2], si = L.n[1] * L.n[2];
    const uint32_t base = (c[0] * L.n[1] + c[1]) * L.n[2] + c[2];
    // v[4i + 2j + k]: both arrays, all loads before the first use
    if constexpr (LOAD_BYTES == 4) {
#pragma unroll
      for (uint32_t c8 = 0; c8 < 8u; ++c8) {
        const uint32_t at = base + ((c8 & 4u) ? si : 0u) + ((c8 & 2u) ? sj : 0u) + (c8 & 1u);
        w[c8] = weight[at];
        v[c8] = tsdf[at];
      }
    } else {
#pragma unroll
      for (uint32_t c4 = 0; c4 < 4u; ++c4) {
        const uint32_t at = base + ((c4 & 2u) ? si : 0u) + ((c4 & 1u) ? sj : 0u);
        float2 pw, pv;
        __builtin_memcpy(&pw, weight + at, sizeof(float2));
        __builtin_memcpy(&pv, tsdf + at, sizeof(float2));
        w[2u * c4] = pw.x, w[2u * c4 + 1u] = pw.y;
        v[2u * c4] = pv.x, v[2u * c4 + 1u] = pv.y;
      }
    }
  }
  s.observed = inside;
#pragma unroll
  for (int c = 0; c < 8; ++c) s.observed = s.observed && w[c] >= min_weight;
  const float c00 = tsdf_lerp(v[0], v[1], f[2]), c01 = tsdf_lerp(v[2], v[3], f[2]);
  const float c10 = tsdf_lerp(v[4], v[5], f[2]), c11 = tsdf_lerp(v[6], v[7], f[2]);
  const float c_0 = tsdf_lerp(c00, c01, f[1]), c_1 = tsdf_lerp(c10, c11, f[1]);
  s.F = tsdf_lerp(c_0, c_1, f[0]);
  s.G[0] = c_1 - c_0;
  s.G[1] = tsdf_lerp(c01 - c00, c11 - c10, f[0]);
  s.G[2] = tsdf_lerp(tsdf_lerp(v[1] - v[0], v[3] - v[2], f[1]),
                     tsdf_lerp(v[5] - v[4], v[7] - v[6], f[1]), f[0]);
#pragma unroll
  for (int a = 0; a < 3; ++a) s.G[a] = s.G[a] / L.h[a];
  s.ln = sqrtf((s.G[0] * s.G[0] + s.G[1] * s.G[1]) + s.G[2] * s.G[2]);
  return s;
}

}  // namespace
