// Scores of many rigid hypotheses against a TSDF volume in one call (not in the
// reference): ucsa_tsdf_score_transforms.  The contract is stated in
// include/ucsa_hip.h; tests/global_register_numpy.py restates it over the sample
// of tests/tsdf_register_numpy.py and the four integers per transform match it
// byte for byte.
//
// k_tsdf_score  a lane per point in work-groups of 256 points (blockIdx.y), a
//               tile of TS_TILE transforms per work-group (blockIdx.x).  The
//               point is loaded once.  The loop over the tile is uniform, and so
//               is the address of a transform's twelve floats: they arrive as
//               scalar loads.  Per transform the point is moved, its cell found,
//               the cell's eight weights and eight values gathered (eight
//               8-byte loads issued together, before the first use) and the
//               trilinear value F formed in k_tsdf_icp_sums' expressions (restated here:
//               mesh_register.hip is not touched; the gradient is not needed).
//               The two counts are a ballot and a popcount, sum e is reduced
//               over the wave in 32 bits (64 * 2^20 = 2^26), sum e^2 in 64; lane
//               0 of each wave puts the four numbers into LDS.  Behind the one
//               barrier a lane per (transform, number) adds the four waves and
//               adds the result, if it is not zero, to the zeroed output with a
//               64-bit integer atomic (as label_fusion.hip does).
//
// Integer sums only: no float atomics, and the result does not depend on the
// order of the points, the adds or the work-groups.  The barrier is reached by
// every lane: the loop's bounds are uniform, a lane with i >= n holds a NaN
// point (outside every lattice) and nothing returns early.
//
// Why every index is in range: as in k_tsdf_icp_sums, no float is converted to
// an integer and no index is formed before `inside` holds, that is
// 0 <= g_a <= n_a - 1 on every axis (a NaN fails both comparisons).  Then
// fl_a = min(floor(g_a), n_a - 2) is an integer in [0, n_a - 2] (the host checks
// n_a >= 2), the cell's far corner is a lattice point, and its linear index is
// at most nx*ny*nz - 1 <= 2^31 - 2, so the uint32 products do not wrap; an
// 8-byte load at a corner with k = 0 ends with the corner at k = 1, inside the
// array.  A
// transform's index k0 + blockIdx.x * TS_TILE + t is below K by the loop's
// bound; a point's index is below n before it is read; a row of `scores` is
// written only for such a k.
#include "ucsa_common.h"

namespace {

constexpr uint32_t TS_THREADS = 256;
constexpr uint32_t TS_WAVES = TS_THREADS / UCSA_WAVE;
constexpr uint32_t TS_TILE = UCSA_TSDF_SCORE_TILE;  // transforms per work-group
constexpr uint32_t TS_MAX_TILES = 65535;            // tiles per launch, at most
constexpr uint32_t TS_MAX_GROUPS = 1u << 22;        // work-groups per launch, at most

struct TsLattice {
  uint32_t n[3];
  float o[3], h[3];
};

inline bool ts_host_finite(float v) { return v - v == 0.0f; }

__device__ __forceinline__ float ts_lerp(float x, float y, float f) { return x + f * (y - x); }

template <int CTRL>
__device__ __forceinline__ uint32_t ts_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}

template <int CTRL>
__device__ __forceinline__ unsigned long long ts_dpp64(unsigned long long v) {
  const uint32_t lo = ts_dpp<CTRL>((uint32_t)v), hi = ts_dpp<CTRL>((uint32_t)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// the sum over the wave's 64 lanes, in every lane; all lanes are active (the
// exchange steps are those of icp_wave_tree in mesh_register.hip)
__device__ __forceinline__ uint32_t ts_wave_sum(uint32_t v) {
  v += ts_dpp<0xB1>(v);   // quad_perm:[1,0,3,2]
  v += ts_dpp<0x4E>(v);   // quad_perm:[2,3,0,1]
  v += ts_dpp<0x141>(v);  // row_half_mirror
  v += ts_dpp<0x140>(v);  // row_mirror
  v += (uint32_t)__shfl_xor((int)v, 16, 64);
  v += (uint32_t)__shfl_xor((int)v, 32, 64);
  return v;
}

__device__ __forceinline__ unsigned long long ts_wave_sum(unsigned long long v) {
  v += ts_dpp64<0xB1>(v);
  v += ts_dpp64<0x4E>(v);
  v += ts_dpp64<0x141>(v);
  v += ts_dpp64<0x140>(v);
  v += (unsigned long long)__shfl_xor((long long)v, 16, 64);
  v += (unsigned long long)__shfl_xor((long long)v, 32, 64);
  return v;
}

__global__ void __launch_bounds__(TS_THREADS) k_tsdf_score(const float* __restrict__ tsdf,
                                                           const float* __restrict__ weight,
                                                           TsLattice L,
                                                           const float* __restrict__ points,
                                                           uint32_t n,
                                                           const float* __restrict__ transforms,
                                                           uint32_t k0, uint32_t K,
                                                           float min_weight, float max_tsdf,
                                                           unsigned long long* __restrict__ scores) {
  __shared__ unsigned long long sh[TS_TILE * 4u * TS_WAVES];  // [transform][number][wave]
  const uint32_t i = blockIdx.y * TS_THREADS + threadIdx.x;   // < 2^23 + 256
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  float x = NAN, y = NAN, z = NAN;  // no point: outside every lattice
  if (i < n) {
    x = points[3ull * i];
    y = points[3ull * i + 1u];
    z = points[3ull * i + 2u];
  }
  const uint32_t first = k0 + blockIdx.x * TS_TILE;  // < K: the host sizes the grid
  const uint32_t count = K - first < TS_TILE ? K - first : TS_TILE;
  const uint32_t sj = L.n[2], si = L.n[1] * L.n[2];
#pragma unroll 1
  for (uint32_t t = 0; t < count; ++t) {
    const float* __restrict__ T = transforms + 12ull * (first + t);  // uniform: scalar loads
    float q[3];
    q[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    q[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    q[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    float g[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      g[a] = (q[a] - L.o[a]) / L.h[a];
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
      const uint32_t base = (c[0] * L.n[1] + c[1]) * L.n[2] + c[2];
      // v[4i + 2j + k]: both arrays, all loads before the first use.  The corners k = 0, 1
      // are neighbours in memory: one 8-byte load each (4-byte aligned, which a global load
      // takes), eight loads for the sixteen floats: 1.27x the rate of sixteen 4-byte loads
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
    bool observed = inside;
#pragma unroll
    for (int c = 0; c < 8; ++c) observed = observed && w[c] >= min_weight;
    const float c00 = ts_lerp(v[0], v[1], f[2]), c01 = ts_lerp(v[2], v[3], f[2]);
    const float c10 = ts_lerp(v[4], v[5], f[2]), c11 = ts_lerp(v[6], v[7], f[2]);
    const float c_0 = ts_lerp(c00, c01, f[1]), c_1 = ts_lerp(c10, c11, f[1]);
    const float F = ts_lerp(c_0, c_1, f[0]);
    const bool inlier = observed && fabsf(F) <= max_tsdf;  // a NaN is neither
    const bool free_space = observed && F > max_tsdf;
    // |F| <= max_tsdf < 1: the product is exact, e <= 2^20 and e * e <= 2^40
    const uint32_t e = inlier ? (uint32_t)rintf(fabsf(F) * 1048576.0f) : 0u;
    const uint32_t n_in = (uint32_t)__popcll(__ballot(inlier));
    const uint32_t n_free = (uint32_t)__popcll(__ballot(free_space));
    const uint32_t s1 = ts_wave_sum(e);
    const unsigned long long s2 = ts_wave_sum((unsigned long long)e * e);
    if (lane == 0u) {
      unsigned long long* row = sh + (size_t)t * 4u * TS_WAVES + wave;
      row[0] = n_in;
      row[TS_WAVES] = n_free;
      row[2u * TS_WAVES] = s1;
      row[3u * TS_WAVES] = s2;
    }
  }
  __syncthreads();
  const uint32_t c = threadIdx.x;  // (transform c / 4, number c % 4)
  if (c < count * 4u) {
    const unsigned long long* row = sh + (size_t)c * TS_WAVES;
    const unsigned long long sum = (row[0] + row[1]) + (row[2] + row[3]);
    if (sum != 0ull) atomicAdd(scores + 4ull * first + c, sum);
  }
}

}  // namespace

extern "C" int32_t ucsa_tsdf_score_transforms(const float* tsdf, const float* weight, uint32_t nx,
                                              uint32_t ny, uint32_t nz, const float* origin3,
                                              const float* spacing3, const float* points,
                                              uint32_t n, const float* transforms, uint32_t K,
                                              float min_weight, float max_tsdf, int64_t* scores,
                                              void* stream) {
  UCSA_CHECK_ARG(tsdf, 0);
  UCSA_CHECK_ARG(weight, 1);
  UCSA_CHECK_ARG(nx >= 2 && ny >= 1 && nz >= 1 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 2);
  UCSA_CHECK_ARG(ny >= 2, 3);
  UCSA_CHECK_ARG(nz >= 2, 4);
  UCSA_CHECK_ARG(origin3 && ts_host_finite(origin3[0]) && ts_host_finite(origin3[1]) &&
                     ts_host_finite(origin3[2]), 5);
  UCSA_CHECK_ARG(spacing3, 6);
  for (int a = 0; a < 3; ++a) UCSA_CHECK_ARG(spacing3[a] > 0.0f && ts_host_finite(spacing3[a]), 6);
  UCSA_CHECK_ARG(n <= (1u << 23), 8);
  UCSA_CHECK_ARG(n == 0 || points, 7);
  UCSA_CHECK_ARG(K <= 0x7FFFFFFFu, 10);
  UCSA_CHECK_ARG(K == 0 || transforms, 9);
  UCSA_CHECK_ARG(min_weight > 0.0f, 11);
  UCSA_CHECK_ARG(max_tsdf > 0.0f && max_tsdf < 1.0f, 12);
  UCSA_CHECK_ARG(K == 0 || scores, 13);
  if (K == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  UCSA_CLEAR_ERR();
  const hipError_t zeroed = hipMemsetAsync(scores, 0, (size_t)K * 4u * sizeof(int64_t), s);
  if (zeroed != hipSuccess) return -(int32_t)zeroed;
  if (n == 0) return 0;
  TsLattice L;
  L.n[0] = nx, L.n[1] = ny, L.n[2] = nz;
  for (int a = 0; a < 3; ++a) L.o[a] = origin3[a], L.h[a] = spacing3[a];
  const uint32_t groups_y = ucsa_div_up(n, TS_THREADS);  // <= 2^15
  const uint32_t tiles = ucsa_div_up(K, TS_TILE);        // <= 2^27
  uint32_t per_launch = TS_MAX_GROUPS / groups_y;        // >= 128
  if (per_launch > TS_MAX_TILES) per_launch = TS_MAX_TILES;
  for (uint32_t done = 0; done < tiles; done += per_launch) {
    const uint32_t now = tiles - done < per_launch ? tiles - done : per_launch;
    hipLaunchKernelGGL(k_tsdf_score, dim3(now, groups_y), dim3(TS_THREADS), 0, s, tsdf, weight, L,
                       points, n, transforms, done * TS_TILE, K, min_weight, max_tsdf,
                       (unsigned long long*)scores);
  }
  return ucsa_launch_status();
}
