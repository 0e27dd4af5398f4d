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
//               scalar loads.  Per transform the sample is tsdf_sample's
//               (tsdf_sample.h, which states why every index of the gather is in
//               range): the point is moved, its cell found, the cell's eight
//               weights and eight values gathered as eight 8-byte loads issued
//               together, before the first use (1.27x the rate of sixteen 4-byte
//               loads), and the trilinear value F formed; the gradient is not
//               used and is dead code here.  The two counts are a ballot and a
//               popcount, sum e is reduced over the wave in 32 bits
//               (64 * 2^20 = 2^26), sum e^2 in 64 (wave_tree_sum, wave_ops.h);
//               lane 0 of each wave puts the four numbers into LDS.  Behind the
//               one barrier a lane per (transform, number) adds the four waves
//               and adds the result, if it is not zero, to the zeroed output with
//               a 64-bit integer atomic (as label_fusion.hip does).
//
// Integer sums only: no float atomics, and the result does not depend on the
// order of the points, the adds or the work-groups.  The barrier is reached by
// every lane: the loop's bounds are uniform, a lane with i >= n holds a NaN
// point (outside every lattice: it loads nothing) and nothing returns early.
// A transform's index k0 + blockIdx.x * TS_TILE + t is below K by the loop's
// bound; a point's index is below n before it is read; a row of `scores` is
// written only for such a k.
#include "tsdf_sample.h"
#include "wave_ops.h"

namespace {

constexpr uint32_t TS_THREADS = 256;
constexpr uint32_t TS_WAVES = TS_THREADS / UCSA_WAVE;
constexpr uint32_t TS_TILE = UCSA_TSDF_SCORE_TILE;  // transforms per work-group
constexpr uint32_t TS_MAX_TILES = 65535;            // tiles per launch, at most
constexpr uint32_t TS_MAX_GROUPS = 1u << 22;        // work-groups per launch, at most

__global__ void __launch_bounds__(TS_THREADS) k_tsdf_score(const float* __restrict__ tsdf,
                                                           const float* __restrict__ weight,
                                                           TsdfLattice L,
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
#pragma unroll 1
  for (uint32_t t = 0; t < count; ++t) {
    const TsdfSample sm = tsdf_sample<8>(tsdf, weight, L, transforms + 12ull * (first + t), x, y, z,
                                         min_weight);
    const float F = sm.F;
    const bool inlier = sm.observed && fabsf(F) <= max_tsdf;  // a NaN is neither
    const bool free_space = sm.observed && F > max_tsdf;
    // |F| <= max_tsdf < 1: the product is exact, e <= 2^20 and e * e <= 2^40
    const uint32_t e = inlier ? (uint32_t)rintf(fabsf(F) * 1048576.0f) : 0u;
    const uint32_t n_in = (uint32_t)__popcll(__ballot(inlier));
    const uint32_t n_free = (uint32_t)__popcll(__ballot(free_space));
    const uint32_t s1 = wave_tree_sum(e);
    const unsigned long long s2 = wave_tree_sum((unsigned long long)e * e);
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
    const unsigned long long sum = waves4_sum(row);
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
  TsdfLattice L;
  const int bad = tsdf_lattice_args(tsdf, weight, nx, ny, nz, origin3, spacing3, L);
  UCSA_CHECK_ARG(bad < 0, bad);
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
