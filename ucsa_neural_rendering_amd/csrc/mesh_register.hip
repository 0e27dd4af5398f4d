// One step of ICP against a triangle mesh (not in the reference): ucsa_icp_sums.
// The contract is stated in include/ucsa_hip.h; tests/register_numpy.py restates
// it over the brute-force search of tests/surface_numpy.py and the 29 sums match
// it byte for byte.  The same step against a TSDF volume, ucsa_tsdf_icp_sums
// (k_tsdf_icp_sums, further down), shares the reduction and the reduce kernel,
// and so does the step against a pair of vertex and normal maps by projection,
// ucsa_projective_icp_sums (k_projective_icp_sums, after it).  The TSDF step for
// K transforms in one launch, ucsa_tsdf_icp_sums_batch (k_tsdf_icp_sums_batch,
// k_icp_reduce_batch), sits between the two and forms the same tree per row.
// The two frame trackers' steps with a weight per row (a robust kernel on the
// residual, a weight per point), ucsa_projective_icp_sums_weighted and
// ucsa_tsdf_icp_sums_weighted, come last: sibling kernels, the same reduction.
//
// k_icp_sums<MODE>  a lane per point in work-groups of 256: the point is moved by
//                   [R | t], the nearest-triangle search of triangle_grid.hip
//                   (pg_walk over FaceWalk with TG_KS) runs from the moved point,
//                   the closest point of the face found is evaluated again on the
//                   mesh's own corners (tri_closest.h: the same operands, the same
//                   bits, as in mesh_sdf.hip), and the rows (J, r) follow.  Only
//                   then are the 29 float64 terms formed, one after another from
//                   those floats, each reduced over the work-group at once: no
//                   term is live across the walk.  The work-group's 29 sums go to
//                   its row of the workspace (or to `sums` if it is the only one).
// k_icp_reduce      a lane per row of the previous stage, 256 rows per
//                   work-group, the same reduction: repeated until one row is left.
//
// The reduction is the contract's tree of adjacent pairs.  Inside a wave six
// exchange steps pair lane l with l^1, l^2, a lane of the neighbouring quad, a
// lane of the neighbouring half row, l^16 and l^32: after step k every lane of
// an aligned group of 2^k lanes holds the sum of that group's balanced tree
// (a + b is commutative in IEEE, so both partners compute the same bits), and
// any lane of the partner group will do as the source.  The first four steps
// are DPP moves of the two halves of the double (quad_perm, row_half_mirror,
// row_mirror: no LDS), the last two are __shfl_xor.  The four waves meet in LDS
// as (w0 + w1) + (w2 + w3): levels seven and eight.  A lane without a point
// (i >= n, no match) holds +0.0, which is the contract's padding.
//
// No atomics.  One barrier per work-group, which every lane reaches: a lane with
// i >= n takes the unmatched path and does not return early.  Every loop is
// bounded as in pg_walk (cell_grid.h); no lane waits for another outside that
// barrier.  A lane writes its own slots of face / dist2, a work-group its own row
// of the workspace; every index read from memory is checked before use.
#include "tri_closest.h"

namespace {

constexpr uint32_t ICP_SUMS = 29;

struct Rigid {
  float m[12];  // the rows of [R | t]
};

template <int CTRL>
__device__ __forceinline__ double icp_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// the balanced tree of adjacent pairs over the wave's 64 values, in every lane
__device__ __forceinline__ double icp_wave_tree(double v) {
  v = v + icp_dpp<0xB1>(v);   // quad_perm:[1,0,3,2]: l ^ 1
  v = v + icp_dpp<0x4E>(v);   // quad_perm:[2,3,0,1]: l ^ 2
  v = v + icp_dpp<0x141>(v);  // row_half_mirror: l -> 7 - l, the other quad of the eight
  v = v + icp_dpp<0x140>(v);  // row_mirror: l -> 15 - l, the other eight of the row
  v = v + __shfl_xor(v, 16, 64);
  v = v + __shfl_xor(v, 32, 64);
  return v;
}

// one of the 29 sums over the work-group: `sh` is [ICP_SUMS][4]
__device__ __forceinline__ void icp_put(double v, uint32_t c, double* sh) {
  v = icp_wave_tree(v);
  if ((threadIdx.x & 63u) == 0u) sh[4u * c + (threadIdx.x >> 6)] = v;
}

__device__ __forceinline__ void icp_finish(const double* sh, double* __restrict__ out) {
  __syncthreads();
  const uint32_t c = threadIdx.x;
  if (c < ICP_SUMS)
    out[(uint64_t)blockIdx.x * ICP_SUMS + c] = (sh[4u * c] + sh[4u * c + 1u]) + (sh[4u * c + 2u] + sh[4u * c + 3u]);
}

// the row k of one normal: J, r and the row's 1, each entry of J a product, then the difference
template <int ROWS>
__device__ __forceinline__ void icp_row(float q0, float q1, float q2, float p0, float p1, float p2,
                                        float n0, float n1, float n2, float (*V)[ROWS], int k) {
  V[0][k] = q1 * n2 - q2 * n1;
  V[1][k] = q2 * n0 - q0 * n2;
  V[2][k] = q0 * n1 - q1 * n0;
  V[3][k] = n0;
  V[4][k] = n1;
  V[5][k] = n2;
  V[6][k] = tg_dot(n0, n1, n2, p0, p1, p2);
  V[7][k] = 1.0f;
}

// a point's term of one sum: the products of the converted floats are exact in
// float64; the rows' terms are added in order; no match is a select of +0.0
template <int ROWS>
__device__ __forceinline__ double icp_term(bool matched, const float* x, const float* y) {
  double t = (double)x[0] * (double)y[0];
  if constexpr (ROWS == 3)
    t = (t + (double)x[1] * (double)y[1]) + (double)x[2] * (double)y[2];
  return matched ? t : 0.0;
}

template <int MODE>
__global__ void __launch_bounds__(PG_THREADS) k_icp_sums(const float4* __restrict__ rec,
                                                         const int32_t* __restrict__ offsets,
                                                         uint32_t n_pairs, GridArgs g,
                                                         const float* __restrict__ verts,
                                                         uint32_t nv,
                                                         const int32_t* __restrict__ faces,
                                                         uint32_t nf,
                                                         const float* __restrict__ unit,
                                                         const float* __restrict__ points,
                                                         uint32_t n, Rigid T, float limit2,
                                                         double* __restrict__ out,
                                                         int32_t* __restrict__ face,
                                                         float* __restrict__ dist2) {
  __shared__ double sh[ICP_SUMS * 4u];
  constexpr int ROWS = MODE == 0 ? 1 : 3;
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;  // < 2^31 + 256
  const bool live = i < n;
  FaceWalk w;
  w.rec = rec;
  w.qx = w.qy = w.qz = NAN;  // no point, or no candidates: no ring is walked
  if (live) {
    const float x = points[3ull * i], y = points[3ull * i + 1u], z = points[3ull * i + 2u];
    w.qx = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
    w.qy = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
    w.qz = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
  }
  w.best = limit2;
  w.bidx = PG_NONE;
  w.v = 0.0f;
  w.w = 0.0f;
  if (live && n_pairs != 0u) pg_walk(offsets, n_pairs, g, TG_KS, limit2, w);
  const bool hit = w.bidx != PG_NONE;
  if (live) {
    if (face) face[i] = hit ? (int32_t)w.bidx : -1;
    if (dist2) dist2[i] = hit ? w.best : INFINITY;
  }
  float V[8][ROWS];  // per row: J (0..5), r (6) and 1 (7)
#pragma unroll
  for (int a = 0; a < 8; ++a) {
#pragma unroll
    for (int k = 0; k < ROWS; ++k) V[a][k] = 0.0f;
  }
  bool matched = false;
  if (hit && w.bidx < nf) {  // a record that names no face matches nothing
    const Corners c = tg_corners(verts, nv, faces, w.bidx);
    if (c.ok) {
      matched = true;
      const float4 A = make_float4(c.ax, c.ay, c.az, 0.0f), B = make_float4(c.bx, c.by, c.bz, 0.0f),
                   C = make_float4(c.cx, c.cy, c.cz, 0.0f);
      float v, wt, d2, px, py, pz;
      int region;
      tg_closest_point(A, B, C, w.qx, w.qy, w.qz, v, wt, d2, region, px, py, pz);
      if constexpr (ROWS == 1) {
        const float* nn = unit + 3ull * w.bidx;
        icp_row<ROWS>(w.qx, w.qy, w.qz, px, py, pz, nn[0], nn[1], nn[2], V, 0);
      } else {
        icp_row<ROWS>(w.qx, w.qy, w.qz, px, py, pz, 1.0f, 0.0f, 0.0f, V, 0);
        icp_row<ROWS>(w.qx, w.qy, w.qz, px, py, pz, 0.0f, 1.0f, 0.0f, V, 1);
        icp_row<ROWS>(w.qx, w.qy, w.qz, px, py, pz, 0.0f, 0.0f, 1.0f, V, 2);
      }
    }
  }
  uint32_t col = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = a; b < 6; ++b) icp_put(icp_term<ROWS>(matched, V[a], V[b]), col++, sh);
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) icp_put(icp_term<ROWS>(matched, V[a], V[6]), col++, sh);
  icp_put(icp_term<ROWS>(matched, V[6], V[6]), col++, sh);
  icp_put(icp_term<ROWS>(matched, V[7], V[7]), col++, sh);  // the rows that count
  icp_finish(sh, out);
}

__global__ void __launch_bounds__(PG_THREADS) k_icp_reduce(const double* __restrict__ in,
                                                           uint32_t count,
                                                           double* __restrict__ out) {
  __shared__ double sh[ICP_SUMS * 4u];
  const uint32_t row = blockIdx.x * PG_THREADS + threadIdx.x;
  const bool live = row < count;
#pragma unroll 1
  for (uint32_t c = 0; c < ICP_SUMS; ++c)
    icp_put(live ? in[(uint64_t)row * ICP_SUMS + c] : 0.0, c, sh);
  icp_finish(sh, out);
}

// the rows of all stages but the last: what the workspace holds, in 29 doubles each
uint64_t icp_workspace_rows(uint32_t n) {
  uint64_t rows = 0;
  uint32_t c = n ? ucsa_div_up(n, PG_THREADS) : 1u;
  while (c > 1u) {
    rows += c;
    c = ucsa_div_up(c, PG_THREADS);
  }
  return rows;
}

// ---- one step of ICP against a TSDF volume: ucsa_tsdf_icp_sums ----
// k_tsdf_icp_sums  a lane per point in work-groups of 256: the point is moved by
//                  [R | t], its cell of the lattice is found, the cell's eight
//                  weights and eight values are gathered (sixteen loads issued
//                  together, before the first use), the trilinear value F and its
//                  gradient follow in the ray-caster's expressions (restated
//                  here: voxel_map.hip is not touched), and the row is
//                  r = -(F * trunc), J = (q x n, n).  The 29 terms are formed
//                  afterwards, one at a time, and reduced as in k_icp_sums:
//                  icp_put / icp_finish, then k_icp_reduce on the group results.
//
// Why every index is in range: no float is converted to an integer and no index
// is formed before `inside` holds, that is 0 <= g_a <= n_a - 1 on every axis (a
// NaN fails both comparisons).  Then fl_a = min(floor(g_a), n_a - 2) is an
// integer in [0, n_a - 2] (the host checks n_a >= 2), so c_a <= n_a - 2 and the
// cell's far corner c_a + 1 <= n_a - 1 is a lattice point; its linear index is
// at most nx*ny*nz - 1, and the host checks nx*ny*nz <= 2^31 - 1, so the uint32
// products do not wrap.  A lane with i >= n, or outside the lattice, loads
// nothing, holds +0.0 for all 29 terms and still reaches the one barrier.
struct TsdfLattice {
  uint32_t n[3];
  float o[3], h[3];
};

__device__ __forceinline__ float ti_lerp(float x, float y, float f) { return x + f * (y - x); }

__global__ void __launch_bounds__(PG_THREADS) k_tsdf_icp_sums(const float* __restrict__ tsdf,
                                                              const float* __restrict__ weight,
                                                              TsdfLattice L,
                                                              const float* __restrict__ points,
                                                              uint32_t n, Rigid T, float trunc,
                                                              float min_weight, float max_tsdf,
                                                              double* __restrict__ out,
                                                              float* __restrict__ value,
                                                              uint8_t* __restrict__ match) {
  __shared__ double sh[ICP_SUMS * 4u];
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;  // < 2^31 + 256
  const bool live = i < n;
  float q[3] = {NAN, NAN, NAN};
  if (live) {
    const float x = points[3ull * i], y = points[3ull * i + 1u], z = points[3ull * i + 2u];
    q[0] = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
    q[1] = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
    q[2] = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
  }
  float g[3];
  bool inside = live;
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
    const uint32_t sj = L.n[2], si = L.n[1] * L.n[2];
    const uint32_t base = (c[0] * L.n[1] + c[1]) * L.n[2] + c[2];
    // v[4i + 2j + k]: both arrays, all sixteen loads before the first use
#pragma unroll
    for (uint32_t c8 = 0; c8 < 8u; ++c8) {
      const uint32_t at = base + ((c8 & 4u) ? si : 0u) + ((c8 & 2u) ? sj : 0u) + (c8 & 1u);
      w[c8] = weight[at];
      v[c8] = tsdf[at];
    }
  }
  bool observed = inside;
#pragma unroll
  for (int c = 0; c < 8; ++c) observed = observed && w[c] >= min_weight;
  const float c00 = ti_lerp(v[0], v[1], f[2]), c01 = ti_lerp(v[2], v[3], f[2]);
  const float c10 = ti_lerp(v[4], v[5], f[2]), c11 = ti_lerp(v[6], v[7], f[2]);
  const float c_0 = ti_lerp(c00, c01, f[1]), c_1 = ti_lerp(c10, c11, f[1]);
  const float F = ti_lerp(c_0, c_1, f[0]);
  float G[3];
  G[0] = c_1 - c_0;
  G[1] = ti_lerp(c01 - c00, c11 - c10, f[0]);
  G[2] = ti_lerp(ti_lerp(v[1] - v[0], v[3] - v[2], f[1]), ti_lerp(v[5] - v[4], v[7] - v[6], f[1]),
                 f[0]);
#pragma unroll
  for (int a = 0; a < 3; ++a) G[a] = G[a] / L.h[a];
  const float ln = sqrtf((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
  const bool matched = observed && ln > 0.0f && isfinite(ln) && fabsf(F) <= max_tsdf;
  if (live) {
    if (value) value[i] = observed ? F : NAN;
    if (match) match[i] = matched ? 1 : 0;
  }
  float V[8][1];  // J (0..5), r (6) and 1 (7); unused bits of an unmatched row are selected away
  icp_row<1>(q[0], q[1], q[2], 0.0f, 0.0f, 0.0f, G[0] / ln, G[1] / ln, G[2] / ln, V, 0);
  V[6][0] = -(F * trunc);
  uint32_t col = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = a; b < 6; ++b) icp_put(icp_term<1>(matched, V[a], V[b]), col++, sh);
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) icp_put(icp_term<1>(matched, V[a], V[6]), col++, sh);
  icp_put(icp_term<1>(matched, V[6], V[6]), col++, sh);
  icp_put(icp_term<1>(matched, V[7], V[7]), col++, sh);
  icp_finish(sh, out);
}

// ---- the same step for K transforms in one launch: ucsa_tsdf_icp_sums_batch ----
// k_tsdf_icp_sums_batch  shaped like k_tsdf_score (tsdf_score.hip): a lane per
//                  point in work-groups of 256 points (blockIdx.y), a tile of
//                  TB_TILE transforms per work-group (blockIdx.x).  The point is
//                  loaded once.  The loop over the tile is uniform, and so is the
//                  address of a transform's twelve floats: they arrive as scalar
//                  loads.  Per transform the body is k_tsdf_icp_sums' (restated
//                  here: that kernel is not touched): the move, the cell, the
//                  sixteen floats gathered before their first use (as eight
//                  8-byte loads, the corners k = 0, 1 being neighbours in memory,
//                  as in k_tsdf_score), F, the gradient, the row, and the 29
//                  terms through icp_put into the transform's own [29][4] of
//                  LDS.  Behind the one barrier a lane per (transform, sum) adds
//                  the four waves as (w0 + w1) + (w2 + w3) and writes the sum to
//                  row (transform, work-group) of the stage's output.
// k_icp_reduce_batch  k_icp_reduce with the transform on blockIdx.y; k_icp_reduce
//                  itself is as it was.
//
// A stage's output is [K][count][29], count its work-groups along the points; the
// stages follow one another in the workspace as in ucsa_tsdf_icp_sums, each K
// times as large, and the last (count == 1) is `sums` [K][29].
//
// No atomics: the same operands meet in the same tree as in the single call, so a
// row holds the same bits.  The barrier is reached by every lane: the loop's trip
// count comes from blockIdx.x and K alone, a lane with i >= n holds a NaN point
// (outside every lattice) and nothing returns early.
//
// Why every index is in range: as in k_tsdf_icp_sums, no float is converted to
// an integer and no index is formed before `inside` holds, that is
// 0 <= g_a <= n_a - 1 on every axis (a NaN fails both comparisons).  Then
// fl_a = min(floor(g_a), n_a - 2) is an integer in [0, n_a - 2] (the host checks
// n_a >= 2), the cell's far corner is a lattice point and its linear index is at
// most nx*ny*nz - 1 <= 2^31 - 2, so the uint32 products do not wrap; an 8-byte
// load at a corner with k = 0 ends with the corner at k = 1, inside the array.
// A transform's index first + t is below K by the loop's bound (the host sizes
// the grid so that first < K); a point's index is below n before it is read; a
// row (k, group) with k < K and group < count is below K * count, which the host
// checks against the workspace.
constexpr uint32_t TB_TILE = UCSA_TSDF_ICP_BATCH_TILE;  // transforms per work-group

__global__ void __launch_bounds__(PG_THREADS) k_tsdf_icp_sums_batch(
    const float* __restrict__ tsdf, const float* __restrict__ weight, TsdfLattice L,
    const float* __restrict__ points, uint32_t n, const float* __restrict__ transforms, uint32_t K,
    float trunc, float min_weight, float max_tsdf, double* __restrict__ out) {
  __shared__ double sh[TB_TILE * ICP_SUMS * 4u];            // [transform][sum][wave]
  const uint32_t i = blockIdx.y * PG_THREADS + threadIdx.x;  // < 2^23 + 256
  float x = NAN, y = NAN, z = NAN;  // no point: outside every lattice
  if (i < n) {
    x = points[3ull * i];
    y = points[3ull * i + 1u];
    z = points[3ull * i + 2u];
  }
  const uint32_t first = blockIdx.x * TB_TILE;  // < K: the host sizes the grid
  const uint32_t count = K - first < TB_TILE ? K - first : TB_TILE;
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
      // v[4i + 2j + k]: both arrays, all eight 8-byte loads before the first use
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
    const float c00 = ti_lerp(v[0], v[1], f[2]), c01 = ti_lerp(v[2], v[3], f[2]);
    const float c10 = ti_lerp(v[4], v[5], f[2]), c11 = ti_lerp(v[6], v[7], f[2]);
    const float c_0 = ti_lerp(c00, c01, f[1]), c_1 = ti_lerp(c10, c11, f[1]);
    const float F = ti_lerp(c_0, c_1, f[0]);
    float G[3];
    G[0] = c_1 - c_0;
    G[1] = ti_lerp(c01 - c00, c11 - c10, f[0]);
    G[2] = ti_lerp(ti_lerp(v[1] - v[0], v[3] - v[2], f[1]), ti_lerp(v[5] - v[4], v[7] - v[6], f[1]),
                   f[0]);
#pragma unroll
    for (int a = 0; a < 3; ++a) G[a] = G[a] / L.h[a];
    const float ln = sqrtf((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
    const bool matched = observed && ln > 0.0f && isfinite(ln) && fabsf(F) <= max_tsdf;
    float V[8][1];  // J (0..5), r (6) and 1 (7); unused bits of an unmatched row are selected away
    icp_row<1>(q[0], q[1], q[2], 0.0f, 0.0f, 0.0f, G[0] / ln, G[1] / ln, G[2] / ln, V, 0);
    V[6][0] = -(F * trunc);
    double* row = sh + t * (ICP_SUMS * 4u);
    uint32_t col = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = a; b < 6; ++b) icp_put(icp_term<1>(matched, V[a], V[b]), col++, row);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) icp_put(icp_term<1>(matched, V[a], V[6]), col++, row);
    icp_put(icp_term<1>(matched, V[6], V[6]), col++, row);
    icp_put(icp_term<1>(matched, V[7], V[7]), col++, row);
  }
  __syncthreads();
  const uint32_t c = threadIdx.x;  // (transform c / 29, sum c % 29)
  if (c < count * ICP_SUMS) {
    const uint32_t t = c / ICP_SUMS, s = c - t * ICP_SUMS;
    const double* p = sh + 4u * c;
    out[((uint64_t)(first + t) * gridDim.y + blockIdx.y) * ICP_SUMS + s] =
        (p[0] + p[1]) + (p[2] + p[3]);
  }
}

// stage `in` [K][count][29] -> `out` [K][gridDim.x][29]; blockIdx.y is the transform
__global__ void __launch_bounds__(PG_THREADS) k_icp_reduce_batch(const double* __restrict__ in,
                                                                 uint32_t count,
                                                                 double* __restrict__ out) {
  __shared__ double sh[ICP_SUMS * 4u];
  const uint32_t row = blockIdx.x * PG_THREADS + threadIdx.x;
  const bool live = row < count;
  const double* mine = in + (uint64_t)blockIdx.y * count * ICP_SUMS;
#pragma unroll 1
  for (uint32_t c = 0; c < ICP_SUMS; ++c)
    icp_put(live ? mine[(uint64_t)row * ICP_SUMS + c] : 0.0, c, sh);
  __syncthreads();
  const uint32_t c = threadIdx.x;
  if (c < ICP_SUMS)
    out[((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * ICP_SUMS + c] =
        (sh[4u * c] + sh[4u * c + 1u]) + (sh[4u * c + 2u] + sh[4u * c + 3u]);
}

// ---- one step of projective ICP against a pair of maps: ucsa_projective_icp_sums ----
// k_projective_icp_sums  a lane per point in work-groups of 256: the point (and
//                  its normal) is moved by [R | t], projected into the target
//                  camera with ucsa_tsdf_integrate's expression, and the target's
//                  point, normal and mask at that pixel are gathered (seven loads
//                  issued together).  The gates (mask, finite, distance, normal
//                  compatibility) follow, then r = nt . (c - q), J = (q x nt, nt)
//                  and the 29 terms, reduced as in k_icp_sums: icp_put /
//                  icp_finish, then k_icp_reduce on the group results.
//
// Why every index is in range: no float is converted to an integer and no index
// is formed before `inside` holds, that is q2 > 0 and 0 <= u < (float)W and
// 0 <= v < (float)H for the floored u, v (a NaN fails every comparison).  u and
// v are then integers in [0, W - 1] and [0, H - 1]; the host checks H, W <=
// 16384, so v*W + u <= 2^28 - 1 and the uint32 product does not wrap.  A lane
// with i >= n, or without a pixel, loads nothing from the maps, holds +0.0 for
// all 29 terms and still reaches the one barrier.
struct ProjTarget {
  const float* points;
  const float* normals;
  const uint8_t* mask;
  uint32_t H, W, reject;
  float fx, fy, cx, cy;
};

__global__ void __launch_bounds__(PG_THREADS) k_projective_icp_sums(
    const float* __restrict__ points, const float* __restrict__ normals, uint32_t n, ProjTarget G,
    Rigid T, float limit2, float min_cos, double* __restrict__ out, int32_t* __restrict__ pixel,
    float* __restrict__ residual) {
  __shared__ double sh[ICP_SUMS * 4u];
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;  // < 2^31 + 256
  const bool live = i < n;
  float q[3] = {NAN, NAN, NAN}, m[3] = {0.0f, 0.0f, 0.0f};
  if (live) {
    const float x = points[3ull * i], y = points[3ull * i + 1u], z = points[3ull * i + 2u];
    q[0] = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
    q[1] = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
    q[2] = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
    if (normals) {
      const float s0 = normals[3ull * i], s1 = normals[3ull * i + 1u], s2 = normals[3ull * i + 2u];
      m[0] = (T.m[0] * s0 + T.m[1] * s1) + T.m[2] * s2;
      m[1] = (T.m[4] * s0 + T.m[5] * s1) + T.m[6] * s2;
      m[2] = (T.m[8] * s0 + T.m[9] * s1) + T.m[10] * s2;
    }
  }
  bool inside = live && q[2] > 0.0f;
  float u = 0.0f, v = 0.0f;
  if (inside) {
    u = floorf((G.fx * q[0]) / q[2] + G.cx);
    v = floorf((G.fy * q[1]) / q[2] + G.cy);
    inside = u >= 0.0f && u < (float)G.W && v >= 0.0f && v < (float)G.H;
  }
  float c[3] = {0.0f, 0.0f, 0.0f}, nt[3] = {0.0f, 0.0f, 0.0f};
  uint32_t mk = 0u, pix = 0u;
  if (inside) {
    pix = (uint32_t)v * G.W + (uint32_t)u;
    // all seven loads before the first use
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      c[a] = G.points[3ull * pix + a];
      nt[a] = G.normals[3ull * pix + a];
    }
    mk = G.mask[pix];
  }
  bool matched = inside && (mk & UCSA_DEPTH_NORMAL) != 0u && (mk & G.reject) == 0u;
#pragma unroll
  for (int a = 0; a < 3; ++a) matched = matched && isfinite(c[a]) && isfinite(nt[a]);
  float d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) d[a] = c[a] - q[a];
  const float dist2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  matched = matched && dist2 <= limit2;
  if (normals) matched = matched && (m[0] * nt[0] + m[1] * nt[1]) + m[2] * nt[2] >= min_cos;
  float V[8][1];  // J (0..5), r (6) and 1 (7); unused bits of an unmatched row are selected away
  icp_row<1>(q[0], q[1], q[2], d[0], d[1], d[2], nt[0], nt[1], nt[2], V, 0);
  if (live) {
    if (pixel) pixel[i] = matched ? (int32_t)pix : -1;
    if (residual) residual[i] = matched ? V[6][0] : NAN;
  }
  uint32_t col = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = a; b < 6; ++b) icp_put(icp_term<1>(matched, V[a], V[b]), col++, sh);
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) icp_put(icp_term<1>(matched, V[a], V[6]), col++, sh);
  icp_put(icp_term<1>(matched, V[6], V[6]), col++, sh);
  icp_put(icp_term<1>(matched, V[7], V[7]), col++, sh);
  icp_finish(sh, out);
}

// ---- the two frame trackers' steps with a weight per row: iteratively reweighted
// least squares (ucsa_projective_icp_sums_weighted, ucsa_tsdf_icp_sums_weighted) ----
// k_projective_icp_sums_weighted, k_tsdf_icp_sums_weighted
//                  the bodies of k_projective_icp_sums and k_tsdf_icp_sums up to
//                  the gates and the row (J, r), restated here operand for
//                  operand (those kernels are not touched), then the row's
//                  weight w = p * rho(|r|) in float32 (icp_robust_weight), the
//                  row scaled by sqrtf(w), and the 29 terms through icp_term /
//                  icp_put / icp_finish as they are.  A product by sqrt(w) = 1
//                  is exact, so without weights the sums are the siblings' bits;
//                  slot 27 is sum w r^2 and slot 28 the rows with w > 0.
//
// The point's weight is loaded with the point, before the gathers: it is on no
// dependent path.  A lane with i >= n loads nothing, holds +0.0 for all 29 terms
// and still reaches the one barrier; no index is formed before `inside` holds,
// exactly as in the siblings (their range arguments apply word for word: the
// indices are the same expressions).  weight_out[i] is the lane's own slot.
// No atomics.
struct RobustArgs {
  const float* point_weight;  // [n] or NULL: 1
  float* weight_out;          // [n] or NULL
  int32_t kind;               // UCSA_ROBUST_NONE / HUBER / TUKEY
  float scale;                // k or c, in the residual's units
};

// w = p * rho(|r|): each operation rounded once.  p that is not finite and > 0
// gives 0: the row takes no part (ucsa_tsdf_integrate_weighted's rule for a pixel).
__device__ __forceinline__ float icp_robust_weight(float r, float p, int32_t kind, float scale) {
  const float a = fabsf(r);
  float rho = 1.0f;
  if (kind == UCSA_ROBUST_HUBER) {
    rho = a <= scale ? 1.0f : scale / a;
  } else if (kind == UCSA_ROBUST_TUKEY) {
    const float t = a / scale;
    const float u = 1.0f - t * t;
    rho = a < scale ? u * u : 0.0f;
  }
  const bool usable = p > 0.0f && isfinite(p);
  return usable ? p * rho : 0.0f;
}

// scale the row by sqrt(w), report the weight and reduce the 29 terms
__device__ __forceinline__ void icp_weighted_finish(bool matched, bool live, uint32_t i, float p,
                                                    const RobustArgs& Q, float (*V)[1], double* sh,
                                                    double* __restrict__ out) {
  const float w = icp_robust_weight(V[6][0], p, Q.kind, Q.scale);
  const bool counts = matched && w > 0.0f;
  if (live && Q.weight_out) Q.weight_out[i] = counts ? w : 0.0f;
  const float s = sqrtf(w);
#pragma unroll
  for (int a = 0; a < 7; ++a) V[a][0] = s * V[a][0];
  uint32_t col = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = a; b < 6; ++b) icp_put(icp_term<1>(counts, V[a], V[b]), col++, sh);
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) icp_put(icp_term<1>(counts, V[a], V[6]), col++, sh);
  icp_put(icp_term<1>(counts, V[6], V[6]), col++, sh);
  icp_put(icp_term<1>(counts, V[7], V[7]), col++, sh);
  icp_finish(sh, out);
}

__global__ void __launch_bounds__(PG_THREADS) k_tsdf_icp_sums_weighted(
    const float* __restrict__ tsdf, const float* __restrict__ weight, TsdfLattice L,
    const float* __restrict__ points, uint32_t n, Rigid T, float trunc, float min_weight,
    float max_tsdf, RobustArgs Q, double* __restrict__ out, float* __restrict__ value,
    uint8_t* __restrict__ match) {
  __shared__ double sh[ICP_SUMS * 4u];
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;  // < 2^31 + 256
  const bool live = i < n;
  float q[3] = {NAN, NAN, NAN};
  float p = 0.0f;
  if (live) {
    const float x = points[3ull * i], y = points[3ull * i + 1u], z = points[3ull * i + 2u];
    p = Q.point_weight ? Q.point_weight[i] : 1.0f;
    q[0] = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
    q[1] = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
    q[2] = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
  }
  float g[3];
  bool inside = live;
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
    const uint32_t sj = L.n[2], si = L.n[1] * L.n[2];
    const uint32_t base = (c[0] * L.n[1] + c[1]) * L.n[2] + c[2];
    // v[4i + 2j + k]: both arrays, all sixteen loads before the first use
#pragma unroll
    for (uint32_t c8 = 0; c8 < 8u; ++c8) {
      const uint32_t at = base + ((c8 & 4u) ? si : 0u) + ((c8 & 2u) ? sj : 0u) + (c8 & 1u);
      w[c8] = weight[at];
      v[c8] = tsdf[at];
    }
  }
  bool observed = inside;
#pragma unroll
  for (int c = 0; c < 8; ++c) observed = observed && w[c] >= min_weight;
  const float c00 = ti_lerp(v[0], v[1], f[2]), c01 = ti_lerp(v[2], v[3], f[2]);
  const float c10 = ti_lerp(v[4], v[5], f[2]), c11 = ti_lerp(v[6], v[7], f[2]);
  const float c_0 = ti_lerp(c00, c01, f[1]), c_1 = ti_lerp(c10, c11, f[1]);
  const float F = ti_lerp(c_0, c_1, f[0]);
  float G[3];
  G[0] = c_1 - c_0;
  G[1] = ti_lerp(c01 - c00, c11 - c10, f[0]);
  G[2] = ti_lerp(ti_lerp(v[1] - v[0], v[3] - v[2], f[1]), ti_lerp(v[5] - v[4], v[7] - v[6], f[1]),
                 f[0]);
#pragma unroll
  for (int a = 0; a < 3; ++a) G[a] = G[a] / L.h[a];
  const float ln = sqrtf((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
  const bool matched = observed && ln > 0.0f && isfinite(ln) && fabsf(F) <= max_tsdf;
  if (live) {
    if (value) value[i] = observed ? F : NAN;
    if (match) match[i] = matched ? 1 : 0;
  }
  float V[8][1];  // J (0..5), r (6) and 1 (7); unused bits of an unmatched row are selected away
  icp_row<1>(q[0], q[1], q[2], 0.0f, 0.0f, 0.0f, G[0] / ln, G[1] / ln, G[2] / ln, V, 0);
  V[6][0] = -(F * trunc);
  icp_weighted_finish(matched, live, i, p, Q, V, sh, out);
}

__global__ void __launch_bounds__(PG_THREADS) k_projective_icp_sums_weighted(
    const float* __restrict__ points, const float* __restrict__ normals, uint32_t n, ProjTarget G,
    Rigid T, float limit2, float min_cos, RobustArgs Q, double* __restrict__ out,
    int32_t* __restrict__ pixel, float* __restrict__ residual) {
  __shared__ double sh[ICP_SUMS * 4u];
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;  // < 2^31 + 256
  const bool live = i < n;
  float q[3] = {NAN, NAN, NAN}, m[3] = {0.0f, 0.0f, 0.0f};
  float p = 0.0f;
  if (live) {
    const float x = points[3ull * i], y = points[3ull * i + 1u], z = points[3ull * i + 2u];
    p = Q.point_weight ? Q.point_weight[i] : 1.0f;
    q[0] = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
    q[1] = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
    q[2] = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
    if (normals) {
      const float s0 = normals[3ull * i], s1 = normals[3ull * i + 1u], s2 = normals[3ull * i + 2u];
      m[0] = (T.m[0] * s0 + T.m[1] * s1) + T.m[2] * s2;
      m[1] = (T.m[4] * s0 + T.m[5] * s1) + T.m[6] * s2;
      m[2] = (T.m[8] * s0 + T.m[9] * s1) + T.m[10] * s2;
    }
  }
  bool inside = live && q[2] > 0.0f;
  float u = 0.0f, v = 0.0f;
  if (inside) {
    u = floorf((G.fx * q[0]) / q[2] + G.cx);
    v = floorf((G.fy * q[1]) / q[2] + G.cy);
    inside = u >= 0.0f && u < (float)G.W && v >= 0.0f && v < (float)G.H;
  }
  float c[3] = {0.0f, 0.0f, 0.0f}, nt[3] = {0.0f, 0.0f, 0.0f};
  uint32_t mk = 0u, pix = 0u;
  if (inside) {
    pix = (uint32_t)v * G.W + (uint32_t)u;
    // all seven loads before the first use
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      c[a] = G.points[3ull * pix + a];
      nt[a] = G.normals[3ull * pix + a];
    }
    mk = G.mask[pix];
  }
  bool matched = inside && (mk & UCSA_DEPTH_NORMAL) != 0u && (mk & G.reject) == 0u;
#pragma unroll
  for (int a = 0; a < 3; ++a) matched = matched && isfinite(c[a]) && isfinite(nt[a]);
  float d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) d[a] = c[a] - q[a];
  const float dist2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  matched = matched && dist2 <= limit2;
  if (normals) matched = matched && (m[0] * nt[0] + m[1] * nt[1]) + m[2] * nt[2] >= min_cos;
  float V[8][1];  // J (0..5), r (6) and 1 (7); unused bits of an unmatched row are selected away
  icp_row<1>(q[0], q[1], q[2], d[0], d[1], d[2], nt[0], nt[1], nt[2], V, 0);
  if (live) {
    if (pixel) pixel[i] = matched ? (int32_t)pix : -1;
    if (residual) residual[i] = matched ? V[6][0] : NAN;  // the unscaled r
  }
  icp_weighted_finish(matched, live, i, p, Q, V, sh, out);
}

// the robust arguments' checks, shared by the two entry points: 0, or 1 (kind), 2 (scale)
int icp_robust_args(int32_t kind, float scale) {
  if (kind != UCSA_ROBUST_NONE && kind != UCSA_ROBUST_HUBER && kind != UCSA_ROBUST_TUKEY) return 1;
  if (kind != UCSA_ROBUST_NONE && !(scale > 0.0f && pg_host_finite(scale))) return 2;
  return 0;
}

}  // namespace

extern "C" int32_t ucsa_projective_icp_sums_weighted(
    const float* points, const float* normals, uint32_t n, const float* target_points,
    const float* target_normals, const uint8_t* target_mask, uint32_t H, uint32_t W,
    uint32_t reject, float fx, float fy, float cx, float cy, const float* transform,
    float max_dist, float min_cos, const float* point_weight, int32_t robust_kind,
    float robust_scale, double* workspace, uint64_t workspace_doubles, double* sums,
    int32_t* pixel, float* residual, float* weight_out, void* stream) {
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFu, 2);
  UCSA_CHECK_ARG(n == 0 || points, 0);
  UCSA_CHECK_ARG(target_points, 3);
  UCSA_CHECK_ARG(target_normals, 4);
  UCSA_CHECK_ARG(target_mask, 5);
  UCSA_CHECK_ARG(H >= 1 && H <= 16384, 6);
  UCSA_CHECK_ARG(W >= 1 && W <= 16384, 7);
  UCSA_CHECK_ARG((reject & ~(UCSA_DEPTH_EDGE | UCSA_DEPTH_GRAZING)) == 0u, 8);
  UCSA_CHECK_ARG(fx > 0.0f && pg_host_finite(fx), 9);
  UCSA_CHECK_ARG(fy > 0.0f && pg_host_finite(fy), 10);
  UCSA_CHECK_ARG(pg_host_finite(cx), 11);
  UCSA_CHECK_ARG(pg_host_finite(cy), 12);
  UCSA_CHECK_ARG(transform, 13);
  const float limit2 = max_dist * max_dist;
  UCSA_CHECK_ARG(max_dist > 0.0f && pg_host_finite(max_dist) && pg_host_finite(limit2), 14);
  UCSA_CHECK_ARG(min_cos >= -1.0f && min_cos <= 1.0f, 15);
  const int bad = icp_robust_args(robust_kind, robust_scale);
  UCSA_CHECK_ARG(bad != 1, 17);
  UCSA_CHECK_ARG(bad != 2, 18);
  const uint64_t ws_rows = icp_workspace_rows(n);
  UCSA_CHECK_ARG(ws_rows == 0 || workspace, 19);
  UCSA_CHECK_ARG(workspace_doubles >= ws_rows * ICP_SUMS, 20);
  UCSA_CHECK_ARG(sums, 21);
  ProjTarget G;
  G.points = target_points, G.normals = target_normals, G.mask = target_mask;
  G.H = H, G.W = W, G.reject = reject;
  G.fx = fx, G.fy = fy, G.cx = cx, G.cy = cy;
  Rigid T;
  for (int k = 0; k < 12; ++k) T.m[k] = transform[k];
  RobustArgs Q;
  Q.point_weight = point_weight, Q.weight_out = weight_out;
  Q.kind = robust_kind, Q.scale = robust_kind == UCSA_ROBUST_NONE ? 1.0f : robust_scale;
  hipStream_t s = (hipStream_t)stream;
  uint32_t count = n ? ucsa_div_up(n, PG_THREADS) : 1u;  // at least one stage: n == 0 gives +0.0
  double* out = count == 1u ? sums : workspace;
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_projective_icp_sums_weighted, dim3(count), dim3(PG_THREADS), 0, s, points,
                     normals, n, G, T, limit2, min_cos, Q, out, pixel, residual);
  while (count > 1u) {  // as in ucsa_icp_sums: at most three passes for n < 2^31
    const uint32_t next = ucsa_div_up(count, PG_THREADS);
    const double* in = out;
    out = next == 1u ? sums : out + (uint64_t)count * ICP_SUMS;
    hipLaunchKernelGGL(k_icp_reduce, dim3(next), dim3(PG_THREADS), 0, s, in, count, out);
    count = next;
  }
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_tsdf_icp_sums_weighted(
    const float* tsdf, const float* weight, uint32_t nx, uint32_t ny, uint32_t nz,
    const float* origin3, const float* spacing3, const float* points, uint32_t n,
    const float* transform, float trunc, float min_weight, float max_tsdf,
    const float* point_weight, int32_t robust_kind, float robust_scale, double* workspace,
    uint64_t workspace_doubles, double* sums, float* value, uint8_t* matched, float* weight_out,
    void* stream) {
  UCSA_CHECK_ARG(tsdf, 0);
  UCSA_CHECK_ARG(weight, 1);
  UCSA_CHECK_ARG(nx >= 2 && ny >= 1 && nz >= 1 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 2);
  UCSA_CHECK_ARG(ny >= 2, 3);
  UCSA_CHECK_ARG(nz >= 2, 4);
  UCSA_CHECK_ARG(origin3 && pg_host_finite(origin3[0]) && pg_host_finite(origin3[1]) &&
                     pg_host_finite(origin3[2]), 5);
  UCSA_CHECK_ARG(spacing3, 6);
  for (int a = 0; a < 3; ++a) UCSA_CHECK_ARG(spacing3[a] > 0.0f && pg_host_finite(spacing3[a]), 6);
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFu, 8);
  UCSA_CHECK_ARG(n == 0 || points, 7);
  UCSA_CHECK_ARG(transform, 9);
  UCSA_CHECK_ARG(trunc > 0.0f && pg_host_finite(trunc), 10);
  UCSA_CHECK_ARG(min_weight > 0.0f, 11);
  UCSA_CHECK_ARG(max_tsdf > 0.0f && max_tsdf <= 1.0f, 12);
  const int bad = icp_robust_args(robust_kind, robust_scale);
  UCSA_CHECK_ARG(bad != 1, 14);
  UCSA_CHECK_ARG(bad != 2, 15);
  const uint64_t ws_rows = icp_workspace_rows(n);
  UCSA_CHECK_ARG(ws_rows == 0 || workspace, 16);
  UCSA_CHECK_ARG(workspace_doubles >= ws_rows * ICP_SUMS, 17);
  UCSA_CHECK_ARG(sums, 18);
  TsdfLattice L;
  L.n[0] = nx, L.n[1] = ny, L.n[2] = nz;
  for (int a = 0; a < 3; ++a) L.o[a] = origin3[a], L.h[a] = spacing3[a];
  Rigid T;
  for (int k = 0; k < 12; ++k) T.m[k] = transform[k];
  RobustArgs Q;
  Q.point_weight = point_weight, Q.weight_out = weight_out;
  Q.kind = robust_kind, Q.scale = robust_kind == UCSA_ROBUST_NONE ? 1.0f : robust_scale;
  hipStream_t s = (hipStream_t)stream;
  uint32_t count = n ? ucsa_div_up(n, PG_THREADS) : 1u;  // at least one stage: n == 0 gives +0.0
  double* out = count == 1u ? sums : workspace;
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_tsdf_icp_sums_weighted, dim3(count), dim3(PG_THREADS), 0, s, tsdf, weight, L,
                     points, n, T, trunc, min_weight, max_tsdf, Q, out, value, matched);
  while (count > 1u) {  // as in ucsa_icp_sums: at most three passes for n < 2^31
    const uint32_t next = ucsa_div_up(count, PG_THREADS);
    const double* in = out;
    out = next == 1u ? sums : out + (uint64_t)count * ICP_SUMS;
    hipLaunchKernelGGL(k_icp_reduce, dim3(next), dim3(PG_THREADS), 0, s, in, count, out);
    count = next;
  }
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_projective_icp_sums(const float* points, const float* normals, uint32_t n,
                                            const float* target_points,
                                            const float* target_normals,
                                            const uint8_t* target_mask, uint32_t H, uint32_t W,
                                            uint32_t reject, float fx, float fy, float cx, float cy,
                                            const float* transform, float max_dist, float min_cos,
                                            double* workspace, uint64_t workspace_doubles,
                                            double* sums, int32_t* pixel, float* residual,
                                            void* stream) {
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFu, 2);
  UCSA_CHECK_ARG(n == 0 || points, 0);
  UCSA_CHECK_ARG(target_points, 3);
  UCSA_CHECK_ARG(target_normals, 4);
  UCSA_CHECK_ARG(target_mask, 5);
  UCSA_CHECK_ARG(H >= 1 && H <= 16384, 6);
  UCSA_CHECK_ARG(W >= 1 && W <= 16384, 7);
  UCSA_CHECK_ARG((reject & ~(UCSA_DEPTH_EDGE | UCSA_DEPTH_GRAZING)) == 0u, 8);
  UCSA_CHECK_ARG(fx > 0.0f && pg_host_finite(fx), 9);
  UCSA_CHECK_ARG(fy > 0.0f && pg_host_finite(fy), 10);
  UCSA_CHECK_ARG(pg_host_finite(cx), 11);
  UCSA_CHECK_ARG(pg_host_finite(cy), 12);
  UCSA_CHECK_ARG(transform, 13);
  const float limit2 = max_dist * max_dist;
  UCSA_CHECK_ARG(max_dist > 0.0f && pg_host_finite(max_dist) && pg_host_finite(limit2), 14);
  UCSA_CHECK_ARG(min_cos >= -1.0f && min_cos <= 1.0f, 15);
  const uint64_t ws_rows = icp_workspace_rows(n);
  UCSA_CHECK_ARG(ws_rows == 0 || workspace, 16);
  UCSA_CHECK_ARG(workspace_doubles >= ws_rows * ICP_SUMS, 17);
  UCSA_CHECK_ARG(sums, 18);
  ProjTarget G;
  G.points = target_points, G.normals = target_normals, G.mask = target_mask;
  G.H = H, G.W = W, G.reject = reject;
  G.fx = fx, G.fy = fy, G.cx = cx, G.cy = cy;
  Rigid T;
  for (int k = 0; k < 12; ++k) T.m[k] = transform[k];
  hipStream_t s = (hipStream_t)stream;
  uint32_t count = n ? ucsa_div_up(n, PG_THREADS) : 1u;  // at least one stage: n == 0 gives +0.0
  double* out = count == 1u ? sums : workspace;
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_projective_icp_sums, dim3(count), dim3(PG_THREADS), 0, s, points, normals, n,
                     G, T, limit2, min_cos, out, pixel, residual);
  while (count > 1u) {  // as in ucsa_icp_sums: at most three passes for n < 2^31
    const uint32_t next = ucsa_div_up(count, PG_THREADS);
    const double* in = out;
    out = next == 1u ? sums : out + (uint64_t)count * ICP_SUMS;
    hipLaunchKernelGGL(k_icp_reduce, dim3(next), dim3(PG_THREADS), 0, s, in, count, out);
    count = next;
  }
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_tsdf_icp_sums(const float* tsdf, const float* weight, uint32_t nx,
                                      uint32_t ny, uint32_t nz, const float* origin3,
                                      const float* spacing3, const float* points, uint32_t n,
                                      const float* transform, float trunc, float min_weight,
                                      float max_tsdf, double* workspace,
                                      uint64_t workspace_doubles, double* sums, float* value,
                                      uint8_t* matched, void* stream) {
  UCSA_CHECK_ARG(tsdf, 0);
  UCSA_CHECK_ARG(weight, 1);
  UCSA_CHECK_ARG(nx >= 2 && ny >= 1 && nz >= 1 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 2);
  UCSA_CHECK_ARG(ny >= 2, 3);
  UCSA_CHECK_ARG(nz >= 2, 4);
  UCSA_CHECK_ARG(origin3 && pg_host_finite(origin3[0]) && pg_host_finite(origin3[1]) &&
                     pg_host_finite(origin3[2]), 5);
  UCSA_CHECK_ARG(spacing3, 6);
  for (int a = 0; a < 3; ++a) UCSA_CHECK_ARG(spacing3[a] > 0.0f && pg_host_finite(spacing3[a]), 6);
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFu, 8);
  UCSA_CHECK_ARG(n == 0 || points, 7);
  UCSA_CHECK_ARG(transform, 9);
  UCSA_CHECK_ARG(trunc > 0.0f && pg_host_finite(trunc), 10);
  UCSA_CHECK_ARG(min_weight > 0.0f, 11);
  UCSA_CHECK_ARG(max_tsdf > 0.0f && max_tsdf <= 1.0f, 12);
  const uint64_t ws_rows = icp_workspace_rows(n);
  UCSA_CHECK_ARG(ws_rows == 0 || workspace, 13);
  UCSA_CHECK_ARG(workspace_doubles >= ws_rows * ICP_SUMS, 14);
  UCSA_CHECK_ARG(sums, 15);
  TsdfLattice L;
  L.n[0] = nx, L.n[1] = ny, L.n[2] = nz;
  for (int a = 0; a < 3; ++a) L.o[a] = origin3[a], L.h[a] = spacing3[a];
  Rigid T;
  for (int k = 0; k < 12; ++k) T.m[k] = transform[k];
  hipStream_t s = (hipStream_t)stream;
  uint32_t count = n ? ucsa_div_up(n, PG_THREADS) : 1u;  // at least one stage: n == 0 gives +0.0
  double* out = count == 1u ? sums : workspace;
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_tsdf_icp_sums, dim3(count), dim3(PG_THREADS), 0, s, tsdf, weight, L, points,
                     n, T, trunc, min_weight, max_tsdf, out, value, matched);
  while (count > 1u) {  // as in ucsa_icp_sums: at most three passes for n < 2^31
    const uint32_t next = ucsa_div_up(count, PG_THREADS);
    const double* in = out;
    out = next == 1u ? sums : out + (uint64_t)count * ICP_SUMS;
    hipLaunchKernelGGL(k_icp_reduce, dim3(next), dim3(PG_THREADS), 0, s, in, count, out);
    count = next;
  }
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_tsdf_icp_sums_batch(const float* tsdf, const float* weight, uint32_t nx,
                                            uint32_t ny, uint32_t nz, const float* origin3,
                                            const float* spacing3, const float* points, uint32_t n,
                                            const float* transforms, uint32_t K, float trunc,
                                            float min_weight, float max_tsdf, double* workspace,
                                            uint64_t workspace_doubles, double* sums,
                                            void* stream) {
  UCSA_CHECK_ARG(tsdf, 0);
  UCSA_CHECK_ARG(weight, 1);
  UCSA_CHECK_ARG(nx >= 2 && ny >= 1 && nz >= 1 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 2);
  UCSA_CHECK_ARG(ny >= 2, 3);
  UCSA_CHECK_ARG(nz >= 2, 4);
  UCSA_CHECK_ARG(origin3 && pg_host_finite(origin3[0]) && pg_host_finite(origin3[1]) &&
                     pg_host_finite(origin3[2]), 5);
  UCSA_CHECK_ARG(spacing3, 6);
  for (int a = 0; a < 3; ++a) UCSA_CHECK_ARG(spacing3[a] > 0.0f && pg_host_finite(spacing3[a]), 6);
  UCSA_CHECK_ARG(n <= (1u << 23), 8);
  UCSA_CHECK_ARG(n == 0 || points, 7);
  UCSA_CHECK_ARG(K <= UCSA_TSDF_ICP_BATCH_MAX, 10);
  UCSA_CHECK_ARG(K == 0 || transforms, 9);
  UCSA_CHECK_ARG(trunc > 0.0f && pg_host_finite(trunc), 11);
  UCSA_CHECK_ARG(min_weight > 0.0f, 12);
  UCSA_CHECK_ARG(max_tsdf > 0.0f && max_tsdf <= 1.0f, 13);
  const uint64_t ws_rows = (uint64_t)K * icp_workspace_rows(n);  // <= 2^10 * (2^15 + 2^7)
  UCSA_CHECK_ARG(ws_rows == 0 || workspace, 14);
  UCSA_CHECK_ARG(workspace_doubles >= ws_rows * ICP_SUMS, 15);
  UCSA_CHECK_ARG(K == 0 || sums, 16);
  if (K == 0) return 0;
  TsdfLattice L;
  L.n[0] = nx, L.n[1] = ny, L.n[2] = nz;
  for (int a = 0; a < 3; ++a) L.o[a] = origin3[a], L.h[a] = spacing3[a];
  hipStream_t s = (hipStream_t)stream;
  uint32_t count = n ? ucsa_div_up(n, PG_THREADS) : 1u;  // <= 2^15; n == 0 gives +0.0
  const uint32_t tiles = ucsa_div_up(K, TB_TILE);        // <= 2^7: one launch, at most 2^22 groups
  double* out = count == 1u ? sums : workspace;
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_tsdf_icp_sums_batch, dim3(tiles, count), dim3(PG_THREADS), 0, s, tsdf,
                     weight, L, points, n, transforms, K, trunc, min_weight, max_tsdf, out);
  while (count > 1u) {  // at most two passes for n <= 2^23
    const uint32_t next = ucsa_div_up(count, PG_THREADS);
    const double* in = out;
    out = next == 1u ? sums : out + (uint64_t)K * count * ICP_SUMS;
    hipLaunchKernelGGL(k_icp_reduce_batch, dim3(next, K), dim3(PG_THREADS), 0, s, in, count, out);
    count = next;
  }
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_icp_sums(const float* records, const int32_t* offsets, uint32_t n_pairs,
                                 const float* origin, float cell, const uint32_t* dims,
                                 const float* verts, uint32_t nv, const int32_t* faces,
                                 uint32_t nf, const float* unit_normal, const float* points,
                                 uint32_t n, const float* transform, float max_dist, int32_t mode,
                                 double* workspace, uint64_t workspace_doubles, double* sums,
                                 int32_t* face, float* dist2, void* stream) {
  UCSA_CHECK_ARG(n_pairs <= 0x7FFFFFFFu, 2);
  GridArgs g;
  const int bad = pg_grid_args(origin, cell, dims, g);
  UCSA_CHECK_ARG(bad != 1, 3);
  UCSA_CHECK_ARG(bad != 2, 4);
  UCSA_CHECK_ARG(bad != 3, 5);
  UCSA_CHECK_ARG(nv <= 0x7FFFFFFFu, 7);
  UCSA_CHECK_ARG(nf <= 0x7FFFFFFFu, 9);
  UCSA_CHECK_ARG(nv == 0 || verts, 6);
  UCSA_CHECK_ARG(nf == 0 || faces, 8);
  UCSA_CHECK_ARG(nf == 0 || unit_normal, 10);
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFu, 12);
  UCSA_CHECK_ARG(n == 0 || points, 11);
  UCSA_CHECK_ARG(transform, 13);
  const float limit2 = max_dist * max_dist;
  UCSA_CHECK_ARG(max_dist > 0.0f && pg_host_finite(max_dist) && pg_host_finite(limit2), 14);
  UCSA_CHECK_ARG(mode == 0 || mode == 1, 15);
  const uint64_t ws_rows = icp_workspace_rows(n);
  UCSA_CHECK_ARG(ws_rows == 0 || workspace, 16);
  UCSA_CHECK_ARG(workspace_doubles >= ws_rows * ICP_SUMS, 17);
  UCSA_CHECK_ARG(sums, 18);
  UCSA_CHECK_ARG(n_pairs == 0 || (records && ((uintptr_t)records & 15u) == 0), 0);
  UCSA_CHECK_ARG(n_pairs == 0 || offsets, 1);
  Rigid T;
  for (int k = 0; k < 12; ++k) T.m[k] = transform[k];
  hipStream_t s = (hipStream_t)stream;
  uint32_t count = n ? ucsa_div_up(n, PG_THREADS) : 1u;  // at least one stage: n == 0 gives +0.0
  double* out = count == 1u ? sums : workspace;
  UCSA_CLEAR_ERR();
  if (mode == 0)
    hipLaunchKernelGGL(k_icp_sums<0>, dim3(count), dim3(PG_THREADS), 0, s, (const float4*)records,
                       offsets, n_pairs, g, verts, nv, faces, nf, unit_normal, points, n, T, limit2,
                       out, face, dist2);
  else
    hipLaunchKernelGGL(k_icp_sums<1>, dim3(count), dim3(PG_THREADS), 0, s, (const float4*)records,
                       offsets, n_pairs, g, verts, nv, faces, nf, unit_normal, points, n, T, limit2,
                       out, face, dist2);
  // count shrinks by 256 per pass: at most three passes for n < 2^31
  while (count > 1u) {
    const uint32_t next = ucsa_div_up(count, PG_THREADS);
    const double* in = out;
    out = next == 1u ? sums : out + (uint64_t)count * ICP_SUMS;
    hipLaunchKernelGGL(k_icp_reduce, dim3(next), dim3(PG_THREADS), 0, s, in, count, out);
    count = next;
  }
  return ucsa_launch_status();
}
