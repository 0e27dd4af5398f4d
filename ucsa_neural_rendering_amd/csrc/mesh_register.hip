// One step of ICP on the GPU (not in the reference): the Gauss-Newton normal
// equations of a set of points against a target, as 29 float64 sums in a fixed
// tree.  The contracts are stated in include/ucsa_hip.h and restated in numpy
// under tests/ (register_numpy.py, tsdf_register_numpy.py, projective_numpy.py,
// lockstep_numpy.py, robust_numpy.py); the sums match them byte for byte.  The
// file reads as shared pieces first, then the kernels, then five entry points.
//
// The pieces, each stated once:
//   the reduction     icp_put reduces one term over the wave (wave_tree_sum,
//                     wave_ops.h: the contract's balanced tree of adjacent
//                     pairs) and lane 0 of each wave parks it in LDS; behind the
//                     work-group's one barrier icp_finish adds the four waves as
//                     waves4_sum does, levels seven and eight of the tree.  A
//                     lane without a row holds +0.0, the contract's padding.
//   the 29 terms      icp_put29<ROWS>: the 21 entries of the upper triangle of
//                     J^T J (row-major), the 6 of J^T r, r^2 and the count, in
//                     this column order, each formed from the row's floats
//                     (icp_row, icp_term) and reduced at once: no term is live
//                     across what came before.
//   k_icp_reduce      a lane per row of the previous stage, 256 rows per
//                     work-group, the same reduction, repeated by
//                     icp_reduce_stages until one row per transform is left.
//                     The transform is blockIdx.y: 0 in a single step.
//   the TSDF sample   tsdf_sample (tsdf_sample.h), which also states why every
//                     index of the gather is in range.
//   the association   proj_associate: the projective step's move, projection,
//                     gather and gates.
//   the row's weight  icp_weigh_row: iteratively reweighted least squares for the
//                     two frame trackers, a template switch of their kernels.
//
// The kernels, a lane per point in work-groups of 256:
//   k_icp_sums<MODE>              against a triangle mesh: the nearest-triangle
//                                 search of triangle_grid.hip from the moved point.
//   k_tsdf_icp_sums<WEIGHTED>     against a TSDF volume.
//   k_tsdf_icp_sums_batch         the same for a tile of TB_TILE transforms per
//                                 work-group: K steps in one launch.
//   k_projective_icp_sums<WEIGHTED>  against a pair of vertex and normal maps.
//
// In all of them: no atomics.  One barrier per work-group, which every lane
// reaches: a lane with i >= n loads nothing, contributes +0.0 to all 29 sums and
// does not return early, and no lane waits for another outside that barrier.
// A lane writes its own slots of the per-point outputs, a work-group its own row
// of the workspace; every index read from memory is checked before use.
#include "tri_closest.h"
#include "tsdf_sample.h"
#include "wave_ops.h"

namespace {

constexpr uint32_t ICP_SUMS = 29;
constexpr uint32_t TB_TILE = UCSA_TSDF_ICP_BATCH_TILE;  // transforms per work-group

struct Rigid {
  float m[12];  // the rows of [R | t]
};

// one of the 29 sums over the work-group: `sh` is [ICP_SUMS][4]
__device__ __forceinline__ void icp_put(double v, uint32_t c, double* sh) {
  v = wave_tree_sum(v);
  if ((threadIdx.x & 63u) == 0u) sh[4u * c + (threadIdx.x >> 6)] = v;
}

// the work-group's one barrier, then its 29 sums to `row`
__device__ __forceinline__ void icp_finish(const double* sh, double* __restrict__ row) {
  __syncthreads();
  const uint32_t c = threadIdx.x;
  if (c < ICP_SUMS) row[c] = waves4_sum(sh + 4u * c);
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

// the 29 terms of a point's rows V (J 0..5, r 6, 1 7), each reduced into `sh`;
// unused bits of an unmatched row are selected away
template <int ROWS>
__device__ __forceinline__ void icp_put29(bool matched, const float (*V)[ROWS], double* sh) {
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
}

// stage `in` [K][count][29] -> `out` [K][gridDim.x][29]; blockIdx.y is the transform
__global__ void __launch_bounds__(PG_THREADS) k_icp_reduce(const double* __restrict__ in,
                                                           uint32_t count,
                                                           double* __restrict__ out) {
  __shared__ double sh[ICP_SUMS * 4u];
  const uint32_t row = blockIdx.x * PG_THREADS + threadIdx.x;
  const bool live = row < count;
  const double* mine = in + (uint64_t)blockIdx.y * count * ICP_SUMS;
#pragma unroll 1
  for (uint32_t c = 0; c < ICP_SUMS; ++c)
    icp_put(live ? mine[(uint64_t)row * ICP_SUMS + c] : 0.0, c, sh);
  icp_finish(sh, out + ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * ICP_SUMS);
}

// a lane's point: NaN without one, which is outside every lattice
__device__ __forceinline__ void icp_point(const float* __restrict__ points, uint32_t i, bool live,
                                          float& x, float& y, float& z) {
  x = y = z = NAN;
  if (live) {
    x = points[3ull * i];
    y = points[3ull * i + 1u];
    z = points[3ull * i + 2u];
  }
}

// ---- the row's weight: w = p * rho(|r|), for the two frame trackers ----
// A product by sqrt(w) = 1 is exact, so without weights the sums are the plain
// kernels' bits; slot 27 is then sum w r^2 and slot 28 the rows with w > 0.
struct RobustArgs {
  const float* point_weight;  // [n] or NULL: 1
  float* weight_out;          // [n] or NULL
  int32_t kind;               // UCSA_ROBUST_NONE / HUBER / TUKEY
  float scale;                // k or c, in the residual's units
};

// the point's weight, loaded with the point and before the gathers: it is on no
// dependent path
__device__ __forceinline__ float icp_point_weight(const RobustArgs& Q, uint32_t i, bool live) {
  float p = 0.0f;
  if (live) p = Q.point_weight ? Q.point_weight[i] : 1.0f;
  return p;
}

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

// scale the row by sqrt(w) and report the weight to the lane's own slot
// -> whether the row counts
__device__ __forceinline__ bool icp_weigh_row(bool matched, bool live, uint32_t i, float p,
                                              const RobustArgs& Q, float (*V)[1]) {
  const float w = icp_robust_weight(V[6][0], p, Q.kind, Q.scale);
  const bool counts = matched && w > 0.0f;
  if (live && Q.weight_out) Q.weight_out[i] = counts ? w : 0.0f;
  const float s = sqrtf(w);
#pragma unroll
  for (int a = 0; a < 7; ++a) V[a][0] = s * V[a][0];
  return counts;
}

// ---- against a triangle mesh ----
// The point is moved by [R | t], the nearest-triangle search of triangle_grid.hip
// (pg_walk over FaceWalk with TG_KS) runs from the moved point, the closest
// point of the face found is evaluated again on the mesh's own corners
// (tri_closest.h: the same operands, the same bits, as in mesh_sdf.hip), and the
// rows (J, r) follow.  Every loop is bounded as in pg_walk (cell_grid.h).
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
  icp_put29<ROWS>(matched, V, sh);
  icp_finish(sh, out + (uint64_t)blockIdx.x * ICP_SUMS);
}

// ---- against a TSDF volume ----
// The sample is tsdf_sample's (the range argument is stated there): the point is
// moved, its cell found, the cell's sixteen floats gathered before the first
// use, and F and the gradient follow in the ray-caster's expressions.  A point
// matches where the cell is observed, the gradient has a length and |F| <=
// max_tsdf; the row is r = -(F * trunc), J = (q x n, n) with n the unit gradient.
__device__ __forceinline__ bool tsdf_matched(const TsdfSample& s, float max_tsdf) {
  return s.observed && s.ln > 0.0f && isfinite(s.ln) && fabsf(s.F) <= max_tsdf;
}

__device__ __forceinline__ void tsdf_icp_row(const TsdfSample& s, float trunc, float (*V)[1]) {
  icp_row<1>(s.q[0], s.q[1], s.q[2], 0.0f, 0.0f, 0.0f, s.G[0] / s.ln, s.G[1] / s.ln,
             s.G[2] / s.ln, V, 0);
  V[6][0] = -(s.F * trunc);
}

// The single step keeps sixteen 4-byte loads.  value / match report the
// geometric match, whatever the weights.
template <bool WEIGHTED>
__global__ void __launch_bounds__(PG_THREADS) k_tsdf_icp_sums(
    const float* __restrict__ tsdf, const float* __restrict__ weight, TsdfLattice L,
    const float* __restrict__ points, uint32_t n, Rigid T, float trunc, float min_weight,
    float max_tsdf, RobustArgs Q, double* __restrict__ out, float* __restrict__ value,
    uint8_t* __restrict__ match) {
  __shared__ double sh[ICP_SUMS * 4u];
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;  // < 2^31 + 256
  const bool live = i < n;
  float x, y, z;
  icp_point(points, i, live, x, y, z);
  const float p = WEIGHTED ? icp_point_weight(Q, i, live) : 0.0f;
  const TsdfSample s = tsdf_sample<4>(tsdf, weight, L, T.m, x, y, z, min_weight);
  bool matched = tsdf_matched(s, max_tsdf);
  if (live) {
    if (value) value[i] = s.observed ? s.F : NAN;
    if (match) match[i] = matched ? 1 : 0;
  }
  float V[8][1];
  tsdf_icp_row(s, trunc, V);
  if constexpr (WEIGHTED) matched = icp_weigh_row(matched, live, i, p, Q, V);
  icp_put29<1>(matched, V, sh);
  icp_finish(sh, out + (uint64_t)blockIdx.x * ICP_SUMS);
}

// The same step for K transforms in one launch, shaped like k_tsdf_score
// (tsdf_score.hip): 256 points per work-group (blockIdx.y), a tile of TB_TILE
// transforms (blockIdx.x).  The point is loaded once.  The loop over the tile is
// uniform -- its trip count comes from blockIdx.x and K alone -- and so is the
// address of a transform's twelve floats: they arrive as scalar loads.  Per
// transform the body is the single step's, with the gather as eight 8-byte
// loads, and the 29 terms go to the transform's own [29][4] of LDS.  Behind the
// one barrier a lane per (transform, sum) adds the four waves and writes row
// (transform, work-group) of the stage's output [K][gridDim.y][29]: the same
// operands meet in the same tree as in the single step, so a row holds its bits.
//
// first + t is below K by the loop's bound (the host sizes the grid so that
// first < K); a row (k, group) with k < K and group < gridDim.y is below
// K * gridDim.y rows, which the host checks against the workspace.
__global__ void __launch_bounds__(PG_THREADS) k_tsdf_icp_sums_batch(
    const float* __restrict__ tsdf, const float* __restrict__ weight, TsdfLattice L,
    const float* __restrict__ points, uint32_t n, const float* __restrict__ transforms, uint32_t K,
    float trunc, float min_weight, float max_tsdf, double* __restrict__ out) {
  __shared__ double sh[TB_TILE * ICP_SUMS * 4u];            // [transform][sum][wave]
  const uint32_t i = blockIdx.y * PG_THREADS + threadIdx.x;  // < 2^23 + 256
  float x, y, z;
  icp_point(points, i, i < n, x, y, z);
  const uint32_t first = blockIdx.x * TB_TILE;  // < K: the host sizes the grid
  const uint32_t count = K - first < TB_TILE ? K - first : TB_TILE;
#pragma unroll 1
  for (uint32_t t = 0; t < count; ++t) {
    const TsdfSample s = tsdf_sample<8>(tsdf, weight, L, transforms + 12ull * (first + t), x, y, z,
                                        min_weight);
    float V[8][1];
    tsdf_icp_row(s, trunc, V);
    icp_put29<1>(tsdf_matched(s, max_tsdf), V, sh + t * (ICP_SUMS * 4u));
  }
  __syncthreads();
  const uint32_t c = threadIdx.x;  // (transform c / 29, sum c % 29)
  if (c < count * ICP_SUMS) {
    const uint32_t t = c / ICP_SUMS, sum = c - t * ICP_SUMS;
    out[((uint64_t)(first + t) * gridDim.y + blockIdx.y) * ICP_SUMS + sum] = waves4_sum(sh + 4u * c);
  }
}

// ---- against a pair of vertex and normal maps, by projection ----
struct ProjTarget {
  const float* points;
  const float* normals;
  const uint8_t* mask;
  uint32_t H, W, reject;
  float fx, fy, cx, cy;
};

struct ProjMatch {
  float q[3];    // the moved point
  float d[3];    // the target's point minus q
  float nt[3];   // the target's normal
  uint32_t pix;  // the pixel's row-major index
  bool matched;
};

// The point (and its normal) moved by the twelve floats T of [R | t], projected
// into the target camera with ucsa_tsdf_integrate's expression, the target's
// point, normal and mask at that pixel (seven loads, all issued before the
// first use) and the gates: mask, finite, distance, normal compatibility.
//
// Why every index is in range: no float is converted to an integer and no index
// is formed before `inside` holds, that is q2 > 0 and 0 <= u < (float)W and
// 0 <= v < (float)H for the floored u, v (a NaN fails every comparison).  u and
// v are then integers in [0, W - 1] and [0, H - 1]; the host checks H, W <=
// 16384, so v*W + u <= 2^28 - 1 and the uint32 product does not wrap.  A lane
// with i >= n, or without a pixel, loads nothing from the maps.
__device__ __forceinline__ ProjMatch proj_associate(const float* __restrict__ points,
                                                    const float* __restrict__ normals, uint32_t i,
                                                    bool live, const ProjTarget& G,
                                                    const float* __restrict__ T, float limit2,
                                                    float min_cos) {
  ProjMatch r;
  float m[3] = {0.0f, 0.0f, 0.0f};
  r.q[0] = r.q[1] = r.q[2] = NAN;
  if (live) {
    const float x = points[3ull * i], y = points[3ull * i + 1u], z = points[3ull * i + 2u];
    r.q[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    r.q[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    r.q[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    if (normals) {
      const float s0 = normals[3ull * i], s1 = normals[3ull * i + 1u], s2 = normals[3ull * i + 2u];
      m[0] = (T[0] * s0 + T[1] * s1) + T[2] * s2;
      m[1] = (T[4] * s0 + T[5] * s1) + T[6] * s2;
      m[2] = (T[8] * s0 + T[9] * s1) + T[10] * s2;
    }
  }
  bool inside = live && r.q[2] > 0.0f;
  float u = 0.0f, v = 0.0f;
  if (inside) {
    u = floorf((G.fx * r.q[0]) / r.q[2] + G.cx);
    v = floorf((G.fy * r.q[1]) / r.q[2] + G.cy);
    inside = u >= 0.0f && u < (float)G.W && v >= 0.0f && v < (float)G.H;
  }
  float c[3] = {0.0f, 0.0f, 0.0f};
  r.nt[0] = r.nt[1] = r.nt[2] = 0.0f;
  uint32_t mk = 0u;
  r.pix = 0u;
  if (inside) {
    r.pix = (uint32_t)v * G.W + (uint32_t)u;
    // all seven loads before the first use
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      c[a] = G.points[3ull * r.pix + a];
      r.nt[a] = G.normals[3ull * r.pix + a];
    }
    mk = G.mask[r.pix];
  }
  r.matched = inside && (mk & UCSA_DEPTH_NORMAL) != 0u && (mk & G.reject) == 0u;
#pragma unroll
  for (int a = 0; a < 3; ++a) r.matched = r.matched && isfinite(c[a]) && isfinite(r.nt[a]);
#pragma unroll
  for (int a = 0; a < 3; ++a) r.d[a] = c[a] - r.q[a];
  const float dist2 = (r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2];
  r.matched = r.matched && dist2 <= limit2;
  if (normals)
    r.matched = r.matched && (m[0] * r.nt[0] + m[1] * r.nt[1]) + m[2] * r.nt[2] >= min_cos;
  return r;
}

// r = nt . (c - q), J = (q x nt, nt).  pixel / residual (the unscaled r) report
// the geometric match, whatever the weights.
template <bool WEIGHTED>
__global__ void __launch_bounds__(PG_THREADS) k_projective_icp_sums(
    const float* __restrict__ points, const float* __restrict__ normals, uint32_t n, ProjTarget G,
    Rigid T, float limit2, float min_cos, RobustArgs Q, double* __restrict__ out,
    int32_t* __restrict__ pixel, float* __restrict__ residual) {
  __shared__ double sh[ICP_SUMS * 4u];
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;  // < 2^31 + 256
  const bool live = i < n;
  const float p = WEIGHTED ? icp_point_weight(Q, i, live) : 0.0f;
  const ProjMatch a = proj_associate(points, normals, i, live, G, T.m, limit2, min_cos);
  float V[8][1];
  icp_row<1>(a.q[0], a.q[1], a.q[2], a.d[0], a.d[1], a.d[2], a.nt[0], a.nt[1], a.nt[2], V, 0);
  bool matched = a.matched;
  if (live) {
    if (pixel) pixel[i] = matched ? (int32_t)a.pix : -1;
    if (residual) residual[i] = matched ? V[6][0] : NAN;
  }
  if constexpr (WEIGHTED) matched = icp_weigh_row(matched, live, i, p, Q, V);
  icp_put29<1>(matched, V, sh);
  icp_finish(sh, out + (uint64_t)blockIdx.x * ICP_SUMS);
}

// ---- the host side: the arguments the entry points share, and the launch path ----
Rigid icp_rigid(const float* transform) {
  Rigid T;
  for (int k = 0; k < 12; ++k) T.m[k] = transform[k];
  return T;
}

// the robust arguments' checks (0, or 1: kind, 2: scale) and the kernels' copy
int icp_robust_args(const float* point_weight, int32_t kind, float scale, float* weight_out,
                    RobustArgs& Q) {
  if (kind != UCSA_ROBUST_NONE && kind != UCSA_ROBUST_HUBER && kind != UCSA_ROBUST_TUKEY) return 1;
  if (kind != UCSA_ROBUST_NONE && !(scale > 0.0f && pg_host_finite(scale))) return 2;
  Q.point_weight = point_weight, Q.weight_out = weight_out;
  Q.kind = kind, Q.scale = kind == UCSA_ROBUST_NONE ? 1.0f : scale;
  return 0;
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

// workspace, workspace_doubles, sums of a call with K transforms: the position
// 0..2 of the first that fails, or -1
int icp_workspace_args(uint32_t K, uint32_t n, const double* workspace, uint64_t workspace_doubles,
                       const double* sums) {
  const uint64_t ws_rows = (uint64_t)K * icp_workspace_rows(n);  // <= 2^10 * (2^15 + 2^7) in a batch
  if (!(ws_rows == 0 || workspace)) return 0;
  if (!(workspace_doubles >= ws_rows * ICP_SUMS)) return 1;
  if (!(K == 0 || sums)) return 2;
  return -1;
}

// The stages of a call.  The first has a work-group per 256 points (at least one:
// n == 0 gives +0.0) and writes [K][count][29] to the workspace, or to `sums` if
// it is the only one; every later stage follows its input in the workspace, K
// times as large as in a single step, and the last (count == 1) is `sums`
// [K][29].  count shrinks by 256 per pass: at most three passes for n < 2^31.
struct IcpStages {
  uint32_t count;
  double* out;
  IcpStages(uint32_t n, double* workspace, double* sums)
      : count(n ? ucsa_div_up(n, PG_THREADS) : 1u), out(count == 1u ? sums : workspace) {}
};

int32_t icp_reduce_stages(uint32_t K, IcpStages st, double* sums, hipStream_t s) {
  while (st.count > 1u) {
    const uint32_t next = ucsa_div_up(st.count, PG_THREADS);
    const double* in = st.out;
    st.out = next == 1u ? sums : st.out + (uint64_t)K * st.count * ICP_SUMS;
    hipLaunchKernelGGL(k_icp_reduce, dim3(next, K), dim3(PG_THREADS), 0, s, in, st.count, st.out);
    st.count = next;
  }
  return ucsa_launch_status();
}

// the checks ucsa_tsdf_icp_sums and its weighted form share: the index 0..12, or -1
int tsdf_step_args(const float* tsdf, const float* weight, uint32_t nx, uint32_t ny, uint32_t nz,
                   const float* origin3, const float* spacing3, const float* points, uint32_t n,
                   const float* transform, float trunc, float min_weight, float max_tsdf,
                   TsdfLattice& L) {
  const int bad = tsdf_lattice_args(tsdf, weight, nx, ny, nz, origin3, spacing3, L);
  if (bad >= 0) return bad;
  if (!(n <= 0x7FFFFFFFu)) return 8;
  if (!(n == 0 || points)) return 7;
  if (!transform) return 9;
  if (!(trunc > 0.0f && pg_host_finite(trunc))) return 10;
  if (!(min_weight > 0.0f)) return 11;
  if (!(max_tsdf > 0.0f && max_tsdf <= 1.0f)) return 12;
  return -1;
}

template <bool WEIGHTED>
int32_t tsdf_step_launch(const float* tsdf, const float* weight, const TsdfLattice& L,
                         const float* points, uint32_t n, const float* transform, float trunc,
                         float min_weight, float max_tsdf, const RobustArgs& Q, double* workspace,
                         double* sums, float* value, uint8_t* matched, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const IcpStages st(n, workspace, sums);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_tsdf_icp_sums<WEIGHTED>, dim3(st.count), dim3(PG_THREADS), 0, s, tsdf, weight,
                     L, points, n, icp_rigid(transform), trunc, min_weight, max_tsdf, Q, st.out,
                     value, matched);
  return icp_reduce_stages(1, st, sums, s);
}

// the checks ucsa_projective_icp_sums and its weighted form share: the index
// 0..15, or -1; fills G and limit2
int proj_step_args(const float* points, uint32_t n, const float* target_points,
                   const float* target_normals, const uint8_t* target_mask, uint32_t H, uint32_t W,
                   uint32_t reject, float fx, float fy, float cx, float cy, const float* transform,
                   float max_dist, float min_cos, ProjTarget& G, float& limit2) {
  if (!(n <= 0x7FFFFFFFu)) return 2;
  if (!(n == 0 || points)) return 0;
  if (!target_points) return 3;
  if (!target_normals) return 4;
  if (!target_mask) return 5;
  if (!(H >= 1 && H <= 16384)) return 6;
  if (!(W >= 1 && W <= 16384)) return 7;
  if (!((reject & ~(UCSA_DEPTH_EDGE | UCSA_DEPTH_GRAZING)) == 0u)) return 8;
  if (!(fx > 0.0f && pg_host_finite(fx))) return 9;
  if (!(fy > 0.0f && pg_host_finite(fy))) return 10;
  if (!pg_host_finite(cx)) return 11;
  if (!pg_host_finite(cy)) return 12;
  if (!transform) return 13;
  limit2 = max_dist * max_dist;
  if (!(max_dist > 0.0f && pg_host_finite(max_dist) && pg_host_finite(limit2))) return 14;
  if (!(min_cos >= -1.0f && min_cos <= 1.0f)) return 15;
  G.points = target_points, G.normals = target_normals, G.mask = target_mask;
  G.H = H, G.W = W, G.reject = reject;
  G.fx = fx, G.fy = fy, G.cx = cx, G.cy = cy;
  return -1;
}

template <bool WEIGHTED>
int32_t proj_step_launch(const float* points, const float* normals, uint32_t n, const ProjTarget& G,
                         const float* transform, float limit2, float min_cos, const RobustArgs& Q,
                         double* workspace, double* sums, int32_t* pixel, float* residual,
                         void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const IcpStages st(n, workspace, sums);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_projective_icp_sums<WEIGHTED>, dim3(st.count), dim3(PG_THREADS), 0, s, points,
                     normals, n, G, icp_rigid(transform), limit2, min_cos, Q, st.out, pixel,
                     residual);
  return icp_reduce_stages(1, st, sums, s);
}

}  // namespace

extern "C" int32_t ucsa_projective_icp_sums(const float* points, const float* normals, uint32_t n,
                                            const float* target_points,
                                            const float* target_normals,
                                            const uint8_t* target_mask, uint32_t H, uint32_t W,
                                            uint32_t reject, float fx, float fy, float cx, float cy,
                                            const float* transform, float max_dist, float min_cos,
                                            double* workspace, uint64_t workspace_doubles,
                                            double* sums, int32_t* pixel, float* residual,
                                            void* stream) {
  ProjTarget G;
  float limit2;
  int bad = proj_step_args(points, n, target_points, target_normals, target_mask, H, W, reject, fx,
                           fy, cx, cy, transform, max_dist, min_cos, G, limit2);
  UCSA_CHECK_ARG(bad < 0, bad);
  bad = icp_workspace_args(1, n, workspace, workspace_doubles, sums);
  UCSA_CHECK_ARG(bad < 0, 16 + bad);
  return proj_step_launch<false>(points, normals, n, G, transform, limit2, min_cos, RobustArgs{},
                                 workspace, sums, pixel, residual, stream);
}

extern "C" int32_t ucsa_projective_icp_sums_weighted(
    const float* points, const float* normals, uint32_t n, const float* target_points,
    const float* target_normals, const uint8_t* target_mask, uint32_t H, uint32_t W,
    uint32_t reject, float fx, float fy, float cx, float cy, const float* transform,
    float max_dist, float min_cos, const float* point_weight, int32_t robust_kind,
    float robust_scale, double* workspace, uint64_t workspace_doubles, double* sums,
    int32_t* pixel, float* residual, float* weight_out, void* stream) {
  ProjTarget G;
  float limit2;
  int bad = proj_step_args(points, n, target_points, target_normals, target_mask, H, W, reject, fx,
                           fy, cx, cy, transform, max_dist, min_cos, G, limit2);
  UCSA_CHECK_ARG(bad < 0, bad);
  RobustArgs Q;
  bad = icp_robust_args(point_weight, robust_kind, robust_scale, weight_out, Q);
  UCSA_CHECK_ARG(bad == 0, 16 + bad);
  bad = icp_workspace_args(1, n, workspace, workspace_doubles, sums);
  UCSA_CHECK_ARG(bad < 0, 19 + bad);
  return proj_step_launch<true>(points, normals, n, G, transform, limit2, min_cos, Q, workspace,
                                sums, pixel, residual, stream);
}

extern "C" int32_t ucsa_tsdf_icp_sums(const float* tsdf, const float* weight, uint32_t nx,
                                      uint32_t ny, uint32_t nz, const float* origin3,
                                      const float* spacing3, const float* points, uint32_t n,
                                      const float* transform, float trunc, float min_weight,
                                      float max_tsdf, double* workspace,
                                      uint64_t workspace_doubles, double* sums, float* value,
                                      uint8_t* matched, void* stream) {
  TsdfLattice L;
  int bad = tsdf_step_args(tsdf, weight, nx, ny, nz, origin3, spacing3, points, n, transform, trunc,
                           min_weight, max_tsdf, L);
  UCSA_CHECK_ARG(bad < 0, bad);
  bad = icp_workspace_args(1, n, workspace, workspace_doubles, sums);
  UCSA_CHECK_ARG(bad < 0, 13 + bad);
  return tsdf_step_launch<false>(tsdf, weight, L, points, n, transform, trunc, min_weight, max_tsdf,
                                 RobustArgs{}, workspace, sums, value, matched, stream);
}

extern "C" int32_t ucsa_tsdf_icp_sums_weighted(
    const float* tsdf, const float* weight, uint32_t nx, uint32_t ny, uint32_t nz,
    const float* origin3, const float* spacing3, const float* points, uint32_t n,
    const float* transform, float trunc, float min_weight, float max_tsdf,
    const float* point_weight, int32_t robust_kind, float robust_scale, double* workspace,
    uint64_t workspace_doubles, double* sums, float* value, uint8_t* matched, float* weight_out,
    void* stream) {
  TsdfLattice L;
  int bad = tsdf_step_args(tsdf, weight, nx, ny, nz, origin3, spacing3, points, n, transform, trunc,
                           min_weight, max_tsdf, L);
  UCSA_CHECK_ARG(bad < 0, bad);
  RobustArgs Q;
  bad = icp_robust_args(point_weight, robust_kind, robust_scale, weight_out, Q);
  UCSA_CHECK_ARG(bad == 0, 13 + bad);
  bad = icp_workspace_args(1, n, workspace, workspace_doubles, sums);
  UCSA_CHECK_ARG(bad < 0, 16 + bad);
  return tsdf_step_launch<true>(tsdf, weight, L, points, n, transform, trunc, min_weight, max_tsdf,
                                Q, workspace, sums, value, matched, stream);
}

extern "C" int32_t ucsa_tsdf_icp_sums_batch(const float* tsdf, const float* weight, uint32_t nx,
                                            uint32_t ny, uint32_t nz, const float* origin3,
                                            const float* spacing3, const float* points, uint32_t n,
                                            const float* transforms, uint32_t K, float trunc,
                                            float min_weight, float max_tsdf, double* workspace,
                                            uint64_t workspace_doubles, double* sums,
                                            void* stream) {
  TsdfLattice L;
  int bad = tsdf_lattice_args(tsdf, weight, nx, ny, nz, origin3, spacing3, L);
  UCSA_CHECK_ARG(bad < 0, bad);
  UCSA_CHECK_ARG(n <= (1u << 23), 8);
  UCSA_CHECK_ARG(n == 0 || points, 7);
  UCSA_CHECK_ARG(K <= UCSA_TSDF_ICP_BATCH_MAX, 10);
  UCSA_CHECK_ARG(K == 0 || transforms, 9);
  UCSA_CHECK_ARG(trunc > 0.0f && pg_host_finite(trunc), 11);
  UCSA_CHECK_ARG(min_weight > 0.0f, 12);
  UCSA_CHECK_ARG(max_tsdf > 0.0f && max_tsdf <= 1.0f, 13);
  bad = icp_workspace_args(K, n, workspace, workspace_doubles, sums);
  UCSA_CHECK_ARG(bad < 0, 14 + bad);
  if (K == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const IcpStages st(n, workspace, sums);               // count <= 2^15: at most two passes
  const uint32_t tiles = ucsa_div_up(K, TB_TILE);        // <= 2^7: one launch, at most 2^22 groups
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_tsdf_icp_sums_batch, dim3(tiles, st.count), dim3(PG_THREADS), 0, s, tsdf,
                     weight, L, points, n, transforms, K, trunc, min_weight, max_tsdf, st.out);
  return icp_reduce_stages(K, st, sums, s);
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
  int bad = pg_grid_args(origin, cell, dims, g);
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
  bad = icp_workspace_args(1, n, workspace, workspace_doubles, sums);
  UCSA_CHECK_ARG(bad < 0, 16 + bad);
  UCSA_CHECK_ARG(n_pairs == 0 || (records && ((uintptr_t)records & 15u) == 0), 0);
  UCSA_CHECK_ARG(n_pairs == 0 || offsets, 1);
  hipStream_t s = (hipStream_t)stream;
  const IcpStages st(n, workspace, sums);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(mode == 0 ? k_icp_sums<0> : k_icp_sums<1>, dim3(st.count), dim3(PG_THREADS), 0,
                     s, (const float4*)records, offsets, n_pairs, g, verts, nv, faces, nf,
                     unit_normal, points, n, icp_rigid(transform), limit2, st.out, face, dist2);
  return icp_reduce_stages(1, st, sums, s);
}
