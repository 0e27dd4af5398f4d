// Mesh simplification by vertex clustering (Rossignac-Borrel; not in the
// reference): ucsa_vertex_cluster_keys, ucsa_cluster_reduce and
// ucsa_cluster_faces.  The contract is stated in include/ucsa_hip.h;
// tests/simplify_numpy.py restates it in plain loops and the outputs match it
// byte for byte.
//
// k_cluster_keys    a lane per vertex: the cell of cell_grid.h (t = (p - origin)
//                   / cell, clamped as a float into [0, dim - 1], floored) packed
//                   with the vertex's label into one int64,
//                   (((ix << 18 | iy) << 18 | iz) << 8) | label; INT64_MAX for a
//                   non-finite vertex, which sorts last and joins no cluster.
// k_cluster_reduce  a lane per cluster walks its members in the sorted order
//                   (by label, then by original index) and writes the cluster's
//                   row of every output.  The float sums are sequential: that
//                   order IS the definition, so a long cluster is one lane's
//                   loop and is not split across lanes.  A call that puts every
//                   vertex into one cell costs one lane walking all of them.
// k_cluster_faces   a lane per face: corners through vertex_map, degenerate
//                   faces dropped, the rest rotated to start at their smallest
//                   index (the cyclic order, and so the orientation, stays).
//
// Every index is clamped or tested before it is used, every loop is bounded by
// an argument (a cluster's walk by n), a lane writes its own row only; no
// atomics, no LDS, no waiting on another thread.
#include "cell_grid.h"

namespace {

constexpr uint32_t VC_MAX_DIM = 1u << 18;
constexpr int64_t VC_NO_CLUSTER = 0x7FFFFFFFFFFFFFFFll;

__global__ void __launch_bounds__(PG_THREADS) k_cluster_keys(const float* __restrict__ verts,
                                                             uint32_t n, GridArgs g,
                                                             const uint8_t* __restrict__ labels,
                                                             int64_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;
  if (i >= n) return;
  const float x = verts[3ull * i], y = verts[3ull * i + 1u], z = verts[3ull * i + 2u];
  const float tx = (x - g.o[0]) / g.cell, ty = (y - g.o[1]) / g.cell, tz = (z - g.o[2]) / g.cell;
  const uint64_t ix = pg_cell(tx, g.d[0]), iy = pg_cell(ty, g.d[1]), iz = pg_cell(tz, g.d[2]);
  const uint64_t lab = labels ? labels[i] : 0u;
  const uint64_t key = ((((ix << 18) | iy) << 18 | iz) << 8) | lab;  // < 2^62
  keys[i] = pg_finite3(x, y, z) ? (int64_t)key : VC_NO_CLUSTER;
}

__global__ void __launch_bounds__(PG_THREADS)
k_cluster_reduce(const float* __restrict__ verts, const float* __restrict__ normals,
                 const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ labels, uint32_t n,
                 const int32_t* __restrict__ order, const int32_t* __restrict__ first, uint32_t K,
                 float* __restrict__ out_verts, float* __restrict__ out_normals,
                 uint8_t* __restrict__ out_rgb, uint8_t* __restrict__ out_labels,
                 int32_t* __restrict__ out_count) {
  const uint32_t c = blockIdx.x * PG_THREADS + threadIdx.x;
  if (c >= K) return;
  // offsets clamped into [0, n]; a decreasing pair is an empty walk
  int32_t b = first[c], e = first[c + 1u];
  b = b < 0 ? 0 : (b > (int32_t)n ? (int32_t)n : b);
  e = e < 0 ? 0 : (e > (int32_t)n ? (int32_t)n : e);
  float x0[3] = {0.0f, 0.0f, 0.0f}, s[3] = {0.0f, 0.0f, 0.0f}, sn[3] = {0.0f, 0.0f, 0.0f};
  uint64_t sc[3] = {0u, 0u, 0u};
  uint32_t count = 0, best = 0, best_run = 0, run = 0, prev = 0xFFFFFFFFu;
  for (int32_t k = b; k < e; ++k) {  // 0 <= k < n: at most n passes
    const uint32_t m = (uint32_t)order[k];
    if (m >= n) continue;  // a malformed entry is no member
    const float p[3] = {verts[3ull * m], verts[3ull * m + 1u], verts[3ull * m + 2u]};
    if (count == 0) {
      x0[0] = p[0];
      x0[1] = p[1];
      x0[2] = p[2];
    }
    ++count;
    for (int a = 0; a < 3; ++a) s[a] = s[a] + (p[a] - x0[a]);
    if (normals)
      for (int a = 0; a < 3; ++a) sn[a] = sn[a] + normals[3ull * m + a];
    if (rgb)
      for (int a = 0; a < 3; ++a) sc[a] += rgb[3ull * m + a];
    if (labels) {
      const uint32_t l = labels[m];
      run = l == prev ? run + 1u : 1u;
      prev = l;
      if (l > 0u && run > best_run) {  // strictly: the first longest run wins
        best = l;
        best_run = run;
      }
    }
  }
  const float fc = (float)count;
  for (int a = 0; a < 3; ++a)
    out_verts[3ull * c + a] = count == 0 ? 0.0f : (count == 1 ? x0[a] : x0[a] + s[a] / fc);
  if (normals) {
    const float len = sqrtf((sn[0] * sn[0] + sn[1] * sn[1]) + sn[2] * sn[2]);
    for (int a = 0; a < 3; ++a) out_normals[3ull * c + a] = len > 0.0f ? sn[a] / len : 0.0f;
  }
  if (rgb)
    for (int a = 0; a < 3; ++a)
      out_rgb[3ull * c + a] =
          count == 0 ? (uint8_t)0 : (uint8_t)((2ull * sc[a] + count) / (2ull * count));
  if (labels) out_labels[c] = (uint8_t)best;
  out_count[c] = (int32_t)count;
}

__global__ void __launch_bounds__(PG_THREADS) k_cluster_faces(const int32_t* __restrict__ faces,
                                                              uint32_t nf,
                                                              const int32_t* __restrict__ vertex_map,
                                                              uint32_t nv,
                                                              int32_t* __restrict__ tri,
                                                              uint8_t* __restrict__ keep) {
  const uint32_t f = blockIdx.x * PG_THREADS + threadIdx.x;
  if (f >= nf) return;
  const uint32_t i0 = (uint32_t)faces[3ull * f], i1 = (uint32_t)faces[3ull * f + 1u],
                 i2 = (uint32_t)faces[3ull * f + 2u];
  int32_t a = -1, b = -1, c = -1;
  bool ok = i0 < nv && i1 < nv && i2 < nv;  // a negative index is a large unsigned one
  if (ok) {
    a = vertex_map[i0];
    b = vertex_map[i1];
    c = vertex_map[i2];
    ok = a >= 0 && b >= 0 && c >= 0 && a != b && b != c && a != c;
  }
  if (ok) {
    if (b < a && b < c) {
      const int32_t t = a;
      a = b;
      b = c;
      c = t;
    } else if (c < a && c < b) {
      const int32_t t = c;
      c = b;
      b = a;
      a = t;
    }
  } else {
    a = b = c = -1;
  }
  tri[3ull * f] = a;
  tri[3ull * f + 1u] = b;
  tri[3ull * f + 2u] = c;
  keep[f] = ok ? 1u : 0u;
}

}  // namespace

extern "C" int32_t ucsa_vertex_cluster_keys(const float* verts, uint32_t n, const float* origin,
                                            float cell, const uint32_t* dims,
                                            const uint8_t* labels, int64_t* keys, void* stream) {
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFu, 1);
  GridArgs g;
  // dims of at most 2^18 each; there is no per-cell table, so no cap on their product
  const int bad = pg_grid_args(origin, cell, dims, g, VC_MAX_DIM, ~0ull);
  UCSA_CHECK_ARG(bad != 1, 2);
  UCSA_CHECK_ARG(bad != 2, 3);
  UCSA_CHECK_ARG(bad != 3, 4);
  if (n == 0) return 0;
  UCSA_CHECK_ARG(verts, 0);
  UCSA_CHECK_ARG(keys, 6);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_cluster_keys, dim3(ucsa_div_up(n, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, verts, n, g, labels, keys);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_cluster_reduce(const float* verts, const float* normals,
                                       const uint8_t* rgb, const uint8_t* labels, uint32_t n,
                                       const int32_t* order, const int32_t* first, uint32_t K,
                                       float* out_verts, float* out_normals, uint8_t* out_rgb,
                                       uint8_t* out_labels, int32_t* out_count, void* stream) {
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFu, 4);
  UCSA_CHECK_ARG(K <= n, 7);  // a cluster has a member
  if (K == 0) return 0;
  UCSA_CHECK_ARG(verts, 0);
  UCSA_CHECK_ARG(order, 5);
  UCSA_CHECK_ARG(first, 6);
  UCSA_CHECK_ARG(out_verts, 8);
  UCSA_CHECK_ARG(!normals || out_normals, 9);
  UCSA_CHECK_ARG(!rgb || out_rgb, 10);
  UCSA_CHECK_ARG(!labels || out_labels, 11);
  UCSA_CHECK_ARG(out_count, 12);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_cluster_reduce, dim3(ucsa_div_up(K, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, verts, normals, rgb, labels, n, order, first, K,
                     out_verts, out_normals, out_rgb, out_labels, out_count);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_cluster_faces(const int32_t* faces, uint32_t nf,
                                      const int32_t* vertex_map, uint32_t nv, int32_t* tri,
                                      uint8_t* keep, void* stream) {
  UCSA_CHECK_ARG(nf <= 0x7FFFFFFFu, 1);
  UCSA_CHECK_ARG(nv <= 0x7FFFFFFFu, 3);
  if (nf == 0) return 0;
  UCSA_CHECK_ARG(faces, 0);
  UCSA_CHECK_ARG(nv == 0 || vertex_map, 2);
  UCSA_CHECK_ARG(tri, 4);
  UCSA_CHECK_ARG(keep, 5);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_cluster_faces, dim3(ucsa_div_up(nf, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, faces, nf, vertex_map, nv, tri, keep);
  return ucsa_launch_status();
}
