// Signed distance to a triangle mesh (not in the reference): ucsa_face_unit_normals,
// ucsa_normal_runs, ucsa_mesh_sign and ucsa_mesh_tsdf.  The contract is stated
// in include/ucsa_hip.h; tests/sdf_numpy.py restates it in plain loops and the
// outputs match it byte for byte.
//
// k_face_normals   a lane per face: the unit normal of (B - A) x (C - A), a zero
//                  row for an invalid or degenerate face.
// k_normal_runs    a lane per run (a vertex's corners or an edge's half-edges):
//                  a sequential float32 sum of weighted unit normals in the
//                  order of `items`, as mesh_simplify.hip's reduce kernel sums a
//                  cluster.  A long run is one lane's loop.
// k_mesh_sign      a lane per query: the closest point of the face the search
//                  found, evaluated again on the same operands (tri_closest.h),
//                  gives the feature (face, edge or vertex) the point lies on;
//                  the sign is that of the feature's angle-weighted pseudonormal
//                  (Baerentzen and Aanaes 2005) against the direction to the query.
// k_mesh_tsdf      a lane per voxel, z fastest: the nearest-triangle search of
//                  triangle_grid.hip (pg_walk over FaceWalk with TG_KS) from the
//                  voxel's point with limit2 = trunc^2, then the sign as above,
//                  and tsdf / weight written where a face was found.  One launch,
//                  no queries array and no face / dist2 / bary round trip.
//
// No atomics, no LDS, no waiting on another thread.  Every loop is bounded: the
// walk by the grid's dims and n_pairs (cell_grid.h), a run by n_items.  A lane
// writes its own row of the outputs and nothing else; every index read from
// memory (a face's corners, an item, a record's face) is checked before use.
#include "tri_closest.h"

namespace {

struct MeshNormals {
  const float* __restrict__ unit;    // [nf][3]
  const float* __restrict__ vertex;  // [nv][3]
  const float* __restrict__ edge;    // [nf][3][3]
};

__global__ void __launch_bounds__(PG_THREADS) k_face_normals(const float* __restrict__ verts,
                                                             uint32_t nv,
                                                             const int32_t* __restrict__ faces,
                                                             uint32_t nf,
                                                             float* __restrict__ unit) {
  const uint32_t f = blockIdx.x * PG_THREADS + threadIdx.x;
  if (f >= nf) return;
  const Corners c = tg_corners(verts, nv, faces, f);
  float ux = 0.0f, uy = 0.0f, uz = 0.0f;
  if (c.ok) {
    const float e1x = c.bx - c.ax, e1y = c.by - c.ay, e1z = c.bz - c.az;
    const float e2x = c.cx - c.ax, e2y = c.cy - c.ay, e2z = c.cz - c.az;
    const float nx = e1y * e2z - e1z * e2y;
    const float ny = e1z * e2x - e1x * e2z;
    const float nz = e1x * e2y - e1y * e2x;
    const float l = sqrtf(tg_dot(nx, ny, nz, nx, ny, nz));
    if (l > 0.0f && isfinite(l)) {
      ux = nx / l;
      uy = ny / l;
      uz = nz / l;
    }
  }
  unit[3ull * f] = ux;
  unit[3ull * f + 1u] = uy;
  unit[3ull * f + 2u] = uz;
}

__global__ void __launch_bounds__(PG_THREADS) k_normal_runs(const int32_t* __restrict__ items,
                                                            const int32_t* __restrict__ run_first,
                                                            uint32_t n_runs, uint32_t n_items,
                                                            const float* __restrict__ weight,
                                                            const float* __restrict__ unit,
                                                            uint32_t nf, float* __restrict__ out) {
  const uint32_t r = blockIdx.x * PG_THREADS + threadIdx.x;
  if (r >= n_runs) return;
  int32_t b = run_first[r], e = run_first[r + 1u];
  b = b < 0 ? 0 : b;
  e = e > (int32_t)n_items ? (int32_t)n_items : e;
  const uint32_t n_corners = 3u * nf;  // nf <= (2^31-1)/3: no wrap
  float ax = 0.0f, ay = 0.0f, az = 0.0f;
  for (int32_t pos = b; pos < e; ++pos) {  // 0 <= pos < n_items
    const uint32_t it = (uint32_t)items[pos];  // a negative item is >= 2^31 > n_corners
    if (it >= n_corners) continue;
    const float w = weight ? weight[it] : 1.0f;
    const uint32_t f = it / 3u;
    ax = ax + w * unit[3ull * f];
    ay = ay + w * unit[3ull * f + 1u];
    az = az + w * unit[3ull * f + 2u];
  }
  out[3ull * r] = ax;
  out[3ull * r + 1u] = ay;
  out[3ull * r + 2u] = az;
}

// The signed distance from the query to face f < nf and the feature its closest
// point lies on -> false (nothing written) for an invalid face.
__device__ __forceinline__ bool sd_signed(const float* __restrict__ verts, uint32_t nv,
                                          const int32_t* __restrict__ faces, uint32_t f,
                                          const MeshNormals& N, float qx, float qy, float qz,
                                          float& sdf, int& feature) {
  const Corners c = tg_corners(verts, nv, faces, f);
  if (!c.ok) return false;
  const float4 A = make_float4(c.ax, c.ay, c.az, 0.0f), B = make_float4(c.bx, c.by, c.bz, 0.0f),
               C = make_float4(c.cx, c.cy, c.cz, 0.0f);
  float v, w, dist2, px, py, pz;
  int region;
  tg_closest_point(A, B, C, qx, qy, qz, v, w, dist2, region, px, py, pz);
  // regions 0 A, 1 B, 2 AB, 3 C, 4 CA, 5 BC, 6 interior -> features 0 face,
  // 1 AB, 2 BC, 3 CA, 4 A, 5 B, 6 C
  int ft = 0;
  ft = region == 0 ? 4 : ft;
  ft = region == 1 ? 5 : ft;
  ft = region == 3 ? 6 : ft;
  ft = region == 2 ? 1 : ft;
  ft = region == 5 ? 2 : ft;
  ft = region == 4 ? 3 : ft;
  const float* n = N.unit + 3ull * f;
  if (ft >= 4) {
    const uint32_t vi = (uint32_t)faces[3ull * f + (uint32_t)(ft - 4)];  // < nv: the face is valid
    n = N.vertex + 3ull * vi;
  } else if (ft >= 1) {
    n = N.edge + 9ull * f + 3u * (uint32_t)(ft - 1);
  }
  const float s = -tg_dot(px, py, pz, n[0], n[1], n[2]);
  const float d = sqrtf(dist2);
  sdf = s < 0.0f ? -d : d;  // a zero or NaN normal: +d
  feature = ft;
  return true;
}

__global__ void __launch_bounds__(PG_THREADS) k_mesh_sign(const float* __restrict__ verts,
                                                          uint32_t nv,
                                                          const int32_t* __restrict__ faces,
                                                          uint32_t nf, MeshNormals N,
                                                          const float* __restrict__ queries,
                                                          uint32_t nq,
                                                          const int32_t* __restrict__ face,
                                                          float* __restrict__ sdf,
                                                          int32_t* __restrict__ feature) {
  const uint32_t i = blockIdx.x * PG_THREADS + threadIdx.x;
  if (i >= nq) return;
  const uint32_t f = (uint32_t)face[i];  // a negative face is >= 2^31 > nf
  float s = INFINITY;
  int ft = -1;
  if (f < nf) {
    float sv;
    int fv;
    if (sd_signed(verts, nv, faces, f, N, queries[3ull * i], queries[3ull * i + 1u],
                  queries[3ull * i + 2u], sv, fv)) {
      s = sv;
      ft = fv;
    }
  }
  sdf[i] = s;
  feature[i] = ft;
}

struct Lattice {
  float o[3];
  float s[3];
  uint32_t d[3];
};

__global__ void __launch_bounds__(PG_THREADS) k_mesh_tsdf(const float4* __restrict__ rec,
                                                          const int32_t* __restrict__ offsets,
                                                          uint32_t n, GridArgs g,
                                                          const float* __restrict__ verts,
                                                          uint32_t nv,
                                                          const int32_t* __restrict__ faces,
                                                          uint32_t nf, MeshNormals N, Lattice L,
                                                          uint32_t n_vox, float trunc, float limit2,
                                                          float weight_value,
                                                          float* __restrict__ tsdf,
                                                          float* __restrict__ weight) {
  // z fastest: a wave is a line of 64 voxels.  A wave per brick of 4 x 4 x 4 voxels
  // was measured too: faster on a fine mesh at 128^3 (7.5 against 10.5 ms), slower
  // at 256^3 on a coarse and on a fine one (2.4 against 1.6, 12.5 against 10.5 ms)
  const uint32_t vox = blockIdx.x * PG_THREADS + threadIdx.x;
  if (vox >= n_vox) return;
  const uint32_t k = vox % L.d[2], ij = vox / L.d[2];
  const uint32_t j = ij % L.d[1], i = ij / L.d[1];
  FaceWalk w;
  w.rec = rec;
  w.qx = L.o[0] + (float)i * L.s[0];
  w.qy = L.o[1] + (float)j * L.s[1];
  w.qz = L.o[2] + (float)k * L.s[2];
  w.best = limit2;
  w.bidx = PG_NONE;
  w.v = 0.0f;
  w.w = 0.0f;
  pg_walk(offsets, n, g, TG_KS, limit2, w);
  if (w.bidx >= nf) return;  // PG_NONE, or a record that names no face: not touched
  float s;
  int ft;
  if (!sd_signed(verts, nv, faces, w.bidx, N, w.qx, w.qy, w.qz, s, ft)) return;
  float t = s / trunc;
  t = t < -1.0f ? -1.0f : t;
  t = t > 1.0f ? 1.0f : t;
  tsdf[vox] = t;
  weight[vox] = weight_value;
}

}  // namespace

extern "C" int32_t ucsa_face_unit_normals(const float* verts, uint32_t nv, const int32_t* faces,
                                          uint32_t nf, float* unit_normal, void* stream) {
  UCSA_CHECK_ARG(nv <= 0x7FFFFFFFu, 1);
  UCSA_CHECK_ARG(nf <= 0x7FFFFFFFu, 3);
  if (nf == 0) return 0;
  UCSA_CHECK_ARG(nv == 0 || verts, 0);
  UCSA_CHECK_ARG(faces, 2);
  UCSA_CHECK_ARG(unit_normal, 4);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_face_normals, dim3(ucsa_div_up(nf, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, verts, nv, faces, nf, unit_normal);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_normal_runs(const int32_t* items, const int32_t* run_first,
                                    uint32_t n_runs, uint32_t n_items, const float* weight,
                                    const float* unit_normal, uint32_t nf, float* out,
                                    void* stream) {
  UCSA_CHECK_ARG(n_runs <= 0x7FFFFFFFu, 2);
  UCSA_CHECK_ARG(n_items <= 0x7FFFFFFFu, 3);
  UCSA_CHECK_ARG(nf <= 0x7FFFFFFFu / 3u, 6);
  if (n_runs == 0) return 0;
  UCSA_CHECK_ARG(n_items == 0 || items, 0);
  UCSA_CHECK_ARG(run_first, 1);
  UCSA_CHECK_ARG(nf == 0 || unit_normal, 5);
  UCSA_CHECK_ARG(out, 7);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_normal_runs, dim3(ucsa_div_up(n_runs, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, items, run_first, n_runs, n_items, weight, unit_normal,
                     nf, out);
  return ucsa_launch_status();
}

namespace {

// the mesh and its normals as ucsa_mesh_sign and ucsa_mesh_tsdf take them, at
// positions `at` ...: verts, nv, faces, nf, unit_normal, vertex_normal, edge_normal
int32_t sd_mesh_args(const float* verts, uint32_t nv, const int32_t* faces, uint32_t nf,
                     const float* unit_normal, const float* vertex_normal,
                     const float* edge_normal, int at) {
  UCSA_CHECK_ARG(nv <= 0x7FFFFFFFu, at + 1);
  UCSA_CHECK_ARG(nf <= 0x7FFFFFFFu, at + 3);
  UCSA_CHECK_ARG(nv == 0 || verts, at);
  UCSA_CHECK_ARG(nf == 0 || faces, at + 2);
  UCSA_CHECK_ARG(nf == 0 || unit_normal, at + 4);
  UCSA_CHECK_ARG(nv == 0 || vertex_normal, at + 5);
  UCSA_CHECK_ARG(nf == 0 || edge_normal, at + 6);
  return 0;
}

}  // namespace

extern "C" int32_t ucsa_mesh_sign(const float* verts, uint32_t nv, const int32_t* faces,
                                  uint32_t nf, const float* unit_normal,
                                  const float* vertex_normal, const float* edge_normal,
                                  const float* queries, uint32_t nq, const int32_t* face,
                                  float* sdf, int32_t* feature, void* stream) {
  const int32_t st = sd_mesh_args(verts, nv, faces, nf, unit_normal, vertex_normal, edge_normal, 0);
  if (st != 0) return st;
  UCSA_CHECK_ARG(nq <= 0x7FFFFFFFu, 8);
  if (nq == 0) return 0;
  UCSA_CHECK_ARG(queries, 7);
  UCSA_CHECK_ARG(face, 9);
  UCSA_CHECK_ARG(sdf, 10);
  UCSA_CHECK_ARG(feature, 11);
  const MeshNormals N = {unit_normal, vertex_normal, edge_normal};
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_mesh_sign, dim3(ucsa_div_up(nq, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, verts, nv, faces, nf, N, queries, nq, face, sdf, feature);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_mesh_tsdf(const float* records, const int32_t* offsets, uint32_t n_pairs,
                                  const float* origin, float cell, const uint32_t* dims,
                                  const float* verts, uint32_t nv, const int32_t* faces,
                                  uint32_t nf, const float* unit_normal,
                                  const float* vertex_normal, const float* edge_normal,
                                  float* tsdf, float* weight, uint32_t nx, uint32_t ny,
                                  uint32_t nz, const float* vol_origin, const float* vol_spacing,
                                  float trunc, float weight_value, void* stream) {
  UCSA_CHECK_ARG(n_pairs <= 0x7FFFFFFFu, 2);
  GridArgs g;
  const int bad = pg_grid_args(origin, cell, dims, g);
  UCSA_CHECK_ARG(bad != 1, 3);
  UCSA_CHECK_ARG(bad != 2, 4);
  UCSA_CHECK_ARG(bad != 3, 5);
  const int32_t st = sd_mesh_args(verts, nv, faces, nf, unit_normal, vertex_normal, edge_normal, 6);
  if (st != 0) return st;
  UCSA_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2, 15);
  UCSA_CHECK_ARG((uint64_t)nx * ny <= 0x7FFFFFFFull && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 15);
  UCSA_CHECK_ARG(vol_origin, 18);
  UCSA_CHECK_ARG(vol_spacing, 19);
  const float limit2 = trunc * trunc;
  UCSA_CHECK_ARG(trunc > 0.0f && pg_host_finite(trunc) && pg_host_finite(limit2), 20);
  if (n_pairs == 0) return 0;
  UCSA_CHECK_ARG(records && ((uintptr_t)records & 15u) == 0, 0);
  UCSA_CHECK_ARG(offsets, 1);
  UCSA_CHECK_ARG(tsdf, 13);
  UCSA_CHECK_ARG(weight, 14);
  Lattice L;
  for (int a = 0; a < 3; ++a) {
    L.o[a] = vol_origin[a];
    L.s[a] = vol_spacing[a];
  }
  L.d[0] = nx; L.d[1] = ny; L.d[2] = nz;
  const uint32_t n_vox = nx * ny * nz;
  const MeshNormals N = {unit_normal, vertex_normal, edge_normal};
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_mesh_tsdf, dim3(ucsa_div_up(n_vox, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, (const float4*)records, offsets, n_pairs, g, verts, nv,
                     faces, nf, N, L, n_vox, trunc, limit2, weight_value, tsdf, weight);
  return ucsa_launch_status();
}
