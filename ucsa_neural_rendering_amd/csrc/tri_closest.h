// The closest point of a triangle to a query and the state of one query's ring
// walk over (cell, face) records, shared by triangle_grid.hip (the search) and
// mesh_sdf.hip (the sign and the mesh-to-volume fill).  The arithmetic is the
// nearest-triangle contract of include/ucsa_hip.h, restated in
// tests/surface_numpy.py (closest), and must stay as it is there: both files
// promise numpy's float32 bits.
//
// The closest point of a face (Ericson's regions on the triangle moved so that
// the query is the origin) is evaluated without a branch: the region picks a
// numerator and a denominator, one division follows, the region picks (v, w).
// In every region that is the definition's expression on the definition's
// operands (the interior's den = 1 / sum is the same division).
#pragma once
#include "cell_grid.h"

namespace {

constexpr float TG_KS = 2.0f * PG_K;  // 2^-19

struct Corners {
  float ax, ay, az, bx, by, bz, cx, cy, cz;
  bool ok;
};

__device__ __forceinline__ Corners tg_corners(const float* __restrict__ verts, uint32_t nv,
                                              const int32_t* __restrict__ faces, uint32_t f) {
  Corners c;
  const uint32_t i0 = (uint32_t)faces[3ull * f], i1 = (uint32_t)faces[3ull * f + 1u],
                 i2 = (uint32_t)faces[3ull * f + 2u];  // a negative index is >= 2^31 > nv
  c.ok = i0 < nv && i1 < nv && i2 < nv;
  if (c.ok) {
    c.ax = verts[3ull * i0]; c.ay = verts[3ull * i0 + 1u]; c.az = verts[3ull * i0 + 2u];
    c.bx = verts[3ull * i1]; c.by = verts[3ull * i1 + 1u]; c.bz = verts[3ull * i1 + 2u];
    c.cx = verts[3ull * i2]; c.cy = verts[3ull * i2 + 1u]; c.cz = verts[3ull * i2 + 2u];
    c.ok = pg_finite3(c.ax, c.ay, c.az) && pg_finite3(c.bx, c.by, c.bz) &&
           pg_finite3(c.cx, c.cy, c.cz);
  }
  return c;
}

__device__ __forceinline__ float tg_dot(float x0, float x1, float x2, float y0, float y1, float y2) {
  return (x0 * y0 + x1 * y1) + x2 * y2;
}

// the closest point of one face to the query: (v, w), its squared distance, the
// region in the definition's order (0 A, 1 B, 2 AB, 3 C, 4 CA, 5 BC, 6 interior)
// and the point itself with the query at the origin
__device__ __forceinline__ void tg_closest_point(const float4 A, const float4 B, const float4 C,
                                                 float qx, float qy, float qz, float& v, float& w,
                                                 float& dist2, int& region_out, float& px_out,
                                                 float& py_out, float& pz_out) {
  const float ax = A.x - qx, ay = A.y - qy, az = A.z - qz;
  const float bx = B.x - qx, by = B.y - qy, bz = B.z - qz;
  const float cx = C.x - qx, cy = C.y - qy, cz = C.z - qz;
  const float abx = bx - ax, aby = by - ay, abz = bz - az;
  const float acx = cx - ax, acy = cy - ay, acz = cz - az;
  const float d1 = tg_dot(abx, aby, abz, -ax, -ay, -az), d2 = tg_dot(acx, acy, acz, -ax, -ay, -az);
  const float d3 = tg_dot(abx, aby, abz, -bx, -by, -bz), d4 = tg_dot(acx, acy, acz, -bx, -by, -bz);
  const float d5 = tg_dot(abx, aby, abz, -cx, -cy, -cz), d6 = tg_dot(acx, acy, acz, -cx, -cy, -cz);
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  // the regions in the definition's order; the last assignment that holds is the first true
  int region = 6;
  region = (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) ? 5 : region;
  region = (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) ? 4 : region;
  region = (d6 >= 0.0f && d5 <= d6) ? 3 : region;
  region = (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) ? 2 : region;
  region = (d3 >= 0.0f && d4 <= d3) ? 1 : region;
  region = (d1 <= 0.0f && d2 <= 0.0f) ? 0 : region;
  float num = 1.0f, den = (va + vb) + vc;
  num = region == 5 ? e43 : num;  den = region == 5 ? e43 + e56 : den;
  num = region == 4 ? d2 : num;   den = region == 4 ? d2 - d6 : den;
  num = region == 2 ? d1 : num;   den = region == 2 ? d1 - d3 : den;
  const float r = num / den;  // unused in the corner regions
  // the interior: clamps are selects, so that a NaN stays a NaN
  float vi = vb * r, wi = vc * r;
  vi = vi < 0.0f ? 0.0f : vi;
  vi = vi > 1.0f ? 1.0f : vi;
  const float t = 1.0f - vi;
  wi = wi < 0.0f ? 0.0f : wi;
  wi = wi > t ? t : wi;
  v = vi; w = wi;
  v = region == 5 ? 1.0f - r : v;  w = region == 5 ? r : w;
  v = region == 4 ? 0.0f : v;      w = region == 4 ? r : w;
  v = region == 3 ? 0.0f : v;      w = region == 3 ? 1.0f : w;
  v = region == 2 ? r : v;         w = region == 2 ? 0.0f : w;
  v = region == 1 ? 1.0f : v;      w = region == 1 ? 0.0f : w;
  v = region == 0 ? 0.0f : v;      w = region == 0 ? 0.0f : w;
  const float px = (ax + abx * v) + acx * w;
  const float py = (ay + aby * v) + acy * w;
  const float pz = (az + abz * v) + acz * w;
  dist2 = (px * px + py * py) + pz * pz;
  region_out = region;
  px_out = px; py_out = py; pz_out = pz;
}

// the closest point of one face to the query: (v, w) and its squared distance
__device__ __forceinline__ void tg_closest(const float4 A, const float4 B, const float4 C,
                                           float qx, float qy, float qz, float& v, float& w,
                                           float& dist2) {
  int region;
  float px, py, pz;
  tg_closest_point(A, B, C, qx, qy, qz, v, w, dist2, region, px, py, pz);
}

// the state of one query's walk (cell_grid.h)
struct FaceWalk {
  const float4* __restrict__ rec;
  float qx, qy, qz;
  float best;     // B = min(best dist2, max_dist^2)
  float v, w;     // the best face's weights of its second and third corner
  uint32_t bidx;  // PG_NONE: no match yet
  __device__ __forceinline__ void score(uint32_t k) {
    const float4 A = rec[3ull * k], B = rec[3ull * k + 1u], C = rec[3ull * k + 2u];
    float fv, fw, d2;
    tg_closest(A, B, C, qx, qy, qz, fv, fw, d2);
    const uint32_t j = __float_as_uint(A.w);
    if (d2 < best || (d2 == best && j < bidx)) {
      best = d2;
      bidx = j;
      v = fv;
      w = fw;
    }
  }
};

}  // namespace
