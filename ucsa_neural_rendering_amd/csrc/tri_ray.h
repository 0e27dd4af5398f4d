// The intersection of a ray with a triangle, as mesh_raycast.hip evaluates it
// for every candidate.  The arithmetic is the ray-cast contract of
// include/ucsa_hip.h, restated in tests/raycast_numpy.py (intersect), and must
// stay as it is there: the kernels promise the definition's bits.
//
// It is the watertight test of Woop, Benthin and Wald (2013) with the zero-case
// fallback made unconditional: the corners are moved to the ray's origin,
// permuted so that the ray's largest direction component comes last, and
// sheared so that the ray runs along that axis, all in float32; the three edge
// functions are then taken in float64, where the products of two converted
// float32 values are exact and the sign of their difference is exact.  An edge
// shared by two faces gives exactly negated values in the two, so no ray slips
// between them.  The parameter is a float64 quotient rounded to float32 once.
// The box clause keeps a hit only where the ray's own point at that parameter
// lies inside the face's box (grown by 2^-20 of the magnitudes involved): that
// box is what the grid registered, which is what lets a traversal promise to
// find every hit (the proof is at the head of mesh_raycast.hip).
#pragma once
#include <cfloat>

#include "cell_grid.h"

namespace {

constexpr float RC_K = PG_K;  // 2^-20: the box clause

__device__ __forceinline__ float rc_sel(int k, float x, float y, float z) {
  return k == 0 ? x : (k == 1 ? y : z);
}

struct TriRay {
  float ox, oy, oz, dx, dy, dz;  // the ray as given
  float tmin, tmax;
  int kz;                // argmax |d|, the first on ties; kx = (kz+1)%3, ky = (kz+2)%3
  float okx, oky, okz;   // the origin, permuted
  float Sx, Sy;          // d[kx] / d[kz], d[ky] / d[kz]
  double dkz;
  bool valid;            // finite, d != 0

  __device__ __forceinline__ void init(const float* __restrict__ o, const float* __restrict__ d,
                                       float t0, float t1) {
    ox = o[0]; oy = o[1]; oz = o[2];
    dx = d[0]; dy = d[1]; dz = d[2];
    tmin = t0; tmax = t1;
    valid = pg_finite3(ox, oy, oz) && pg_finite3(dx, dy, dz) &&
            (dx != 0.0f || dy != 0.0f || dz != 0.0f);
    const float a0 = fabsf(dx), a1 = fabsf(dy), a2 = fabsf(dz);
    kz = a1 > a0 ? 1 : 0;
    kz = a2 > fmaxf(a0, a1) ? 2 : kz;
    okx = rc_sel(kz, oy, oz, ox);
    oky = rc_sel(kz, oz, ox, oy);
    okz = rc_sel(kz, ox, oy, oz);
    const float fkz = rc_sel(kz, dx, dy, dz);
    Sx = rc_sel(kz, dy, dz, dx) / fkz;
    Sy = rc_sel(kz, dz, dx, dy) / fkz;
    dkz = (double)fkz;
  }

  // one axis of the box clause: the ray's point at t inside [mn - S, mx + S]
  __device__ __forceinline__ bool in_box(float o, float d, float t, float a, float b,
                                         float c) const {
    const float td = t * d;
    const float p = o + td;
    const float mn = fminf(fminf(a, b), c), mx = fmaxf(fmaxf(a, b), c);
    const float S = RC_K * ((fabsf(o) + fabsf(td)) + fmaxf(fabsf(mn), fabsf(mx)));
    return mn - S <= p && p <= mx + S;
  }

  // steps 2 to 7 of the contract for one face with finite corners -> hit, and
  // then t and the edge functions
  __device__ __forceinline__ bool hit(const float4 A, const float4 B, const float4 C, float& t,
                                      double& U, double& V, double& W, double& det) const {
    const float apx = rc_sel(kz, A.y, A.z, A.x) - okx, apy = rc_sel(kz, A.z, A.x, A.y) - oky,
                apz = rc_sel(kz, A.x, A.y, A.z) - okz;
    const float bpx = rc_sel(kz, B.y, B.z, B.x) - okx, bpy = rc_sel(kz, B.z, B.x, B.y) - oky,
                bpz = rc_sel(kz, B.x, B.y, B.z) - okz;
    const float cpx = rc_sel(kz, C.y, C.z, C.x) - okx, cpy = rc_sel(kz, C.z, C.x, C.y) - oky,
                cpz = rc_sel(kz, C.x, C.y, C.z) - okz;
    const double Ax = (double)(apx - Sx * apz), Ay = (double)(apy - Sy * apz);
    const double Bx = (double)(bpx - Sx * bpz), By = (double)(bpy - Sy * bpz);
    const double Cx = (double)(cpx - Sx * cpz), Cy = (double)(cpy - Sy * cpz);
    U = Cx * By - Cy * Bx;
    V = Ax * Cy - Ay * Cx;
    W = Bx * Ay - By * Ax;
    det = (U + V) + W;
    const bool inside = ((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0)) &&
                        det != 0.0;
    if (!inside) return false;
    t = (float)(((U * (double)apz + V * (double)bpz) + W * (double)cpz) / det / dkz);
    if (!(isfinite(t) && tmin <= t && t <= tmax)) return false;
    return in_box(ox, dx, t, A.x, B.x, C.x) && in_box(oy, dy, t, A.y, B.y, C.y) &&
           in_box(oz, dz, t, A.z, B.z, C.z);
  }
};

}  // namespace
