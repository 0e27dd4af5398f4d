// The projection shared by the kernels that walk the TSDF lattice view by view
// (tsdf_fusion.hip, voxel_map.hip): the camera point of a voxel centre and the
// conservative test that lets a work-group skip a view for its whole brick.
#pragma once
#include <cmath>

#include "ucsa_common.h"

namespace {

// camera point of world point p: d = p - t, c_r = (d0*R0r + d1*R1r) + d2*R2r
__device__ __forceinline__ void ts_camera(const float* __restrict__ P, const float p[3],
                                          float c[3]) {
  const float d0 = p[0] - P[3], d1 = p[1] - P[7], d2 = p[2] - P[11];
#pragma unroll
  for (int r = 0; r < 3; ++r) c[r] = (d0 * P[r] + d1 * P[4 + r]) + d2 * P[8 + r];
}

// Can view P touch any voxel of the box [lo, hi] (fp32 voxel centres, per axis)?
// c[8][3]: the computed camera points of its corners.  p - t is monotone in p,
// so the box of d = p - t is exact; the computed camera coordinate r of any
// voxel in it differs from the exact one by at most a few ulp of
// L_r = sum_a max|d_a| * |R_ar|, and exact coordinates of the box lie between
// the exact corner values.  E_r = 1e-6 * L_r (8 ulp) bounds that error; every
// test below keeps 4 E_r of room, and anything non-finite culls nothing.
template <class Args>
__device__ bool ts_cull(const Args& a, const float* __restrict__ P, const float lo[3],
                        const float hi[3], const float (*c)[3]) {
  float E[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    float L = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float t = P[4 * k + 3];
      L += fmaxf(fabsf(lo[k] - t), fabsf(hi[k] - t)) * fabsf(P[4 * k + r]);
    }
    E[r] = 1e-6f * L;
  }
  float zmin = c[0][2], zmax = c[0][2];
  for (int q = 1; q < 8; ++q) {
    zmin = fminf(zmin, c[q][2]);
    zmax = fmaxf(zmax, c[q][2]);
  }
  bool finite = true;
  for (int q = 0; q < 8; ++q)
    finite = finite && isfinite(c[q][0]) && isfinite(c[q][1]) && isfinite(c[q][2]);
  if (!finite || !isfinite(E[0] + E[1] + E[2])) return false;
  if (zmax + 4.0f * E[2] < 0.0f) return true;  // every voxel has pc.z <= 0
  const float zl = zmin - 4.0f * E[2];
  // every voxel has d - pc.z < -trunc for every d <= depth_max
  if (zl > (a.dmax + a.trunc) * 1.00001f) return true;
  if (!(zl > 0.0f)) return false;
  // the box is in front of the camera: its projection lies in the hull of the
  // corners' projections
  const float f[2] = {a.fx, a.fy}, c0[2] = {a.cx, a.cy}, n[2] = {(float)a.W, (float)a.H};
  for (int r = 0; r < 2; ++r) {
    float umin = INFINITY, umax = -INFINITY, q = 0.0f;
    for (int k = 0; k < 8; ++k) {
      const float s = c[k][r] / c[k][2];
      const float u = f[r] * s + c0[r];
      umin = fminf(umin, u);
      umax = fmaxf(umax, u);
      q = fmaxf(q, fabsf(s));
    }
    const float m = 4.0f * f[r] * (E[r] + (q + 1.0f) * E[2]) / zl +
                    1e-5f * (f[r] * q + fabsf(c0[r])) + 1.0f;
    if (!isfinite(m) || !isfinite(umin) || !isfinite(umax)) continue;
    if (umax + m < 0.0f || umin - m >= n[r]) return true;
  }
  return false;
}

}  // namespace
