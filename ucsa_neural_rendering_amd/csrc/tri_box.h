// meets(face, box): the 13-axis separating-axis test of a triangle against an
// axis-aligned box in fp32, closed, with a rounding slack that keeps every
// touching pair.  The contract (expression order included) is stated in
// include/ucsa_hip.h under ucsa_mesh_voxelize_*; tests/voxelize_numpy.py
// restates it and docs/DESIGN_NOTEBOOK.md (section VX) derives TB_SLACK.  Every
// expression here is written in the header's order and is compiled without
// contraction: do not reassociate.
//
// A caller sets the face up once (tb_face_setup), then per box sets the three
// box axes (tb_box_axis: centre, grown half extent, corners relative to the
// centre) and asks the nine unit_a x edge_i axes (tb_cross_meets, a = 0, 1, 2)
// and the normal (tb_normal_meets).  The box-axis test is on lo / hi directly,
// mn[a] <= hi + slack && mx[a] >= lo - slack, and monotone in the cell index: a
// caller that walks a lattice settles it per axis once (vx_axis in
// mesh_voxelize.hip).  tb_cross_meets(., ., a) reads only the two other axes of
// the box, so a walk along axis a may ask it once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define TB_SLACK 9.5367431640625e-07f   // K * 2^-24 with K = 16: 2^-20
#define TB_MAX_COORD 1099511627776.0f   // 2^40: no product of the test overflows below it

struct TbFace {
  float p[3][3];  // corner j, axis a
  float e[3][3];  // e0 = p1 - p0, e1 = p2 - p1, e2 = p0 - p2
  float n[3];     // e0 x e1
  float mn[3], mx[3];
  float slack;
};

struct TbBox {
  float c[3], g[3];
  float v[3][3];  // corner j relative to the centre, axis a
};

// false: the face meets nothing (a corner that is not finite or lies beyond
// TB_MAX_COORD).  bmax: the family's largest absolute box bound.
__host__ __device__ __forceinline__ bool tb_face_setup(TbFace& f, const float* p0, const float* p1,
                                                       const float* p2, float bmax) {
  float s = bmax;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    f.p[0][a] = p0[a];
    f.p[1][a] = p1[a];
    f.p[2][a] = p2[a];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float m = fabsf(f.p[j][a]);
      ok = ok && m <= TB_MAX_COORD;  // NaN and inf fail
      s = fmaxf(s, m);
    }
    f.mn[a] = fminf(fminf(p0[a], p1[a]), p2[a]);
    f.mx[a] = fmaxf(fmaxf(p0[a], p1[a]), p2[a]);
    f.e[0][a] = p1[a] - p0[a];
    f.e[1][a] = p2[a] - p1[a];
    f.e[2][a] = p0[a] - p2[a];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    f.n[a] = f.e[0][b] * f.e[1][c] - f.e[0][c] * f.e[1][b];
  }
  f.slack = TB_SLACK * s;
  return ok;
}

__host__ __device__ __forceinline__ void tb_box_axis(const TbFace& f, TbBox& b, int a, float lo,
                                                     float hi) {
  b.c[a] = 0.5f * (lo + hi);
  b.g[a] = 0.5f * (hi - lo) + f.slack;
#pragma unroll
  for (int j = 0; j < 3; ++j) b.v[j][a] = f.p[j][a] - b.c[a];
}

// the three axes unit_a x e_i
__host__ __device__ __forceinline__ bool tb_cross_meets(const TbFace& f, const TbBox& x, int a) {
  const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float eb = f.e[i][b], ec = f.e[i][c];
    const float q0 = eb * x.v[0][c] - ec * x.v[0][b];
    const float q1 = eb * x.v[1][c] - ec * x.v[1][b];
    const float q2 = eb * x.v[2][c] - ec * x.v[2][b];
    const float r = x.g[b] * fabsf(ec) + x.g[c] * fabsf(eb);
    if (fminf(fminf(q0, q1), q2) > r || fmaxf(fmaxf(q0, q1), q2) < -r) return false;
  }
  return true;
}

__host__ __device__ __forceinline__ bool tb_normal_meets(const TbFace& f, const TbBox& x) {
  const float d0 = (f.n[0] * x.v[0][0] + f.n[1] * x.v[0][1]) + f.n[2] * x.v[0][2];
  const float d1 = (f.n[0] * x.v[1][0] + f.n[1] * x.v[1][1]) + f.n[2] * x.v[1][2];
  const float d2 = (f.n[0] * x.v[2][0] + f.n[1] * x.v[2][1]) + f.n[2] * x.v[2][2];
  const float r = (fabsf(f.n[0]) * x.g[0] + fabsf(f.n[1]) * x.g[1]) + fabsf(f.n[2]) * x.g[2];
  return !(fminf(fminf(d0, d1), d2) > r || fmaxf(fmaxf(d0, d1), d2) < -r);
}
