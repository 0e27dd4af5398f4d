// Rays against a triangle mesh (not in the reference): ucsa_raycast_mesh (the
// nearest hit) and ucsa_mesh_occluded (any hit).  The contract is stated in
// include/ucsa_hip.h; tests/raycast_numpy.py restates it as brute force over all
// faces, and the outputs match that byte for byte whatever the cell size.
//
// k_raycast  a lane per ray, lane t takes ray order[t].  The ray walks the
//            triangle grid (triangle_grid.hip: a face is registered in every
//            cell of the box between its corners' cells) layer by layer along
//            its major axis kz, in ray order: a slab supercover.  Per layer i:
//              the layer's walls zl = o_g + i h, zh = o_g + (i+1) h, grown by
//              the slack Sz, give the parameter interval [t0, t1] in which the
//              ray is inside the layer; cut to [t_min, t_max] it is [c0, c1];
//              the ray's points at c0 and c1 give, per minor axis, a range of
//              coordinates, grown by that axis's slack, and the cells between
//              pg_cell(low) and pg_cell(high) are visited (|Sx|, |Sy| <= 1: a
//              few cells); a layer whose range lies off the grid is skipped;
//              every record of a visited cell is a candidate (tri_ray.h).
//            The walk ends when best t < t0 of the layer to come, when t0 is
//            past t_max, or after the last layer; the any-hit form ends at its
//            first hit.  A face met in several cells is evaluated again: the
//            result is the minimum of (t, face) over a set.
//
// Why no hit is lost.  Let a face be hit at t (float32) by the definition, and
// p_a = fl(o_a + fl(t d_a)) be the ray's point of the box clause, which holds:
// mn_a - S_a <= p_a <= mx_a + S_a with S_a = 2^-20 (|o_a| + |t d_a| + |corner_a|).
// All corners lie in the grid's box, and |t d_a| <= |o_a| + |p_a|, so
// S_a <= 2^-19 (1 + 2^-19) (|o_a| + M_a), M_a the larger of |o_g| and |top| on that
// axis.  The traversal's slack is Sa' = 2^-17 (|o_a| + |o_g| + |top|) >= 4 S_a.
// q_a = p_a clamped into [mn_a, mx_a] is within S_a of p_a and pg_cell is
// monotone, so the cell of q lies in the face's registered box on every axis.
// (1) Its layer i* is walked: t is in [tlo, thi] = [t_min, t_max] cut to the
//     finite floats, the ray's point is the same monotone float32 expression
//     of t as p_kz, so p_kz lies between the points at tlo and thi exactly, and
//     fl(low - Sz') <= q_kz <= fl(high + Sz') since Sz' exceeds S_kz and the
//     roundings of that difference (2^-24 of the same magnitudes).
// (2) t is in layer i*'s interval: q_kz is in the layer up to the rounding of
//     the cell arithmetic and of the walls (each 2^-23 (|o_g| + |top|) at most),
//     the ray's exact point at t is within 2^-23 (|o| + |t d|) of p_kz, p_kz
//     within S_kz of q_kz, and t0, t1 are three float32 operations from the
//     exact parameters of the grown walls: in all less than 2^-19 + 5 * 2^-23 of
//     (|o| + |o_g| + |top|) against a slack of 2^-17 of it.
// (3) Its minor cells are visited: t is in [c0, c1], the minor coordinate is
//     again the definition's monotone expression, so p_kx lies between the two
//     end points exactly, and fl(low - Sx') <= fl(p_kx - Sx') <= q_kx likewise.
//     A skipped layer has high + Sx' < o_g <= mn or low - Sx' > top + Sx' >= mx
//     (the far corner is a rounding, not Sx', below the largest vertex): no q.
// (4) No stop precedes layer i*: t0 is monotone in the walk's order, t >= t0
//     of layer i* >= t0 of every layer walked before it, and the walk stops
//     only on best < t0 (strictly, so an equal t with a smaller face index is
//     still found) or t0 > thi >= t.
// Non-finite slack (coordinates near the float32 limit) walks every layer and
// every minor cell.  tests/test_raycast_cpu.py runs the model of exactly this
// walk against the brute force; docs/DESIGN_NOTEBOOK.md, section RC.
//
// No atomics, no LDS, nothing waits on another thread.  Every loop is bounded
// by the grid's dims or by n_pairs (offsets are clamped into [0, n_pairs]).  A
// lane writes its own ray's slots and nothing else.
#include "tri_ray.h"

namespace {

constexpr float RC_KT = 8.0f * PG_K;  // 2^-17: the traversal's slack

struct RayArgs {
  const float* __restrict__ origins;  // [n][3]
  const float* __restrict__ dirs;     // [n][3]
  const float* __restrict__ t_min;    // [n] or NULL: t_min_all
  const float* __restrict__ t_max;
  float t_min_all, t_max_all;
  const int32_t* __restrict__ order;  // [n] or NULL
  uint32_t n;
};

struct RayBest {
  float t;
  uint32_t face;
  float b0, b1, b2;
};

// the candidates of the cells lin0 .. lin1 of one row -> true: the any-hit form is done
template <bool ANY>
__device__ __forceinline__ bool rc_run(const float4* __restrict__ rec,
                                       const int32_t* __restrict__ offsets, uint32_t n,
                                       uint32_t lin0, uint32_t lin1, const TriRay& r, RayBest& b) {
  int32_t k0 = offsets[lin0], k1 = offsets[lin1 + 1u];
  k0 = k0 < 0 ? 0 : k0;
  k1 = k1 > (int32_t)n ? (int32_t)n : k1;
  for (int32_t k = k0; k < k1; ++k) {  // 0 <= k < n
    const float4 A = rec[3ull * (uint32_t)k], B = rec[3ull * (uint32_t)k + 1u],
                 C = rec[3ull * (uint32_t)k + 2u];
    float t;
    double U, V, W, det;
    if (!r.hit(A, B, C, t, U, V, W, det)) continue;
    const uint32_t j = __float_as_uint(A.w);
    if (t < b.t || (t == b.t && j < b.face)) {
      b.t = t;
      b.face = j;
      if (ANY) return true;
      b.b0 = (float)(U / det);
      b.b1 = (float)(V / det);
      b.b2 = (float)(W / det);
    }
  }
  return false;
}

template <bool ANY>
__device__ __forceinline__ void rc_walk(const float4* __restrict__ rec,
                                        const int32_t* __restrict__ offsets, uint32_t n,
                                        const GridArgs& g, const TriRay& r, RayBest& b) {
  const float h = g.cell;
  const int kz = r.kz;
  const float top0 = g.o[0] + (float)g.d[0] * h, top1 = g.o[1] + (float)g.d[1] * h,
              top2 = g.o[2] + (float)g.d[2] * h;
  const float S0 = RC_KT * ((fabsf(r.ox) + fabsf(g.o[0])) + fabsf(top0));
  const float S1 = RC_KT * ((fabsf(r.oy) + fabsf(g.o[1])) + fabsf(top1));
  const float S2 = RC_KT * ((fabsf(r.oz) + fabsf(g.o[2])) + fabsf(top2));
  const bool wide = !pg_finite3(S0, S1, S2);
  // the major axis, then the two minor ones (kx, ky)
  const float oz = r.okz, dz = rc_sel(kz, r.dx, r.dy, r.dz), gz = rc_sel(kz, g.o[0], g.o[1], g.o[2]),
              Sz = rc_sel(kz, S0, S1, S2);
  const float ox = r.okx, dx = rc_sel(kz, r.dy, r.dz, r.dx), gx = rc_sel(kz, g.o[1], g.o[2], g.o[0]),
              Sx = rc_sel(kz, S1, S2, S0), tx = rc_sel(kz, top1, top2, top0);
  const float oy = r.oky, dy = rc_sel(kz, r.dz, r.dx, r.dy), gy = rc_sel(kz, g.o[2], g.o[0], g.o[1]),
              Sy = rc_sel(kz, S2, S0, S1), ty = rc_sel(kz, top2, top0, top1);
  const uint32_t nz = kz == 0 ? g.d[0] : (kz == 1 ? g.d[1] : g.d[2]);
  const uint32_t nx = kz == 0 ? g.d[1] : (kz == 1 ? g.d[2] : g.d[0]);
  const uint32_t ny = kz == 0 ? g.d[2] : (kz == 1 ? g.d[0] : g.d[1]);
  const float tlo = fmaxf(r.tmin, -FLT_MAX), thi = fminf(r.tmax, FLT_MAX);
  const float za = oz + tlo * dz, zb = oz + thi * dz;
  int32_t ia = (int32_t)pg_cell(((fminf(za, zb) - Sz) - gz) / h, nz);
  int32_t ib = (int32_t)pg_cell(((fmaxf(za, zb) + Sz) - gz) / h, nz);
  if (wide) {
    ia = 0;
    ib = (int32_t)nz - 1;
  }
  const bool fwd = dz > 0.0f;
  const uint32_t gdy = g.d[1], gdz = g.d[2];
  // ia <= i <= ib < nz: at most nz passes
  for (int32_t i = fwd ? ia : ib; i >= ia && i <= ib; i += fwd ? 1 : -1) {
    const float zl = gz + (float)i * h, zh = gz + (float)(i + 1) * h;
    const float tA = ((zl - Sz) - oz) / dz, tB = ((zh + Sz) - oz) / dz;
    const float t0 = fminf(tA, tB), t1 = fmaxf(tA, tB);
    if (b.t < t0 || t0 > thi) break;  // no later layer can win
    const float c0 = fmaxf(t0, tlo), c1 = fminf(t1, thi);
    if (c0 > c1) continue;
    const float xa = ox + c0 * dx, xb = ox + c1 * dx;
    const float xl = fminf(xa, xb) - Sx, xh = fmaxf(xa, xb) + Sx;
    const float ya = oy + c0 * dy, yb = oy + c1 * dy;
    const float yl = fminf(ya, yb) - Sy, yh = fmaxf(ya, yb) + Sy;
    if (!wide && (xh < gx || xl > tx + Sx || yh < gy || yl > ty + Sy)) continue;
    const uint32_t cx0 = wide ? 0u : pg_cell((xl - gx) / h, nx);
    const uint32_t cx1 = wide ? nx - 1u : pg_cell((xh - gx) / h, nx);
    const uint32_t cy0 = wide ? 0u : pg_cell((yl - gy) / h, ny);
    const uint32_t cy1 = wide ? ny - 1u : pg_cell((yh - gy) / h, ny);
    // back to the grid's axes: kz = 0: (i, x, y), 1: (y, i, x), 2: (x, y, i)
    const uint32_t ui = (uint32_t)i;
    const uint32_t X0 = kz == 0 ? ui : (kz == 1 ? cy0 : cx0), X1 = kz == 0 ? ui : (kz == 1 ? cy1 : cx1);
    const uint32_t Y0 = kz == 0 ? cx0 : (kz == 1 ? ui : cy0), Y1 = kz == 0 ? cx1 : (kz == 1 ? ui : cy1);
    const uint32_t Z0 = kz == 0 ? cy0 : (kz == 1 ? cx0 : ui), Z1 = kz == 0 ? cy1 : (kz == 1 ? cx1 : ui);
    // every index is a pg_cell of its axis or a layer of it: inside the grid
    for (uint32_t x = X0; x <= X1; ++x)
      for (uint32_t y = Y0; y <= Y1; ++y) {
        const uint32_t row = (x * gdy + y) * gdz;
        if (rc_run<ANY>(rec, offsets, n, row + Z0, row + Z1, r, b)) return;
      }
  }
}

template <bool ANY>
__global__ void __launch_bounds__(PG_THREADS) k_raycast(const float4* __restrict__ rec,
                                                        const int32_t* __restrict__ offsets,
                                                        uint32_t n, GridArgs g, RayArgs a,
                                                        int32_t* __restrict__ face,
                                                        float* __restrict__ t_out,
                                                        float* __restrict__ bary,
                                                        uint8_t* __restrict__ occluded) {
  const uint32_t lane = blockIdx.x * PG_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  const uint32_t qi = a.order ? (uint32_t)a.order[lane] : lane;  // a negative entry is >= 2^31
  if (qi >= a.n) return;
  TriRay r;
  r.init(a.origins + 3ull * qi, a.dirs + 3ull * qi, a.t_min ? a.t_min[qi] : a.t_min_all,
         a.t_max ? a.t_max[qi] : a.t_max_all);
  RayBest b;
  b.t = INFINITY;
  b.face = PG_NONE;
  b.b0 = b.b1 = b.b2 = 0.0f;
  if (r.valid && n != 0) rc_walk<ANY>(rec, offsets, n, g, r, b);
  const bool hit = b.face != PG_NONE;
  if (ANY) {
    occluded[qi] = hit ? 1 : 0;
  } else {
    face[qi] = hit ? (int32_t)b.face : -1;
    t_out[qi] = hit ? b.t : INFINITY;
    bary[3ull * qi] = hit ? b.b0 : 0.0f;
    bary[3ull * qi + 1u] = hit ? b.b1 : 0.0f;
    bary[3ull * qi + 2u] = hit ? b.b2 : 0.0f;
  }
}

// the arguments the two entry points share, at the positions both give them
int32_t rc_args(const float* records, const int32_t* offsets, uint32_t n_pairs, const float* origin,
                float cell, const uint32_t* dims, const float* origins, const float* dirs,
                uint32_t n_rays, GridArgs& g) {
  UCSA_CHECK_ARG(n_pairs <= 0x7FFFFFFFu, 2);
  const int bad = pg_grid_args(origin, cell, dims, g);
  UCSA_CHECK_ARG(bad != 1, 3);
  UCSA_CHECK_ARG(bad != 2, 4);
  UCSA_CHECK_ARG(bad != 3, 5);
  UCSA_CHECK_ARG(n_rays <= 0x7FFFFFFFu, 13);
  if (n_rays == 0) return 0;
  UCSA_CHECK_ARG(origins, 6);
  UCSA_CHECK_ARG(dirs, 7);
  UCSA_CHECK_ARG(n_pairs == 0 || records, 0);
  UCSA_CHECK_ARG(n_pairs == 0 || offsets, 1);
  UCSA_CHECK_ARG(n_pairs == 0 || ((uintptr_t)records & 15u) == 0, 0);
  return 0;
}

}  // namespace

extern "C" int32_t ucsa_raycast_mesh(const float* records, const int32_t* offsets, uint32_t n_pairs,
                                     const float* origin, float cell, const uint32_t* dims,
                                     const float* origins, const float* dirs, const float* t_min,
                                     const float* t_max, float t_min_all, float t_max_all,
                                     const int32_t* order, uint32_t n_rays, int32_t* face, float* t,
                                     float* bary, void* stream) {
  GridArgs g;
  const int32_t st = rc_args(records, offsets, n_pairs, origin, cell, dims, origins, dirs, n_rays, g);
  if (st != 0 || n_rays == 0) return st;
  UCSA_CHECK_ARG(face, 14);
  UCSA_CHECK_ARG(t, 15);
  UCSA_CHECK_ARG(bary, 16);
  const RayArgs a = {origins, dirs, t_min, t_max, t_min_all, t_max_all, order, n_rays};
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_raycast<false>, dim3(ucsa_div_up(n_rays, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, (const float4*)records, offsets, n_pairs, g, a, face, t,
                     bary, (uint8_t*)nullptr);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_mesh_occluded(const float* records, const int32_t* offsets, uint32_t n_pairs,
                                      const float* origin, float cell, const uint32_t* dims,
                                      const float* origins, const float* dirs, const float* t_min,
                                      const float* t_max, float t_min_all, float t_max_all,
                                      const int32_t* order, uint32_t n_rays, uint8_t* occluded,
                                      void* stream) {
  GridArgs g;
  const int32_t st = rc_args(records, offsets, n_pairs, origin, cell, dims, origins, dirs, n_rays, g);
  if (st != 0 || n_rays == 0) return st;
  UCSA_CHECK_ARG(occluded, 14);
  const RayArgs a = {origins, dirs, t_min, t_max, t_min_all, t_max_all, order, n_rays};
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_raycast<true>, dim3(ucsa_div_up(n_rays, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, (const float4*)records, offsets, n_pairs, g, a,
                     (int32_t*)nullptr, (float*)nullptr, (float*)nullptr, occluded);
  return ucsa_launch_status();
}
