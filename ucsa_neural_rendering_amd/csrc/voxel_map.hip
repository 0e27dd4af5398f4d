// The voxel route of the mapping baseline (not in the reference): per-voxel class
// votes taken while depth is integrated (ucsa_tsdf_vote), their resolution to
// one label per voxel (ucsa_voxel_label_resolve) and a ray-caster over the TSDF
// volume (ucsa_tsdf_raycast).  The contracts are stated in include/ucsa_hip.h;
// tests/voxel_map_numpy.py restates them in numpy and the outputs match it bit
// for bit.
//
// k_tsdf_vote     k_tsdf_integrate's shape: one thread per voxel, a work-group
//                 per brick of 1 x 4 x 64 voxels, k across the lanes, the same
//                 brick cull (tsdf_project.h).  votes is class-major, so the
//                 lanes of a wave that vote for one class touch one line of one
//                 plane.  A thread keeps a pending (class, count) in registers
//                 through the views of a launch and flushes it (one uint16
//                 read-modify-write) when the class changes: a voxel that every
//                 view labels alike costs one flush per launch.
// k_voxel_resolve one thread per voxel, the planes read one after the other.
// k_tsdf_evidence the soft sibling of k_tsdf_vote (ucsa_tsdf_evidence), same
//                 bricks and cull: a voxel adds the row of C evidence bytes of
//                 its pixel to uint32 sums.  CT sums at a time live in
//                 registers through the views of a launch (CT = 8 or 40; for
//                 C > 40 the views are walked once per 40 classes, the first
//                 walk recording which views count) and go out as one
//                 saturating read-modify-write per plane, only for a voxel
//                 that a view reached.  A row is fetched as the aligned words
//                 that hold it and shifted into place.
// k_evidence_resolve  argmax, runner-up margin and view count per voxel.
// k_rc_mark       one work-group per brick of 8^3 cells, one thread per cell:
//                 marks[brick] = 1 iff a cell of it has eight valid corners, one
//                 of them <= RC_MARK_EPS.
// k_tsdf_raycast  one thread per pixel, a wave per 8x8 pixel patch, four
//                 patches per work-group.  Sample k+1 of one index is sample k
//                 of the next and is carried over.  With SKIP an index is
//                 evaluated only if one of its two samples lies in a marked
//                 brick: the walk through free and unobserved space costs a
//                 byte load from an L1-resident table per sample, not sixteen
//                 gathers.
// No atomics anywhere.
#include <cmath>

#include "tsdf_project.h"
#include "ucsa_common.h"

namespace {

constexpr uint32_t VM_BK = 64;    // the vote's brick: k = one wave
constexpr uint32_t VM_BJ = 4;     // j = waves per work-group
constexpr uint32_t VM_MAXB = 32;  // views per launch = VM_BK * VM_BJ / 8 corners

struct VoteArgs {
  uint16_t* votes;
  const float* depth;
  const uint8_t* pred;
  const float* poses;
  uint32_t nx, ny, nz, B, H, W, C;
  float o[3], h[3];
  float fx, fy, cx, cy, trunc, dmin, dmax;
};

__device__ __forceinline__ void vm_flush(uint16_t* __restrict__ plane0, size_t n, size_t idx,
                                         uint32_t cls, uint32_t cnt) {
  if (cnt == 0u) return;
  uint16_t* p = plane0 + (size_t)cls * n + idx;
  const uint32_t s = (uint32_t)*p + cnt;
  *p = (uint16_t)(s > 65535u ? 65535u : s);
}

__global__ void __launch_bounds__(VM_BK* VM_BJ) k_tsdf_vote(VoteArgs a) {
  __shared__ float s_c[VM_MAXB][8][3];
  __shared__ uint32_t s_cull;
  const uint32_t tid = threadIdx.y * VM_BK + threadIdx.x;
  const uint32_t i = blockIdx.z, j0 = blockIdx.y * VM_BJ, k0 = blockIdx.x * VM_BK;
  const uint32_t j1 = min(j0 + VM_BJ - 1u, a.ny - 1u), k1 = min(k0 + VM_BK - 1u, a.nz - 1u);
  float lo[3], hi[3];
  lo[0] = hi[0] = a.o[0] + (float)i * a.h[0];
  lo[1] = a.o[1] + (float)j0 * a.h[1];
  hi[1] = a.o[1] + (float)j1 * a.h[1];
  lo[2] = a.o[2] + (float)k0 * a.h[2];
  hi[2] = a.o[2] + (float)k1 * a.h[2];
#pragma unroll
  for (int r = 1; r < 3; ++r) {
    const float x = fminf(lo[r], hi[r]), y = fmaxf(lo[r], hi[r]);
    lo[r] = x;
    hi[r] = y;
  }
  if (tid == 0) s_cull = 0u;
  if (tid < 8u * a.B) {
    const uint32_t v = tid >> 3, q = tid & 7u;
    const float p[3] = {lo[0], (q & 1u) ? hi[1] : lo[1], (q & 2u) ? hi[2] : lo[2]};
    float c[3];
    ts_camera(a.poses + 16u * v, p, c);
    s_c[v][q][0] = c[0];
    s_c[v][q][1] = c[1];
    s_c[v][q][2] = c[2];
  }
  __syncthreads();
  if (tid < a.B && ts_cull(a, a.poses + 16u * tid, lo, hi, s_c[tid])) atomicOr(&s_cull, 1u << tid);
  __syncthreads();
  const uint32_t cull = s_cull;

  const uint32_t j = j0 + threadIdx.y, k = k0 + threadIdx.x;
  if (j >= a.ny || k >= a.nz) return;
  const size_t n = (size_t)a.nx * a.ny * a.nz;
  const size_t idx = ((size_t)i * a.ny + j) * a.nz + k;
  const float p[3] = {lo[0], a.o[1] + (float)j * a.h[1], a.o[2] + (float)k * a.h[2]};
  const float fW = (float)a.W, fH = (float)a.H;
  uint32_t cls = 0u, cnt = 0u;  // the pending votes
  for (uint32_t b = 0; b < a.B; ++b) {
    if ((cull >> b) & 1u) continue;  // uniform over the work-group
    float c[3];
    ts_camera(a.poses + 16u * b, p, c);
    if (!(c[2] > 0.0f)) continue;
    const float u = floorf((a.fx * c[0]) / c[2] + a.cx);
    const float v = floorf((a.fy * c[1]) / c[2] + a.cy);
    if (!(u >= 0.0f && u < fW && v >= 0.0f && v < fH)) continue;
    const size_t pix = ((size_t)b * a.H + (uint32_t)v) * a.W + (uint32_t)u;
    const float d = a.depth[pix];
    if (!(isfinite(d) && d >= a.dmin && d <= a.dmax)) continue;
    const float sdf = d - c[2];
    if (!(sdf >= -a.trunc && sdf <= a.trunc)) continue;
    const uint32_t pr = a.pred[pix];
    if (pr < 1u || pr > a.C) continue;
    if (pr != cls) {
      vm_flush(a.votes, n, idx, cls, cnt);
      cls = pr;
      cnt = 0u;
    }
    ++cnt;
  }
  vm_flush(a.votes, n, idx, cls, cnt);
}

__global__ void __launch_bounds__(256) k_voxel_resolve(const uint16_t* __restrict__ votes,
                                                        uint32_t C, uint64_t n,
                                                        uint32_t min_votes,
                                                        uint8_t* __restrict__ label,
                                                        uint32_t* __restrict__ total,
                                                        uint32_t* __restrict__ winner) {
  const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (x >= n) return;
  uint32_t sum = 0u, best = 0u, arg = 0u;
  for (uint32_t c = 1; c <= C; ++c) {
    const uint32_t s = votes[(uint64_t)c * n + x];
    sum += s;
    if (s > best || c == 1u) {
      best = s;
      arg = c;
    }
  }
  label[x] = (uint8_t)(sum >= min_votes ? arg : 0u);
  total[x] = sum;
  winner[x] = best;
}

// ---- evidence (soft votes) ---------------------------------------------------
struct EvArgs {
  uint32_t* ev;
  const float* depth;
  const uint8_t* scores;
  const float* poses;
  uint32_t nx, ny, nz, B, H, W, C;
  float o[3], h[3];
  float fx, fy, cx, cy, trunc, dmin, dmax;
};

__device__ __forceinline__ uint32_t ev_sat_add(uint32_t x, uint32_t y) {
  const uint32_t s = x + y;
  return s < x ? 0xFFFFFFFFu : s;
}

// the pixel that view b gives the voxel at p under k_tsdf_vote's rule; false: none
__device__ __forceinline__ bool ev_pixel(const EvArgs& a, uint32_t b, const float p[3],
                                         size_t& pix) {
  float c[3];
  ts_camera(a.poses + 16u * b, p, c);
  if (!(c[2] > 0.0f)) return false;
  const float u = floorf((a.fx * c[0]) / c[2] + a.cx);
  const float v = floorf((a.fy * c[1]) / c[2] + a.cy);
  if (!(u >= 0.0f && u < (float)a.W && v >= 0.0f && v < (float)a.H)) return false;
  pix = ((size_t)b * a.H + (uint32_t)v) * a.W + (uint32_t)u;
  const float d = a.depth[pix];
  if (!(isfinite(d) && d >= a.dmin && d <= a.dmax)) return false;
  const float sdf = d - c[2];
  return sdf >= -a.trunc && sdf <= a.trunc;
}

// Bytes [0, nc) of `row` (any alignment), nc <= 4*NW, as NW words with the
// bytes past nc zeroed.  Only the aligned words that hold a byte of the row are
// loaded, so nothing outside the words the row lives in is touched.
template <uint32_t NW>
__device__ __forceinline__ void ev_row(const uint8_t* row, uint32_t nc, const uint32_t msk[NW],
                                       uint32_t w[NW]) {
  const uintptr_t at = (uintptr_t)row;
  const uint32_t sh = (uint32_t)(at & 3u);
  const uint32_t* __restrict__ q = (const uint32_t*)(at - sh);
  const uint32_t end = sh + nc;  // bytes from q to the row's end
  uint32_t d[NW + 1];
#pragma unroll
  for (uint32_t i = 0; i <= NW; ++i) d[i] = 4u * i < end ? q[i] : 0u;
#pragma unroll
  for (uint32_t i = 0; i < NW; ++i)
    w[i] = (uint32_t)((((uint64_t)d[i + 1] << 32) | d[i]) >> (8u * sh)) & msk[i];
}

// is any of the bytes [0, n) of `row` non-zero?
__device__ __forceinline__ bool ev_any(const uint8_t* row, uint32_t n) {
  const uintptr_t at = (uintptr_t)row;
  const uint32_t sh = (uint32_t)(at & 3u);
  const uint32_t* __restrict__ q = (const uint32_t*)(at - sh);
  const uint32_t end = sh + n, words = (end + 3u) >> 2;
  uint32_t any = 0u;
  for (uint32_t i = 0; i < words; ++i) {
    uint32_t x = q[i];
    if (i == 0u) x &= 0xFFFFFFFFu << (8u * sh);
    if (i + 1u == words && (end & 3u)) x &= 0xFFFFFFFFu >> (8u * (4u - (end & 3u)));
    any |= x;
  }
  return any != 0u;
}

// CT: classes carried in registers at a time (a multiple of 4)
template <uint32_t CT>
__global__ void __launch_bounds__(VM_BK* VM_BJ) k_tsdf_evidence(EvArgs a) {
  constexpr uint32_t NW = CT / 4u;
  __shared__ float s_c[VM_MAXB][8][3];
  __shared__ uint32_t s_cull;
  const uint32_t tid = threadIdx.y * VM_BK + threadIdx.x;
  const uint32_t i = blockIdx.z, j0 = blockIdx.y * VM_BJ, k0 = blockIdx.x * VM_BK;
  const uint32_t j1 = min(j0 + VM_BJ - 1u, a.ny - 1u), k1 = min(k0 + VM_BK - 1u, a.nz - 1u);
  float lo[3], hi[3];
  lo[0] = hi[0] = a.o[0] + (float)i * a.h[0];
  lo[1] = a.o[1] + (float)j0 * a.h[1];
  hi[1] = a.o[1] + (float)j1 * a.h[1];
  lo[2] = a.o[2] + (float)k0 * a.h[2];
  hi[2] = a.o[2] + (float)k1 * a.h[2];
#pragma unroll
  for (int r = 1; r < 3; ++r) {
    const float x = fminf(lo[r], hi[r]), y = fmaxf(lo[r], hi[r]);
    lo[r] = x;
    hi[r] = y;
  }
  if (tid == 0) s_cull = 0u;
  if (tid < 8u * a.B) {
    const uint32_t v = tid >> 3, q = tid & 7u;
    const float p[3] = {lo[0], (q & 1u) ? hi[1] : lo[1], (q & 2u) ? hi[2] : lo[2]};
    float c[3];
    ts_camera(a.poses + 16u * v, p, c);
    s_c[v][q][0] = c[0];
    s_c[v][q][1] = c[1];
    s_c[v][q][2] = c[2];
  }
  __syncthreads();
  if (tid < a.B && ts_cull(a, a.poses + 16u * tid, lo, hi, s_c[tid])) atomicOr(&s_cull, 1u << tid);
  __syncthreads();
  const uint32_t cull = s_cull;

  const uint32_t j = j0 + threadIdx.y, k = k0 + threadIdx.x;
  if (j >= a.ny || k >= a.nz) return;
  const size_t n = (size_t)a.nx * a.ny * a.nz;
  const size_t idx = ((size_t)i * a.ny + j) * a.nz + k;
  const float p[3] = {lo[0], a.o[1] + (float)j * a.h[1], a.o[2] + (float)k * a.h[2]};
  uint32_t took = 0u;  // bit b: view b's row is added (set in the first pass)
  for (uint32_t c0 = 0; c0 < a.C; c0 += CT) {  // uniform over the grid
    const uint32_t nc = min(CT, a.C - c0);
    uint32_t msk[NW];
#pragma unroll
    for (uint32_t q = 0; q < NW; ++q) {
      const uint32_t r = nc > 4u * q ? nc - 4u * q : 0u;
      msk[q] = r >= 4u ? 0xFFFFFFFFu : (1u << (8u * r)) - 1u;
    }
    uint32_t acc[CT];
#pragma unroll
    for (uint32_t c = 0; c < CT; ++c) acc[c] = 0u;
    for (uint32_t b = 0; b < a.B; ++b) {
      if ((cull >> b) & 1u) continue;  // uniform over the work-group
      if (c0 != 0u && !((took >> b) & 1u)) continue;
      size_t pix;
      if (!ev_pixel(a, b, p, pix)) continue;
      const uint8_t* row = a.scores + pix * a.C;
      uint32_t w[NW];
      ev_row<NW>(row + c0, nc, msk, w);
      if (c0 == 0u) {
        uint32_t any = 0u;
#pragma unroll
        for (uint32_t q = 0; q < NW; ++q) any |= w[q];
        if (any == 0u && !(a.C > CT && ev_any(row + CT, a.C - CT))) continue;  // abstains
        took |= 1u << b;
      }
#pragma unroll
      for (uint32_t c = 0; c < CT; ++c) acc[c] += (w[c >> 2] >> (8u * (c & 3u))) & 0xFFu;
    }
    if (took == 0u) return;  // no view of the launch reaches the voxel: not touched
    uint32_t* __restrict__ e = a.ev + (size_t)(c0 + 1u) * n + idx;
#pragma unroll
    for (uint32_t c = 0; c < CT; ++c)
      if (c < nc) e[(size_t)c * n] = ev_sat_add(e[(size_t)c * n], acc[c]);
  }
  a.ev[idx] = ev_sat_add(a.ev[idx], (uint32_t)__popc(took));
}

__global__ void __launch_bounds__(256) k_evidence_resolve(const uint32_t* __restrict__ ev,
                                                           uint32_t C, uint64_t n,
                                                           uint32_t min_views,
                                                           uint32_t min_margin,
                                                           uint8_t* __restrict__ label,
                                                           uint32_t* __restrict__ views,
                                                           uint32_t* __restrict__ best_out,
                                                           uint32_t* __restrict__ margin) {
  const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (x >= n) return;
  uint32_t best = ev[n + x], second = 0u, arg = 1u;
  for (uint32_t c = 2; c <= C; ++c) {
    const uint32_t s = ev[(uint64_t)c * n + x];
    if (s > best) {
      second = best;
      best = s;
      arg = c;
    } else if (s > second) {
      second = s;
    }
  }
  const uint32_t nv = ev[x], m = best - second;
  label[x] = (uint8_t)(nv >= min_views && m >= min_margin ? arg : 0u);
  views[x] = nv;
  best_out[x] = best;
  margin[x] = m;
}

// ---- ray-caster ------------------------------------------------------------
constexpr uint32_t RC_BRICK = 8;           // cells per brick and axis
constexpr float RC_MARK_EPS = 1.52587890625e-05f;  // 2^-16
constexpr uint32_t RC_MAXK = 1u << 20;

struct RcArgs {
  const float* tsdf;
  const float* weight;
  const float* rgb;
  const uint8_t* labels;
  const float* poses;
  uint8_t* marks;
  float* depth;
  int32_t* vid;
  float* normal;
  float* rgb_out;
  int32_t* label;
  uint32_t nx, ny, nz, H, W;
  uint32_t nbx, nby, nbz;  // bricks per axis
  float o[3], h[3];
  float fx, fy, cx, cy, near, far, step, min_weight;
};

__global__ void __launch_bounds__(512) k_rc_mark(RcArgs a) {
  const uint32_t t = threadIdx.x;
  const uint32_t ci = blockIdx.z * RC_BRICK + (t >> 6), cj = blockIdx.y * RC_BRICK + ((t >> 3) & 7u),
                 ck = blockIdx.x * RC_BRICK + (t & 7u);
  int hit = 0;
  if (ci + 1u < a.nx && cj + 1u < a.ny && ck + 1u < a.nz) {
    const size_t base = ((size_t)ci * a.ny + cj) * a.nz + ck;
    const size_t sj = a.nz, si = (size_t)a.ny * a.nz;
    bool valid = true, low = false;
#pragma unroll
    for (uint32_t q = 0; q < 8u; ++q) {
      const size_t at = base + ((q & 4u) ? si : 0) + ((q & 2u) ? sj : 0) + (q & 1u);
      valid = valid && a.weight[at] >= a.min_weight;
      low = low || a.tsdf[at] <= RC_MARK_EPS;
    }
    hit = valid && low;
  }
  hit = __syncthreads_or(hit);
  if (t == 0)
    a.marks[((size_t)blockIdx.z * a.nby + blockIdx.y) * a.nbz + blockIdx.x] = hit ? 1 : 0;
}

struct RcCell {
  size_t base;  // index of corner (0,0,0)
  float f[3];
};

__device__ __forceinline__ RcCell rc_cell(const RcArgs& a, const float q0[3], const float qd[3],
                                          float z, uint32_t c[3]) {
  const uint32_t n[3] = {a.nx, a.ny, a.nz};
  RcCell r;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float g = q0[k] + z * qd[k];
    const float top = (float)(n[k] - 2u);
    float fl = floorf(g);
    fl = fl < 0.0f ? 0.0f : (fl > top ? top : fl);
    c[k] = (uint32_t)fl;
    r.f[k] = fminf(fmaxf(g - fl, 0.0f), 1.0f);
  }
  r.base = ((size_t)c[0] * a.ny + c[1]) * a.nz + c[2];
  return r;
}

__device__ __forceinline__ bool rc_marked(const RcArgs& a, const uint32_t c[3]) {
  return a.marks[((size_t)(c[0] / RC_BRICK) * a.nby + c[1] / RC_BRICK) * a.nbz +
                 c[2] / RC_BRICK] != 0;
}

// v[4*i + 2*j + k] of the cell's corners, `stride` floats per lattice point
__device__ __forceinline__ void rc_corners(const RcArgs& a, const float* __restrict__ src,
                                           size_t base, uint32_t stride, float v[8]) {
  const size_t sj = a.nz, si = (size_t)a.ny * a.nz;
#pragma unroll
  for (uint32_t q = 0; q < 8u; ++q)
    v[q] = src[(base + ((q & 4u) ? si : 0) + ((q & 2u) ? sj : 0) + (q & 1u)) * stride];
}

__device__ __forceinline__ float rc_lerp(float x, float y, float f) { return x + f * (y - x); }

__device__ __forceinline__ float rc_trilerp(const float v[8], const float f[3]) {
  const float c00 = rc_lerp(v[0], v[1], f[2]), c01 = rc_lerp(v[2], v[3], f[2]);
  const float c10 = rc_lerp(v[4], v[5], f[2]), c11 = rc_lerp(v[6], v[7], f[2]);
  return rc_lerp(rc_lerp(c00, c01, f[1]), rc_lerp(c10, c11, f[1]), f[0]);
}

// do all eight corners of the cell have weight >= min_weight?
__device__ __forceinline__ bool rc_valid(const RcArgs& a, const RcCell& cell) {
  float w[8];
  rc_corners(a, a.weight, cell.base, 1u, w);
  bool valid = true;
#pragma unroll
  for (int q = 0; q < 8; ++q) valid = valid && w[q] >= a.min_weight;
  return valid;
}

// the sample at z: its value, or valid = false when a corner is unobserved
__device__ __forceinline__ float rc_sample(const RcArgs& a, const RcCell& cell, bool& valid) {
  valid = rc_valid(a, cell);
  if (!valid) return 0.0f;
  float v[8];
  rc_corners(a, a.tsdf, cell.base, 1u, v);
  return rc_trilerp(v, cell.f);
}

template <bool SKIP>
__global__ void __launch_bounds__(256) k_tsdf_raycast(RcArgs a) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t x = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
  const uint32_t y = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
  const uint32_t b = blockIdx.z;
  if (x >= a.W || y >= a.H) return;
  const size_t pix = ((size_t)b * a.H + y) * a.W + x;
  const float* __restrict__ P = a.poses + 16u * (size_t)b;

  const float d0 = (((float)x + 0.5f) - a.cx) / a.fx;
  const float d1 = (((float)y + 0.5f) - a.cy) / a.fy;
  const uint32_t n[3] = {a.nx, a.ny, a.nz};
  float q0[3], qd[3];
  float z_in = a.near, z_out = a.far;
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float w = (P[4 * r] * d0 + P[4 * r + 1] * d1) + P[4 * r + 2];
    q0[r] = (P[4 * r + 3] - a.o[r]) / a.h[r];
    qd[r] = w / a.h[r];
    const float top = (float)(n[r] - 1u);
    ok = ok && isfinite(q0[r]) && isfinite(qd[r]);
    if (qd[r] == 0.0f) {
      ok = ok && q0[r] >= 0.0f && q0[r] <= top;
    } else {
      const float z1 = (0.0f - q0[r]) / qd[r], z2 = (top - q0[r]) / qd[r];
      const float lo = z1 < z2 ? z1 : z2, hi = z1 < z2 ? z2 : z1;
      z_in = lo > z_in ? lo : z_in;
      z_out = hi < z_out ? hi : z_out;
    }
  }
  const float dz = a.step / sqrtf((d0 * d0 + d1 * d1) + 1.0f);
  ok = ok && z_in <= z_out && isfinite(z_in) && isfinite(z_out) && dz > 0.0f && isfinite(dz);

  float zh = 0.0f;
  bool found = false;
  if (ok) {
    // sample k: carried over from the previous index when that was evaluated
    uint32_t have = 0xFFFFFFFFu;
    float f_have = 0.0f;
    bool v_have = false;
    uint32_t c1[3];
    RcCell cell1 = rc_cell(a, q0, qd, z_in, c1);
    bool m1 = SKIP ? rc_marked(a, c1) : true;
    float zk1 = z_in;
    for (uint32_t k = 0; k + 1u < RC_MAXK; ++k) {
      const float zk = zk1;
      const RcCell cell0 = cell1;
      const bool m0 = m1;
      zk1 = z_in + (float)(k + 1u) * dz;
      if (!(zk1 <= z_out)) break;
      cell1 = rc_cell(a, q0, qd, zk1, c1);
      m1 = SKIP ? rc_marked(a, c1) : true;
      if (!(m0 || m1)) continue;
      float f0;
      bool v0;
      if (have == k) {
        f0 = f_have;
        v0 = v_have;
      } else {
        f0 = rc_sample(a, cell0, v0);
      }
      bool v1;
      const float f1 = rc_sample(a, cell1, v1);
      have = k + 1u;
      f_have = f1;
      v_have = v1;
      if (v0 && v1 && f0 > 0.0f && f1 <= 0.0f) {
        float z = zk + dz * (f0 / (f0 - f1));
        z = z < zk ? zk : (z > zk1 ? zk1 : z);
        // a crossing whose own cell has an unobserved corner is no hit
        uint32_t ch[3];
        if (rc_valid(a, rc_cell(a, q0, qd, z, ch))) {
          zh = z;
          found = true;
          break;
        }
      }
    }
  }

  float nrm[3] = {0.0f, 0.0f, 0.0f}, col[3] = {0.0f, 0.0f, 0.0f};
  int32_t vid = -1, lab = 0;
  if (found) {
    uint32_t c[3];
    const RcCell cell = rc_cell(a, q0, qd, zh, c);
    uint32_t id[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float g = q0[r] + zh * qd[r];
      const float top = (float)(n[r] - 1u);
      float q = rintf(g);
      q = q < 0.0f ? 0.0f : (q > top ? top : q);
      id[r] = (uint32_t)q;
    }
    vid = (int32_t)((id[0] * a.ny + id[1]) * a.nz + id[2]);
    if (a.labels) lab = (int32_t)a.labels[(uint32_t)vid];
    if (a.normal) {
      float v[8];
      rc_corners(a, a.tsdf, cell.base, 1u, v);
      const float* f = cell.f;
      const float c00 = rc_lerp(v[0], v[1], f[2]), c01 = rc_lerp(v[2], v[3], f[2]);
      const float c10 = rc_lerp(v[4], v[5], f[2]), c11 = rc_lerp(v[6], v[7], f[2]);
      const float c_0 = rc_lerp(c00, c01, f[1]), c_1 = rc_lerp(c10, c11, f[1]);
      float G[3];
      G[0] = c_1 - c_0;
      G[1] = rc_lerp(c01 - c00, c11 - c10, f[0]);
      G[2] = rc_lerp(rc_lerp(v[1] - v[0], v[3] - v[2], f[1]),
                     rc_lerp(v[5] - v[4], v[7] - v[6], f[1]), f[0]);
#pragma unroll
      for (int r = 0; r < 3; ++r) G[r] = G[r] / a.h[r];
      const float len = sqrtf((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
      if (len > 0.0f && isfinite(len)) {
#pragma unroll
        for (int r = 0; r < 3; ++r) nrm[r] = G[r] / len;
      }
    }
    if (a.rgb_out) {
#pragma unroll
      for (uint32_t ch = 0; ch < 3u; ++ch) {
        float v[8];
        rc_corners(a, a.rgb + ch, cell.base, 3u, v);
        col[ch] = rc_trilerp(v, cell.f);
      }
    }
  }
  a.depth[pix] = zh;
  a.vid[pix] = vid;
  if (a.label) a.label[pix] = lab;
  if (a.normal) {
#pragma unroll
    for (int r = 0; r < 3; ++r) a.normal[3 * pix + r] = nrm[r];
  }
  if (a.rgb_out) {
#pragma unroll
    for (int r = 0; r < 3; ++r) a.rgb_out[3 * pix + r] = col[r];
  }
}

}  // namespace

extern "C" int32_t ucsa_tsdf_vote(uint16_t* votes, uint64_t votes_capacity, uint32_t C,
                                  uint32_t nx, uint32_t ny, uint32_t nz, const float* origin3,
                                  const float* spacing3, const float* depth,
                                  const uint8_t* pred, const float* poses, uint32_t B, float fx,
                                  float fy, float cx, float cy, uint32_t H, uint32_t W,
                                  float trunc, float depth_min, float depth_max,
                                  void* stream) {
  UCSA_CHECK_ARG(votes, 0);
  UCSA_CHECK_ARG(C >= 1 && C <= 255, 2);
  UCSA_CHECK_ARG(nx >= 2 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 3);
  UCSA_CHECK_ARG(ny >= 2, 4);
  UCSA_CHECK_ARG(nz >= 2, 5);
  const uint64_t need = (uint64_t)(C + 1u) * ((uint64_t)nx * ny * nz);
  UCSA_CHECK_ARG(need <= (1ull << 40) && votes_capacity >= need, 1);
  UCSA_CHECK_ARG(origin3, 6);
  UCSA_CHECK_ARG(spacing3, 7);
  UCSA_CHECK_ARG(depth, 8);
  UCSA_CHECK_ARG(pred, 9);
  UCSA_CHECK_ARG(poses, 10);
  UCSA_CHECK_ARG(B >= 1, 11);
  UCSA_CHECK_ARG(fx > 0.0f && std::isfinite(fx), 12);
  UCSA_CHECK_ARG(fy > 0.0f && std::isfinite(fy), 13);
  UCSA_CHECK_ARG(std::isfinite(cx), 14);
  UCSA_CHECK_ARG(std::isfinite(cy), 15);
  UCSA_CHECK_ARG(H >= 1 && H <= 16384, 16);
  UCSA_CHECK_ARG(W >= 1 && W <= 16384, 17);
  UCSA_CHECK_ARG(trunc > 0.0f && std::isfinite(trunc), 18);
  UCSA_CHECK_ARG(!std::isnan(depth_min), 19);
  UCSA_CHECK_ARG(depth_max >= depth_min, 20);
  const uint32_t gy = ucsa_div_up(ny, VM_BJ);
  UCSA_CHECK_ARG(gy <= 65535u, 4);
  UCSA_CHECK_ARG(nx <= 65535u, 3);
  VoteArgs a;
  a.votes = votes;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.H = H;
  a.W = W;
  a.C = C;
  for (int r = 0; r < 3; ++r) {
    a.o[r] = origin3[r];
    a.h[r] = spacing3[r];
  }
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.trunc = trunc;
  a.dmin = depth_min;
  a.dmax = depth_max;
  const dim3 grid(ucsa_div_up(nz, VM_BK), gy, nx), block(VM_BK, VM_BJ);
  hipStream_t s = (hipStream_t)stream;
  UCSA_CLEAR_ERR();
  for (uint32_t b0 = 0; b0 < B; b0 += VM_MAXB) {
    a.B = B - b0 < VM_MAXB ? B - b0 : VM_MAXB;
    a.depth = depth + (size_t)b0 * H * W;
    a.pred = pred + (size_t)b0 * H * W;
    a.poses = poses + 16 * (size_t)b0;
    hipLaunchKernelGGL(k_tsdf_vote, grid, block, 0, s, a);
  }
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_voxel_label_resolve(const uint16_t* votes, uint32_t C,
                                            uint64_t n_voxels, uint32_t min_votes,
                                            uint8_t* label, uint32_t* total, uint32_t* winner,
                                            uint64_t max_voxels, void* stream) {
  UCSA_CHECK_ARG(votes, 0);
  UCSA_CHECK_ARG(C >= 1 && C <= 255, 1);
  UCSA_CHECK_ARG(n_voxels <= 0x7FFFFFFFull, 2);
  UCSA_CHECK_ARG(min_votes >= 1, 3);
  UCSA_CHECK_ARG(label, 4);
  UCSA_CHECK_ARG(total, 5);
  UCSA_CHECK_ARG(winner, 6);
  UCSA_CHECK_ARG(max_voxels >= n_voxels, 7);
  if (n_voxels == 0) return 0;
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_voxel_resolve, dim3(ucsa_div_up(n_voxels, 256)), dim3(256), 0,
                     (hipStream_t)stream, votes, C, n_voxels, min_votes, label, total, winner);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_tsdf_evidence(uint32_t* evidence, uint64_t evidence_capacity, uint32_t C,
                                      uint32_t nx, uint32_t ny, uint32_t nz,
                                      const float* origin3, const float* spacing3,
                                      const float* depth, const uint8_t* scores,
                                      const float* poses, uint32_t B, float fx, float fy,
                                      float cx, float cy, uint32_t H, uint32_t W, float trunc,
                                      float depth_min, float depth_max, void* stream) {
  UCSA_CHECK_ARG(evidence, 0);
  UCSA_CHECK_ARG(C >= 1 && C <= 255, 2);
  UCSA_CHECK_ARG(nx >= 2 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 3);
  UCSA_CHECK_ARG(ny >= 2, 4);
  UCSA_CHECK_ARG(nz >= 2, 5);
  const uint64_t need = (uint64_t)(C + 1u) * ((uint64_t)nx * ny * nz);
  UCSA_CHECK_ARG(need <= (1ull << 40) && evidence_capacity >= need, 1);
  UCSA_CHECK_ARG(origin3, 6);
  UCSA_CHECK_ARG(spacing3, 7);
  UCSA_CHECK_ARG(depth, 8);
  UCSA_CHECK_ARG(scores, 9);
  UCSA_CHECK_ARG(poses, 10);
  UCSA_CHECK_ARG(B >= 1, 11);
  UCSA_CHECK_ARG(fx > 0.0f && std::isfinite(fx), 12);
  UCSA_CHECK_ARG(fy > 0.0f && std::isfinite(fy), 13);
  UCSA_CHECK_ARG(std::isfinite(cx), 14);
  UCSA_CHECK_ARG(std::isfinite(cy), 15);
  UCSA_CHECK_ARG(H >= 1 && H <= 16384, 16);
  UCSA_CHECK_ARG(W >= 1 && W <= 16384, 17);
  UCSA_CHECK_ARG((uint64_t)B * H * W * C <= (1ull << 40), 9);
  UCSA_CHECK_ARG(trunc > 0.0f && std::isfinite(trunc), 18);
  UCSA_CHECK_ARG(!std::isnan(depth_min), 19);
  UCSA_CHECK_ARG(depth_max >= depth_min, 20);
  const uint32_t gy = ucsa_div_up(ny, VM_BJ);
  UCSA_CHECK_ARG(gy <= 65535u, 4);
  UCSA_CHECK_ARG(nx <= 65535u, 3);
  EvArgs a;
  a.ev = evidence;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.H = H;
  a.W = W;
  a.C = C;
  for (int r = 0; r < 3; ++r) {
    a.o[r] = origin3[r];
    a.h[r] = spacing3[r];
  }
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.trunc = trunc;
  a.dmin = depth_min;
  a.dmax = depth_max;
  const dim3 grid(ucsa_div_up(nz, VM_BK), gy, nx), block(VM_BK, VM_BJ);
  hipStream_t s = (hipStream_t)stream;
  UCSA_CLEAR_ERR();
  for (uint32_t b0 = 0; b0 < B; b0 += VM_MAXB) {
    a.B = B - b0 < VM_MAXB ? B - b0 : VM_MAXB;
    a.depth = depth + (size_t)b0 * H * W;
    a.scores = scores + (size_t)b0 * H * W * C;
    a.poses = poses + 16 * (size_t)b0;
    if (C <= 8u)
      hipLaunchKernelGGL(k_tsdf_evidence<8>, grid, block, 0, s, a);
    else
      hipLaunchKernelGGL(k_tsdf_evidence<40>, grid, block, 0, s, a);
  }
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_voxel_evidence_resolve(const uint32_t* evidence, uint32_t C,
                                               uint64_t n_voxels, uint32_t min_views,
                                               uint32_t min_margin, uint8_t* label,
                                               uint32_t* views, uint32_t* best,
                                               uint32_t* margin, uint64_t max_voxels,
                                               void* stream) {
  UCSA_CHECK_ARG(evidence, 0);
  UCSA_CHECK_ARG(C >= 1 && C <= 255, 1);
  UCSA_CHECK_ARG(n_voxels <= 0x7FFFFFFFull, 2);
  UCSA_CHECK_ARG(min_views >= 1, 3);
  UCSA_CHECK_ARG(label, 5);
  UCSA_CHECK_ARG(views, 6);
  UCSA_CHECK_ARG(best, 7);
  UCSA_CHECK_ARG(margin, 8);
  UCSA_CHECK_ARG(max_voxels >= n_voxels, 9);
  if (n_voxels == 0) return 0;
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_evidence_resolve, dim3(ucsa_div_up(n_voxels, 256)), dim3(256), 0,
                     (hipStream_t)stream, evidence, C, n_voxels, min_views, min_margin, label,
                     views, best, margin);
  return ucsa_launch_status();
}

extern "C" uint64_t ucsa_tsdf_raycast_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
  if (nx < 2 || ny < 2 || nz < 2) return 0;
  const uint64_t bricks = (uint64_t)ucsa_div_up(nx - 1u, RC_BRICK) *
                          ucsa_div_up(ny - 1u, RC_BRICK) * ucsa_div_up(nz - 1u, RC_BRICK);
  return (bricks + 255u) & ~(uint64_t)255u;
}

extern "C" int32_t ucsa_tsdf_raycast(const float* tsdf, const float* weight, const float* rgb,
                                     const uint8_t* voxel_labels, uint32_t nx, uint32_t ny,
                                     uint32_t nz, const float* origin3, const float* spacing3,
                                     const float* poses, uint32_t B, float fx, float fy,
                                     float cx, float cy, uint32_t H, uint32_t W, float near,
                                     float far, float trunc, float step, float min_weight,
                                     float* depth, int32_t* voxel_id, float* normal,
                                     float* rgb_out, int32_t* label, uint64_t max_pixels,
                                     void* workspace, uint64_t workspace_bytes, uint32_t flags,
                                     void* stream) {
  UCSA_CHECK_ARG(tsdf, 0);
  UCSA_CHECK_ARG(weight, 1);
  UCSA_CHECK_ARG((rgb == nullptr) == (rgb_out == nullptr), rgb ? 25 : 2);
  UCSA_CHECK_ARG((voxel_labels == nullptr) == (label == nullptr), voxel_labels ? 26 : 3);
  UCSA_CHECK_ARG(nx >= 2 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 4);
  UCSA_CHECK_ARG(ny >= 2, 5);
  UCSA_CHECK_ARG(nz >= 2, 6);
  UCSA_CHECK_ARG(origin3, 7);
  UCSA_CHECK_ARG(spacing3, 8);
  for (int r = 0; r < 3; ++r) {
    UCSA_CHECK_ARG(std::isfinite(origin3[r]), 7);
    UCSA_CHECK_ARG(std::isfinite(spacing3[r]) && spacing3[r] != 0.0f, 8);
  }
  UCSA_CHECK_ARG(poses, 9);
  UCSA_CHECK_ARG(B >= 1 && B <= 65535, 10);
  UCSA_CHECK_ARG(fx > 0.0f && std::isfinite(fx), 11);
  UCSA_CHECK_ARG(fy > 0.0f && std::isfinite(fy), 12);
  UCSA_CHECK_ARG(std::isfinite(cx), 13);
  UCSA_CHECK_ARG(std::isfinite(cy), 14);
  UCSA_CHECK_ARG(H >= 1 && H <= 16384, 15);
  UCSA_CHECK_ARG(W >= 1 && W <= 16384, 16);
  UCSA_CHECK_ARG(near > 0.0f && std::isfinite(near), 17);
  UCSA_CHECK_ARG(far >= near && std::isfinite(far), 18);
  UCSA_CHECK_ARG(trunc > 0.0f && std::isfinite(trunc), 19);
  UCSA_CHECK_ARG(step > 0.0f && step < trunc, 20);
  UCSA_CHECK_ARG(min_weight > 0.0f && std::isfinite(min_weight), 21);
  UCSA_CHECK_ARG(depth, 22);
  UCSA_CHECK_ARG(voxel_id, 23);
  UCSA_CHECK_ARG(max_pixels >= (uint64_t)B * H * W, 27);
  UCSA_CHECK_ARG((flags & ~UCSA_RAYCAST_PLAIN_MARCH) == 0u, 30);
  const bool skip = !(flags & UCSA_RAYCAST_PLAIN_MARCH);
  if (skip) {
    UCSA_CHECK_ARG(workspace, 28);
    UCSA_CHECK_ARG(workspace_bytes >= ucsa_tsdf_raycast_workspace_bytes(nx, ny, nz), 29);
  }
  RcArgs a;
  a.tsdf = tsdf;
  a.weight = weight;
  a.rgb = rgb;
  a.labels = voxel_labels;
  a.poses = poses;
  a.marks = skip ? (uint8_t*)workspace : nullptr;
  a.depth = depth;
  a.vid = voxel_id;
  a.normal = normal;
  a.rgb_out = rgb_out;
  a.label = label;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.H = H;
  a.W = W;
  a.nbx = ucsa_div_up(nx - 1u, RC_BRICK);
  a.nby = ucsa_div_up(ny - 1u, RC_BRICK);
  a.nbz = ucsa_div_up(nz - 1u, RC_BRICK);
  for (int r = 0; r < 3; ++r) {
    a.o[r] = origin3[r];
    a.h[r] = spacing3[r];
  }
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.near = near;
  a.far = far;
  a.step = step;
  a.min_weight = min_weight;
  // the mark grid's y and z stay below 65536 only if the brick counts do
  UCSA_CHECK_ARG(a.nbx <= 65535u, 4);
  UCSA_CHECK_ARG(a.nby <= 65535u, 5);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ucsa_div_up(W, 16u), ucsa_div_up(H, 16u), B);
  UCSA_CLEAR_ERR();
  if (skip) {
    hipLaunchKernelGGL(k_rc_mark, dim3(a.nbz, a.nby, a.nbx), dim3(512), 0, s, a);
    hipLaunchKernelGGL(k_tsdf_raycast<true>, grid, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(k_tsdf_raycast<false>, grid, dim3(256), 0, s, a);
  }
  return ucsa_launch_status();
}
