// Mesh rasterization (ucsa_raster_setup / ucsa_raster_draw): a labelled
// triangle mesh seen from posed pinhole cameras -> per-pixel face id, z-depth,
// NYU40 label and colour.  Not in the reference; it renders the meshes of the
// mesh export (and ScanNet's labelled meshes) into the project's 2D frames.
// The contract (cameras, clipping, snapping, fill rule, depth, attributes) is
// stated in include/ucsa_hip.h; tests/raster_numpy.py restates it in numpy and
// the GPU output matches it bit for bit.
//
// Schedule (TILE = 16x16 pixels, one record per (view, face)):
//   k_rs_setup     one thread per (view, face): transform, clip, project,
//                  snap; a 128-byte record, the number of tiles its snapped
//                  bounding box touches, and 4 integer atomic adds into a 2D
//                  difference grid of per-tile counts (so the setup of a
//                  screen-filling face is O(1), not O(tiles));
//   k_rs_block     exclusive scan of the per-record tile counts inside blocks
//                  of 1024 records, block sums;
//   k_rs_scan      ONE work-group: scan of the block sums (64-bit), 2D prefix
//                  sums of the difference grid (= per-tile counts), exclusive
//                  scan over the tiles; the pair total to the caller;
//   k_rs_emit      one thread per (tile, record) pair, found by binary search
//                  in the record scan: a slot in its tile's list through an
//                  integer atomic on a per-tile cursor (the order inside a
//                  list does not matter: the winner is a minimum);
//   k_rs_tile      one work-group per tile: records staged through LDS, one
//                  lane per pixel keeps the minimum 64-bit key (z bits, face),
//                  then resolves its pixel's attributes and writes every output.
// No z-buffer in HBM, no 64-bit atomics, no float atomics: two runs give the
// same bytes.  Workspace: 132 bytes per (view, face), 8 per 1024 of them, and
// 12 bytes per (view, tile) plus one row and column of the difference grid.
#include <cmath>

#include "ucsa_common.h"

namespace {

constexpr uint32_t RS_TILE = 16;
constexpr uint32_t RS_TILE_PIX = RS_TILE * RS_TILE;
constexpr uint32_t RS_MAXP = 8;      // polygon vertices a record holds
constexpr uint32_t RS_WORK = 12;     // clipping scratch (only rounding exceeds 8)
constexpr uint32_t RS_BLOCK = 1024;  // records per block of the record scan
constexpr uint32_t RS_SCAN_THREADS = 1024;
constexpr uint32_t RS_REC_WORDS = 32;  // 128 bytes
constexpr uint32_t RS_LDS_WORDS = 25;  // words 0..23 staged, odd stride
constexpr uint32_t RS_MAX_DIM = 16384;
constexpr float RS_GUARD = 65536.0f;   // guard band, pixels beyond each border
constexpr float RS_CLAMP = 2097152.0f; // 2^21 px: |snapped| < 2^29

// record words: 0..7 snapped x, 8..15 snapped y, 16..18 plane normal n,
// 19 n.c0, 20 zlo, 21 zhi, 22 face id, 23 nv | fan flags << 8,
// 24 tx0 | ty0 << 16, 25 tx1 | ty1 << 16 (tile box, inclusive), 26..31 unused.

struct RsCam {
  float fx, fy, cx, cy, near;
  float kL, kR, kT, kB;  // guard-band plane constants
  uint32_t H, W, tX, tY;
};

struct RsLayout {
  uint64_t rec, foff, boff, grid, toff, cur, total;
};

inline uint64_t rs_al(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

RsLayout rs_layout(uint64_t BF, uint32_t B, uint32_t tX, uint32_t tY) {
  RsLayout l;
  const uint64_t nblk = (BF + RS_BLOCK - 1) / RS_BLOCK;
  const uint64_t tiles = (uint64_t)B * tX * tY;
  uint64_t o = 0;
  l.rec = o;  o = rs_al(o + BF * RS_REC_WORDS * 4);
  l.foff = o; o = rs_al(o + BF * 4);
  l.boff = o; o = rs_al(o + nblk * 8);
  l.grid = o; o = rs_al(o + (uint64_t)B * (tX + 1) * (tY + 1) * 4);
  l.toff = o; o = rs_al(o + tiles * 4);
  l.cur = o;  o = rs_al(o + tiles * 4);
  l.total = o;
  return l;
}

__device__ __forceinline__ void rs_cam(const float* __restrict__ P,
                                       const float* __restrict__ v, float c[3]) {
  const float d0 = v[0] - P[3], d1 = v[1] - P[7], d2 = v[2] - P[11];
#pragma unroll
  for (int r = 0; r < 3; ++r) c[r] = (d0 * P[r] + d1 * P[4 + r]) + d2 * P[8 + r];
}

__device__ __forceinline__ float rs_plane(const RsCam& k, int p, float x, float y,
                                          float z) {
  switch (p) {
    case 0: return z - k.near;
    case 1: return x * k.fx + z * k.kL;
    case 2: return z * k.kR - x * k.fx;
    case 3: return y * k.fy + z * k.kT;
    default: return z * k.kB - y * k.fy;
  }
}

__device__ __forceinline__ void rs_cross(const float a[3], const float b[3], float o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ float rs_dot(const float a[3], const float b[3]) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__device__ __forceinline__ bool rs_finite3(const float c[3]) {
  return isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]);
}

// the three camera-space corners of face f (false: index out of range)
__device__ __forceinline__ bool rs_corners(const float* __restrict__ verts, uint32_t V,
                                           const int32_t* __restrict__ faces, uint32_t f,
                                           const float* __restrict__ P, float c[3][3],
                                           uint32_t idx[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    idx[k] = (uint32_t)faces[(size_t)f * 3 + k];
    if (idx[k] >= V) return false;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) rs_cam(P, verts + (size_t)idx[k] * 3, c[k]);
  return true;
}

__device__ __forceinline__ int64_t rs_edge(int32_t px, int32_t py, int32_t qx, int32_t qy,
                                           int32_t x, int32_t y) {
  return (int64_t)(qx - px) * (int64_t)(y - py) - (int64_t)(qy - py) * (int64_t)(x - px);
}

// edge P->Q of a positively oriented triangle owns the points on it
__device__ __forceinline__ bool rs_owns(int32_t px, int32_t py, int32_t qx, int32_t qy) {
  const int32_t dy = qy - py, dx = qx - px;
  return dy > 0 || (dy == 0 && dx < 0);
}

__device__ __forceinline__ bool rs_in_edge(int32_t px, int32_t py, int32_t qx, int32_t qy,
                                           int32_t x, int32_t y) {
  const int64_t e = rs_edge(px, py, qx, qy, x, y);
  return e > 0 || (e == 0 && rs_owns(px, py, qx, qy));
}

__global__ void __launch_bounds__(256)
k_rs_setup(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ faces,
           uint32_t F, const float* __restrict__ poses, uint32_t BF, RsCam k,
           uint32_t* __restrict__ rec, uint32_t* __restrict__ ntile,
           uint32_t* __restrict__ grid) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= BF) return;
  const uint32_t b = r / F, f = r - b * F;
  ntile[r] = 0;
  const float* P = poses + (size_t)b * 16;
  float c[3][3];
  uint32_t idx[3];
  if (!rs_corners(verts, V, faces, f, P, c, idx)) return;
  if (!(rs_finite3(c[0]) && rs_finite3(c[1]) && rs_finite3(c[2]))) return;

  bool all_in = true;
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    int n_out = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) n_out += !(rs_plane(k, p, c[q][0], c[q][1], c[q][2]) >= 0.0f);
    if (n_out == 3) return;  // wholly outside one plane: nothing to draw
    all_in = all_in && n_out == 0;
  }

  float vx[RS_WORK], vy[RS_WORK], vz[RS_WORK];
  uint32_t n = 3;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    vx[q] = c[q][0];
    vy[q] = c[q][1];
    vz[q] = c[q][2];
  }
  if (!all_in) {
    // Sutherland-Hodgman against near, left, right, top, bottom.  A vertex
    // carries the mask of the corners it lies between; a new vertex on an
    // original edge is computed from that edge's corners, lower vertex index
    // first, so that the faces sharing the edge get the same bits.
    uint32_t vm[RS_WORK], wm[RS_WORK];
    float wx[RS_WORK], wy[RS_WORK], wz[RS_WORK];
    for (int q = 0; q < 3; ++q) vm[q] = 1u << q;
    for (int p = 0; p < 5 && n > 0; ++p) {
      uint32_t m = 0;
      for (uint32_t i = 0; i < n; ++i) {
        const uint32_t j = i + 1 == n ? 0 : i + 1;
        const float sA = rs_plane(k, p, vx[i], vy[i], vz[i]);
        const float sB = rs_plane(k, p, vx[j], vy[j], vz[j]);
        const bool inA = sA >= 0.0f, inB = sB >= 0.0f;
        if (inA) {
          if (m < RS_WORK) {
            wx[m] = vx[i]; wy[m] = vy[i]; wz[m] = vz[i]; wm[m] = vm[i];
          }
          ++m;
        }
        if (inA != inB) {
          const uint32_t um = vm[i] | vm[j];
          float Px, Py, Pz, Qx, Qy, Qz, sP, sQ;
          uint32_t om;
          if (__popc(um) == 2) {
            const uint32_t a = __ffs(um) - 1, bb = __ffs(um & (um - 1)) - 1;
            const uint32_t lo = idx[a] <= idx[bb] ? a : bb, hi = lo == a ? bb : a;
            Px = c[lo][0]; Py = c[lo][1]; Pz = c[lo][2];
            Qx = c[hi][0]; Qy = c[hi][1]; Qz = c[hi][2];
            sP = rs_plane(k, p, Px, Py, Pz);
            sQ = rs_plane(k, p, Qx, Qy, Qz);
            om = um;
          } else {
            Px = vx[i]; Py = vy[i]; Pz = vz[i];
            Qx = vx[j]; Qy = vy[j]; Qz = vz[j];
            sP = sA;
            sQ = sB;
            om = 7u;
          }
          float t = sP / (sP - sQ);
          if (!(t >= 0.0f)) t = 0.0f;
          if (t > 1.0f) t = 1.0f;
          if (m < RS_WORK) {
            wx[m] = Px + t * (Qx - Px);
            wy[m] = Py + t * (Qy - Py);
            wz[m] = Pz + t * (Qz - Pz);
            wm[m] = om;
          }
          ++m;
        }
      }
      if (m > RS_WORK) return;
      for (uint32_t i = 0; i < m; ++i) {
        vx[i] = wx[i]; vy[i] = wy[i]; vz[i] = wz[i]; vm[i] = wm[i];
      }
      n = m;
    }
    if (n < 3 || n > RS_MAXP) return;
  }

  // project, clamp, snap to 1/256 px (round half to even)
  int32_t sx[RS_MAXP], sy[RS_MAXP];
  float zmin = vz[0], zmax = vz[0];
  int32_t x0 = 0x7FFFFFFF, x1 = -0x7FFFFFFF, y0 = 0x7FFFFFFF, y1 = -0x7FFFFFFF;
#pragma unroll
  for (uint32_t i = 0; i < RS_MAXP; ++i) {
    if (i >= n) break;
    float u = k.fx * (vx[i] / vz[i]) + k.cx;
    float v = k.fy * (vy[i] / vz[i]) + k.cy;
    if (!(u >= -RS_CLAMP)) u = -RS_CLAMP;
    if (u > RS_CLAMP) u = RS_CLAMP;
    if (!(v >= -RS_CLAMP)) v = -RS_CLAMP;
    if (v > RS_CLAMP) v = RS_CLAMP;
    sx[i] = (int32_t)rintf(u * 256.0f);
    sy[i] = (int32_t)rintf(v * 256.0f);
    x0 = min(x0, sx[i]); x1 = max(x1, sx[i]);
    y0 = min(y0, sy[i]); y1 = max(y1, sy[i]);
    zmin = vz[i] < zmin ? vz[i] : zmin;
    zmax = vz[i] > zmax ? vz[i] : zmax;
  }
  uint32_t flags = 0;
#pragma unroll
  for (uint32_t t = 0; t + 2 < RS_MAXP; ++t) {
    if (t + 2 >= n) break;
    const int64_t area = rs_edge(sx[0], sy[0], sx[t + 1], sy[t + 1], sx[t + 2], sy[t + 2]);
    flags |= (area != 0 ? 1u : 0u) << (2 * t);
    flags |= (area < 0 ? 1u : 0u) << (2 * t + 1);
  }
  if (flags == 0) return;  // zero area: covers nothing
  // pixel centres x*256+128 inside [x0, x1]
  int32_t px0 = (x0 - 128 + 255) >> 8, px1 = (x1 - 128) >> 8;
  int32_t py0 = (y0 - 128 + 255) >> 8, py1 = (y1 - 128) >> 8;
  px0 = max(px0, 0); py0 = max(py0, 0);
  px1 = min(px1, (int32_t)k.W - 1); py1 = min(py1, (int32_t)k.H - 1);
  if (px0 > px1 || py0 > py1) return;
  const uint32_t tx0 = px0 / RS_TILE, tx1 = px1 / RS_TILE;
  const uint32_t ty0 = py0 / RS_TILE, ty1 = py1 / RS_TILE;

  float e1[3], e2[3], nn[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    e1[q] = c[1][q] - c[0][q];
    e2[q] = c[2][q] - c[0][q];
  }
  rs_cross(e1, e2, nn);
  const float zlo = zmin < k.near ? k.near : zmin;
  const float zhi = zmax < zlo ? zlo : zmax;

  uint32_t w[26];
  for (uint32_t i = 0; i < RS_MAXP; ++i) {
    w[i] = i < n ? (uint32_t)sx[i] : 0u;
    w[8 + i] = i < n ? (uint32_t)sy[i] : 0u;
  }
  w[16] = __float_as_uint(nn[0]);
  w[17] = __float_as_uint(nn[1]);
  w[18] = __float_as_uint(nn[2]);
  w[19] = __float_as_uint(rs_dot(nn, c[0]));
  w[20] = __float_as_uint(zlo);
  w[21] = __float_as_uint(zhi);
  w[22] = f;
  w[23] = n | (flags << 8);
  w[24] = tx0 | (ty0 << 16);
  w[25] = tx1 | (ty1 << 16);
  uint4* dst = (uint4*)(rec + (size_t)r * RS_REC_WORDS);
#pragma unroll
  for (int q = 0; q < 6; ++q) dst[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  dst[6] = make_uint4(w[24], w[25], 0u, 0u);
  ntile[r] = (tx1 - tx0 + 1) * (ty1 - ty0 + 1);
  // +1 on the tile box in the difference grid (wrapping uint32 arithmetic)
  uint32_t* g = grid + (size_t)b * (k.tX + 1) * (k.tY + 1);
  const uint32_t gw = k.tX + 1;
  atomicAdd(g + ty0 * gw + tx0, 1u);
  atomicAdd(g + ty0 * gw + tx1 + 1, 0xFFFFFFFFu);
  atomicAdd(g + (ty1 + 1) * gw + tx0, 0xFFFFFFFFu);
  atomicAdd(g + (ty1 + 1) * gw + tx1 + 1, 1u);
}

// exclusive scan of the tile counts inside blocks of RS_BLOCK records (in
// place), block sums
__global__ void __launch_bounds__(RS_BLOCK)
k_rs_block(uint32_t* __restrict__ foff, uint32_t BF, uint64_t* __restrict__ bsum) {
  __shared__ uint32_t sh[RS_BLOCK];
  const uint32_t t = threadIdx.x, r = blockIdx.x * RS_BLOCK + t;
  const uint32_t v = r < BF ? foff[r] : 0u;
  sh[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < RS_BLOCK; d <<= 1) {
    const uint32_t a = t >= d ? sh[t - d] : 0u;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  if (r < BF) foff[r] = sh[t] - v;
  if (t == RS_BLOCK - 1) bsum[blockIdx.x] = sh[t];
}

// exclusive scan of n uint64 values (in place) by one work-group; returns the
// sum to every thread
__device__ uint64_t rs_wg_scan_u64(uint64_t* __restrict__ a, uint32_t n, uint64_t* sh) {
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n + RS_SCAN_THREADS - 1) / RS_SCAN_THREADS;
  const uint32_t lo = min(n, t * per), hi = min(n, lo + per);
  uint64_t s = 0;
  for (uint32_t i = lo; i < hi; ++i) s += a[i];
  sh[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < RS_SCAN_THREADS; d <<= 1) {
    const uint64_t x = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  uint64_t run = sh[t] - s;
  const uint64_t total = sh[RS_SCAN_THREADS - 1];
  for (uint32_t i = lo; i < hi; ++i) {
    const uint64_t x = a[i];
    a[i] = run;
    run += x;
  }
  __syncthreads();
  return total;
}

__global__ void __launch_bounds__(RS_SCAN_THREADS)
k_rs_scan(uint64_t* __restrict__ boff, uint32_t nblk, uint32_t* __restrict__ grid,
          uint32_t B, uint32_t tX, uint32_t tY, uint32_t* __restrict__ toff,
          uint64_t* __restrict__ total_dev) {
  __shared__ uint64_t sh[RS_SCAN_THREADS];
  const uint32_t t = threadIdx.x;
  const uint64_t total = rs_wg_scan_u64(boff, nblk, sh);
  const uint32_t gw = tX + 1, gh = tY + 1;
  // difference grid -> per-tile counts: prefix along x, then along y
  for (uint32_t i = t; i < B * gh; i += RS_SCAN_THREADS) {
    uint32_t* row = grid + (size_t)i * gw;
    uint32_t s = 0;
    for (uint32_t x = 0; x < gw; ++x) row[x] = (s += row[x]);
  }
  __syncthreads();
  for (uint32_t i = t; i < B * gw; i += RS_SCAN_THREADS) {
    const uint32_t b = i / gw, x = i - b * gw;
    uint32_t* col = grid + (size_t)b * gw * gh + x;
    uint32_t s = 0;
    for (uint32_t y = 0; y < gh; ++y) col[(size_t)y * gw] = (s += col[(size_t)y * gw]);
  }
  __syncthreads();
  // exclusive scan over the tiles in (view, row, column) order
  const uint32_t n = B * tX * tY;
  const uint32_t per = (n + RS_SCAN_THREADS - 1) / RS_SCAN_THREADS;
  const uint32_t lo = min(n, t * per), hi = min(n, lo + per);
  uint64_t s = 0;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t b = i / (tX * tY), q = i - b * tX * tY, y = q / tX, x = q - y * tX;
    s += grid[((size_t)b * gh + y) * gw + x];
  }
  sh[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < RS_SCAN_THREADS; d <<= 1) {
    const uint64_t x = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  uint64_t run = sh[t] - s;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t b = i / (tX * tY), q = i - b * tX * tY, y = q / tX, x = q - y * tX;
    toff[i] = (uint32_t)run;
    run += grid[((size_t)b * gh + y) * gw + x];
  }
  if (t == 0) total_dev[0] = total;
}

__device__ __forceinline__ uint32_t rs_tile_count(const uint32_t* __restrict__ grid,
                                                  const RsCam& k, uint32_t b, uint32_t ty,
                                                  uint32_t tx) {
  return grid[((size_t)b * (k.tY + 1) + ty) * (k.tX + 1) + tx];
}

__global__ void __launch_bounds__(256)
k_rs_emit(const uint32_t* __restrict__ rec, const uint32_t* __restrict__ foff,
          const uint64_t* __restrict__ boff, uint32_t nblk, uint32_t BF, uint32_t F,
          RsCam k, const uint32_t* __restrict__ grid, const uint32_t* __restrict__ toff,
          uint32_t* __restrict__ cursor, uint32_t total, uint32_t* __restrict__ pairs,
          uint64_t max_pairs) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  // the block: last i with boff[i] <= p
  uint32_t lo = 0, hi = nblk;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (boff[mid] <= p) lo = mid; else hi = mid;
  }
  const uint32_t kk = p - (uint32_t)boff[lo];
  // the record: last r of the block with foff[r] <= kk (a record with no tile
  // shares its offset with the next one and is never the last)
  uint32_t rl = lo * RS_BLOCK, rh = min(BF, rl + RS_BLOCK);
  while (rh - rl > 1) {
    const uint32_t mid = (rl + rh) >> 1;
    if (foff[mid] <= kk) rl = mid; else rh = mid;
  }
  const uint32_t r = rl, j = kk - foff[r];
  const uint32_t* R = rec + (size_t)r * RS_REC_WORDS;
  const uint32_t a0 = R[24], a1 = R[25];
  const uint32_t tx0 = a0 & 0xFFFF, ty0 = a0 >> 16, tx1 = a1 & 0xFFFF, ty1 = a1 >> 16;
  const uint32_t bw = tx1 - tx0 + 1;
  if (j >= bw * (ty1 - ty0 + 1)) return;
  const uint32_t tx = tx0 + j % bw, ty = ty0 + j / bw, b = r / F;
  const uint32_t t = (b * k.tY + ty) * k.tX + tx;
  const uint32_t slot = atomicAdd(cursor + t, 1u);
  const uint64_t at = (uint64_t)toff[t] + slot;
  if (slot < rs_tile_count(grid, k, b, ty, tx) && at < max_pairs) pairs[at] = r;
}

__global__ void __launch_bounds__(RS_TILE_PIX)
k_rs_tile(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ faces,
          uint32_t F, uint32_t BF,
          const float* __restrict__ poses, const int32_t* __restrict__ vlab,
          const float* __restrict__ vrgb, RsCam k, const uint32_t* __restrict__ rec,
          const uint32_t* __restrict__ grid, const uint32_t* __restrict__ toff,
          const uint32_t* __restrict__ pairs, uint64_t max_pairs,
          int32_t* __restrict__ tri_id, float* __restrict__ depth,
          int32_t* __restrict__ label, float* __restrict__ rgb) {
  __shared__ uint32_t sh[RS_TILE_PIX * RS_LDS_WORDS];
  const uint32_t tid = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y, b = blockIdx.z;
  const uint32_t x = tx * RS_TILE + (tid & (RS_TILE - 1)), y = ty * RS_TILE + tid / RS_TILE;
  const bool on = x < k.W && y < k.H;
  const uint32_t t = (b * k.tY + ty) * k.tX + tx;
  const uint32_t start = toff[t], cnt = rs_tile_count(grid, k, b, ty, tx);
  const int32_t PX = (int32_t)(x * 256 + 128), PY = (int32_t)(y * 256 + 128);
  const float dx = ((float)x + 0.5f - k.cx) / k.fx;
  const float dy = ((float)y + 0.5f - k.cy) / k.fy;
  uint64_t best = ~0ull;
  for (uint32_t c0 = 0; c0 < cnt; c0 += RS_TILE_PIX) {
    const uint32_t m = min(RS_TILE_PIX, cnt - c0);
    __syncthreads();
    if (tid < m) {
      const uint64_t at = (uint64_t)start + c0 + tid;
      uint32_t* d = sh + tid * RS_LDS_WORDS;
      const uint32_t r = at < max_pairs ? pairs[at] : 0xFFFFFFFFu;
      if (r < BF) {
        const uint4* s = (const uint4*)(rec + (size_t)r * RS_REC_WORDS);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const uint4 v = s[q];
          d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
        }
      } else {
        d[23] = 0u;  // nothing
      }
    }
    __syncthreads();
    if (!on) continue;
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t* R = sh + j * RS_LDS_WORDS;
      const uint32_t nvf = R[23], nv = min(nvf & 0xFFu, RS_MAXP), fl = nvf >> 8;
      const int32_t ax = (int32_t)R[0], ay = (int32_t)R[8];
      bool cov = false;
      for (uint32_t q = 0; q + 2 < nv && !cov; ++q) {
        const uint32_t f2 = fl >> (2 * q);
        if (!(f2 & 1u)) continue;
        int32_t bx = (int32_t)R[q + 1], by = (int32_t)R[8 + q + 1];
        int32_t cx = (int32_t)R[q + 2], cy = (int32_t)R[8 + q + 2];
        if (f2 & 2u) {
          const int32_t ux = bx, uy = by;
          bx = cx; by = cy; cx = ux; cy = uy;
        }
        cov = rs_in_edge(ax, ay, bx, by, PX, PY) && rs_in_edge(bx, by, cx, cy, PX, PY) &&
              rs_in_edge(cx, cy, ax, ay, PX, PY);
      }
      if (!cov) continue;
      const float n0 = __uint_as_float(R[16]), n1 = __uint_as_float(R[17]);
      const float n2 = __uint_as_float(R[18]);
      const float zlo = __uint_as_float(R[20]), zhi = __uint_as_float(R[21]);
      float z = __uint_as_float(R[19]) / ((n0 * dx + n1 * dy) + n2);
      if (!isfinite(z)) z = zhi;
      if (z < zlo) z = zlo;
      if (z > zhi) z = zhi;
      const uint64_t key = ((uint64_t)__float_as_uint(z) << 32) | R[22];
      best = key < best ? key : best;
    }
  }
  if (!on) return;
  const size_t o = ((size_t)b * k.H + y) * k.W + x;
  const uint32_t f = (uint32_t)best;
  float c[3][3];
  uint32_t idx[3];
  if (best == ~0ull || f >= F ||
      !rs_corners(verts, V, faces, f, poses + (size_t)b * 16, c, idx)) {
    tri_id[o] = -1;
    depth[o] = 0.0f;
    label[o] = 0;
    if (rgb) {
      rgb[o * 3] = 0.0f; rgb[o * 3 + 1] = 0.0f; rgb[o * 3 + 2] = 0.0f;
    }
    return;
  }
  const float z = __uint_as_float((uint32_t)(best >> 32));
  // perspective-correct barycentrics of the hit point h = z*(dx, dy, 1)
  float e1[3], e2[3], nn[3], q[3], a[3], bb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    e1[i] = c[1][i] - c[0][i];
    e2[i] = c[2][i] - c[0][i];
  }
  rs_cross(e1, e2, nn);
  q[0] = z * dx - c[0][0];
  q[1] = z * dy - c[0][1];
  q[2] = z - c[0][2];
  rs_cross(q, e2, a);
  rs_cross(e1, q, bb);
  const float nsq = rs_dot(nn, nn);
  float w1 = rs_dot(nn, a) / nsq, w2 = rs_dot(nn, bb) / nsq;
  float w0 = (1.0f - w1) - w2;
  if (!(isfinite(w0) && isfinite(w1) && isfinite(w2))) {
    w0 = 1.0f; w1 = 0.0f; w2 = 0.0f;
  }
  const uint32_t corner = (w0 >= w1 && w0 >= w2) ? 0u : (w1 >= w2 ? 1u : 2u);
  tri_id[o] = (int32_t)f;
  depth[o] = z;
  label[o] = vlab ? vlab[idx[corner]] : 0;
  if (rgb) {
    const float* r0 = vrgb + (size_t)idx[0] * 3;
    const float* r1 = vrgb + (size_t)idx[1] * 3;
    const float* r2 = vrgb + (size_t)idx[2] * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) rgb[o * 3 + i] = (w0 * r0[i] + w1 * r1[i]) + w2 * r2[i];
  }
}

bool rs_cam_host(float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                 float near, RsCam* k) {
  k->fx = fx; k->fy = fy; k->cx = cx; k->cy = cy; k->near = near;
  // fp32 on the host as in the numpy restatement
  const float g = RS_GUARD;
  k->kL = cx + g;
  k->kR = ((float)W + g) - cx;
  k->kT = cy + g;
  k->kB = ((float)H + g) - cy;
  k->H = H; k->W = W;
  k->tX = (W + RS_TILE - 1) / RS_TILE;
  k->tY = (H + RS_TILE - 1) / RS_TILE;
  return true;
}

}  // namespace

#define RS_COMMON_CHECKS()                                                        \
  UCSA_CHECK_ARG(B >= 1 && B <= 65535, 5);                                        \
  UCSA_CHECK_ARG((uint64_t)B * F <= 0x7FFFFFFFull, 3);                            \
  UCSA_CHECK_ARG(F == 0 || faces, 2);                                             \
  UCSA_CHECK_ARG(V == 0 || verts, 0);                                             \
  UCSA_CHECK_ARG(poses, 4);                                                       \
  UCSA_CHECK_ARG(std::isfinite(fx) && fx > 0.0f, 6);                              \
  UCSA_CHECK_ARG(std::isfinite(fy) && fy > 0.0f, 7);                              \
  UCSA_CHECK_ARG(std::isfinite(cx), 8);                                           \
  UCSA_CHECK_ARG(std::isfinite(cy), 9);                                           \
  UCSA_CHECK_ARG(H >= 1 && H <= RS_MAX_DIM, 10);                                  \
  UCSA_CHECK_ARG(W >= 1 && W <= RS_MAX_DIM, 11);                                  \
  UCSA_CHECK_ARG(std::isfinite(near) && near > 0.0f, 12)

extern "C" uint64_t ucsa_raster_workspace_bytes(uint32_t B, uint32_t F, uint32_t H,
                                                uint32_t W) {
  const uint32_t tX = (W + RS_TILE - 1) / RS_TILE, tY = (H + RS_TILE - 1) / RS_TILE;
  return rs_layout((uint64_t)B * F, B, tX, tY).total;
}

extern "C" int32_t ucsa_raster_setup(const float* verts, uint32_t V, const int32_t* faces,
                                     uint32_t F, const float* poses, uint32_t B, float fx,
                                     float fy, float cx, float cy, uint32_t H, uint32_t W,
                                     float near, void* workspace, uint64_t* total_dev,
                                     void* stream) {
  RS_COMMON_CHECKS();
  UCSA_CHECK_ARG(workspace, 13);
  UCSA_CHECK_ARG(total_dev, 14);
  RsCam k;
  rs_cam_host(fx, fy, cx, cy, H, W, near, &k);
  const uint32_t BF = B * F;
  const RsLayout l = rs_layout(BF, B, k.tX, k.tY);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t nblk = ucsa_div_up(BF, RS_BLOCK);
  UCSA_CLEAR_ERR();
  hipError_t e = hipMemsetAsync(ws + l.grid, 0, l.total - l.grid, s);
  if (e != hipSuccess) return -(int32_t)e;
  if (BF > 0) {
    hipLaunchKernelGGL(k_rs_setup, dim3(ucsa_div_up(BF, 256)), dim3(256), 0, s, verts, V,
                       faces, F, poses, BF, k, (uint32_t*)(ws + l.rec),
                       (uint32_t*)(ws + l.foff), (uint32_t*)(ws + l.grid));
    hipLaunchKernelGGL(k_rs_block, dim3(nblk), dim3(RS_BLOCK), 0, s,
                       (uint32_t*)(ws + l.foff), BF, (uint64_t*)(ws + l.boff));
  }
  hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(RS_SCAN_THREADS), 0, s,
                     (uint64_t*)(ws + l.boff), nblk, (uint32_t*)(ws + l.grid), B, k.tX, k.tY,
                     (uint32_t*)(ws + l.toff), total_dev);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_raster_draw(const float* verts, uint32_t V, const int32_t* faces,
                                    uint32_t F, const float* poses, uint32_t B, float fx,
                                    float fy, float cx, float cy, uint32_t H, uint32_t W,
                                    float near, const int32_t* vertex_labels,
                                    const float* vertex_rgb, void* workspace,
                                    uint32_t* pairs, uint64_t total_pairs,
                                    uint64_t max_pairs, int32_t* tri_id, float* depth,
                                    int32_t* label, float* rgb, uint64_t max_pixels,
                                    void* stream) {
  RS_COMMON_CHECKS();
  UCSA_CHECK_ARG(workspace, 15);
  UCSA_CHECK_ARG(pairs || total_pairs == 0, 16);
  UCSA_CHECK_ARG(total_pairs <= 0x7FFFFFFFull && ((uint64_t)B * F > 0 || total_pairs == 0), 17);
  UCSA_CHECK_ARG(total_pairs <= max_pairs, 18);
  UCSA_CHECK_ARG(tri_id, 19);
  UCSA_CHECK_ARG(depth, 20);
  UCSA_CHECK_ARG(label, 21);
  UCSA_CHECK_ARG(rgb || !vertex_rgb, 22);
  UCSA_CHECK_ARG(max_pixels >= (uint64_t)B * H * W, 23);
  RsCam k;
  rs_cam_host(fx, fy, cx, cy, H, W, near, &k);
  const uint32_t BF = B * F;
  const RsLayout l = rs_layout(BF, B, k.tX, k.tY);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t nblk = ucsa_div_up(BF, RS_BLOCK);
  UCSA_CLEAR_ERR();
  hipError_t e = hipMemsetAsync(ws + l.cur, 0, l.total - l.cur, s);
  if (e != hipSuccess) return -(int32_t)e;
  if (total_pairs > 0) {
    hipLaunchKernelGGL(k_rs_emit, dim3(ucsa_div_up(total_pairs, 256)), dim3(256), 0, s,
                       (const uint32_t*)(ws + l.rec), (const uint32_t*)(ws + l.foff),
                       (const uint64_t*)(ws + l.boff), nblk, BF, F, k,
                       (const uint32_t*)(ws + l.grid), (const uint32_t*)(ws + l.toff),
                       (uint32_t*)(ws + l.cur), (uint32_t)total_pairs, pairs, max_pairs);
  }
  hipLaunchKernelGGL(k_rs_tile, dim3(k.tX, k.tY, B), dim3(RS_TILE_PIX), 0, s, verts, V, faces,
                     F, BF, poses, vertex_labels, vertex_rgb, k, (const uint32_t*)(ws + l.rec),
                     (const uint32_t*)(ws + l.grid), (const uint32_t*)(ws + l.toff), pairs,
                     total_pairs, tri_id, depth, label, vertex_rgb ? rgb : nullptr);
  return ucsa_launch_status();
}
