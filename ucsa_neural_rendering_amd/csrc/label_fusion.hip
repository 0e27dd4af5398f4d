// Label fusion (ucsa_label_fuse_accumulate / ucsa_label_fuse_resolve): per-frame
// 2D label maps voted onto the vertices of a mesh.  Not in the reference.  The
// contract is stated in include/ucsa_hip.h; tests/fusion_numpy.py restates it in
// numpy and the GPU tables match it bit for bit (integer sums: no order).
//
// k_lf_accumulate  one wave per 16x16 pixel tile, held as four 8x8 patches
//                  (slot j of lane l: pixel (8*(j&1) + l%8, 8*(j/2) + l/8) of the
//                  tile), so that the 256 keys (vertex, class) of a wave repeat.
//                  Leader loop: take the key of the first lane that still has
//                  work, compare it in all four slots (the compare IS the
//                  ballot), count the matches and retire them.  A key held by
//                  one pixel only is marked and left to the end, where all of
//                  them go out as ordinary 64-lane atomic instructions (a fine
//                  mesh with random labels costs what one atomic per pixel
//                  costs, plus the loop's scalar work); a key held by several is
//                  summed (popcount, or a wave sum of the matching weights) and
//                  added once, by its leader.  A wave wholly on one wall of a
//                  coarse mesh issues ONE atomic for 256 pixels.
//                  NAIVE: one atomic per voting pixel, the baseline of
//                  tools/label_fusion_time.py; same table.
// k_lf_resolve     one wave per vertex row, lane c-1 reads class c (coalesced),
//                  wave reduction of (sum, class) and of the total.
// k_lf_evidence    the soft sibling (ucsa_label_fuse_evidence): a pixel adds a
//                  row of C bytes to its vertex's row.  Same tiles and the same
//                  leader loop over the distinct vertices of a wave; the pixels
//                  of one vertex are then walked one by one with the classes
//                  across the lanes (one coalesced read of C bytes each), and
//                  the sums go out as one atomic per class, C lanes to an
//                  instruction: a wave on one wall issues C atomics for 256
//                  pixels, a wave of 256 vertices what one row per pixel costs.
// Only 64-bit integer atomic adds, no float atomics, no LDS.
#include <cmath>

#include "ucsa_common.h"

namespace {

constexpr uint32_t LF_TILE = 16;
constexpr uint32_t LF_SLOTS = 4;
constexpr uint32_t LF_NONE = 0xFFFFFFFFu;  // keys are < 2^31
constexpr uint32_t LF_WAVES = 4;           // per work-group

struct LfArgs {
  const int32_t* vid;
  const uint8_t* pred;
  const int32_t* weight;
  const float* mesh_z;
  const float* sensor_z;
  float tol;
  uint32_t N, W, V, C, tilesX, tiles;
};

// the vote of pixel i: its cell in the table (LF_NONE: none) and what it adds
__device__ __forceinline__ uint32_t lf_key(const LfArgs& a, uint32_t i, uint32_t& w) {
  const int32_t v = a.vid[i];
  const uint32_t c = a.pred[i];
  bool ok = v >= 1 && (uint32_t)v <= a.V && c >= 1 && c <= a.C;
  w = 1u;
  if (a.weight) {
    const int32_t x = a.weight[i];
    ok = ok && x >= 1 && x <= 65535;  // adding 0 changes nothing: no work
    w = (uint32_t)x;
  }
  if (a.mesh_z) {
    const float s = a.sensor_z[i];
    ok = ok && s > 0.0f && fabsf(a.mesh_z[i] - s) <= a.tol;
  }
  return ok ? (uint32_t)(v - 1) * (a.C + 1u) + c : LF_NONE;
}

__device__ __forceinline__ uint32_t lf_wave_sum(uint32_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, UCSA_WAVE);
  return x;
}

template <bool NAIVE>
__global__ void __launch_bounds__(LF_WAVES * UCSA_WAVE)
k_lf_accumulate(LfArgs a, unsigned long long* __restrict__ votes) {
  const uint32_t lane = threadIdx.x & (UCSA_WAVE - 1);
  const uint32_t tile = blockIdx.x * LF_WAVES + threadIdx.x / UCSA_WAVE;
  if (tile >= a.tiles) return;  // whole waves leave: every ballot below sees 64 lanes
  const uint32_t ty = tile / a.tilesX, tx = tile - ty * a.tilesX;
  uint32_t key[LF_SLOTS], w[LF_SLOTS];
#pragma unroll
  for (uint32_t j = 0; j < LF_SLOTS; ++j) {
    const uint32_t px = tx * LF_TILE + (j & 1u) * 8u + (lane & 7u);
    const uint64_t row = (uint64_t)ty * LF_TILE + (j >> 1) * 8u + (lane >> 3);
    const uint64_t i = row * a.W + px;
    key[j] = LF_NONE;
    w[j] = 0u;
    if (px < a.W && i < a.N) key[j] = lf_key(a, (uint32_t)i, w[j]);
  }
  if (NAIVE) {
#pragma unroll
    for (uint32_t j = 0; j < LF_SLOTS; ++j)
      if (key[j] != LF_NONE) atomicAdd(votes + key[j], (unsigned long long)w[j]);
    return;
  }
  unsigned long long todo[LF_SLOTS];
#pragma unroll
  for (uint32_t j = 0; j < LF_SLOTS; ++j) todo[j] = __ballot(key[j] != LF_NONE);
  uint32_t alone = 0;  // bit j: slot j's key occurs once in the wave
#pragma unroll
  for (uint32_t s = 0; s < LF_SLOTS; ++s) {
    // slots below s are drained, and with them every key they held
    while (todo[s]) {
      const uint32_t lead = (uint32_t)__ffsll((long long)todo[s]) - 1u;
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key[s], (int)lead);
      uint32_t n = 0, mine = 0;
#pragma unroll
      for (uint32_t j = s; j < LF_SLOTS; ++j) {
        const bool eq = key[j] == k;
        const unsigned long long m = __ballot(eq);
        n += (uint32_t)__popcll(m);
        todo[j] &= ~m;
        mine += eq ? w[j] : 0u;
      }
      if (n == 1u) {
        alone |= (lane == lead ? 1u : 0u) << s;
      } else {
        // at most 256 * 65535 < 2^32
        const uint32_t sum = a.weight ? lf_wave_sum(mine) : n;
        if (lane == lead) atomicAdd(votes + k, (unsigned long long)sum);
      }
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < LF_SLOTS; ++j)
    if ((alone >> j) & 1u) atomicAdd(votes + key[j], (unsigned long long)w[j]);
}

// ---- evidence (soft votes): a row of C codes per pixel -----------------------
struct LeArgs {
  const int32_t* vid;
  const uint8_t* scores;
  const float* mesh_z;
  const float* sensor_z;
  float tol;
  uint32_t N, W, V, C, tilesX, tiles;
};

constexpr uint32_t LE_STRIDES = 4;  // lane l sums classes l + 64 q: C <= 255

// index of the pixel that slot j of lane l holds; a.N and beyond: none
__device__ __forceinline__ uint64_t le_pixel(const LeArgs& a, uint32_t tx, uint32_t ty,
                                             uint32_t j, uint32_t l) {
  const uint32_t px = tx * LF_TILE + (j & 1u) * 8u + (l & 7u);
  const uint64_t row = (uint64_t)ty * LF_TILE + (j >> 1) * 8u + (l >> 3);
  const uint64_t i = row * a.W + px;
  return px < a.W && i < a.N ? i : (uint64_t)a.N;
}

__global__ void __launch_bounds__(LF_WAVES * UCSA_WAVE)
k_lf_evidence(LeArgs a, unsigned long long* __restrict__ votes) {
  const uint32_t lane = threadIdx.x & (UCSA_WAVE - 1);
  const uint32_t tile = blockIdx.x * LF_WAVES + threadIdx.x / UCSA_WAVE;
  if (tile >= a.tiles) return;  // whole waves leave: every ballot below sees 64 lanes
  const uint32_t ty = tile / a.tilesX, tx = tile - ty * a.tilesX;
  uint32_t key[LF_SLOTS];  // the pixel's vertex, 0-based
  unsigned long long todo[LF_SLOTS];
#pragma unroll
  for (uint32_t j = 0; j < LF_SLOTS; ++j) {
    const uint64_t i = le_pixel(a, tx, ty, j, lane);
    key[j] = LF_NONE;
    if (i < a.N) {
      const int32_t v = a.vid[i];
      bool ok = v >= 1 && (uint32_t)v <= a.V;
      if (a.mesh_z) {
        const float s = a.sensor_z[i];
        ok = ok && s > 0.0f && fabsf(a.mesh_z[i] - s) <= a.tol;
      }
      if (ok) key[j] = (uint32_t)(v - 1);
    }
    todo[j] = __ballot(key[j] != LF_NONE);
  }
#pragma unroll
  for (uint32_t s = 0; s < LF_SLOTS; ++s) {
    // slots below s are drained, and with them every vertex they held
    while (todo[s]) {
      const uint32_t lead = (uint32_t)__ffsll((long long)todo[s]) - 1u;
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key[s], (int)lead);
      uint32_t sum[LE_STRIDES] = {0u, 0u, 0u, 0u};  // at most 256 * 255 each
#pragma unroll
      for (uint32_t j = s; j < LF_SLOTS; ++j) {
        unsigned long long m = __ballot(key[j] == k);
        todo[j] &= ~m;
        while (m) {  // the pixels of vertex k, one after the other: uniform
          const uint32_t l = (uint32_t)__ffsll((long long)m) - 1u;
          m &= m - 1ull;
          const uint8_t* __restrict__ row = a.scores + le_pixel(a, tx, ty, j, l) * a.C;
#pragma unroll
          for (uint32_t q = 0; q < LE_STRIDES; ++q) {
            const uint32_t c = lane + q * UCSA_WAVE;
            if (c < a.C) sum[q] += row[c];
          }
        }
      }
      unsigned long long* __restrict__ out = votes + (size_t)k * (a.C + 1u) + 1u;
#pragma unroll
      for (uint32_t q = 0; q < LE_STRIDES; ++q) {
        const uint32_t c = lane + q * UCSA_WAVE;
        if (c < a.C && sum[q] != 0u) atomicAdd(out + c, (unsigned long long)sum[q]);
      }
    }
  }
}

struct LfBest {
  unsigned long long sum;
  uint32_t cls;
};

__device__ __forceinline__ bool lf_better(const LfBest& x, const LfBest& y) {
  return x.sum > y.sum || (x.sum == y.sum && x.cls < y.cls);
}

__global__ void __launch_bounds__(LF_WAVES * UCSA_WAVE)
k_lf_resolve(const unsigned long long* __restrict__ votes, uint32_t V, uint32_t C,
             unsigned long long min_votes, int32_t* __restrict__ label,
             unsigned long long* __restrict__ total,
             unsigned long long* __restrict__ winner) {
  const uint32_t lane = threadIdx.x & (UCSA_WAVE - 1);
  const uint32_t v = blockIdx.x * LF_WAVES + threadIdx.x / UCSA_WAVE;
  if (v >= V) return;
  const unsigned long long* row = votes + (size_t)v * (C + 1u);
  LfBest b = {0ull, LF_NONE};
  unsigned long long tot = 0ull;
  for (uint32_t c = 1u + lane; c <= C; c += UCSA_WAVE) {
    const LfBest x = {row[c], c};
    tot += x.sum;
    if (lf_better(x, b)) b = x;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    LfBest o;
    o.sum = __shfl_xor(b.sum, d, UCSA_WAVE);
    o.cls = __shfl_xor(b.cls, d, UCSA_WAVE);
    tot += __shfl_xor(tot, d, UCSA_WAVE);
    if (lf_better(o, b)) b = o;
  }
  if (lane == 0) {
    label[v] = tot >= min_votes ? (int32_t)b.cls : 0;
    total[v] = tot;
    winner[v] = b.sum;
  }
}

}  // namespace

extern "C" int32_t ucsa_label_fuse_accumulate(const int32_t* vertex_id, const uint8_t* pred,
                                              const int32_t* weight, const float* mesh_depth,
                                              const float* sensor_depth, float depth_tol,
                                              uint64_t N, uint32_t row_width, uint32_t V,
                                              uint32_t C, uint64_t* votes,
                                              uint64_t votes_capacity, uint32_t flags,
                                              void* stream) {
  UCSA_CHECK_ARG(C >= 1 && C <= 255, 9);
  UCSA_CHECK_ARG((uint64_t)V * (C + 1u) <= 0x7FFFFFFFull, 8);
  UCSA_CHECK_ARG(N <= 0x7FFFFFFFull, 6);
  UCSA_CHECK_ARG(flags <= UCSA_FUSE_ONE_ATOMIC_PER_PIXEL, 12);
  UCSA_CHECK_ARG((mesh_depth == nullptr) == (sensor_depth == nullptr), mesh_depth ? 4 : 3);
  UCSA_CHECK_ARG(!mesh_depth || depth_tol >= 0.0f, 5);
  if (V == 0 || N == 0) return 0;
  UCSA_CHECK_ARG(vertex_id, 0);
  UCSA_CHECK_ARG(pred, 1);
  UCSA_CHECK_ARG(votes, 10);
  UCSA_CHECK_ARG(votes_capacity >= (uint64_t)V * (C + 1u), 11);
  LfArgs a;
  a.vid = vertex_id;
  a.pred = pred;
  a.weight = weight;
  a.mesh_z = mesh_depth;
  a.sensor_z = sensor_depth;
  a.tol = depth_tol;
  a.N = (uint32_t)N;
  a.W = row_width == 0 ? LF_TILE : row_width;
  if (a.W > a.N) a.W = a.N;
  a.V = V;
  a.C = C;
  const uint32_t rows = ucsa_div_up(N, a.W);
  a.tilesX = ucsa_div_up(a.W, LF_TILE);
  // N <= 2^31-1: fewer than 2^27 + 2^27 tiles for every W
  a.tiles = a.tilesX * ucsa_div_up(rows, LF_TILE);
  const dim3 grid(ucsa_div_up(a.tiles, LF_WAVES)), block(LF_WAVES * UCSA_WAVE);
  hipStream_t s = (hipStream_t)stream;
  UCSA_CLEAR_ERR();
  if (flags & UCSA_FUSE_ONE_ATOMIC_PER_PIXEL)
    hipLaunchKernelGGL(k_lf_accumulate<true>, grid, block, 0, s, a, (unsigned long long*)votes);
  else
    hipLaunchKernelGGL(k_lf_accumulate<false>, grid, block, 0, s, a, (unsigned long long*)votes);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_label_fuse_evidence(const int32_t* vertex_id, const uint8_t* scores,
                                            const float* mesh_depth, const float* sensor_depth,
                                            float depth_tol, uint64_t N, uint32_t row_width,
                                            uint32_t V, uint32_t C, uint64_t* votes,
                                            uint64_t votes_capacity, void* stream) {
  UCSA_CHECK_ARG(C >= 1 && C <= 255, 8);
  UCSA_CHECK_ARG((uint64_t)V * (C + 1u) <= 0x7FFFFFFFull, 7);
  UCSA_CHECK_ARG(N <= 0x7FFFFFFFull, 5);
  UCSA_CHECK_ARG((mesh_depth == nullptr) == (sensor_depth == nullptr), mesh_depth ? 3 : 2);
  UCSA_CHECK_ARG(!mesh_depth || depth_tol >= 0.0f, 4);
  if (V == 0 || N == 0) return 0;
  UCSA_CHECK_ARG(vertex_id, 0);
  UCSA_CHECK_ARG(scores, 1);
  UCSA_CHECK_ARG(votes, 9);
  UCSA_CHECK_ARG(votes_capacity >= (uint64_t)V * (C + 1u), 10);
  LeArgs a;
  a.vid = vertex_id;
  a.scores = scores;
  a.mesh_z = mesh_depth;
  a.sensor_z = sensor_depth;
  a.tol = depth_tol;
  a.N = (uint32_t)N;
  a.W = row_width == 0 ? LF_TILE : row_width;
  if (a.W > a.N) a.W = a.N;
  a.V = V;
  a.C = C;
  const uint32_t rows = ucsa_div_up(N, a.W);
  a.tilesX = ucsa_div_up(a.W, LF_TILE);
  a.tiles = a.tilesX * ucsa_div_up(rows, LF_TILE);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_lf_evidence, dim3(ucsa_div_up(a.tiles, LF_WAVES)),
                     dim3(LF_WAVES * UCSA_WAVE), 0, (hipStream_t)stream, a,
                     (unsigned long long*)votes);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_label_fuse_resolve(const uint64_t* votes, uint32_t V, uint32_t C,
                                           uint64_t min_votes, int32_t* label, uint64_t* total,
                                           uint64_t* winner, uint64_t max_vertices,
                                           void* stream) {
  UCSA_CHECK_ARG(C >= 1 && C <= 255, 2);
  UCSA_CHECK_ARG((uint64_t)V * (C + 1u) <= 0x7FFFFFFFull, 1);
  UCSA_CHECK_ARG(min_votes >= 1, 3);
  UCSA_CHECK_ARG(max_vertices >= V, 7);
  if (V == 0) return 0;
  UCSA_CHECK_ARG(votes, 0);
  UCSA_CHECK_ARG(label, 4);
  UCSA_CHECK_ARG(total, 5);
  UCSA_CHECK_ARG(winner, 6);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_lf_resolve, dim3(ucsa_div_up(V, LF_WAVES)), dim3(LF_WAVES * UCSA_WAVE), 0,
                     (hipStream_t)stream, (const unsigned long long*)votes, V, C,
                     (unsigned long long)min_votes, label, (unsigned long long*)total,
                     (unsigned long long*)winner);
  return ucsa_launch_status();
}
