// Neighbourhood pooling of fused label tables (not in the reference): the class
// tables of the voxel route (ucsa_voxel_table_smooth) and of the mesh route
// (ucsa_label_table_smooth).  The contracts are stated in include/ucsa_hip.h;
// tests/smooth_numpy.py restates them in numpy and the outputs match it bit for
// bit.
//
// k_voxel_smooth  a gated 27-point (or 7-point) stencil over the C+1 class-major
//                 planes of a lattice table, all planes in one launch.  A
//                 work-group owns a tile of 4 x 4 x 64 voxels, one thread per
//                 voxel, one wave per z-row: a wave's global reads and writes
//                 are contiguous runs along z, and all lanes of an LDS read are
//                 in one row of the halo at consecutive dwords (no bank
//                 conflict whatever the row pitch).  The gate (is the
//                 neighbour inside the lattice and observed?) is the same for
//                 every plane: the tile's 6 x 6 x 66 halo of observed flags
//                 goes through LDS once, each thread folds its 27 flags into a
//                 mask in one register, and the planes then stream through
//                 two LDS buffers (elements widened to 32 bits), one barrier
//                 per plane, the loads of plane p+1 in flight while plane p is
//                 summed.  Halo cells outside the lattice are never loaded
//                 (they are stored as zero).  A tile without an observed voxel
//                 copies its columns and stages nothing.
// k_label_smooth  votes [V][C+1] uint64: a group of G lanes (G a power of two,
//                 G >= min(C+1, 64)) owns a vertex, the columns go across the
//                 lanes, and the group walks the vertex's neighbour list: one
//                 coalesced row read per neighbour, one store per element.
// No atomics anywhere.
#include <cmath>

#include "ucsa_common.h"

namespace {

constexpr uint32_t TS_X = 4, TS_Y = 4, TS_Z = 64;  // the tile; z = one wave
constexpr uint32_t TS_THREADS = TS_X * TS_Y * TS_Z;
constexpr uint32_t TS_HX = TS_X + 2, TS_HY = TS_Y + 2, TS_HZ = TS_Z + 2;
constexpr uint32_t TS_HALO = TS_HX * TS_HY * TS_HZ;  // 2376 cells
constexpr uint32_t TS_PER = (TS_HALO + TS_THREADS - 1) / TS_THREADS;  // 3 cells per thread
constexpr uint32_t TS_NONE = 0xFFFFFFFFu;
// bits (dx*3 + dy)*3 + dz of the six face neighbours, offsets in 0..2, centre 13
constexpr uint32_t TS_FACES = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) |
                              (1u << 22);
constexpr uint32_t TS_CUBE = ((1u << 27) - 1u) & ~(1u << 13);

template <typename T>
struct SmoothArgs {
  const T* in;
  T* out;
  const float* weight;
  uint32_t nx, ny, nz, planes;
  uint32_t centre;
  float min_weight;
};

template <typename T>
struct Acc;
template <>
struct Acc<uint32_t> {
  typedef uint64_t type;  // 281 * (2^32-1) needs 41 bits
  static constexpr uint64_t SAT = 0xFFFFFFFFull;
};
template <>
struct Acc<uint16_t> {
  typedef uint32_t type;  // 281 * 65535 < 2^25: exact in 32 bits
  static constexpr uint32_t SAT = 0xFFFFu;
};

template <typename T, bool FACES_ONLY>
__global__ void __launch_bounds__(TS_THREADS) k_voxel_smooth(SmoothArgs<T> a) {
  typedef typename Acc<T>::type acc_t;
  __shared__ uint32_t s_tile[2][TS_HALO];
  const uint32_t tid = threadIdx.x;
  const uint32_t tz = tid & (TS_Z - 1u), ty = (tid / TS_Z) & (TS_Y - 1u), tx = tid / (TS_Z * TS_Y);
  const uint32_t x0 = blockIdx.z * TS_X, y0 = blockIdx.y * TS_Y, z0 = blockIdx.x * TS_Z;
  const uint32_t x = x0 + tx, y = y0 + ty, z = z0 + tz;
  const bool inside = x < a.nx && y < a.ny && z < a.nz;
  const uint64_t n = (uint64_t)a.nx * a.ny * a.nz;  // <= 2^31-1
  const uint32_t idx = inside ? (x * a.ny + y) * a.nz + z : 0u;
  const bool obs = inside && a.weight[idx] >= a.min_weight;

  if (!__syncthreads_or(obs)) {  // uniform over the work-group
    if (inside)
      for (uint32_t p = 0; p < a.planes; ++p) a.out[(uint64_t)p * n + idx] = a.in[(uint64_t)p * n + idx];
    return;
  }

  // the halo cells this thread stages: in-plane offset, TS_NONE outside the lattice
  uint32_t cell[TS_PER];
#pragma unroll
  for (uint32_t q = 0; q < TS_PER; ++q) {
    const uint32_t c = tid + q * TS_THREADS;
    cell[q] = TS_NONE;
    if (c < TS_HALO) {
      const uint32_t hz = c % TS_HZ, hy = (c / TS_HZ) % TS_HY, hx = c / (TS_HZ * TS_HY);
      // lattice coordinate + 1, so that 0 is the cell before the lattice
      const uint32_t gx = x0 + hx, gy = y0 + hy, gz = z0 + hz;
      if (gx >= 1u && gx <= a.nx && gy >= 1u && gy <= a.ny && gz >= 1u && gz <= a.nz)
        cell[q] = ((gx - 1u) * a.ny + (gy - 1u)) * a.nz + (gz - 1u);
    }
  }

  // the gate: observed flags of the halo through LDS, folded into one register
#pragma unroll
  for (uint32_t q = 0; q < TS_PER; ++q) {
    const uint32_t c = tid + q * TS_THREADS;
    if (c < TS_HALO)
      s_tile[1][c] = cell[q] != TS_NONE && a.weight[cell[q]] >= a.min_weight ? 1u : 0u;
  }
  __syncthreads();
  const uint32_t at = (tx * TS_HY + ty) * TS_HZ + tz;  // halo index of tap (0,0,0)
  uint32_t mask = 0u;
  if (obs) {
#pragma unroll
    for (uint32_t t = 0; t < 27u; ++t) {
      if (!((FACES_ONLY ? TS_FACES : TS_CUBE) >> t & 1u)) continue;
      const uint32_t off = ((t / 9u) * TS_HY + (t / 3u) % 3u) * TS_HZ + t % 3u;
      mask |= s_tile[1][at + off] << t;
    }
  }
  const uint32_t mid = at + (TS_HY + 1u) * TS_HZ + 1u;  // the thread's own cell

  T next[TS_PER];
#pragma unroll
  for (uint32_t q = 0; q < TS_PER; ++q) next[q] = cell[q] != TS_NONE ? a.in[cell[q]] : (T)0;
  // Plane p is staged in s_tile[p & 1].  A thread overwrites a buffer two planes
  // later, after the barrier of the plane in between, which every thread passes
  // only when it has finished reading: one barrier per plane is enough.  The
  // flags in s_tile[1] are overwritten by plane 1, after plane 0's barrier.
  for (uint32_t p = 0; p < a.planes; ++p) {
    uint32_t* __restrict__ s = s_tile[p & 1u];
#pragma unroll
    for (uint32_t q = 0; q < TS_PER; ++q) {
      const uint32_t c = tid + q * TS_THREADS;
      if (c < TS_HALO) s[c] = (uint32_t)next[q];
    }
    if (p + 1u < a.planes) {
      const T* __restrict__ src = a.in + (uint64_t)(p + 1u) * n;
#pragma unroll
      for (uint32_t q = 0; q < TS_PER; ++q) next[q] = cell[q] != TS_NONE ? src[cell[q]] : (T)0;
    }
    __syncthreads();
    if (!inside) continue;
    const uint32_t own = s[mid];
    T res = (T)own;
    if (obs) {
      acc_t sum = (acc_t)own * a.centre;
#pragma unroll
      for (uint32_t t = 0; t < 27u; ++t) {
        if (!((FACES_ONLY ? TS_FACES : TS_CUBE) >> t & 1u)) continue;
        const uint32_t off = ((t / 9u) * TS_HY + (t / 3u) % 3u) * TS_HZ + t % 3u;
        const uint32_t v = s[at + off];
        sum += (mask >> t & 1u) ? v : 0u;
      }
      res = (T)(sum > Acc<T>::SAT ? Acc<T>::SAT : sum);
    }
    a.out[(uint64_t)p * n + idx] = res;
  }
}

// G lanes per vertex, columns across the lanes
__global__ void __launch_bounds__(256) k_label_smooth(const uint64_t* __restrict__ in,
                                                       uint64_t* __restrict__ out, uint32_t V,
                                                       uint32_t W, const int32_t* __restrict__ offsets,
                                                       const int32_t* __restrict__ neighbours,
                                                       uint64_t E, uint32_t centre, uint32_t G) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t v = t / G;
  const uint32_t lane = (uint32_t)(t % G);
  if (v >= V) return;
  // a malformed list reads nothing outside the arrays: the range is clamped to
  // [0, E] and a neighbour outside 0..V-1 is skipped
  int64_t beg = offsets[v], end = offsets[v + 1u];
  beg = beg < 0 ? 0 : beg;
  end = end > (int64_t)E ? (int64_t)E : end;
  for (uint32_t c = lane; c < W; c += G) {
    uint64_t sum = in[v * W + c] * (uint64_t)centre;
#pragma unroll 4
    for (int64_t e = beg; e < end; ++e) {
      const uint32_t nb = (uint32_t)neighbours[e];
      if (nb < V) sum += in[(uint64_t)nb * W + c];
    }
    out[v * W + c] = sum;
  }
}

bool ranges_overlap(const void* p, uint64_t pn, const void* q, uint64_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qn && b < a + pn;
}

template <typename T>
int32_t launch_voxel_smooth(const void* in, void* out, uint32_t C, uint32_t nx, uint32_t ny,
                            uint32_t nz, const float* weight, float min_weight,
                            uint32_t neighbourhood, uint32_t centre, hipStream_t s) {
  SmoothArgs<T> a;
  a.in = (const T*)in;
  a.out = (T*)out;
  a.weight = weight;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.planes = C + 1u;
  a.centre = centre;
  a.min_weight = min_weight;
  const dim3 grid(ucsa_div_up(nz, TS_Z), ucsa_div_up(ny, TS_Y), ucsa_div_up(nx, TS_X));
  UCSA_CLEAR_ERR();
  if (neighbourhood == 6u)
    hipLaunchKernelGGL((k_voxel_smooth<T, true>), grid, dim3(TS_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL((k_voxel_smooth<T, false>), grid, dim3(TS_THREADS), 0, s, a);
  return ucsa_launch_status();
}

}  // namespace

extern "C" int32_t ucsa_voxel_table_smooth(const void* in, void* out, uint32_t elem_bytes,
                                           uint32_t C, uint32_t nx, uint32_t ny, uint32_t nz,
                                           const float* weight, float min_weight,
                                           uint32_t neighbourhood, uint32_t centre,
                                           void* stream) {
  UCSA_CHECK_ARG(in, 0);
  UCSA_CHECK_ARG(out, 1);
  UCSA_CHECK_ARG(elem_bytes == 2u || elem_bytes == 4u, 2);
  UCSA_CHECK_ARG(C >= 1 && C <= 255, 3);
  UCSA_CHECK_ARG(nx >= 2 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 4);
  UCSA_CHECK_ARG(ny >= 2, 5);
  UCSA_CHECK_ARG(nz >= 2, 6);
  UCSA_CHECK_ARG(ucsa_div_up(nx, TS_X) <= 65535u, 4);
  UCSA_CHECK_ARG(ucsa_div_up(ny, TS_Y) <= 65535u, 5);
  const uint64_t n = (uint64_t)nx * ny * nz, elems = (uint64_t)(C + 1u) * n;
  UCSA_CHECK_ARG(elems <= (1ull << 40), 3);
  UCSA_CHECK_ARG(weight, 7);
  UCSA_CHECK_ARG(!std::isnan(min_weight), 8);
  UCSA_CHECK_ARG(neighbourhood == 6u || neighbourhood == 26u, 9);
  UCSA_CHECK_ARG(centre >= 1 && centre <= 255, 10);
  const uint64_t bytes = elems * elem_bytes;
  UCSA_CHECK_ARG(!ranges_overlap(in, bytes, out, bytes), 1);
  UCSA_CHECK_ARG(!ranges_overlap(weight, n * sizeof(float), out, bytes), 1);
  if (elem_bytes == 4u)
    return launch_voxel_smooth<uint32_t>(in, out, C, nx, ny, nz, weight, min_weight,
                                         neighbourhood, centre, (hipStream_t)stream);
  return launch_voxel_smooth<uint16_t>(in, out, C, nx, ny, nz, weight, min_weight, neighbourhood,
                                       centre, (hipStream_t)stream);
}

extern "C" int32_t ucsa_label_table_smooth(const uint64_t* in, uint64_t* out, uint32_t V,
                                           uint32_t C, const int32_t* offsets,
                                           const int32_t* neighbours, uint64_t E,
                                           uint32_t centre, void* stream) {
  UCSA_CHECK_ARG(C >= 1 && C <= 255, 3);
  const uint32_t W = C + 1u;
  UCSA_CHECK_ARG((uint64_t)V * W <= 0x7FFFFFFFull, 2);
  UCSA_CHECK_ARG(E <= 0x7FFFFFFFull, 6);
  UCSA_CHECK_ARG(centre >= 1 && centre <= 255, 7);
  if (V == 0) return 0;
  UCSA_CHECK_ARG(in, 0);
  UCSA_CHECK_ARG(out, 1);
  UCSA_CHECK_ARG(offsets, 4);
  UCSA_CHECK_ARG(neighbours || E == 0, 5);
  const uint64_t bytes = (uint64_t)V * W * sizeof(uint64_t);
  UCSA_CHECK_ARG(!ranges_overlap(in, bytes, out, bytes), 1);
  UCSA_CHECK_ARG(!ranges_overlap(offsets, ((uint64_t)V + 1u) * 4u, out, bytes), 1);
  UCSA_CHECK_ARG(E == 0 || !ranges_overlap(neighbours, E * 4u, out, bytes), 1);
  uint32_t G = 2u;
  while (G < W && G < 64u) G *= 2u;
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_label_smooth, dim3(ucsa_div_up((uint64_t)V * G, 256u)), dim3(256), 0,
                     (hipStream_t)stream, in, out, V, W, offsets, neighbours, E, centre, G);
  return ucsa_launch_status();
}
