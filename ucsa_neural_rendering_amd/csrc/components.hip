// Connected components (not in the reference): of a voxel mask
// (ucsa_voxel_components), of a graph in compressed rows (ucsa_graph_components),
// and the size of each element's component (ucsa_component_sizes).  The
// contracts are stated in include/ucsa_hip.h; tests/components_numpy.py restates
// them in numpy and the outputs match it byte for byte: a label is the smallest
// index of its component, which no schedule can change.
//
// Union-find in the output array itself, a fixed number of launches per call, no
// host read-back and no "changed" flag.  The rules every kernel here keeps:
//   * parent[x] <= x at every instant, for every value a load can return (the
//     initial x, or what an atomic min put there later: smaller).  A find walk
//     therefore strictly descends and ends after at most x steps, whatever other
//     waves do meanwhile and however stale a cached line is.
//   * every value ever stored in parent[x] is an element of x's component, so a
//     stale load only makes a walk start higher up, never in another tree.
//   * a union hooks the larger root under the smaller with one integer atomic
//     min (executed at the memory side: coherent over the whole chip) and learns
//     from the returned value whether it met a root; if not, it goes on with the
//     pair (returned parent, other root), whose sum is smaller.
//   * no loop's exit waits for another wave: there are no spins, flags or locks.
// The forest is final when the hooking launch has ended; the flatten launch makes
// every element point at its root, which is the minimum of its tree because only
// larger roots are ever hooked under smaller ones.
//
// k_tile_components    a work-group labels its 4 x 4 x 64 tile (z = one wave, the
//                      tile of table_smooth.hip) in LDS: 1024 parents as tile-local
//                      indices, each voxel hooks to the earlier half of its
//                      neighbourhood (3 of 6, 13 of 26) inside the tile with LDS
//                      atomics, and the tile's local roots go out as global
//                      indices.  Local and global order agree inside a tile, so
//                      parent[x] <= x holds globally.
// k_lattice_hook       unions across tile faces, edges and corners with global
//                      atomics (BORDER_ONLY), or over every earlier neighbour (the
//                      variant without the LDS stage, UCSA_COMPONENTS_NO_LDS=1:
//                      tools/components_time.py measures one against the other).
// k_flatten            labels[x] = find(x); -1 stays -1.
// k_graph_hook         a lane per vertex hooks over its neighbours n < v; rows
//                      longer than 64 entries are left to the whole wave, which
//                      walks them 64 entries at a time (a star's centre does not
//                      hold 63 idle lanes behind one lane's row).
// k_size_count/gather  counts by root with 32-bit integer atomics, the lanes of a
//                      wave that share a root summed first (ballot + popcount, as
//                      label_fusion.hip does for vertices): a wall that is one
//                      root for millions of voxels costs one atomic per wave.
#include "ucsa_common.h"

namespace {

constexpr uint32_t CC_X = 4, CC_Y = 4, CC_Z = 64;  // the tile; z = one wave
constexpr uint32_t CC_THREADS = CC_X * CC_Y * CC_Z;
constexpr uint32_t CC_LONG_ROW = 64;  // graph rows above this are walked by the wave

#define CC_AGENT __HIP_MEMORY_SCOPE_AGENT
#define CC_GROUP __HIP_MEMORY_SCOPE_WORKGROUP

// The walk moves only to a smaller, non-negative index: it ends after at most x
// steps and never leaves [0, x], whatever the array holds.
template <int SCOPE>
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x) {
  int32_t p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE);
  while (p < x && p >= 0) {
    x = p;
    p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE);
  }
  return x;
}

// Each pass either returns or replaces (a, b) by a pair with a smaller sum (the
// finds only descend, and `old` < a): at most a + b passes, no waiting on anyone.
template <int SCOPE>
__device__ __forceinline__ void uf_union(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find<SCOPE>(parent, a);
    b = uf_find<SCOPE>(parent, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old >= a || old < 0) return;  // a was a root: hooked
    a = old;  // a had a parent already; its tree still has to meet b's
  }
}

// offsets of the "earlier" half of the neighbourhood, in the order of the linear
// index: 13 of the 26, of which the 3 face neighbours come at t = 4, 10, 12
__device__ __forceinline__ void cc_offset(uint32_t t, int32_t& dx, int32_t& dy, int32_t& dz) {
  dx = (int32_t)(t / 9u) - 1;
  dy = (int32_t)((t / 3u) % 3u) - 1;
  dz = (int32_t)(t % 3u) - 1;
}
constexpr uint32_t CC_FACES = (1u << 4) | (1u << 10) | (1u << 12);
constexpr uint32_t CC_EARLIER = (1u << 13) - 1u;

struct LatticeArgs {
  const uint8_t* mask;
  int32_t* parent;
  uint32_t nx, ny, nz;
};

template <bool FACES_ONLY>
__global__ void __launch_bounds__(CC_THREADS) k_tile_components(LatticeArgs a) {
  __shared__ int32_t s_par[CC_THREADS];
  const uint32_t tid = threadIdx.x;
  const uint32_t tz = tid & (CC_Z - 1u), ty = (tid / CC_Z) & (CC_Y - 1u), tx = tid / (CC_Z * CC_Y);
  const uint32_t x0 = blockIdx.z * CC_X, y0 = blockIdx.y * CC_Y, z0 = blockIdx.x * CC_Z;
  const uint32_t x = x0 + tx, y = y0 + ty, z = z0 + tz;
  const bool inside = x < a.nx && y < a.ny && z < a.nz;
  const uint32_t idx = inside ? (x * a.ny + y) * a.nz + z : 0u;
  const bool set = inside && a.mask[idx] != 0;

  if (!__syncthreads_or(set)) {  // uniform over the work-group
    if (inside) a.parent[idx] = -1;
    return;
  }
  s_par[tid] = set ? (int32_t)tid : -1;
  __syncthreads();
  if (set) {
#pragma unroll
    for (uint32_t t = 0; t < 13u; ++t) {
      if (!((FACES_ONLY ? CC_FACES : CC_EARLIER) >> t & 1u)) continue;
      int32_t dx, dy, dz;
      cc_offset(t, dx, dy, dz);
      const uint32_t ux = tx + (uint32_t)dx, uy = ty + (uint32_t)dy, uz = tz + (uint32_t)dz;
      if (ux >= CC_X || uy >= CC_Y || uz >= CC_Z) continue;  // another tile's (wraps when < 0)
      const uint32_t nb = (ux * CC_Y + uy) * CC_Z + uz;
      // a cell that is not set holds -1 for the whole launch
      if (__hip_atomic_load(s_par + nb, __ATOMIC_RELAXED, CC_GROUP) >= 0)
        uf_union<CC_GROUP>(s_par, (int32_t)tid, (int32_t)nb);
    }
  }
  __syncthreads();
  if (!inside) return;
  int32_t out = -1;
  if (set) {
    const uint32_t r = (uint32_t)uf_find<CC_GROUP>(s_par, (int32_t)tid);  // a set cell of this tile
    const uint32_t rz = r & (CC_Z - 1u), ry = (r / CC_Z) & (CC_Y - 1u), rx = r / (CC_Z * CC_Y);
    out = (int32_t)(((x0 + rx) * a.ny + (y0 + ry)) * a.nz + (z0 + rz));
  }
  a.parent[idx] = out;
}

// the variant without the LDS stage starts from parent[x] = x
__global__ void __launch_bounds__(256) k_lattice_init(const uint8_t* __restrict__ mask,
                                                      int32_t* __restrict__ parent, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) parent[i] = mask[i] != 0 ? (int32_t)i : -1;
}

template <bool FACES_ONLY, bool BORDER_ONLY>
__global__ void __launch_bounds__(CC_THREADS) k_lattice_hook(LatticeArgs a) {
  const uint32_t tid = threadIdx.x;
  const uint32_t tz = tid & (CC_Z - 1u), ty = (tid / CC_Z) & (CC_Y - 1u), tx = tid / (CC_Z * CC_Y);
  const uint32_t x = blockIdx.z * CC_X + tx, y = blockIdx.y * CC_Y + ty, z = blockIdx.x * CC_Z + tz;
  if (!(x < a.nx && y < a.ny && z < a.nz)) return;
  const uint32_t idx = (x * a.ny + y) * a.nz + z;
  if (a.mask[idx] == 0) return;
#pragma unroll
  for (uint32_t t = 0; t < 13u; ++t) {
    if (!((FACES_ONLY ? CC_FACES : CC_EARLIER) >> t & 1u)) continue;
    int32_t dx, dy, dz;
    cc_offset(t, dx, dy, dz);
    if (BORDER_ONLY) {
      const uint32_t ux = tx + (uint32_t)dx, uy = ty + (uint32_t)dy, uz = tz + (uint32_t)dz;
      if (ux < CC_X && uy < CC_Y && uz < CC_Z) continue;  // the tile's own: done in LDS
    }
    const uint32_t gx = x + (uint32_t)dx, gy = y + (uint32_t)dy, gz = z + (uint32_t)dz;
    if (gx >= a.nx || gy >= a.ny || gz >= a.nz) continue;  // outside the lattice (wraps when < 0)
    const uint32_t nb = (gx * a.ny + gy) * a.nz + gz;
    if (a.mask[nb] != 0) uf_union<CC_AGENT>(a.parent, (int32_t)idx, (int32_t)nb);
  }
}

__global__ void __launch_bounds__(256) k_flatten(int32_t* parent, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  // other threads store roots over parents meanwhile: both lead to the same root
  if (__hip_atomic_load(parent + i, __ATOMIC_RELAXED, CC_AGENT) < 0) return;
  const int32_t r = uf_find<CC_AGENT>(parent, (int32_t)i);
  __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, CC_AGENT);
}

__global__ void __launch_bounds__(256) k_graph_init(int32_t* __restrict__ parent, uint32_t V) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v < V) parent[v] = (int32_t)v;
}

__global__ void __launch_bounds__(256) k_graph_hook(const int32_t* __restrict__ offsets,
                                                    const int32_t* __restrict__ neighbours,
                                                    uint32_t V, uint64_t E, int32_t* parent) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & (UCSA_WAVE - 1u);
  // no lane leaves early: the wave walks long rows together below.  A malformed
  // list reads nothing outside the arrays: the range is clamped to [0, E] and a
  // neighbour outside 0..V-1 is skipped.
  int64_t beg = 0, end = 0;
  if (v < V) {
    beg = offsets[v];
    end = offsets[v + 1u];
    beg = beg < 0 ? 0 : beg;
    end = end > (int64_t)E ? (int64_t)E : end;
    if (end < beg) end = beg;
  }
  const bool is_long = end - beg > (int64_t)CC_LONG_ROW;
  if (!is_long)
    for (int64_t e = beg; e < end; ++e) {  // at most CC_LONG_ROW entries
      const uint32_t nb = (uint32_t)neighbours[e];
      if (nb < v) uf_union<CC_AGENT>(parent, (int32_t)v, (int32_t)nb);
    }
  // One long row per pass, its owner the lowest lane still on the list; the pass
  // clears that lane's bit, so the list (the same in all lanes) empties after at
  // most 64 passes.
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int lead = __ffsll(todo) - 1;
    todo &= todo - 1ull;
    const uint32_t lv = (uint32_t)__shfl((int)v, lead, UCSA_WAVE);
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)beg, lead, UCSA_WAVE);  // <= E <= 2^31-1
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)end, lead, UCSA_WAVE);
    for (uint32_t e = lo + lane; e < hi; e += UCSA_WAVE) {  // e < hi <= E
      const uint32_t nb = (uint32_t)neighbours[e];
      if (nb < lv) uf_union<CC_AGENT>(parent, (int32_t)lv, (int32_t)nb);
    }
  }
}

__global__ void __launch_bounds__(256) k_size_count(const int32_t* __restrict__ labels,
                                                    uint32_t* scratch, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & (UCSA_WAVE - 1u);
  // no lane leaves early: every ballot below sees the whole wave
  const int32_t r = i < n ? labels[i] : -1;
  const bool counts = r >= 0 && (uint32_t)r < n;
  // Each pass retires every lane that holds the leader's root, the leader
  // included: the list (the same in all lanes) empties after at most 64 passes.
  unsigned long long todo = __ballot(counts);
  while (todo) {
    const int lead = __ffsll(todo) - 1;
    const int32_t k = __shfl(r, lead, UCSA_WAVE);
    const unsigned long long m = __ballot(counts && r == k);
    if ((int)lane == lead) atomicAdd(scratch + k, (uint32_t)__popcll(m));
    todo &= ~(m | (1ull << lead));
  }
}

__global__ void __launch_bounds__(256) k_size_gather(const int32_t* __restrict__ labels,
                                                     const uint32_t* __restrict__ scratch,
                                                     int32_t* __restrict__ sizes, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int32_t r = labels[i];
  sizes[i] = r >= 0 && (uint32_t)r < n ? (int32_t)scratch[r] : 0;
}

bool cc_overlap(const void* p, uint64_t pn, const void* q, uint64_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qn && b < a + pn;
}

bool cc_no_lds() { return ucsa_env().components_no_lds; }

}  // namespace

extern "C" int32_t ucsa_voxel_components(const uint8_t* mask, int32_t* labels, uint32_t nx,
                                         uint32_t ny, uint32_t nz, uint32_t connectivity,
                                         void* stream) {
  UCSA_CHECK_ARG(mask, 0);
  UCSA_CHECK_ARG(labels, 1);
  UCSA_CHECK_ARG(nx >= 1 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 2);
  UCSA_CHECK_ARG(ny >= 1, 3);
  UCSA_CHECK_ARG(nz >= 1, 4);
  UCSA_CHECK_ARG(ucsa_div_up(nx, CC_X) <= 65535u, 2);
  UCSA_CHECK_ARG(ucsa_div_up(ny, CC_Y) <= 65535u, 3);
  UCSA_CHECK_ARG(connectivity == 6u || connectivity == 26u, 5);
  const uint32_t n = nx * ny * nz;
  UCSA_CHECK_ARG(!cc_overlap(mask, n, labels, (uint64_t)n * 4u), 1);
  LatticeArgs a;
  a.mask = mask;
  a.parent = labels;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ucsa_div_up(nz, CC_Z), ucsa_div_up(ny, CC_Y), ucsa_div_up(nx, CC_X));
  const bool faces = connectivity == 6u;
  UCSA_CLEAR_ERR();
  if (cc_no_lds()) {
    hipLaunchKernelGGL(k_lattice_init, dim3(ucsa_div_up(n, 256u)), dim3(256), 0, s, mask, labels, n);
    if (faces)
      hipLaunchKernelGGL((k_lattice_hook<true, false>), grid, dim3(CC_THREADS), 0, s, a);
    else
      hipLaunchKernelGGL((k_lattice_hook<false, false>), grid, dim3(CC_THREADS), 0, s, a);
  } else if (faces) {
    hipLaunchKernelGGL((k_tile_components<true>), grid, dim3(CC_THREADS), 0, s, a);
    hipLaunchKernelGGL((k_lattice_hook<true, true>), grid, dim3(CC_THREADS), 0, s, a);
  } else {
    hipLaunchKernelGGL((k_tile_components<false>), grid, dim3(CC_THREADS), 0, s, a);
    hipLaunchKernelGGL((k_lattice_hook<false, true>), grid, dim3(CC_THREADS), 0, s, a);
  }
  hipLaunchKernelGGL(k_flatten, dim3(ucsa_div_up(n, 256u)), dim3(256), 0, s, labels, n);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_graph_components(const int32_t* offsets, const int32_t* neighbours,
                                         uint32_t V, uint64_t E, int32_t* labels, void* stream) {
  UCSA_CHECK_ARG(V <= 0x7FFFFFFFu, 2);
  UCSA_CHECK_ARG(E <= 0x7FFFFFFFull, 3);
  if (V == 0) return 0;
  UCSA_CHECK_ARG(offsets, 0);
  UCSA_CHECK_ARG(neighbours || E == 0, 1);
  UCSA_CHECK_ARG(labels, 4);
  const uint64_t bytes = (uint64_t)V * 4u;
  UCSA_CHECK_ARG(!cc_overlap(offsets, bytes + 4u, labels, bytes), 4);
  UCSA_CHECK_ARG(E == 0 || !cc_overlap(neighbours, E * 4u, labels, bytes), 4);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ucsa_div_up(V, 256u));
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_graph_init, grid, dim3(256), 0, s, labels, V);
  if (E != 0)
    hipLaunchKernelGGL(k_graph_hook, grid, dim3(256), 0, s, offsets, neighbours, V, E, labels);
  hipLaunchKernelGGL(k_flatten, grid, dim3(256), 0, s, labels, V);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_component_sizes(const int32_t* labels, int32_t* sizes, int32_t* scratch,
                                        uint64_t n, void* stream) {
  UCSA_CHECK_ARG(n <= 0x7FFFFFFFull, 3);
  if (n == 0) return 0;
  UCSA_CHECK_ARG(labels, 0);
  UCSA_CHECK_ARG(sizes, 1);
  UCSA_CHECK_ARG(scratch, 2);
  const uint64_t bytes = n * 4u;
  UCSA_CHECK_ARG(!cc_overlap(labels, bytes, sizes, bytes), 1);
  UCSA_CHECK_ARG(!cc_overlap(labels, bytes, scratch, bytes), 2);
  UCSA_CHECK_ARG(!cc_overlap(sizes, bytes, scratch, bytes), 2);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ucsa_div_up(n, 256u));
  UCSA_CLEAR_ERR();
  const hipError_t e = hipMemsetAsync(scratch, 0, bytes, s);
  if (e != hipSuccess) return -(int32_t)e;
  hipLaunchKernelGGL(k_size_count, grid, dim3(256), 0, s, labels, (uint32_t*)scratch, (uint32_t)n);
  hipLaunchKernelGGL(k_size_gather, grid, dim3(256), 0, s, labels, (const uint32_t*)scratch, sizes,
                     (uint32_t)n);
  return ucsa_launch_status();
}
