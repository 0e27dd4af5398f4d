// Occupancy prior from a TSDF volume (ucsa_tsdf_occupancy): which cells of the
// marcher's cascade grid may hold matter, given the space the depth sensor saw
// to be empty.  Not in the reference (its parent code base had
// mark_untrained_grid).  The contract is stated in include/ucsa_hip.h;
// tests/occupancy_numpy.py restates it in numpy and the masks match it byte for
// byte.  A cell's value is a pure OR over the box of voxels that its dilated
// box meets: no atomics, no order, two runs give the same bytes.
//
// k_occ_pack   the blocking predicate ("not free") is one bit per voxel.  One
//              wave takes 64 consecutive z of one (x, y) row: coalesced loads of
//              tsdf and weight, one ballot, lane 0 stores the 64-bit word.
//              bits [nx][ny][ceil(nz/64)]; bits past nz are 0.  A 512^3 volume
//              packs to 16 MB, which stays in L2 / MALL for the second kernel.
// k_occ_cells  one lane per cell of [cascade,H,H,H]; z, the contiguous index,
//              runs across the lanes, so the byte stores coalesce and the lanes
//              of a wave share their (x, y) rows of words.  Per axis the lane
//              finds the index interval of overlapping voxels by two binary
//              searches over the contract's own predicate (monotone in the
//              voxel index because p(i) is non-decreasing): no floor of its own,
//              no estimate to repair.  It then walks the (x, y) box and tests
//              each z-run with masked words, leaving at the first blocked bit.
// Work per lane: 6 * ceil(log2(n + 1)) <= 186 predicate evaluations for the
// searches, then at most rx * ry * ceil((rz + 63) / 64) word loads, where r_a is
// the number of voxels the dilated cell meets on axis a: r_a <=
// (cell + 2 * dilate) / spacing_a + 2.  The worst case is a cell that covers the
// whole volume with nothing blocked, nx * ny * ceil(nz / 64) loads; the room at
// 512^3 under cascade 2 of 128^3 cells is 8 * 8 * 2.  No LDS.
#include <cmath>

#include "ucsa_common.h"

namespace {

constexpr uint32_t OC_BLOCK = 256;

struct OcArgs {
  const float* tsdf;
  const float* weight;
  uint64_t* bits;
  uint8_t* mask;
  uint32_t n[3], nwz;
  float o[3], h[3], half[3];
  float min_weight, free_tsdf, bound, dilate;
  uint32_t unknown_keeps, cascade, H;
};

__global__ void __launch_bounds__(OC_BLOCK) k_occ_pack(OcArgs a, uint64_t words) {
  const uint64_t w = ((uint64_t)blockIdx.x * OC_BLOCK + threadIdx.x) >> 6;
  if (w >= words) return;  // uniform over the wave
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t row = w / a.nwz;
  const uint32_t k = (uint32_t)(w - row * a.nwz) * 64u + lane;
  bool blocked = false;
  if (k < a.n[2]) {
    const uint64_t idx = row * a.n[2] + k;
    const float t = a.tsdf[idx], wt = a.weight[idx];
    const bool seen = wt >= a.min_weight;  // NaN: not seen
    // free iff seen && t >= free_tsdf; an unseen voxel is free as well when
    // unknown space counts as empty
    blocked = a.unknown_keeps ? !(seen && t >= a.free_tsdf) : (seen && !(t >= a.free_tsdf));
  }
  const uint64_t word = __ballot(blocked);
  if (lane == 0) a.bits[w] = word;
}

__device__ __forceinline__ float oc_centre(const OcArgs& a, int ax, uint32_t i) {
  return a.o[ax] + (float)i * a.h[ax];
}

// One axis of one cell: the closed index interval [i0, i1] of the voxels whose
// boxes meet [lo, hi] (empty when i0 > i1), and whether the cell reaches outside
// the volume.  Both predicates are monotone in i; each search keeps the
// invariant "every index below x is on the left side, every index from y on is
// on the right side" and ends with x == y, the first index of the right side.
__device__ __forceinline__ void oc_axis(const OcArgs& a, int ax, uint32_t j, float b, int32_t& i0,
                                        int32_t& i1, bool& outside) {
  const float Hf = (float)a.H;
  const float lo = b * ((float)(2u * j) / Hf - 1.0f) - a.dilate;
  const float hi = b * ((float)(2u * j + 2u) / Hf - 1.0f) + a.dilate;
  const float hv = a.half[ax];
  const uint32_t n = a.n[ax];
  uint32_t x = 0, y = n;  // first i with p(i) + h >= lo
  while (x < y) {
    const uint32_t m = x + ((y - x) >> 1);
    if (oc_centre(a, ax, m) + hv >= lo)
      y = m;
    else
      x = m + 1;
  }
  i0 = (int32_t)x;
  x = 0, y = n;  // first i with !(p(i) - h <= hi)
  while (x < y) {
    const uint32_t m = x + ((y - x) >> 1);
    if (oc_centre(a, ax, m) - hv <= hi)
      x = m + 1;
    else
      y = m;
  }
  i1 = (int32_t)x - 1;
  outside = lo < oc_centre(a, ax, 0) - hv || hi > oc_centre(a, ax, n - 1) + hv;
}

__global__ void __launch_bounds__(OC_BLOCK) k_occ_cells(OcArgs a, uint64_t cells) {
  const uint64_t i = (uint64_t)blockIdx.x * OC_BLOCK + threadIdx.x;
  if (i >= cells) return;
  const uint32_t H = a.H;
  const uint32_t jz = (uint32_t)(i % H);
  const uint64_t q = i / H;
  const uint32_t jy = (uint32_t)(q % H);
  const uint64_t r = q / H;
  const uint32_t jx = (uint32_t)(r % H), cas = (uint32_t)(r / H);
  const float b = fminf(exp2f((float)cas), a.bound);
  int32_t x0, x1, y0, y1, z0, z1;
  bool ox, oy, oz;
  oc_axis(a, 0, jx, b, x0, x1, ox);
  oc_axis(a, 1, jy, b, y0, y1, oy);
  oc_axis(a, 2, jz, b, z0, z1, oz);
  bool keep = a.unknown_keeps && (ox || oy || oz);
  if (!keep && x0 <= x1 && y0 <= y1 && z0 <= z1) {
    const uint32_t w0 = (uint32_t)z0 >> 6, w1 = (uint32_t)z1 >> 6;
    const uint64_t first = ~0ull << ((uint32_t)z0 & 63u);
    const uint64_t last = ~0ull >> (63u - ((uint32_t)z1 & 63u));
    for (int32_t x = x0; x <= x1 && !keep; ++x) {
      for (int32_t y = y0; y <= y1 && !keep; ++y) {
        const uint64_t* row = a.bits + ((uint64_t)x * a.n[1] + (uint32_t)y) * a.nwz;
        for (uint32_t w = w0; w <= w1; ++w) {
          uint64_t m = ~0ull;
          if (w == w0) m &= first;
          if (w == w1) m &= last;
          if (row[w] & m) {
            keep = true;
            break;
          }
        }
      }
    }
  }
  a.mask[i] = keep ? 1 : 0;
}

}  // namespace

extern "C" uint64_t ucsa_tsdf_occupancy_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
  return 8ull * nx * ny * (((uint64_t)nz + 63u) / 64u);
}

extern "C" int32_t ucsa_tsdf_occupancy(const float* tsdf, const float* weight, uint32_t nx,
                                       uint32_t ny, uint32_t nz, const float* origin3,
                                       const float* spacing3, float min_weight, float free_tsdf,
                                       uint32_t unknown_keeps, float bound, uint32_t cascade,
                                       uint32_t H, float dilate, uint8_t* mask,
                                       uint64_t mask_capacity, void* workspace,
                                       uint64_t workspace_bytes, void* stream) {
  UCSA_CHECK_ARG(tsdf, 0);
  UCSA_CHECK_ARG(weight, 1);
  UCSA_CHECK_ARG(nx >= 1, 2);
  UCSA_CHECK_ARG(ny >= 1, 3);
  UCSA_CHECK_ARG(nz >= 1, 4);
  UCSA_CHECK_ARG((uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 2);
  UCSA_CHECK_ARG(origin3, 5);
  UCSA_CHECK_ARG(spacing3, 6);
  for (int r = 0; r < 3; ++r) {
    UCSA_CHECK_ARG(std::isfinite(origin3[r]), 5);
    UCSA_CHECK_ARG(spacing3[r] > 0.0f && std::isfinite(spacing3[r]), 6);
  }
  UCSA_CHECK_ARG(!std::isnan(min_weight), 7);
  UCSA_CHECK_ARG(!std::isnan(free_tsdf), 8);
  UCSA_CHECK_ARG(unknown_keeps <= 1, 9);
  UCSA_CHECK_ARG(bound > 0.0f && std::isfinite(bound), 10);
  UCSA_CHECK_ARG(cascade >= 1 && cascade <= 31, 11);
  UCSA_CHECK_ARG(H >= 2 && H <= 1024, 12);
  UCSA_CHECK_ARG(dilate >= 0.0f && std::isfinite(dilate), 13);
  UCSA_CHECK_ARG(mask, 14);
  const uint64_t cells = (uint64_t)cascade * H * H * H;
  UCSA_CHECK_ARG(mask_capacity >= cells, 15);
  UCSA_CHECK_ARG(workspace, 16);
  UCSA_CHECK_ARG(workspace_bytes >= ucsa_tsdf_occupancy_workspace_bytes(nx, ny, nz), 17);
  OcArgs a;
  a.tsdf = tsdf;
  a.weight = weight;
  a.bits = (uint64_t*)workspace;
  a.mask = mask;
  a.n[0] = nx;
  a.n[1] = ny;
  a.n[2] = nz;
  a.nwz = (nz + 63u) / 64u;
  for (int r = 0; r < 3; ++r) {
    a.o[r] = origin3[r];
    a.h[r] = spacing3[r];
    a.half[r] = 0.5f * spacing3[r];
  }
  a.min_weight = min_weight;
  a.free_tsdf = free_tsdf;
  a.bound = bound;
  a.dilate = dilate;
  a.unknown_keeps = unknown_keeps;
  a.cascade = cascade;
  a.H = H;
  const uint64_t words = (uint64_t)nx * ny * a.nwz;
  hipStream_t s = (hipStream_t)stream;
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_occ_pack, dim3(ucsa_div_up(words * 64u, OC_BLOCK)), dim3(OC_BLOCK), 0, s, a,
                     words);
  hipLaunchKernelGGL(k_occ_cells, dim3(ucsa_div_up(cells, OC_BLOCK)), dim3(OC_BLOCK), 0, s, a,
                     cells);
  return ucsa_launch_status();
}
