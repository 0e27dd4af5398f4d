// Surface voxelization of a triangle mesh (not in the reference):
// ucsa_mesh_voxelize_count and ucsa_mesh_voxelize_fill mark the cells of a
// lattice (a tsdf_volume's voxels) or of the marcher's cascade grid that some
// face meets.  The contract is stated in include/ucsa_hip.h; the predicate is
// tri_box.h; tests/voxelize_numpy.py restates both and the masks match it byte
// for byte.  A cell's value is a pure OR over the faces: every writer stores the
// constant 1 with a plain byte store, so no atomics, no order, and two runs
// give the same bytes.
//
// k_vx_count  a lane per item = (face, cascade): the corners, the slack, and per
//             axis the index interval of the cells whose boxes meet the face's
//             bounding interval, by two binary searches over the contract's own
//             box-axis predicate (monotone in the cell index: lo and hi are
//             non-decreasing), as oc_axis of occupancy_prior.hip does.  Writes
//             the index box (6 x int32) into the workspace and the number of its
//             (x, y) columns, 0 when a corner is invalid or an interval empty.
// (host)      the caller sums the counts (int64) and reads the total back.
// k_vx_fill   a lane per column: the item by an upper-bound binary search in
//             the offsets (at most 32 steps), (ix, iy) from the index inside
//             the item, then the z-run of the index box.  The three axes
//             unit_z x edge_i read x and y only: when one of them separates, the
//             whole column is skipped.  Every other cell of the run gets the six
//             remaining cross axes and the normal; the box axes hold on the
//             whole index box by construction.
// Work per lane: count 6 * ceil(log2(n + 1)) box-axis predicates; fill the
// search, 3 axes, then at most n_z cells of 7 axes.  A wall of 128 x 128 x 2
// cells is 16 384 lanes of 2 cells; a slanted scene-sized triangle 16 384 lanes
// of up to 128.  Every index read from the workspace or the offsets is tested
// against the dims before it is used.  No LDS.
#include <cmath>

#include "tri_box.h"
#include "ucsa_common.h"

namespace {

constexpr uint32_t VX_BLOCK = 256;

struct VxArgs {
  const float* verts;
  const int32_t* faces;
  uint32_t nv, nf;
  uint32_t family, n[3], ncas;
  float o[3], sp[3], half[3];
  float bound, dilate, bmax;
};

// lo / hi of cell j on axis ax (the header's two families)
__host__ __device__ __forceinline__ void vx_cell(const VxArgs& a, int ax, uint32_t cas, uint32_t j,
                                                 float& lo, float& hi) {
  if (a.family == UCSA_VOXELIZE_LATTICE) {
    const float p = a.o[ax] + (float)j * a.sp[ax];
    lo = (p - a.half[ax]) - a.dilate;
    hi = (p + a.half[ax]) + a.dilate;
  } else {
    const float b = fminf(ldexpf(1.0f, (int)cas), a.bound);
    const float Hf = (float)a.n[ax];
    lo = b * ((float)(2u * j) / Hf - 1.0f) - a.dilate;
    hi = b * ((float)(2u * j + 2u) / Hf - 1.0f) + a.dilate;
  }
}

// false: the face meets nothing (an index outside [0, nv) or tb_face_setup)
__device__ __forceinline__ bool vx_face(const VxArgs& a, uint32_t f, TbFace& t) {
  const uint32_t i0 = (uint32_t)a.faces[3ull * f], i1 = (uint32_t)a.faces[3ull * f + 1u],
                 i2 = (uint32_t)a.faces[3ull * f + 2u];
  if (!(i0 < a.nv && i1 < a.nv && i2 < a.nv)) return false;  // negative: a large unsigned
  return tb_face_setup(t, a.verts + 3ull * i0, a.verts + 3ull * i1, a.verts + 3ull * i2, a.bmax);
}

// One axis: the closed interval [i0, i1] of the cells whose boxes pass the
// box-axis test (empty when i0 > i1).  Each search keeps "every index below x
// fails, every index from y on passes" (the other way round for the second)
// and ends with x == y.
__device__ __forceinline__ void vx_axis(const VxArgs& a, const TbFace& t, int ax, uint32_t cas,
                                        int32_t& i0, int32_t& i1) {
  const uint32_t n = a.n[ax];
  float lo, hi;
  uint32_t x = 0, y = n;  // first i with mn <= hi(i) + slack
  while (x < y) {
    const uint32_t m = x + ((y - x) >> 1);
    vx_cell(a, ax, cas, m, lo, hi);
    if (t.mn[ax] <= hi + t.slack)
      y = m;
    else
      x = m + 1;
  }
  i0 = (int32_t)x;
  x = 0, y = n;  // first i with !(mx >= lo(i) - slack)
  while (x < y) {
    const uint32_t m = x + ((y - x) >> 1);
    vx_cell(a, ax, cas, m, lo, hi);
    if (t.mx[ax] >= lo - t.slack)
      x = m + 1;
    else
      y = m;
  }
  i1 = (int32_t)x - 1;
}

__global__ void __launch_bounds__(VX_BLOCK)
k_vx_count(VxArgs a, uint32_t items, int32_t* __restrict__ count, int32_t* __restrict__ boxes) {
  const uint32_t k = blockIdx.x * VX_BLOCK + threadIdx.x;
  if (k >= items) return;
  const uint32_t f = k / a.ncas, cas = k - f * a.ncas;
  int32_t b[6] = {0, -1, 0, -1, 0, -1};
  int32_t c = 0;
  TbFace t;
  if (vx_face(a, f, t)) {
    vx_axis(a, t, 0, cas, b[0], b[1]);
    vx_axis(a, t, 1, cas, b[2], b[3]);
    vx_axis(a, t, 2, cas, b[4], b[5]);
    if (b[0] <= b[1] && b[2] <= b[3] && b[4] <= b[5])
      c = (b[1] - b[0] + 1) * (b[3] - b[2] + 1);  // <= n_x * n_y <= 2^31 - 1
  }
  count[k] = c;
  for (int i = 0; i < 6; ++i) boxes[6ull * k + i] = b[i];
}

__global__ void __launch_bounds__(VX_BLOCK)
k_vx_fill(VxArgs a, uint32_t items, const int64_t* __restrict__ first, uint64_t total,
          const int32_t* __restrict__ boxes, uint8_t* __restrict__ mask) {
  const uint64_t s = (uint64_t)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (s >= total) return;
  // the smallest k in [0, items) with first[k + 1] > s: k + 1 <= items stays
  // inside first[items + 1] whatever the entries hold
  uint32_t lo = 0, hi = items;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (first[mid + 1u] > (int64_t)s)
      hi = mid;
    else
      lo = mid + 1u;
  }
  if (lo >= items) return;  // only a malformed `first`
  const uint32_t k = lo;
  const uint32_t f = k / a.ncas, cas = k - f * a.ncas;
  int32_t b[6];
  for (int i = 0; i < 6; ++i) b[i] = boxes[6ull * k + i];
  if (b[0] < 0 || b[2] < 0 || b[4] < 0 || b[1] >= (int32_t)a.n[0] || b[3] >= (int32_t)a.n[1] ||
      b[5] >= (int32_t)a.n[2] || b[0] > b[1] || b[2] > b[3] || b[4] > b[5])
    return;
  const int64_t j = (int64_t)s - first[k];
  const uint32_t wy = (uint32_t)(b[3] - b[2] + 1);
  if (j < 0 || j >= (int64_t)wy * (uint32_t)(b[1] - b[0] + 1)) return;
  const uint32_t ix = (uint32_t)b[0] + (uint32_t)(j / wy), iy = (uint32_t)b[2] + (uint32_t)(j % wy);
  TbFace t;
  if (!vx_face(a, f, t)) return;
  TbBox x;
  float l, h;
  vx_cell(a, 0, cas, ix, l, h);
  tb_box_axis(t, x, 0, l, h);
  vx_cell(a, 1, cas, iy, l, h);
  tb_box_axis(t, x, 1, l, h);
  if (!tb_cross_meets(t, x, 2)) return;  // unit_z x e_i: the same for the whole column
  uint8_t* col = mask + (((uint64_t)cas * a.n[0] + ix) * a.n[1] + iy) * a.n[2];
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (int32_t iz = b[4]; iz <= b[5]; ++iz) {
    vx_cell(a, 2, cas, (uint32_t)iz, l, h);
    tb_box_axis(t, x, 2, l, h);
    if (tb_cross_meets(t, x, 0) && tb_cross_meets(t, x, 1) && tb_normal_meets(t, x)) col[iz] = 1;
  }
}

// the arguments the two entries share: checks and the device copy
int32_t vx_args(VxArgs& a, const float* verts, uint32_t nv, const int32_t* faces, uint32_t nf,
                uint32_t family, uint32_t nx, uint32_t ny, uint32_t nz, const float* origin3,
                const float* spacing3, float bound, uint32_t cascade, float dilate) {
  UCSA_CHECK_ARG(nv <= 0x7FFFFFFFu, 1);
  UCSA_CHECK_ARG(nf <= 0x7FFFFFFFu, 3);
  UCSA_CHECK_ARG(nf == 0 || nv == 0 || verts, 0);
  UCSA_CHECK_ARG(nf == 0 || faces, 2);
  UCSA_CHECK_ARG(family == UCSA_VOXELIZE_LATTICE || family == UCSA_VOXELIZE_CASCADE, 4);
  UCSA_CHECK_ARG(dilate >= 0.0f && dilate <= TB_MAX_COORD, 12);  // NaN and inf fail
  a.verts = verts;
  a.faces = faces;
  a.nv = nv;
  a.nf = nf;
  a.family = family;
  a.n[0] = nx;
  a.n[1] = ny;
  a.n[2] = nz;
  a.dilate = dilate;
  if (family == UCSA_VOXELIZE_LATTICE) {
    UCSA_CHECK_ARG(nx >= 1, 5);
    UCSA_CHECK_ARG(ny >= 1, 6);
    UCSA_CHECK_ARG(nz >= 1, 7);
    UCSA_CHECK_ARG((uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 5);
    UCSA_CHECK_ARG(origin3, 8);
    UCSA_CHECK_ARG(spacing3, 9);
    UCSA_CHECK_ARG(cascade == 1, 11);
    a.bound = 0.0f;
    a.bmax = 0.0f;
    for (int r = 0; r < 3; ++r) {
      UCSA_CHECK_ARG(std::isfinite(origin3[r]), 8);
      UCSA_CHECK_ARG(spacing3[r] > 0.0f && std::isfinite(spacing3[r]), 9);
      a.o[r] = origin3[r];
      a.sp[r] = spacing3[r];
      a.half[r] = 0.5f * spacing3[r];
      float lo, hi, skip;
      vx_cell(a, r, 0, 0, lo, skip);
      vx_cell(a, r, 0, a.n[r] - 1u, skip, hi);
      a.bmax = fmaxf(a.bmax, fmaxf(fabsf(lo), fabsf(hi)));
    }
    UCSA_CHECK_ARG(a.bmax <= TB_MAX_COORD, 8);
  } else {
    UCSA_CHECK_ARG(nx >= 2 && nx <= 1024, 5);
    UCSA_CHECK_ARG(ny == nx, 6);
    UCSA_CHECK_ARG(nz == nx, 7);
    UCSA_CHECK_ARG(bound > 0.0f && std::isfinite(bound), 10);
    UCSA_CHECK_ARG(cascade >= 1 && cascade <= 31, 11);
    for (int r = 0; r < 3; ++r) a.o[r] = a.sp[r] = a.half[r] = 0.0f;
    a.bound = bound;
    a.bmax = fminf(ldexpf(1.0f, (int)cascade - 1), bound) + dilate;
  }
  a.ncas = cascade;
  UCSA_CHECK_ARG((uint64_t)nf * cascade <= 0x7FFFFFFFull, 3);
  return 0;
}

}  // namespace

extern "C" uint64_t ucsa_mesh_voxelize_workspace_bytes(uint32_t nf, uint32_t cascade) {
  return 24ull * nf * cascade;
}

extern "C" int32_t ucsa_mesh_voxelize_count(const float* verts, uint32_t nv, const int32_t* faces,
                                            uint32_t nf, uint32_t family, uint32_t nx, uint32_t ny,
                                            uint32_t nz, const float* origin3,
                                            const float* spacing3, float bound, uint32_t cascade,
                                            float dilate, int32_t* count, void* workspace,
                                            uint64_t workspace_bytes, void* stream) {
  VxArgs a;
  const int32_t rc = vx_args(a, verts, nv, faces, nf, family, nx, ny, nz, origin3, spacing3, bound,
                             cascade, dilate);
  if (rc) return rc;
  const uint32_t items = nf * cascade;
  if (items == 0) return 0;
  UCSA_CHECK_ARG(count, 13);
  UCSA_CHECK_ARG(workspace, 14);
  UCSA_CHECK_ARG(workspace_bytes >= ucsa_mesh_voxelize_workspace_bytes(nf, cascade), 15);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_vx_count, dim3(ucsa_div_up(items, VX_BLOCK)), dim3(VX_BLOCK), 0,
                     (hipStream_t)stream, a, items, count, (int32_t*)workspace);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_mesh_voxelize_fill(const float* verts, uint32_t nv, const int32_t* faces,
                                           uint32_t nf, uint32_t family, uint32_t nx, uint32_t ny,
                                           uint32_t nz, const float* origin3, const float* spacing3,
                                           float bound, uint32_t cascade, float dilate,
                                           const int64_t* first, uint64_t total,
                                           uint32_t accumulate, uint8_t* mask,
                                           uint64_t mask_capacity, const void* workspace,
                                           uint64_t workspace_bytes, void* stream) {
  VxArgs a;
  const int32_t rc = vx_args(a, verts, nv, faces, nf, family, nx, ny, nz, origin3, spacing3, bound,
                             cascade, dilate);
  if (rc) return rc;
  const uint32_t items = nf * cascade;
  UCSA_CHECK_ARG(total <= (1ull << 38), 14);
  UCSA_CHECK_ARG(items > 0 || total == 0, 14);  // a column lies in an item
  UCSA_CHECK_ARG(accumulate <= 1, 15);
  UCSA_CHECK_ARG(mask, 16);
  const uint64_t cells = (uint64_t)cascade * nx * ny * nz;
  UCSA_CHECK_ARG(mask_capacity >= cells, 17);
  if (total > 0) {
    UCSA_CHECK_ARG(first, 13);
    UCSA_CHECK_ARG(workspace, 18);
    UCSA_CHECK_ARG(workspace_bytes >= ucsa_mesh_voxelize_workspace_bytes(nf, cascade), 19);
  }
  hipStream_t s = (hipStream_t)stream;
  UCSA_CLEAR_ERR();
  if (!accumulate) {
    const hipError_t e = hipMemsetAsync(mask, 0, cells, s);
    if (e != hipSuccess) return -(int32_t)e;
  }
  if (total == 0) return 0;
  hipLaunchKernelGGL(k_vx_fill, dim3(ucsa_div_up(total, VX_BLOCK)), dim3(VX_BLOCK), 0, s, a, items,
                     first, total, (const int32_t*)workspace, mask);
  return ucsa_launch_status();
}
