// The depth front end (ucsa_depth_filter, ucsa_depth_normals,
// ucsa_depth_frontend): what KinectFusion does to a depth frame before it
// integrates or tracks it.  A table-driven bilateral filter, the back-projected
// point and a normal per pixel, and a mask that rejects depth edges and grazing
// views.  Not in the reference.  The contracts are stated in include/ucsa_hip.h;
// tests/depth_numpy.py restates them in numpy and every output matches it bit
// for bit.
//
// k_depth<MODE, R>  one thread per pixel, a work-group per 16 x 16 tile.
//   MODE 0 (filter)   the tile with a halo of R raw pixels goes to LDS once; a
//                     thread walks its (2R+1)^2 window there.
//   MODE 1 (normals)  the tile with a halo of one pixel goes to LDS; a thread
//                     reads its eight neighbours there.
//   MODE 2 (fused)    the tile with a halo of R + 1 raw pixels goes to LDS, the
//                     work-group filters the 18 x 18 region (324 pixels over 256
//                     threads: two passes) into a second LDS tile, and MODE 1's
//                     code runs on that.  The halo's filtered values are
//                     recomputed by the neighbouring work-groups from the same
//                     inputs in the same order, so they are the same bits and
//                     the outputs are those of MODE 0 followed by MODE 1.
// A pixel outside the image is a NaN in LDS: it is not measured, which is all
// the contracts ask of it, so no code below tests an image bound again.  The two
// weight tables sit in LDS as well (w_range is gathered by value).  Rows of
// both tiles are DF_STRIDE = 48 floats apart: a wave covers four tile rows of 16
// lanes and 48 = 16 mod 32 puts the two rows of a 32-lane group on disjoint
// banks for every tap.  No atomics, no scratch; R is a template argument so
// that the window loops unroll.
//
// k_depth_confidence  (ucsa_depth_confidence) one thread per pixel, no LDS: the
//                     weight of a pixel's measurement for
//                     ucsa_tsdf_integrate_weighted from the points, normals and
//                     mask above; tests/weighted_numpy.py restates it.
//
// k_depth_pyramid_down  (ucsa_depth_pyramid_down) one thread per coarse pixel, no
//                     LDS: one level of the depth pyramid of coarse-to-fine
//                     tracking; tests/projective_numpy.py restates it.
#include <cmath>

#include "ucsa_common.h"

namespace {

constexpr int DF_TILE = 16;
constexpr int DF_MAXR = 4;
constexpr int DF_Q = 256;
constexpr int DF_STRIDE = 48;
constexpr int DF_RAW_ROWS = DF_TILE + 2 + 2 * DF_MAXR;  // 26
constexpr int DF_F_ROWS = DF_TILE + 2;                  // 18
constexpr uint32_t DF_MAXB = 65535;                     // images per launch (grid.y)

struct DfArgs {
  const float* depth;
  const float* w_space;
  const float* w_range;
  float* filtered;
  float* clean;
  float* points;
  float* normals;
  uint8_t* mask;
  uint32_t H, W, tiles_x;
  float fx, fy, cx, cy, dmin, dmax;
  float sigma_depth, sigma_z2, max_jump, max_jump_z2, min_cos;
  uint32_t reject;
};

__device__ __forceinline__ bool df_measured(const DfArgs& a, float z) {
  return isfinite(z) && z >= a.dmin && z <= a.dmax;
}

// the filtered value of the pixel at (ly, lx) of the raw tile s (rows DF_STRIDE apart)
template <int R>
__device__ __forceinline__ float df_filter(const DfArgs& a, const float* s, const float* s_ws,
                                           const float* s_wr, int ly, int lx) {
  const float z = s[ly * DF_STRIDE + lx];
  if (!df_measured(a, z)) return 0.0f;
  const float sigma = a.sigma_depth + a.sigma_z2 * (z * z);
  const float scale = (float)DF_Q / (3.0f * sigma);
  float num = 0.0f, den = 0.0f;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      const float zn = s[(ly + dy) * DF_STRIDE + (lx + dx)];
      if (!df_measured(a, zn)) continue;
      const float d = zn - z;
      const float t = fabsf(d) * scale;
      if (!(t < (float)DF_Q)) continue;
      const float w = s_ws[(dy + R) * (2 * R + 1) + (dx + R)] * s_wr[(int)t];
      num = num + w * d;
      den = den + w;
    }
  }
  return z + num / den;
}

__device__ __forceinline__ void df_point(const DfArgs& a, int i, int j, float z, float p[3]) {
  p[0] = ((((float)j + 0.5f) - a.cx) / a.fx) * z;
  p[1] = ((((float)i + 0.5f) - a.cy) / a.fy) * z;
  p[2] = z;
}

// one axis of the tangent: minus at (im, jm) with depth zm, plus at (ip, jp) with zp
__device__ __forceinline__ bool df_diff(const DfArgs& a, const float p[3], bool um, bool up, int im,
                                        int jm, float zm, int ip, int jp, float zp, float d[3]) {
  if (!um && !up) return false;
  float lo[3], hi[3];
  if (um)
    df_point(a, im, jm, zm, lo);
  else
    lo[0] = p[0], lo[1] = p[1], lo[2] = p[2];
  if (up)
    df_point(a, ip, jp, zp, hi);
  else
    hi[0] = p[0], hi[1] = p[1], hi[2] = p[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) d[r] = hi[r] - lo[r];
  return true;
}

// points, normals, mask (and clean) of pixel (i, j) from the tile s of depths
// with a halo of one: the pixel sits at (ly, lx)
template <bool CLEAN>
__device__ __forceinline__ void df_normals(const DfArgs& a, const float* s, int ly, int lx, int i,
                                           int j, size_t pix) {
  const float z = s[ly * DF_STRIDE + lx];
  float p[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f};
  uint32_t m = 0u;
  if (df_measured(a, z)) {
    m = 1u;
    df_point(a, i, j, z, p);
    const float thr = a.max_jump + a.max_jump_z2 * (z * z);
    float zn[3][3];
    bool us[3][3];
    bool edge = false;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const float v = s[(ly + dy) * DF_STRIDE + (lx + dx)];
        const bool meas = df_measured(a, v);
        const bool use = meas && fabsf(v - z) <= thr;
        zn[dy + 1][dx + 1] = v;
        us[dy + 1][dx + 1] = use;
        if ((dy != 0 || dx != 0) && meas && !use) edge = true;
      }
    }
    if (edge) m |= 4u;
    float du[3], dv[3];
    const bool hu = df_diff(a, p, us[1][0], us[1][2], i, j - 1, zn[1][0], i, j + 1, zn[1][2], du);
    const bool hv = df_diff(a, p, us[0][1], us[2][1], i - 1, j, zn[0][1], i + 1, j, zn[2][1], dv);
    if (hu && hv) {
      float c[3];
      c[0] = dv[1] * du[2] - dv[2] * du[1];
      c[1] = dv[2] * du[0] - dv[0] * du[2];
      c[2] = dv[0] * du[1] - dv[1] * du[0];
      const float nn = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
      if (nn > 0.0f && isfinite(nn)) {
        const float len = sqrtf(nn);
#pragma unroll
        for (int r = 0; r < 3; ++r) n[r] = c[r] / len;
        float dot = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2];
        if (dot > 0.0f) {
#pragma unroll
          for (int r = 0; r < 3; ++r) n[r] = -n[r];
          dot = -dot;
        }
        const float cosv = (-dot) / sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
        m |= 2u;
        if (cosv < a.min_cos) m |= 8u;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    a.points[3 * pix + r] = p[r];
    a.normals[3 * pix + r] = n[r];
  }
  a.mask[pix] = (uint8_t)m;
  if (CLEAN) {
    a.filtered[pix] = z;
    a.clean[pix] = (m & a.reject) ? 0.0f : z;
  }
}

// rows x cols floats of image b around (i0, j0) -> s, NaN outside the image
__device__ __forceinline__ void df_load(const DfArgs& a, const float* img, float* s, int i0, int j0,
                                        int rows, int cols, int tid) {
  for (int e = tid; e < rows * cols; e += DF_TILE * DF_TILE) {
    const int y = e / cols, x = e - y * cols;
    const int gi = i0 + y, gj = j0 + x;
    float v = __builtin_nanf("");
    if (gi >= 0 && gi < (int)a.H && gj >= 0 && gj < (int)a.W) v = img[(size_t)gi * a.W + gj];
    s[y * DF_STRIDE + x] = v;
  }
}

template <int MODE, int R>
__global__ void __launch_bounds__(DF_TILE* DF_TILE) k_depth(DfArgs a) {
  __shared__ float s_raw[MODE == 1 ? 1 : DF_RAW_ROWS * DF_STRIDE];
  __shared__ float s_f[MODE == 0 ? 1 : DF_F_ROWS * DF_STRIDE];
  __shared__ float s_ws[(2 * DF_MAXR + 1) * (2 * DF_MAXR + 1)];
  __shared__ float s_wr[DF_Q];
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * DF_TILE + tx;
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
  const int i0 = tile_y * DF_TILE, j0 = tile_x * DF_TILE;
  const int i = i0 + ty, j = j0 + tx;
  const size_t image = (size_t)blockIdx.y * a.H * a.W;
  const float* img = a.depth + image;
  const bool inside = i < (int)a.H && j < (int)a.W;
  const size_t pix = image + (size_t)i * a.W + j;

  if (MODE != 1) {
    constexpr int HALO = MODE == 0 ? R : R + 1, T = DF_TILE + 2 * HALO;
    df_load(a, img, s_raw, i0 - HALO, j0 - HALO, T, T, tid);
    if (tid < (2 * R + 1) * (2 * R + 1)) s_ws[tid] = a.w_space[tid];
    s_wr[tid] = a.w_range[tid];  // DF_Q = the 256 threads
    __syncthreads();
    if (MODE == 0) {
      if (inside) a.filtered[pix] = df_filter<R>(a, s_raw, s_ws, s_wr, ty + R, tx + R);
      return;
    }
    for (int e = tid; e < DF_F_ROWS * DF_F_ROWS; e += DF_TILE * DF_TILE) {
      const int y = e / DF_F_ROWS, x = e - y * DF_F_ROWS;
      const int gi = i0 - 1 + y, gj = j0 - 1 + x;
      float v = __builtin_nanf("");
      if (gi >= 0 && gi < (int)a.H && gj >= 0 && gj < (int)a.W)
        v = df_filter<R>(a, s_raw, s_ws, s_wr, y + R, x + R);
      s_f[y * DF_STRIDE + x] = v;
    }
  } else {
    df_load(a, img, s_f, i0 - 1, j0 - 1, DF_F_ROWS, DF_F_ROWS, tid);
  }
  __syncthreads();
  if (inside) df_normals<MODE == 2>(a, s_f, ty + 1, tx + 1, i, j, pix);
}

template <int MODE>
void df_launch(int r, dim3 grid, hipStream_t s, const DfArgs& a) {
  const dim3 block(DF_TILE, DF_TILE);
  switch (r) {
    case 1: hipLaunchKernelGGL((k_depth<MODE, 1>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_depth<MODE, 2>), grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL((k_depth<MODE, 3>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((k_depth<MODE, 4>), grid, block, 0, s, a); break;
  }
}

// MODE's launches over B images, DF_MAXB per launch
template <int MODE>
int32_t df_run(DfArgs a, uint32_t B, int r, void* stream) {
  a.tiles_x = ucsa_div_up(a.W, DF_TILE);
  const uint32_t tiles = a.tiles_x * ucsa_div_up(a.H, DF_TILE);
  const size_t hw = (size_t)a.H * a.W;
  UCSA_CLEAR_ERR();
  for (uint32_t b0 = 0; b0 < B; b0 += DF_MAXB) {
    DfArgs c = a;
    const size_t off = (size_t)b0 * hw;
    c.depth = a.depth + off;
    if (a.filtered) c.filtered = a.filtered + off;
    if (a.clean) c.clean = a.clean + off;
    if (a.points) c.points = a.points + 3 * off;
    if (a.normals) c.normals = a.normals + 3 * off;
    if (a.mask) c.mask = a.mask + off;
    const dim3 grid(tiles, B - b0 < DF_MAXB ? B - b0 : DF_MAXB);
    if constexpr (MODE == 1)
      hipLaunchKernelGGL((k_depth<1, 1>), grid, dim3(DF_TILE, DF_TILE), 0, (hipStream_t)stream, c);
    else
      df_launch<MODE>(r, grid, (hipStream_t)stream, c);
  }
  return ucsa_launch_status();
}

// ucsa_depth_confidence: the weight a pixel's measurement gets in
// ucsa_tsdf_integrate_weighted.  One thread per pixel, 28 bytes in and 4 out,
// no LDS, no atomics: the kernel is its loads.
constexpr int DC_BLOCK = 256;

struct DcArgs {
  const float* points;
  const float* normals;
  const uint8_t* mask;
  float* weight;
  uint32_t hw;
  float sigma_depth, sigma_z2, cos_floor;
  uint32_t reject;
};

__global__ void __launch_bounds__(DC_BLOCK) k_depth_confidence(DcArgs a) {
  const uint32_t e = blockIdx.x * DC_BLOCK + threadIdx.x;
  if (e >= a.hw) return;
  const size_t pix = (size_t)blockIdx.y * a.hw + e;
  const uint32_t m = a.mask[pix];
  float w = 0.0f;
  if ((m & 1u) && !(m & a.reject)) {
    const float p0 = a.points[3 * pix], p1 = a.points[3 * pix + 1], p2 = a.points[3 * pix + 2];
    const float sigma = a.sigma_depth + a.sigma_z2 * (p2 * p2);
    const float s = a.sigma_depth / sigma;
    const float wz = s * s;
    float wa = a.cos_floor;
    if (m & 2u) {
      const float n0 = a.normals[3 * pix], n1 = a.normals[3 * pix + 1], n2 = a.normals[3 * pix + 2];
      const float dot = (n0 * p0 + n1 * p1) + n2 * p2;
      const float cosv = (-dot) / sqrtf((p0 * p0 + p1 * p1) + p2 * p2);
      wa = fminf(fmaxf(cosv, a.cos_floor), 1.0f);  // a NaN cosv gives cos_floor
    }
    w = wz * wa;
  }
  a.weight[pix] = w;
}

// ucsa_depth_pyramid_down: one level of the depth pyramid.  One thread per
// coarse pixel, up to four loads and one store, no LDS, no atomics.  A member of
// the 2 x 2 block is read only where it exists: 2I + dy < H and 2J + dx < W.
struct DpArgs {
  const float* depth;
  float* out;
  uint32_t H, W, h, w;
  float dmin, dmax, max_jump, max_jump_z2;
};

__global__ void __launch_bounds__(DC_BLOCK) k_depth_pyramid_down(DpArgs a) {
  const uint32_t e = blockIdx.x * DC_BLOCK + threadIdx.x;
  if (e >= a.h * a.w) return;
  const uint32_t I = e / a.w, J = e - I * a.w;
  const float* img = a.depth + (size_t)blockIdx.y * a.H * a.W;
  float z[4];
  bool ok[4];
  float z0 = INFINITY;
  bool any = false;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {  // row-major over the block
    const uint32_t i = 2u * I + (k >> 1), j = 2u * J + (k & 1u);
    z[k] = 0.0f;
    ok[k] = false;
    if (i < a.H && j < a.W) {
      z[k] = img[(size_t)i * a.W + j];
      ok[k] = isfinite(z[k]) && z[k] >= a.dmin && z[k] <= a.dmax;
    }
    if (ok[k]) {
      if (z[k] < z0) z0 = z[k];  // the first of equal ones: a -0.0 after a +0.0 does not replace it
      any = true;
    }
  }
  float r = 0.0f;
  if (any) {
    const float thr = a.max_jump + a.max_jump_z2 * (z0 * z0);
    float s = 0.0f, count = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = z[k] - z0;
      if (ok[k] && d <= thr) {
        s = s + d;
        count = count + 1.0f;
      }
    }
    r = z0 + s / count;
  }
  a.out[(size_t)blockIdx.y * a.h * a.w + e] = r;
}

}  // namespace

// the frames: arguments k0 .. k0 + 3 of every entry point
#define DF_CHECK_FRAME(k0)                                \
  UCSA_CHECK_ARG(depth, (k0));                            \
  UCSA_CHECK_ARG(B >= 1, (k0) + 1);                       \
  UCSA_CHECK_ARG(H >= 1 && H <= 16384, (k0) + 2);         \
  UCSA_CHECK_ARG(W >= 1 && W <= 16384, (k0) + 3)

extern "C" int32_t ucsa_depth_filter(const float* depth, uint32_t B, uint32_t H, uint32_t W,
                                     const float* w_space, uint32_t radius, const float* w_range,
                                     float sigma_depth, float sigma_z2, float depth_min,
                                     float depth_max, float* filtered, void* stream) {
  DF_CHECK_FRAME(0);
  UCSA_CHECK_ARG(w_space, 4);
  UCSA_CHECK_ARG(radius >= 1 && radius <= (uint32_t)DF_MAXR, 5);
  UCSA_CHECK_ARG(w_range, 6);
  UCSA_CHECK_ARG(sigma_depth > 0.0f && std::isfinite(sigma_depth), 7);
  UCSA_CHECK_ARG(sigma_z2 >= 0.0f && std::isfinite(sigma_z2), 8);
  UCSA_CHECK_ARG(!std::isnan(depth_min), 9);
  UCSA_CHECK_ARG(depth_max >= depth_min, 10);
  UCSA_CHECK_ARG(filtered && filtered != depth, 11);
  DfArgs a = {};
  a.depth = depth;
  a.w_space = w_space;
  a.w_range = w_range;
  a.filtered = filtered;
  a.H = H;
  a.W = W;
  a.dmin = depth_min;
  a.dmax = depth_max;
  a.sigma_depth = sigma_depth;
  a.sigma_z2 = sigma_z2;
  return df_run<0>(a, B, (int)radius, stream);
}

extern "C" int32_t ucsa_depth_normals(const float* depth, uint32_t B, uint32_t H, uint32_t W,
                                      float fx, float fy, float cx, float cy, float max_jump,
                                      float max_jump_z2, float min_cos, float depth_min,
                                      float depth_max, float* points, float* normals,
                                      uint8_t* mask, void* stream) {
  DF_CHECK_FRAME(0);
  UCSA_CHECK_ARG(fx > 0.0f && std::isfinite(fx), 4);
  UCSA_CHECK_ARG(fy > 0.0f && std::isfinite(fy), 5);
  UCSA_CHECK_ARG(std::isfinite(cx), 6);
  UCSA_CHECK_ARG(std::isfinite(cy), 7);
  UCSA_CHECK_ARG(max_jump >= 0.0f && std::isfinite(max_jump), 8);
  UCSA_CHECK_ARG(max_jump_z2 >= 0.0f && std::isfinite(max_jump_z2), 9);
  UCSA_CHECK_ARG(min_cos >= -1.0f && min_cos <= 1.0f, 10);
  UCSA_CHECK_ARG(!std::isnan(depth_min), 11);
  UCSA_CHECK_ARG(depth_max >= depth_min, 12);
  UCSA_CHECK_ARG(points, 13);
  UCSA_CHECK_ARG(normals, 14);
  UCSA_CHECK_ARG(mask, 15);
  DfArgs a = {};
  a.depth = depth;
  a.points = points;
  a.normals = normals;
  a.mask = mask;
  a.H = H;
  a.W = W;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.dmin = depth_min;
  a.dmax = depth_max;
  a.max_jump = max_jump;
  a.max_jump_z2 = max_jump_z2;
  a.min_cos = min_cos;
  return df_run<1>(a, B, 1, stream);
}

extern "C" int32_t ucsa_depth_frontend(const float* depth, uint32_t B, uint32_t H, uint32_t W,
                                       const float* w_space, uint32_t radius,
                                       const float* w_range, float sigma_depth, float sigma_z2,
                                       float fx, float fy, float cx, float cy, float max_jump,
                                       float max_jump_z2, float min_cos, uint32_t reject,
                                       float depth_min, float depth_max, float* filtered,
                                       float* clean, float* points, float* normals,
                                       uint8_t* mask, void* stream) {
  DF_CHECK_FRAME(0);
  UCSA_CHECK_ARG(w_space, 4);
  UCSA_CHECK_ARG(radius >= 1 && radius <= (uint32_t)DF_MAXR, 5);
  UCSA_CHECK_ARG(w_range, 6);
  UCSA_CHECK_ARG(sigma_depth > 0.0f && std::isfinite(sigma_depth), 7);
  UCSA_CHECK_ARG(sigma_z2 >= 0.0f && std::isfinite(sigma_z2), 8);
  UCSA_CHECK_ARG(fx > 0.0f && std::isfinite(fx), 9);
  UCSA_CHECK_ARG(fy > 0.0f && std::isfinite(fy), 10);
  UCSA_CHECK_ARG(std::isfinite(cx), 11);
  UCSA_CHECK_ARG(std::isfinite(cy), 12);
  UCSA_CHECK_ARG(max_jump >= 0.0f && std::isfinite(max_jump), 13);
  UCSA_CHECK_ARG(max_jump_z2 >= 0.0f && std::isfinite(max_jump_z2), 14);
  UCSA_CHECK_ARG(min_cos >= -1.0f && min_cos <= 1.0f, 15);
  UCSA_CHECK_ARG((reject & ~(UCSA_DEPTH_EDGE | UCSA_DEPTH_GRAZING)) == 0u, 16);
  UCSA_CHECK_ARG(!std::isnan(depth_min), 17);
  UCSA_CHECK_ARG(depth_max >= depth_min, 18);
  UCSA_CHECK_ARG(filtered && filtered != depth, 19);
  UCSA_CHECK_ARG(clean && clean != depth && clean != filtered, 20);
  UCSA_CHECK_ARG(points, 21);
  UCSA_CHECK_ARG(normals, 22);
  UCSA_CHECK_ARG(mask, 23);
  DfArgs a = {};
  a.depth = depth;
  a.w_space = w_space;
  a.w_range = w_range;
  a.filtered = filtered;
  a.clean = clean;
  a.points = points;
  a.normals = normals;
  a.mask = mask;
  a.H = H;
  a.W = W;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.dmin = depth_min;
  a.dmax = depth_max;
  a.sigma_depth = sigma_depth;
  a.sigma_z2 = sigma_z2;
  a.max_jump = max_jump;
  a.max_jump_z2 = max_jump_z2;
  a.min_cos = min_cos;
  a.reject = reject;
  return df_run<2>(a, B, (int)radius, stream);
}

extern "C" int32_t ucsa_depth_confidence(const float* points, const float* normals,
                                         const uint8_t* mask, uint32_t B, uint32_t H, uint32_t W,
                                         float sigma_depth, float sigma_z2, float cos_floor,
                                         uint32_t reject, float* weight, void* stream) {
  UCSA_CHECK_ARG(points, 0);
  UCSA_CHECK_ARG(normals, 1);
  UCSA_CHECK_ARG(mask, 2);
  UCSA_CHECK_ARG(B >= 1, 3);
  UCSA_CHECK_ARG(H >= 1 && H <= 16384, 4);
  UCSA_CHECK_ARG(W >= 1 && W <= 16384, 5);
  UCSA_CHECK_ARG(sigma_depth > 0.0f && std::isfinite(sigma_depth), 6);
  UCSA_CHECK_ARG(sigma_z2 >= 0.0f && std::isfinite(sigma_z2), 7);
  UCSA_CHECK_ARG(cos_floor > 0.0f && cos_floor <= 1.0f, 8);
  UCSA_CHECK_ARG((reject & ~(UCSA_DEPTH_EDGE | UCSA_DEPTH_GRAZING)) == 0u, 9);
  const size_t n = (size_t)B * H * W;
  // weight [n] floats shares no byte with an input
  const auto apart = [&](const void* p, size_t bytes) {
    const char *w0 = (const char*)weight, *q0 = (const char*)p;
    return w0 + 4 * n <= q0 || q0 + bytes <= w0;
  };
  UCSA_CHECK_ARG(weight && apart(points, 12 * n) && apart(normals, 12 * n) && apart(mask, n), 10);
  DcArgs a;
  a.hw = H * W;
  a.sigma_depth = sigma_depth;
  a.sigma_z2 = sigma_z2;
  a.cos_floor = cos_floor;
  a.reject = reject;
  UCSA_CLEAR_ERR();
  for (uint32_t b0 = 0; b0 < B; b0 += DF_MAXB) {
    const size_t off = (size_t)b0 * a.hw;
    a.points = points + 3 * off;
    a.normals = normals + 3 * off;
    a.mask = mask + off;
    a.weight = weight + off;
    const dim3 grid(ucsa_div_up(a.hw, DC_BLOCK), B - b0 < DF_MAXB ? B - b0 : DF_MAXB);
    hipLaunchKernelGGL(k_depth_confidence, grid, dim3(DC_BLOCK), 0, (hipStream_t)stream, a);
  }
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_depth_pyramid_down(const float* depth, uint32_t B, uint32_t H, uint32_t W,
                                           float max_jump, float max_jump_z2, float depth_min,
                                           float depth_max, float* coarse, void* stream) {
  DF_CHECK_FRAME(0);
  UCSA_CHECK_ARG(max_jump >= 0.0f && std::isfinite(max_jump), 4);
  UCSA_CHECK_ARG(max_jump_z2 >= 0.0f && std::isfinite(max_jump_z2), 5);
  UCSA_CHECK_ARG(!std::isnan(depth_min), 6);
  UCSA_CHECK_ARG(depth_max >= depth_min, 7);
  DpArgs a;
  a.H = H;
  a.W = W;
  a.h = ucsa_div_up(H, 2u);
  a.w = ucsa_div_up(W, 2u);
  const size_t hw = (size_t)H * W, chw = (size_t)a.h * a.w;
  // coarse [B][h][w] floats shares no byte with depth
  const char *c0 = (const char*)coarse, *d0 = (const char*)depth;
  UCSA_CHECK_ARG(coarse && (c0 + 4 * chw * B <= d0 || d0 + 4 * hw * B <= c0), 8);
  a.dmin = depth_min;
  a.dmax = depth_max;
  a.max_jump = max_jump;
  a.max_jump_z2 = max_jump_z2;
  UCSA_CLEAR_ERR();
  for (uint32_t b0 = 0; b0 < B; b0 += DF_MAXB) {
    a.depth = depth + (size_t)b0 * hw;
    a.out = coarse + (size_t)b0 * chw;
    const dim3 grid(ucsa_div_up((uint32_t)chw, DC_BLOCK), B - b0 < DF_MAXB ? B - b0 : DF_MAXB);
    hipLaunchKernelGGL(k_depth_pyramid_down, grid, dim3(DC_BLOCK), 0, (hipStream_t)stream, a);
  }
  return ucsa_launch_status();
}
