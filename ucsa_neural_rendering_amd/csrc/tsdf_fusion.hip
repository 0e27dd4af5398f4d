// Projective TSDF integration (ucsa_tsdf_integrate): posed depth frames fused
// into a dense truncated-signed-distance volume, the first stage of the mapping
// chain (volume -> marching cubes -> label fusion -> rasterizer).  Not in the
// reference.  The contract is stated in include/ucsa_hip.h; tests/tsdf_numpy.py
// restates it in numpy and the volumes match it bit for bit.
//
// k_tsdf_integrate  one thread per voxel, a work-group per brick of
//                   1 x TS_BJ x 64 voxels (i, j, k): k, the contiguous index,
//                   runs across the lanes of a wave, so the state loads and
//                   stores coalesce.  A voxel's state (tsdf, weight, rgb) is
//                   read once, carried in registers through up to TS_MAXB views
//                   in ascending order and written once (not at all when no
//                   view touched it): the volume's traffic per view falls with
//                   the number of views per launch.  The depth images are
//                   gathered (nearest pixel); neighbouring k project to
//                   neighbouring pixels, so a wave's gather stays within a few
//                   rows of one image.
//   brick cull      before the loop, thread 8*v + c takes corner c of the brick
//                   for view v; one thread per view then decides from the eight
//                   camera points whether the view can touch the brick at all
//                   (behind the camera, beyond depth_max + trunc, outside the
//                   image).  The tests are conservative by construction (see
//                   ts_cull) and a culled view is exactly a view that every
//                   voxel of the brick would have skipped: no bit changes.
// No atomics, no LDS beyond the cull's 32 x 8 points.  A call with more than
// TS_MAXB views is a sequence of launches on the stream, in view order.
//
// ucsa_tsdf_integrate_weighted is the same kernel with WEIGHTED set: a view's
// measurement counts with pixel_weight[b][v][u] instead of 1.  The weight is
// gathered with the depth's own index, next to the depth gather; the view loop,
// the cull and the state traffic are shared, and the unweighted instantiation
// compiles to the code it was.
#include <cmath>

#include "tsdf_project.h"
#include "ucsa_common.h"

namespace {

constexpr uint32_t TS_BK = 64;    // brick extent along k = one wave
constexpr uint32_t TS_BJ = 4;     // along j = waves per work-group
constexpr uint32_t TS_MAXB = 32;  // views per launch = TS_BK * TS_BJ / 8 corners

struct TsArgs {
  float* tsdf;
  float* weight;
  float* rgb;
  const float* depth;
  const uint8_t* color;
  const float* poses;
  uint32_t nx, ny, nz, B, H, W;
  float o[3], h[3];
  float fx, fy, cx, cy, trunc, max_weight, dmin, dmax;
  const float* pixel_weight;  // [B,H,W], WEIGHTED only (last: the other offsets stay)
};

template <bool COLOR, bool WEIGHTED>
__global__ void __launch_bounds__(TS_BK* TS_BJ) k_tsdf_integrate(TsArgs a) {
  __shared__ float s_c[TS_MAXB][8][3];
  __shared__ uint32_t s_cull;
  const uint32_t tid = threadIdx.y * TS_BK + threadIdx.x;
  const uint32_t i = blockIdx.z, j0 = blockIdx.y * TS_BJ, k0 = blockIdx.x * TS_BK;
  const uint32_t j1 = min(j0 + TS_BJ - 1u, a.ny - 1u), k1 = min(k0 + TS_BK - 1u, a.nz - 1u);
  float lo[3], hi[3];
  lo[0] = hi[0] = a.o[0] + (float)i * a.h[0];
  lo[1] = a.o[1] + (float)j0 * a.h[1];
  hi[1] = a.o[1] + (float)j1 * a.h[1];
  lo[2] = a.o[2] + (float)k0 * a.h[2];
  hi[2] = a.o[2] + (float)k1 * a.h[2];
  // a negative spacing runs the other way: order the box
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
    // i is one plane: corners 4..7 repeat 0..3
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
  const size_t idx = ((size_t)i * a.ny + j) * a.nz + k;
  const float p[3] = {lo[0], a.o[1] + (float)j * a.h[1], a.o[2] + (float)k * a.h[2]};
  float tsdf = a.tsdf[idx], w = a.weight[idx];
  float rgb[3] = {0.0f, 0.0f, 0.0f};
  if (COLOR) {
#pragma unroll
    for (int r = 0; r < 3; ++r) rgb[r] = a.rgb[3 * idx + r];
  }
  bool dirty = false;
  const float fW = (float)a.W, fH = (float)a.H;
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
    float pw = 1.0f;
    if constexpr (WEIGHTED) pw = a.pixel_weight[pix];  // pix is in range: the depth's index
    if (!(isfinite(d) && d >= a.dmin && d <= a.dmax)) continue;
    if constexpr (WEIGHTED) {
      if (!(pw > 0.0f && isfinite(pw))) continue;
    }
    const float sdf = d - c[2];
    if (sdf < -a.trunc) continue;
    const float val = fminf(1.0f, sdf / a.trunc);
    float w1;
    if constexpr (WEIGHTED) {
      w1 = w + pw;
      tsdf = (tsdf * w + val * pw) / w1;
      if (COLOR) {
#pragma unroll
        for (int r = 0; r < 3; ++r) rgb[r] = (rgb[r] * w + (float)a.color[3 * pix + r] * pw) / w1;
      }
    } else {
      w1 = w + 1.0f;
      tsdf = (tsdf * w + val) / w1;
      if (COLOR) {
#pragma unroll
        for (int r = 0; r < 3; ++r) rgb[r] = (rgb[r] * w + (float)a.color[3 * pix + r]) / w1;
      }
    }
    w = fminf(w1, a.max_weight);
    dirty = true;
  }
  if (!dirty) return;
  a.tsdf[idx] = tsdf;
  a.weight[idx] = w;
  if (COLOR) {
#pragma unroll
    for (int r = 0; r < 3; ++r) a.rgb[3 * idx + r] = rgb[r];
  }
}

// both entry points; weighted: ucsa_tsdf_integrate_weighted, whose arguments
// after depth sit one index higher
int32_t ts_integrate(float* tsdf, float* weight, float* rgb, uint32_t nx, uint32_t ny,
                     uint32_t nz, const float* origin3, const float* spacing3,
                     const float* depth, const float* pixel_weight, const uint8_t* color,
                     const float* poses, uint32_t B, float fx, float fy, float cx, float cy,
                     uint32_t H, uint32_t W, float trunc, float max_weight, float depth_min,
                     float depth_max, void* stream, bool weighted) {
  const int s = weighted ? 1 : 0;
  UCSA_CHECK_ARG(tsdf, 0);
  UCSA_CHECK_ARG(weight, 1);
  UCSA_CHECK_ARG((rgb == nullptr) == (color == nullptr), rgb ? 9 + s : 2);
  UCSA_CHECK_ARG(nx >= 2 && (uint64_t)nx * ny * nz <= 0x7FFFFFFFull, 3);
  UCSA_CHECK_ARG(ny >= 2, 4);
  UCSA_CHECK_ARG(nz >= 2, 5);
  UCSA_CHECK_ARG(origin3, 6);
  UCSA_CHECK_ARG(spacing3, 7);
  UCSA_CHECK_ARG(depth, 8);
  UCSA_CHECK_ARG(!weighted || pixel_weight, 9);
  UCSA_CHECK_ARG(poses, 10 + s);
  UCSA_CHECK_ARG(B >= 1, 11 + s);
  UCSA_CHECK_ARG(fx > 0.0f && std::isfinite(fx), 12 + s);
  UCSA_CHECK_ARG(fy > 0.0f && std::isfinite(fy), 13 + s);
  UCSA_CHECK_ARG(std::isfinite(cx), 14 + s);
  UCSA_CHECK_ARG(std::isfinite(cy), 15 + s);
  UCSA_CHECK_ARG(H >= 1 && H <= 16384, 16 + s);
  UCSA_CHECK_ARG(W >= 1 && W <= 16384, 17 + s);
  UCSA_CHECK_ARG(trunc > 0.0f && std::isfinite(trunc), 18 + s);
  UCSA_CHECK_ARG(max_weight >= 1.0f, 19 + s);
  UCSA_CHECK_ARG(!std::isnan(depth_min), 20 + s);
  UCSA_CHECK_ARG(depth_max >= depth_min, 21 + s);
  TsArgs a;
  a.tsdf = tsdf;
  a.weight = weight;
  a.rgb = rgb;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.H = H;
  a.W = W;
  for (int r = 0; r < 3; ++r) {
    a.o[r] = origin3[r];
    a.h[r] = spacing3[r];
  }
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.trunc = trunc;
  a.max_weight = max_weight;
  a.dmin = depth_min;
  a.dmax = depth_max;
  // nz, ny <= 2^31-1 / 4: the grid's y and z stay below 65536 only if the dims
  // do; larger ones are refused rather than wrapped
  const uint32_t gy = ucsa_div_up(ny, TS_BJ);
  UCSA_CHECK_ARG(gy <= 65535u, 4);
  UCSA_CHECK_ARG(nx <= 65535u, 3);
  const dim3 grid(ucsa_div_up(nz, TS_BK), gy, nx), block(TS_BK, TS_BJ);
  hipStream_t st = (hipStream_t)stream;
  UCSA_CLEAR_ERR();
  for (uint32_t b0 = 0; b0 < B; b0 += TS_MAXB) {
    a.B = B - b0 < TS_MAXB ? B - b0 : TS_MAXB;
    a.depth = depth + (size_t)b0 * H * W;
    a.pixel_weight = weighted ? pixel_weight + (size_t)b0 * H * W : nullptr;
    a.color = color ? color + (size_t)b0 * H * W * 3 : nullptr;
    a.poses = poses + 16 * (size_t)b0;
    if (weighted) {
      if (color)
        hipLaunchKernelGGL((k_tsdf_integrate<true, true>), grid, block, 0, st, a);
      else
        hipLaunchKernelGGL((k_tsdf_integrate<false, true>), grid, block, 0, st, a);
    } else {
      if (color)
        hipLaunchKernelGGL((k_tsdf_integrate<true, false>), grid, block, 0, st, a);
      else
        hipLaunchKernelGGL((k_tsdf_integrate<false, false>), grid, block, 0, st, a);
    }
  }
  return ucsa_launch_status();
}

}  // namespace

extern "C" int32_t ucsa_tsdf_integrate(float* tsdf, float* weight, float* rgb, uint32_t nx,
                                       uint32_t ny, uint32_t nz, const float* origin3,
                                       const float* spacing3, const float* depth,
                                       const uint8_t* color, const float* poses, uint32_t B,
                                       float fx, float fy, float cx, float cy, uint32_t H,
                                       uint32_t W, float trunc, float max_weight,
                                       float depth_min, float depth_max, void* stream) {
  return ts_integrate(tsdf, weight, rgb, nx, ny, nz, origin3, spacing3, depth, nullptr, color,
                      poses, B, fx, fy, cx, cy, H, W, trunc, max_weight, depth_min, depth_max,
                      stream, false);
}

extern "C" int32_t ucsa_tsdf_integrate_weighted(
    float* tsdf, float* weight, float* rgb, uint32_t nx, uint32_t ny, uint32_t nz,
    const float* origin3, const float* spacing3, const float* depth, const float* pixel_weight,
    const uint8_t* color, const float* poses, uint32_t B, float fx, float fy, float cx, float cy,
    uint32_t H, uint32_t W, float trunc, float max_weight, float depth_min, float depth_max,
    void* stream) {
  return ts_integrate(tsdf, weight, rgb, nx, ny, nz, origin3, spacing3, depth, pixel_weight,
                      color, poses, B, fx, fy, cx, cy, H, W, trunc, max_weight, depth_min,
                      depth_max, stream, true);
}
