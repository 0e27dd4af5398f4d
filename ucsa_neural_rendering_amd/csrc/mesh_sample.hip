// Area-uniform, low-discrepancy sample points on a triangle mesh (not in the
// reference): ucsa_face_sample_counts and ucsa_mesh_surface_samples.  The
// contract is stated in include/ucsa_hip.h; tests/sample_numpy.py restates it in
// plain loops and the outputs match it byte for byte.
//
// k_face_sample_counts  a lane per face: the area from the cross product of two
//                       edges, and how many samples the face gets: area *
//                       density rounded down after adding a hashed offset in
//                       [0, 1), so that the expectation over seeds is exact.
// k_surface_samples     a lane per sample: the face by an upper-bound binary
//                       search in the offsets (at most 32 steps), the index j
//                       inside the face, the j-th point of the R2 sequence in
//                       32-bit integers with a hashed per-face offset, folded
//                       into the triangle in integers; then the point and the
//                       attributes blended from the three corners.
//
// A sample is a function of (seed, face, j) and the face's corners alone.
// Every index is clamped or tested before it is used, the search is bounded, a
// lane writes its own row only; no atomics, no LDS, no waiting on another
// thread.
#include "cell_grid.h"

namespace {

constexpr uint32_t MS_ONE = 1u << 24;                  // the weights are k / 2^24
constexpr float MS_INV = 5.9604644775390625e-08f;      // 2^-24
constexpr uint32_t MS_R2_A = 0xC13FA9A9u, MS_R2_B = 0x91E10DA5u;

__host__ __device__ __forceinline__ uint32_t ms_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint32_t ms_face_hash(uint32_t seed, uint32_t f) {
  return ms_mix(seed ^ ms_mix(f + 0x9e3779b9u));
}

__global__ void __launch_bounds__(PG_THREADS)
k_face_sample_counts(const float* __restrict__ verts, uint32_t nv,
                     const int32_t* __restrict__ faces, uint32_t nf, float density, uint32_t seed,
                     float* __restrict__ area, int32_t* __restrict__ count) {
  const uint32_t f = blockIdx.x * PG_THREADS + threadIdx.x;
  if (f >= nf) return;
  const uint32_t i0 = (uint32_t)faces[3ull * f], i1 = (uint32_t)faces[3ull * f + 1u],
                 i2 = (uint32_t)faces[3ull * f + 2u];
  float ar = 0.0f;
  int32_t n = 0;
  if (i0 < nv && i1 < nv && i2 < nv) {  // a negative index is a large unsigned one
    const float ax = verts[3ull * i0], ay = verts[3ull * i0 + 1u], az = verts[3ull * i0 + 2u];
    const float bx = verts[3ull * i1], by = verts[3ull * i1 + 1u], bz = verts[3ull * i1 + 2u];
    const float cx = verts[3ull * i2], cy = verts[3ull * i2 + 1u], cz = verts[3ull * i2 + 2u];
    const float e1x = bx - ax, e1y = by - ay, e1z = bz - az;
    const float e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    const float nx = e1y * e2z - e1z * e2y;
    const float ny = e1z * e2x - e1x * e2z;
    const float nz = e1x * e2y - e1y * e2x;
    const float a = 0.5f * sqrtf((nx * nx + ny * ny) + nz * nz);
    if (pg_finite3(ax, ay, az) && pg_finite3(bx, by, bz) && pg_finite3(cx, cy, cz) && isfinite(a)) {
      ar = a;
      const uint32_t hc = ms_mix(ms_face_hash(seed, f) ^ 0x3c6ef372u);
      const float t = floorf(a * density + (float)(hc >> 8) * MS_INV);
      n = t < 16777216.0f ? (int32_t)t : (int32_t)MS_ONE;  // t >= 0; +inf is clamped
    }
  }
  area[f] = ar;
  count[f] = n;
}

// the smallest k in [lo, hi) with first[k + 1] > s, or hi: k + 1 <= hi <= nf is
// inside first[nf + 1] whatever the entries hold, and 32 halvings empty any range
__device__ __forceinline__ uint32_t ms_search(const int32_t* __restrict__ first, uint32_t lo,
                                              uint32_t hi, uint32_t s) {
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const uint32_t mid = (lo + hi) >> 1;
    if (first[mid + 1u] > (int32_t)s)
      hi = mid;
    else
      lo = mid + 1u;
  }
  return lo;
}

__global__ void __launch_bounds__(PG_THREADS)
k_surface_samples(const float* __restrict__ verts, uint32_t nv, const int32_t* __restrict__ faces,
                  uint32_t nf, const int32_t* __restrict__ first, uint32_t n_samples, uint32_t seed,
                  const float* __restrict__ normals, const uint8_t* __restrict__ rgb,
                  const uint8_t* __restrict__ labels, float* __restrict__ points,
                  int32_t* __restrict__ face, float* __restrict__ bary,
                  float* __restrict__ out_normals, uint8_t* __restrict__ out_rgb,
                  uint8_t* __restrict__ out_labels) {
  const uint32_t s = blockIdx.x * PG_THREADS + threadIdx.x;
  if (s >= n_samples) return;
  // plain per-lane search: searching for the wave's first and last sample first
  // and then between them gave the same bytes 1.04 to 1.36 times slower (README)
  const uint32_t lo = ms_search(first, 0u, nf, s);
  const uint32_t f = lo < nf ? lo : nf - 1u;  // nf >= 1 (checked on the host)
  const uint32_t j = s - (uint32_t)first[f];
  const uint32_t h0 = ms_face_hash(seed, f);
  const uint32_t h1 = ms_mix(h0 ^ 0x68bc21ebu), h2 = ms_mix(h0 ^ 0x02e5be93u);
  uint32_t a = (j * MS_R2_A + h1) >> 8, b = (j * MS_R2_B + h2) >> 8;
  if (a + b > MS_ONE) {
    a = MS_ONE - a;
    b = MS_ONE - b;
  }
  const uint32_t c = MS_ONE - a - b;
  const float w0 = (float)c * MS_INV, w1 = (float)a * MS_INV, w2 = (float)b * MS_INV;
  face[s] = (int32_t)f;
  bary[3ull * s] = w0;
  bary[3ull * s + 1u] = w1;
  bary[3ull * s + 2u] = w2;
  const uint32_t i0 = (uint32_t)faces[3ull * f], i1 = (uint32_t)faces[3ull * f + 1u],
                 i2 = (uint32_t)faces[3ull * f + 2u];
  const bool ok = i0 < nv && i1 < nv && i2 < nv;
  float p[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f};
  uint32_t col[3] = {0u, 0u, 0u}, lab = 0u;
  if (ok) {  // only a malformed `first` leads to a face that is not
    for (int k = 0; k < 3; ++k) {
      const float A = verts[3ull * i0 + k];
      const float e1 = verts[3ull * i1 + k] - A, e2 = verts[3ull * i2 + k] - A;
      p[k] = A + (w1 * e1 + w2 * e2);
    }
    if (normals) {
      for (int k = 0; k < 3; ++k)
        n[k] = (w0 * normals[3ull * i0 + k] + w1 * normals[3ull * i1 + k]) +
               w2 * normals[3ull * i2 + k];
      const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
      for (int k = 0; k < 3; ++k) n[k] = len > 0.0f ? n[k] / len : 0.0f;
    }
    if (rgb)
      for (int k = 0; k < 3; ++k) {
        const float v = floorf(((w0 * (float)rgb[3ull * i0 + k] + w1 * (float)rgb[3ull * i1 + k]) +
                                w2 * (float)rgb[3ull * i2 + k]) + 0.5f);
        col[k] = (uint32_t)v;  // 0 <= v <= 255: the weights sum to 1
      }
    if (labels)  // the largest weight, the first corner on a tie
      lab = (c >= a && c >= b) ? labels[i0] : (a >= b ? labels[i1] : labels[i2]);
  }
  for (int k = 0; k < 3; ++k) points[3ull * s + k] = p[k];
  if (normals)
    for (int k = 0; k < 3; ++k) out_normals[3ull * s + k] = n[k];
  if (rgb)
    for (int k = 0; k < 3; ++k) out_rgb[3ull * s + k] = (uint8_t)col[k];
  if (labels) out_labels[s] = (uint8_t)lab;
}

}  // namespace

extern "C" int32_t ucsa_face_sample_counts(const float* verts, uint32_t nv, const int32_t* faces,
                                           uint32_t nf, float density, uint32_t seed, float* area,
                                           int32_t* count, void* stream) {
  UCSA_CHECK_ARG(nv <= 0x7FFFFFFFu, 1);
  UCSA_CHECK_ARG(nf <= 0x7FFFFFFFu, 3);
  UCSA_CHECK_ARG(density > 0.0f && pg_host_finite(density), 4);
  if (nf == 0) return 0;
  UCSA_CHECK_ARG(nv == 0 || verts, 0);
  UCSA_CHECK_ARG(faces, 2);
  UCSA_CHECK_ARG(area, 6);
  UCSA_CHECK_ARG(count, 7);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_face_sample_counts, dim3(ucsa_div_up(nf, PG_THREADS)), dim3(PG_THREADS), 0,
                     (hipStream_t)stream, verts, nv, faces, nf, density, seed, area, count);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_mesh_surface_samples(const float* verts, uint32_t nv, const int32_t* faces,
                                             uint32_t nf, const int32_t* first, uint32_t n_samples,
                                             uint32_t seed, const float* normals,
                                             const uint8_t* rgb, const uint8_t* labels,
                                             float* points, int32_t* face, float* bary,
                                             float* out_normals, uint8_t* out_rgb,
                                             uint8_t* out_labels, void* stream) {
  UCSA_CHECK_ARG(nv <= 0x7FFFFFFFu, 1);
  UCSA_CHECK_ARG(nf <= 0x7FFFFFFFu, 3);
  UCSA_CHECK_ARG(n_samples <= 0x7FFFFFFFu, 5);
  if (n_samples == 0) return 0;
  UCSA_CHECK_ARG(nf > 0, 3);  // a sample lies on a face
  UCSA_CHECK_ARG(nv == 0 || verts, 0);
  UCSA_CHECK_ARG(faces, 2);
  UCSA_CHECK_ARG(first, 4);
  UCSA_CHECK_ARG(points, 10);
  UCSA_CHECK_ARG(face, 11);
  UCSA_CHECK_ARG(bary, 12);
  UCSA_CHECK_ARG(!normals || out_normals, 13);
  UCSA_CHECK_ARG(!rgb || out_rgb, 14);
  UCSA_CHECK_ARG(!labels || out_labels, 15);
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_surface_samples, dim3(ucsa_div_up(n_samples, PG_THREADS)),
                     dim3(PG_THREADS), 0, (hipStream_t)stream, verts, nv, faces, nf, first,
                     n_samples, seed, normals, rgb, labels, points, face, bary, out_normals,
                     out_rgb, out_labels);
  return ucsa_launch_status();
}
