/*
 * ucsa_hip.h -- C ABI of libucsa_hip.so, the MI355X (gfx950) implementation of
 * the Semantic-NeRF volume-rendering hot path of ethz-asl/ucsa_neural_rendering.
 *
 * This is the drop-in boundary.  The reference's only native
 * FFI on this path is the pybind11 module `_raymarching`
 * (reference nr4seg/nerf/raymarching/src/bindings.cpp:5-17, signatures
 * raymarching.h:7-18) plus the tiny-cuda-nn Python objects constructed in
 * nr4seg/nerf/network_tcnn_semantics.py:36-100.  Every entry point below names
 * the reference interface it replaces.
 *
 * Conventions (all entry points):
 *   - plain C, no torch / C++ types; pointers are DEVICE pointers unless a
 *     parameter is documented as host;
 *   - the caller owns every buffer; nothing is allocated, nothing syncs;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*);
 *   - return 0 on success, a negative hipError_t on a launch error, or
 *     UCSA_ERR_ARG (-1000 - k) when argument k (0-based) is invalid;
 *   - buffers are contiguous, fp32 unless stated, 16-byte aligned;
 *   - re-entrant.  Process-wide state is limited to: (a) the table of tuning
 *     switches read from the environment ONCE, at the first call that consults
 *     it (INTEGRATION.md "Environment variables": launch shapes and kernel
 *     choices, never results); (b) per caller-stream sets of internal streams /
 *     events created on first use by the calls documented as pipelined
 *     (ucsa_render_view, the merged grid backward); (c) the device's LDS per
 *     workgroup, asked of the runtime at the first ucsa_resample.
 */
#ifndef UCSA_HIP_H_
#define UCSA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UCSA_VERSION 100 /* major*10000 + minor*100 + patch */
#define UCSA_ERR_ARG (-1000)
#define UCSA_MAX_LEVELS 16

int32_t ucsa_version(void);
/* Human-readable text for a return code (static storage). */
const char* ucsa_error_string(int32_t code);
/* Re-read the tuning switches from the environment (lab tools and tests that
 * flip one inside a process; not for production code, not thread-safe against
 * concurrent calls into the library). */
void ucsa_env_reload(void);

/* ---- hash-grid level table -------------------------------------------------
 * Host-side description of tcnn.Encoding("HashGrid") as configured at
 * reference network_tcnn_semantics.py:34-46.  Filled on the HOST. */
typedef struct ucsa_grid_level {
  float scale;      /* 2^(l*log2 s)*base - 1, float64-evaluated then cast */
  uint32_t res;     /* ceil(scale)+1 */
  uint32_t entries; /* min(roundup8(res^3), 2^log2_hashmap_size) */
  uint32_t offset;  /* first entry of this level in the flat table */
  uint32_t hashed;  /* 1: spatial hash, 0: dense x + y*res + z*res^2 */
} ucsa_grid_level;

typedef struct ucsa_grid {
  uint32_t n_levels;   /* <= UCSA_MAX_LEVELS */
  uint32_t n_features; /* must be 2 */
  uint32_t total_entries;
  float bound; /* positions are mapped (x+bound)/(2*bound) */
  ucsa_grid_level level[UCSA_MAX_LEVELS];
} ucsa_grid;

/* HOST function.  Replaces the tcnn HashGrid constructor
 * (reference network_tcnn_semantics.py:36-46). */
int32_t ucsa_grid_init(ucsa_grid* grid, float bound, uint32_t n_levels,
                       uint32_t log2_hashmap_size, uint32_t base_resolution,
                       double per_level_scale);

/* ---- rays ------------------------------------------------------------------
 * Full-image pinhole rays, row-major pixels, pixel centres at +0.5.
 * Replaces get_rays (reference nr4seg/dataset/ngp_utils.py:28-69) and, with
 * `inds` != NULL, get_rays_train (reference
 * nr4seg/lightning/joint_train_lightning_net.py:108-157).
 *   poses [B,4,4]; intrinsics are HOST scalars (fx,fy,cx,cy);
 *   inds [n] int64 or NULL (then n must be H*W and pixel i is ray i);
 *   out: rays_o, rays_d [B,n,3], norms [B,n]. */
int32_t ucsa_get_rays(const float* poses, uint32_t B, float fx, float fy,
                      float cx, float cy, uint32_t H, uint32_t W,
                      const int64_t* inds, uint32_t n, float* rays_o,
                      float* rays_d, float* norms, void* stream);

/* The pixel indices drawn by get_rays_train (reference
 * joint_train_lightning_net.py:141; int64 [n], duplicates allowed, values in
 * [0, H*W)), reordered tile by tile (tile x tile pixels, row-major inside a
 * tile): the same multiset, neighbours adjacent, which makes the hash-grid
 * backward of the batch about twice as fast.  n <= 8192 (one
 * workgroup sorts in LDS); out may not alias inds. */
int32_t ucsa_tile_order(const int64_t* inds, uint32_t n, uint32_t H, uint32_t W,
                        uint32_t tile, int64_t* out, void* stream);

/* Replaces _backend.near_far_from_aabb (reference
 * nr4seg/nerf/raymarching/src/raymarching.cu:62-126, bindings.cpp:6).
 * aabb is 6 HOST floats (xmin,ymin,zmin,xmax,ymax,zmax). */
int32_t ucsa_near_far_from_aabb(const float* rays_o, const float* rays_d,
                                const float* aabb_host, uint32_t N,
                                float min_near, float* nears, float* fars,
                                void* stream);

/* Coarse sample depths, reference renderer_semantics.py:154-168.
 * t_rand [N,T] or NULL (perturb=False).  out z [N,T]. */
int32_t ucsa_sample_coarse(const float* nears, const float* fars,
                           const float* t_rand, uint32_t N, uint32_t T,
                           float* z, void* stream);

/* ---- field: hash grid + sigma MLP -----------------------------------------
 * Encodes the positions clamp(o + d*z, aabb) of all N*T samples.
 * Replaces tcnn.Encoding.forward as called from density()
 * (reference network_tcnn_semantics.py:133-134) together with the position
 * generation/clip of renderer_semantics.py:171-173.
 *   table [total_entries,2] fp32; out feat [n_levels][N*T][2] (level-major).
 */
int32_t ucsa_hashgrid_encode_rays(const ucsa_grid* grid_host,
                                  const float* table, const float* rays_o,
                                  const float* rays_d, const float* z,
                                  const float* aabb_host, uint32_t N,
                                  uint32_t T, float* feat, void* stream);

/* Same for IMAGE-ORDERED rays: ray r is pixel (r / image_width,
 * r % image_width) of full rows of an image (any number of rows).  The fine
 * levels are gathered one 8x8 pixel tile per wave so that neighbouring pixels
 * share cache lines; the features are bit-identical to
 * ucsa_hashgrid_encode_rays'. */
int32_t ucsa_hashgrid_encode_rays_image(
    const ucsa_grid* grid_host, const float* table, const float* rays_o,
    const float* rays_d, const float* z, const float* aabb_host, uint32_t N,
    uint32_t T, uint32_t image_width, float* feat, void* stream);

/* Same encoder for explicit positions x [M,3] in [-bound,bound] (the
 * reference's network.density(x) entry, network_tcnn_semantics.py:130-135). */
int32_t ucsa_hashgrid_encode_points(const ucsa_grid* grid_host,
                                    const float* table, const float* x,
                                    uint32_t M, float* feat, void* stream);

/* MLP kinds: which of the three tcnn.Network objects
 * (reference network_tcnn_semantics.py:48-58, 74-84, 90-100). */
#define UCSA_MLP_SIGMA 0 /* 32 -> 64 -> 16        (3072 params) */
#define UCSA_MLP_COLOR 1 /* 32 -> 64 -> 64 -> 16  (7168 params) */
#define UCSA_MLP_SEM 2   /* 16 -> 64 -> 48        (4096 params) */

/* Re-lays a tcnn-format flat weight vector (row-major [out,in] matrices back
 * to back, padded shapes) into MFMA A-fragment order.  Must be called after
 * every parameter update, before the kernels below.
 *   packed: same element count as params. */
int32_t ucsa_mlp_pack(int32_t kind, const float* params, float* packed,
                      uint32_t n_classes, void* stream);

/* sigma MLP over level-major features: h [M,16] raw outputs
 * (h[:,0] = log-density, h[:,1:16] = geo_feat), sigma [M] = exp(h[:,0]).
 * Replaces sigma_net + trunc_exp in density()
 * (reference network_tcnn_semantics.py:135-139, activation.py:13). */
int32_t ucsa_sigma_mlp_fwd(const float* feat, const float* packed_sigma,
                           uint32_t M, uint32_t n_levels, float* h,
                           float* sigma, void* stream);


/* ---- hierarchical resampling ----------------------------------------------
 * Coarse weights -> pdf over interior bins -> inverse CDF at u.
 * Replaces renderer_semantics.py:182-207 and sample_pdf :10-46.
 *   z [N,T], sigma [N,T], u [N,t] in [0,1); out new_z [N,t], ASCENDING per
 *   ray (the uniforms are sorted first; the reference only ever consumes
 *   new_z through its sort/merge, :221-222, so the order is unobservable).
 *   Sizes: 3 <= T <= 4096, t <= 4096, AND the ray's arrays fit the LDS of one
 *   workgroup: 16 (3 T + tpad) bytes, tpad = the next power of two >= t (>= 2),
 *   at most hipDeviceAttributeMaxSharedMemoryPerBlock (163,840 B on gfx950, asked
 *   of the runtime once per process): T = t = 2048 fits, T = 2048 with t = 4096
 *   fills it exactly, T >= 3414 never fits.  A larger request returns UCSA_ERR_ARG - 4 (the T arrays
 *   alone are too large) or UCSA_ERR_ARG - 5 before anything is launched. */
int32_t ucsa_resample(const float* z, const float* sigma, const float* u,
                      uint32_t N, uint32_t T, uint32_t t,
                      float density_scale, float* new_z, void* stream);

/* ---- merge + weights + masked colour/semantics + compositing ---------------
 * Replaces renderer_semantics.py:220-299 and the masked color()/semantics()
 * of network_tcnn_semantics.py:147-207.
 *   z_c/sigma_c/h_c: coarse [N,T], [N,T], [N*T,16]
 *   z_f/sigma_f/h_f: fine   [N,t], [N,t], [N*t,16]   (t may be 0)
 *   out: image [N,3], depth [N], semantics [N,n_classes].
 * Optional training outputs (NULL to skip): merged order `src` [N,S] int32
 * (index into the concatenated [coarse|fine] sample list of the ray),
 * `weights` [N,S] (unmasked weights), S = T+t. */
int32_t ucsa_composite_fwd(const float* rays_d, const float* norms,
                           const float* z_c, const float* sigma_c,
                           const float* h_c, const float* z_f,
                           const float* sigma_f, const float* h_f,
                           const float* packed_color, const float* packed_sem,
                           uint32_t N, uint32_t T, uint32_t t,
                           uint32_t n_classes, float density_scale,
                           float* image, float* depth, float* semantics,
                           int32_t* src, float* weights, void* stream);

/* Scratch bytes the caller must provide for ucsa_render_fwd. */
uint64_t ucsa_render_workspace_bytes(uint32_t N, uint32_t T, uint32_t t,
                                     uint32_t n_levels);

/* Whole forward pass for N rays (the reference's SemanticNeRFRenderer.run,
 * renderer_semantics.py:123-299): near/far, coarse sampling, density,
 * resampling, density, merge, masked colour/semantics, compositing.
 *   t_rand [N,T] or NULL; u [N,t]; ws: workspace of
 *   ucsa_render_workspace_bytes(); packed_*: see ucsa_mlp_pack.
 *   image_width: 0, or the width of the image whose full rows the rays are
 *   (ray r = pixel (r / image_width, r % image_width)): selects the
 *   tile-ordered gather of ucsa_hashgrid_encode_rays_image, same results. */
int32_t ucsa_render_fwd(const ucsa_grid* grid_host, const float* table,
                        const float* packed_sigma, const float* packed_color,
                        const float* packed_sem, const float* rays_o,
                        const float* rays_d, const float* norms,
                        const float* aabb_host, float min_near,
                        const float* t_rand, const float* u, uint32_t N,
                        uint32_t T, uint32_t t, uint32_t n_classes,
                        float density_scale, uint32_t image_width, float* image,
                        float* depth, float* semantics, void* ws, void* stream);

/* The same computation for INFERENCE as two dense kernels (no `src` /
 * `weights` outputs): k_weights_compact (one wave per ray: merge, weights,
 * mask, depth, survivors compacted into a global list) and k_shade_dense /
 * k_shade16 (colour + semantics nets over the survivor list with a
 * software-pipelined operand fetch, per-ray sums in sample order).  Bit-identical outputs to
 * ucsa_composite_fwd; what ucsa_render_fwd uses.  `workspace`:
 * ucsa_composite_infer_workspace_bytes(N, T, t) bytes, caller-owned. */
uint64_t ucsa_composite_infer_workspace_bytes(uint32_t N, uint32_t T, uint32_t t);
int32_t ucsa_composite_infer(const float* rays_d, const float* norms,
                             const float* z_c, const float* sigma_c,
                             const float* h_c, const float* z_f,
                             const float* sigma_f, const float* h_f,
                             const float* packed_color, const float* packed_sem,
                             uint32_t N, uint32_t T, uint32_t t,
                             uint32_t n_classes, float density_scale,
                             float* image, float* depth, float* semantics,
                             void* workspace, void* stream);
/* fp16-MFMA form (weights from ucsa_mlp_pack_f16) */
int32_t ucsa_composite_infer_f16(const float* rays_d, const float* norms,
                                 const float* z_c, const float* sigma_c,
                                 const float* h_c, const float* z_f,
                                 const float* sigma_f, const float* h_f,
                                 const void* packed_color_half,
                                 const void* packed_sem_half, uint32_t N,
                                 uint32_t T, uint32_t t, uint32_t n_classes,
                                 float density_scale, float* image,
                                 float* depth, float* semantics,
                                 void* workspace, void* stream);

/* Pointwise colour / semantics queries: network.color() / network.semantics()
 * (reference network_tcnn_semantics.py:147-207).  dirs [M,3], geo_feat [M,15],
 * mask [M] uint8 or NULL; rgb [M,3] and/or probs [M,n_classes] (either may be
 * NULL); rows with mask == 0 are zero. */
int32_t ucsa_point_shade(const float* dirs, const float* geo_feat,
                         const uint8_t* mask, const float* packed_color,
                         const float* packed_sem, uint32_t M,
                         uint32_t n_classes, float* rgb, float* probs,
                         void* stream);

/* Same, reading the geometry features from the raw sigma-MLP rows h [M,16]
 * (ucsa_sigma_mlp_fwd; slot 0, the log-density, is skipped) so that
 * network.forward(x, d) (reference network_tcnn_semantics.py:102-128) needs
 * no repacking between density() and color()/semantics(). */
int32_t ucsa_point_shade_h(const float* dirs, const float* h,
                           const uint8_t* mask, const float* packed_color,
                           const float* packed_sem, uint32_t M,
                           uint32_t n_classes, float* rgb, float* probs,
                           void* stream);

/* ============================ fp16 hash table ============================== */
/* tiny-cuda-nn stores the hash grid in fp16 (fp32 master copy in the optimizer)
 * and its encoding emits fp16 features.  Optional here: `table_half` = the
 * fp32 table rounded to half (ucsa_cast_f32_to_f16; half2 entries, same level
 * offsets); `feat_half` [L][N*T] half2.  Values are widened on load and
 * interpolated in fp32, so the features equal the fp32 kernels' on the
 * rounded table, rounded to half once (where ucsa_sigma_mlp_fwd_f16 would
 * round them anyway); 4-byte entries let one 16-byte access serve four
 * x-neighbours (5 instead of 6 accesses per sample and hashed level).
 * image_width = 0: ray-ordered samples, else as
 * ucsa_hashgrid_encode_rays_image.  Call site: reference
 * network_tcnn_semantics.py:36-46,133-134. */
int32_t ucsa_cast_f32_to_f16(const float* src, void* dst_half, uint64_t n,
                             void* stream);
int32_t ucsa_hashgrid_encode_rays_h16(const ucsa_grid* grid,
                                      const void* table_half,
                                      const float* rays_o, const float* rays_d,
                                      const float* z, const float* aabb_host,
                                      uint32_t N, uint32_t T,
                                      uint32_t image_width, void* feat_half,
                                      void* stream);
/* fp32 table, fp16 features (for ucsa_sigma_mlp_fwd_f16_h: same h / sigma as
 * ucsa_hashgrid_encode_rays[_image] + ucsa_sigma_mlp_fwd_f16, half the
 * feature traffic) */
int32_t ucsa_hashgrid_encode_rays_hf(const ucsa_grid* grid, const float* table,
                                     const float* rays_o, const float* rays_d,
                                     const float* z, const float* aabb_host,
                                     uint32_t N, uint32_t T,
                                     uint32_t image_width, void* feat_half,
                                     void* stream);
/* ---- depth-ordered encoding of the FINE samples of image-ordered rays ----
 * Replaces, for rays that are the pixels of whole image rows, the
 * `self.encoder(x)` + `self.sigma_net(x)` of the second `density()` call of
 * run() (nr4seg/nerf/renderer_semantics.py:214-226 ->
 * network_tcnn_semantics.py:130-144).  The fine samples of neighbouring rays sit
 * at unrelated depths (importance sampling with independent uniforms), so a wave
 * that holds one sample index of an 8x8 pixel tile shares no cells; dealt to the
 * lanes in DEPTH order the same samples share their cache lines as in the coarse
 * pass.  Three calls, bit-identical h / sigma to ucsa_hashgrid_encode_rays_image
 * + ucsa_sigma_mlp_fwd*:
 *   ucsa_tile_depth_order: counting sort of every tile's 64 x T samples by
 *     depth -> z_sorted [N*T] (depths), pix [N*T] (pixel inside the 8x8 tile),
 *     slot [N*T] (ray-major index r * T + s), tiles back to back.  N must be a
 *     multiple of image_width (whole rows), T <= 1024.
 *   ucsa_hashgrid_encode_sorted[_hf]: features [L][N*T] (float2 / half2) in that
 *     order.
 *   ucsa_sigma_mlp_fwd_scatter: the sigma MLP on such an array, h [N*T,16] and
 *     sigma [N*T] written at the ray-major slots.  mode 0 = f32-input MFMA
 *     (ucsa_mlp_pack), 1 = f16 nets on fp16 features (ucsa_mlp_pack_f16),
 *     2 = bf16x3 (ucsa_mlp_pack_x3), 3 = f16x2 (ucsa_mlp_pack_h2). */
int32_t ucsa_tile_depth_order(const float* z, uint32_t N, uint32_t T,
                              uint32_t image_width, float* z_sorted,
                              uint8_t* pix, uint32_t* slot, void* stream);
/* The same three arrays for COARSE samples without a sort: "sample index, then
 * pixel" (sample s of every ray of an 8x8 tile sits at nearly one depth:
 * renderer_semantics.py:154-173).  The render path uses it for coarse passes of
 * more than 128 samples per ray, where the depth sort costs more than it brings. */
int32_t ucsa_tile_index_order(const float* z, uint32_t N, uint32_t T,
                              uint32_t image_width, float* z_sorted, uint8_t* pix,
                              uint32_t* slot, void* stream);
int32_t ucsa_hashgrid_encode_sorted(const ucsa_grid* grid, const float* table,
                                    const float* rays_o, const float* rays_d,
                                    const float* z_sorted, const uint8_t* pix,
                                    const float* aabb_host, uint32_t N,
                                    uint32_t T, uint32_t image_width,
                                    float* feat, void* stream);
int32_t ucsa_hashgrid_encode_sorted_hf(const ucsa_grid* grid, const float* table,
                                       const float* rays_o, const float* rays_d,
                                       const float* z_sorted, const uint8_t* pix,
                                       const float* aabb_host, uint32_t N,
                                       uint32_t T, uint32_t image_width,
                                       void* feat_half, void* stream);
int32_t ucsa_sigma_mlp_fwd_scatter(int32_t mode, const void* feat,
                                   const void* packed_sigma, uint32_t M,
                                   uint32_t n_levels, const uint32_t* slot,
                                   float* h, float* sigma, void* stream);
/* ucsa_hashgrid_encode_sorted + ucsa_sigma_mlp_fwd_scatter as ONE call in which the
 * sigma MLP encodes levels 0-11 itself (0-7 with UCSA_DENSITY_LEVELS=8) -- a wave owns
 * 64 consecutive samples of the depth order, the level is wave-uniform, the feature pairs
 * go through a wave-private LDS tile and never through HBM -- and reads the remaining
 * levels (12-15: the ones bound by L2 -> L1 line fills) from feat_ws [16][N*T][2]
 * (written here by the per-level depth-ordered encoder): `density()` of a sample
 * batch, reference network_tcnn_semantics.py:130-144, with three quarters of the
 * feature round trip gone.  mode 2 = bf16x3, 3 = f16x2 packs; 16 levels.  The same h / sigma
 * BITS as the two separate calls. */
int32_t ucsa_density_sorted(int32_t mode, const ucsa_grid* grid, const float* table,
                            const float* rays_o, const float* rays_d,
                            const float* z_sorted, const uint8_t* pix,
                            const uint32_t* slot, const float* aabb_host, uint32_t N,
                            uint32_t T, uint32_t image_width, const void* packed_sigma,
                            float* feat_ws, float* h, float* sigma, void* stream);
/* ucsa_sigma_mlp_fwd_f16 on fp16 features (same h / sigma) */
int32_t ucsa_sigma_mlp_fwd_f16_h(const void* feat_half,
                                 const void* packed_sigma_half, uint32_t M,
                                 uint32_t n_levels, float* h, float* sigma,
                                 void* stream);
/* ucsa_render_fwd_f16 reading the fp16 table */
int32_t ucsa_render_fwd_f16_h16(const ucsa_grid* grid, const void* table_half,
                                const void* packed_sigma_half,
                                const void* packed_color_half,
                                const void* packed_sem_half,
                                const float* rays_o, const float* rays_d,
                                const float* norms, const float* aabb_host,
                                float min_near, const float* t_rand,
                                const float* u, uint32_t N, uint32_t T,
                                uint32_t t, uint32_t n_classes,
                                float density_scale, uint32_t image_width,
                                float* image, float* depth, float* semantics,
                                void* workspace, void* stream);

/* ================= bf16x3: fp32-grade nets on the bf16 MFMA pipe ============ */
/* Every fp32 weight and layer input is split exactly into three bf16 terms and
 * each product is accumulated in fp32 from six bf16 partial products
 * (csrc/mfma_mlp_x3.h): ordinary fp32 round-off, NOT bit-identical to the
 * f32-input MFMA of the entry points above, 144 16-cycle MFMAs per 16 samples
 * instead of 176 32-cycle ones.  Same call sites as the fp32 forms
 * (reference network_tcnn_semantics.py:147-207, renderer_semantics.py:238-299).
 * packed_*_x3: ucsa_mlp_pack_x3_bytes(kind, n_classes) bytes from
 * ucsa_mlp_pack_x3. */
uint32_t ucsa_mlp_pack_x3_bytes(int32_t kind, uint32_t n_classes);
int32_t ucsa_mlp_pack_x3(int32_t kind, const float* params, void* packed_x3,
                         uint32_t n_classes, void* stream);
/* density() nets of a sample batch (cf. ucsa_sigma_mlp_fwd) */
int32_t ucsa_sigma_mlp_fwd_x3(const float* feat, const void* packed_sigma_x3,
                              uint32_t M, uint32_t n_levels, float* h,
                              float* sigma, void* stream);
/* ---- "f16x2": the nets on the f16 MFMA pipe with TWO-term operands ----------
 * x ~ f16(x) + f16((x - f16(x)) * 2^11) * 2^-11: 22 significant bits per
 * operand, products accumulated in fp32 from three f16 MFMA passes (bf16x3: six)
 * -- the same 2^-23-per-product error class as bf16x3 and the f32-input MFMA
 * chain (csrc/mfma_mlp_h2.h).  RANGE: that of the reference's own fp16 nets --
 * layer inputs and weights below 65504 in magnitude, hidden activations below
 * 2^20 (ucsa_mlp_pack_h2 scales the first layer by 2^-4 and the last by 2^4,
 * exact for the bias-free ReLU nets).  Values beyond it are not detected (the
 * _x3 entries have fp32's range).
 * Same interfaces as the _x3 entries with packs from ucsa_mlp_pack_h2
 * (ucsa_mlp_pack_h2_bytes bytes).  Replaces what the _x3 entries replace
 * (tcnn.Network forward, reference network_tcnn_semantics.py:135,147-207). */
uint32_t ucsa_mlp_pack_h2_bytes(int32_t kind, uint32_t n_classes);
int32_t ucsa_mlp_pack_h2(int32_t kind, const float* params, void* packed_h2,
                         uint32_t n_classes, void* stream);
/* The same, and *range_bits (uint32 in device memory or in pinned host memory
 * the device can address -- hipHostMalloc / torch pin_memory --, caller-zeroed,
 * accumulated over calls: the waves raise a device word, the last workgroup
 * publishes it with ONE system-scope atomic max) = the largest |value| it converted to f16, as an fp32
 * bit pattern: >= 0x477FE000 (65504.0f) means a weight outside f16x2's range or
 * not finite -- values the kernels would turn into zeros silently
 * (mfma_mlp_h2.h).  The range guard of `nerf: {precision: f16x2}`
 * (network_tcnn_semantics.py `h2_guard`) without a launch of its own. */
int32_t ucsa_mlp_pack_h2_checked(int32_t kind, const float* params, void* packed_h2,
                                 uint32_t n_classes, uint32_t* range_bits,
                                 uint32_t* scratch /* 2 device uint32, zeroed once */,
                                 void* stream);
int32_t ucsa_sigma_mlp_fwd_h2(const float* feat, const void* packed_sigma_h2,
                              uint32_t M, uint32_t n_levels, float* h,
                              float* sigma, void* stream);
int32_t ucsa_composite_infer_h2(
    const float* rays_d, const float* norms, const float* z_c,
    const float* sigma_c, const float* h_c, const float* z_f,
    const float* sigma_f, const float* h_f, const void* packed_color_h2,
    const void* packed_sem_h2, uint32_t N, uint32_t T, uint32_t t,
    uint32_t n_classes, float density_scale, float* image, float* depth,
    float* semantics, void* workspace, void* stream);
/* ucsa_composite_train_fwd_x3 with f16x2 nets (same outputs and aux arrays). */
int32_t ucsa_composite_train_fwd_h2(
    const float* rays_d, const float* norms, const float* z_c,
    const float* sigma_c, const float* h_c, const float* z_f,
    const float* sigma_f, const float* h_f, const void* packed_color_h2,
    const void* packed_sem_h2, uint32_t N, uint32_t T, uint32_t t,
    uint32_t n_classes, float density_scale, float* image, float* depth,
    float* semantics, int32_t* src, float* w, void* workspace, void* stream);
int32_t ucsa_render_fwd_h2(
    const ucsa_grid* grid, const float* table, const void* packed_sigma_h2,
    const void* packed_color_h2, const void* packed_sem_h2, const float* rays_o,
    const float* rays_d, const float* norms, const float* aabb_host,
    float min_near, const float* t_rand, const float* u, uint32_t N, uint32_t T,
    uint32_t t, uint32_t n_classes, float density_scale, uint32_t image_width,
    float* image, float* depth, float* semantics, void* ws, void* stream);

/* A whole batch of rays (e.g. one view) in `chunk`-ray pieces, what the
 * reference's staged `render` loop does (renderer_semantics.py:321-342), as ONE
 * call: software-pipelined over two internal streams (density half of chunk
 * k+1 || shading half of chunk k; events fork from / join to `stream`), two
 * workspaces of ucsa_render_workspace_bytes(min(N, chunk), T, t, L) bytes each
 * (ws1 NULL = serial loop).  mode: 0 = ucsa_render_fwd, 1 = _f16, 2 = _x3,
 * 3 = _f16_h16, 4 = _h2 (their table / packed-weight formats).  Arrays are for all N
 * rays; image_width as in ucsa_render_fwd (needs chunk % (8 * image_width) == 0
 * and N % image_width == 0, else the ray-ordered gather is used -- same
 * results).  Bit-identical to calling ucsa_render_fwd* per chunk. */
int32_t ucsa_render_view(uint32_t mode, const ucsa_grid* grid, const void* table,
                         const void* packed_sigma, const void* packed_color,
                         const void* packed_sem, const float* rays_o,
                         const float* rays_d, const float* norms,
                         const float* aabb_host, float min_near,
                         const float* t_rand, const float* u, uint32_t N,
                         uint32_t T, uint32_t t, uint32_t n_classes,
                         float density_scale, uint32_t image_width,
                         uint32_t chunk, float* image, float* depth,
                         float* semantics, void* ws0, void* ws1, void* stream);

/* run() as one enqueue (cf. ucsa_render_fwd; same workspace) */
int32_t ucsa_render_fwd_x3(const ucsa_grid* grid, const float* table,
                           const void* packed_sigma_x3,
                           const void* packed_color_x3,
                           const void* packed_sem_x3, const float* rays_o,
                           const float* rays_d, const float* norms,
                           const float* aabb_host, float min_near,
                           const float* t_rand, const float* u, uint32_t N,
                           uint32_t T, uint32_t t, uint32_t n_classes,
                           float density_scale, uint32_t image_width,
                           float* image, float* depth, float* semantics,
                           void* workspace, void* stream);
int32_t ucsa_composite_infer_x3(const float* rays_d, const float* norms,
                                const float* z_c, const float* sigma_c,
                                const float* h_c, const float* z_f,
                                const float* sigma_f, const float* h_f,
                                const void* packed_color_x3,
                                const void* packed_sem_x3, uint32_t N,
                                uint32_t T, uint32_t t, uint32_t n_classes,
                                float density_scale, float* image,
                                float* depth, float* semantics,
                                void* workspace, void* stream);

/* Training forward of the same stage on the split pair with the bf16x3 nets:
 * outputs of ucsa_composite_fwd plus its aux arrays src [N, T + t] (int32
 * source index of every depth-sorted sample: < T coarse, else T + fine index)
 * and w [N, T + t] (its weight) for ucsa_composite_bwd.  Reference:
 * renderer_semantics.py:220-299 as called from forward_nerf_train
 * (joint_train_lightning_net.py:167-223). */
int32_t ucsa_composite_train_fwd_x3(
    const float* rays_d, const float* norms, const float* z_c,
    const float* sigma_c, const float* h_c, const float* z_f,
    const float* sigma_f, const float* h_f, const void* packed_color_x3,
    const void* packed_sem_x3, uint32_t N, uint32_t T, uint32_t t,
    uint32_t n_classes, float density_scale, float* image, float* depth,
    float* semantics, int32_t* src, float* w, void* workspace, void* stream);

/* ======================= fp16-MFMA inference option ======================== */
/* tiny-cuda-nn evaluates the three MLPs with fp16 weights / layer inputs and
 * fp32 accumulation; the entry points below do the same (16x16x32 f16 MFMA)
 * for inference.  Hash-grid, sampling and compositing stay fp32.  The default
 * (and parity) path is the fp32 one above. */
uint32_t ucsa_mlp_pack_f16_halves(int32_t kind, uint32_t n_classes);
int32_t ucsa_mlp_pack_f16(int32_t kind, const float* params, void* packed_half,
                          uint32_t n_classes, void* stream);
/* Limit: a feature below 2^-14 is an fp16 subnormal (below 2^-25: zero).  The
 * f16 MFMA aligns its products to the largest product EXPONENT and takes a
 * subnormal operand at the exponent 2^-14, so such features carry an ABSOLUTE
 * error of up to 2^-23 * 2^-14 * max|w| per term on the layer they enter, not a
 * relative one (measured: docs/DESIGN_NOTEBOOK.md, section DN).  Features beyond
 * 65504 become inf.  The _x3 and _h2 forms have neither limit within 2^20. */
int32_t ucsa_sigma_mlp_fwd_f16(const float* feat, const void* packed_sigma_half,
                               uint32_t M, uint32_t n_levels, float* h,
                               float* sigma, void* stream);
int32_t ucsa_composite_fwd_f16(const float* rays_d, const float* norms,
                               const float* z_c, const float* sigma_c,
                               const float* h_c, const float* z_f,
                               const float* sigma_f, const float* h_f,
                               const void* packed_color_half,
                               const void* packed_sem_half, uint32_t N,
                               uint32_t T, uint32_t t, uint32_t n_classes,
                               float density_scale, float* image, float* depth,
                               float* semantics, int32_t* src, float* weights,
                               void* stream);
int32_t ucsa_render_fwd_f16(const ucsa_grid* grid_host, const float* table,
                            const void* packed_sigma_half,
                            const void* packed_color_half,
                            const void* packed_sem_half, const float* rays_o,
                            const float* rays_d, const float* norms,
                            const float* aabb_host, float min_near,
                            const float* t_rand, const float* u, uint32_t N,
                            uint32_t T, uint32_t t, uint32_t n_classes,
                            float density_scale, uint32_t image_width,
                            float* image, float* depth, float* semantics,
                            void* ws, void* stream);

/* ======================= training (backward) ============================== */

/* A fragments of W^T for the dX = W^T dY passes (layout: DESIGN.md).
 * ucsa_mlp_pack_t_size() elements; call after every parameter update. */
uint32_t ucsa_mlp_pack_t_size(int32_t kind, uint32_t n_classes);
int32_t ucsa_mlp_pack_t(int32_t kind, const float* params, float* packed_t,
                        uint32_t n_classes, void* stream);

/* grad[p] = (accumulate ? grad[p] : 0) + sum_w partial[w][p], summed in a
 * fixed order (deterministic alternative to float atomics for dW). */
int32_t ucsa_reduce_partials(const float* partial, uint32_t n_parts,
                             uint32_t n_params, int32_t accumulate,
                             float* grad, void* stream);

/* The same for up to 4 (partial, grad) pairs in ONE launch (the MLP gradients
 * of a training step).  All arrays are HOST arrays of `count` entries; the
 * summation order per parameter is that of ucsa_reduce_partials. */
int32_t ucsa_reduce_partials_multi(uint32_t count, const float* const* partials,
                                   const uint32_t* n_parts,
                                   const uint32_t* n_params,
                                   float* const* grads, int32_t accumulate,
                                   void* stream);

/* Backward of ucsa_sigma_mlp_fwd (autograd of tcnn.Network in density(),
 * reference network_tcnn_semantics.py:135).  d_h [M,16] is the gradient wrt
 * the RAW outputs (slot 0 already multiplied by the trunc_exp backward,
 * reference activation.py:17-21).  Out: d_feat [n_levels][M][2] and per-wave
 * dW partials [ucsa_sigma_mlp_bwd_parts(M)][3072] (tcnn layout). */
uint32_t ucsa_sigma_mlp_bwd_parts(uint32_t M);
int32_t ucsa_sigma_mlp_bwd(const float* feat, const float* d_h,
                           const float* packed_sigma,
                           const float* packed_sigma_t, uint32_t M,
                           uint32_t n_levels, float* d_feat, float* partial,
                           void* stream);
/* The same with the recomputed hidden layer rounded to fp16 before the ReLU
 * gate and dW2 read it: the backward of tiny-cuda-nn's fp16 sigma net
 * (`train_precision: tcnn`; packs of the fp16-rounded parameters, fp16 features
 * widened to fp32).  Reference network_tcnn_semantics.py:48-58,135. */
int32_t ucsa_sigma_mlp_bwd_h16(const float* feat, const float* d_h,
                               const float* packed_sigma,
                               const float* packed_sigma_t, uint32_t M,
                               uint32_t n_levels, float* d_feat, float* partial,
                               void* stream);
/* The same backward with its contractions on the bf16 MFMA pipe as two-term
 * splits (bf16x2, see ucsa_composite_bwd_x2): packed_sigma_x3 from
 * ucsa_mlp_pack_x3(UCSA_MLP_SIGMA), packed_sigma_t_x3 from ucsa_mlp_pack_t_x3
 * (8 fragments).  Same inputs, outputs and partial-slot count. */
int32_t ucsa_sigma_mlp_bwd_x2(const float* feat, const float* d_h,
                              const void* packed_sigma_x3,
                              const void* packed_sigma_t_x3, uint32_t M,
                              uint32_t n_levels, float* d_feat, float* partial,
                              void* stream);

/* ucsa_hashgrid_bwd_rays with 8-byte bin records: the (entry, vx, vy) records
 * of the fine levels carry their value pair as half2 x rec_scale (a power of
 * two > 0) -- half the record traffic of both passes; sums stay fp32.  For
 * the f16 training mode (tiny-cuda-nn accumulates its grid gradient from half2
 * values too).  The workspace is mandatory. */
int32_t ucsa_hashgrid_bwd_rays_h16(const ucsa_grid* grid, const float* rays_o,
                                   const float* rays_d, const float* z,
                                   const float* aabb_host, uint32_t N,
                                   uint32_t T, const float* d_feat,
                                   float* grad_table, void* workspace,
                                   float rec_scale, void* stream);

/* Transposed fp16 fragments for the f16 backward of the colour / semantics
 * nets (kind = UCSA_MLP_COLOR or UCSA_MLP_SEM), and the backward itself:
 * ucsa_composite_bwd with the two nets and their dX contractions on
 * 16x16x32 f16 MFMA (the forward recompute reproduces ucsa_composite_fwd_f16;
 * dW stays fp32).  `f16_scale` (a power of two, e.g. 1024): gradients entering
 * the f16 MFMAs are multiplied by it and every output divided -- tiny-cuda-nn's
 * loss scale; pass 1 when the incoming gradients already carry a GradScaler
 * scale.  Partials: ucsa_composite_bwd_parts_f16(N) slots. */
uint32_t ucsa_mlp_pack_t_f16_halves(int32_t kind, uint32_t n_classes);
int32_t ucsa_mlp_pack_t_f16(int32_t kind, const float* params, void* packed_half,
                            uint32_t n_classes, void* stream);
uint32_t ucsa_composite_bwd_parts_f16(uint32_t N);
int32_t ucsa_composite_bwd_f16(
    const float* rays_d, const float* norms, const float* z_c,
    const float* sigma_c, const float* h_c, const float* z_f,
    const float* sigma_f, const float* h_f, const int32_t* src,
    const float* weights, const void* packed_color_half,
    const void* packed_sem_half, const void* packed_color_t_half,
    const void* packed_sem_t_half, const float* d_image, const float* d_depth,
    const float* d_sem, uint32_t N, uint32_t T, uint32_t t, uint32_t n_classes,
    float density_scale, float f16_scale, float* G, float* d_h_c, float* d_h_f,
    float* partial_color, float* partial_sem, void* stream);

/* The same backward with every contraction of the two nets on the bf16 MFMA
 * pipe as TWO-term splits ("bf16x2": x = bf16(x) + bf16(x - bf16(x)), three
 * partial products per product, 2^-16 relative, fp32 range: no loss scale) --
 * the gradient contractions of `nerf: {train_precision: bf16x3}`, whose forward
 * is ucsa_composite_train_fwd_x3.  Weights: ucsa_mlp_pack_x3 buffers and their
 * transposed form ucsa_mlp_pack_t_x3 (fragments of ucsa_mlp_pack_t_f16, three
 * exact bf16 terms each; ucsa_mlp_pack_t_x3_bytes).  Partials:
 * ucsa_composite_bwd_parts(N) slots.  Runs as the per-net kernel pair only
 * (argument 0 error under UCSA_SHADE_BWD_SPLIT=0). */
uint32_t ucsa_mlp_pack_t_x3_bytes(int32_t kind, uint32_t n_classes);
int32_t ucsa_mlp_pack_t_x3(int32_t kind, const float* params, void* packed_x3,
                           uint32_t n_classes, void* stream);
int32_t ucsa_composite_bwd_x2(
    const float* rays_d, const float* norms, const float* z_c,
    const float* sigma_c, const float* h_c, const float* z_f,
    const float* sigma_f, const float* h_f, const int32_t* src,
    const float* weights, const void* packed_color_x3, const void* packed_sem_x3,
    const void* packed_color_t_x3, const void* packed_sem_t_x3,
    const float* d_image, const float* d_depth, const float* d_sem, uint32_t N,
    uint32_t T, uint32_t t, uint32_t n_classes, float density_scale, float* G,
    float* d_h_c, float* d_h_f, float* partial_color, float* partial_sem,
    void* stream);

/* Backward of ucsa_hashgrid_encode_rays: adds into grad_table
 * [total_entries,2] (caller zeroes it).  Autograd of tcnn.Encoding.
 * With a workspace of ucsa_hashgrid_bwd_workspace_bytes() the binned two-pass
 * algorithm is used (no global float atomics); workspace == NULL selects the
 * direct-atomics kernels. */
uint64_t ucsa_hashgrid_bwd_workspace_bytes(uint32_t N, uint32_t T,
                                           uint32_t n_levels);
int32_t ucsa_hashgrid_bwd_rays(const ucsa_grid* grid_host, const float* rays_o,
                               const float* rays_d, const float* z,
                               const float* aabb_host, uint32_t N, uint32_t T,
                               const float* d_feat, float* grad_table,
                               void* workspace, void* stream);
/* Both density passes of a training step (the coarse samples z_c [N,Tc] and the
 * resampled ones z_f [N,Tf], renderer_semantics.py:154-236) in ONE call: every
 * ray's Tc + Tf samples are walked in SORTED depth order -- src [N,Tc+Tf] int32
 * as ucsa_composite_fwd / _train_fwd_x3 wrote it (e < Tc: coarse sample e, else
 * fine sample e - Tc).  On the coarse levels the fine samples fall into cells
 * the coarse samples of the same ray already visit: the merged walk combines
 * them into the same runs, so the fine pass adds almost no accumulator traffic;
 * half the launches.  d_feat_c [L][N*Tc][2], d_feat_f [L][N*Tf][2]; workspace
 * ucsa_hashgrid_bwd_workspace_bytes(N, Tc + Tf, L) (required).  The gradient
 * of the two single-pass calls up to the order of fp32 additions. */
int32_t ucsa_hashgrid_bwd_rays_merged(
    const ucsa_grid* grid, const float* rays_o, const float* rays_d,
    const float* z_c, const float* z_f, const int32_t* src, const float* aabb_host,
    uint32_t N, uint32_t Tc, uint32_t Tf, const float* d_feat_c,
    const float* d_feat_f, float* grad_table, void* workspace, void* stream);

/* Deterministic form of ucsa_hashgrid_bwd_rays (debug / reproducibility mode,
 * `UCSA_DETERMINISTIC=1`; SURVEY 5 "race detection": the reference only seeds,
 * scripts/train_joint.py:48 `seed_everything`; this is what
 * torch.use_deterministic_algorithms would ask of its backward,
 * joint_train_lightning_net.py:509-513): every contribution w * d_feat as 64-bit fixed point (2^-44 units) added
 * with integer atomics -- the sum does not depend on the order of the additions,
 * so two runs of a step give the same bits.  `fix`: int64
 * [ucsa_hashgrid_bwd_det_workspace_bytes / 8], zeroed by the caller, accumulates
 * over any number of _det calls (both density passes); _finish adds it into
 * grad_table (NaN everywhere if a contribution was non-finite or >= 2^18, or if
 * an entry's running sum left int64 -- each addition checks its own overflow). */
uint64_t ucsa_hashgrid_bwd_det_workspace_bytes(const ucsa_grid* grid);
int32_t ucsa_hashgrid_bwd_rays_det(const ucsa_grid* grid, const float* rays_o,
                                   const float* rays_d, const float* z,
                                   const float* aabb_host, uint32_t N, uint32_t T,
                                   const float* d_feat, void* fix, void* stream);
int32_t ucsa_hashgrid_bwd_det_finish(const ucsa_grid* grid, const void* fix,
                                     float* grad_table, void* stream);

/* ucsa_hashgrid_bwd_rays / ucsa_hashgrid_bwd_rays_merged with PACKED bin
 * records: one 64-bit word = entry index inside its bin (L bits) | vx | vy,
 * each value the fp32 rounded to nearest-even to its top min(32, (64 - L) / 2)
 * bits -- 26 bits (2^-18 relative) for the 2^19-entry levels of the
 * reference's grid; since round 6 two such words travel as ONE 16-byte record
 * per x-pair of corners (the corners x and x + 1 of a cell share a bin: half the
 * records, counters and staging slots).  Half the record bytes of both passes;
 * the sums stay fp32; non-finite values stay non-finite.  Meant for training modes whose MLP
 * backward is itself a two-term bf16 split (2^-16): the Python host uses them
 * for bwd_precision "bf16x2".  Same arguments; the workspace is mandatory.
 * (No reference counterpart: tiny-cuda-nn scatters with atomics,
 * nr4seg/nerf/network_tcnn_semantics.py:36-46 is the call site.) */
int32_t ucsa_hashgrid_bwd_rays_p64(const ucsa_grid* grid, const float* rays_o,
                                   const float* rays_d, const float* z,
                                   const float* aabb_host, uint32_t N,
                                   uint32_t T, const float* d_feat,
                                   float* grad_table, void* workspace,
                                   void* stream);
int32_t ucsa_hashgrid_bwd_rays_merged_p64(
    const ucsa_grid* grid, const float* rays_o, const float* rays_d,
    const float* z_c, const float* z_f, const int32_t* src, const float* aabb_host,
    uint32_t N, uint32_t Tc, uint32_t Tf, const float* d_feat_c,
    const float* d_feat_f, float* grad_table, void* workspace, void* stream);

/* ---- the differentiable render of a training step as TWO calls --------------
 * SURVEY 8(b)'s ucsa_render_fused_fwd / ucsa_render_fused_bwd.  Replaces
 * SemanticNeRFRenderer.run under autograd (reference
 * nr4seg/nerf/renderer_semantics.py:123-299 as driven by
 * nr4seg/lightning/joint_train_lightning_net.py:473-513): rows a2-a9 for N rays
 * with T coarse + t fine samples, forward keeping what the backward needs, and
 * the backward down to the four flat parameter gradients.  Arithmetic of the
 * default training mode: bf16x3 nets forward (fp32-grade), bf16x2 contractions
 * and 8-byte packed bin records backward.  Both only SEQUENCE the per-stage
 * entry points above on `stream` (same launches, order and arguments as the
 * Python host issues one by one: bit-identical results); they never allocate or
 * synchronise.  All buffers are the caller's, device memory, fp32 unless noted. */
typedef struct ucsa_train_buffers {
  float* z_c;     /* [N,T]  coarse depths */
  float* feat_c;  /* [L][N*T][2]  their hash-grid features */
  float* h_c;     /* [N*T,16]  raw sigma-net outputs */
  float* sigma_c; /* [N,T] */
  float* z_f;     /* [N,t]  resampled depths (t > 0) */
  float* feat_f;  /* [L][N*t][2] */
  float* h_f;     /* [N*t,16] */
  float* sigma_f; /* [N,t] */
  int32_t* src;   /* [N,T+t]  sorted order of the merged samples */
  float* weights; /* [N,T+t]  compositing weights in that order */
} ucsa_train_buffers;

typedef struct ucsa_train_packs {
  const void* sigma_x3;   /* ucsa_mlp_pack_x3(UCSA_MLP_SIGMA) */
  const void* color_x3;   /* ... UCSA_MLP_COLOR */
  const void* sem_x3;     /* ... UCSA_MLP_SEM */
  const void* sigma_t_x3; /* ucsa_mlp_pack_t_x3: backward only (may be NULL forward) */
  const void* color_t_x3;
  const void* sem_t_x3;
  const void* sigma_h2;   /* ucsa_mlp_pack_h2: when all three are non-NULL the FORWARD */
  const void* color_h2;   /* runs the nets as f16x2 (three MFMA passes per product    */
  const void* sem_h2;     /* instead of six; same fp32-grade error) -- may be NULL     */
} ucsa_train_packs;

uint64_t ucsa_render_fused_fwd_workspace_bytes(uint32_t N, uint32_t T, uint32_t t);
/* t_rand [N,T] or NULL (no perturbation), u [N,t] (t > 0).  Writes `out`
 * (every member; the *_f ones only when t > 0), image [N,3], depth [N],
 * semantics [N,n_classes]. */
int32_t ucsa_render_fused_fwd(
    const ucsa_grid* grid, const float* table, const ucsa_train_packs* packs,
    const float* rays_o, const float* rays_d, const float* norms,
    const float* aabb_host, float min_near, const float* t_rand, const float* u,
    uint32_t N, uint32_t T, uint32_t t, uint32_t n_classes, float density_scale,
    const ucsa_train_buffers* out, float* image, float* depth, float* semantics,
    void* workspace, void* stream);

uint64_t ucsa_render_fused_bwd_workspace_bytes(uint32_t N, uint32_t T, uint32_t t,
                                               uint32_t n_classes,
                                               uint32_t n_levels);
/* `saved` as ucsa_render_fused_fwd left it.  grad_table [total_entries,2] is
 * ADDED to (zero it first); grad_sigma [3072], grad_color [7168] and grad_sem
 * [1024 + 1024 * ceil(n_classes / 16)] are overwritten (layouts of the flat
 * tcnn parameter tensors, ucsa_mlp_pack). */
int32_t ucsa_render_fused_bwd(
    const ucsa_grid* grid, const ucsa_train_packs* packs, const float* rays_o,
    const float* rays_d, const float* norms, const float* aabb_host,
    const ucsa_train_buffers* saved, const float* d_image, const float* d_depth,
    const float* d_sem, uint32_t N, uint32_t T, uint32_t t, uint32_t n_classes,
    float density_scale, float* grad_table, float* grad_sigma, float* grad_color,
    float* grad_sem, void* workspace, void* stream);

/* ucsa_hashgrid_bwd_rays_merged with the half2 x rec_scale records of
 * ucsa_hashgrid_bwd_rays_h16 (training modes fp16 / tcnn). */
int32_t ucsa_hashgrid_bwd_rays_merged_h16(
    const ucsa_grid* grid, const float* rays_o, const float* rays_d,
    const float* z_c, const float* z_f, const int32_t* src, const float* aabb_host,
    uint32_t N, uint32_t Tc, uint32_t Tf, const float* d_feat_c,
    const float* d_feat_f, float* grad_table, void* workspace, float rec_scale,
    void* stream);

/* Backward of ucsa_hashgrid_encode_points (x [M,3] explicit points; workspace
 * of ucsa_hashgrid_bwd_workspace_bytes(M, 1, n_levels) or NULL). */
int32_t ucsa_hashgrid_bwd_points(const ucsa_grid* grid_host, const float* x,
                                 uint32_t M, const float* d_feat,
                                 float* grad_table, void* workspace,
                                 void* stream);

/* Backward of ucsa_composite_fwd (autograd of renderer_semantics.py:238-299
 * and the masked color()/semantics()).  Needs the forward's `src` and
 * `weights`.  Out: d_h_c [N*T,16], d_h_f [N*t,16] (all 16 slots; slot 0 is
 * d/d(log-density)), scratch G [N,S], per-wave partials
 * [ucsa_composite_bwd_parts(N)][7168] and [..][1024 + 1024*ceil(C/16)]. */
uint32_t ucsa_composite_bwd_parts(uint32_t N);
int32_t ucsa_composite_bwd(
    const float* rays_d, const float* norms, const float* z_c,
    const float* sigma_c, const float* h_c, const float* z_f,
    const float* sigma_f, const float* h_f, const int32_t* src,
    const float* weights, const float* packed_color, const float* packed_sem,
    const float* packed_color_t, const float* packed_sem_t,
    const float* d_image, const float* d_depth, const float* d_sem, uint32_t N,
    uint32_t T, uint32_t t, uint32_t n_classes, float density_scale, float* G,
    float* d_h_c, float* d_h_f, float* partial_color, float* partial_sem,
    void* stream);

/* torch.optim.Adam step as configured at reference
 * joint_train_lightning_net.py:897-919 (L2 weight decay in the gradient,
 * non-AMSGrad).  `step` is 1-based; grads are multiplied by inv_grad_scale
 * first (GradScaler unscale, :509-513). */
int32_t ucsa_adam_step(float* params, const float* grads, float* exp_avg,
                       float* exp_avg_sq, uint64_t n, uint32_t step, float lr,
                       float beta1, float beta2, float eps, float weight_decay,
                       float inv_grad_scale, void* stream);

/* The same step under torch.amp.GradScaler(enabled=True) (reference
 * joint_train_lightning_net.py:46,:509-513) without a host read-back: the
 * scale and the found-inf flag are DEVICE scalars (what GradScaler hands to
 * optimizers with _step_supports_amp_scaling).  found_inf[0] != 0: nothing is
 * written and the step does not count -- the bias corrections use
 * step - skipped[0].  Call ucsa_adam_count_skipped once per optimizer step
 * after the last tensor (skipped[0] += found_inf[0] != 0). */
int32_t ucsa_adam_step_scaled(float* params, const float* grads, float* exp_avg,
                              float* exp_avg_sq, uint64_t n, uint32_t step,
                              float lr, float beta1, float beta2, float eps,
                              float weight_decay, const float* grad_scale,
                              const float* found_inf, const uint32_t* skipped,
                              void* stream);
int32_t ucsa_adam_count_skipped(const float* found_inf, uint32_t* skipped,
                                void* stream);

/* ======================= losses / post-processing / metric ================ */

/* Scratch floats needed by the reductions below for n rays / pixels. */
uint32_t ucsa_loss_partial_floats(uint32_t n);

/* NeRF losses of reference joint_train_lightning_net.py:180-223 with the
 * weighting of :44-45,:503-507, and (when d_* != NULL) the gradient of
 * grad_scale * total wrt the rendered outputs.
 *   rgb,gt_rgb [N,3]; sem [N,C] composited probabilities; depth, gt_depth [N];
 *   labels [N] int64 (-1 ignored).  stats[8] (device) = {loss_color,
 *   loss_semantics (NaN = the reference's None), loss_depth, n_invalid_sem,
 *   n_valid_depth, total, loss_semantics with None as 0, 0}. */
int32_t ucsa_nerf_loss(const float* rgb, const float* sem, const float* depth,
                       const float* gt_rgb, const int64_t* labels,
                       const float* gt_depth, uint32_t N, uint32_t C,
                       float one_m_to_scene_uom, float w_sem, float w_depth,
                       float grad_scale, float* stats, float* d_rgb,
                       float* d_sem, float* d_depth, float* partial,
                       void* stream);

/* Backward of the loss node of reference joint_train_lightning_net.py:497-513
 * (`total.backward()` / `scaler.scale(total).backward()`) in one launch, from
 * the gradients ucsa_nerf_loss wrote with the same w_sem / w_depth:
 *   out_rgb = d_rgb * (g_total + g_color),  out_sem = d_sem * (g_total + g_sem / w_sem),
 *   out_depth = d_depth * (g_total + g_depth / w_depth)
 * (out_* may alias d_* for an in-place update; the autograd node writes fresh
 * buffers so that a second backward through a retained graph sees the stored
 * gradients unscaled -- ADVICE r4)
 * where g_* are DEVICE scalars (the cotangents autograd hands back: of the
 * total, and of the single terms when a caller combined them itself); NULL = 0.
 * Replaces the ~10 elementwise launches torch's autograd spends on
 * `lc + 0.04 ls + 0.1 ld` and its backward. */
int32_t ucsa_nerf_loss_apply(const float* d_rgb, const float* d_sem,
                             const float* d_depth, float* out_rgb,
                             float* out_sem, float* out_depth,
                             uint32_t N, uint32_t C, const float* g_total,
                             const float* g_color, const float* g_sem,
                             const float* g_depth, float w_sem, float w_depth,
                             void* stream);

/* reference joint_train_lightning_net.py:246-251: rows summing to 0 become
 * uniform, normalise, argmax.  normalised may be NULL. */
int32_t ucsa_semantic_postproc(const float* sem, uint32_t N, uint32_t C,
                               float* normalised, int64_t* argmax,
                               void* stream);

/* Segmentation tail on NCHW logits [B,C,P]: softmax (prob, may be NULL),
 * argmax (may be NULL) and, when labels != NULL, the reference's
 * CrossEntropyLoss(ignore_index=-1, reduction="none")(softmax(out), label)
 * .mean() (double softmax; :37-38,:163,:456-458) plus grad_scale * dLoss/dlogits
 * (d_logits may be NULL). */
int32_t ucsa_seg_tail(const float* logits, const int64_t* labels, uint32_t B,
                      uint32_t C, uint32_t P, float grad_scale, float* prob,
                      int64_t* argmax, float* loss, float* d_logits,
                      float* partial, void* stream);

/* ============ fused BatchNorm2d (+ residual) (+ ReLU), channels-last ======
 * The memory-bound passes between DeepLabV3's convolutions (row a14;
 * reference nr4seg/network/deeplabv3.py:6-19 -> torchvision's bottlenecks:
 * conv -> BatchNorm2d -> ReLU and conv -> BatchNorm2d -> (+ identity) -> ReLU;
 * replaces torch.nn.functional.batch_norm + add + relu and their backward
 * kernels).  Activations are NHWC, i.e. row-major [M = N*H*W][C], C % 4 == 0,
 * 16-byte aligned; dtype 0 = fp32, 1 = bf16 (statistics, gamma / beta and all
 * sums are fp32 / double either way).
 *
 * forward:  y = relu?( (x - mean) * invstd * gamma + beta (+ residual) )
 *   training != 0: batch statistics (biased variance); running_mean /
 *     running_var (may both be NULL) updated as torch.nn.BatchNorm2d does
 *     (momentum, unbiased variance = biased * M / (M - 1), and the biased one
 *     itself when M = 1); save_mean / save_invstd [C] written for the backward.
 *     Without running statistics the variance is summed around 0: its
 *     accuracy falls with (mean / std)^2 (table in csrc/batchnorm.hip).
 *   training == 0: the running statistics normalise; save_* untouched.
 *   The fused ReLU keeps NaN (y = pre < 0 ? 0 : pre), as torch.relu does.
 * backward: g = dy * (y > 0) when relu (y = the forward's output), else dy;
 *   dresidual (may be NULL) = g; dbeta = sum g; dgamma = sum g * xhat;
 *   dx = gamma * invstd * (g - dbeta / M - xhat * dgamma / M)   (training mode).
 * workspace: ucsa_bn_workspace_bytes(M, C) bytes of caller-owned scratch.
 * C <= 4096. */
uint64_t ucsa_bn_workspace_bytes(uint32_t M, uint32_t C);
int32_t ucsa_bn_act_fwd(const void* x, const void* residual, const float* gamma,
                        const float* beta, float* running_mean,
                        float* running_var, float momentum, float eps,
                        uint32_t M, uint32_t C, int32_t relu, int32_t training,
                        int32_t dtype, void* y, float* save_mean,
                        float* save_invstd, void* workspace, void* stream);
int32_t ucsa_bn_act_bwd(const void* dy, const void* x, const void* y,
                        const float* gamma, const float* save_mean,
                        const float* save_invstd, uint32_t M, uint32_t C,
                        int32_t relu, int32_t dtype, void* dx, void* dresidual,
                        float* dgamma, float* dbeta, void* workspace,
                        void* stream);

/* Confusion matrix, rows = truth, truth == -1 dropped (reference
 * nr4seg/utils/metrics.py:31-46); adds into cm [C,C] int64. */
int32_t ucsa_confusion_matrix(const int64_t* preds, const int64_t* truths,
                              uint64_t n, uint32_t C, int64_t* cm,
                              void* stream);

/* ============ occupancy-grid ray marching ===============
 * The `_raymarching` functions that are dormant in the reference
 * (bindings.cpp:8-16, raymarching.h:9-18).  Same argument meaning as the
 * reference's host functions; at::Tensor -> device pointer.  Where the CUDA
 * kernels hand out output slots with atomicAdd (arrival order), these use
 * prefix sums over the ray index: deterministic, and one of the orders the
 * reference can produce.  density_grid is [C,H,H,H] fp32. */

/* Scratch for ucsa_march_rays_train over N rays. */
uint64_t ucsa_march_workspace_bytes(uint32_t N);

/* Replaces march_rays_train (reference raymarching.cu:138-307,:490-498;
 * wrapper raymarching.py:54-163).  xyzs, dirs [M,3], deltas [M,2] (dt, and
 * t - last_t for depth), rays [N,3] int32 = (ray id, first point, n points);
 * counter[2] int32 += (points, rays), its old values are the bases.  A ray
 * whose span would reach M is counted but not written.  perturb != 0 jitters
 * the start by MIN_STEPSIZE * pcg32(n).next_float(). */
int32_t ucsa_march_rays_train(const float* rays_o, const float* rays_d,
                              const float* density_grid, float mean_density,
                              float bound, float dt_gamma, uint32_t N,
                              uint32_t C, uint32_t H, uint32_t M,
                              const float* nears, const float* fars,
                              float* xyzs, float* dirs, float* deltas,
                              int32_t* rays, int32_t* counter, uint32_t perturb,
                              void* workspace, void* stream);

/* Replaces composite_rays_train_forward (reference raymarching.cu:318-394,
 * :501-509) and, with n_sem > 0, the disabled
 * composite_rays_train_semantics_forward (raymarching.h:12,
 * raymarching.py:249-309): local_sem [M,n_sem] is composited with the same
 * weights into semantics [N,n_sem].  Outputs are indexed by ray id. */
int32_t ucsa_composite_rays_train_fwd(const float* sigmas, const float* rgbs,
                                      const float* local_sem,
                                      const float* deltas, const int32_t* rays,
                                      uint32_t M, uint32_t N, uint32_t n_sem,
                                      float* weights_sum, float* depth,
                                      float* image, float* semantics,
                                      void* stream);

/* Replaces composite_rays_train_backward (reference raymarching.cu:408-487,
 * :512-520).  Rows of grad_sigmas / grad_rgbs / grad_local_sem that belong to
 * no composited ray are left untouched (the caller zero-fills,
 * raymarching.py:225-226).  The semantic weights are detached, as on the live
 * path (reference renderer_semantics.py:268-271). */
int32_t ucsa_composite_rays_train_bwd(
    const float* grad_weights_sum, const float* grad_image,
    const float* grad_semantics, const float* sigmas, const float* rgbs,
    const float* deltas, const int32_t* rays, const float* weights_sum,
    const float* image, uint32_t M, uint32_t N, uint32_t n_sem,
    float* grad_sigmas, float* grad_rgbs, float* grad_local_sem, void* stream);

/* Replaces march_rays (reference raymarching.cu:528-634,:637-643; wrapper
 * raymarching.py:367-449): up to n_step points for each of the first n_alive
 * entries of rays_alive / rays_t into rows [n*n_step, (n+1)*n_step); rows
 * past a ray's last point are left untouched (zero-filled by the caller). */
int32_t ucsa_march_rays(uint32_t n_alive, uint32_t n_step,
                        const int32_t* rays_alive, const float* rays_t,
                        const float* rays_o, const float* rays_d, float bound,
                        float dt_gamma, uint32_t C, uint32_t H,
                        const float* density_grid, float mean_density,
                        const float* nears, const float* fars, float* xyzs,
                        float* dirs, float* deltas, uint32_t perturb,
                        void* stream);

/* Replaces composite_rays (reference raymarching.cu:647-729,:732-738, unbound
 * in bindings.cpp; wrapper raymarching.py:455-501) and, with n_sem > 0,
 * composite_rays_semantics (raymarching.py:507-555).  In place on
 * weights_sum/depth/image/semantics (by ray id) and rays_t (by slot; -1 marks
 * a ray that stopped: zero delta, or transmittance below 1e-4). */
int32_t ucsa_composite_rays(uint32_t n_alive, uint32_t n_step,
                            const int32_t* rays_alive, float* rays_t,
                            const float* sigmas, const float* rgbs,
                            const float* local_sem, const float* deltas,
                            uint32_t n_sem, float* weights_sum, float* depth,
                            float* image, float* semantics, void* stream);

/* Scratch for ucsa_compact_rays over n_alive slots. */
uint64_t ucsa_compact_workspace_bytes(uint32_t n_alive);

/* Replaces compact_rays (reference raymarching.cu:838-864; wrapper
 * raymarching.py:561-592): slots with rays_t_old >= 0 are copied, in order,
 * to rays_alive / rays_t starting at alive_counter[0], which is advanced. */
int32_t ucsa_compact_rays(uint32_t n_alive, int32_t* rays_alive,
                          const int32_t* rays_alive_old, float* rays_t,
                          const float* rays_t_old, int32_t* alive_counter,
                          void* workspace, void* stream);

/* ---- training through the marcher ---------------------------------------------
 * Forward / backward of one training batch sampled by ucsa_march_rays_train
 * (rays [N,3] = ray id, first point, count; M points).  What the reference's
 * parent code did with march_rays_train -> network -> composite_rays_train,
 * fused like the inference path: sigma / h [M,16] come from the sigma MLP,
 * the colour and semantics nets run inside, only on samples with w > w_min.
 *   rays rows must be in point order (row n's span starts where row n-1's
 *   ends, as ucsa_march_rays_train writes them): a wave streams the points
 *   of its rows as one contiguous range.
 *   fwd: weights_sum, depth (= sum w*t, t measured from the ray origin:
 *        nears[ray] + the accumulated deltas), image, semantics by ray id --
 *        ADDED to zero-filled buffers; w_out, t_out [M] (zero-filled) keep
 *        each sample's weight and ray parameter for the backward.  No early
 *        stop (raymarching.cu:363 is commented out in the reference as well);
 *        spans reaching M are skipped (:338).
 *   span length: a rays row composites at most 1024 samples (the marcher's
 *        MAX_STEPS; ucsa_march_rays_train writes no longer span).  A row with
 *        count > 1024 is DROPPED by both passes exactly like one with
 *        first + count >= M: its ray's outputs stay zero, its rows of w_out /
 *        t_out / d_h stay zero, its rows of G are not written, and the spans
 *        after it are composited as usual.  (The backward keeps one LDS float
 *        per sample of a span, 1024 per wave.)
 *   bwd: d_image [N,3], d_depth [N] (wrt depth/norms[ray]), d_sem [N,C] ->
 *        d_h [M,16] (slot 0: d/d log-density incl. the trunc_exp backward),
 *        scratch G [M], per-wave dW partials
 *        [ucsa_composite_bwd_parts(N)][7168] and [..][1024+1024*ceil(C/16)].
 *        Semantic weights are detached (reference renderer_semantics.py:270).
 *        Unlike the reference's composite_rays_train backward
 *        (raymarching.py:209) the depth gradient IS propagated, as the live
 *        path does. */
int32_t ucsa_march_train_fwd(
    const int32_t* rays, uint32_t N, uint32_t M, const float* nears,
    const float* rays_d, const float* sigmas, float sigma_scale, const float* h,
    const float* deltas, const float* packed_color, const float* packed_sem,
    uint32_t n_classes, float w_min, float* weights_sum, float* depth,
    float* image, float* semantics, float* w_out, float* t_out, void* stream);

int32_t ucsa_march_train_bwd(
    const int32_t* rays, uint32_t N, uint32_t M, const float* rays_d,
    const float* norms, const float* sigmas, float sigma_scale, const float* h,
    const float* deltas, const float* w_all, const float* t_all,
    const float* packed_color, const float* packed_sem,
    const float* packed_color_t, const float* packed_sem_t, uint32_t n_classes,
    float w_min, const float* d_image, const float* d_depth, const float* d_sem,
    float* G, float* d_h, float* partial_color, float* partial_sem,
    void* stream);

/* ---- density-grid maintenance -----------------------------------------------
 * No counterpart in the reference's FFI: the reference keeps the state
 * (density_grid [cascade,128,128,128], mean_density, iter_density:
 * renderer_semantics.py:91-103,111-121) that march_rays* read, but ships no
 * code that fills it.  These two entries do, for cuda_ray=True. */

/* One point per cell of cascade `cascade` of an [H,H,H] grid over
 * [-b,b]^3, b = min(2^cascade, bound): the cell centre plus, when seed != 0, a
 * pcg32(cell, seed) jitter inside the cell.  xyz [H^3,3], cell order
 * x*H*H + y*H + z (the marcher's lookup order, raymarching.cu:204). */
int32_t ucsa_density_grid_points(uint32_t cascade, uint32_t H, float bound,
                                 uint32_t seed, float* xyz, void* stream);

uint64_t ucsa_density_grid_workspace_bytes(void);

/* density_grid[i] = max(density_grid[i]*decay, fresh[i]*fresh_scale) where
 * both are >= 0 (negative marks "never update"); *mean_density (device) =
 * mean(max(density_grid, 0)).  n = cascade*H^3. */
int32_t ucsa_density_grid_update(float* density_grid, const float* fresh,
                                 uint64_t n, float decay, float fresh_scale,
                                 float* mean_density, void* workspace,
                                 void* stream);

/* ---- segmented marching: the inference loop without per-step host round trips
 * No counterpart in the reference's FFI.  The reference API above pads every
 * alive ray to n_step rows and needs the survivor count on the host after
 * every iteration; these entries march up to `cap` samples per alive ray into
 * an exact-size buffer, composite them with the same early-termination rule
 * (raymarching.cu:693-706) one wave per ray, and keep the alive count in
 * device memory.  n_cap = host upper bound of the alive count (launch size);
 * n_alive_dev = device int32 holding the actual count, or NULL (= n_cap).
 * Slot n of rays_alive / rays_t / span is alive ray n of this round. */
uint64_t ucsa_march_segment_workspace_bytes(uint32_t n_cap);

/* Count the samples of each alive ray (<= cap) from rays_t[n] on;
 * span[n] = (first point, count) int32 [n_cap,2]; workspace uint32[0] = total
 * points, [1] = alive count used (device; read them back to size the point
 * buffers).  perturb != 0 jitters the start by MIN_STEPSIZE*pcg32(ray,
 * perturb) -- pass it in the first round only, and to _write as well. */
int32_t ucsa_march_segment_count(uint32_t n_cap, const int32_t* n_alive_dev,
                                 uint32_t cap, const int32_t* rays_alive,
                                 const float* rays_t, const float* rays_o,
                                 const float* rays_d, float bound,
                                 float dt_gamma, uint32_t C, uint32_t H,
                                 const float* density_grid, float mean_density,
                                 const float* fars, uint32_t perturb,
                                 int32_t* span, void* workspace, float* stage,
                                 void* stream);

/* `stage` (optional, ucsa_march_segment_stage_bytes(n_cap, cap) bytes): when
 * given to _count, the samples are kept in slot-major staging rows during the
 * counting march and _write (same `stage`, same `cap`) only copies them into
 * place -- one march per round instead of two.
 * Write the counted samples: xyzs, dirs [M,3], deltas [M,2] as march_rays. */
uint64_t ucsa_march_segment_stage_bytes(uint32_t n_cap, uint32_t cap);
int32_t ucsa_march_segment_write(uint32_t n_cap, const int32_t* n_alive_dev,
                                 const int32_t* rays_alive, const float* rays_t,
                                 const float* rays_o, const float* rays_d,
                                 float bound, float dt_gamma, uint32_t C,
                                 uint32_t H, const float* density_grid,
                                 float mean_density, const float* fars,
                                 uint32_t perturb, const int32_t* span,
                                 float* xyzs, float* dirs, float* deltas,
                                 const float* stage, uint32_t cap,
                                 void* stream);

/* Composite each slot's span onto weights_sum/depth/image/semantics (by ray
 * id, accumulated in place; sigma is multiplied by sigma_scale) and set
 * rays_t[n] = -1 if the ray is finished (transmittance fell below 1e-4, or the
 * span is shorter than cap), else the ray parameter after its last sample. */
int32_t ucsa_march_segment_composite(
    uint32_t n_cap, const int32_t* n_alive_dev, uint32_t cap,
    const int32_t* rays_alive, float* rays_t, const int32_t* span,
    const float* sigmas, float sigma_scale, const float* rgbs,
    const float* local_sem, const float* deltas, uint32_t n_sem,
    float* weights_sum, float* depth, float* image, float* semantics,
    void* stream);

/* Fused alternative to ucsa_point_shade_h + ucsa_march_segment_composite: the
 * weights (same early-stop rule) are formed first, the samples with
 * w > w_min are compacted with wave ballots, only those go through the colour
 * and semantics nets (MFMA, weights in LDS; h [M,16] = raw sigma-MLP rows,
 * rays_d [N,3] by ray id), and the per-ray sums are added in place.  w_min = 0
 * is the reference's composite exactly; 1e-4 is the mask of the live path
 * (reference renderer_semantics.py:249-250; depth is masked with it, as
 * there).  weights_sum always takes every sample. */
int32_t ucsa_march_segment_shade(
    uint32_t n_cap, const int32_t* n_alive_dev, uint32_t cap,
    const int32_t* rays_alive, float* rays_t, const int32_t* span,
    const float* rays_d, const float* sigmas, float sigma_scale, const float* h,
    const float* deltas, const float* packed_color, const float* packed_sem,
    uint32_t n_classes, float w_min, float* weights_sum, float* depth,
    float* image, float* semantics, void* stream);

/* Same with the fp16-MFMA nets (packed by ucsa_mlp_pack_f16). */
int32_t ucsa_march_segment_shade_f16(
    uint32_t n_cap, const int32_t* n_alive_dev, uint32_t cap,
    const int32_t* rays_alive, float* rays_t, const int32_t* span,
    const float* rays_d, const float* sigmas, float sigma_scale, const float* h,
    const float* deltas, const void* packed_color_half,
    const void* packed_sem_half, uint32_t n_classes, float w_min,
    float* weights_sum, float* depth, float* image, float* semantics,
    void* stream);

/* Same with the f16x2 nets (packed by ucsa_mlp_pack_h2: two f16 terms per operand,
 * three MFMA passes per product -- the fp32-grade arithmetic of ucsa_render_fwd_h2;
 * round 6). */
int32_t ucsa_march_segment_shade_h2(
    uint32_t n_cap, const int32_t* n_alive_dev, uint32_t cap,
    const int32_t* rays_alive, float* rays_t, const int32_t* span,
    const float* rays_d, const float* sigmas, float sigma_scale, const float* h,
    const float* deltas, const void* packed_color_h2, const void* packed_sem_h2,
    uint32_t n_classes, float w_min, float* weights_sum, float* depth,
    float* image, float* semantics, void* stream);

/* Stable compaction of the slots with rays_t_old >= 0 into rays_alive/rays_t;
 * n_alive_out[0] (device, != n_alive_dev) = number of survivors. */
int32_t ucsa_march_segment_compact(uint32_t n_cap, const int32_t* n_alive_dev,
                                   int32_t* rays_alive,
                                   const int32_t* rays_alive_old, float* rays_t,
                                   const float* rays_t_old,
                                   int32_t* n_alive_out, void* workspace,
                                   void* stream);

/* ---- rendered-image augmentation of the joint step -------
 * Replaces data_aug (reference joint_train_lightning_net.py:259-302; the
 * transforms of :89-101 are torchvision 0.12.0 tensor ops, ~40 kernels per
 * image).  Every random draw is an argument. */
typedef struct ucsa_aug_params {
  int32_t order[4];  /* ColorJitter's drawn permutation of 0 brightness,
                        1 contrast, 2 saturation, 3 hue */
  float brightness, contrast, saturation, hue; /* the four drawn factors */
  float angle_deg;   /* tvf.rotate angle (counter-clockwise, degrees) */
  int32_t flip;      /* != 0: tvf.hflip */
  int32_t crop_i, crop_j; /* RandomCrop.get_params top / left */
} ucsa_aug_params;

uint64_t ucsa_augment_workspace_bytes(uint32_t B, uint32_t H, uint32_t W);

/* img [B,3,H,W] in [0,1], label [B,H,W] int64 (-1 unknown) or NULL;
 * params_host: B structs on the HOST.  out_img [B,3,oh,ow], out_label
 * [B,oh,ow]: jitter -> rotate (bilinear, resp. nearest on label+1, fill 0) ->
 * crop to (oh,ow) at (crop_i,crop_j) -> flip. */
int32_t ucsa_augment(const float* img, const int64_t* label, uint32_t B,
                     uint32_t H, uint32_t W, const ucsa_aug_params* params_host,
                     uint32_t oh, uint32_t ow, float* out_img,
                     int64_t* out_label, void* workspace, void* stream);

/* ---- marching cubes (labelled-mesh export of the field) --------------------
 * Not on the reference's path (its parent code base, torch-ngp, ran marching
 * cubes on the CPU in extract_geometry / save_mesh).  Two passes over a dense
 * lattice field [nx,ny,nz] fp32, point (i,j,k) at field[(i*ny + j)*nz + k] and
 * at origin + (i,j,k)*spacing; a point is inside iff field > iso.
 *   ucsa_mc_count: cell cases, edge crossings and their prefix sums into the
 *     workspace; totals_dev[0] = V vertices, [1] = F triangles (uint32, device).
 *     A total above 2^31-1 is written as 0xFFFFFFFF in both: do not emit then.
 *   ucsa_mc_emit: verts [V,3], normals [V,3] fp32, tris [F,3] int32 into
 *     caller buffers sized from the totals (max_verts / max_faces: their
 *     capacities; nothing is written beyond them).  origin3 / spacing3 are HOST
 *     float[3].  Pass the same field, dims, iso and workspace as to the count.
 * Point p owns its +x,+y,+z edges (edge id 3*p + axis); one vertex per
 * crossing edge, in ascending edge id, shared by all its triangles.  Triangles
 * by ascending cell (= lower-corner point) index, then in table order, wound so
 * that face normals point toward lower field values.  Vertex on an edge:
 * t = (iso - f0) / (f1 - f0) (f0 at the lower index), coordinate along the
 * axis x0 + t*spacing.  Normal: -grad f by central differences (one-sided on
 * the lattice boundary) at both ends, lerped by t, normalised; (0,0,0) when
 * zero.  All fp32, no contraction, correctly rounded division / sqrt: the same
 * bits as the obvious numpy float32 code.  No atomics: two runs give the same
 * bytes.  Dims >= 2 each, nx*ny*nz <= 2^31-1 (else argument 1). */
uint64_t ucsa_mc_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int32_t ucsa_mc_count(const float* field, uint32_t nx, uint32_t ny, uint32_t nz,
                      float iso, void* workspace, uint32_t* totals_dev,
                      void* stream);
int32_t ucsa_mc_emit(const float* field, uint32_t nx, uint32_t ny, uint32_t nz,
                     float iso, const float* origin3, const float* spacing3,
                     const void* workspace, float* verts, float* normals,
                     int32_t* tris, uint32_t max_verts, uint32_t max_faces,
                     void* stream);

/* The same two passes over the observed part of a lattice: `valid` [nx,ny,nz]
 * uint8 (0 = invalid, anything else = valid; a TSDF volume's weight > 0).  An
 * edge carries a vertex iff it crosses the iso value AND both its end points
 * are valid; a cell emits its triangles iff ALL EIGHT corners are valid (every
 * edge of such a cell has two valid ends, so every index it emits exists).
 * Order, winding, interpolation as above.  Normal: per axis, the difference at
 * an end point runs from its lower to its upper neighbour as above, except that
 * a neighbour that is invalid (or off the lattice) is replaced by the point
 * itself -- the one-sided difference, divided by 1*spacing -- and with neither
 * neighbour usable the component is +0; then lerp and normalise as above.
 * Field values at invalid points are never used for positions or normals; they
 * are still compared with iso, which changes nothing that is emitted.  With
 * every point valid the output is byte for byte that of ucsa_mc_count /
 * ucsa_mc_emit.  Same workspace, totals, capacities and limits; dims are
 * arguments 2..4 here.  tests/tsdf_numpy.py restates it. */
int32_t ucsa_mc_count_masked(const float* field, const uint8_t* valid, uint32_t nx,
                             uint32_t ny, uint32_t nz, float iso, void* workspace,
                             uint32_t* totals_dev, void* stream);
int32_t ucsa_mc_emit_masked(const float* field, const uint8_t* valid, uint32_t nx,
                            uint32_t ny, uint32_t nz, float iso, const float* origin3,
                            const float* spacing3, const void* workspace, float* verts,
                            float* normals, int32_t* tris, uint32_t max_verts,
                            uint32_t max_faces, void* stream);

/* ---- mesh rasterization (not in the reference) ----------------------------
 * A triangle mesh seen from B posed pinhole cameras -> per pixel the visible
 * face, its z-depth, NYU40 label and colour (mesh-rendered labels / depth at
 * any pose; utils/mesh_render.py, scripts/render_mesh_labels.py).  Two passes:
 *   ucsa_raster_setup: per (view, face) a clipped, snapped record and the
 *     number of 16x16 screen tiles its box touches; per-tile counts and their
 *     scan.  total_dev[0] (uint64, device) = the (tile, face) pair total.
 *   ucsa_raster_draw: the tile lists into `pairs` (uint32, capacity
 *     max_pairs; total_pairs = the value read back from total_dev, at most
 *     2^31-1), then one work-group per tile writes tri_id / depth / label
 *     [B,H,W] and rgb [B,H,W,3] (capacity max_pixels >= B*H*W elements each).
 *     A capacity too small: argument error, nothing is written.  Pass the same
 *     mesh, cameras and workspace as to the setup.
 * Inputs: verts [V,3], faces [F,3] int32 (a face with an index outside
 * [0,V), read as unsigned, is skipped), poses [B,4,4] camera-to-world in the
 * field's (NGP) frame (the poses of ucsa_get_rays), fx, fy > 0, cx, cy HOST
 * scalars, 1 <= H, W <= 16384, near > 0, B <= 65535, B*F <= 2^31-1;
 * vertex_labels [V] int32 and vertex_rgb [V,3] may be NULL (label 0; rgb not
 * written, rgb may then be NULL).
 * Contract (fp32, no contraction, correctly rounded division; a numpy
 * restatement gives the same bits: tests/raster_numpy.py).  R = P[0:3,0:3],
 * t = P[0:3,3]:
 *   camera point of vertex p: d = p - t, c_r = (d0*R0r + d1*R1r) + d2*R2r;
 *   planes s(c) >= 0 keep: near z - near; guard band with G = 65536 px:
 *     x*fx + z*kL, z*kR - x*fx, y*fy + z*kT, z*kB - y*fy, where kL = cx + G,
 *     kR = (W + G) - cx, kT = cy + G, kB = (H + G) - cy (fp32);
 *   a face with a non-finite camera coordinate, or with all three corners
 *     outside one plane (s < 0 or NaN), draws nothing; a face inside all five
 *     is not clipped; otherwise Sutherland-Hodgman in that plane order,
 *     polygon from corners (0,1,2), edges (i, i+1 mod n), each kept vertex
 *     then the crossing vertex.  Every vertex carries the mask of the
 *     corners it lies on (corner k: 1<<k; new vertex: the union when that has
 *     two bits, else 7).  Crossing point of edge (A,B): with a two-bit union
 *     {i,j}, P and Q are the corners i and j, lower vertex index first (equal
 *     indices: lower corner), else P = A, Q = B; t = s(P) / (s(P) - s(Q)),
 *     NaN or < 0 -> 0, > 1 -> 1; X = P + t*(Q - P) per coordinate.  Faces
 *     sharing an edge thus get the same bits on it.  More than 12 vertices
 *     during, fewer than 3 or more than 8 after (rounding only): nothing;
 *   projection u = fx*(x/z) + cx, v = fy*(y/z) + cy, NaN or < -2^21 -> -2^21,
 *     > 2^21 -> 2^21; snapped X = rint(u*256), Y = rint(v*256) (round half to
 *     even, int32);
 *   coverage: fan triangles (0, k+1, k+2) of the polygon; area
 *     E(A->B, C) with E(P->Q, X) = (Qx-Px)(Xy-Py) - (Qy-Py)(Xx-Px) in int64;
 *     area 0 covers nothing, area < 0 swaps B and C; pixel (x, y) has centre
 *     (256x + 128, 256y + 128) and is covered iff for each edge P->Q of
 *     (A,B,C): E > 0, or E == 0 and the edge owns it (dy > 0, or dy == 0 and
 *     dx < 0, with (dx, dy) = Q - P).  No culling: both windings are drawn;
 *   depth of a covered pixel: ray d = ((x+0.5-cx)/fx, (y+0.5-cy)/fy, 1)
 *     (k_get_rays' order), e1 = c1-c0, e2 = c2-c0 of the UNCLIPPED corners,
 *     n = e1 x e2 (n0 = e1y*e2z - e1z*e2y, n1 = e1z*e2x - e1x*e2z,
 *     n2 = e1x*e2y - e1y*e2x), z = dot(n, c0) / ((n0*dx + n1*dy) + n2)
 *     (dot(a,b) = (a0*b0 + a1*b1) + a2*b2); non-finite -> zhi; clamped into
 *     [zlo, zhi], zlo = max(min z of the polygon, near), zhi = max(max z, zlo);
 *   visibility: the smallest key (float_bits(z) << 32) | face id wins;
 *   attributes: q = (z*dx - c0x, z*dy - c0y, z - c0z), w1 = dot(n, q x e2) /
 *     dot(n, n), w2 = dot(n, e1 x q) / dot(n, n), w0 = (1 - w1) - w2; any
 *     non-finite -> (1, 0, 0); label = vertex_labels of the corner with the
 *     largest w (ties: lowest corner); rgb = (w0*rgb0 + w1*rgb1) + w2*rgb2;
 *     depth = z, tri_id = face id.  Empty pixel: -1, 0, 0, (0, 0, 0).
 * Deterministic (integer atomics only, the winner is a minimum): two runs give
 * the same bytes.  Workspace (ucsa_raster_workspace_bytes): 132 bytes per
 * (view, face), 8 per 1024 (view, face), 12 per (view, 16x16 tile) plus
 * (tilesX + tilesY + 1) * 4 per view. */
uint64_t ucsa_raster_workspace_bytes(uint32_t B, uint32_t F, uint32_t H, uint32_t W);
int32_t ucsa_raster_setup(const float* verts, uint32_t V, const int32_t* faces,
                          uint32_t F, const float* poses, uint32_t B, float fx,
                          float fy, float cx, float cy, uint32_t H, uint32_t W,
                          float near, void* workspace, uint64_t* total_dev,
                          void* stream);
int32_t ucsa_raster_draw(const float* verts, uint32_t V, const int32_t* faces,
                         uint32_t F, const float* poses, uint32_t B, float fx,
                         float fy, float cx, float cy, uint32_t H, uint32_t W,
                         float near, const int32_t* vertex_labels,
                         const float* vertex_rgb, void* workspace, uint32_t* pairs,
                         uint64_t total_pairs, uint64_t max_pairs, int32_t* tri_id,
                         float* depth, int32_t* label, float* rgb,
                         uint64_t max_pixels, void* stream);

/* ---- label fusion: 2D label maps voted onto mesh vertices (not in the
 * reference) ---------------------------------------------------------------
 * Per-frame label maps -> per-vertex labels by multi-view voting
 * (utils/mesh_fusion.py, scripts/fuse_mesh_labels.py).  The projection is the
 * rasterizer's: render the mesh with vertex_labels = 1..V and every pixel's
 * `label` is the 1-based id of the vertex it votes for.
 *   ucsa_label_fuse_accumulate: N pixels vote into votes [V][C+1] uint64,
 *     row-major, allocated AND zeroed by the caller, accumulated over calls.
 *     Column 0 of a row is never written (kept so that column = class id).
 *     Pixel i votes iff ALL of
 *       1 <= vertex_id[i] <= V          (int32; <= 0 = no vote; > V is the
 *                                        caller's error and is skipped),
 *       1 <= pred[i] <= C               (uint8 class id, what the PNGs hold),
 *       weight == NULL or 0 <= weight[i] <= 65535   (int32),
 *       mesh_depth == NULL, or sensor_depth[i] > 0 and
 *         fabsf(mesh_depth[i] - sensor_depth[i]) <= depth_tol
 *         (fp32 z in scene units, ONE fp32 subtraction; a NaN anywhere fails);
 *     and then votes[vertex_id[i]-1][pred[i]] += weight ? weight[i] : 1.
 *     mesh_depth and sensor_depth come as a pair (both or neither); with them
 *     depth_tol must be >= 0 and not NaN, without them it is ignored.
 *     Sums are uint64 and wrap modulo 2^64; integer adds commute, so the table
 *     does not depend on the order or grouping of pixels or calls: two runs
 *     give the same bytes.  row_width is a scheduling hint only (the arrays
 *     are images of that width, stacked: B*H rows of W; 0 = no structure): a
 *     wave takes a 16x16 pixel tile as four 8x8 patches, adds up its lanes
 *     with an equal (vertex, class) before touching memory and issues one
 *     64-bit integer atomic add per distinct pair; the result is the same for
 *     every row_width.  flags: 0, or UCSA_FUSE_ONE_ATOMIC_PER_PIXEL (the
 *     uncombined form with the same result, kept as the baseline of
 *     tools/label_fusion_time.py).
 *     Limits: 1 <= C <= 255, V*(C+1) <= 2^31-1, N <= 2^31-1,
 *     votes_capacity (uint64 elements) >= V*(C+1), else an argument error and
 *     nothing is written.  V == 0 or N == 0: returns 0, launches nothing.
 *   ucsa_label_fuse_resolve: per vertex v from its row, with s_c = votes[v][c]:
 *     total[v] = sum of s_c over c = 1..C (uint64, wrapping);
 *     winner[v] = max of s_c; label[v] (int32) = the lowest c with
 *     s_c == winner[v] if total[v] >= min_votes, else 0 (winner[v] is the
 *     maximum either way).  min_votes >= 1.  label / total / winner hold
 *     max_vertices >= V elements each; nothing is written past V.  No atomics.
 *     Confidence = winner / total is the caller's, in float64. */
#define UCSA_FUSE_ONE_ATOMIC_PER_PIXEL 1u
int32_t ucsa_label_fuse_accumulate(const int32_t* vertex_id, const uint8_t* pred,
                                   const int32_t* weight, const float* mesh_depth,
                                   const float* sensor_depth, float depth_tol,
                                   uint64_t N, uint32_t row_width, uint32_t V,
                                   uint32_t C, uint64_t* votes,
                                   uint64_t votes_capacity, uint32_t flags,
                                   void* stream);
int32_t ucsa_label_fuse_resolve(const uint64_t* votes, uint32_t V, uint32_t C,
                                uint64_t min_votes, int32_t* label, uint64_t* total,
                                uint64_t* winner, uint64_t max_vertices,
                                void* stream);

/* ---- TSDF fusion: posed depth frames into a dense volume (not in the
 * reference) ---------------------------------------------------------------
 * Projective integration of B depth views into a truncated signed distance
 * volume in the poses' (NGP) frame, scene units (utils/tsdf_fusion.py,
 * scripts/fuse_tsdf_mesh.py); -tsdf at iso 0 with valid = weight > 0 goes to
 * ucsa_mc_count_masked / ucsa_mc_emit_masked.  Lattice as for marching cubes:
 * point (i,j,k) at origin + (i,j,k)*spacing, stored at [(i*ny + j)*nz + k].
 * State, allocated and initialised by the caller, updated in place over calls:
 *   tsdf [nx,ny,nz] fp32 in [-1, 1], units of trunc, initial 1;
 *   weight [nx,ny,nz] fp32, initial 0;
 *   rgb [nx,ny,nz,3] fp32 running average of the colour frames, initial 0, or
 *     NULL; rgb and color come as a pair (both or neither).
 * Inputs: depth [B,H,W] fp32 z-depth in scene units, color [B,H,W,3] uint8,
 * poses [B,4,4] camera-to-world (the poses of ucsa_get_rays), all on the
 * device; origin3 / spacing3 HOST float[3]; fx, fy, cx, cy, trunc, max_weight,
 * depth_min, depth_max HOST scalars.
 * Contract per voxel, for b = 0..B-1 in ascending order (fp32, every operation
 * as written, no contraction, correctly rounded division; a numpy restatement
 * gives the same bits: tests/tsdf_numpy.py).  R = P_b[0:3,0:3], t = P_b[0:3,3]:
 *   p_a = origin_a + (float)index_a * spacing_a;
 *   d = p - t, c_r = (d0*R0r + d1*R1r) + d2*R2r  (the rasterizer's camera point);
 *   skip the view unless c_z > 0 (NaN skips);
 *   u = floor((fx*c_x)/c_z + cx), v = floor((fy*c_y)/c_z + cy): pixel centres at
 *     +0.5 as in ucsa_get_rays / the rasterizer, nearest pixel; skip unless
 *     0 <= u < W and 0 <= v < H (compared in fp32; NaN skips);
 *   z = depth[b][v][u]; skip unless z is finite and depth_min <= z <= depth_max
 *     (with depth_min > 0, 0 means "no measurement" as in the depth PNGs);
 *   sdf = z - c_z; skip if sdf < -trunc; x = min(1, sdf / trunc);
 *   w1 = weight + 1; tsdf = (tsdf*weight + x) / w1;
 *   rgb_c = (rgb_c*weight + (float)color[b][v][u][c]) / w1  for c = 0, 1, 2;
 *   weight = min(w1, max_weight).
 * One thread owns a voxel: no atomics, two runs give the same bytes, and since
 * a voxel's views are applied in order, one call with B views, B calls with one
 * view and every split in between give the same bytes.  The state is read
 * once, carried in registers through up to 32 views per launch and written
 * once (a voxel no view touched is not written); a work-group may skip a view
 * for its whole 1x4x64 brick when the brick's corners prove that every voxel
 * of it would skip that view (an optimisation that changes no bit).
 * Limits: dims >= 2 each, nx*ny*nz <= 2^31-1, nx <= 65535, ny <= 262140 (else
 * the dim's argument), B >= 1, 1 <= H, W <= 16384, fx, fy > 0, trunc > 0,
 * max_weight >= 1, depth_min not NaN, depth_max >= depth_min; an argument error
 * comes before any launch and nothing outside the three volumes is written. */
int32_t ucsa_tsdf_integrate(float* tsdf, float* weight, float* rgb, uint32_t nx,
                            uint32_t ny, uint32_t nz, const float* origin3,
                            const float* spacing3, const float* depth,
                            const uint8_t* color, const float* poses, uint32_t B,
                            float fx, float fy, float cx, float cy, uint32_t H,
                            uint32_t W, float trunc, float max_weight, float depth_min,
                            float depth_max, void* stream);

/* ucsa_tsdf_integrate_weighted: the same integration with a weight per pixel,
 * pixel_weight [B,H,W] fp32 on the device (ucsa_depth_confidence makes one from
 * the depth front end's outputs; any map of finite positive numbers will do).
 * The contract is ucsa_tsdf_integrate's, verbatim, with these lines changed:
 *   z = depth[b][v][u]; skip unless measured (as above);
 *   w = pixel_weight[b][v][u]; skip unless w > 0 and w is finite (NaN skips);
 *   sdf = z - c_z; skip if sdf < -trunc; x = min(1, sdf / trunc);
 *   w1 = weight + w; tsdf = (tsdf*weight + x*w) / w1;
 *   rgb_c = (rgb_c*weight + (float)color[b][v][u][c]*w) / w1  for c = 0, 1, 2;
 *   weight = min(w1, max_weight).
 * tests/weighted_numpy.py restates it and the volumes match it bit for bit.
 * Consequences: pixel_weight == 1.0f everywhere gives ucsa_tsdf_integrate's
 * bytes (x*1.0f and c*1.0f are exact); a view whose weights are all 0 (or
 * negative, NaN, inf) leaves the volume's bytes alone; the updated tsdf lies
 * between the old value and x up to rounding; one call with B views, B calls
 * with one view and every split in between give the same bytes, and so do two
 * runs.  The accumulated weight is in units of pixel weight: a voxel seen once
 * at w = 0.3 holds 0.3, so a consumer's min_weight threshold is in those units
 * too.  One thread owns a voxel, no atomics, the state is read once and
 * written once, a voxel no view touched is not written: the same kernel, the
 * same view loop and the same brick cull, with the weight gathered at the
 * depth's own index (b*H + v)*W + u next to the depth gather.
 * Limits as for ucsa_tsdf_integrate; pixel_weight (argument 9) must not be
 * NULL, and the arguments after it sit one index higher than there: color
 * (10), poses (11), B (12), fx (13), fy (14), cx (15), cy (16), H (17), W (18),
 * trunc (19), max_weight (20), depth_min (21), depth_max (22). */
int32_t ucsa_tsdf_integrate_weighted(float* tsdf, float* weight, float* rgb, uint32_t nx,
                                     uint32_t ny, uint32_t nz, const float* origin3,
                                     const float* spacing3, const float* depth,
                                     const float* pixel_weight, const uint8_t* color,
                                     const float* poses, uint32_t B, float fx, float fy,
                                     float cx, float cy, uint32_t H, uint32_t W, float trunc,
                                     float max_weight, float depth_min, float depth_max,
                                     void* stream);

/* ---- occupancy prior: a TSDF volume carves the marcher's cascade grid (not in
 * the reference; its parent code base had mark_untrained_grid) ---------------
 * ucsa_tsdf_occupancy: the volume (tsdf, weight [nx,ny,nz] fp32, origin3 /
 * spacing3 HOST float[3]: the state and lattice of ucsa_tsdf_integrate) ->
 * mask uint8 [cascade,H,H,H], 1 = the cell may hold matter (keep), 0 = the
 * sensor saw it to be empty, in density_grid's linear layout
 * ((cas*H + ix)*H + iy)*H + iz.  SemanticNeRFRenderer.set_occupancy_prior
 * writes -1 into the 0 cells; ucsa_density_grid_update never touches a negative
 * cell and the marcher's grid > thresh never enters one.
 * Contract (fp32, every operation as written and rounded on its own, no
 * contraction, correctly rounded division; tests/occupancy_numpy.py restates it
 * and the masks match byte for byte).  Per axis a, with n = the dim:
 *   voxel i: centre p(i) = origin_a + (float)i * spacing_a (the lattice point of
 *     ucsa_tsdf_integrate), box [p(i) - h, p(i) + h] with h = 0.5f * spacing_a;
 *   cell j of cascade c: b = min(2^c, bound),
 *     lo = b * ((float)(2j) / (float)H - 1) - dilate,
 *     hi = b * ((float)(2j + 2) / (float)H - 1) + dilate
 *     (the cells of ucsa_density_grid_points and of the marcher's lookup, grown
 *     by dilate on every side);
 *   voxel i meets cell j iff p(i) + h >= lo && p(i) - h <= hi: closed
 *     intervals, the conservative choice.
 * A voxel overlaps a cell iff it meets it on all three axes.  p(i) is
 * non-decreasing in i (spacing > 0; every rounding is monotone), so per axis the
 * overlapping voxels are one index interval and the overlap set is a box; an
 * implementation may find the interval any way it likes but its ends are
 * settled by the predicate above, never by a floor of its own.
 * A voxel is FREE iff weight >= min_weight && tsdf >= free_tsdf (NaN in either:
 * not free).  With free_tsdf = 1 that is "every view that saw it saw it more
 * than trunc in front of its surface": integrate gives such a voxel exactly 1.
 * With unknown_keeps = 0 a voxel with !(weight >= min_weight) is free as well,
 * and so is all space outside the volume.
 * A cell is KEPT (1) iff
 *   some overlapping voxel is not free, or
 *   unknown_keeps != 0 and on some axis lo < p(0) - h or hi > p(n-1) + h (the
 *     dilated cell reaches outside the volume).
 * A pure OR over a box: no order, no atomics, two runs give the same bytes.
 * Two launches whatever the data: the "not free" bits are packed along z into
 * `workspace` (ucsa_tsdf_occupancy_workspace_bytes = 8*nx*ny*ceil(nz/64),
 * checked against workspace_bytes), then one lane per cell walks its box over
 * the packed words (csrc/occupancy_prior.hip states the work per lane).  No
 * host read-back.
 * Limits, ERR_ARG - argument index: tsdf, weight, origin3, spacing3, mask,
 * workspace not NULL; dims >= 1 each (nx*ny*nz <= 2^31-1: argument 2); origin
 * finite; spacing > 0 and finite; min_weight, free_tsdf not NaN; unknown_keeps
 * 0 or 1; bound > 0 and finite; 1 <= cascade <= 31; 2 <= H <= 1024; dilate >= 0
 * and finite; mask_capacity (bytes) >= cascade*H^3.  An argument error comes
 * before any launch; nothing outside mask[0 .. cascade*H^3) and the workspace is
 * written. */
uint64_t ucsa_tsdf_occupancy_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int32_t ucsa_tsdf_occupancy(const float* tsdf, const float* weight, uint32_t nx,
                            uint32_t ny, uint32_t nz, const float* origin3,
                            const float* spacing3, float min_weight, float free_tsdf,
                            uint32_t unknown_keeps, float bound, uint32_t cascade,
                            uint32_t H, float dilate, uint8_t* mask,
                            uint64_t mask_capacity, void* workspace,
                            uint64_t workspace_bytes, void* stream);

/* ---- mesh voxelization: the cells a triangle mesh passes through (not in the
 * reference) ------------------------------------------------------------------
 * ucsa_mesh_voxelize_count / ucsa_mesh_voxelize_fill: verts [V,3] fp32, faces
 * [F,3] int32 (device) -> mask uint8, 1 = some face meets the cell's box.  Two
 * families of axis-aligned boxes (fp32, every operation as written and rounded
 * on its own, no contraction, correctly rounded division, as for
 * ucsa_tsdf_occupancy; tests/voxelize_numpy.py restates all of it and the masks
 * match byte for byte):
 *   UCSA_VOXELIZE_LATTICE  the voxels of a tsdf_volume: nx, ny, nz, origin3 /
 *     spacing3 HOST float[3]; voxel i on axis a has
 *       p = origin_a + (float)i * spacing_a, h = 0.5f * spacing_a,
 *       lo = (p - h) - dilate, hi = (p + h) + dilate;
 *     mask [nx,ny,nz], linear (ix*ny + iy)*nz + iz; cascade must be 1, bound is
 *     ignored.
 *   UCSA_VOXELIZE_CASCADE  the marcher's cells: nx = ny = nz = H; cell j of
 *     cascade c has, with b = min(2^c, bound),
 *       lo = b * ((float)(2j) / (float)H - 1) - dilate,
 *       hi = b * ((float)(2j + 2) / (float)H - 1) + dilate
 *     (ucsa_tsdf_occupancy's formulas); mask [cascade,H,H,H] in density_grid's
 *     layout ((c*H + ix)*H + iy)*H + iz; origin3 / spacing3 are ignored.
 * meets(face, box), csrc/tri_box.h: the separating-axis test of a triangle
 * against a box on 13 axes, closed, with a rounding slack.  Corners p0, p1, p2
 * (the rows faces[f][0..2] of verts), per face and call:
 *   S = the largest of |p_j.a| (9 numbers) and Bmax, the family's largest
 *     absolute box bound: cascade min(2^(cascade-1), bound) + dilate; lattice
 *     the largest of |lo(0)|, |hi(n-1)| over the three axes;
 *   slack = 2^-20 * S  (K * 2^-24 with K = 16; docs/DESIGN_NOTEBOOK.md, VX);
 *   mn_a / mx_a = the smallest / largest of p0.a, p1.a, p2.a;
 *   e_0 = p1 - p0, e_1 = p2 - p1, e_2 = p0 - p2 (per component);
 *   n_a = e_0.b * e_1.c - e_0.c * e_1.b, where (a, b, c) runs over (x, y, z),
 *     (y, z, x), (z, x, y) here and below.
 * Per box [lo, hi]:
 *   box axes (3): mn_a <= hi_a + slack && mx_a >= lo_a - slack;
 *   c_a = 0.5f * (lo_a + hi_a), g_a = 0.5f * (hi_a - lo_a) + slack,
 *   v_j.a = p_j.a - c_a;
 *   unit_a x e_i (9): q_j = e_i.b * v_j.c - e_i.c * v_j.b  for j = 0, 1, 2,
 *     r = g_b * |e_i.c| + g_c * |e_i.b|;
 *     the axis separates iff min(q_0, q_1, q_2) > r or max(q_0, q_1, q_2) < -r;
 *   the normal (1): d_j = (n_x * v_j.x + n_y * v_j.y) + n_z * v_j.z,
 *     r = (|n_x| * g_x + |n_y| * g_y) + |n_z| * g_z;
 *     separates iff min(d_0, d_1, d_2) > r or max(d_0, d_1, d_2) < -r.  In exact
 *     arithmetic the three d_j are equal and this is |n . v_0| <= |n| . g; in
 *     fp32 they are not, and for a thin triangle they differ by more than the
 *     slack covers, so all three are asked: whatever n came out as, it is an
 *     axis, and an axis on which the projections overlap cannot lose a pair.
 *   meets iff the three box axes hold and none of the ten separates.
 * A face with an index outside [0, V) or a corner that is not finite or larger
 * in magnitude than 2^40 (beyond it the products could overflow) meets nothing;
 * the kernels test every index before use and are memory-safe on any faces.  A
 * face of zero area (a segment, a point) takes the same test: n = 0 makes the
 * normal axis pass and the other twelve decide.
 * The guarantee, in exact arithmetic on the same fp32 inputs: a face and a box
 * that intersect meet (never a touching pair lost: proven for every face, K >=
 * 14 suffices), and a face that meets a box intersects that box grown by
 * 2 * slack on every side (proven for the twelve box and cross axes; on the
 * normal axis the rounded n tilts the plane, to first order by at most
 * 24 * 2^-24 * L^2 / w at the far end of a face of longest edge L and width w,
 * which 2 * slack covers for faces that are small beside the scene and not
 * slivers; no pair outside the grown box was found among thousands built to
 * graze, thin and scene-sized faces included).
 * slack does not depend on the cell and lo, hi are non-decreasing in the cell
 * index, so the box-axis test is monotone: per axis the cells that pass are one
 * index interval.  An implementation may find it any way it likes but its ends
 * are settled by the predicate above, never by a floor of its own, and it may
 * skip a cell only where it can prove the predicate false.
 * Result: mask[cell] = 1 iff some face meets the cell's box, else 0: a pure OR,
 * stored as the constant 1 by plain byte stores, so no atomics, any face order
 * and two runs give the same bytes.  With accumulate = 1 the mask is not
 * cleared first: met cells are set to 1 and every other byte is left alone, so
 * calls over any split of the face list give the bytes of one call.
 * Two entries with the caller's prefix sum between them:
 *   count: per item k = f * cascade + c the number count[k] (int32 [F*cascade])
 *     of (x, y) columns of the index box of face f in cascade c, 0 when the
 *     face meets nothing or an interval is empty; the index boxes go to
 *     `workspace` (ucsa_mesh_voxelize_workspace_bytes = 24 * F * cascade);
 *   the caller: first int64 [F*cascade + 1] = the exclusive prefix sum of count,
 *     total = first[F*cascade], read back once;
 *   fill: clears the mask (unless accumulate), then one lane per column walks
 *     the column's z-run (csrc/mesh_voxelize.hip states the work per lane).
 *     It takes the geometry arguments of the count call and its workspace.
 * Neither entry allocates or reads anything back.
 * Limits, ERR_ARG - argument index: verts / faces not NULL unless F = 0 (verts
 * also when V = 0); V, F <= 2^31-1 and F * cascade <= 2^31-1 (argument 3);
 * family 0 or 1; lattice: dims >= 1 each, nx*ny*nz <= 2^31-1 (argument 5),
 * origin3 / spacing3 not NULL, origin finite with Bmax <= 2^40, spacing > 0 and
 * finite, cascade = 1; cascade family: 2 <= nx <= 1024, ny = nz = nx, bound > 0
 * and finite, 1 <= cascade <= 31; 0 <= dilate <= 2^40; count, mask, first,
 * workspace not NULL when there is an item / a column; total <= 2^38, and 0
 * when F = 0; accumulate 0 or 1; mask_capacity (bytes) >= cascade*nx*ny*nz;
 * workspace_bytes as above.  An argument error comes before any launch;
 * nothing outside mask[0 .. cascade*nx*ny*nz), count and the workspace is
 * written. */
#define UCSA_VOXELIZE_LATTICE 0u
#define UCSA_VOXELIZE_CASCADE 1u
uint64_t ucsa_mesh_voxelize_workspace_bytes(uint32_t nf, uint32_t cascade);
int32_t ucsa_mesh_voxelize_count(const float* verts, uint32_t nv, const int32_t* faces,
                                 uint32_t nf, uint32_t family, uint32_t nx, uint32_t ny,
                                 uint32_t nz, const float* origin3, const float* spacing3,
                                 float bound, uint32_t cascade, float dilate, int32_t* count,
                                 void* workspace, uint64_t workspace_bytes, void* stream);
int32_t ucsa_mesh_voxelize_fill(const float* verts, uint32_t nv, const int32_t* faces,
                                uint32_t nf, uint32_t family, uint32_t nx, uint32_t ny,
                                uint32_t nz, const float* origin3, const float* spacing3,
                                float bound, uint32_t cascade, float dilate,
                                const int64_t* first, uint64_t total, uint32_t accumulate,
                                uint8_t* mask, uint64_t mask_capacity, const void* workspace,
                                uint64_t workspace_bytes, void* stream);

/* ---- voxel map: per-voxel class votes and a ray-caster over the TSDF volume
 * (not in the reference) ----------------------------------------------------
 * The voxel route of the mapping baseline (utils/voxel_map.py,
 * scripts/voxel_map_labels.py): label maps vote into the voxels of the band
 * around the measured surface while depth is integrated, the votes resolve to
 * one label per voxel, and the volume is ray-cast into any camera view.  No
 * mesh, no vertex-id render, no 64-bit table.  tests/voxel_map_numpy.py
 * restates the three contracts; the outputs match it bit for bit.
 *
 * ucsa_tsdf_vote: B views vote into votes [C+1][nx][ny][nz] uint16, allocated
 *   AND zeroed by the caller, accumulated over calls; plane 0 is never written
 *   (plane = class id).  Class-major: the 64 voxels of a wave are consecutive
 *   in k and mostly vote for one class, so their read-modify-write is one
 *   coalesced line per plane.  Lattice, depth, poses, intrinsics as for
 *   ucsa_tsdf_integrate; pred [B,H,W] uint8 class ids.
 *   Per voxel, for b = 0..B-1: the projection and the skip tests of
 *   ucsa_tsdf_integrate verbatim (camera point, c_z > 0, floor to the nearest
 *   pixel, bounds, z finite and depth_min <= z <= depth_max, sdf = z - c_z);
 *   the voxel votes iff -trunc <= sdf <= trunc (the band only, not the free
 *   space in front) and 1 <= pred[b][v][u] <= C, and then
 *   votes[pred][voxel] = min(votes[pred][voxel] + 1, 65535).
 *   The votes do not depend on the TSDF state.  One thread owns a voxel: no
 *   atomics; a saturating add of ones commutes, so every split and every order
 *   of the views over calls gives the same bytes, and so do two runs.  Within a
 *   launch (up to 32 views) a thread keeps a pending (class, count) in
 *   registers and flushes it when the class changes; a work-group skips a view
 *   for its whole 1x4x64 brick by ucsa_tsdf_integrate's corner test.  Neither
 *   changes a bit.
 *   Limits as for ucsa_tsdf_integrate (dims: argument 3..5 here), 1 <= C <= 255
 *   (argument 2), (C+1)*nx*ny*nz <= 2^40 and votes_capacity (uint16 elements)
 *   >= that (argument 1); an argument error comes before any launch and
 *   nothing is written.
 * ucsa_voxel_label_resolve: per voxel x of n_voxels, s_c = votes[c][x]:
 *   total[x] = sum of s_c over c = 1..C (uint32), winner[x] = max of s_c,
 *   label[x] (uint8) = the lowest c with s_c == winner[x] if total[x] >=
 *   min_votes, else 0 (ucsa_label_fuse_resolve's rule).  min_votes >= 1.  The
 *   planes are read one after the other, coalesced; no atomics.  label / total
 *   / winner hold max_voxels >= n_voxels elements each.
 * ucsa_tsdf_raycast: the volume (tsdf, weight, rgb or NULL: the state of
 *   ucsa_tsdf_integrate) seen from B posed pinhole cameras.  Outputs, one
 *   element per pixel, capacity max_pixels >= B*H*W each:
 *     depth [B,H,W] fp32: z-depth of the hit in scene units (the rasterizer's
 *       depth, the depth PNGs), 0 on a miss;
 *     voxel_id [B,H,W] int32: (i*ny + j)*nz + k of the lattice point nearest to
 *       the hit, -1 on a miss;
 *     normal [B,H,W,3] fp32 or NULL: world frame, toward free space;
 *     rgb_out [B,H,W,3] fp32, iff rgb is given (both or neither);
 *     label [B,H,W] int32 = voxel_labels[voxel_id] (voxel_labels [nx,ny,nz]
 *       uint8), iff voxel_labels is given (both or neither); 0 on a miss.
 *   Contract (fp32, every operation as written, no contraction, correctly
 *   rounded division and sqrt).  R = P[0:3,0:3], t = P[0:3,3], top_a = n_a - 1:
 *   ray of pixel (x, y): d = ((x+0.5-cx)/fx, (y+0.5-cy)/fy, 1) (k_get_rays'
 *     order); world direction w_a = (R_a0*d0 + R_a1*d1) + R_a2, NOT normalised:
 *     the ray parameter is camera z and the hit parameter is the depth itself;
 *   lattice coordinates: q0_a = (t_a - origin_a)/spacing_a, qd_a = w_a/spacing_a,
 *     g_a(z) = q0_a + z*qd_a;
 *   interval: z_in = near, z_out = far, then per axis a = 0, 1, 2: with
 *     qd_a == 0 the ray misses unless 0 <= q0_a <= top_a; otherwise
 *     z1 = (0 - q0_a)/qd_a, z2 = (top_a - q0_a)/qd_a, lo = min, hi = max,
 *     z_in = lo > z_in ? lo : z_in, z_out = hi < z_out ? hi : z_out.  A miss
 *     unless z_in <= z_out and q0, qd, z_in, z_out are all finite;
 *   samples: dz = step / sqrt((d0*d0 + d1*d1) + 1), z_k = z_in + (float)k*dz
 *     for k = 0, 1, ... while z_k <= z_out and k < 2^20 (indexed, not
 *     accumulated: an implementation may skip indices);
 *   cell of a sample at z: per axis c_a = min(max(floor(g_a), 0), n_a - 2),
 *     fraction f_a = min(max(g_a - (float)c_a, 0), 1); corners v_{ijk} at
 *     (c_0+i, c_1+j, c_2+k); the sample is valid iff all eight corners have
 *     weight >= min_weight (the cell rule of ucsa_mc_*_masked);
 *   value, seven lerps l(a, b, f) = a + f*(b - a): along k first,
 *     c_ij = l(v_ij0, v_ij1, f_2); then along j, c_i = l(c_i0, c_i1, f_1); then
 *     f = l(c_0, c_1, f_0);
 *   hit: the first k with z_{k+1} <= z_out, both samples valid, f_k > 0,
 *     f_{k+1} <= 0 and, with z = z_k + dz*(f_k / (f_k - f_{k+1})) clamped into
 *     [z_k, z_{k+1}], the cell of z valid too (the crossing can lie in a third
 *     cell; with an unobserved corner there the masked mesh has no face, the
 *     march goes on, and no output is interpolated from an unobserved voxel).
 *     No other stop rule: a surface within one step of the box's far side can
 *     be stepped over (pad the volume by trunc, or shorten the step);
 *   at g(z) of the hit, in its cell with its fractions: gradient
 *     G_0 = c_1 - c_0, G_1 = l(c_01 - c_00, c_11 - c_10, f_0),
 *     G_2 = l(l(e_00, e_01, f_1), l(e_10, e_11, f_1), f_0) with
 *     e_ij = v_ij1 - v_ij0; n_a = G_a/spacing_a, normal = n / sqrt((n_0*n_0 +
 *     n_1*n_1) + n_2*n_2), (0,0,0) when that length is zero or non-finite;
 *     rgb_out: the seven lerps of rgb per channel; voxel_id from
 *     min(max(rint(g_a), 0), top_a) per axis (round half to even).
 *   One thread per pixel, a wave per 8x8 pixel patch (its rays stay in
 *   neighbouring cells); no atomics: two runs give the same bytes.
 *   Empty-space skipping (the default): a crossing needs f_{k+1} <= 0, a
 *   clamped-fraction lerp of eight valid corners, so one of them is <= 2^-16
 *   (the margin covers the rounding of the seven lerps of values in [-1, 1]).
 *   A pre-pass marks the 8x8x8-cell bricks that hold such a cell into
 *   `workspace` (ucsa_tsdf_raycast_workspace_bytes, checked against
 *   workspace_bytes), and index k is evaluated only if the cell of sample k or
 *   of sample k+1 lies in a marked brick.  The bytes are those of the plain
 *   march, flags = UCSA_RAYCAST_PLAIN_MARCH, which needs no workspace and is
 *   kept as the baseline of tools/voxel_map_time.py.
 *   Limits: dims >= 2 each, nx*ny*nz <= 2^31-1, spacing finite and non-zero,
 *   1 <= B <= 65535, 1 <= H, W <= 16384, fx, fy > 0, near > 0, far >= near,
 *   trunc > 0, 0 < step < trunc (the truncation distance the volume was
 *   integrated with: a longer step can jump the band), min_weight > 0; an
 *   argument error comes before any launch and nothing is written. */
#define UCSA_RAYCAST_PLAIN_MARCH 1u
int32_t ucsa_tsdf_vote(uint16_t* votes, uint64_t votes_capacity, uint32_t C,
                       uint32_t nx, uint32_t ny, uint32_t nz, const float* origin3,
                       const float* spacing3, const float* depth, const uint8_t* pred,
                       const float* poses, uint32_t B, float fx, float fy, float cx,
                       float cy, uint32_t H, uint32_t W, float trunc, float depth_min,
                       float depth_max, void* stream);
int32_t ucsa_voxel_label_resolve(const uint16_t* votes, uint32_t C, uint64_t n_voxels,
                                 uint32_t min_votes, uint8_t* label, uint32_t* total,
                                 uint32_t* winner, uint64_t max_voxels, void* stream);
uint64_t ucsa_tsdf_raycast_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int32_t ucsa_tsdf_raycast(const float* tsdf, const float* weight, const float* rgb,
                          const uint8_t* voxel_labels, uint32_t nx, uint32_t ny,
                          uint32_t nz, const float* origin3, const float* spacing3,
                          const float* poses, uint32_t B, float fx, float fy, float cx,
                          float cy, uint32_t H, uint32_t W, float near, float far,
                          float trunc, float step, float min_weight, float* depth,
                          int32_t* voxel_id, float* normal, float* rgb_out,
                          int32_t* label, uint64_t max_pixels, void* workspace,
                          uint64_t workspace_bytes, uint32_t flags, void* stream);

/* ---- soft label fusion: per-class evidence sums (not in the reference) -----
 * The soft sibling of the two hard-vote paths above.  A pixel's belief is a row
 * of C uint8 evidence codes, e_c = 255 - rint(255 * min(-ln p_c, 8) / 8)
 * (ops.log_evidence: p = 1 gives 255, p <= e^-8 gives 0); a sum of codes over
 * views is the clamped log-likelihood sum, scaled by 255/8 and shifted by a
 * constant, and its argmax is the MAP class under independent views and a
 * uniform prior.  An ALL-ZERO row means "this pixel abstains" (no softmax over
 * C <= 255 classes produces one).  scores is pixel-major, [B,H,W,C] uint8: the
 * C codes of a pixel are C consecutive bytes at scores + pixel*C, at any
 * alignment.  Everything is integer adds; tests/evidence_numpy.py restates the
 * three contracts and the outputs match it bit for bit.
 *
 * ucsa_tsdf_evidence: B views add into evidence [C+1][nx][ny][nz] uint32,
 *   class-major, allocated AND zeroed by the caller, accumulated over calls.
 *   Plane c (1..C) is the evidence sum of class c, plane 0 the number of
 *   (view, voxel) contributions.  Lattice, depth, poses, intrinsics as for
 *   ucsa_tsdf_integrate.  Per voxel, for b = 0..B-1: the pixel and the band of
 *   ucsa_tsdf_vote verbatim (the projection of ucsa_tsdf_integrate, z finite
 *   and depth_min <= z <= depth_max, -trunc <= z - c_z <= trunc); the voxel
 *   takes the row of that pixel iff the row is not all zero, and then
 *     evidence[c][voxel] = min(evidence[c][voxel] + row[c-1], 2^32-1), c = 1..C,
 *     evidence[0][voxel] = min(evidence[0][voxel] + 1, 2^32-1).
 *   Independent of the TSDF state.  One thread owns a voxel: no atomics;
 *   saturating adds of non-negative numbers commute, so every split and every
 *   order of the views over calls gives the same bytes, and so do two runs.
 *   Within a launch (up to 32 views) a thread carries its running sums in
 *   registers, 40 classes at a time (8 when C <= 8; for C > 40 the views are
 *   walked once per group of 40 classes), and reads and writes its C+1 table
 *   entries once, and only if a view of the launch contributed: a voxel that no
 *   view of the call reaches in its band is neither read nor written, so a call
 *   costs the band, not the volume.  A work-group skips a view for its whole
 *   1x4x64 brick by ucsa_tsdf_integrate's corner test.  A row is fetched as the
 *   aligned 32-bit words that hold a byte of it (never a word wholly outside
 *   the row).
 *   Limits as for ucsa_tsdf_vote: dims (arguments 3..5), 1 <= C <= 255
 *   (argument 2), (C+1)*nx*ny*nz <= 2^40 and evidence_capacity (uint32
 *   elements) >= that (argument 1), B*H*W*C <= 2^40 (argument 9); an argument
 *   error comes before any launch and nothing is written.
 * ucsa_voxel_evidence_resolve: per voxel x of n_voxels, s_c = evidence[c][x]:
 *   views[x] = evidence[0][x]; best[x] = max of s_c over c = 1..C; margin[x] =
 *   best[x] minus the largest s_c over the other classes (the runner-up; for
 *   C = 1 margin = best); label[x] (uint8) = the lowest c with s_c == best[x]
 *   if views[x] >= min_views and margin[x] >= min_margin, else 0.
 *   min_views >= 1.  label feeds ucsa_tsdf_raycast's voxel_labels.  The planes
 *   are read one after the other, coalesced; no atomics.  The four outputs hold
 *   max_voxels >= n_voxels elements each.
 * ucsa_label_fuse_evidence: N pixels add into votes [V][C+1] uint64, the table
 *   of ucsa_label_fuse_accumulate (column 0 is never touched).  Pixel i adds
 *   iff 1 <= vertex_id[i] <= V and it passes the optional depth gate of
 *   ucsa_label_fuse_accumulate (same rule, same arguments), and then
 *     votes[vertex_id[i]-1][c] += scores[i*C + c-1]   for c = 1..C
 *   (an all-zero row adds nothing: it abstains).  ucsa_label_fuse_resolve reads
 *   the table as it is; min_votes is then in evidence units.  Sums are uint64,
 *   integer adds commute: the table does not depend on the order or grouping of
 *   pixels or calls.  row_width is the scheduling hint of
 *   ucsa_label_fuse_accumulate: a wave takes a 16x16 pixel tile as four 8x8
 *   patches and, per distinct vertex of the tile, walks the pixels that hold it
 *   with lane l summing classes l+1, l+65, ... (one coalesced read of the row
 *   per pixel), then issues ONE 64-bit integer atomic add per class with a
 *   non-zero sum: a wave wholly on one wall issues C atomics, not 256*C.
 *   Limits: those of ucsa_label_fuse_accumulate; an argument error comes before
 *   any launch.  V == 0 or N == 0: returns 0, launches nothing. */
int32_t ucsa_tsdf_evidence(uint32_t* evidence, uint64_t evidence_capacity, uint32_t C,
                           uint32_t nx, uint32_t ny, uint32_t nz, const float* origin3,
                           const float* spacing3, const float* depth,
                           const uint8_t* scores, const float* poses, uint32_t B, float fx,
                           float fy, float cx, float cy, uint32_t H, uint32_t W,
                           float trunc, float depth_min, float depth_max, void* stream);
int32_t ucsa_voxel_evidence_resolve(const uint32_t* evidence, uint32_t C,
                                    uint64_t n_voxels, uint32_t min_views,
                                    uint32_t min_margin, uint8_t* label, uint32_t* views,
                                    uint32_t* best, uint32_t* margin, uint64_t max_voxels,
                                    void* stream);
int32_t ucsa_label_fuse_evidence(const int32_t* vertex_id, const uint8_t* scores,
                                 const float* mesh_depth, const float* sensor_depth,
                                 float depth_tol, uint64_t N, uint32_t row_width,
                                 uint32_t V, uint32_t C, uint64_t* votes,
                                 uint64_t votes_capacity, void* stream);

/* ---- neighbourhood pooling of fused label tables (not in the reference) ----
 * Every voxel and every vertex of the tables above decides on its own.  These
 * two entries pool a table over the immediate neighbourhood, in integers, into
 * a NEW table of the same layout that the resolve entries read as it is (their
 * thresholds then count pooled units: up to centre + 26 times what one voxel
 * held).  The input is never modified.  tests/smooth_numpy.py restates both
 * contracts; the outputs match it bit for bit.
 *
 * ucsa_voxel_table_smooth: in / out are tables [C+1][nx][ny][nz], class-major,
 *   of elem_bytes = 4 (uint32: ucsa_tsdf_evidence) or 2 (uint16:
 *   ucsa_tsdf_vote) per element; weight [nx][ny][nz] fp32 is the volume's.
 *   obs(v) = weight[v] >= min_weight (an fp32 compare, the ray-caster's cell
 *   rule; a NaN weight is not observed).  For a voxel v with obs(v) and every
 *   plane p = 0..C, plane 0 included:
 *     out[p][v] = min(SAT, centre * in[p][v] + sum of in[p][n] over n in N(v)),
 *   N(v) = the 6 face neighbours (neighbourhood = 6) or the 26 other voxels of
 *   the 3x3x3 cube around v (neighbourhood = 26) that lie inside the lattice
 *   AND have obs(n); SAT = 2^32-1 or 65535; the sum is exact (it cannot exceed
 *   281 * SAT).  For a voxel without obs(v), out[p][v] = in[p][v]: evidence
 *   neither crosses into an unobserved voxel nor comes out of one.  Plane 0 of
 *   an evidence table becomes a pooled contribution count.  k calls, each
 *   reading the previous call's output, are k iterations.
 *   One launch for all planes: a work-group owns a tile of 4 x 4 x 64 voxels,
 *   the gate is folded into a 27-bit mask per thread once and reused for every
 *   plane, and each plane's tile with its one-voxel halo goes through LDS; a
 *   halo cell outside the lattice is not loaded (nothing outside in, out and
 *   weight is touched).  A tile without an observed voxel is copied.  No
 *   atomics: two runs give the same bytes.
 *   Limits: elem_bytes 2 or 4 (argument 2), 1 <= C <= 255 and
 *   (C+1)*nx*ny*nz <= 2^40 (argument 3), dims >= 2 each, nx*ny*nz <= 2^31-1,
 *   nx, ny <= 262140 (arguments 4..6), min_weight not NaN (argument 8),
 *   neighbourhood 6 or 26 (argument 9), 1 <= centre <= 255 (argument 10); out
 *   must not overlap in or weight, in == out included (argument 1).  An
 *   argument error comes before any launch and nothing is written.
 * ucsa_label_table_smooth: in / out are tables [V][C+1] uint64 (the table of
 *   ucsa_label_fuse_accumulate / ucsa_label_fuse_evidence); the mesh's edges
 *   come as compressed rows: the neighbours of vertex v are
 *   neighbours[offsets[v] .. offsets[v+1]), offsets int32 [V+1], neighbours
 *   int32 [E] (ops.mesh_adjacency: each undirected edge once per direction, no
 *   self edges, no duplicates).  For every vertex v and column c = 0..C:
 *     out[v][c] = centre * in[v][c] + sum of in[n][c] over n in the list of v,
 *   modulo 2^64 (the table's own adds wrap); a vertex with an empty list gets
 *   centre * in[v].  A list entry outside 0..V-1 is the caller's error and is
 *   skipped, and offsets are clamped into [0, E]: a malformed list reads
 *   nothing outside the arrays.  The columns go across the lanes of a group of
 *   G lanes per vertex (G = the power of two >= min(C+1, 64)), which walks the
 *   list with one coalesced row read per neighbour and one store per element.
 *   No atomics.
 *   Limits: 1 <= C <= 255 (argument 3), V*(C+1) <= 2^31-1 (argument 2),
 *   E <= 2^31-1 (argument 6), 1 <= centre <= 255 (argument 7); out must not
 *   overlap in, offsets or neighbours (argument 1).  V == 0: returns 0,
 *   launches nothing. */
int32_t ucsa_voxel_table_smooth(const void* in, void* out, uint32_t elem_bytes, uint32_t C,
                                uint32_t nx, uint32_t ny, uint32_t nz, const float* weight,
                                float min_weight, uint32_t neighbourhood, uint32_t centre,
                                void* stream);
int32_t ucsa_label_table_smooth(const uint64_t* in, uint64_t* out, uint32_t V, uint32_t C,
                                const int32_t* offsets, const int32_t* neighbours, uint64_t E,
                                uint32_t centre, void* stream);

/* ---- connected components (not in the reference) ----
 * Which pieces of a map hang together: of a voxel mask, of a mesh's vertex
 * graph, and how large each piece is.  A label is the smallest index of its
 * component, which is unique whatever the schedule does, and the counts are
 * integer adds: tests/components_numpy.py restates the three contracts and the
 * outputs match it byte for byte; two runs give the same bytes.  The inputs are
 * never modified.  Union-find in the output array itself (parent[x] <= x at
 * every instant, so every walk strictly descends; the larger root is hooked
 * under the smaller with a 32-bit integer atomic min; a last launch makes every
 * element point at its root): a fixed number of launches per call, no host
 * read-back, and no loop whose exit waits for another wave.
 *
 * ucsa_voxel_components: mask [nx][ny][nz] uint8, labels [nx][ny][nz] int32.
 *   Two voxels with mask != 0 are neighbours if they differ by one step along
 *   one axis (connectivity = 6) or lie in each other's 3x3x3 cube (connectivity
 *   = 26, the neighbourhoods of ucsa_voxel_table_smooth).  labels[v] = the
 *   smallest linear index (i*ny + j)*nz + k over the component of v if
 *   mask[v] != 0, else -1.  Three launches: a work-group labels its tile of
 *   4 x 4 x 64 voxels in LDS (each voxel hooks to the earlier half of its
 *   neighbourhood, 3 of 6 or 13 of 26) and writes the tile's roots as global
 *   indices; unions across tile faces, edges and corners with global atomics;
 *   flatten.  Nothing outside mask and labels is touched.
 *   Limits: dims >= 1 each, nx*ny*nz <= 2^31-1, nx, ny <= 262140 (arguments
 *   2..4), connectivity 6 or 26 (argument 5); labels must not overlap mask
 *   (argument 1).  An argument error comes before any launch and nothing is
 *   written.
 * ucsa_graph_components: the graph comes as the compressed rows of
 *   ucsa_label_table_smooth (ops.mesh_adjacency): offsets int32 [V+1],
 *   neighbours int32 [E], each undirected edge once per direction (what counts
 *   is that every edge is listed in the row of its larger end).  labels[v]
 *   (int32 [V]) = the smallest vertex index of v's component; an isolated
 *   vertex gets v.  A lane per vertex hooks over its neighbours n < v; a row of
 *   more than 64 entries is walked by the whole wave, 64 entries at a time.  A
 *   list entry outside 0..V-1 is skipped and offsets are clamped into [0, E]: a
 *   malformed list reads nothing outside the arrays.
 *   Limits: V <= 2^31-1 (argument 2), E <= 2^31-1 (argument 3); labels must not
 *   overlap offsets or neighbours (argument 4).  V == 0: returns 0, launches
 *   nothing; E == 0: labels[v] = v.
 * ucsa_component_sizes: labels, sizes, scratch int32 [n] each.  sizes[x] = the
 *   number of elements y with labels[y] == labels[x] if 0 <= labels[x] < n,
 *   else 0 (the -1 of an unset voxel).  scratch is zeroed, every element adds 1
 *   to scratch[labels[x]] with 32-bit integer atomics -- the lanes of a wave
 *   that share a label are counted first and add once -- and sizes gathers.
 *   scratch holds the count of label r at r afterwards.
 *   Limits: n <= 2^31-1 (argument 3); the three arrays must not overlap
 *   (arguments 1, 2).  n == 0: returns 0, launches nothing. */
int32_t ucsa_voxel_components(const uint8_t* mask, int32_t* labels, uint32_t nx, uint32_t ny,
                              uint32_t nz, uint32_t connectivity, void* stream);
int32_t ucsa_graph_components(const int32_t* offsets, const int32_t* neighbours, uint32_t V,
                              uint64_t E, int32_t* labels, void* stream);
int32_t ucsa_component_sizes(const int32_t* labels, int32_t* sizes, int32_t* scratch,
                             uint64_t n, void* stream);

/* ---- nearest point within a radius (not in the reference) ----
 * For each query the nearest of n points within max_dist: what carries labels
 * from one mesh to another and what accuracy, completeness and F-score of a
 * mesh are made of.  tests/nearest_numpy.py states the contract as plain brute
 * force and the outputs match it byte for byte:
 *   every operation is rounded to float32 and nothing is fused; per pair
 *   dx = q.x - p.x (dy, dz likewise), d2 = (dx*dx + dy*dy) + dz*dz; point j
 *   matches query i iff d2 <= max_dist*max_dist (inclusive; a NaN compares
 *   false, so a non-finite point never matches and a non-finite query matches
 *   nothing); index[i] = the matching j with the smallest d2, among equal d2 the
 *   smallest j; dist2[i] = that d2; no match: index[i] = -1, dist2[i] = +inf.
 * The result therefore does not depend on the cell size, on the grid's origin
 * or on the order in which queries are processed.  The grid is cells of edge
 * `cell` from `origin`, dims[0] x dims[1] x dims[2] of them, linear index
 * (x*dims[1] + y)*dims[2] + z; origin[3] and dims[3] are host arrays.
 *
 * ucsa_point_cell_keys: points [n][3] float32 -> keys [n] int32.  The cell
 *   coordinate is floor((p - origin) / cell) per axis (float32, the division
 *   correctly rounded), clamped into the grid as a float before it becomes an
 *   integer.  clamp = 1 (the points): a finite point outside the box gets its
 *   border cell, a non-finite point the key dims[0]*dims[1]*dims[2], which sorts
 *   last and is never visited.  clamp = 0 (a sort key for queries): a point
 *   outside the grid gets that last key as well.
 *   A stable sort of the keys gives `order`; offsets [cells + 1] int32 is the
 *   position of each cell's first point in that order (offsets[cells] = the
 *   number of finite points); sorted_points [n][4] float32 holds x, y, z of
 *   point order[k] and, in w, the bits of the int32 order[k] (ops.point_grid
 *   builds the three in torch).
 * ucsa_nearest_point: one lane per query; lane t takes query q_order[t]
 *   (int32 [nq], a permutation; NULL: query t) and writes that query's slots of
 *   index [nq] int32 and dist2 [nq] float32.  The lane walks Chebyshev rings of
 *   cells around the query's clamped cell; a run of cells along z costs two
 *   offset reads.  After each ring every slab of unvisited cells whose near
 *   wall is farther than min(best d2, max_dist^2) is cut off, strictly and with
 *   a margin: the gap to the wall is shortened by 2^-20 * (|origin| + |origin +
 *   dims*cell| + |q|) on that axis and its square must exceed the bound times
 *   1 + 2^-20, which covers the rounding of the cell assignment, of the wall
 *   and of d2, and keeps ties (an unvisited point's d2 is strictly larger).  The
 *   walk ends when no slab is left; every loop is bounded by dims; offsets are
 *   clamped into [0, n].  No atomics, no LDS, no lane waits for another.  A
 *   query farther than max_dist from the box [origin, origin + dims*cell]
 *   writes -1 without a ring: points are expected inside that box (as
 *   ops.point_grid makes it); a point outside it sits in a border cell and is
 *   still found by every query within max_dist of the box.
 *   Cost: a query with nothing within max_dist walks every cell within
 *   max_dist; max_dist = the scene's diagonal costs what brute force costs.
 *   Limits (both entry points): origin finite, cell > 0 and finite with a finite
 *   far corner, dims >= 1 each with at most 2^24 cells, n and nq <= 2^31-1,
 *   max_dist > 0 with a finite float32 square, sorted_points 16-byte aligned; an
 *   argument error comes before any launch and nothing is written.  n == 0:
 *   every query gets -1 (sorted_points and offsets may be NULL); nq == 0:
 *   returns 0, launches nothing. */
int32_t ucsa_point_cell_keys(const float* points, uint32_t n, const float* origin, float cell,
                             const uint32_t* dims, uint32_t clamp, int32_t* keys, void* stream);
int32_t ucsa_nearest_point(const float* sorted_points, const int32_t* offsets, uint32_t n,
                           const float* origin, float cell, const uint32_t* dims,
                           const float* queries, const int32_t* q_order, uint32_t nq,
                           float max_dist, int32_t* index, float* dist2, void* stream);

/* ---- nearest point on a triangle mesh within a radius (not in the reference) ----
 * For each query the nearest point of the surface of nf triangles within
 * max_dist: what the 3D scores use when the target mesh is tessellated more
 * coarsely than the queries.  tests/surface_numpy.py states the contract as
 * plain brute force over all faces and the outputs match it byte for byte:
 *   every operation is rounded to float32 and nothing is fused; with
 *   dot(x,y) = (x0*y0 + x1*y1) + x2*y2 and, per (query q, face A B C),
 *     a = A - q; b = B - q; c = C - q; ab = b - a; ac = c - a
 *     d1 = dot(ab,-a); d2 = dot(ac,-a); d3 = dot(ab,-b); d4 = dot(ac,-b);
 *     d5 = dot(ab,-c); d6 = dot(ac,-c)
 *     vc = d1*d4 - d3*d2; vb = d5*d2 - d1*d6; va = d3*d6 - d5*d4
 *   the first that holds decides (v, w):
 *     d1 <= 0 and d2 <= 0                    (0, 0)
 *     d3 >= 0 and d4 <= d3                   (1, 0)
 *     vc <= 0 and d1 >= 0 and d3 <= 0        (d1/(d1-d3), 0)
 *     d6 >= 0 and d5 <= d6                   (0, 1)
 *     vb <= 0 and d2 >= 0 and d6 <= 0        (0, d2/(d2-d6))
 *     va <= 0 and d4-d3 >= 0 and d5-d6 >= 0  wb = (d4-d3)/((d4-d3)+(d5-d6)): (1-wb, wb)
 *     otherwise  den = 1/((va+vb)+vc); v = vb*den; w = vc*den, then as selects
 *                (a NaN stays a NaN) v = v<0 ? 0 : v; v = v>1 ? 1 : v; t = 1-v;
 *                w = w<0 ? 0 : w; w = w>t ? t : w
 *   p = (a + ab*v) + ac*w per component; dist2 = (p0*p0 + p1*p1) + p2*p2.
 *   A face matches iff dist2 <= max_dist*max_dist (inclusive; a NaN compares
 *   false); the smallest dist2 wins, among equal ones the smallest face index.
 *   face[i] = that face, dist2[i] = its dist2, bary[i] = ((1-v)-w, v, w); no
 *   match: -1, +inf and a zero row.  A face with a corner index outside [0, nv)
 *   or a non-finite corner matches nothing; a non-finite query matches nothing.
 * The result does not depend on the cell size, on the grid's origin or on the
 * order of the queries.  The grid is the one of ucsa_point_cell_keys; all
 * finite vertices are expected inside its box (as ops.triangle_grid makes it).
 *
 * ucsa_triangle_cell_counts: verts [nv][3] float32, faces [nf][3] int32 ->
 *   counts [nf] int32.  A lane per face: per axis the face covers the cells from
 *   the cell of its smallest corner coordinate to the cell of its largest (the
 *   cell of ucsa_point_cell_keys: (x - origin)/cell, clamped, floored);
 *   counts[f] is the number of cells of that box, 0 for an invalid face.
 * ucsa_triangle_cell_pairs: first [nf] int32 is the exclusive scan of counts
 *   and n_pairs their sum; face f writes the linear keys of its cells, in x, y, z
 *   order, to keys[first[f] ...] and f to pair_face at the same places: fixed
 *   positions, no atomics.  A position outside [0, n_pairs) is not written.
 *   A stable sort of keys gives the pairs by cell with faces ascending in a
 *   cell; offsets [cells + 1] int32 is the position of each cell's first pair;
 *   records [n_pairs][12] float32 holds per sorted pair A.xyz and the bits of
 *   the int32 face index, B.xyz and 0, C.xyz and 0 (ops.triangle_grid builds
 *   the three in torch).
 * ucsa_nearest_triangle: one lane per query; lane t takes query q_order[t]
 *   (int32 [nq], a permutation; NULL: query t; an entry outside [0, nq) writes
 *   nothing) and writes that query's slots of face [nq] int32, dist2 [nq]
 *   float32 and bary [nq][3] float32.  The walk is ucsa_nearest_point's: rings
 *   of cells around the query's clamped cell, a run of cells along z as two
 *   offset reads, and after each ring every slab of unvisited cells whose near
 *   wall is farther than min(best dist2, max_dist^2) cut off.  A face none of
 *   whose cells was visited lies with all corners, and so with its closest
 *   point, beyond such a wall.  The margin: the gap to the wall is shortened by
 *   2^-19 * (|origin| + |origin + dims*cell| + |q|) on that axis and its square
 *   must exceed the bound times 1 + 2^-20 (docs/DESIGN_NOTEBOOK.md, section NT).
 *   A face registered in several cells is evaluated more than once, which does
 *   not change a minimum.  Every loop is bounded by dims; offsets are clamped
 *   into [0, n_pairs]; no atomics, no LDS, no lane waits for another.  A query
 *   farther than max_dist from the grid's box gets no match without a ring.
 *   Limits: origin finite, cell > 0 and finite with a finite far corner, dims
 *   >= 1 each with at most 2^24 cells, nv, nf, n_pairs and nq <= 2^31-1,
 *   max_dist > 0 with a finite float32 square, records 16-byte aligned; an
 *   argument error comes before any launch and nothing is written.  nf == 0 or
 *   n_pairs == 0 in the two build calls: returns 0, launches nothing.
 *   n_pairs == 0 in the search: every query gets no match (records and offsets
 *   may be NULL); nq == 0: returns 0, launches nothing. */
int32_t ucsa_triangle_cell_counts(const float* verts, uint32_t nv, const int32_t* faces,
                                  uint32_t nf, const float* origin, float cell,
                                  const uint32_t* dims, int32_t* counts, void* stream);
int32_t ucsa_triangle_cell_pairs(const float* verts, uint32_t nv, const int32_t* faces,
                                 uint32_t nf, const float* origin, float cell,
                                 const uint32_t* dims, const int32_t* first, uint32_t n_pairs,
                                 int32_t* keys, int32_t* pair_face, void* stream);
int32_t ucsa_nearest_triangle(const float* records, const int32_t* offsets, uint32_t n_pairs,
                              const float* origin, float cell, const uint32_t* dims,
                              const float* queries, const int32_t* q_order, uint32_t nq,
                              float max_dist, int32_t* face, float* dist2, float* bary,
                              void* stream);

/* ---- mesh simplification by vertex clustering (not in the reference) ----
 * Rossignac-Borrel: the vertices of one cell of a uniform grid become one
 * vertex, faces follow their corners, faces that collapse are dropped.  It
 * carries what this project's meshes carry per vertex: label, colour, normal.
 * One sort, no atomics, no data-dependent iteration: tests/simplify_numpy.py
 * restates the three contracts in plain loops and the outputs match it byte
 * for byte.  The inputs are never modified.  The grid is cells of edge `cell`
 * from `origin`, dims[0] x dims[1] x dims[2] of them; origin[3] and dims[3] are
 * host arrays.  The stable sort of the keys, the cluster boundaries, the face
 * de-duplication and the compaction are torch on the device (ops.simplify_mesh).
 *
 * ucsa_vertex_cluster_keys: verts [n][3] float32, labels [n] uint8 or NULL ->
 *   keys [n] int64.  One lane per vertex.  The cell of a coordinate is that of
 *   ucsa_point_cell_keys: t = (p - origin) / cell in float32 (the division
 *   correctly rounded), clamped as a float into [0, dim - 1], then floored.
 *   keys[i] = (((ix << 18 | iy) << 18 | iz) << 8) | label, label = labels[i] or
 *   0 without labels; a vertex with a non-finite coordinate gets INT64_MAX,
 *   which sorts last and belongs to no cluster.  Ascending keys are x-major
 *   cell order, then label.
 *   Limits: n <= 2^31-1 (argument 1), origin finite (2), cell > 0 and finite
 *   with a finite far corner (3), 1 <= dims <= 2^18 each (4; there is no
 *   per-cell table, so the 2^24-cell limit of the point grid does not apply).
 *   n == 0: returns 0, launches nothing.
 * ucsa_cluster_reduce: one lane per cluster.  order [n] int32 is the stable
 *   sort of the keys, first [K+1] int32 the clusters' offsets into it: the
 *   members of cluster c are order[first[c] .. first[c+1]), ordered by label,
 *   then by original index.  Per cluster, over its members in that order:
 *   position  x0 = the first member's position; s = 0; s = s + (x - x0) per
 *             member and axis, in float32; out = x0 + s / (float)count.
 *             Offsets from a member keep the error independent of where the
 *             scene sits.  A cluster of one returns its vertex's bits.
 *   normal    (normals [n][3] float32 or NULL) s = 0; s = s + n per member and
 *             axis; len = sqrtf((x*x + y*y) + z*z); out = len > 0 ? s / len : 0
 *             (the expression of the marching-cubes normals).
 *   colour    (rgb [n][3] uint8 or NULL) 64-bit integer sums per channel;
 *             out = (2*sum + count) / (2*count) in integers: rounds half up.
 *   label     (labels [n] uint8 or NULL) the most frequent label among the
 *             members with label > 0: the members are sorted by label, so this
 *             is the longest run, and the first longest run wins (the smallest
 *             such label); 0 if no member has a label.
 *   count     int32, the number of members.
 *   A sequential float sum is the definition: a long cluster is one lane's
 *   loop and is not split across lanes, so a call that puts every vertex into
 *   one cell costs one lane walking all of them.  The loop is bounded by n.
 *   Offsets are clamped into [0, n] and a decreasing pair is an empty cluster;
 *   an entry of order outside [0, n) is no member; a cluster without members
 *   writes zeros.  A lane writes row c of the outputs and nothing else.
 *   Limits: n <= 2^31-1 (argument 4), K <= n (7); out_normals, out_rgb and
 *   out_labels are required where their input is given (9..11) and untouched
 *   where it is not.  K == 0: returns 0, launches nothing.
 * ucsa_cluster_faces: faces [nf][3] int32, vertex_map [nv] int32 (the cluster of
 *   every vertex, -1 for a dropped one) -> tri [nf][3] int32, keep [nf] uint8.
 *   One lane per face.  A face with a corner index outside [0, nv), with a
 *   corner mapped to a negative value, or with two corners on one cluster is
 *   dropped: keep 0 and the row -1 -1 -1.  Otherwise keep is 1 and the row is
 *   the mapped triple rotated so that its smallest index comes first; the
 *   cyclic order, and so the orientation, is preserved.
 *   Limits: nf, nv <= 2^31-1 (arguments 1, 3).  nf == 0: returns 0, launches
 *   nothing; nv == 0: every face is dropped (vertex_map may be NULL).
 * An argument error comes before any launch and nothing is written. */
int32_t ucsa_vertex_cluster_keys(const float* verts, uint32_t n, const float* origin, float cell,
                                 const uint32_t* dims, const uint8_t* labels, int64_t* keys,
                                 void* stream);
int32_t ucsa_cluster_reduce(const float* verts, const float* normals, const uint8_t* rgb,
                            const uint8_t* labels, uint32_t n, const int32_t* order,
                            const int32_t* first, uint32_t K, float* out_verts,
                            float* out_normals, uint8_t* out_rgb, uint8_t* out_labels,
                            int32_t* out_count, void* stream);
int32_t ucsa_cluster_faces(const int32_t* faces, uint32_t nf, const int32_t* vertex_map,
                           uint32_t nv, int32_t* tri, uint8_t* keep, void* stream);

/* ---- area-uniform sample points on a triangle mesh (not in the reference) ----
 * A deterministic, low-discrepancy point set on the surface of a mesh, with a
 * density of `density` points per unit area: the query points of 3D scores that
 * weigh a surface by its area and not by its tessellation.  A sample is a
 * function of (seed, face index, index inside the face) and the face's corners
 * alone: raising the density keeps every earlier sample of a face and appends
 * new ones, and editing one face changes no sample of another.  No atomics, no
 * LDS; tests/sample_numpy.py restates both contracts in plain loops and the
 * outputs match it byte for byte.  The inputs are never modified.  All float
 * arithmetic is float32 in the order written, without fused multiply-add, with
 * sqrt and divide correctly rounded; all integer arithmetic is uint32, wrapping.
 *
 * Hash   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
 *        x ^= x >> 16.  Per face f: h0 = mix(seed ^ mix(f + 0x9e3779b9)),
 *        hc = mix(h0 ^ 0x3c6ef372), h1 = mix(h0 ^ 0x68bc21eb),
 *        h2 = mix(h0 ^ 0x02e5be93).
 *
 * ucsa_face_sample_counts: verts [nv][3] float32, faces [nf][3] int32 ->
 *   area [nf] float32, count [nf] int32.  One lane per face with corners A, B, C:
 *   e1 = B - A, e2 = C - A, c = e1 x e2 with each component a*b - c*d,
 *   area = 0.5f * sqrtf((cx*cx + cy*cy) + cz*cz), expect = area * density,
 *   count = (int)floorf(expect + (float)(hc >> 8) * 2^-24), at most 2^24: the
 *   offset is uniform in [0, 1), so the rounding has no bias and a face smaller
 *   than 1 / density gets a sample at the right rate.  A face with a corner
 *   index outside [0, nv), a non-finite corner or a non-finite area gets area 0
 *   and count 0.
 *   Limits: nv, nf <= 2^31-1 (arguments 1, 3), density > 0 and finite (4).
 *   nf == 0: returns 0, launches nothing.
 * ucsa_mesh_surface_samples: first [nf+1] int32 is the exclusive prefix sum of
 *   the counts and n_samples = first[nf] (torch on the device in
 *   ops.sample_mesh_surface).  One lane per sample s:
 *   face    the f with first[f] <= s < first[f+1]: the smallest k in [0, nf)
 *           with first[k+1] > s, by a binary search of at most 32 steps over
 *           lo = 0, hi = nf (mid = (lo + hi) >> 1; first[mid+1] > s ? hi = mid :
 *           lo = mid + 1), then f = min(lo, nf - 1).  Every read of `first` is
 *           at an index in [1, nf] whatever its entries hold.  j = s - first[f]
 *           (as a uint32).
 *   bary    a = (j * 0xC13FA9A9 + h1) >> 8, b = (j * 0x91E10DA5 + h2) >> 8: the
 *           R2 sequence (Roberts; the plastic number's powers) in 32-bit fixed
 *           point with a per-face offset, 24 bits each.  Folded in integers: if
 *           a + b > 2^24 then a = 2^24 - a, b = 2^24 - b; c = 2^24 - a - b;
 *           bary = (c, a, b) * 2^-24, exact, non-negative, summing to 1.
 *   point   per axis A + (bary[1] * e1 + bary[2] * e2): offsets from A, so the
 *           error does not grow with the scene's distance from the origin.
 *   labels  (labels [nv] uint8 or NULL) the label of the corner with the largest
 *           weight, the first such corner on a tie.
 *   rgb     (rgb [nv][3] uint8 or NULL) per channel
 *           floorf(((w0*r0 + w1*r1) + w2*r2) + 0.5f).
 *   normals (normals [nv][3] float32 or NULL) n = (w0*n0 + w1*n1) + w2*n2 per
 *           axis, len = sqrtf((x*x + y*y) + z*z), out = len > 0 ? n / len : 0.
 *   -> points [n_samples][3] float32, face [n_samples] int32, bary
 *   [n_samples][3] float32, and out_normals, out_rgb, out_labels (rows per
 *   sample) where their input is given.  Only a malformed `first` can lead to a
 *   face with a corner index outside [0, nv): its samples get the face and the
 *   weights as above, a zero point and zero attributes.  A lane writes row s
 *   of the outputs and nothing else.
 *   Limits: nv, nf <= 2^31-1 (arguments 1, 3), n_samples <= 2^31-1 (5), nf > 0
 *   where n_samples > 0 (3); out_normals, out_rgb and out_labels are required
 *   where their input is given (13..15) and untouched where it is not.
 *   n_samples == 0: returns 0, launches nothing.
 * An argument error comes before any launch and nothing is written. */
int32_t ucsa_face_sample_counts(const float* verts, uint32_t nv, const int32_t* faces,
                                uint32_t nf, float density, uint32_t seed, float* area,
                                int32_t* count, void* stream);
int32_t ucsa_mesh_surface_samples(const float* verts, uint32_t nv, const int32_t* faces,
                                  uint32_t nf, const int32_t* first, uint32_t n_samples,
                                  uint32_t seed, const float* normals, const uint8_t* rgb,
                                  const uint8_t* labels, float* points, int32_t* face,
                                  float* bary, float* out_normals, uint8_t* out_rgb,
                                  uint8_t* out_labels, void* stream);

/* ---- signed distance to a triangle mesh (not in the reference) ----
 * The nearest-triangle search says how far a point is from a surface; this
 * section says on which side.  The sign is that of the angle-weighted
 * pseudonormal of the feature (face, edge or vertex) the closest point lies on
 * (Baerentzen and Aanaes 2005): the nearest face's own normal gives the wrong
 * sign near convex edges and vertices, the pseudonormal does not.  Positive is
 * the side (B - A) x (C - A) points to.  tests/sdf_numpy.py restates the four
 * contracts in plain loops and the outputs match it byte for byte.  The inputs
 * are never modified.  All arithmetic is float32, every operation rounded and
 * nothing fused, sqrt and divide correctly rounded;
 * dot(x,y) = (x0*y0 + x1*y1) + x2*y2 and a face is valid as in the
 * nearest-triangle section: corner indices in [0, nv), finite corners.
 *
 * ucsa_face_unit_normals: verts [nv][3] float32, faces [nf][3] int32 ->
 *   unit_normal [nf][3] float32.  One lane per face with corners A, B, C:
 *   e1 = B - A, e2 = C - A, n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z,
 *   e1x*e2y - e1y*e2x), l = sqrt(dot(n, n)); the row is n / l per component if
 *   l > 0 and finite, else zeros; zeros for an invalid face too.
 *   Limits: nv, nf <= 2^31-1 (arguments 1, 3).  nf == 0: returns 0, launches
 *   nothing.
 * ucsa_normal_runs: items [n_items] int32, run_first [n_runs+1] int32, weight
 *   [3*nf] float32 or NULL, unit_normal [nf][3] -> out [n_runs][3] float32.  One
 *   lane per run r: acc = 0; for pos = run_first[r] .. run_first[r+1]-1 in
 *   order, it = items[pos], w = weight ? weight[it] : 1, f = it / 3:
 *   acc_c = acc_c + w * unit_normal[f][c] (the product, then the sum);
 *   out[r] = acc, not normalised: only its direction is used.  Offsets are
 *   clamped into [0, n_items] and a decreasing pair is an empty run (zeros); an
 *   item outside [0, 3*nf) is skipped.  The same entry point serves
 *   vertices: runs are vertices, items the corners 3f+k that touch the vertex,
 *             weights the corner angles (an input: no transcendental function is
 *             part of a byte promise here);
 *   edges:    runs are undirected edges, items the half-edges 3f+k (edge k of
 *             face f runs from corner k to corner (k+1)%3), no weights.
 *   ops.mesh_pseudonormals builds the runs with stable sorts, so the items of a
 *   run ascend and a sum has one order.  A sequential float sum is the
 *   definition: no atomics, no LDS, and a run is one lane's loop that is not
 *   split across lanes, so a vertex shared by every face of a mesh costs one
 *   lane walking all of them.  The loop is bounded by n_items.
 *   Limits: n_runs, n_items <= 2^31-1 (arguments 2, 3), nf <= (2^31-1)/3 (6).
 *   n_runs == 0: returns 0, launches nothing.
 * ucsa_mesh_sign: vertex_normal [nv][3] and edge_normal [nf][3][3] (row k of a
 *   face: the sum of its edge k, scattered to every half-edge of that edge) are
 *   the sums above; queries [nq][3], face [nq] int32 (an input: the face the
 *   search found) -> sdf [nq] float32, feature [nq] int32.  One lane per query.
 *   face < 0, face >= nf or an invalid face: sdf = +inf, feature = -1.
 *   Otherwise the closest-point expressions of the nearest-triangle section are
 *   evaluated again for (query, face): the same operands, so the same bits.
 *   The region that decided (v, w), numbered in that section's order from 0,
 *   gives the feature:  0 -> 4 (vertex A)   1 -> 5 (vertex B)   3 -> 6 (vertex C)
 *                       2 -> 1 (edge AB)    5 -> 2 (edge BC)    4 -> 3 (edge CA)
 *                       otherwise -> 0 (the face's interior).
 *   N = unit_normal[f] (feature 0), edge_normal[f][feature-1] (1..3) or
 *   vertex_normal[faces[f][feature-4]] (4..6); s = -dot(p, N) with p the closest
 *   point, the query at the origin; d = sqrt(dist2); sdf = s < 0 ? -d : d.  A
 *   zero or NaN N gives +d; a query on the surface (p = 0) gives +0.
 *   Limits: nv, nf, nq <= 2^31-1 (arguments 1, 3, 8).  nq == 0: returns 0,
 *   launches nothing.
 * ucsa_mesh_tsdf: records, offsets, n_pairs, origin, cell, dims are the grid of
 *   ucsa_nearest_triangle; tsdf and weight [nx][ny][nz] float32 are the arrays of
 *   ucsa_tsdf_integrate with its lattice vol_origin[3], vol_spacing[3] (host
 *   arrays; a spacing may be negative).  One launch, one lane per voxel, z
 *   fastest, so a wave walks neighbouring cells.  The voxel's point is
 *   vol_origin[a] + (float)i_a * vol_spacing[a] (the product, then the sum).
 *   From it runs exactly ucsa_nearest_triangle's search with max_dist = trunc
 *   (the smallest dist2 within trunc*trunc, inclusive, the smallest face index
 *   on a tie), without a queries array and without a face / dist2 / bary round
 *   trip; then the sign as in ucsa_mesh_sign.  On a match t = sdf / trunc, then
 *   as selects t = t < -1 ? -1 : t; t = t > 1 ? 1 : t; tsdf[v] = t and
 *   weight[v] = weight_value.  A voxel without a match is neither read nor
 *   written: the band is overwritten, not averaged with what the volume held.
 *   Cost: that of the search; a voxel farther than trunc from the grid's box
 *   walks nothing, one with nothing near walks every cell within trunc.
 *   Limits: n_pairs <= 2^31-1 (argument 2), the grid as in ucsa_nearest_triangle
 *   (3..5), nv, nf <= 2^31-1 (7, 9), nx, ny, nz >= 2 each with at most 2^31-1
 *   voxels (15), trunc > 0 with a finite float32 square (20), records 16-byte
 *   aligned (0).  n_pairs == 0: returns 0 and writes nothing.
 * An argument error comes before any launch and nothing is written. */
int32_t ucsa_face_unit_normals(const float* verts, uint32_t nv, const int32_t* faces, uint32_t nf,
                               float* unit_normal, void* stream);
int32_t ucsa_normal_runs(const int32_t* items, const int32_t* run_first, uint32_t n_runs,
                         uint32_t n_items, const float* weight, const float* unit_normal,
                         uint32_t nf, float* out, void* stream);
int32_t ucsa_mesh_sign(const float* verts, uint32_t nv, const int32_t* faces, uint32_t nf,
                       const float* unit_normal, const float* vertex_normal,
                       const float* edge_normal, const float* queries, uint32_t nq,
                       const int32_t* face, float* sdf, int32_t* feature, void* stream);
int32_t ucsa_mesh_tsdf(const float* records, const int32_t* offsets, uint32_t n_pairs,
                       const float* origin, float cell, const uint32_t* dims, const float* verts,
                       uint32_t nv, const int32_t* faces, uint32_t nf, const float* unit_normal,
                       const float* vertex_normal, const float* edge_normal, float* tsdf,
                       float* weight, uint32_t nx, uint32_t ny, uint32_t nz,
                       const float* vol_origin, const float* vol_spacing, float trunc,
                       float weight_value, void* stream);

/* ---- rays against a triangle mesh (not in the reference) ----
 * "What does this ray hit on this mesh" and "is this segment free": the query
 * the visibility-aware 3D scores need, exact where a depth-buffer test through
 * the rasterizer is pixel-quantised.  tests/raycast_numpy.py states the contract
 * as plain brute force over all faces and the outputs match it byte for byte,
 * whatever the cell size, the grid's origin or the order of the rays.
 * A ray is o, d (float32) with the parameter range [t_min, t_max]; t_max may be
 * +inf and t_min -inf.  A face counts by the rule of the triangle grid (corner
 * indices in [0, nv), finite corners A, B, C).  Nothing is fused.
 *  1. A ray with a non-finite component, or d = 0, hits nothing.
 *  2. kz = argmax |d| (the first on ties), kx = (kz+1)%3, ky = (kz+2)%3;
 *     Sx = d[kx]/d[kz], Sy = d[ky]/d[kz] in float32.
 *  3. Per corner P in float32: px = P[kx]-o[kx], py = P[ky]-o[ky],
 *     pz = P[kz]-o[kz]; X = px - Sx*pz, Y = py - Sy*pz (the product, then the
 *     difference).
 *  4. In float64, on the converted X, Y: U = Cx*By - Cy*Bx, V = Ax*Cy - Ay*Cx,
 *     W = Bx*Ay - By*Ax.  The products are exact, so the signs are exact and an
 *     edge shared by two faces gives exactly negated values in the two: the
 *     watertight test of Woop, Benthin and Wald (2013), its zero-case fallback
 *     made unconditional.
 *  5. The face is hit if U, V, W are all >= 0 or all <= 0, and
 *     det = (U+V)+W != 0.  No back-face culling.
 *  6. t = (float)(((U*pz_A + V*pz_B) + W*pz_C) / det / (double)d[kz]); t must be
 *     finite and t_min <= t <= t_max (inclusive; a NaN bound admits nothing).
 *  7. The box clause.  Per axis a, in float32: p = o[a] + t*d[a];
 *     mn, mx = the corners' minimum and maximum on that axis;
 *     S = 2^-20 * ((|o[a]| + |t*d[a]|) + max(|mn|, |mx|)); mn - S <= p <= mx + S
 *     must hold.  t is a convex sum of the corners' depths and the weights put
 *     the sheared ray through the sheared face, so p lies in the face's box up
 *     to the rounding of the shear; the clause turns that into a statement
 *     about computed numbers, which is what a traversal of the grid (a face is
 *     registered in the cells of its box) needs to promise every hit.  It
 *     rejects a hit only where the shear's rounding, about
 *     2^-22 |S| (the face's reach from o along kz), exceeds S on a minor axis:
 *     a face that reaches many times farther along the ray's major axis than
 *     the coordinates on a minor axis are large (docs/DESIGN_NOTEBOOK.md,
 *     section RC).
 *  8. The hit with the smallest t wins, among equal t the smallest face index.
 *     face [n] int32 (-1 on a miss), t [n] float32 (+inf on a miss), bary
 *     [n][3] float32 = ((float)(U/det), (float)(V/det), (float)(W/det)), the
 *     weights of A, B, C (a zero row on a miss).
 * ucsa_mesh_occluded is the any-hit form: occluded [n] uint8, 1 if any face is
 * hit in the range.
 *
 * records, offsets, n_pairs, origin, cell, dims are the grid of
 * ucsa_nearest_triangle (all finite vertices inside its box).  origins, dirs
 * [n_rays][3] float32; t_min, t_max [n_rays] float32, or NULL for t_min_all,
 * t_max_all; order int32 [n_rays], a permutation, or NULL: lane t takes ray
 * order[t] (an entry outside [0, n_rays) writes nothing) and writes that ray's
 * slots.  One lane per ray walks the grid's layers along kz in ray order (a
 * slab supercover): per layer the parameter interval between its walls, the
 * ray's points at both ends on the two minor axes, and the cells between
 * them; walls and ranges are grown by 2^-17 * (|o| + |origin| + |origin +
 * dims*cell|) on their axis.  The walk ends when the best t lies before the
 * next layer's entry (strictly) or that entry lies past t_max; the any-hit form
 * ends at its first hit.  Why no hit is lost is argued at the head of
 * csrc/mesh_raycast.hip.  A face registered in several cells is evaluated more
 * than once, which does not change a minimum.  Every loop is bounded by dims or
 * n_pairs; offsets are clamped into [0, n_pairs]; no atomics, no LDS, no lane
 * waits for another.  The inputs are never modified.
 * Limits: n_pairs <= 2^31-1 (argument 2), the grid as in ucsa_nearest_triangle
 * (3..5), n_rays <= 2^31-1 (13), records 16-byte aligned (0).  An argument
 * error comes before any launch and nothing is written.  n_pairs == 0: every
 * ray misses (records and offsets may be NULL); n_rays == 0: returns 0,
 * launches nothing. */
int32_t ucsa_raycast_mesh(const float* records, const int32_t* offsets, uint32_t n_pairs,
                          const float* origin, float cell, const uint32_t* dims,
                          const float* origins, const float* dirs, const float* t_min,
                          const float* t_max, float t_min_all, float t_max_all,
                          const int32_t* order, uint32_t n_rays, int32_t* face, float* t,
                          float* bary, void* stream);
int32_t ucsa_mesh_occluded(const float* records, const int32_t* offsets, uint32_t n_pairs,
                           const float* origin, float cell, const uint32_t* dims,
                           const float* origins, const float* dirs, const float* t_min,
                           const float* t_max, float t_min_all, float t_max_all,
                           const int32_t* order, uint32_t n_rays, uint8_t* occluded, void* stream);

/* ---- registration of points to a triangle mesh (not in the reference) ----
 * One step of ICP in one call: move the source points by a rigid transform,
 * find each moved point's closest point on the target mesh, and reduce the
 * Gauss-Newton normal equations of the step to 29 float64 numbers on the device.
 * The host solves the 6 x 6 system and composes the transform
 * (utils/registration.py).  tests/register_numpy.py restates the contract over
 * the brute-force search of tests/surface_numpy.py and the 29 sums match it byte
 * for byte, whatever the cell size or the grid's origin.
 *
 * records, offsets, n_pairs, origin, cell, dims are the grid of
 * ucsa_nearest_triangle; verts [nv][3] float32 and faces [nf][3] int32 the mesh
 * it was built over; unit_normal [nf][3] float32 the output of
 * ucsa_face_unit_normals; points [n][3] float32; transform 12 float32 on the
 * host, the rows of [R | t]; mode 0 = point to plane, 1 = point to point;
 * workspace: float64 on the device for the partial sums, workspace_doubles its
 * size.  With c_1 = ceil(n / 256) and c_(k+1) = ceil(c_k / 256) it must hold
 * 29 * (the sum of all c_k > 1) doubles; for n <= 256 that is none and it may be
 * NULL.  Outputs: sums [29] float64 on the device; face [n] int32 and dist2 [n]
 * float32, each optional (NULL: not written).
 * Per point i, everything in float32 and nothing fused unless float64 is named:
 *  1. q_k = ((R[k][0]*x + R[k][1]*y) + R[k][2]*z) + t[k] for k = 0, 1, 2.
 *  2. From q runs exactly ucsa_nearest_triangle's search with max_dist: the
 *     smallest dist2 within max_dist*max_dist (inclusive) wins, among equal ones
 *     the smallest face index; a non-finite q matches nothing, an invalid face
 *     matches nothing.  face[i] and dist2[i] receive what ucsa_nearest_triangle
 *     writes for the query q (-1 and +inf without a match).
 *  3. On a match the closest-point expressions of the nearest-triangle section
 *     are evaluated again for (q, face) on the mesh's corners, as in
 *     ucsa_mesh_sign: the same operands, so the same bits.  p is the closest
 *     point with the query at the origin (the closest point minus q).
 *  4. Mode 0 has one row with n = unit_normal[face]; mode 1 three rows with
 *     n = (1,0,0), (0,1,0), (0,0,1).  Per row r = (n0*p0 + n1*p1) + n2*p2 and
 *     J = (q1*n2 - q2*n1, q2*n0 - q0*n2, q0*n1 - q1*n0, n0, n1, n2), each of
 *     the first three a product, a product, then the difference (the products
 *     with the 0 and 1 of mode 1 are carried out like any other).  This
 *     linearises q <- q + omega x q + upsilon: the step minimises
 *     sum (r - J . xi)^2 over xi = (omega, upsilon).
 *  5. In float64, on the converted floats (the products are exact): the 21
 *     entries J_a*J_b for a <= b, row-major; the 6 entries J_a*r; r*r; 1.0: 29
 *     terms.  In mode 1 a point's term is (x's + y's) + z's, the three rows in
 *     that order, so the last sum counts rows: 3 per matched point.  A point
 *     without a match contributes +0.0 to all 29, by a select, so that no NaN
 *     leaks in.
 *  6. The sum is a fixed tree.  The n rows of terms are padded with rows of +0.0
 *     to a multiple of 256; every group of 256 consecutive rows is reduced by
 *     eight levels of adjacent pairs (2j, 2j+1); the group results are rows
 *     again, padded and reduced the same way, until one row is left: sums.  At
 *     least one stage always runs, so n == 0 gives 29 times +0.0 and a lone
 *     -0.0 term gives +0.0.  No atomics; the result depends on the order of the
 *     points only through this tree and is the same bytes every run.
 * One lane per point in work-groups of 256 (k_icp_sums), then a lane per group
 * result (k_icp_reduce) while more than one row is left: at most four launches.
 * Every lane of a work-group reaches its one barrier; every loop is bounded as
 * in ucsa_nearest_triangle; no lane waits for another outside the barrier.
 * Cost: that of the search.  The inputs are never modified.
 * Limits: n_pairs <= 2^31-1 (argument 2), the grid as in ucsa_nearest_triangle
 * (3..5), nv, nf, n <= 2^31-1 (7, 9, 12), max_dist > 0 with a finite float32
 * square (14), mode 0 or 1 (15), the workspace (16, 17), records 16-byte aligned
 * (0).  An argument error comes before any launch and nothing is written.
 * n_pairs == 0 or nf == 0: no point matches (records and offsets may be NULL),
 * sums is 29 times +0.0. */
int32_t ucsa_icp_sums(const float* records, const int32_t* offsets, uint32_t n_pairs,
                      const float* origin, float cell, const uint32_t* dims, const float* verts,
                      uint32_t nv, const int32_t* faces, uint32_t nf, const float* unit_normal,
                      const float* points, uint32_t n, const float* transform, float max_dist,
                      int32_t mode, double* workspace, uint64_t workspace_doubles, double* sums,
                      int32_t* face, float* dist2, void* stream);

/* ---- registration of points to a TSDF volume (not in the reference) ----
 * The tracking half of KinectFusion as one step: move the points by a rigid
 * transform, sample the volume's signed distance and its gradient at each moved
 * point (one trilinear cell: sixteen loads), and reduce the point-to-plane
 * normal equations to the 29 float64 numbers of ucsa_icp_sums, mode 0, in the
 * same order and the same tree, so that utils/registration.py's solve_step and
 * compose take them unchanged.  No mesh, no grid, no search.
 * tests/tsdf_register_numpy.py restates the contract; sums, value and matched
 * equal it byte for byte.
 *
 * tsdf, weight: the state and lattice of ucsa_tsdf_integrate, float32
 * [nx][ny][nz], tsdf in units of trunc; lattice point (i,j,k) sits at
 * origin + (i,j,k)*spacing and is stored at (i*ny+j)*nz+k.  origin3, spacing3,
 * transform (12 float32, the rows of [R | t]) are read on the host.  points
 * [n][3] float32.  workspace, workspace_doubles and sums as for ucsa_icp_sums.
 * value [n] float32 and matched [n] uint8 are optional (NULL: not written).
 * Per point i < n, in float32, every operation as written, nothing fused,
 * division and sqrt correctly rounded:
 *  1. q_k = ((R[k][0]*x + R[k][1]*y) + R[k][2]*z) + t[k], as ucsa_icp_sums.
 *  2. g_a = (q_a - origin_a) / spacing_a.  inside iff on every axis
 *     g_a >= 0 && g_a <= (float)(n_a - 1); a NaN fails.  Nothing is converted
 *     to an integer and no index is formed before inside holds; a point outside
 *     the lattice is unmatched, not clamped into it (ucsa_tsdf_raycast clamps).
 *  3. fl_a = min(floorf(g_a), (float)(n_a - 2)), c_a = (uint32_t)fl_a,
 *     f_a = g_a - fl_a: exact, in [0, 1]; g_a = n_a - 1 is the last cell at
 *     f_a = 1.  v[4i+2j+k] are the cell's eight corners (c0+i, c1+j, c2+k), of
 *     both arrays, in ucsa_tsdf_raycast's order.
 *  4. observed iff all eight weights >= min_weight (ucsa_tsdf_raycast's rule).
 *  5. With lerp(x, y, f) = x + f*(y - x): c00 = lerp(v0, v1, f2),
 *     c01 = lerp(v2, v3, f2), c10 = lerp(v4, v5, f2), c11 = lerp(v6, v7, f2),
 *     c0 = lerp(c00, c01, f1), c1 = lerp(c10, c11, f1), F = lerp(c0, c1, f0);
 *     G0 = c1 - c0, G1 = lerp(c01 - c00, c11 - c10, f0),
 *     G2 = lerp(lerp(v1 - v0, v3 - v2, f1), lerp(v5 - v4, v7 - v6, f1), f0),
 *     each divided by spacing_a; ln = sqrt((G0*G0 + G1*G1) + G2*G2),
 *     n_a = G_a / ln: the value and the normal of ucsa_tsdf_raycast at a hit.
 *  6. matched iff inside && observed && ln > 0 && ln finite &&
 *     fabsf(F) <= max_tsdf (a NaN fails).  Free space in front of a surface
 *     (eight corners at 1) has a zero gradient and never matches.
 *  7. r = -(F * trunc), J = (q1*n2 - q2*n1, q2*n0 - q0*n2, q0*n1 - q1*n0, n0, n1,
 *     n2).  n points toward free space and the surface point is
 *     q - F*trunc*n, so r has the sign of ucsa_icp_sums' n.(c - q).
 *  8. The 29 float64 terms and their tree are items 5 and 6 of ucsa_icp_sums in
 *     mode 0: +0.0 by a select for an unmatched row, 256 rows per group, eight
 *     levels of adjacent pairs, repeated on the group results; n == 0 gives 29
 *     times +0.0.
 *  9. value[i] = F where inside && observed, NaN otherwise; matched[i] is 0 or 1.
 * One lane per point in work-groups of 256 (k_tsdf_icp_sums), then
 * k_icp_reduce while more than one row is left.  Every lane reaches the one
 * barrier; no atomics; the same bytes every run.  The inputs are never modified.
 * Limits: tsdf, weight not NULL (0, 1); nx, ny, nz >= 2 and nx*ny*nz <= 2^31-1
 * (2, 3, 4); origin finite (5); spacing finite and > 0 (6); n <= 2^31-1 (8),
 * points not NULL unless n == 0 (7); transform (9); trunc > 0 and finite (10);
 * min_weight > 0 (11); 0 < max_tsdf <= 1 (12); the workspace (13, 14); sums
 * (15).  An argument error comes before any launch and nothing is written. */
int32_t ucsa_tsdf_icp_sums(const float* tsdf, const float* weight, uint32_t nx, uint32_t ny,
                           uint32_t nz, const float* origin3, const float* spacing3,
                           const float* points, uint32_t n, const float* transform, float trunc,
                           float min_weight, float max_tsdf, double* workspace,
                           uint64_t workspace_doubles, double* sums, float* value,
                           uint8_t* matched, void* stream);

/* ---- the same step for K transforms in one call (not in the reference) ----
 * The lock-step half of a global registration (utils/registration.py:
 * register_points_tsdf_batch): the normal equations of K rigid hypotheses of the
 * same n points against the same volume from one launch, so that K loops advance
 * together, one launch and one read per iteration.
 * tests/test_gpu_lockstep.py checks every row against tests/tsdf_register_numpy.py
 * and against ucsa_tsdf_icp_sums as int64 words.
 *
 * tsdf, weight, nx, ny, nz, origin3, spacing3, points, n, trunc, min_weight,
 * max_tsdf: as for ucsa_tsdf_icp_sums.  transforms [K][12] float32 (the rows of
 * [R | t] of every hypothesis) is on the device, like points.  sums [K][29]
 * float64 on the device is written here.
 * For every k < K, sums[k][0..28] are the 29 numbers ucsa_tsdf_icp_sums writes
 * to its sums for transform k, all other arguments equal: steps 1 to 8 of its
 * contract per point, the same float32 expressions in the same order, the same
 * float64 terms and the same tree (rows padded with +0.0 to a multiple of 256,
 * eight levels of adjacent pairs per group, repeated on the group results).
 * The bytes are equal, not close.  A row depends on its own transform alone,
 * not on K, on its position in the batch or on its neighbours.  There is no
 * value and no matched output (step 9): they would be K x n.
 * One lane per point in work-groups of 256, UCSA_TSDF_ICP_BATCH_TILE transforms
 * per work-group along the grid's x axis (k_tsdf_icp_sums_batch); each
 * (work-group, transform) writes its own 29 doubles, then k_icp_reduce (the
 * transform on the grid's y axis) while more than one row per transform is left.  Every lane reaches the one
 * barrier; no atomics; the same bytes every run.  The inputs are never modified.
 * workspace: the stages' rows, K times those of ucsa_tsdf_icp_sums:
 * workspace_doubles >= K * rows(n) * 29 with rows(n) the sum of the counts
 * c_0 = ceil(n / 256), c_{j+1} = ceil(c_j / 256) that are greater than 1
 * (0 for n <= 256: workspace may then be NULL).
 * Limits: tsdf, weight not NULL (0, 1); nx, ny, nz >= 2 and nx*ny*nz <= 2^31-1
 * (2, 3, 4); origin finite (5); spacing finite and > 0 (6); n <= 2^23 (8),
 * points not NULL unless n == 0 (7); K <= UCSA_TSDF_ICP_BATCH_MAX (10): with
 * n <= 2^23 that is at most 2^7 tiles by 2^15 work-groups, one launch, which is
 * never split; transforms not NULL unless K == 0 (9); trunc > 0 and finite
 * (11); min_weight > 0 (12); 0 < max_tsdf <= 1 (13); the workspace (14, 15);
 * sums not NULL unless K == 0 (16).  An argument error returns UCSA_ERR_ARG -
 * index before any launch and nothing is written.  K == 0: nothing is done;
 * n == 0: all K rows are 29 times +0.0. */
#define UCSA_TSDF_ICP_BATCH_TILE 8
#define UCSA_TSDF_ICP_BATCH_MAX 1024
int32_t ucsa_tsdf_icp_sums_batch(const float* tsdf, const float* weight, uint32_t nx, uint32_t ny,
                                 uint32_t nz, const float* origin3, const float* spacing3,
                                 const float* points, uint32_t n, const float* transforms,
                                 uint32_t K, float trunc, float min_weight, float max_tsdf,
                                 double* workspace, uint64_t workspace_doubles, double* sums,
                                 void* stream);

/* ---- scores of many rigid hypotheses against a TSDF volume (not in the reference) ----
 * The evaluation half of a global registration (utils/registration.py:
 * global_register_points_tsdf): K rigid transforms, each applied to the same n
 * points and scored against the volume's distance field, in one call.  Four
 * exact integers per transform, so that the result depends neither on the order
 * of the points nor on the order of the adds.
 * tests/global_register_numpy.py restates the contract; scores equals it byte
 * for byte.
 *
 * tsdf, weight, nx, ny, nz, origin3, spacing3: as for ucsa_tsdf_icp_sums.
 * points [n][3] float32 and transforms [K][12] float32 (the rows of [R | t] of
 * every hypothesis) are on the device; min_weight and max_tsdf are host
 * scalars.  scores [K][4] int64 on the device is zeroed and written here.
 * Per (transform k, point i), in float32, every operation as written, nothing
 * fused, division correctly rounded: steps 1 to 5 of ucsa_tsdf_icp_sums with
 * transform k (q, g, inside, the cell, observed, F; the gradient is not
 * formed).  Then
 *   inlier = inside && observed && fabsf(F) <= max_tsdf,
 *   free   = inside && observed && F > max_tsdf: the point lies in space the
 *            volume saw to be empty (a NaN F is neither),
 *   e      = (int64)rintf(fabsf(F) * 1048576.0f) for an inlier, else 0: the
 *            product is exact, the rounding half-to-even, e <= 2^20.
 * scores[k] = (sum inlier, sum free, sum e, sum e*e) over the points.
 * One lane per point in work-groups of 256, UCSA_TSDF_SCORE_TILE transforms per
 * work-group (k_tsdf_score); each work-group adds its four numbers per transform
 * to scores with 64-bit integer atomics.  No float atomics; every lane reaches
 * the one barrier; the same bytes every run.  The entry point splits K over as
 * many launches as the grid needs.  The inputs are never modified.
 * Limits: tsdf, weight not NULL (0, 1); nx, ny, nz >= 2 and nx*ny*nz <= 2^31-1
 * (2, 3, 4); origin finite (5); spacing finite and > 0 (6); n <= 2^23 (8), so
 * that sum e*e stays below 2^63, points not NULL unless n == 0 (7);
 * K <= 2^31-1 (10), transforms not NULL unless K == 0 (9); min_weight > 0 (11);
 * 0 < max_tsdf < 1 (12): at 1 free space would count as inlier; scores not NULL
 * unless K == 0 (13).  An argument error returns UCSA_ERR_ARG - index before
 * any launch and nothing is written.  K == 0: nothing is done; n == 0: scores
 * is zeroed and nothing that reads points is launched. */
#define UCSA_TSDF_SCORE_TILE 16
int32_t ucsa_tsdf_score_transforms(const float* tsdf, const float* weight, uint32_t nx,
                                   uint32_t ny, uint32_t nz, const float* origin3,
                                   const float* spacing3, const float* points, uint32_t n,
                                   const float* transforms, uint32_t K, float min_weight,
                                   float max_tsdf, int64_t* scores, void* stream);

/* ---- projective ICP against a pair of maps (not in the reference) ----
 * KinectFusion's own tracker as one step: move the source points (and their
 * normals) by a rigid transform into the target camera's frame, project each
 * into the target's image, gather the target's point and normal at that pixel
 * (projective data association: a gather, not a search), gate the pair, and
 * reduce the point-to-plane normal equations to the 29 float64 numbers of
 * ucsa_icp_sums, mode 0, in the same order and the same tree, so that
 * utils/registration.py's solve_step and compose take them unchanged.  The
 * target maps are those of a second frame (ucsa_depth_normals /
 * ucsa_depth_frontend: frame to frame) or of the model ray-cast from the last
 * pose (ucsa_tsdf_raycast: frame to model).  No volume, mesh or grid.
 * tests/projective_numpy.py restates the contract; sums, pixel and residual
 * equal it byte for byte.
 *
 * points [n][3] float32, the source points; normals [n][3] float32, their
 * normals, or NULL: no compatibility gate.  target_points [H][W][3] and
 * target_normals [H][W][3] float32 in the target camera's frame, target_mask
 * [H][W] uint8, ucsa_depth_normals' bit field; reject a subset of
 * UCSA_DEPTH_EDGE | UCSA_DEPTH_GRAZING.  fx, fy, cx, cy, max_dist, min_cos and
 * transform (12 float32, the rows of [R | t]: source frame -> target camera
 * frame) are read on the host.  workspace, workspace_doubles and sums as for
 * ucsa_icp_sums.  pixel [n] int32 and residual [n] float32 are optional (NULL:
 * not written).
 * Per point i < n, in float32, every operation as written, nothing fused,
 * division correctly rounded:
 *  1. q_k = ((R[k][0]*x + R[k][1]*y) + R[k][2]*z) + t[k], as ucsa_icp_sums.
 *  2. With source normals s: m_k = (R[k][0]*s0 + R[k][1]*s1) + R[k][2]*s2.
 *  3. Unmatched unless q2 > 0 (a NaN fails).
 *  4. u = floorf((fx*q0)/q2 + cx), v = floorf((fy*q1)/q2 + cy):
 *     ucsa_tsdf_integrate's own expression (pixel (row v, column u) covers
 *     [u, u+1) x [v, v+1), its centre at +0.5).
 *  5. inside iff 0 <= u < (float)W and 0 <= v < (float)H, compared in float32
 *     (a NaN fails).  Nothing is converted to an integer and no index is formed
 *     before inside holds.
 *  6. c = target_points[v][u], nt = target_normals[v][u], mk = target_mask[v][u].
 *     The target is valid iff mk & UCSA_DEPTH_NORMAL, !(mk & reject) and all
 *     six floats are finite.
 *  7. d = c - q; dist2 = (d0*d0 + d1*d1) + d2*d2; matched iff
 *     dist2 <= max_dist*max_dist, the square taken in float32, inclusive.
 *  8. With source normals also (m0*nt0 + m1*nt1) + m2*nt2 >= min_cos (a NaN
 *     fails).  Without them min_cos is checked and otherwise unused.
 *  9. r = (nt0*d0 + nt1*d1) + nt2*d2,
 *     J = (q1*nt2 - q2*nt1, q2*nt0 - q0*nt2, q0*nt1 - q1*nt0, nt0, nt1, nt2),
 *     each of the first three a product, a product, then the difference.
 * 10. The 29 float64 terms and their tree are items 5 and 6 of ucsa_icp_sums in
 *     mode 0: +0.0 by a select for an unmatched row, so that no NaN leaks in;
 *     n == 0 gives 29 times +0.0.
 * 11. pixel[i] = v*W + u where matched, -1 otherwise; residual[i] = r where
 *     matched, NaN otherwise.
 * One lane per point in work-groups of 256 (k_projective_icp_sums), then
 * k_icp_reduce while more than one row is left.  Every lane reaches the one
 * barrier (a lane with i >= n takes the unmatched path); no atomics; the same
 * bytes every run.  The inputs are never modified.
 * Limits: points not NULL unless n == 0 (0); n <= 2^31-1 (2); the three maps
 * not NULL (3, 4, 5); 1 <= H <= 16384 (6), 1 <= W <= 16384 (7); reject within
 * EDGE | GRAZING (8); fx, fy > 0 and finite (9, 10); cx, cy finite (11, 12);
 * transform (13); max_dist > 0 with a finite float32 square (14);
 * -1 <= min_cos <= 1 (15); the workspace (16, 17); sums (18).  An argument
 * error returns UCSA_ERR_ARG - index before any launch and nothing is
 * written. */
int32_t ucsa_projective_icp_sums(const float* points, const float* normals, uint32_t n,
                                 const float* target_points, const float* target_normals,
                                 const uint8_t* target_mask, uint32_t H, uint32_t W,
                                 uint32_t reject, float fx, float fy, float cx, float cy,
                                 const float* transform, float max_dist, float min_cos,
                                 double* workspace, uint64_t workspace_doubles, double* sums,
                                 int32_t* pixel, float* residual, void* stream);

/* ---- the two frame trackers' steps with a weight per row (not in the reference) ----
 * Iteratively reweighted least squares for ucsa_projective_icp_sums and
 * ucsa_tsdf_icp_sums: a robust kernel (Huber, Tukey) on the residual and an
 * optional weight per source point (ucsa_depth_confidence's, for one), so that a
 * pair that passes the gates but belongs to something the target does not show
 * stops pulling on the pose.  The entry points stand beside their siblings and
 * run the same kernels with the weight switched on.  tests/robust_numpy.py
 * restates the contract; sums (as int64 words), the weights and the per-point
 * outputs equal it bit for bit.
 *
 * Each takes its sibling's arguments, with the same meaning, and in addition
 * point_weight [n] float32 on the device or NULL (every p = 1), robust_kind
 * (UCSA_ROBUST_NONE / HUBER / TUKEY), robust_scale (a host float in the
 * residual's units: Huber's k, Tukey's c; not read for NONE) and the optional
 * output weight_out [n] float32 (NULL: not written).
 * Per point i < n: the sibling's steps up to and including the gates and the
 * row (J, r) -- steps 1 to 9 of ucsa_projective_icp_sums, 1 to 7 of
 * ucsa_tsdf_icp_sums -- operand for operand.  Then, in float32, each operation
 * rounded once, division and sqrt correctly rounded:
 *   a   = fabsf(r).
 *   rho = 1 for NONE;
 *         Huber: 1 if a <= k, else k / a;
 *         Tukey: t = a / c, u = 1 - t*t, rho = u*u if a < c, else 0.
 *   p   = point_weight[i], or 1; a p that is not finite and > 0 gives w = 0: the
 *         point takes no part (ucsa_tsdf_integrate_weighted's rule for a pixel).
 *   w   = p * rho.
 *   The row counts iff it matched and w > 0.
 *   s   = sqrtf(w); J_k <- s*J_k for the six entries and r <- s*r.  The row's 1
 *         stays 1.
 * The 29 float64 terms of a row that counts are the siblings' products of the
 * scaled floats (exact in float64), +0.0 by a select otherwise, and the tree is
 * the siblings': sums[0..20] = sum w J^T J, sums[21..26] = sum w J^T r,
 * sums[27] = sum w r^2, sums[28] = the rows that count.  With NONE and no
 * point_weight s = 1, a product by 1 is exact, and the sums are the sibling's
 * as int64 words.
 * weight_out[i] = w for a row that counts, +0.0 otherwise.  The siblings'
 * per-point outputs report the geometric match whatever the weight: pixel /
 * residual (the unscaled r) and value / matched.
 * One lane per point in work-groups of 256 (k_projective_icp_sums<true>,
 * k_tsdf_icp_sums<true>: the siblings' kernel templates with WEIGHTED set), the
 * weight loaded with the point, then k_icp_reduce
 * while more than one row is left.  Every lane reaches the one barrier; no
 * atomics; the same bytes every run.  The inputs are never modified.
 * Limits: the siblings', at the siblings' indices up to min_cos (15) and
 * max_tsdf (12); then robust_kind one of the three (17; 14), robust_scale
 * finite and > 0 unless NONE (18; 15), the workspace (19, 20; 16, 17), sums
 * (21; 18).  An argument error returns UCSA_ERR_ARG - index before any launch
 * and nothing is written. */
#define UCSA_ROBUST_NONE 0
#define UCSA_ROBUST_HUBER 1
#define UCSA_ROBUST_TUKEY 2
int32_t ucsa_projective_icp_sums_weighted(const float* points, const float* normals, uint32_t n,
                                          const float* target_points, const float* target_normals,
                                          const uint8_t* target_mask, uint32_t H, uint32_t W,
                                          uint32_t reject, float fx, float fy, float cx, float cy,
                                          const float* transform, float max_dist, float min_cos,
                                          const float* point_weight, int32_t robust_kind,
                                          float robust_scale, double* workspace,
                                          uint64_t workspace_doubles, double* sums, int32_t* pixel,
                                          float* residual, float* weight_out, void* stream);
int32_t ucsa_tsdf_icp_sums_weighted(const float* tsdf, const float* weight, uint32_t nx,
                                    uint32_t ny, uint32_t nz, const float* origin3,
                                    const float* spacing3, const float* points, uint32_t n,
                                    const float* transform, float trunc, float min_weight,
                                    float max_tsdf, const float* point_weight, int32_t robust_kind,
                                    float robust_scale, double* workspace,
                                    uint64_t workspace_doubles, double* sums, float* value,
                                    uint8_t* matched, float* weight_out, void* stream);

/* ---- The depth front end: bilateral filter, points, normals, edge rejection
 * (not in the reference) -----------------------------------------------------
 * What KinectFusion does to a depth frame before it integrates or tracks it
 * (utils/depth_frontend.py): everything above reads depth[v][u] as the sensor
 * gave it.  Three entry points over depth [B,H,W] fp32 z-depth on the device
 * (and ucsa_depth_confidence, last in this section, over their outputs);
 * fx, fy, cx, cy, depth_min, depth_max and every threshold are HOST scalars.
 * All arithmetic is fp32, every operation as written, no contraction, division
 * and sqrt correctly rounded; tests/depth_numpy.py restates the three contracts
 * and every output equals it bit for bit.  One thread per pixel, a work-group
 * per 16 x 16 tile, the tile and its halo in LDS; no atomics, no scratch, the
 * same bytes every run.  The input is never written and must not alias an
 * output.
 *
 * measured(z) iff z is finite and depth_min <= z <= depth_max: the validity
 * rule of ucsa_tsdf_integrate.  A pixel outside the image is not measured.
 *
 * ucsa_depth_filter: a bilateral filter whose weights come from two tables on
 * the device, so that no exp is evaluated here and the result can be restated
 * exactly: w_space [(2r+1)^2] fp32, row-major over the window, 1 <= r <= 4,
 * and w_range [Q] fp32 with Q = UCSA_DEPTH_RANGE_BINS = 256, bin q covering
 * |z_n - z| in [q, q+1) * 3 sigma / Q.  Per pixel (i, j) with depth z:
 *   not measured: filtered = 0.  Otherwise
 *   sigma = sigma_depth + sigma_z2 * (z*z);  scale = 256.0f / (3.0f * sigma);
 *   num = den = 0; for dy = -r..r, for dx = -r..r (row-major), z_n the depth at
 *   (i+dy, j+dx), taken iff measured (the centre is):
 *     d = z_n - z;  t = fabsf(d) * scale;  skipped unless t < 256.0f (NaN skips);
 *     w = w_space[(dy+r)*(2r+1) + (dx+r)] * w_range[(int)t];
 *     num = num + w*d;  den = den + w;
 *   filtered = z + num / den.
 * The value is an offset from the centre: a constant image comes back with its
 * own bits and the rounding error does not grow with z.  The tables are the
 * caller's (ops.depth.bilateral_tables): where they leave den at 0 the result
 * is a NaN of unspecified payload.
 * Arguments: depth (0), B >= 1 (1), 1 <= H <= 16384 (2), 1 <= W <= 16384 (3),
 * w_space (4), r (5), w_range (6), sigma_depth > 0 finite (7), sigma_z2 >= 0
 * finite (8), depth_min not NaN (9), depth_max >= depth_min (10), filtered
 * [B,H,W], not depth (11).
 *
 * ucsa_depth_normals: per pixel (i, j) with depth z, P(i', j') the point of a
 * pixel with depth z':
 *   P = ((((float)j' + 0.5f) - cx) / fx) * z', ((((float)i' + 0.5f) - cy) / fy) * z', z'
 *   (utils/registration.backproject's expression and order).
 *   not measured: points = normals = 0, mask = 0.  Otherwise mask bit 1,
 *   points = p = P(i, j), thr = max_jump + max_jump_z2 * (z*z);
 *   a neighbour with depth z_n is usable iff measured and fabsf(z_n - z) <= thr;
 *   mask bit 4 (depth edge) iff one of the eight neighbours is measured and not
 *   usable;
 *   du = P(i,j+1) - P(i,j-1) when both are usable, else P(i,j+1) - p, else
 *   p - P(i,j-1), else there is no normal; dv likewise along i
 *   (P(i+1,j) - P(i-1,j), ...);
 *   c = dv x du = (dv1*du2 - dv2*du1, dv2*du0 - dv0*du2, dv0*du1 - dv1*du0);
 *   nn = (c0*c0 + c1*c1) + c2*c2; no normal unless nn > 0 and finite;
 *   n = c / sqrtf(nn); dot = (n0*p0 + n1*p1) + n2*p2; if dot > 0: n = -n,
 *   dot = -dot (the normal faces the camera at the origin);
 *   cosv = (-dot) / sqrtf((p0*p0 + p1*p1) + p2*p2);
 *   mask bit 2 (has a normal), bit 8 (grazing) iff cosv < min_cos;
 *   normals = n, or 0 without a normal.
 * Arguments: depth (0), B (1), H (2), W (3), fx > 0 finite (4), fy (5), cx
 * finite (6), cy (7), max_jump >= 0 finite (8), max_jump_z2 >= 0 finite (9),
 * -1 <= min_cos <= 1 (10), depth_min not NaN (11), depth_max >= depth_min (12),
 * points [B,H,W,3] (13), normals [B,H,W,3] (14), mask [B,H,W] uint8 (15).
 *
 * ucsa_depth_frontend: both in one launch.  filtered is ucsa_depth_filter's
 * output; points, normals and mask are ucsa_depth_normals' of it, with the same
 * depth_min / depth_max (with depth_min <= 0 the filter's 0 is a measurement
 * there, as it would be for the two calls); clean = 0 where mask & reject,
 * filtered elsewhere: an image ucsa_tsdf_integrate and the vote kernels take.
 * reject is a set of UCSA_DEPTH_EDGE | UCSA_DEPTH_GRAZING.  A work-group filters
 * its tile and a halo of one pixel (18 x 18) from a (18 + 2r)^2 load and keeps
 * the values in LDS; the five outputs are the bytes of the two calls.
 * Arguments: depth (0), B (1), H (2), W (3), w_space (4), r (5), w_range (6),
 * sigma_depth (7), sigma_z2 (8), fx (9), fy (10), cx (11), cy (12), max_jump
 * (13), max_jump_z2 (14), min_cos (15), reject (16), depth_min (17), depth_max
 * (18), filtered (19), clean (20), points (21), normals (22), mask (23).
 * An argument error returns UCSA_ERR_ARG - index before any launch.
 *
 * ucsa_depth_confidence: the weight of a pixel's measurement for
 * ucsa_tsdf_integrate_weighted, from the outputs of ucsa_depth_normals /
 * ucsa_depth_frontend: points [B,H,W,3], normals [B,H,W,3], mask [B,H,W] ->
 * weight [B,H,W] fp32.  A plain kernel, one thread per pixel, no LDS.  Per
 * pixel, with p the point, n the normal, m the mask:
 *   if !(m & MEASURED) or m & reject: w = 0 (reject a set of EDGE | GRAZING);
 *   z = p2; sigma = sigma_depth + sigma_z2 * (z*z); s = sigma_depth / sigma;
 *   wz = s*s  (the inverse variance of the filter's own noise model, relative
 *   to z = 0; exactly 1 with sigma_z2 = 0);
 *   if m & NORMAL: dot = (n0*p0 + n1*p1) + n2*p2;
 *     cosv = (-dot) / sqrtf((p0*p0 + p1*p1) + p2*p2)  (ucsa_depth_normals' own
 *     expression on the same operands: the same bits);
 *     wa = fminf(fmaxf(cosv, cos_floor), 1.0f); a NaN cosv gives cos_floor;
 *   without a normal: wa = cos_floor;
 *   w = wz * wa, in (0, 1] unless wz underflows.
 * Arguments: points (0), normals (1), mask (2), B >= 1 (3), 1 <= H <= 16384
 * (4), 1 <= W <= 16384 (5), sigma_depth > 0 finite (6), sigma_z2 >= 0 finite
 * (7), 0 < cos_floor <= 1 (8), reject within EDGE | GRAZING (9), weight
 * [B,H,W], sharing no byte with an input (10).
 *
 * ucsa_depth_pyramid_down: one level of the depth pyramid that coarse-to-fine
 * tracking runs on: depth [B,H,W] -> coarse [B,h,w] with h = ceil(H/2),
 * w = ceil(W/2).  A plain kernel, one thread per coarse pixel, no LDS.  Coarse
 * pixel (I, J) takes the block (2I, 2J), (2I, 2J+1), (2I+1, 2J), (2I+1, 2J+1)
 * in that (row-major) order, or what exists of it at an odd edge:
 *   z0 = the smallest measured depth of the block (found by `z < z0` in that
 *   order, so the first of equal ones); none measured: coarse = 0.  Otherwise
 *   thr = max_jump + max_jump_z2 * (z0*z0);  s = 0, count = 0;
 *   for each measured member z_k in that order: d = z_k - z0; taken iff
 *   d <= thr: s = s + d, count = count + 1  (z0's own 0 is taken);
 *   coarse = z0 + s / (float)count.
 * The foreground wins: a block straddling a depth edge returns the mean of its
 * near side and nothing is averaged across the edge.  The value is an offset
 * from z0, the filter's form: a constant block comes back with its own bits.
 * The coarse level's camera is fx/2, fy/2, cx/2, cy/2: exact under the +0.5
 * centre convention (coarse pixel J covers [2J, 2J+2) of the fine image).
 * Arguments: depth (0), B >= 1 (1), 1 <= H <= 16384 (2), 1 <= W <= 16384 (3),
 * max_jump >= 0 finite (4), max_jump_z2 >= 0 finite (5), depth_min not NaN
 * (6), depth_max >= depth_min (7), coarse [B,h,w], sharing no byte with depth
 * (8). */
#define UCSA_DEPTH_RANGE_BINS 256u
#define UCSA_DEPTH_MEASURED 1u
#define UCSA_DEPTH_NORMAL 2u
#define UCSA_DEPTH_EDGE 4u
#define UCSA_DEPTH_GRAZING 8u
int32_t ucsa_depth_filter(const float* depth, uint32_t B, uint32_t H, uint32_t W,
                          const float* w_space, uint32_t radius, const float* w_range,
                          float sigma_depth, float sigma_z2, float depth_min, float depth_max,
                          float* filtered, void* stream);
int32_t ucsa_depth_normals(const float* depth, uint32_t B, uint32_t H, uint32_t W, float fx,
                           float fy, float cx, float cy, float max_jump, float max_jump_z2,
                           float min_cos, float depth_min, float depth_max, float* points,
                           float* normals, uint8_t* mask, void* stream);
int32_t ucsa_depth_frontend(const float* depth, uint32_t B, uint32_t H, uint32_t W,
                            const float* w_space, uint32_t radius, const float* w_range,
                            float sigma_depth, float sigma_z2, float fx, float fy, float cx,
                            float cy, float max_jump, float max_jump_z2, float min_cos,
                            uint32_t reject, float depth_min, float depth_max, float* filtered,
                            float* clean, float* points, float* normals, uint8_t* mask,
                            void* stream);
int32_t ucsa_depth_confidence(const float* points, const float* normals, const uint8_t* mask,
                              uint32_t B, uint32_t H, uint32_t W, float sigma_depth,
                              float sigma_z2, float cos_floor, uint32_t reject, float* weight,
                              void* stream);
int32_t ucsa_depth_pyramid_down(const float* depth, uint32_t B, uint32_t H, uint32_t W,
                                float max_jump, float max_jump_z2, float depth_min,
                                float depth_max, float* coarse, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UCSA_HIP_H_ */
