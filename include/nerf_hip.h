/*
 * nerf_hip.h — C ABI of the MI355X (gfx950) NeRF training hot path.
 *
 * This is the drop-in boundary beneath the Python host package `noisy_src`
 * (robust-nerf_amd/noisy_src), which mirrors the reference package
 * ShawnnnLiu/Robust-NeRF `noisy_src/` (rays.py, model.py, rendering.py,
 * train_pose_opt.py, data_pose_opt.py).  The reference is pure PyTorch and has
 * no FFI of its own; every entry point below replaces the reference function
 * cited beside it, and the ctypes binding a maintainer would add is shown in
 * INTEGRATION.md.
 *
 * Contract shared by every entry point:
 *   - returns NR_OK (0) on success, a positive hipError_t on a HIP runtime
 *     failure, or NR_EARG on an argument error; nr_last_error() describes it;
 *   - all array pointers are CALLER-OWNED DEVICE pointers (PyTorch caching
 *     allocator); fp32 arrays are dense row-major exactly like the torch
 *     tensors of the reference ((..., 3) arrays are AoS);
 *   - no entry point allocates, frees or synchronises: kernels are enqueued on
 *     `stream` (the caller's torch.cuda.current_stream()), so calls can be
 *     captured into a hipGraph;
 *   - "nullable" pointers may be NULL to skip an optional input/output.
 */
#ifndef NERF_HIP_H
#define NERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NR_OK 0
#define NR_EARG (-22)

typedef void* nr_stream_t; /* a hipStream_t */

/* ---- library ----------------------------------------------------------- */
const char* nr_last_error(void);
int nr_abi_version(void);
/* Toolchain probe (no reference counterpart): out[i] = value + i. */
int nr_probe_fill(float* out, int n, float value, nr_stream_t stream);
/* Diagnostic: one MFMA tile, kind 0 = bf16 32x32x16 (A 32x16, B 16x32),
 * kind 1 = f32 32x32x2 (A 32x2, B 2x32); D (32,32) row-major = A @ B. */
int nr_probe_mfma(int kind, const float* A, const float* B, float* D,
                  nr_stream_t stream);

/* ---- A1: get_ray_directions  (noisy_src/rays.py:17-64) ------------------
 * dirs (H,W,3): ((i-cx)/focal, -(j-cy)/focal, -1), meshgrid indexing='xy'. */
int nr_ray_directions(int H, int W, float focal, float cx, float cy,
                      float* dirs, nr_stream_t stream);

/* ---- A2: get_rays  (noisy_src/rays.py:67-99) -----------------------------
 * dirs (N,3), c2w (4,4) -> rays_o (N,3) = t, rays_d (N,3) = normalize(R d). */
int nr_get_rays(const float* dirs, const float* c2w, int64_t N,
                float* rays_o, float* rays_d, nr_stream_t stream);
/* Backward of get_rays (the reference's is differentiable in c2w and dirs):
 * g_c2w (4,4) ACCUMULATED (caller zeroes), rows 0..2 / cols 0..3 (R and t);
 * g_dirs (N,3) OVERWRITTEN, nullable; g_rays_o / g_rays_d nullable (not both;
 * g_dirs needs g_rays_d).  Fixed-order reduction over the N rays through
 * nr_get_rays_bwd_workspace_bytes() of scratch.                             */
int64_t nr_get_rays_bwd_workspace_bytes(void);
int nr_get_rays_bwd(const float* dirs, const float* c2w, int64_t N,
                    const float* g_rays_o, const float* g_rays_d,
                    float* g_dirs, float* g_c2w, void* workspace,
                    nr_stream_t stream);

/* ---- A3: PixelDataset.get_rays_from_pixels  (noisy_src/data_pose_opt.py:83-148,
 *          PixelSampler.get_rays_for_batch :200-223) ---------------------
 * One pass over the batch, no per-image host loop.  img_idx (B,) int64,
 * pix (B,2) fp32 (u,v) pixel coords, poses (n_img,4,4) indexed by img_idx.
 * Validating mode: bad_index (nullable, one device int the caller zeroes) is
 * set to 1 when any img_idx lies outside [0, n_img) -- the reference's
 * poses[idx] raises IndexError there (data_pose_opt.py:105-148); the entry
 * point stays asynchronous (graph-capturable), so the host wrapper reads the
 * flag and raises.  Such rays come out NaN either way.                      */
int nr_rays_from_pixels_fwd(const int64_t* img_idx, const float* pix,
                            const float* poses, int n_img, int H, int W,
                            float focal, int B, float* rays_o, float* rays_d,
                            int* bad_index, nr_stream_t stream);
/* Backward: g_poses (n_img,4,4) must be zeroed by the caller; it receives
 * dL/dposes summed over the pixels of each image (g_rays_d nullable).  One
 * workgroup per image sums its rays in a fixed order: no atomics, the result is
 * bit-identical from run to run.  Rays whose img_idx is outside [0, n_img)
 * contribute nothing (the forward writes NaN rays for them); callers that take
 * indices from outside validate them with nr_check_index_range.            */
int nr_rays_from_pixels_bwd(const int64_t* img_idx, const float* pix,
                            const float* poses, int n_img, int H, int W,
                            float focal, int B, const float* g_rays_o,
                            const float* g_rays_d, float* g_poses,
                            nr_stream_t stream);
/* ---- A1 / A3 with learned intrinsics (no reference counterpart; its
 *          POSE_OPTIMIZATION.md lists focal-length optimisation as future work)
 * nr_ray_directions with a focal length per axis (the same kernel; it passes
 * focal twice): dirs (H,W,3) = ((i-cx)/fx, -(j-cy)/fy, -1).                 */
int nr_ray_directions_xy(int H, int W, float fx, float fy, float cx, float cy,
                         float* dirs, nr_stream_t stream);
/* nr_rays_from_pixels_fwd with fxy = {fx, fy}, two floats in DEVICE memory
 * read when the kernel runs (a captured graph sees the current value):
 * dx = (u - W/2)/fx, dy = -((v - H/2)/fy).  Both entries run one kernel body
 * (the focal pair an argument there, a load here), so with fx == fy == focal
 * the rays are those of nr_rays_from_pixels_fwd bit for bit; out-of-range
 * img_idx and bad_index behave as there.  An empty batch (B == 0) may come
 * with null arrays here, not there.                                          */
int nr_rays_from_pixels_intr_fwd(const int64_t* img_idx, const float* pix,
                                 const float* poses, int n_img, int H, int W,
                                 const float* fxy, int B, float* rays_o,
                                 float* rays_d, int* bad_index,
                                 nr_stream_t stream);
/* Backward of the above: the kernel body of nr_rays_from_pixels_bwd with two
 * more rows in its reduction.  g_poses exactly as there (ACCUMULATED, caller
 * zeroes; each row is reduced on its own, so the same bits when fx == fy).
 * g_fxy (2 floats) is WRITTEN: dL/dfx, dL/dfy summed over the batch, 0 when
 * g_rays_d is NULL or B == 0.  Each image's workgroup carries the two sums
 * through its fixed tree into workspace ((n_img,2) floats,
 * nr_..._workspace_bytes(n_img), fully overwritten); a second one-workgroup
 * launch, made for an empty batch too, adds them over the images in a fixed
 * order.  No atomics; rays with an out-of-range img_idx contribute nothing.  */
int64_t nr_rays_from_pixels_intr_bwd_workspace_bytes(int n_img);
int nr_rays_from_pixels_intr_bwd(const int64_t* img_idx, const float* pix,
                                 const float* poses, int n_img, int H, int W,
                                 const float* fxy, int B, const float* g_rays_o,
                                 const float* g_rays_d, float* g_poses,
                                 float* g_fxy, void* workspace,
                                 nr_stream_t stream);
/* ---- A1 / A3 with a learned lens (no reference counterpart; the other half
 *          of the same future-work bullet).  A lens is six floats
 *          {fx, fy, cx, cy, k1, k2}, the NeRF-- / SCNeRF form: the radial
 *          polynomial acts on the ray side, so it is closed form.  For the
 *          truncated pixel (u, v), every operation fp32 and rounded once:
 *            xn = (u - cx)/fx,  yn = (v - cy)/fy,  r2 = xn*xn + yn*yn,
 *            s = 1 + r2*(k1 + k2*r2),  d = (xn*s, -(yn*s), -1),
 *          then R d, normalised, as everywhere.  k1 == k2 == 0 makes s exactly
 *          1 and xn*1 == xn, so with cx = W/2, cy = H/2 the rays are those of the
 *          _intr_ entries (and of the fixed-focal ones when fx == fy) bit for
 *          bit: all three run one kernel body.
 * nr_ray_directions_lens: the direction table under that model, from host
 * numbers (the evaluation path); the same kernel as nr_ray_directions[_xy],
 * which pass k1 = k2 = 0, so equal to _xy bit for bit at k = 0.             */
int nr_ray_directions_lens(int H, int W, float fx, float fy, float cx, float cy,
                           float k1, float k2, float* dirs, nr_stream_t stream);
/* nr_rays_from_pixels_intr_fwd with lens = six floats in DEVICE memory, read
 * when the kernel runs (a captured graph sees the current value).  bad_index,
 * NaN rays for an out-of-range img_idx and B == 0 (null arrays allowed) as
 * there.                                                                     */
int nr_rays_from_pixels_lens_fwd(const int64_t* img_idx, const float* pix,
                                 const float* poses, int n_img, int H, int W,
                                 const float* lens, int B, float* rays_o,
                                 float* rays_d, int* bad_index,
                                 nr_stream_t stream);
/* Backward of the above: the kernel body of nr_rays_from_pixels_bwd with six
 * more rows (18 in all) in its reduction.  g_poses exactly as there
 * (ACCUMULATED, caller zeroes; each row is reduced on its own, so the
 * fixed-focal bits at the neutral lens).  g_lens (6 floats) is WRITTEN:
 * dL/d{fx, fy, cx, cy, k1, k2} summed over the batch, exact zeros when
 * g_rays_d is NULL or B == 0.  Each image's workgroup carries its six sums
 * through the fixed tree into workspace ((n_img,6) floats,
 * nr_..._workspace_bytes(n_img) = n_img*6*4, fully overwritten: an image
 * without rays writes exact zeros, so no initialisation); a second
 * one-workgroup launch, made for an empty batch too, adds them over the images
 * in the order of the _intr_ entry's.  No atomics, the same bits from run to
 * run; rays with an out-of-range img_idx contribute nothing.                 */
int64_t nr_rays_from_pixels_lens_bwd_workspace_bytes(int n_img);
int nr_rays_from_pixels_lens_bwd(const int64_t* img_idx, const float* pix,
                                 const float* poses, int n_img, int H, int W,
                                 const float* lens, int B, const float* g_rays_o,
                                 const float* g_rays_d, float* g_poses,
                                 float* g_lens, void* workspace,
                                 nr_stream_t stream);
/* flag[0] = 1 if any idx[i] (i < n) lies outside [0, limit); flag untouched
 * otherwise (caller zeroes it).  Validation for host wrappers that receive
 * indices from a user (the reference raises IndexError on them).            */
int nr_check_index_range(const int64_t* idx, int n, int limit, int* flag,
                         nr_stream_t stream);

/* ---- A4: CameraPoseParameters.get_poses  (noisy_src/train_pose_opt.py:122-226)
 * poses_out[i] = [[R_delta(rot[idx_i]) @ R_init[idx_i], t_init[idx_i] + trans[idx_i]],
 *                 [0 0 0 1]], with the reference's theta < 1e-6 -> I rule
 * (train_pose_opt.py:143-144,161).  rot / trans / indices nullable.        */
int nr_se3_poses_fwd(const float* init_poses, const float* rot_deltas,
                     const float* trans_deltas, const int64_t* indices, int n,
                     float* poses_out, nr_stream_t stream);
/* Backward of the above.  g_rot / g_trans (n_poses,3) are ACCUMULATED (indices
 * may repeat; each pose sums its rows in row order, deterministically); the
 * caller zeroes them.  At theta < 1e-6 dL/drot is exactly 0, as in the
 * reference (the torch.where blocks the gradient). fixed_small_angle != 0
 * selects the first-order small-angle Jacobian instead (non-default flag).  */
int nr_se3_poses_bwd(const float* init_poses, const float* rot_deltas,
                     const int64_t* indices, int n, int n_poses,
                     const float* g_poses,
                     int fixed_small_angle, float* g_rot, float* g_trans,
                     nr_stream_t stream);

/* ---- batch assembly: RaySampler  (noisy_src/data.py:264-321) -----------
 * out_*[b] = table_*[idx[b]] for the (n_rays,3) ray table (rays_o, rays_d,
 * colors) in one launch; idx outside [0, n_rays) gives NaN rows and, in the
 * validating mode (bad_index non-NULL, caller-zeroed device int), sets
 * *bad_index = 1 for the host wrapper to raise IndexError (torch indexing in
 * the reference's data.py:305-309 raises).                                   */
int nr_gather_rays(const int64_t* idx, int64_t n_rays, int B,
                   const float* rays_o, const float* rays_d, const float* colors,
                   float* out_o, float* out_d, float* out_rgb, int* bad_index,
                   nr_stream_t stream);

/* ---- batch assembly: PixelSampler.sample_batch  (noisy_src/data_pose_opt.py:178-198)
 * For the flat pixel index idx[b] into images (n_img,H,W,3): out_img[b] =
 * idx / (H*W), out_pix[b] = (u, v) = (idx % W, (idx % (H*W)) / W) as fp32,
 * out_rgb[b] = images[idx] -- the reference's image_indices / pixel_coords /
 * target_rgb tables without the two n_pixels-long tables.  64-bit index
 * arithmetic (n_img*H*W may exceed 2^31).  idx outside [0, n_img*H*W) gives
 * NaN pix / rgb rows and out_img = -1 and, in the validating mode (bad_index
 * non-NULL, caller-zeroed device int), sets *bad_index = 1.                  */
int nr_gather_pixels(const int64_t* idx, int n_img, int H, int W,
                     const float* images, int B, int64_t* out_img,
                     float* out_pix, float* out_rgb, int* bad_index,
                     nr_stream_t stream);

/* ---- A5: sample_along_rays  (noisy_src/rays.py:145-210) ------------------
 * z (B,N); pts (B,N,3) nullable.  t_rand (B,N) nullable -> no perturbation.
 * viewdirs (B*N,3) nullable: rays_d / |rays_d| per sample (rendering.py:165), as
 * nr_expand_viewdirs writes it.                                               */
int nr_stratified_sample(const float* rays_o, const float* rays_d,
                         const float* t_rand, float near_, float far_,
                         int lindisp, int B, int N, float* z_vals, float* pts,
                         float* viewdirs, nr_stream_t stream);

/* ---- A6: PositionalEncoding.forward  (noisy_src/model.py:58-80) ----------
 * x (M,C) -> out (M, C*(include_input + 2L)) laid out [x | sin f0x | cos f0x | ...]. */
int nr_positional_encoding(const float* x, int64_t M, int C, int num_freqs,
                           int include_input, int log_sampling, float* out,
                           nr_stream_t stream);
int nr_positional_encoding_bwd(const float* x, int64_t M, int C, int num_freqs,
                               int include_input, int log_sampling,
                               const float* g_out, float* g_x,
                               nr_stream_t stream);
/* The windowed encoding (no reference counterpart; additive to ABI 5): frequency
 * k's sin and cos columns times w[k]; the raw input columns are not weighted.
 * w: num_freqs floats in DEVICE memory, read by the kernel (capturable; a replay
 * sees the values of its time), nullable = all ones: the plain entry points
 * above launch these kernels with w null, so the two agree bit for bit.      */
int nr_positional_encoding_windowed(const float* x, int64_t M, int C,
                                    int num_freqs, int include_input,
                                    int log_sampling, const float* w,
                                    float* out, nr_stream_t stream);
int nr_positional_encoding_windowed_bwd(const float* x, int64_t M, int C,
                                        int num_freqs, int include_input,
                                        int log_sampling, const float* w,
                                        const float* g_out, float* g_x,
                                        nr_stream_t stream);

/* ---- A9: sample_pdf  (noisy_src/rays.py:213-279) -------------------------
 * bins (B,Nb), weights (B,Nb-1), u (B,Ns) nullable -> det=True linspace(0,1).
 * samples (B,Ns) in the order of u.  Nb <= 4097 (above 513 bins a ray takes a
 * workgroup of its own); a larger Nb is NR_EARG.                             */
int nr_sample_pdf(const float* bins, const float* weights, const float* u,
                  int B, int Nb, int Ns, float* samples, nr_stream_t stream);

/* ---- A10: sample_hierarchical  (noisy_src/rays.py:282-333) ---------------
 * z_coarse (B,Nc), w_coarse (B,Nc) -> z_fine (B,Nc+Nf) = sort(cat(z, sample_pdf(
 * mid(z), w[:,1:-1], Nf, det))), pts_fine (B,Nc+Nf,3) nullable.  u nullable=det.
 * viewdirs (B*(Nc+Nf),3) nullable, as in nr_stratified_sample.  z_coarse may be
 * in any order.  Nc + Nf <= 4096 (above 512 a ray takes a workgroup of its own
 * and is sorted in runs of 512); a larger sum is NR_EARG.                     */
int nr_sample_hierarchical(const float* rays_o, const float* rays_d,
                           const float* z_coarse, const float* w_coarse,
                           const float* u, int B, int Nc, int Nf,
                           float* z_fine, float* pts_fine, float* viewdirs,
                           nr_stream_t stream);

/* ---- A8: raw2outputs  (noisy_src/rendering.py:20-116) --------------------
 * rgb (B,S,3), sigma (B,S), z (B,S), rays_d (B,3), sigma_noise (B,S) nullable
 * (already scaled by raw_noise_std) -> rgb_map (B,3), depth (B), acc (B),
 * weights (B,S).                                                           */
int nr_composite_fwd(const float* rgb, const float* sigma, const float* z,
                     const float* rays_d, const float* sigma_noise, int B,
                     int S, int white_bg, float* rgb_map, float* depth_map,
                     float* acc_map, float* weights, nr_stream_t stream);
/* Backward: g_depth / g_acc / g_weights nullable (zero); g_rays_d nullable
 * (ACCUMULATED: dL/drays_d through dists * |rays_d|). */
int nr_composite_bwd(const float* rgb, const float* sigma, const float* z,
                     const float* rays_d, const float* sigma_noise, int B,
                     int S, int white_bg, const float* g_rgb_map,
                     const float* g_depth, const float* g_acc,
                     const float* g_weights, float* g_rgb, float* g_sigma,
                     float* g_rays_d, nr_stream_t stream);

/* ---- A7: NeRF MLP  (noisy_src/model.py:83-221) ---------------------------
 * Parameters live in one flat fp32 buffer in nn.Module.parameters() order:
 * pts_linears.{0..L-1}.{weight,bias}, sigma_linear, feature_linear,
 * dir_linear, rgb_linear (weights (out,in) row-major, as nn.Linear).       */
typedef struct NrMlpConfig {
    int pos_freqs;      /* ModelConfig.pos_freqs (10)          */
    int dir_freqs;      /* ModelConfig.dir_freqs (4)           */
    int hidden;         /* ModelConfig.hidden_dim (256)        */
    int n_layers;       /* ModelConfig.num_hidden_layers (8)   */
    uint32_t skip_mask; /* bit i set <=> i in ModelConfig.skips */
    int use_view_dirs;  /* ModelConfig.use_view_dirs (1)       */
    int precision;      /* NR_PREC_FP32 / NR_PREC_BF16         */
    int dense_backward; /* 0: the backward skips 32-sample tiles whose incoming
                           gradient (g_rgb, g_sigma) is exactly zero; nonzero:
                           every tile (the dense reference form)          */
} NrMlpConfig;

#define NR_PREC_FP32 0
#define NR_PREC_BF16 1
#define NR_PREC_FP16 2  /* cfg #5: fp16 MFMA operands, fp32 accumulate, 2^14 backward loss scale */

/* Sizes (bytes unless stated).  M = number of samples. */
int64_t nr_mlp_param_count(const NrMlpConfig* cfg);
int64_t nr_mlp_packed_bytes(const NrMlpConfig* cfg);
int64_t nr_mlp_saved_bytes(const NrMlpConfig* cfg, int64_t M);
int64_t nr_mlp_workspace_bytes(const NrMlpConfig* cfg, int64_t M);

/* Re-pack the flat fp32 parameters into the MFMA fragment images used by the
 * forward (W) and backward (W^T) kernels.  Call after every optimizer step. */
int nr_mlp_pack(const NrMlpConfig* cfg, const float* params, void* packed,
                nr_stream_t stream);

/* Coarse-to-fine positional encoding (no reference counterpart; additive to ABI 5).
 * A window puts a weight on every frequency of the two encoders the MLP fuses:
 * gamma_w(x) = [x | w_0 sin x, w_0 cos x | ... | w_{L-1} sin 2^{L-1} x, w_{L-1} cos ..].
 * w_pos (pos_freqs floats) and w_dir (dir_freqs floats; NULL without
 * use_view_dirs) are DEVICE pointers read inside the kernels, each nullable =
 * all ones.  No allocation, no synchronisation: both calls are capturable.
 *
 * nr_mlp_fold_window: W . (s * gamma) = (W * s) . gamma, so the window is folded
 * into the images: every element of the W and W^T images that holds an encoding
 * column of layer 0, of the layer after each skip, or of dir_linear is rewritten
 * as convert(params[row, col] * s(col)), s = 1 on the 3 raw columns and
 * w[(c - 3) / 6] on encoding column c, by the index maps and conversions of
 * nr_mlp_pack.  The forward and the input gradients then are the windowed
 * network's.  With all-ones weights packed is left byte-identical to nr_mlp_pack's.
 * nr_mlp_pack and a nr_adam_multi refresh write those elements unfolded again.
 *
 * nr_mlp_window_grad: the backward on folded images leaves dL/d(W * s) in
 * g_params; this multiplies the same columns by s(col) in place, giving dL/dW
 * (exactly zero where w_k = 0).                                              */
int nr_mlp_fold_window(const NrMlpConfig* cfg, const float* params,
                       const float* w_pos, const float* w_dir, void* packed,
                       nr_stream_t stream);
int nr_mlp_window_grad(const NrMlpConfig* cfg, const float* w_pos,
                       const float* w_dir, float* g_params, nr_stream_t stream);

/* Forward: x (M,3) positions, d (M,3) view directions -> rgb (M,3) in [0,1],
 * sigma (M) >= 0.  saved (nr_mlp_saved_bytes) nullable: inference only.   */
int nr_mlp_forward(const NrMlpConfig* cfg, const void* packed,
                   const float* params, const float* x, const float* d,
                   int64_t M, float* rgb, float* sigma, void* saved,
                   nr_stream_t stream);

/* Backward: g_rgb (M,3), g_sigma (M) -> g_params (flat, OVERWRITTEN),
 * g_x (M,3) / g_d (M,3) nullable (OVERWRITTEN).  Needs the forward's
 * `saved` and rgb/sigma outputs, and nr_mlp_workspace_bytes of workspace.
 * Runs the split form: nr_mlp_backward_dx, _dw, _reduce.                    */
int nr_mlp_backward(const NrMlpConfig* cfg, const void* packed,
                    const float* params, const float* x, const float* d,
                    int64_t M, const float* rgb, const float* sigma,
                    const void* saved, const float* g_rgb,
                    const float* g_sigma, float* g_params, float* g_x,
                    float* g_d, void* workspace, nr_stream_t stream);

/* The three stages of nr_mlp_backward, callable separately (per-kernel timing):
 * dx: the list of ACTIVE 32-sample tiles (any nonzero g_rgb / g_sigma entry;
 * every tile with cfg->dense_backward) and the dz of every layer for them into
 * the workspace (+ g_x / g_d, zero for inactive samples); dw: per-chunk dW/db
 * slabs from the saved activations and dz of the active tiles, split over the
 * chunks in list order; reduce: slabs -> g_params (chunk order, deterministic).
 * A tile whose incoming gradient is exactly zero has dz == 0 in every layer, so
 * skipping it drops only exact-zero terms; when every tile is active the result
 * is bit-identical to the dense form.  Same arguments and workspace as
 * nr_mlp_backward; dw must follow dx on the same workspace.                 */
int nr_mlp_backward_dx(const NrMlpConfig* cfg, const void* packed,
                       const float* params, const float* x, const float* d,
                       int64_t M, const float* rgb, const float* sigma,
                       const void* saved, const float* g_rgb,
                       const float* g_sigma, float* g_x, float* g_d,
                       void* workspace, nr_stream_t stream);
int nr_mlp_backward_dw(const NrMlpConfig* cfg, int64_t M, const void* saved,
                       void* workspace, nr_stream_t stream);
int nr_mlp_backward_reduce(const NrMlpConfig* cfg, int64_t M,
                           const void* workspace, float* g_params,
                           nr_stream_t stream);
/* Byte offset in the workspace of the uint32 count of active tiles that
 * nr_mlp_backward_dx wrote (of ceil(M / 32)), or -1: the work the backward ran. */
int64_t nr_mlp_active_tiles_offset(const NrMlpConfig* cfg, int64_t M);

/* Frozen field (additive to ABI 5): the input gradients of a network whose
 * parameters get no gradient -- a pose step against a fixed field.  The pair
 * computes rgb / sigma and g_x / g_d bit-identical to nr_mlp_forward (with
 * saved) and nr_mlp_backward_dx: the same products in the same order.  No
 * parameter gradient, no dW list or count.  Caller-owned buffers, no allocation,
 * no synchronisation, capturable.
 *   bf16 / fp16: the forward keeps only the ReLU masks (ceil(M / 32) * (n_layers
 *     + 1) KB: 288 B per sample for the default model, against about 5.3 KB), and
 *     the backward stores only the dz images the input gradients read (layer 0,
 *     the layer after each skip, dir_linear: 1.28 KB of about 4.9 KB per sample).
 *   fp32 (parity mode, not the fast one): the backward reads the activations, so
 *     both buffers have the training sizes and layout and the pair is
 *     nr_mlp_forward + nr_mlp_backward_dx.
 * saved_frozen and this workspace have layouts of their own (csrc/mlp_plan.hpp,
 * FrozenSizes): a saved_frozen buffer must not be given to nr_mlp_backward_dx /
 * _dw / nr_mlp_backward, nor a `saved` buffer of nr_mlp_forward to
 * nr_mlp_backward_input.  Neither can be checked at run time.
 * g_x / g_d: each nullable, OVERWRITTEN (exact zeros for the samples of tiles
 * without incoming gradient, unless cfg->dense_backward).  M == 0: NR_OK.        */
int64_t nr_mlp_frozen_saved_bytes(const NrMlpConfig* cfg, int64_t M);
int64_t nr_mlp_frozen_workspace_bytes(const NrMlpConfig* cfg, int64_t M);
int nr_mlp_forward_frozen(const NrMlpConfig* cfg, const void* packed,
                          const float* params, const float* x, const float* d,
                          int64_t M, float* rgb, float* sigma,
                          void* saved_frozen, nr_stream_t stream);
int nr_mlp_backward_input(const NrMlpConfig* cfg, const void* packed,
                          const float* params, const float* x, const float* d,
                          int64_t M, const float* rgb, const float* sigma,
                          const void* saved_frozen, const float* g_rgb,
                          const float* g_sigma, float* g_x, float* g_d,
                          void* workspace, nr_stream_t stream);

/* ---- A13: optimizer tail  (noisy_src/train.py:112-117, train_pose_opt.py:398-409)
 * Sum of squares of n fp32 values added into *acc (device scalar, caller-zeroed):
 * the squared global norm of torch.nn.utils.clip_grad_norm_.  A fixed-shape
 * two-pass reduction (deterministic) through nr_sumsq_workspace_bytes() of
 * caller-owned scratch; calls on one stream may share the scratch.          */
int64_t nr_sumsq_workspace_bytes(void);
int nr_sumsq(const float* x, int64_t n, float* acc, void* workspace,
             nr_stream_t stream);
/* torch.optim.Adam (amsgrad=False, maximize=False, weight_decay=0) on a flat
 * buffer: grads are first scaled by clip = min(1, max_norm / (sqrt(*sumsq)
 * + 1e-6)) when sumsq != NULL (torch.nn.utils.clip_grad_norm_), lr is read
 * from the host (LambdaLR already applied), step is the 1-based Adam step. */
int nr_adam_step(float* params, float* grads, float* exp_avg,
                 float* exp_avg_sq, int64_t n, double lr, double beta1,
                 double beta2, double eps, int64_t step, const float* sumsq,
                 float max_norm, nr_stream_t stream);

/* The fused optimizer tail of one training step (train.py:112-117: clip_grad_norm_
 * + optimizer.step(); train_pose_opt.py:398-409 with one clip per network), in two
 * launches however many flat buffers it covers, and without the re-pack after it:
 *
 * nr_sumsq_partials: the nr_sumsq_workspace_bytes() of fixed-order partial sums of
 * squares over the concatenation of nspan (<= 8) fp32 buffers (one clip group),
 * written to `partials` (OVERWRITTEN; no caller-zeroed accumulator).          */
int nr_sumsq_partials(const float* const* xs, const int64_t* ns, int nspan,
                      float* partials, nr_stream_t stream);
/* One flat buffer of nr_adam_multi.  sumsq_partials (nullable: no clip) is the
 * nr_sumsq_partials output of the buffer's clip group, whose grads are scaled by
 * min(1, max_norm / (sqrt(sum) + 1e-6)) as nr_adam_step does.  pack_table
 * (nullable) refreshes the MFMA images `packed` of an MLP whose flat parameters
 * are `params`: every updated parameter is written, converted as nr_mlp_pack
 * converts it, to each image position the table lists, so `packed` equals
 * nr_mlp_pack(params) afterwards when it did before (bit-identical).          */
typedef struct NrAdamSpan {
    float* params;
    float* grads;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    const float* sumsq_partials;
    float max_norm;
    const uint32_t* pack_table;
    void* packed;
} NrAdamSpan;
/* torch.optim.Adam over nspan (<= 8) buffers of one param group (same lr and
 * 1-based step), one launch.  sched (nullable, device): {lr / (1 - beta1^step),
 * sqrt(1 - beta2^step)} as fp32, read by the kernel instead of the host lr/step,
 * so a captured hipGraph of the step can be replayed with the schedule advanced
 * by a 8-byte copy (lr / step then only validate).                          */
int nr_adam_multi(const NrAdamSpan* spans, int nspan, double lr, double beta1,
                  double beta2, double eps, int64_t step, const float* sched,
                  nr_stream_t stream);
/* The destination table of an MLP's packed images for nr_adam_multi: for each
 * of the nr_mlp_param_count() flat parameters, 3 slots of (kind << 29 | byte
 * offset in packed), slot-major (table[s * n + i]); built once per config by
 * the index maps of nr_mlp_pack itself.                                     */
int64_t nr_mlp_pack_table_bytes(const NrMlpConfig* cfg);
int nr_mlp_pack_table(const NrMlpConfig* cfg, uint32_t* table,
                      nr_stream_t stream);

/* ---- per-ray glue used by render_rays (rendering.py:119-240) ------------ */
/* viewdirs = d/|d| broadcast to every sample: out (B*S,3). */
int nr_expand_viewdirs(const float* rays_d, int B, int S, float* out,
                       nr_stream_t stream);
/* g_rays_o[b] += sum_s g_pts[b,s]; g_rays_d[b] += sum_s g_pts[b,s]*z[b,s]
 * (pts = o + d z, rays.py:208/331).  Either output nullable. */
int nr_pts_bwd(const float* g_pts, const float* z, int B, int S,
               float* g_rays_o, float* g_rays_d, nr_stream_t stream);
/* g_rays_d[b] += d(viewdir)/d(rays_d)^T sum_s g_viewdirs[b,s] (rendering.py:165). */
int nr_viewdirs_bwd(const float* rays_d, const float* g_viewdirs, int B,
                    int S, float* g_rays_d, nr_stream_t stream);
/* loss = mean((pred - target)^2) over B*3; g_pred = 2/(3B) (pred-target)*scale;
 * loss_out (device scalar, OVERWRITTEN) may be NULL. */
int nr_mse_fwd_bwd(const float* pred, const float* target, int B, float scale,
                   float* loss_out, float* g_pred, nr_stream_t stream);
/* The training form of raw2outputs + the MSE loss (rendering.py:20-116 then
 * train.py:89/98): the composite forward (outputs as nr_composite_fwd), the loss
 * (device scalar, OVERWRITTEN) against target (B,3), and the backward of
 * grad_scale * loss (g_rgb, g_sigma OVERWRITTEN; g_rays_d nullable, ACCUMULATED) in one
 * wave per ray -- gradients bit-identical to nr_composite_fwd, nr_mse_fwd_bwd and
 * nr_composite_bwd in sequence.  ticket (nullable): a device uint32 that is 0 before
 * the call and is left 0; with it (and B <= 1024) the launch's last workgroup sums the
 * loss, otherwise a second launch does.  Calls sharing a ticket must not run concurrently.
 * workspace: nr_composite_mse_workspace_bytes(B).                                 */
int64_t nr_composite_mse_workspace_bytes(int B);
int nr_composite_mse(const float* rgb, const float* sigma, const float* z,
                     const float* rays_d, const float* sigma_noise,
                     const float* target, int B, int S, int white,
                     float grad_scale, float* rgb_map, float* depth_map,
                     float* acc_map, float* weights, float* loss, float* g_rgb,
                     float* g_sigma, float* g_rays_d, uint32_t* ticket,
                     void* workspace, nr_stream_t stream);

/* ---- robust photometric losses  (no reference counterpart; additive to ABI 5)
 * Per colour channel: d = pred - target, a scale c > 0 in colour units, q = (d/c)^2.
 * The loss is the mean of rho(d) over the 3B channels; every rho is normalised so that
 * rho ~ d^2 for |d| << c (c -> inf is the MSE), and rho' = 2 d w(d):
 *   NR_LOSS_MSE            rho = d^2                            w = 1
 *   NR_LOSS_HUBER          rho = d^2 (|d| <= c), 2c|d| - c^2    w = 1 (|d| <= c), c/|d|
 *   NR_LOSS_CHARBONNIER    rho = 2 d^2 / (1 + sqrt(1 + q))      w = 1/sqrt(1 + q)
 *                          (= 2c^2 (sqrt(1 + q) - 1) without the cancellation)
 *   NR_LOSS_CAUCHY         rho = c^2 log1p(q)                   w = 1/(1 + q)
 *   NR_LOSS_GEMAN_MCCLURE  rho = d^2 / (1 + q)                  w = 1/(1 + q)^2
 * fp32 operation order, every operation rounded once (no contraction; / and sqrt
 * correctly rounded):  d2 = d*d, u = d/c, q = u*u;
 *   huber  a = |d|; a <= c: rho = d2, w = 1.0f; else rho = (2c)*a - c*c, w = c/a
 *   charbonnier  s = sqrtf(1 + q); rho = (2*d2)/(1 + s); w = 1/s
 *   cauchy  rho = (c*c)*log1pf(q); w = 1/(1 + q)
 *   geman_mcclure  t = 1 + q; rho = d2/t; w = 1/(t*t)
 * and the gradient is nr_mse_fwd_bwd's ((2*d)*(1/3B)*scale) times w -- for huber with
 * |d| <= c, and for mse, the MSE's bits.  A ray's three rho are added as (r + g) + b.
 *
 * nr_robust_fwd_bwd is nr_mse_fwd_bwd for the family: loss2 (device, 2 floats,
 * OVERWRITTEN, nullable) = {mean rho, mean d^2}, each summed in nr_mse_fwd_bwd's order;
 * g_pred (B,3, nullable) = scale * d(mean rho)/d pred.
 *
 * nr_composite_robust is nr_composite_mse with the family's seed: the same contract
 * (outputs, nullable / OVERWRITTEN / ACCUMULATED buffers, B > 0, ticket rules, one wave
 * per ray up to 512 samples and the three separate passes beyond), plus kind and c, and
 * loss2 = {mean rho, mean d^2} in place of the scalar loss: the second word is the plain
 * MSE whatever is being minimised.  Gradients are bit-identical to nr_composite_fwd,
 * nr_robust_fwd_bwd and nr_composite_bwd in sequence; with NR_LOSS_MSE every output is
 * nr_composite_mse's and loss2[0] == loss2[1].  workspace:
 * nr_composite_robust_workspace_bytes(B) = 20 B bytes, no initialisation needed:
 * floats [0, B) rho per ray, [B, 2B) squared error per ray, [2B, 5B) the seed gradient
 * of the long-ray form.  No float atomics: bit-identical from run to run.
 * NR_EARG: kind outside the enum, c not finite or <= 0 (also under NR_LOSS_MSE, which
 * does not read it), and the null and size cases of nr_mse_fwd_bwd / nr_composite_mse. */
enum {
    NR_LOSS_MSE = 0,
    NR_LOSS_HUBER,
    NR_LOSS_CHARBONNIER,
    NR_LOSS_CAUCHY,
    NR_LOSS_GEMAN_MCCLURE
};
int nr_robust_fwd_bwd(const float* pred, const float* target, int B, int kind,
                      float c, float scale, float* loss2, float* g_pred,
                      nr_stream_t stream);
int64_t nr_composite_robust_workspace_bytes(int B);
int nr_composite_robust(const float* rgb, const float* sigma, const float* z,
                        const float* rays_d, const float* sigma_noise,
                        const float* target, int B, int S, int white, int kind,
                        float c, float grad_scale, float* rgb_map,
                        float* depth_map, float* acc_map, float* weights,
                        float* loss2, float* g_rgb, float* g_sigma,
                        float* g_rays_d, uint32_t* ticket, void* workspace,
                        nr_stream_t stream);

/* ---- distortion regulariser on the ray weights  (no reference counterpart;
 *      mip-NeRF 360 eq. 15; additive to ABI 5) -------------------------------
 * weights, z (B,S): a ray's compositing weights and its sample depths, which
 * must be nondecreasing and lie in [near, far] (preconditions, not checked).
 *   s_i = (z_i - near)/(far - near), e_i = s_i (i < S), e_S = 1 (the last
 *   interval is closed at far), m_i = (e_i + e_{i+1})/2, d_i = e_{i+1} - e_i
 *   L = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
 * loss (device scalar, OVERWRITTEN): the mean of L over the B rays, without
 * grad_scale.  loss_rays (B), nullable: L per ray.  g_weights (B,S), nullable,
 * OVERWRITTEN: grad_scale * d(mean L)/d weights (a buffer of its own, not one
 * of the inputs); z gets no gradient.  One wave
 * per ray for every S (two passes over the ray, prefix sums in fp64), then a
 * one-workgroup launch for the mean in a fixed order: no atomics, bit-identical
 * from run to run.  workspace: nr_distortion_workspace_bytes(B), no
 * initialisation needed.  NR_EARG for B < 1, S < 1, S > 4096, far <= near or a
 * null weights, z, loss or workspace.                                        */
int64_t nr_distortion_workspace_bytes(int B);
int nr_distortion_loss(const float* weights, const float* z, int B, int S,
                       float near, float far, float grad_scale, float* loss,
                       float* loss_rays, float* g_weights, void* workspace,
                       nr_stream_t stream);

/* ---- evaluation image tail (noisy_src/metrics.py:43-116, inference.py:108-125)
 * Additive to ABI 5.
 *
 * nr_image_metrics: compute_ssim (metrics.py:48-116) and compute_mse (metrics.py:43-45)
 * of one image pair in one pass.  pred / target (H,W,C) fp32 row-major, C = 1 or 3.
 * g: the 11 one-dimensional Gaussian weights, a HOST array read during the call and
 * passed to the kernel by value (exp(-(i-5)^2 / (2 1.5^2)) normalised, in fp32, as
 * metrics._gaussian_window builds them).  The blur is zero-padded (pad 5, no
 * renormalisation at the borders), per channel, of p, t, p^2, t^2 and p t;
 * ssim_map = ((2 mu_p mu_t + C1)(2 s_pt + C2)) / ((mu_p^2 + mu_t^2 + C1)(s_p + s_t + C2)).
 * The fp32 inputs are promoted to double and ALL arithmetic after that is fp64 (a
 * separable 11-tap blur across, then down).  out (device, 2 doubles, OVERWRITTEN) =
 * {sum ssim_map, sum (p - t)^2}; the caller divides by H*W*C.  One workgroup per
 * 32 x 16 tile and channel writes its partials to its own slot of workspace
 * (nr_image_metrics_workspace_bytes, no zero-initialisation needed) and a second,
 * one-workgroup launch sums the slots in a fixed order: no atomics, bit-identical
 * from run to run.  NR_EARG (workspace_bytes: -1) for C not in {1, 3}, H < 1, W < 1,
 * or more tiles x channels than the workspace indexes with an int (INT_MAX / 256).  */
int64_t nr_image_metrics_workspace_bytes(int H, int W, int C);
int nr_image_metrics(const float* pred, const float* target, int H, int W, int C,
                     const float* g, double C1, double C2, double* out,
                     void* workspace, nr_stream_t stream);
/* save_image's quantisation (inference.py:108-111) on the device: src (H,W,C) fp32 ->
 * bytes (uint8)(clip(x * 255.0f, 0, 255)), truncated, written to row y, columns
 * [dst_x0, dst_x0 + W) of a frame whose rows are dst_stride bytes apart:
 * dst[y * dst_stride + (dst_x0 + x) * C + c].  Two calls fill the halves of a
 * side-by-side comparison frame without a concatenation.  Non-finite input is outside
 * the contract: 0 is written for it.                                               */
int nr_frame_u8(const float* src, int H, int W, int C, uint8_t* dst,
                int64_t dst_stride, int dst_x0, nr_stream_t stream);
/* depth_to_colormap (inference.py:114-125) then the quantisation above: depth (H,W)
 * fp32 -> dst (H,W,3) uint8 dense.  n = (d - min) / (max - min + 1e-8f), r = clamp(4n -
 * 1.5), g = clamp(2 - 4|n - 0.5|), b = clamp(1.5 - 4n): the host function's fp32
 * operations in its order (no contraction, correctly rounded division), so the bytes
 * equal the host path's.  Min and max come from per-workgroup partials in workspace
 * (nr_depth_frame_u8_workspace_bytes), reduced in a fixed order, no atomics.        */
int64_t nr_depth_frame_u8_workspace_bytes(void);
int nr_depth_frame_u8(const float* depth, int H, int W, uint8_t* dst,
                      void* workspace, nr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NERF_HIP_H */
