/*
 * goslam_neus.h -- C ABI of the mapping hot path (hash-grid NeuS renderer) in libgoslam_hip.so.
 *
 * Replaces the reference's use of tiny-cuda-nn (`tcnn.Encoding`, `tcnn.Network`;
 * reference src/InstantNeuS.py:62,192) and the PyTorch op chains of
 * `Renderer.render_batch_ray` (src/render.py:73-175) and `InstantNeuS.forward`
 * (src/InstantNeuS.py:295-370).  Conventions as in goslam_hip.h: device pointers unless the name
 * ends in `_host`, dense row-major tensors, hipStream_t as void*, no sync / no allocation.
 */
#ifndef GOSLAM_NEUS_H
#define GOSLAM_NEUS_H

#include "goslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Hash-grid geometry shared by host and device (tiny-cuda-nn HashGrid as configured at
 * src/InstantNeuS.py:44-52: 16 levels x 2 features, T=2^19, base 16, scale 1.447269237440378). */
#define GS_GRID_LEVELS 16
#define GS_GRID_FEATS 2
typedef struct {
  float scale[GS_GRID_LEVELS];
  uint32_t resolution[GS_GRID_LEVELS];
  uint32_t size[GS_GRID_LEVELS];     /* entries in the level's table */
  uint32_t offset[GS_GRID_LEVELS];   /* first entry of the level in the flat table */
  uint32_t hashed[GS_GRID_LEVELS];   /* 1 if the level is hashed, 0 if dense */
  uint32_t total;                    /* total entries (x GS_GRID_FEATS parameters) */
} gs_grid_meta;

/* Fill `meta_host` for the InstantNeuS configuration (tcnn grid.h constructor arithmetic). */
int gs_grid_meta_default(gs_grid_meta* meta_host);

/* Renderer.render_batch_ray sample placement (src/render.py:99-171): ray/AABB far bound,
 * stratified + near-surface samples, per-ray sort (merge of the two sorted runs), dists.
 *   rays_o/rays_d f32 [n,3]; gt_depth f32 [n] or NULL (then n_surface is ignored);
 *   bound f32 [3,2] (device); t_samples f32 [n_samples] = torch.linspace(0,1,n_samples),
 *   t_surface f32 [n_surface] likewise; perturb f32 [n_samples] = the shared
 *   torch.rand(N_samples) vector (:159) or NULL; gt_max = gt_depth.max() as a host scalar, or -- when
 *   gt_max_dev != NULL -- read from that device scalar instead (no host round trip per batch); or -- gt_max_dev == NULL
 *   and gt_max == -INFINITY, n_samples / n_surface <= 64 -- taken over gt_depth inside the launch (NaN if any depth is
 *   NaN, as torch.max): no reduction launch in front of this one;
 *   -> z_vals, dists f32 [n, n_samples + n_surface].                                          */
int gs_render_sample(const float* rays_o, const float* rays_d, const float* gt_depth,
                     const float* bound, const float* t_samples, const float* t_surface,
                     const float* perturb, float gt_max, const float* gt_max_dev, float* z_vals, float* dists,
                     int n, int n_samples, int n_surface, gs_stream_t stream);

/* tcnn.Encoding.__call__ (src/InstantNeuS.py:62,86): x f32 [n,3] in [0,1], grid f16
 * [total*2] -> out f16 [n,32]; optional dy_dx f32 [n,32,3] (analytic d out / d x).            */
int gs_grid_encode(const float* x, const void* grid, void* out, float* dy_dx, int n,
                   gs_stream_t stream);

/* Backward passes of tcnn.Encoding (the autograd the reference drives at src/InstantNeuS.py:134-148: the encoding is
 * differentiated w.r.t. x with create_graph=True on EVERY forward, and that gradient is differentiated again by
 * loss.backward()).  x f32 [n,3] in [0,1]; dy [n,32] f16 or f32 (dy_dtype), read as dy * dy_scale; grid f16
 * [total*2] (may be NULL when neither dx nor ddy is requested).
 *   v == NULL -- first order (tcnn kernel_grid_backward / kernel_grid_backward_input):
 *       grid_grad += sum_points w_corner(x) * dy     (atomically accumulated; zero it first; NULL = skip)
 *       dx f32 [n,3] = sum_c dy_c * d y_c / d x      (NULL = skip)
 *   v f32 [n,3] = d L / d (dx) -- second order (tcnn kernel_grid_backward_input_backward_*):
 *       ddy f32 [n,32] = (d y / d x) . v             (d L / d dy; NULL = skip)
 *       grid_grad += dy * sum_d v_d * d w_corner / d x_d
 *       dx f32 [n,3] = sum_c dy_c * (d^2 y_c / dx dx) v   (trilinear interpolation: mixed terms only)
 * grid_grad dtype GS_F32, or GS_F16 = tcnn's own mode (one packed fp16 atomic per table entry); every
 * contribution is multiplied by grid_grad_scale (tcnn's loss scale; the caller divides it out).       */
int gs_grid_backward(const float* x, const void* grid, const void* dy, int dy_dtype, float dy_scale,
                     const float* v, void* grid_grad, int grid_grad_dtype, float grid_grad_scale,
                     float* dx, float* ddy, int n, gs_stream_t stream);

/* tcnn.Network.__call__ (src/InstantNeuS.py:192,201): FullyFusedMLP n_in(->80, padded with
 * ones)->64->64->n_out(->16), ReLU, no bias; mlp f16 [64*80+64*64+16*64] row-major [out,in] per
 * layer; x f16 [n,n_in] -> out f16 [n,n_out].  Workspace only needed when n_in != 80.         */
size_t gs_mlp_workspace_bytes(int n, int n_in);
int gs_mlp_forward(const void* x, const void* mlp, void* out, int n, int n_in, int n_out,
                   void* workspace, size_t workspace_bytes, gs_stream_t stream);

/* InstantNeuS.forward (src/InstantNeuS.py:295-370) for one chunk of rays, forward only:
 * hash-grid encode + SDF linear + analytic SDF gradient + NeuS alpha + colour MLP + compositing.
 *   grid f16 [total*2], sdf_w f32 [32,35], sdf_b f32 [32], color_B f32 [3,33], mlp f16 [10240];
 *   inv_s = clip(exp(10*variance), 1e-6, 1e6) as a host scalar, or -- when inv_s_dev != NULL -- read from that device
 *   scalar instead (a training loop then never reads the variance parameter back to the host);
 *   bound_host / rt_bound_host: HOST f32 [3,2] (static bound for normalisation, realtime bound
 *   for the in-bound mask; 6 floats each, passed by value to the kernels).  rt_bound_dev (optional, DEVICE f32
 *   [3,2]): when non-NULL the kernels read the realtime bound from it instead of rt_bound_host, so a captured
 *   hipGraph of the launch follows InstantNeuS.update_bound (src/InstantNeuS.py:255-257,310) without a re-capture.
 * Outputs f32: color [n,3], depth [n], depth_var [n], normal [n,3], weight_sum [n], sdf [n,s],
 *   z_mid [n,s] (= z_vals + dists/2), grad_err_ray [n] (per-ray sum of (|grad|-1)^2 * mask; the
 *   caller divides the total by n*s); optional per-point alpha f32 [n,s], rgb f16 [n,s,3],
 *   grad f32 [n,s,3], mask u8 [n,s], mlp_in f16 [n,s,80] (NULL = keep in the workspace; the
 *   training path saves them for gs_neus_backward_*); enc_aux_out f16 [16,n*s,8] (optional): per level and point
 *   the record [enc0, enc1, d enc0 / dx (3), d enc1 / dx (3)] of the in-bound points -- handed to
 *   gs_neus_backward_points* as `enc_aux`, the backward streams it instead of gathering the table again.
 *   grad_err_scale multiplies grad_err_ray (1 = the raw per-ray sums the training step reduces; 1 / (n s) makes
 *   sum(grad_err_ray) the `gradient_error` of InstantNeuS.py:360-370 directly); sdf_variance_out f32 [n] (optional)
 *   is filled with sdf_variance_value (`sdf_variance` of the same dict).
 * The workspace needs no initial state (the in-bound flags are one byte per wave, each written by its wave).        */
size_t gs_neus_forward_workspace_bytes(int n, int s);
/* gs_neus_forward gathers the hashed levels LEVEL-MAJOR (one 2 MB level at a time per XCD, 16-byte records, then the
 * per-point stage) for batches of at least this many sample points, and per point below it.  Returns the previous value;
 * points < 0 only queries.  Default 524288 (measured: the two orders meet at ~442 K points on MI355X, profiles/r05_level_major_crossover.json).  Same results either way:
 * every per-point output (sdf, d sdf / d x, alpha, rgb, the MLP rows, enc_aux) is bit-identical.                   */
int gs_neus_level_major_min_points(int points);
int gs_neus_forward(const float* rays_o, const float* rays_d, const float* z_vals,
                    const float* dists, const void* grid, const float* sdf_w, const float* sdf_b,
                    const float* color_B, const void* mlp, float inv_s, const float* inv_s_dev,
                    const float* bound_host, const float* rt_bound_host, const float* rt_bound_dev,
                    float* color, float* depth, float* depth_var, float* normal,
                    float* weight_sum, float* sdf, float* z_mid, float* grad_err_ray,
                    float* alpha_out, void* rgb_out, float* grad_out, uint8_t* mask_out,
                    void* mlp_in_out, void* enc_aux_out, float grad_err_scale, float* sdf_variance_out,
                    float sdf_variance_value, int n, int s,
                    void* workspace, size_t workspace_bytes, gs_stream_t stream);

/* gs_neus_forward over MANY reference forward calls at once: the n rays are cut into ray batches of `ray_batch` rays and
 * each batch into pieces of `piece_rays` rays (the last batch and the last piece of every batch ragged; piece k of
 * batch b follows all pieces of batch b - 1) -- the calls Renderer.eval_points makes inside Renderer.render_img
 * (src/render.py:29-71,216-233).  Per piece, as one gs_neus_forward call on its rays would: the first 100 points are
 * forced valid when none of the piece lies in the realtime bound (InstantNeuS.py:311-312), and with piece_mean != 0
 * grad_err_ray[r] is pre-scaled by 1 / (n_piece s) of its own piece (grad_err_scale is then ignored), so that
 * grad_err_piece f32 [gs_neus_forward_pieces(n, ray_batch, piece_rays)] (optional) -- the per-piece sums of grad_err_ray
 * in fp64, in a fixed order -- is the `gradient_error` of every call, in order.  The other arguments and outputs are
 * gs_neus_forward's; gs_neus_forward is this call with one piece (ray_batch = piece_rays = n, piece_mean = 0).
 * The workspace is gs_neus_forward_workspace_bytes(n, s).                                                          */
int gs_neus_forward_pieces(int n, int ray_batch, int piece_rays);
int gs_neus_forward_segmented(const float* rays_o, const float* rays_d, const float* z_vals,
                              const float* dists, const void* grid, const float* sdf_w, const float* sdf_b,
                              const float* color_B, const void* mlp, float inv_s, const float* inv_s_dev,
                              const float* bound_host, const float* rt_bound_host, const float* rt_bound_dev,
                              float* color, float* depth, float* depth_var, float* normal,
                              float* weight_sum, float* sdf, float* z_mid, float* grad_err_ray,
                              float* alpha_out, void* rgb_out, float* grad_out, uint8_t* mask_out,
                              void* mlp_in_out, void* enc_aux_out, float grad_err_scale, int piece_mean,
                              float* grad_err_piece, float* sdf_variance_out, float sdf_variance_value, int n, int s,
                              int ray_batch, int piece_rays, void* workspace, size_t workspace_bytes,
                              gs_stream_t stream);

/* Renderer.render_img's sample placement for a whole frame (src/render.py:177-236 -> :73-171 per ray batch) in two
 * launches: the rays of every pixel p = y W + x from the pose -- rays_o = t, rays_d = ((x-cx)/fx, (y-cy)/fy, 1) R^T
 * (build_all_rays with nerf_coordinate = False; c2w DEVICE f32 [4,4]) -> rays_o, rays_d f32 [H W, 3] -- and the
 * samples of gs_render_sample, bit for bit, with the reference's per-batch semantics: ray batch b = pixels
 * [b B, (b+1) B) (B = ray_batch) clamps its far bound and places its invalid-depth surface samples with ITS OWN
 * gt_depth maximum (one segmented-max launch, NaN propagated as torch.max; written to batch_max f32 [ceil(HW/B)]) and
 * uses perturbation row b of perturb f32 [ceil(HW/B), n_samples] (NULL: no perturbation).  gt_depth f32 [H W] or
 * NULL (then no surface samples, near 0.01: render_batch_ray's no-depth branch).  n_samples, n_surface <= 64.
 *   -> z_vals, dists f32 [H W, n_samples + n_surface (0 without depth)].                                      */
int gs_render_img_sample(const float* c2w, int H, int W, float fx, float fy, float cx, float cy,
                         const float* gt_depth, const float* bound, const float* t_samples, const float* t_surface,
                         const float* perturb, int ray_batch, float* rays_o, float* rays_d, float* batch_max,
                         float* z_vals, float* dists, int n_samples, int n_surface, gs_stream_t stream);

/* Visualizer.vis's image metrics (src/image_visualization.py:57-83) in one deterministic reduction (fp64 partials,
 * fixed order, no atomics): from color f32 [n,3], depth f32 [n], normal f32 [n,3], sdf f32 [n*s], gt_depth f32 [n],
 * gt_color f32 [n,3] and c2w DEVICE f32 [4,4]:
 *   normal_cam f32 [n,3] = R^T normal (camera frame); depth_res f32 [n] = |gt - depth|, color_res f32 [n,3] =
 *   |gt_color - color|, both 0 where gt < 1e-3;
 *   metrics f64 [8] = { colour MSE over the k x 3 values with gt > 1e-3, PSNR = -10 log10(MSE), depth MAE, depth
 *   RMSE (same pixels), fraction of |sdf| < 0.01, fraction of |sdf| < 0.02 (all n s values), k, n s }
 *   (NaN where k = 0).  Any image output may be NULL.  partial: workspace of gs_render_img_metrics_workspace_bytes(). */
size_t gs_render_img_metrics_workspace_bytes(void);
int gs_render_img_metrics(const float* color, const float* depth, const float* normal, const float* sdf,
                          const float* gt_depth, const float* gt_color, const float* c2w, int n, int s,
                          float* normal_cam, float* depth_res, float* color_res, double* metrics,
                          void* workspace, size_t workspace_bytes, gs_stream_t stream);

/* ---- rendering evaluation (neus/render_eval.py), csrc/image_quality.hip ----
 * Quality of a rendered frame against the input frame, over the WHOLE image (gs_render_img_metrics above is the
 * visualiser's: pixels with depth only).  pred_rgb, gt_rgb f32 [H,W,3] interleaved, not clipped; pred_depth, gt_depth
 * f32 [H,W], both NULL or neither.
 *   -> out DEVICE f64 [8] = { mse, psnr, ssim, depth_l1, n_depth, n_windows, 0, 0 }:
 *   mse      mean of (pred - gt)^2 over the 3 H W values; psnr = -10 log10(mse) (data range 1; +inf at mse == 0);
 *   depth_l1 mean of |pred_depth - gt_depth| over the n_depth pixels with gt_depth > 0 (NaN and 0 without such a pixel
 *            or without the depth pair);
 *   ssim     Wang et al. 2004 per channel: 11 x 11 Gaussian window, sigma 1.5, weights the outer product of the
 *            normalised g_k = exp(-(k-5)^2 / 4.5) / sum; valid windows only, no padding: (H-10) x (W-10) positions per
 *            channel, n_windows = 3 (H-10)(W-10).  Per window mu_x, mu_y, E[x^2], E[y^2], E[xy]; var = E[x^2] - mu_x^2,
 *            cov = E[xy] - mu_x mu_y; s = (2 mu_x mu_y + C1)(2 cov + C2) / ((mu_x^2 + mu_y^2 + C1)(var_x + var_y + C2))
 *            with C1 = 0.01^2, C2 = 0.03^2; ssim = the mean of s.
 * Inputs are fp32, every moment and sum is fp64; fixed-order reductions (no atomics): the same bits on every run.  NaN
 * inputs give NaN outputs.  H < 11 or W < 11: GS_ERR_INVALID_ARG before any launch.  The kernel works on tiles of
 * GS_IQ_TILE_H x GS_IQ_TILE_W window positions (gs_image_quality_tile reads them back from the library); workspace:
 * gs_image_quality_workspace_bytes(H, W), one fp64 partial per sum and tile (0 for a refused size).                */
#define GS_IQ_TILE_H 16
#define GS_IQ_TILE_W 32
int gs_image_quality_tile(int* tile_h, int* tile_w);
size_t gs_image_quality_workspace_bytes(int H, int W);
int gs_image_quality(const float* pred_rgb, const float* gt_rgb, const float* pred_depth, const float* gt_depth,
                     int H, int W, double* out, void* workspace, size_t workspace_bytes, gs_stream_t stream);

/* Backward of InstantNeuS.forward, stage 1 (per ray): from the upstream gradients of the ray
 * outputs -- d_color [n,3], d_depth [n], d_depth_var [n], d_normal [n,3], d_weight_sum [n] --
 * and the saved per-point alpha / rgb / z_mid / grad / mask, produce d_alpha f32 [n,s] (w.r.t. the
 * unmasked alpha), d_rgb f32 [n,s,3] and the normal-output part of d_grad f32 [n,s,3].  s <= 128.  */
int gs_neus_backward_rays(const float* alpha, const void* rgb, const float* z_mid, const float* grad,
                          const uint8_t* mask, const float* d_color, const float* d_depth,
                          const float* d_depth_var, const float* d_normal, const float* d_weight_sum,
                          float* d_alpha, float* d_rgb, float* d_grad, int n, int s, gs_stream_t stream);

/* Backward of the fused colour MLP (tcnn FullyFusedMLP 67(->80)->64->64->3(->16), ReLU, sigmoid output) in ONE
 * kernel: recomputes H1, H2 as gs_mlp_forward does, then dX and the three weight gradients on MFMA.
 *   x f16 [n,80] (the saved MLP input rows), d_rgb f32 [n,3] (gradient w.r.t. the sigmoid outputs), rgb f16
 *   [n,3] (the saved outputs; NULL = no output activation, d_rgb is the gradient w.r.t. the raw network outputs,
 *   which is tcnn.Network's own contract: `output_activation: none`, src/InstantNeuS.py:184-192), loss_scale (tcnn: 128) multiplies every gradient that travels in fp16.
 *   wpack f16 [40][64][8]: MFMA A-fragments A[l][e] = M[32 mt + (l&31)][k(ks, l>>5, e)] of, in this
 *   order, M = W1 (mt<2, ks<5), W2 (mt<2, ks<4), W3^T (mt<2, ks=0), W2^T (mt<2, ks<4), W1^T zero-padded to 96
 *   rows (mt<3, ks<4), each block mt-major.  k(ks, hf, e) = 16 ks + 8 hf + e where the contraction runs over inputs /
 *   outputs (W1, W3^T); where it runs over HIDDEN neurons (W2, W2^T, W1^T) it is the order in which an accumulator
 *   tile of the previous GEMM holds them: k = 32 (ks >> 1) + 8 (2 (ks & 1) + (e >> 2)) + 4 hf + (e & 3) -- the kernel
 *   feeds one GEMM's accumulator registers to the next as its B fragments (gs_map_step_prep gathers this layout).
 * Outputs: dx f16 [n,80] = loss_scale * dL/dx;  partial f32 [gs_mlp_backward_blocks(n)][10240]: per-workgroup
 *   partial sums of loss_scale * (dW1 [64,80] | dW2 [64,64] | dW3 [16,64]) in tcnn's parameter layout -- sum
 *   over the first axis and divide by loss_scale.                                                        */
int gs_mlp_backward_blocks(int n);
int gs_mlp_backward(const void* x, const void* wpack, const float* d_rgb, const void* rgb, float loss_scale,
                    void* dx, float* partial, int n, gs_stream_t stream);

/* Stage 2 (per sample point): chain d_alpha, d_sdf (loss on the sdf samples), d_grad (stage 1 +
 * the eikonal term d_gerr_ray[ray] * d(|grad|-1)^2 * mask + the colour MLP's input gradient dX[:,33:36]),
 * d_feat = dX[:,36:67] and d_emb = dX[:,0:33] through NeuS alpha, the SDF linear layer and the hash
 * grid, INCLUDING the second-order path through d sdf / d x (tiny-cuda-nn's double backward).
 *   dX [n*s,80] is the colour MLP's input gradient (computed by the caller's MLP backward): f32, or f16
 *   holding dx_scale * gradient (the loss-scaled output of an fp16 GEMM).
 *   The per-point rows d_out, lin_in, dw0, d_arg, pts are f32 or f16 (row_dtype); the gradient-valued ones
 *   (d_out, dw0, d_arg) are multiplied by row_scale before they are stored (loss scale for fp16 rows).
 *   f16 rows are padded to GEMM-friendly widths -- lin_in / dw0 / d_arg 40, pts 8 (d_out stays 32); the pad
 *   columns are written as zeros, except pts[:,3] = 1 (so that pts^T @ rows also yields column sums).
 *   row_stride = 0: five separate contiguous buffers; row_stride = R (f16 only, R % 8 == 0): consecutive points'
 *   rows are R elements apart in every buffer, i.e. the five pointers address column blocks of ONE [n*s, R]
 *   matrix whose Gram matrix then delivers every dense-parameter gradient in a single GEMM.
 * Outputs: grid_grad [total*2] (atomically accumulated; zero it first) -- dtype GS_F32, or GS_F16 =
 * tiny-cuda-nn's mode: fp16 table gradient, both features of an entry added with one packed atomic,
 * every contribution pre-multiplied by grid_grad_scale (tcnn's loss scale, 128; the caller divides it
 * out) -- d_out f32 [n*s,32]
 * and lin_in f32 [n*s,35] (d sdf_layer.weight = d_out^T @ lin_in, d bias = colsum(d_out)),
 * dw0 f32 [n*s,35] (extra per-point contribution to sdf_layer.weight row 0: colsum),
 * d_arg f32 [n*s,33] (d color_B = pts^T @ d_arg), pts f32 [n*s,3], d_inv_s f32 [1] (atomic; zero it). */
int gs_neus_backward_points(const float* rays_o, const float* rays_d, const float* z_vals,
                            const float* dists, const void* grid, const float* sdf_w,
                            const float* color_B, float inv_s, const float* inv_s_dev, const float* bound_host,
                            const float* sdf, const float* grad, const uint8_t* mask,
                            const float* d_alpha, const float* d_sdf, const float* d_grad,
                            const void* dX, int dx_dtype, float dx_scale, const float* d_gerr_ray,
                            void* grid_grad, int grid_grad_dtype, float grid_grad_scale, void* d_out,
                            void* lin_in, void* dw0, void* d_arg, void* pts, int row_dtype, float row_scale,
                            int row_stride, float* d_inv_s, int n, int s, const void* enc_aux, gs_stream_t stream);
/* The same backward with the table gradient of the HASHED levels accumulated WITHOUT global atomics (bin-and-reduce:
 * workgroups write (13-bit index, 2 x fp16) records to their own segments of per-(level, bin) queues in `bin_ws`, then
 * one workgroup per bin sums its queue exactly in 64-bit fixed-point LDS accumulators (every fp16 record is a multiple of
 * 2^-24), rounds each sum to fp16 once and writes its 8192 entries once; neus_bwd.hip grid_bin_reduce_kernel).
 * grid_grad is the loss-scaled f16 table gradient (zero it first; the dense levels and any overflow records still
 * arrive as packed atomics).  `bin_ws`: gs_neus_bin_workspace_bytes(n * s) bytes of scratch (no initial state).
 * `sdf_wt` (optional, f32 [16][2][32]): sdf_w's encoding columns transposed, sdf_wt[l][f][o] = sdf_w[o][3 + 2 l + f]
 * (gs_map_step_prep writes it), which turns the kernel's strided weight reads into contiguous ones.                */
/* Ray gradients of the renderer (mapping.BA; a pass of its own, after gs_neus_backward_points[_binned], with the same
 * inputs): per sample point dL/dx -- the SDF layer's xyz columns and the hash grid's input gradient, the second-order
 * path through d sdf / d x (the trilinear interpolation's mixed second derivatives, from the 8 corner values gathered
 * again), the colour embedding sin(x B) -- and dL/d dir of the NeuS alpha's cos term; then per ray, in a fixed order:
 * d_rays f32 [n, 6] = [dL/d rays_o | dL/d rays_d] = [sum_k dL/dx_k | sum_k z_mid_k dL/dx_k + dL/d dir_k].
 * Points outside the realtime bound (mask 0) contribute nothing.  point_ws: f32 [n*s, 6] scratch.                      */
int gs_neus_backward_raygrad(const float* rays_o, const float* rays_d, const float* z_vals, const float* dists,
                             const void* grid, const float* sdf_w, const float* color_B, float inv_s,
                             const float* inv_s_dev, const float* bound_host, const float* sdf, const float* grad,
                             const uint8_t* mask, const float* d_alpha, const float* d_sdf, const float* d_grad,
                             const void* dX, int dx_dtype, float dx_scale, const float* d_gerr_ray, float* point_ws,
                             float* d_rays, int n, int s, gs_stream_t stream);
/* Camera-pose gradients per visited keyframe entry: rays [seg[e], seg[e+1]) belong to entry e, whose rays were built as
 * rays_d = dirs @ R^T, rays_o = t.  out f32 [n_entries, 12] = [dL/dR row-major (9) | dL/dt (3)].  One workgroup per
 * entry, fixed summation order, no atomics (reruns are bitwise identical); segments may be ragged or empty.            */
int gs_pose_grad_reduce(const float* ray_grad, const float* dirs, const int* seg, int n_entries, float* out,
                        gs_stream_t stream);
size_t gs_neus_bin_workspace_bytes(int n_points);
int gs_neus_backward_points_binned(const float* rays_o, const float* rays_d, const float* z_vals,
                                   const float* dists, const void* grid, const float* sdf_w, const float* color_B,
                                   float inv_s, const float* inv_s_dev, const float* bound_host, const float* sdf,
                                   const float* grad, const uint8_t* mask, const float* d_alpha, const float* d_sdf,
                                   const float* d_grad, const void* dX, int dx_dtype, float dx_scale,
                                   const float* d_gerr_ray, void* grid_grad, float grid_grad_scale, void* d_out,
                                   void* lin_in, void* dw0, void* d_arg, void* pts, int row_dtype, float row_scale,
                                   int row_stride, float* d_inv_s, int n, int s, void* bin_ws, size_t bin_ws_bytes,
                                   const float* sdf_wt, const void* enc_aux, gs_stream_t stream);

/* The mapper's ray draw for all frames of one joint iteration (src/nerf_func.py:115-181 build_rays after its random pick;
 * src/mapping.py:222-240,262-283 calls it per visited keyframe): ray t = (k, r) of drawn frame k takes the (rank[t] + 1)-th
 * valid pixel p of bank frame f = frame_pos[k] -- the first p with cums[f][p] >= rank[t] + 1, cums = the running sum of the
 * frame's mask over its hw = H * W pixels (row-major), rank[t] < cums[f][hw - 1] -- and writes
 *   rays_d[t] = [(u - cx) / fx, (v - cy) / fy, 1] @ rot_t[f]   (u = p % width, v = p / width; rot_t[f] = c2w[:3,:3]^T)
 *   rays_o[t] = trans[f],  out_color[t] = color[f * hw + p],  out_depth[t] = depth[f * hw + p].
 * rank i64 [n_frames_drawn * n_rays] (the reference's torch.randint draws), frame_pos i32 [n_frames_drawn], cums i32
 * [F][hw], color f32 [F * hw][3], depth f32 [F * hw], rot_t f32 [F][3][3], trans f32 [F][3]; outputs f32.           */
int gs_ray_draw(const long long* rank, const int* frame_pos, const int* cums, const float* color, const float* depth,
                const float* rot_t, const float* trans, int n_frames_drawn, int n_rays, int hw, int width, float fx,
                float fy, float cx, float cy, float* rays_o, float* rays_d, float* out_color, float* out_depth,
                gs_stream_t stream);

/* The mapper's loss without the eikonal term (src/mapping.py:96-132 + InstantNeuS.compute_sdf_error,
 * src/InstantNeuS.py:372-400) and its gradient, one launch.  Rays with rays_depth <= 0 are masked out.
 *   loss_rays[r] = ( w_color |c - c*|_1 / 3 + |d - d*| uw + w_sdf (e_r + f_r) ) / counts[0]
 *   with uw = 1/sqrt(depth_var + 1e-10) if `uncertainty` (treated as a constant, as the reference detaches it),
 *   e_r / f_r the per-ray SDF error / free-space terms; the loss is sum_r loss_rays[r]; counts[0] = number of
 *   valid rays over ALL ranks (device scalar).  d_color [n,3], d_depth [n], d_sdf [n,s] are d(sum loss)/d(.).
 * color [n,3], depth [n], depth_var [n], sdf [n,s], z_vals [n,s] (the sample depths InstantNeuS returns),
 * rays_color [n,3], rays_depth [n]; all f32; s <= 128.                                                      */
int gs_mapping_loss(const float* color, const float* depth, const float* depth_var, const float* sdf,
                    const float* z_vals, const float* rays_color, const float* rays_depth, const float* counts,
                    float truncation, float sparse_factor, float w_color, float w_sdf, int uncertainty,
                    float* d_color, float* d_depth, float* d_sdf, float* loss_rays, int n, int s,
                    gs_stream_t stream);

/* The mapper's optimiser step (src/mapping.py:55-58,135-137: clip_grad_norm_(35) over all trained parameters, then
 * AdamW with lr 1e-2 for the hash table and 1e-3 for the networks) on ONE flat fp32 parameter buffer laid out
 * [hash table (n16 entries) | dense parameters (n - n16)], in two launches.
 *   gs_map_grad_sqnorm: sqnorm_out[0] += sum g^2 (zero it first) over the table gradient g16 (fp16 holding
 *     gradient / inv_scale16, tiny-cuda-nn's loss-scaled form; n16 elements) and the dense gradients g32 (fp32).
 *   gs_map_adamw: coef = min(1, max_norm / (sqrt(sqnorm[0]) + 1e-6)) (sqnorm == NULL: no clipping; a NaN sqnorm gives
 *     a NaN coef, as torch.clamp does in clip_grad_norm_), then for every
 *     element g' = g * coef, p *= 1 - lr wd, m = b1 m + (1 - b1) g', v = b2 v + (1 - b2) g'^2,
 *     p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)   (torch.optim.AdamW), lr = lr16 on the table
 *     and lr32 on the dense range; p16 (optional, fp16 [n]) receives the fp16 working copy of the new parameters.
 *   All buffers 16-byte aligned, n16 % 8 == 0, step >= 1.                                                      */
int gs_map_grad_sqnorm(const void* g16, size_t n16, float inv_scale16, const float* g32, size_t n32,
                       float* sqnorm_out, gs_stream_t stream);
int gs_map_adamw(float* p, float* m, float* v, void* p16, const void* g16, size_t n16, float inv_scale16,
                 const float* g32, size_t n, float lr16, float lr32, float beta1, float beta2, float eps,
                 float weight_decay, int step, const float* sqnorm, float max_norm, gs_stream_t stream);
/* gs_map_adamw_seg: the same update with the two ranges given separately -- (p, m, v, p16, g16, n16) one contiguous
 * run of table entries: the whole table, or the 1/G slice a rank owns when the optimiser state is sharded over the G
 * ranks of a node (reduce-scatter of the table gradient -> this call on the slice -> all-gather of p16); (pd, md, vd,
 * p16d, g32, n32) the dense parameters.  `step_dev` (device int32 >= 1; may be NULL) overrides `step`, so a captured
 * hipGraph replays with the right bias corrections.  n16 need not be a multiple of 8; table pointers 16-byte aligned. */
int gs_map_adamw_seg(float* p, float* m, float* v, void* p16, const void* g16, size_t n16, float inv_scale16,
                     float* pd, float* md, float* vd, void* p16d, const float* g32, size_t n32, float lr16, float lr32,
                     float beta1, float beta2, float eps, float weight_decay, int step, const int* step_dev,
                     const float* sqnorm, float max_norm, gs_stream_t stream);

/* The scalar / reduction arithmetic around the mapper step's kernels in two launches (map_opt.hip):
 *   gs_map_step_prep: counts_out = counts_in if given, else [#rays with depth > 0, n, max depth] of rays_depth [n]
 *     (max depth = 0 for n = 0, NaN if any depth is NaN, as torch.max);
 *     inv_s_out[0] = clamp(exp(variance[0] * scale_factor), 1e-6, 1e6); d_gerr_out[0:n] = w_eikonal / (counts[1] * samples);
 *     d_invs[0] = sqnorm[0] = 0; step_dev[0] += 1; sdf_wt_out[l][f][o] = sdf_w[o][3 + 2 l + f] (both optional);
 *     mlp_wpack_out[i] = frag_index[i] == 10240 ? 0 : mlp16[frag_index[i]] for i < 20480 (all three optional): the
 *     40 A-fragments gs_mlp_backward takes, gathered from the fp16 parameter vector (frag_index: int32 [20480]).
 *   gs_map_step_post: g32 [mlp 10240 | sdf_w 32x35 | sdf_b 32 | color_B 3x33 | variance 1 | loss 1] from the chunked Gram
 *     product of the per-point rows laid out [d_out 32 | x y z 1 .. 8 | lin_in 40 | dw0 40 | d_arg 40] (gram_chunks f32
 *     [nchunk,40,160] = rows[:, :40]^T rows per chunk, summed over chunks, x inv_loss_scale), the MLP
 *     backward's workgroup partials (f32 [nb,10240]), d inv_s, and loss = sum(loss_rays) + w_eikonal * sum(gerr) /
 *     (counts[1] * samples).                                                                                        */
/* rows[:, :40]^T rows of the backward's per-point rows (f16 [n_rows,160], n_rows % 16 == 0, zero rows as padding) on the
 * matrix cores: partial f32 [gs_map_gram_blocks(n_rows)][40][160], one slab per workgroup (workgroup b sums the groups of
 * 16 rows [b per, min(n_rows / 16, (b + 1) per)), per = ceil(n_rows / 16 / blocks): trailing workgroups may be empty and
 * write zeros), in a fixed order (two runs are bit-equal).  Only the entries gs_map_step_post reads are written: rows
 * 0..31 x columns 32..95 and rows 32..39 x columns 0..31 and 64..159 (rows 32..39 x columns 32..63 are not formed) --
 * pass it as that function's gram_chunks with nchunk = gs_map_gram_blocks(n_rows).  Replaces a batched library GEMM. */
int gs_map_gram_blocks(int n_rows);
int gs_map_gram(const void* rows, int n_rows, float* partial, gs_stream_t stream);
int gs_map_step_prep(const float* rays_depth, int n, const float* variance, float scale_factor, float w_eikonal,
                     int samples, const float* counts_in, float* counts_out, float* inv_s_out, float* d_gerr_out,
                     float* d_invs, float* sqnorm, int* step_dev, const float* sdf_w, float* sdf_wt_out,
                     const void* mlp16, const int* frag_index, void* mlp_wpack_out, gs_stream_t stream);
int gs_map_step_post(const float* gram_chunks, int nchunk, float inv_loss_scale, const float* mlp_partial, int nb,
                     const float* d_invs, const float* variance, const float* inv_s, float scale_factor,
                     const float* loss_rays, const float* gerr, int n, float w_eikonal, int samples, const float* counts,
                     float* g32, gs_stream_t stream);

/* Mesh extraction (InstantNeuS.extract_geometry, src/InstantNeuS.py:457-497; mesh.hip).
 *
 * gs_sdf_lattice: u f32 [nx,ny,nz] (z fastest) = -sdf(xs[i], ys[j], zs[k]) -- the volume InstantNeuS.extract_fields
 *   returns -- in one launch: xs/ys/zs f32 [nx]/[ny]/[nz] (torch.linspace on the device, as extract_fields builds them);
 *   bound, realtime_bound f32 [3,2]; grid f16 [total*2]; sdf_w0 f32 [35] = row 0 of sdf_layer.weight, sdf_b0 f32 [1] =
 *   its bias[0].  A point not strictly inside realtime_bound gets -100 and gathers nothing.  Otherwise p = clamp((x - b0)
 *   / span * 2 - 1, -1, 1) and the 16 levels at (p + 1) / 2 op by op as SDFNetwork._query / gs_grid_encode (the fp16
 *   features equal gs_grid_encode's bit for bit), dotted with sdf_w0 in fp32 (fmaf, p first, then the levels in order),
 *   plus sdf_b0.  1 <= nx, ny, nz <= 1024.
 *
 * Marching cubes over a float32 volume u [nx,ny,nz] (1 <= nx, ny, nz <= 1024), the mcubes.marching_cubes(u, level)
 * contract: vertices in index space, x along axis 0.
 *   - corner below iff u < level (NaN is not below); a lattice edge crosses iff exactly one endpoint is below; every
 *     crossing edge gets exactly one vertex, shared by every cube touching it (also on a volume thinner than 2 along an
 *     axis, where no cube exists and no face references it);
 *   - vertex on the edge from its lower endpoint a0 (value u0) to a1 = a0 + 1: t = (level - u0) / (u1 - u0),
 *     pos = a0 + t * (a1 - a0) in fp32 without contraction; the other two coordinates are the lattice coordinates;
 *   - vertices in ascending linear index of the edge's lower endpoint, then axis x < y < z; faces in ascending linear
 *     index of the cube's lowest corner, then the order of the case's table entry;
 *   - the 256-case table resolves every cube face from its four corner classes alone (below corners meeting only
 *     diagonally stay separated), so cubes sharing a face agree and the mesh has no cracks; triangles are wound so that
 *     (v1 - v0) x (v2 - v0) points toward decreasing u.
 * Three steps, no workgroup ever waits on another:
 *   gs_mcubes_count: per point its crossing edges and in-workgroup vertex offset, per workgroup its V and F totals;
 *   gs_mcubes_scan:  the workgroup totals' prefix (two launches; in place, so once per count) and totals = [V, F]
 *                    (device int64 [2]) -- the one value the host reads, to size the outputs;
 *   gs_mcubes_emit:  vertices f32 [n_vertices,3] and faces int32 [n_faces,3] (n_* = the totals).  Returns
 *                    GS_ERR_UNSUPPORTED and launches nothing if either exceeds INT32_MAX; every store is bounded by
 *                    n_vertices / n_faces; nothing is launched when both are 0.
 * gs_mcubes_workspace_bytes: the three steps' transient device memory, 2 bytes per lattice point plus 8 per 256 points
 *   (+ alignment): 272,642,048 B at 512^3, 2,181,136,384 B at 1024^3; 0 for unsupported sizes.            */
int gs_sdf_lattice(const float* xs, const float* ys, const float* zs, int nx, int ny, int nz, const float* bound,
                   const float* realtime_bound, const void* grid, const float* sdf_w0, const float* sdf_b0, float* u,
                   gs_stream_t stream);
size_t gs_mcubes_workspace_bytes(int nx, int ny, int nz);
int gs_mcubes_count(const float* u, int nx, int ny, int nz, float level, void* workspace, size_t workspace_bytes,
                    gs_stream_t stream);
int gs_mcubes_scan(int nx, int ny, int nz, void* workspace, size_t workspace_bytes, long long* totals,
                   gs_stream_t stream);
int gs_mcubes_emit(const float* u, int nx, int ny, int nz, float level, const void* workspace, size_t workspace_bytes,
                   long long n_vertices, long long n_faces, float* vertices, int* faces, gs_stream_t stream);

/* ---- mesh culling (Mesher.cull_mesh, src/mesher.py:155-240), csrc/cull.hip ----
 *
 * gs_mesh_depth: depth maps f32 [n_poses,H,W] of a mesh (vertices f32 [V,3], faces i32 [F,3]) at n_poses world-to-camera
 * matrices w2c f32 [n_poses,3,4] (OpenCV convention; the host inverts c2w in float64).  Replaces extract_depth_from_mesh
 * (src/mesher.py:444-480: pyrender IntrinsicsCamera, DEPTH_ONLY | SKIP_CULL_FACES, znear 0.001, zfar = far).
 *   - pixel (row r, column c) holds the camera-space z of the nearest surface along the ray through the pixel centre
 *     (u, v) = (c + 0.5, r + 0.5): the GL pixel centre after pyrender's vertical flip.  (Mesher.point_masks samples the
 *     same maps at (u, v) = (c, r) through grid_sample(align_corners=True); that half-pixel mismatch is the reference's.)
 *   - 0 where no face covers the pixel centre, or where every hit is beyond zfar;
 *   - no back-face culling; the part of a triangle with z >= znear renders (camera-space near clipping, exact: the ray
 *     from the camera through the pixel centre hits the triangle's plane at z >= znear inside the triangle); triangles
 *     wholly in front of znear, degenerate faces, faces with an index outside [0, V), repeated indices or non-finite
 *     vertices render nothing;
 *   - coverage is inclusive (a centre exactly on an edge is covered) and watertight: every edge function is the fp64
 *     d . (P_lo x P_hi) of the edge's endpoints in ascending vertex-index order (times +-1), evaluated identically from
 *     both faces sharing it, with d = ((u - cx) / fx, (v - cy) / fy, 1) and P the fp64 camera-space vertices;
 *   - depth is the ray-plane intersection z = P0 . n / (d . n) in fp64 (perspective-correct), rounded to fp32 once;
 *   - the min over fragments is an atomicMin on the fp32 bit pattern (positive floats order as uint32), so the maps do
 *     not depend on arrival order and reruns are bitwise identical.
 *   One thread per face loads its vertices once for all n_poses poses; triangles whose pixel range exceeds 256 pixels go
 *   to a list (GS_MESH_DEPTH_LARGE_CAP entries in the workspace) that a second launch rasterises one workgroup per
 *   (face, pose).  workspace: gs_mesh_depth_workspace_bytes().  H * W <= 2^24.
 *
 * gs_mesh_visibility: Mesher.point_masks (src/mesher.py:56-137) for points f32 [n,3] against one chunk of n_poses
 * depth maps f32 [n_poses,H,W], w2c f32 [n_poses,4,4] = torch.inverse(c2w) in fp32.  Per frame, in fp32:
 *   cam = w2c . [p, 1], z = cam_z + 1e-8, u = (fx cam_x + cx cam_z) / z, v = (fy cam_y + cy cam_z) / z;
 *   in_frustum = 0 <= u <= W-1 && 0 <= v <= H-1 && z > 0; forecast_frustum likewise on the image grown by
 *   r = forecast_radius pixels per side (r < 0 shrinks it);
 *   d = grid_sample(depth, (u / (W-1) * 2 - 1, v / (H-1) * 2 - 1), padding_mode='border', align_corners=True) (bilinear,
 *   clamped to the border, zero texels blended); front = d > 0 ? z < d + 0.05 : true;
 *   seen |= in_frustum && front; forecast |= (in_frustum && front) || (forecast_frustum && front).
 *   seen / forecast uint8 [n] are read and OR-ed into (zero them before the first chunk).  One thread per point, the pose
 *   loop inside the kernel.  The fp32 sums of cam and uv are not torch's matmul order: decisions within a few ulps of a
 *   bound may differ.
 *
 * gs_face_components: trimesh's mesh.split(only_watertight=False) as get_connected_mesh (src/mesher.py:139-153) uses
 * it.  Faces i32 [F,3]; two faces are adjacent iff they share an edge (the same unordered pair of vertex indices); an
 * edge with equal endpoints connects nothing; an edge of more than two faces connects all of them.  labels i32 [F] =
 * the smallest face index of the face's component.  Edge -> smallest face in a device hash table (64-bit keys, linear
 * probing), union by compare-and-swap hooking of the larger root under the smaller, then pointer jumping.  F <= 2^28;
 * workspace: gs_face_components_workspace_bytes(F).
 *
 * gs_face_component_areas: from float64 vertices [V,3], faces, perm i32 [F] (the face order sorted by label, stable)
 * and sorted_labels i32 [F] (labels[perm]): comp_area f64 [F] (comp_area[label] = the component's area, 0 at indices
 * that are no label) and total f64 [1] = the sum of comp_area.  Face area 0.5 |(v1 - v0) x (v2 - v0)| in fp64; each
 * component summed in ascending sorted position within 1024-face tiles, the tiles' partial sums in tile order, the
 * total in a fixed strided-then-tree order: bitwise reproducible.  workspace: 16 bytes per face.
 *
 * gs_hull_extremes / gs_hull_prefilter: an exact interior-discard filter in front of the convex hull behind
 * OrientedBoundingBox.compute_from_pointcloud (Open3D's create_from_points: PCA of the convex-hull vertices).
 *   gs_hull_extremes: idx i32 [26] = for each of the 13 axis / face-diagonal / body-diagonal directions d, the point
 *     maximising +d . p, then -d . p (fp64; ties to the lower index; -1 if no point has a finite value).
 *     workspace: gs_hull_extremes_workspace_bytes(n).
 *   gs_hull_prefilter: keep u8 [n] = 0 iff n_k . p + c_k < -margin for every plane k (planes f64 [n_planes,4], the
 *     facets of the hull of those points as qhull writes them, outward normals), in fp64.  A point strictly inside the
 *     hull of a subset of the cloud is never a vertex of the cloud's hull; margin absorbs the planes' rounding.    */
#define GS_MESH_DEPTH_LARGE_CAP (1 << 20)
size_t gs_mesh_depth_workspace_bytes(void);
int gs_mesh_depth(const float* vertices, int n_vertices, const int* faces, int n_faces, const float* w2c, int n_poses,
                  float fx, float fy, float cx, float cy, int height, int width, float znear, float zfar, float* depth,
                  void* workspace, size_t workspace_bytes, gs_stream_t stream);
int gs_mesh_visibility(const float* points, int n_points, const float* w2c, const float* depth, int n_poses, float fx,
                       float fy, float cx, float cy, int height, int width, float forecast_radius, uint8_t* seen,
                       uint8_t* forecast, gs_stream_t stream);
size_t gs_face_components_workspace_bytes(int n_faces);
int gs_face_components(const int* faces, int n_faces, int* labels, void* workspace, size_t workspace_bytes,
                       gs_stream_t stream);
int gs_face_component_areas(const double* vertices, const int* faces, int n_faces, const int* perm,
                            const int* sorted_labels, double* comp_area, double* total, void* workspace,
                            size_t workspace_bytes, gs_stream_t stream);
size_t gs_hull_extremes_workspace_bytes(int n_points);
int gs_hull_extremes(const float* points, int n_points, int* idx, void* workspace, size_t workspace_bytes,
                     gs_stream_t stream);
int gs_hull_prefilter(const float* points, int n_points, const double* planes, int n_planes, double margin,
                      uint8_t* keep, gs_stream_t stream);

/* ---- mesh video (MeshVideo, src/tools/meshvideo.py), csrc/mesh_shade.hip ----
 * A visibility-buffer renderer: surface and line fragments compete in one uint64 buffer, a resolve pass shades what won.
 * No float atomics and nothing that depends on arrival order: reruns are bitwise identical.  The look is this project's
 * own contract (below), not Open3D's GL pipeline.
 *
 * gs_mesh_visbuf: visbuf u64 [n_poses,H,W], every word = (fp32 depth bits << 32) | face index of the nearest fragment,
 *   all ones where there is none (the call initialises the buffer).  Arguments, coverage, near clipping, rejection rules
 *   and the fp64 ray-plane depth are gs_mesh_depth's (same code, csrc/mesh_raster.h): the high word is gs_mesh_depth's map
 *   bit for bit wherever that is non-zero.  One 64-bit atomicMin per fragment, so equal fp32 depths resolve to the lower
 *   face index.  Same two launches and workspace layout as gs_mesh_depth: gs_mesh_visbuf_workspace_bytes().  H * W <= 2^24.
 *
 * gs_line_visbuf: world-space segments f32 [S,2,3] written into an initialised visbuf under the ids id_base + s (the host
 *   passes id_base = n_faces; id_base + S <= 2^32 - 1).  Per (segment, pose), in fp64 with every product and sum rounded
 *   on its own:
 *   - both end points to camera space, P = ((M0 x + M1 y) + M2 z) + M3 per row of w2c; a segment with a non-finite
 *     coordinate or with both z < znear draws nothing; an end point with z < znear is replaced by the crossing
 *     A + a (B - A), a = (znear - zA) / (zB - zA), with z = znear exactly (A the end in front of the plane);
 *   - (u, v) = (fx X / Z + cx, fy Y / Z + cy), the pixel of a point is (row floor(v), column floor(u));
 *   - n = max(|column1 - column0|, |row1 - row0|); the n + 1 steps i = 0..n sit at t = i / n (t = 0 when n = 0) on
 *     (u0 + t (u1 - u0), v0 + t (v1 - v0)): one pixel wide, as Open3D's LineSet; a step outside the image is skipped
 *     (the walk only visits the steps that can be inside, so a segment that leaves the screen costs its visible part);
 *   - the step's depth is z = 1 / (1/z0 + t (1/z1 - 1/z0)), perspective-correct along the projected line; steps with
 *     z < znear or z > zfar are skipped; the fragment is the same atomicMin of (fp32 bits of z << 32) | id.
 *   Lines are hidden by nearer surface and hide farther surface with no separate depth test; overlapping lines at equal
 *   depth resolve to the lower id.  One wave per (segment, pose), lanes striding the steps.
 *
 * gs_vertex_normals: area-weighted vertex normals f32 [V,3] (world space), Open3D's compute_vertex_normals: the
 *   normalised sum over a vertex' faces of (v1 - v0) x (v2 - v0).  Each face's cross product is computed in fp64 from the
 *   fp32 vertices, each component converted to fixed point q = rint(x * scale) (int64, round to nearest even) and added to
 *   its three vertices with integer atomics: integer addition is associative, so the sums -- sums i64 [V,3], zeroed by the
 *   call and left for the caller to read -- and the normals are bitwise reproducible.  A second launch converts the sums
 *   to fp64, normalises and rounds to fp32 once; a zero sum (zero-area faces only, or an unreferenced vertex) gives
 *   (0, 0, 0).  Faces with an index outside [0, V), or whose scaled cross product is non-finite or reaches 2^62 in a
 *   component, add nothing.  The caller chooses scale so that no sum can overflow: with extent the bounding box's
 *   diagonal, |component| <= extent^2 per face, so scale <= 2^62 / (extent^2 * F) is safe for any valence.
 *
 * gs_visbuf_resolve: image u8 [n_poses,H,W,3] from a visbuf, one thread per pixel:
 *   - an empty word (or an id that names nothing) gives `background`, packed 0xRRGGBB;
 *   - id >= n_faces: line_colors u8 [S,3] of segment id - n_faces;
 *   - a face: P and the canonical edge functions e0, e1, e2 of gs_mesh_depth at this pixel's ray d, recomputed in fp64;
 *     the perspective-correct barycentric weights are (w0, w1, w2) = (e1, e2, e0) / (e0 + e1 + e2);
 *     albedo = sum_j w_j vertex_colors[v_j] (u8 [V,3], levels 0..255), or 255 * GS_SHADE_GREY per channel when
 *     vertex_colors is NULL; n = R sum_j w_j vertex_normals[v_j] (R = the rotation of w2c), or with flat != 0 (or
 *     vertex_normals NULL) the face's camera-space normal s0 C0 + s1 C1 + s2 C2;
 *     shade = ambient + diffuse * |n . d| / (|n| |d|) -- a headlight at the camera, two-sided; 0 for the cosine when
 *     |n| = 0; channel = rint(min(max(albedo * shade, 0), 255)), rounded once (to nearest even).
 *   The host's defaults are ambient 0.3, diffuse 0.7, a white background.                                              */
#define GS_SHADE_GREY 0.7
size_t gs_mesh_visbuf_workspace_bytes(void);
int gs_mesh_visbuf(const float* vertices, int n_vertices, const int* faces, int n_faces, const float* w2c, int n_poses,
                   float fx, float fy, float cx, float cy, int height, int width, float znear, float zfar,
                   unsigned long long* visbuf, void* workspace, size_t workspace_bytes, gs_stream_t stream);
int gs_line_visbuf(const float* segments, int n_segments, unsigned id_base, const float* w2c, int n_poses, float fx,
                   float fy, float cx, float cy, int height, int width, float znear, float zfar,
                   unsigned long long* visbuf, gs_stream_t stream);
int gs_vertex_normals(const float* vertices, int n_vertices, const int* faces, int n_faces, double scale,
                      long long* sums, float* normals, gs_stream_t stream);
int gs_visbuf_resolve(const unsigned long long* visbuf, int n_poses, int height, int width, const float* vertices,
                      int n_vertices, const int* faces, int n_faces, const float* w2c, float fx, float fy, float cx,
                      float cy, const uint8_t* vertex_colors, const float* vertex_normals, int flat,
                      const uint8_t* line_colors, int n_segments, float ambient, float diffuse, unsigned background,
                      uint8_t* image, gs_stream_t stream);

/* Mesh evaluation (Mesher.__call__ at the end of a run, reference src/mesher.py:309-327): exact nearest neighbours
 * between fp64 point clouds -- the two cKDTree passes of eval_mesh (src/mesher.py:390-421) and the hybrid search of the
 * Open3D point-to-point ICP behind align_mesh (src/mesher.py:339-357) -- and the moments of an ICP correspondence set.
 *
 * Contract of a query (gs_nn_query): reference points R f64 [N,3], queries Q f64 [M,3], optional transform f64 [4,4]
 * (row-major, device) applied to each query as q'_r = ((T[r,0] q_x + T[r,1] q_y) + T[r,2] q_z) + T[r,3];
 *   d2 = dx*dx + dy*dy + dz*dz (left to right, no contraction), index = the nearest point of R, the smallest index on
 *   equal d2.  max_distance >= 0: Open3D's hybrid search with one neighbour: the nearest point is returned iff
 *   d2 < max_distance^2 (strict, as FLANN's radius result set), otherwise index -1 and d2 = +inf.  max_distance < 0:
 *   no limit.  A query with a non-finite coordinate gets index -1, d2 = +inf.  Exact, so reruns are bitwise identical.
 *
 * Grid: a uniform grid over R's bounding box, grid_host f64 [5] = (lo_x, lo_y, lo_z, h, scale) and dims_host i32 [3]
 * (nx, ny, nz; nx ny nz <= GS_NN_MAX_CELLS), scale = the largest |coordinate| of the box + h.  The cell of a point is
 * floor((p - lo) / h) per axis (clamped to the grid for R), key = (cz ny + cy) nx + cx.
 *   gs_nn_cell_keys: keys i32 [N].
 *   gs_nn_grid_build: from sorted_keys i32 [N] and perm i64 [N] (a stable sort of the keys, so ascending index within
 *     a cell): cell_start i32 [nx ny nz + 1] (the first sorted position of each cell), sorted_points f64 [N,3] =
 *     points[perm], sorted_index i32 [N] = perm.
 *   gs_nn_query: one lane per query visits rings of cells of growing Chebyshev radius around the query's cell and stops
 *     when the best d2 is below the squared distance to the unvisited region, that distance first reduced by a slack
 *     1e-9 (scale + |q|_1) that dwarfs fp64 rounding (so rounding can never end a search early); with max_distance it
 *     also stops once that bound reaches max_distance^2.  A query that would visit more than GS_NN_CELL_BUDGET cells is
 *     put on a list that a brute-force launch resolves (R streamed through LDS, ascending index, strict <): the work per
 *     query is bounded by GS_NN_CELL_BUDGET cells plus N points.  workspace: gs_nn_query_workspace_bytes(M); its first
 *     int32 is the number of queries that fell back.  No host synchronisation.
 *
 * gs_icp_moments: over the correspondences i (index[i] >= 0) of source f64 [n,3] (transformed as above when transform
 * != NULL) and target f64 [*,3]: moments f64 [17] = count, sum d2, source centroid [3], target centroid [3] (0 when
 * the count is 0), then sum_i (t_i - t_mean)(s_i - s_mean)^T row-major [3,3] (row = target axis).  Two passes (the
 * sums, then the centred products), each summed within tiles of 2048 correspondences (per thread in ascending order,
 * then a fixed tree) and the tiles in tile order: bitwise reproducible.  workspace: gs_icp_moments_workspace_bytes(n). */
#define GS_NN_MAX_CELLS (1 << 25)
#define GS_NN_CELL_BUDGET 16384
int gs_nn_cell_keys(const double* points, int n_points, const double* grid_host, const int* dims_host, int* keys,
                    gs_stream_t stream);
int gs_nn_grid_build(const double* points, int n_points, const int* sorted_keys, const int64_t* perm,
                     const int* dims_host, int* cell_start, double* sorted_points, int* sorted_index, gs_stream_t stream);
size_t gs_nn_query_workspace_bytes(int n_queries);
int gs_nn_query(const double* points, const double* sorted_points, const int* sorted_index, const int* cell_start,
                int n_points, const double* grid_host, const int* dims_host, const double* queries, int n_queries,
                const double* transform, double max_distance, double* d2, int* index, void* workspace,
                size_t workspace_bytes, gs_stream_t stream);
size_t gs_icp_moments_workspace_bytes(int n_source);
int gs_icp_moments(const double* source, int n_source, const double* transform, const double* target, const int* index,
                   const double* d2, double* moments, void* workspace, size_t workspace_bytes, gs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GOSLAM_NEUS_H */
