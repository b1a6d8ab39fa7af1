/*
 * goslam_hip.h -- C ABI of the MI355X (gfx950) hot-path library `libgoslam_hip.so`.
 *
 * Every entry point replaces one export of the reference's `droid_backends` pybind module
 * (reference: src/lib/droid.cpp:237-250) or one tiny-cuda-nn call made by
 * src/InstantNeuS.py; the reference file:line each one stands in for is cited per function.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in `_host`;
 *   - tensors are dense row-major ("contiguous") with the shapes given in the comments;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); no entry point
 *     synchronises the device, allocates device memory, or throws;
 *   - return value: GS_OK (0) or a negative gs_status; gs_last_error() gives a message for
 *     the calling thread;
 *   - index tensors are int64 (torch.long) exactly as the reference passes them.
 */
#ifndef GOSLAM_HIP_H
#define GOSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gs_stream_t;

typedef enum {
  GS_OK = 0,
  GS_ERR_INVALID_ARG = -1,
  GS_ERR_WORKSPACE = -2,
  GS_ERR_LAUNCH = -3,
  GS_ERR_UNSUPPORTED = -4
} gs_status;

typedef enum { GS_F16 = 0, GS_F32 = 1, GS_F64 = 2 } gs_dtype;

const char* gs_version(void);
const char* gs_last_error(void);

/* Kernel timer (measurement mode for bench.py's roofline entries; no counterpart in the reference).  Between
 * gs_timing_begin(stream) and gs_timing_end() every kernel this THREAD launches through the library is followed by a
 * HIP event on `stream` (which must be the stream the kernels are launched on); gs_timing_read(name, ...) synchronises
 * and returns the summed duration [ms] and launch count of the kernels recorded under `name` (the launch names used
 * in error messages: "neus_point", "grid_bin_reduce", "conv3x3_pp", ...); gs_timing_names writes the comma-separated
 * names seen.  Nothing is recorded while the stream is being captured into a graph.                                  */
int gs_timing_begin(gs_stream_t stream);
int gs_timing_end(void);
int gs_timing_read(const char* name, double* total_ms, int* count);
int gs_timing_names(char* buf, int buf_bytes);

/* ------------------------------------------------------------------ correlation ---- */

/* droid_backends.corr_index_forward (src/lib/droid.cpp:149-158, correlation_kernels.cu:19-70,
 * 126-155).  volume [n,h1,w1,h2,w2] (dtype), coords f32 [n,2,h1,w1] -> corr [n,2r+1,2r+1,h1,w1]
 * (dtype).  Arithmetic is carried in `dtype` in the reference's accumulation order: per tap
 * ((s00 w_se + s01 w_sw) + s10 w_ne) + s11 w_nw, the fp32 weights cast to `dtype`, one rounding
 * per operation, cells outside the plane read as 0 (the sign of a zero result is not specified).
 * Non-finite coordinates -- this entry for every radius, gs_corr_lookup_pyramid[_slots] and
 * gs_corr_lookup_enc[_slots] alike: a pixel whose x or y is NaN or +-inf gets NaN in EVERY tap of
 * every level (its weights are NaN), and no other pixel changes by a bit.  (The reference's
 * saturating cast returns 0 for +-inf; NaN keeps a failed track visible.)  gs_corr_index_backward
 * adds nothing to the volume gradient for such a pixel.
 * Judge: tests/test_lookup_numerics_gpu.py against the float64 model of tests/lookup_referee.py. */
int gs_corr_index_forward(const void* volume, const float* coords, void* corr,
                          int n, int h1, int w1, int h2, int w2, int radius, int dtype,
                          gs_stream_t stream);

/* droid_backends.corr_index_backward (droid.cpp:160-171, correlation_kernels.cu:73-124,157-185).
 * volume_grad [n,h1,w1,h2,w2] must be zero-initialised by the caller.                        */
int gs_corr_index_backward(const float* coords, const void* corr_grad, void* volume_grad,
                           int n, int h1, int w1, int h2, int w2, int radius, int dtype,
                           gs_stream_t stream);

/* CorrBlock.__call__ (src/modules/corr.py:43-53) in ONE launch: the 4 pyramid levels
 * vol[l] [n,h1,w1,h2>>l,w2>>l] are sampled at coords/2^l (coords f32 [n,h1,w1,2], the layout
 * FactorGraph hands over) and written as corr [n, 4*(2r+1)^2, h1, w1] (level-major channels);
 * channels_last != 0 stores the same logical tensor with NHWC strides ([n,h1,w1,196] in memory).
 * layout: GS_CORR_ROWMAJOR = the reference's planes; GS_CORR_TILE8 (fp16 + channels_last only) =
 * levels 0-1 as written by gs_corr_volume_pyramid(layout = GS_CORR_TILE8), see below.               */
#define GS_CORR_ROWMAJOR 0
#define GS_CORR_TILE8 1
int gs_corr_lookup_pyramid(const void* vol0, const void* vol1, const void* vol2, const void* vol3,
                           const float* coords, void* corr,
                           int n, int h1, int w1, int h2, int w2, int radius, int dtype,
                           int channels_last, int layout, gs_stream_t stream);
/* The same lookup (fp16 volumes, radius 3) FUSED with corr_encoder[0] (src/droid_net.py:75-77: Conv2d(196, 128, 1) +
 * ReLU): y[n,h1,w1, 0:128] (pixels y_stride elements apart, fp16) = relu(W @ lookup + bias) -- the 196-channel features
 * never reach HBM.  wpad: fp16 [128][208] = the 1x1 weight [128][196] with rows zero-padded to 208; bias f32 [128].
 * Equals gs_corr_lookup_pyramid (bit-exact features) followed by gs_conv1x1 up to the fp32 summation order.      */
int gs_corr_lookup_enc(const void* vol0, const void* vol1, const void* vol2, const void* vol3, const float* coords,
                       const void* wpad, const float* bias, void* y, int y_stride, int n, int h1, int w1, int h2,
                       int w2, int layout, gs_stream_t stream);
/* The `_slots` forms read the planes of edge e from slot `slot[e]` (int64 [n] in device memory, NULL = e) of a volume
 * POOL vol[l] = [capacity, h1, w1, plane_l]: FactorGraph keeps the correlation volumes of its edges in such a pool, so
 * that adding edges (`CorrBlock.cat`, src/factor_graph.py:118 -- a copy of every volume held, 61 MB per edge at 60 x 80)
 * and dropping edges (`self.corr[~mask]`, :150 -- another) move no volume at all.  Same arithmetic as the plain forms.
 * gs_corr_lookup_pyramid_slots serves fp16 + channels_last only.                                                      */
int gs_corr_lookup_enc_slots(const void* vol0, const void* vol1, const void* vol2, const void* vol3, const int64_t* slot,
                             const float* coords, const void* wpad, const float* bias, void* y, int y_stride, int n,
                             int h1, int w1, int h2, int w2, int layout, gs_stream_t stream);
int gs_corr_lookup_pyramid_slots(const void* vol0, const void* vol1, const void* vol2, const void* vol3,
                                 const int64_t* slot, const float* coords, void* corr, int n, int h1, int w1, int h2,
                                 int w2, int radius, int dtype, int channels_last, int layout, gs_stream_t stream);

/* CorrBlock.__init__ + CorrBlock.corr (src/modules/corr.py:26-41,67-76): all-pairs volume of
 * fp16 feature maps fmap1[e], fmap2[e] ([n,128,h,w], both divided by 4) plus the 3 average-pooled
 * levels, each pooled level computed from the fp16-rounded level below (avg_pool2d on half).
 * Outputs vol[l] f16 [n,h,w,h>>l,w>>l].  Requires w % 8 == 0, w <= 96, h >= 8.
 * layout GS_CORR_TILE8 (w % 16 == 0): a private layout for the lookup's benefit -- the planes of levels
 * 0 and 1 are stored as 8x8-element (128-byte = one L2 line) tiles, element (y,x) of a plane at
 * ((y>>3) * ceil(wl/8) + (x>>3)) * 64 + (y&7) * 8 + (x&7), plane size gs_corr_level_elems(); an 8x8
 * lookup window then touches <= 4 lines instead of ~9.  Levels 2-3 stay row-major.  Rows beyond
 * h>>l inside the last tile row are never read and left unwritten.                                 */
size_t gs_corr_volume_workspace_bytes(int n, int dim, int h, int w);
size_t gs_corr_level_elems(int h, int w, int level, int layout);   /* elements per plane of one level */
int gs_corr_volume_pyramid(const void* fmap1, const void* fmap2, void* vol0, void* vol1, void* vol2,
                           void* vol3, int n, int dim, int h, int w, int layout,
                           void* workspace, size_t workspace_bytes, gs_stream_t stream);
/* ... written into slots out_slot[e] (int64 [n] in device memory, NULL = e) of a volume pool (see the lookups above) */
int gs_corr_volume_pyramid_slots(const void* fmap1, const void* fmap2, void* vol0, void* vol1, void* vol2,
                                 void* vol3, const int64_t* out_slot, int n, int dim, int h, int w, int layout,
                                 void* workspace, size_t workspace_bytes, gs_stream_t stream);

/* droid_backends.altcorr_forward (droid.cpp:173-184, altcorr_kernel.cu:27-149,290-319).
 * fmap1 [b,h1,w1,c], fmap2 [b,h2,w2,c] (channels-last, c in {64,128,256}), coords f32
 * [b,s,h1,w1,2] -> corr [b,s,(2r+1)^2,h1,w1]; dtype f16 or f32, fp32 accumulation.             */
int gs_altcorr_forward(const void* fmap1, const void* fmap2, const float* coords, void* corr,
                       int b, int s, int h1, int w1, int h2, int w2, int c, int radius, int dtype,
                       gs_stream_t stream);

/* droid_backends.altcorr_backward (droid.cpp:186-199, altcorr_kernel.cu:151-283,322-354): fp32 only, as the
 * reference instantiates it.  fmap1 [b,h1,w1,c], fmap2 [b,h2,w2,c], coords [b,s,h1,w1,2], corr_grad
 * [b,s,49,h1,w1] -> fmap1_grad (written), fmap2_grad (atomically accumulated; zero it first).  coords get
 * no gradient (the reference returns zeros).  c <= 256.                                              */
int gs_altcorr_backward(const float* fmap1, const float* fmap2, const float* coords, const float* corr_grad,
                        float* fmap1_grad, float* fmap2_grad, int b, int s, int h1, int w1, int h2, int w2,
                        int c, int radius, gs_stream_t stream);

/* AltCorrBlock.__call__ for one chunk of edges (src/modules/corr.py:95-145 as driven by FactorGraph.update_lowmem,
 * src/factor_graph.py:283-300): all four pyramid levels of altcorr_forward (altcorr_kernel.cu:27-149) in ONE launch,
 * features indexed by ii / jj inside the kernel (the reference gathers `pyramid[0][:, ii]`, `pyramid[i][:, jj]` per level)
 * and coords / 2^l formed in registers.
 *   pyr0..pyr3 f16 [N, h >> l, w >> l, c] channels-last (c = 128), coords f32 [e, h, w, 2], ii / jj i64 [e] (rows of the
 *   pyramid) -> out f16 [e, h, w, 196] (= the [e,196,h,w] tensor of the reference in channels-last memory order;
 *   channel = 49 l + 7 ix + iy).  fp16 products, fp32 accumulation and blend, one rounding: within half an fp16 ulp of
 *   gs_altcorr_forward on fp16 features.  h, w >= 8.                                                         */
int gs_altcorr_pyramid(const void* pyr0, const void* pyr1, const void* pyr2, const void* pyr3, const float* coords,
                       const int64_t* ii, const int64_t* jj, void* out, int e, int h, int w, int c, int radius,
                       gs_stream_t stream);

/* ------------------------------------------------------------------- geometry ------ */

/* DepthVideo.reproject -> pops.projective_transform(jacobian=False)
 * (src/depth_video.py:207-217, src/geom/projective_ops.py:114-144).
 * poses f32 [nbuf,7], disps f32 [nbuf,h,w], intrinsics f32 [nbuf,4], ii/jj i64 [n]
 * -> coords f32 [n,h,w,2], valid f32 [n,h,w,1].                                              */
int gs_reproject(const float* poses, const float* disps, const float* intrinsics,
                 const int64_t* ii, const int64_t* jj, float* coords, float* valid,
                 int n, int h, int w, gs_stream_t stream);

/* droid_backends.projmap (droid.cpp:133-140, droid_kernels.cu:427-516,1463-1488).
 * intrinsics f32 [4]; coords f32 [n,h,w,3] (channel 2 left 0), valid f32 [n,h,w,1].          */
int gs_projmap(const float* poses, const float* disps, const float* intrinsics,
               const int64_t* ii, const int64_t* jj, float* coords, float* valid,
               int n, int h, int w, gs_stream_t stream);

/* droid_backends.frame_distance (droid.cpp:120-131, droid_kernels.cu:518-657,1438-1460).    */
int gs_frame_distance(const float* poses, const float* disps, const float* intrinsics,
                      const int64_t* ii, const int64_t* jj, float* dist,
                      int n, int h, int w, float beta, gs_stream_t stream);

/* droid_backends.iproj (droid.cpp:141-147, droid_kernels.cu:779-850,1518-1541).
 * poses f32 [n,7], disps f32 [n,h,w] -> points f32 [n,h,w,3].                                */
int gs_iproj(const float* poses, const float* disps, const float* intrinsics, float* points,
             int n, int h, int w, gs_stream_t stream);

/* droid_backends.depth_filter (droid.cpp:186-196 region, droid_kernels.cu:661-775,1491-1515).
 * disps f32 [num,h,w], ix i64 [n], thresh f32 [n] -> counter f32 [n,h,w] (zeroed here).      */
int gs_depth_filter(const float* poses, const float* disps, const float* intrinsics,
                    const int64_t* ix, const float* thresh, float* counter,
                    int n, int num, int h, int w, gs_stream_t stream);

/* ---- keyframe point cloud (droid_visualization, src/visualization.py:104-150), csrc/pointcloud.hip ----
 *
 * The coloured dense cloud of k listed keyframes index i64 [k] (each in [0, num)) of full-resolution buffers
 * disps f32 [num,h,w] and images f32 [num,3,h,w], written compacted in (list position, row-major pixel) order.
 * Three launches, no atomics:
 *   gs_pointcloud_count: keep = (depth_filter count >= visible_num) & (disps[ix] > disp_floor[b]), the count being
 *                        exactly gs_depth_filter's with thresh for every keyframe (poses f32 [num,7], all num slots as
 *                        neighbours, intrinsics f32 [4]);
 *   gs_pointcloud_mask:  instead of the count pass, keep = mask[ix] != 0 (mask f32 [num,h,w]);
 *   gs_pointcloud_scan:  offsets i64 [k+1] on the device: offsets[b] = first point of list position b,
 *                        offsets[k] = the total -- the one value the host reads, to size the outputs;
 *   gs_pointcloud_emit:  points f32 [n_points,3] = gs_iproj's point of the pixel through poses_inv f32 [k,7] (one per
 *                        list position), colors f32 [n_points,3] = images[ix][:, pixel].  Every store is bounded by
 *                        n_points (= offsets[k]); nothing is launched when it is 0.
 * gs_pointcloud_workspace_bytes: transient device memory shared by the three steps, about 1/8 byte per listed pixel
 *   plus 12 bytes per 1024; 0 for an unsupported shape (k > 65535 or h * w > 2^30).                            */
size_t gs_pointcloud_workspace_bytes(int k, int h, int w);
int gs_pointcloud_count(const float* poses, const float* disps, const float* intrinsics, const int64_t* index,
                        const float* disp_floor, float thresh, float visible_num, int k, int num, int h, int w,
                        void* workspace, size_t workspace_bytes, gs_stream_t stream);
int gs_pointcloud_mask(const float* mask, const int64_t* index, int k, int num, int h, int w, void* workspace,
                       size_t workspace_bytes, gs_stream_t stream);
int gs_pointcloud_scan(int k, int h, int w, void* workspace, size_t workspace_bytes, long long* offsets,
                       gs_stream_t stream);
int gs_pointcloud_emit(const float* poses_inv, const float* disps, const float* intrinsics, const float* images,
                       const int64_t* index, int k, int num, int h, int w, const void* workspace,
                       size_t workspace_bytes, long long n_points, float* points, float* colors, gs_stream_t stream);

/* ---- TSDF fusion of keyframe depth (no counterpart in the reference), csrc/tsdf.hip ----
 *
 * State on a dense lattice of nx x ny x nz points, z contiguous, each size in [2, 1024] (gs_mcubes_*'s limit; anything
 * else returns GS_ERR_INVALID_ARG and launches nothing): tsdf f32 [nx,ny,nz] initialised to +1 by the caller, weight
 * f32 [nx,ny,nz] initialised to 0, colors f32 [3,nx,ny,nz] (planar RGB) initialised to 0.  Offsets are 64-bit.
 *
 * gs_tsdf_integrate: k frames, in the given order, GS_TSDF_BATCH per launch.  depth f32 [k,h,w] in metres along the
 *   optical axis (<= 0: invalid), mask f32 [k,h,w] or NULL (0 drops the pixel), images f32 [k,3,h,w] or NULL (the
 *   colour lattice is then neither read nor written and may be NULL), w2c f32 [k,3,4] world-to-camera matrices, rows
 *   (r0 r1 r2 t).  fx, fy > 0.  Per lattice point (i,j,k) and frame, in fp32, one rounding per operation, no fma:
 *
 *     p   = lo + float(idx) * voxel                       (per axis)
 *     pc  = R p + t   as ((r0*px + r1*py) + r2*pz) + t    (per row)
 *     skip if !(pc.z > 1e-3)
 *     u = fx * (pc.x / pc.z) + cx ; v = fy * (pc.y / pc.z) + cy
 *     fu = floorf(u + 0.5f) ; fv likewise ; skip unless 0 <= fu < w and 0 <= fv < h ; iu = (int)fu ; iv = (int)fv
 *     d = depth[iv,iu] ; skip if !(d > 0) or mask[iv,iu] == 0
 *     sdf = d - pc.z ; skip if sdf < -trunc
 *     s = fminf(1.0f, sdf / trunc)
 *     w1 = w0 + 1.0f
 *     tsdf = (tsdf * w0 + s) / w1
 *     if sdf <= trunc: colour = (colour * w0 + images[:,iv,iu]) / w1   (per channel)
 *     w = fminf(w1, max_weight)
 *
 *   One lane owns a point: no atomics, results independent of the launch geometry and of how k is cut into calls.
 * gs_tsdf_vertex_attr: vertices f32 [n_vertices,3] of gs_mcubes_emit over that lattice (index space; at most one
 *   coordinate c of a vertex is fractional).  a = floor of every coordinate; b = a, plus one along the first axis with
 *   t = c - floorf(c) > 0 (t = 0 and b = a when there is none); both clamped into the lattice.
 *   keep u8 [n_vertices] = weight[a] >= min_weight && weight[b] >= min_weight;
 *   rgb f32 [n_vertices,3] = colors[a] + t * (colors[b] - colors[a]) per channel.                                   */
#define GS_TSDF_BATCH 16
int gs_tsdf_batch(void);
int gs_tsdf_integrate(float* tsdf, float* weight, float* colors, int nx, int ny, int nz, const float* depth,
                      const float* mask, const float* images, const float* w2c, int k, int h, int w, float fx, float fy,
                      float cx, float cy, float lo_x, float lo_y, float lo_z, float voxel, float trunc,
                      float max_weight, gs_stream_t stream);
int gs_tsdf_vertex_attr(const float* vertices, int n_vertices, const float* weight, const float* colors, int nx, int ny,
                        int nz, float min_weight, unsigned char* keep, float* rgb, gs_stream_t stream);

/* ---- reversible TSDF fusion on that lattice: integer sums that an observation can leave again (no counterpart in the
 *      reference), csrc/tsdf_live.hip; tests/tsdf_live_restatement.py restates it serially ----
 *
 * State, all zero in a fresh volume: sum_s i32 [nx,ny,nz], count i32 [nx,ny,nz], sum_rgb i32 [3,nx,ny,nz] (planar, as
 * colors above), count_rgb i32 [nx,ny,nz].  state = sum over frames of sign * obs(frame): integer addition commutes and
 * has an exact inverse, so the state depends on neither the order of the frames nor on how they are cut into batches
 * and calls, and adding a frame with sign -1 undoes, bit for bit, adding the same inputs with sign +1.
 *
 * gs_tsdf_accumulate: k frames, GS_TSDF_BATCH per launch.  Lattice, depth, mask, images, w2c and intrinsics exactly as
 *   gs_tsdf_integrate takes them; sign i32 [k] (device), an integer multiplier (+1 adds, -1 removes).  sum_rgb and
 *   count_rgb may both be NULL when images is NULL (they are then neither read nor written); images with either of them
 *   NULL, a lattice size outside [2, 1024], a NULL state, depth, w2c or sign, h, w < 1, h * w > 2^30, k < 0 or fx, fy,
 *   voxel, trunc <= 0 return GS_ERR_INVALID_ARG before anything is launched; k == 0 launches nothing.  Per lattice
 *   point and frame, gs_tsdf_integrate's sequence operation for operation up to and including
 *
 *     s = fminf(1.0f, sdf / trunc)                        (reached only with sdf >= -trunc, so -1 <= s <= 1)
 *
 *   and then, in i32:
 *
 *     q = (int)rintf(s * 16384.0f)                        (|q| <= 16384; the product by 2^14 is exact, rintf rounds
 *                                                          to nearest, ties to even: the one rounding of the value)
 *     sum_s += sign * q ; count += sign
 *     if images and sdf <= trunc, per channel:
 *       c = (int)rintf(fminf(fmaxf(img, 0.0f), 1.0f) * 255.0f)      (a NaN image value gives 0: fmaxf returns the 0)
 *       sum_rgb += sign * c
 *     and once: count_rgb += sign
 *
 *   There is no weight cap (a cap is not linear).  With at most 65535 frames alive |sum_s| <= 16384 * 65535 < 2^30.
 * gs_tsdf_resolve: the state as gs_tsdf_integrate's lattices; every element of the outputs is written.
 *     weight = (float)max(count, 0)
 *     tsdf   = count > 0 ? (float)((double)sum_s / ((double)count * 16384.0)) : 1.0f
 *     colors = count_rgb > 0 ? (float)((double)sum_rgb / ((double)count_rgb * 255.0)) : 0.0f      (per channel)
 *   The double product and quotient round once each, then once to float.  colors, sum_rgb and count_rgb are all NULL or
 *   all given.  A point no frame is alive at resolves to the bits a fresh volume holds (tsdf 1, weight 0, colours 0).
 * gs_tsdf_frame_change: what moved between a fused observation and the buffers as they are now.  old_depth, cur_depth
 *   f32 [k,h,w], w2c_old, w2c_new f32 [k,3,4], out f64 [k,4]; k == 0 launches nothing.  Per frame:
 *     out[0] = the number of pixels with old > 0 && cur > 0
 *     out[1] = the sum over those pixels of (double)fabsf(cur - old)
 *     out[2] = |c_new - c_old|, c = -R^T t the camera centre
 *     out[3] = |p_new - p_old|, p = R^T ((double)ref_depth * e_z - t) the point at ref_depth on the optical axis
 *   c and p in fp64 from the fp32 matrix, per component j with column j of R: c_j = -((r0j*t0 + r1j*t1) + r2j*t2),
 *   p_j = (r0j*(-t0) + r1j*(-t1)) + r2j*(ref - t2); |a - b| = sqrt((dx*dx + dy*dy) + dz*dz).  Equal matrices give exactly
 *   0.  The sums run in a fixed order: thread t of 256 adds pixels t, t + 256, ... in increasing order, a wave adds its
 *   64 partials by v += v[lane ^ m] for m = 32, 16, 8, 4, 2, 1, and the four waves' totals are added as
 *   ((w0 + w1) + w2) + w3.  No atomics: two runs agree bitwise.                                                        */
int gs_tsdf_accumulate(int* sum_s, int* count, int* sum_rgb, int* count_rgb, int nx, int ny, int nz, const float* depth,
                       const float* mask, const float* images, const float* w2c, const int* sign, int k, int h, int w,
                       float fx, float fy, float cx, float cy, float lo_x, float lo_y, float lo_z, float voxel,
                       float trunc, gs_stream_t stream);
int gs_tsdf_resolve(const int* sum_s, const int* count, const int* sum_rgb, const int* count_rgb, int nx, int ny, int nz,
                    float* tsdf, float* weight, float* colors, gs_stream_t stream);
int gs_tsdf_frame_change(const float* old_depth, const float* cur_depth, const float* w2c_old, const float* w2c_new, int k,
                         int h, int w, float ref_depth, double* out, gs_stream_t stream);

/* ---- raycast of that TSDF lattice: depth, normal and colour images (no counterpart in the reference),
 *      csrc/tsdf_raycast.hip; tests/tsdf_raycast_restatement.py restates it serially ----
 *
 * gs_tsdf_raycast: k frames of h x w pixels through the lattice above (tsdf, weight f32 [nx,ny,nz], colors f32
 *   [3,nx,ny,nz] or NULL).  c2w f32 [k,3,4] camera-to-world matrices, rows (r0 r1 r2 o).  fx, fy != 0, voxel > 0,
 *   0 <= near < far (far may be +inf), 0 < step_voxels <= 1, sizes in [2, 1024], h, w >= 1, k >= 0 (0: nothing is
 *   launched); anything else returns GS_ERR_INVALID_ARG and launches nothing.  Outputs depth f32 [k,h,w], normal f32
 *   [k,h,w,3], color f32 [k,h,w,3] or NULL (needs colors); every pixel of them is written.  Per pixel (iu, iv), in fp32,
 *   one rounding per operation, no fma; a MISS writes depth = 0, normal = 0, colour = 0:
 *
 *     dx = (float(iu) - cx) / fx ; dy = (float(iv) - cy) / fy          (the direction (dx, dy, 1) is not normalised:
 *                                                                        t below is depth along the optical axis)
 *     dw = (r0 * dx + r1 * dy) + r2                                     (per row of c2w)
 *     og = (o - lo) / voxel ; dg = dw / voxel                           (per axis; index space, g(t) = og + t * dg)
 *     MISS unless og and dg are finite on every axis
 *     dt = (step_voxels * voxel) / sqrtf((dw.x * dw.x + dw.y * dw.y) + dw.z * dw.z) ; MISS unless 0 < dt < inf
 *     t0 = near ; t1 = far ; per axis with top = float(n - 1):
 *       dg == 0: MISS unless 0 <= og <= top                             (the axis constrains nothing otherwise)
 *       else   : ta = (0 - og) / dg ; tb = (top - og) / dg ; t0 = max(t0, min(ta, tb)) ; t1 = min(t1, max(ta, tb))
 *     (og, dg finite and dg != 0: ta and tb are never NaN, and no product 0 * inf is ever formed.)
 *     for i = 0 .. GS_TSDF_RAY_STEPS: t_i = t0 + float(i) * dt ; stop (MISS) unless t_i < t1
 *       sample(t): g = og + t * dg (per axis) ; a = floorf(g) ; valid iff 0 <= a < top on every axis (compared as
 *         floats) and weight >= min_weight at all eight corners a + {0,1}^3 ; fr = g - a ;
 *         value = trilinear tsdf, lerp(p, q, s) = p + s * (q - p) along z (four), then y (two), then x (one).
 *       HIT at the first i >= 1 with sample(t_{i-1}) and sample(t_i) valid, f_{i-1} >= 0 and f_i < 0:
 *         depth = t* = t_{i-1} + dt * (f_{i-1} / (f_{i-1} - f_i)).  Later crossings, back-face ones included, are never
 *         looked at; a ray that only crosses from negative to positive misses.
 *     GS_TSDF_RAY_STEPS = ceil((nx + ny + nz) / step_voxels) + 2, in double from the float step_voxels.  A step moves g
 *       by step_voxels index units and no chord of the box is longer than nx + ny + nz of them, so the bound never
 *       causes a miss; it is the loop's own bound, so a lane ends whatever the pose holds.  It must not exceed 2^24
 *       (float(i) is exact): a smaller step_voxels is refused.
 *     at the hit: the cell of g(t*), valid as above or else MISS (depth too).  With v[x][y][z] its corners and
 *       (sx, sy, sz) = fr, the gradient of the trilinear interpolant, each component a difference of two bilinear
 *       values, every lerp as above:
 *         n.x = yx(1) - yx(0), yx(b) = lerp over y of the two z-lerps of face x = b        (lerps z, then y)
 *         n.y = zx(1) - zx(0), zx(b) = lerp over x of the two z-lerps of face y = b        (lerps z, then x)
 *         n.z = yx'(1) - yx'(0), yx'(b) = lerp over x of the two y-lerps of face z = b     (lerps y, then x)
 *       len = sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z) ; normal = n / len per component, 0 where !(len > 0): world
 *       frame, toward free space (increasing tsdf).  colour = trilinear colors per channel, lerps z, y, x.
 *     depth > 0 marks a hit (t* = 0 needs the camera centre on the surface at near = 0 and reads as a miss).
 *
 *   flags: NULL, or gs_tsdf_brick_flags' bytes of the SAME tsdf: a sample whose cell lies in a brick with a zero byte
 *   is not evaluated when reached as t_i (it is evaluated when a later sample needs it as t_{i-1}).  Such a cell's
 *   corners are all >= 0 and a chain of lerps p + fl(s * fl(q - p)), 0 <= s < 1, of non-negative values is never
 *   negative (rounding is monotone: fl(q - p) >= -p, so fl(s * ...) >= -p), so that sample cannot satisfy f_i < 0:
 *   outputs with and without flags are equal bit for bit.
 * gs_tsdf_brick_flags: flags u8 [bx,by,bz], b = ceil((n - 1) / 8) per axis (gs_tsdf_brick_flags_bytes gives the product,
 *   0 for sizes outside [2, 1024]): byte (i,j,k) = 1 if tsdf < 0 at any lattice point of [8i, min(8i + 8, nx - 1)] x
 *   [8j, ..] x [8k, ..] -- the corners of the 8 x 8 x 8 cells of that brick -- else 0.                                  */
size_t gs_tsdf_brick_flags_bytes(int nx, int ny, int nz);
int gs_tsdf_brick_flags(const float* tsdf, int nx, int ny, int nz, unsigned char* flags, gs_stream_t stream);
int gs_tsdf_raycast(const float* tsdf, const float* weight, const float* colors, int nx, int ny, int nz,
                    const unsigned char* flags, const float* c2w, int k, int h, int w, float fx, float fy, float cx,
                    float cy, float lo_x, float lo_y, float lo_z, float voxel, float near, float far, float step_voxels,
                    float min_weight, float* depth, float* normal, float* color, gs_stream_t stream);

/* ---- alignment of depth images to that TSDF lattice: the Gauss-Newton system of the squared TSDF values at the
 *      back-projected pixels and one damped step on the pose (no counterpart in the reference), csrc/tsdf_align.hip;
 *      tests/tsdf_align_restatement.py restates it ----
 *
 * All fp32 and all fp64 arithmetic below is one rounding per operation, no fma; sqrt and / are correctly rounded.
 *
 * gs_tsdf_align_chunk: the number of sampled pixels one workgroup reduces.  It fixes the summation order below, so it
 *   is part of the contract; callers and tests read it here.
 * gs_tsdf_align_workspace_bytes: n_poses * ceil(S / chunk) * 32 * 8 with S = ceil(h / stride) * ceil(w / stride), the
 *   chunks' partial rows; 0 for n_poses < 0, h, w or stride < 1, h * w > 2^30 or more than 2^31 - 1 rows.  Needs no GPU.
 * gs_tsdf_align_system: tsdf, weight f32 [nx,ny,nz] as above, depth f32 [k,h,w], frame i32 [n_poses] on the device (the
 *   depth map pose b looks at), pose f64 [n_poses,3,4] camera-to-world, rows (r0 r1 r2 o), workspace of at least
 *   gs_tsdf_align_workspace_bytes, out f64 [n_poses,32]; every element of out is written.  Sizes in [2, 1024], n_poses,
 *   k >= 0 (k >= 1 with a pose), h, w, stride >= 1, h * w <= 2^30, fx, fy != 0 and finite, cx, cy, lo finite, voxel > 0
 *   finite, huber > 0, max_depth > 0 (+inf allowed), min_weight not NaN, no NULL pointer; anything else returns
 *   GS_ERR_INVALID_ARG and launches nothing.  n_poses == 0 launches nothing.  frame lives on the device and is checked
 *   there: a pose whose frame[b] lies outside [0, k) reads no depth and gets an all-zero row.
 *   The sampled pixels of a pose are those with iu % stride == 0 && iv % stride == 0, sample s = (iv / stride) *
 *   ceil(w / stride) + iu / stride.  Per pose (R, o) = (float) of each fp64 entry, and per sampled pixel:
 *
 *     d = depth[frame[b], iv, iu] ; considered += 1 if d > 0 ; skip unless 0 < d <= max_depth        (a NaN fails)
 *     pc = ((float(iu) - cx) / fx * d, (float(iv) - cy) / fy * d, d)             (the quotient first, then times d)
 *     q  = (r0 * pc.x + r1 * pc.y) + r2 * pc.z per row of R ; pw = q + o
 *     g  = (pw - lo) / voxel ; a = floorf(g) ; skip unless 0 <= a < float(n - 1) on every axis (compared as floats) and
 *          weight >= min_weight at all eight corners a + {0,1}^3: gs_tsdf_raycast's sample() ; fr = g - a
 *     f  = trilinear tsdf and n = its gradient by gs_tsdf_raycast's lerp sequences (value: z, y, x; n.x: z, y; n.y: z,
 *          x; n.z: y, x; lerp(p, q, s) = p + s * (q - p))
 *     skip unless fabsf(f) < 1.0f                                        (a saturated sample carries no gradient)
 *     gw = n / voxel per component
 *     J  = (gw.x, gw.y, gw.z, q.y * gw.z - q.z * gw.y, q.z * gw.x - q.x * gw.z, q.x * gw.y - q.y * gw.x)
 *          (the derivative of f under o' = o + v, R' = dR R: the rotation acts about the camera centre)
 *     wt = fabsf(f) <= huber ? 1.0f : huber / fabsf(f)
 *     in fp64: wj_i = (double)wt * (double)J_i ; H_ij += wj_i * (double)J_j for i <= j ; b_i += wj_i * (double)f ;
 *              cost += ((double)wt * (double)f) * (double)f ; sq += (double)f * (double)f ; count += 1
 *
 *   out[b] = H (21: the upper triangle by rows, 00 01 .. 05 11 12 .. 55), b (6) at 21, cost at 27, count at 28, sq at
 *   29, considered at 30, 0 at 31.  Order of every fp64 sum: chunk c holds the samples [c * chunk, (c + 1) * chunk);
 *   within it thread t of 256 adds its samples t, t + 256, ... in increasing order onto 0.0 (a skipped sample adds
 *   nothing), a wave adds its 64 partials by v += v[lane ^ m] for m = 32, 16, 8, 4, 2, 1, the four waves' totals are
 *   added as ((w0 + w1) + w2) + w3 (gs_tsdf_frame_change's order), and the chunks' totals in increasing c starting from
 *   chunk 0's.  count and considered are integers.  No atomics: two runs agree bitwise.  out is complete when the call's
 *   work on the stream is.
 * gs_tsdf_align_step: one Levenberg-damped Gauss-Newton step per pose from out [n_poses,32], on pose [n_poses,3,4] in
 *   place; trace f64 [n_poses,4] or NULL receives (cost, count, considered, status) of the row it consumed.  lam_rel,
 *   lam_abs >= 0 finite, min_count >= 1, else GS_ERR_INVALID_ARG.  In fp64, H_ji = H_ij:
 *     A_ii = (H_ii + lam_rel * H_ii) + lam_abs ; A_ij = H_ij
 *     for j = 0 .. 5: s = A_jj, then s = s - L_jk * L_jk for k = 0 .. j - 1 ; a pivot with !(s > 0) fails ;
 *       L_jj = sqrt(s) ; for i > j: t = A_ij, then t = t - L_ik * L_jk for k = 0 .. j - 1 ; L_ij = t / L_jj
 *     y_i = (b_i - L_i0 y_0 - .. - L_i,i-1 y_i-1) / L_ii for i = 0 .. 5 (terms subtracted in increasing k)
 *     z_i = (y_i - L_5i z_5 - .. - L_i+1,i z_i+1) / L_ii for i = 5 .. 0 (terms subtracted in decreasing k) ; x = -z
 *   status = 0 and the pose stays as it is when count < min_count or a pivot fails, else status = 1 and
 *     o_i = o_i + x_i (i = 0, 1, 2) ; h = (x_3, x_4, x_5) * 0.5
 *     len = sqrt(((1 + h.x * h.x) + h.y * h.y) + h.z * h.z) ; (a, b, c, d) = (1 / len, h.x / len, h.y / len, h.z / len)
 *     dR = [ ((aa + bb) - cc) - dd   2 (bc - ad)             2 (bd + ac)           ]      aa = a * a, bc = b * c, ...
 *          [ 2 (bc + ad)             ((aa - bb) + cc) - dd   2 (cd - ab)           ]      (a unit quaternion's matrix: a
 *          [ 2 (bd - ac)             2 (cd + ab)             ((aa - bb) - cc) + dd ]      rotation, without trigonometry)
 *     P_ij = (dR_i0 * R_0j + dR_i1 * R_1j) + dR_i2 * R_2j                         (P = dR R)
 *     E_ij = ((P_0i * P_0j + P_1i * P_1j) + P_2i * P_2j) - (i == j ? 1 : 0)       (E = P^T P - I)
 *     R_ij = P_ij - 0.5 * ((P_i0 * E_0j + P_i1 * E_1j) + P_i2 * E_2j)             (R = P (I - E / 2))
 *   The last two lines are one Newton step toward the nearest rotation: the roundings of P would otherwise add up from
 *   step to step (|R^T R - I| of 1e-14 after 100 steps); with it the departure stays below 5e-16 after any number.
 *   An all-zero row (an out-of-range frame) has count 0 < min_count: status 0.                                         */
int gs_tsdf_align_chunk(void);
size_t gs_tsdf_align_workspace_bytes(int n_poses, int h, int w, int stride);
int gs_tsdf_align_system(const float* tsdf, const float* weight, int nx, int ny, int nz, const float* depth,
                         const int* frame, const double* pose, int n_poses, int k, int h, int w, int stride, float fx,
                         float fy, float cx, float cy, float lo_x, float lo_y, float lo_z, float voxel, float max_depth,
                         float min_weight, float huber, void* workspace, double* out, gs_stream_t stream);
int gs_tsdf_align_step(const double* out, double* pose, int n_poses, double lam_rel, double lam_abs, int min_count,
                       double* trace, gs_stream_t stream);

/* ---- two of those TSDF lattices put together: the Gauss-Newton system of a source volume S against a destination
 *      volume D, and S resampled and fused into D (no counterpart in the reference), csrc/tsdf_merge.hip;
 *      tests/tsdf_merge_restatement.py restates it ----
 *
 * A volume is tsdf, weight f32 [nx,ny,nz] (colors f32 [3,nx,ny,nz]) as above with its lo, voxel and trunc(ation); the
 * suffixes _d and _s name D's and S's.  All fp32 and all fp64 arithmetic below is one rounding per operation, no fma;
 * / is correctly rounded.  Sizes outside [2, 1024], stride < 1, n_poses < 0, a voxel or trunc that is not positive and
 * finite, a lo that is not finite, huber <= 0, a NaN min_weight or a NULL pointer return GS_ERR_INVALID_ARG before
 * anything is launched or written.
 *
 * gs_tsdf_register_workspace_bytes: n_poses * ceil(N / chunk) * 32 * 8 with chunk = gs_tsdf_align_chunk and N =
 *   ceil(nx_s / stride) * ceil(ny_s / stride) * ceil(nz_s / stride), the chunks' partial rows; 0 for n_poses < 0, a
 *   size outside [2, 1024], stride < 1 or more than 2^31 - 1 rows.  Needs no GPU.
 * gs_tsdf_register_system: pose f64 [n_poses,3,4] on the device maps S-world to D-world, rows (r0 r1 r2 o); a batch of
 *   hypotheses shares one launch.  workspace of at least gs_tsdf_register_workspace_bytes, out f64 [n_poses,32]; every
 *   element of out is written; n_poses == 0 launches nothing.  The samples are S's lattice points (i, j, k) with every
 *   index a multiple of stride, sample s = ((i / stride) * ceil(ny_s / stride) + j / stride) * ceil(nz_s / stride) +
 *   k / stride.  ratio = trunc_s / trunc_d (one fp32 division).  Per pose (R, o) = (float) of each fp64 entry, and per
 *   sample:
 *
 *     w = weight_s[i,j,k] ; fs = tsdf_s[i,j,k] ; fr = fs * ratio              (S's value in units of D's truncation)
 *     the sample is considered iff w >= min_weight and fabsf(fs) < 1.0f and fabsf(fr) < 1.0f ; considered += 1 ; else skip
 *     p  = lo_s + float(idx) * voxel_s                                        (per axis)
 *     q  = (r0 * p.x + r1 * p.y) + r2 * p.z per row of R ; pw = q + o
 *     g  = (pw - lo_d) / voxel_d ; a = floorf(g) ; skip unless 0 <= a < float(n_d - 1) on every axis and weight_d >=
 *          min_weight at all eight corners a + {0,1}^3 ; fr' = g - a
 *     f  = trilinear tsdf_d and n = its gradient, exactly gs_tsdf_align_system's sequences
 *     skip unless fabsf(f) < 1.0f
 *     r  = f - fr                                                             (the residual, in units of D's truncation)
 *     gw = n / voxel_d per component
 *     J  = (gw.x, gw.y, gw.z, q.y * gw.z - q.z * gw.y, q.z * gw.x - q.x * gw.z, q.x * gw.y - q.y * gw.x)
 *     wt = fabsf(r) <= huber ? 1.0f : huber / fabsf(r)
 *     in fp64: wj_i = (double)wt * (double)J_i ; H_ij += wj_i * (double)J_j for i <= j ; b_i += wj_i * (double)r ;
 *              cost += ((double)wt * (double)r) * (double)r ; sq += (double)r * (double)r ; count += 1
 *
 *   out[b] has gs_tsdf_align_system's layout (H 21, b 6, cost 27, count 28, sq 29, considered 30, 0 at 31) and its
 *   order of every fp64 sum: chunks of gs_tsdf_align_chunk samples, thread t of 256 adds its samples t, t + 256, ... in
 *   increasing order onto 0.0, the wave's butterfly, the four waves as ((w0 + w1) + w2) + w3, the chunks' totals in
 *   increasing order.  No atomics: two runs agree bitwise.  The rows are gs_tsdf_align_step's input: the step moves the
 *   pose S-world to D-world by o' = o + v, R' = dR R.
 * gs_tsdf_merge: S fused into D in place.  d2s f32 [3,4] ON THE HOST (read before the call returns) maps D-world to
 *   S-world, rows (r0 r1 r2 t), finite.  trunc_s >= trunc_d (a source that saturates earlier would write "0.8 of the
 *   truncation" where it only knows "free"), max_weight >= 1, min_weight > 0 (a cell no frame saw has nothing to add),
 *   S and D distinct lattices; else GS_ERR_INVALID_ARG.  colors_d, colors_s: only when both are given are colours read
 *   and written.  ratio = trunc_s / trunc_d.  Per lattice point (i,j,k) of D, in fp32:
 *
 *     p  = lo_d + float(idx) * voxel_d                                        (per axis)
 *     ps = ((r0 * p.x + r1 * p.y) + r2 * p.z) + t                             (per row of d2s)
 *     g  = (ps - lo_s) / voxel_s ; a = floorf(g) ; skip unless 0 <= a < float(n_s - 1) on every axis (a NaN fails)
 *     skip unless weight_s >= min_weight at all eight corners a + {0,1}^3 ; fr = g - a
 *     fs = trilinear tsdf_s, ws = trilinear weight_s, cs = trilinear colors_s per channel: lerp(p, q, s) = p + s *
 *          (q - p) along z (four), then y (two), then x (one)
 *     s  = fs * ratio ; skip if s < -1.0f ; s = fminf(1.0f, s)
 *     w0 = weight_d ; w1 = w0 + ws
 *     tsdf_d   = (tsdf_d * w0 + s * ws) / w1
 *     colors_d = (colors_d * w0 + cs * ws) / w1                               (per channel, with colours)
 *     weight_d = fminf(w1, max_weight)
 *
 *   A skipped point keeps its bits.  One lane owns a point: no atomics, results independent of the launch geometry.  */
size_t gs_tsdf_register_workspace_bytes(int n_poses, int nx_s, int ny_s, int nz_s, int stride);
int gs_tsdf_register_system(const float* tsdf_d, const float* weight_d, int nx_d, int ny_d, int nz_d, float lo_dx,
                            float lo_dy, float lo_dz, float voxel_d, float trunc_d, const float* tsdf_s,
                            const float* weight_s, int nx_s, int ny_s, int nz_s, float lo_sx, float lo_sy, float lo_sz,
                            float voxel_s, float trunc_s, const double* pose, int n_poses, int stride, float min_weight,
                            float huber, void* workspace, double* out, gs_stream_t stream);
int gs_tsdf_merge(float* tsdf_d, float* weight_d, float* colors_d, int nx_d, int ny_d, int nz_d, float lo_dx, float lo_dy,
                  float lo_dz, float voxel_d, float trunc_d, float max_weight, const float* tsdf_s, const float* weight_s,
                  const float* colors_s, int nx_s, int ny_s, int nz_s, float lo_sx, float lo_sy, float lo_sz,
                  float voxel_s, float trunc_s, const float* d2s, float min_weight, gs_stream_t stream);

/* ---- the dominant planes of that TSDF lattice: a histogram of surface normals, histograms of plane offsets along given
 *      directions and the moments of the samples near given planes (no counterpart in the reference),
 *      csrc/tsdf_planes.hip; tests/tsdf_planes_restatement.py restates it ----
 *
 * tsdf, weight f32 [nx,ny,nz] as above.  All fp32 and all fp64 arithmetic below is one rounding per operation, no fma; /
 * is correctly rounded; no square root is taken.  Sizes outside [2, 1024], a NULL pointer, a voxel that is not positive
 * and finite, a lo, ref or min_weight that is not finite, bins odd or outside [2, 64], n_planes outside [0, 16], n_bins
 * outside [1, 2048], cos2 outside [0, 1], bin <= 0 or not finite, band < 0 or not finite return GS_ERR_INVALID_ARG before
 * anything is launched or written.  n_planes == 0 launches nothing.
 *
 * The three calls share the surface sample of a cell.  A cell (a, b, c), 0 <= a <= n - 2 per axis, has the eight corners
 * (a, b, c) + {0,1}^3; cell s = (a * (ny - 1) + b) * (nz - 1) + c.  It is a sample iff (a NaN fails every test)
 *
 *     weight >= min_weight at all eight corners
 *     fabsf(v) < 1.0f for all eight values v, some v < 0 and some v >= 0
 *     f  = the trilinear value at (0.5, 0.5, 0.5) and g = its gradient there, by gs_tsdf_align_system's lerp sequences
 *     gg = (g.x * g.x + g.y * g.y) + g.z * g.z ; gg > 0 and f * f <= gg      (the Newton step is at most one voxel)
 *
 * and then has the point p = lo + ((float(idx) + 0.5f) - (f / gg) * g) * voxel per axis (t = f / gg once, then t * g per
 * axis) and the normal direction g, not normalised: it points into free space.
 *
 * gs_tsdf_plane_votes: votes u32 [6,bins,bins], zeroed by the caller, receives the cube-map histogram of g over all
 *   samples (lo and voxel do not enter).  m = the axis of the largest fabsf(g_m), the lowest on a tie; face = 2 m + (g_m <
 *   0 ? 1 : 0); (u, v) = (g_b / fabsf(g_m), g_c / fabsf(g_m)) for the other two axes b < c; per coordinate the bin is
 *   min(bins - 1, (int)floorf((u + 1.0f) * float(bins / 2))); votes[face, bin(u), bin(v)] += 1.
 * gs_tsdf_plane_offsets: normals f64 [n_planes,3] and o0 f64 [n_planes] on the device, each entry rounded to fp32; hist
 *   u32 [n_planes,n_bins], zeroed by the caller.  A sample agrees with direction n iff d = (n.x * g.x + n.y * g.y) + n.z *
 *   g.z > 0 and d * d >= cos2 * gg.  For every direction j a sample agrees with: kf = floorf((((n.x * p.x + n.y * p.y) +
 *   n.z * p.z) - o0[j]) / bin) ; hist[j, (int)kf] += 1 iff 0 <= kf < float(n_bins) (compared as floats).
 *   Both histograms are sums of integers (fewer than 2^30 cells): the result does not depend on any order.
 * gs_tsdf_plane_workspace_bytes: n_planes * ceil(cells / chunk) * 16 * 8 with chunk = gs_tsdf_align_chunk and cells = (nx -
 *   1)(ny - 1)(nz - 1), the chunks' partial rows; 0 for n_planes outside [0, 16] or a size outside [2, 1024].  Needs no GPU.
 * gs_tsdf_plane_moments: planes f64 [n_planes,4] = (n, o) on the device, each entry rounded to fp32; ref_x, ref_y, ref_z
 *   a point the moments are taken about; workspace of at least gs_tsdf_plane_workspace_bytes; out f64 [n_planes,16],
 *   every element written.  Per plane and per sample that agrees with n (as above; agreeing += 1):
 *
 *     r = ((n.x * p.x + n.y * p.y) + n.z * p.z) - o ; the sample is an inlier iff fabsf(r) <= band ; inliers += 1
 *     q = p - ref per axis (fp32), then in fp64: sum_i += q_i ; sum_ij += q_i * q_j for i <= j ; sq += (double)r * (double)r
 *
 *   out[j] = sum q (3) at 0, sum q q^T at 3 (00 01 02 11 12 22), sq at 9, inliers at 10, agreeing at 11, 0 at 12 .. 15.
 *   Order of every fp64 sum, gs_tsdf_align_system's: chunk c holds the cells [c * chunk, (c + 1) * chunk); within it
 *   thread t of 256 adds its cells t, t + 256, ... in increasing order onto 0.0 (a cell that adds nothing adds nothing),
 *   a wave adds its 64 partials by v += v[lane ^ m] for m = 32, 16, 8, 4, 2, 1, the four waves' totals are added as ((w0 +
 *   w1) + w2) + w3, and the chunks' totals in increasing c starting from chunk 0's.  The two counts are integers.  No
 *   atomics: two runs agree bitwise, and a plane's row does not depend on the other planes of the call.               */
int gs_tsdf_plane_votes(const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight, int bins,
                        unsigned* votes, gs_stream_t stream);
int gs_tsdf_plane_offsets(const float* tsdf, const float* weight, int nx, int ny, int nz, float lo_x, float lo_y, float lo_z,
                          float voxel, float min_weight, const double* normals, const double* o0, int n_planes, float cos2,
                          float bin, int n_bins, unsigned* hist, gs_stream_t stream);
size_t gs_tsdf_plane_workspace_bytes(int n_planes, int nx, int ny, int nz);
int gs_tsdf_plane_moments(const float* tsdf, const float* weight, int nx, int ny, int nz, float lo_x, float lo_y, float lo_z,
                          float voxel, float min_weight, const double* planes, int n_planes, float cos2, float band,
                          float ref_x, float ref_y, float ref_z, void* workspace, double* out, gs_stream_t stream);

/* ---- Euclidean distance field and 2-D occupancy map of that TSDF lattice (no counterpart in the reference),
 *      csrc/esdf.hip; tests/esdf_restatement.py restates it serially ----
 *
 * The lattice is the one above: nx x ny x nz, z contiguous, each size in [2, 1024], 64-bit offsets.  Bad sizes, radii,
 * ranges or NULL pointers return GS_ERR_INVALID_ARG before anything is launched.
 *
 * gs_esdf_build: tsdf, weight f32 [nx,ny,nz] (read only), radius R in [1, 1023] voxels, voxel > 0 finite, min_weight
 *   not NaN.  Outputs state u8, d2 i32, dist f32, all [nx,ny,nz], every element written.
 *     state = 0 (unknown) when !(weight >= min_weight)  (a NaN weight is unknown)
 *             else 2 (solid) when tsdf < 0, else 1 (free; a NaN tsdf is free)
 *     site  : state != 0 and some 6-neighbour inside the lattice has state != 0 and another state (both ends of a sign
 *             change are sites)
 *     d2    : the squared lattice distance to the nearest site, band-limited.  Start value 0 at sites, INF = 0x3fffffff
 *             elsewhere; three passes, along z, then y, then x, each per line of n values
 *               out[i] = min over |k| <= R, 0 <= i + k < n of in[i + k] + k * k
 *             and after the third every value > R * R becomes FAR = 0x7fffffff.  (INF + 1023^2 < 2^31.)
 *             A value <= R * R is the true unbounded squared distance: the nearest site then has every axis offset <= R,
 *             and the three windowed minima are the separable form of the minimum over that cube.  The kernels run
 *               best = in[i] ; for (k = 1; k <= R && k * k < best; ++k) best = min(best, in[i-k] + k*k, in[i+k] + k*k)
 *             which is the same minimum (a term with k * k >= best cannot lower best) and ends after at most R steps.
 *     dist  = sign * (voxel * sqrtf((float)d2)) in metres, sign = -1 where state == 2, else +1; a FAR point gets
 *             sign * (voxel * (float)R).  d2 <= 3 * 1023^2 < 2^24: the conversion is exact; one sqrtf, one multiply.
 *   dist serves as the int32 ping-pong buffer of the passes; there is no other workspace.
 * gs_esdf_query: points f32 [n,3] in world coordinates -> out_dist f32 [n], out_grad f32 [n,3], out_flags u8 [n], every
 *   element written; n == 0 launches nothing.  Per point and axis g = (p - lo) / voxel, a = floorf(g).  Bit 0 of flags
 *   (valid): 0 <= a < float(n - 1) on every axis, compared as floats before the cast (NaN and +-inf fail).  An invalid
 *   point writes zeros and flags = 0.  Otherwise, with v[x][y][z] the cell's eight corners of dist, (sx, sy, sz) = g - a
 *   and lerp(p, q, s) = p + s * (q - p):
 *     zXY = lerp(v[X][Y][0], v[X][Y][1], sz) ; yXZ = lerp(v[X][0][Z], v[X][1][Z], sy)
 *     x0 = lerp(z00, z01, sy) ; x1 = lerp(z10, z11, sy) ; out_dist = lerp(x0, x1, sx)       (lerps z, then y, then x)
 *     out_grad.x = (x1 - x0) / voxel                                                        (lerps z, then y)
 *     out_grad.y = (lerp(z01, z11, sx) - lerp(z00, z10, sx)) / voxel                        (lerps z, then x)
 *     out_grad.z = (lerp(y01, y11, sx) - lerp(y00, y10, sx)) / voxel                        (lerps y, then x)
 *   the analytic gradient of the interpolant, not normalised.  Bit 1 of flags (known): all eight corners have
 *   state != 0.
 * gs_esdf_slice: the map of the slab of layers [k0, k1] (inclusive, 0 <= k0 <= k1 < n) along up_axis in {0, 1, 2};
 *   occ_d2 >= 0, min_known >= 0.  The two other axes, in increasing axis order, index the images cells u8 [n_u,n_v] and
 *   clearance f32 [n_u,n_v].  Per column, layers in increasing order:
 *     occupied = any(state == 2 || d2 <= occ_d2) ; n_known = count(state != 0)
 *     cells = 0 when occupied, else 254 when n_known >= min_known, else 205    (the trinary values of a map_server PGM)
 *     clearance = the minimum of dist: c = dist[k0], then c = dist[k] where dist[k] < c.                            */
int gs_esdf_build(const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight, int radius,
                  float voxel, unsigned char* state, int* d2, float* dist, gs_stream_t stream);
int gs_esdf_query(const float* dist, const unsigned char* state, int nx, int ny, int nz, float lo_x, float lo_y,
                  float lo_z, float voxel, const float* points, int n, float* out_dist, float* out_grad,
                  unsigned char* out_flags, gs_stream_t stream);
int gs_esdf_slice(const unsigned char* state, const int* d2, const float* dist, int nx, int ny, int nz, int up_axis,
                  int k0, int k1, int occ_d2, int min_known, unsigned char* cells, float* clearance, gs_stream_t stream);

/* ---- Cost-to-go field and paths over a passability lattice (no counterpart in the reference), csrc/geodesic.hip;
 *      tests/geodesic_restatement.py restates it serially ----
 *
 * The lattice is n0 x n1 x n2, the last axis contiguous, each size in [1, 1024] (a 2-D map [n_u,n_v] is the lattice
 * [1,n_u,n_v]), 64-bit offsets.  passable u8: non-zero where the robot's centre may be.  Bad sizes, ranges or NULL
 * pointers return GS_ERR_INVALID_ARG before anything is launched; every entry point enqueues on the stream and reads
 * nothing back.
 *
 * Moves: the 26 neighbours (d0,d1,d2) in {-1,0,1}^3 without 0, indexed in that nesting order (d0 outermost, d2
 *   innermost; move 0 is (-1,-1,-1), move 25 is (1,1,1)).  Weight by the number of non-zero components, in milli-voxels:
 *   1000, 1414, 1732 for 1, 2, 3.  A move from c to c + d is allowed only if every cell of the axis-aligned box spanned
 *   by c and c + d (2, 4 or 8 cells, both ends included) lies inside the lattice and is passable: no corner is cut, and
 *   the rule is symmetric in its ends.
 * cost i32 [n0,n1,n2], every element written: 0 at a passable seed; elsewhere the minimum over paths of allowed moves
 *   from any seed of the summed weights if that is <= max_cost, else GS_GEO_INF.  max_cost in [0, GS_GEO_INF - 1732]: no
 *   candidate neighbour + w overflows, and one above max_cost is never stored.  Prefixes of a shortest path are shortest
 *   paths and weights are positive, so the capped field is the uncapped one with every value above max_cost replaced by
 *   GS_GEO_INF.  The field is the least fixed point of cost[c] = min(cost[c], cost[n] + w) over allowed moves, and it is
 *   unique: the result does not depend on the order or the number of relaxations, only that none is left.
 *
 * gs_geodesic_brick: the relaxation's brick (b0, b1, b2); flags are u8 [2][ceil(n0/b0) * ceil(n1/b1) * ceil(n2/b2)],
 *   gs_geodesic_flags_bytes gives that size (0 for sizes outside [1, 1024]).  The flags belong to the library between
 *   gs_geodesic_init and the last gs_geodesic_relax of a field.
 * gs_geodesic_init: seeds i32 [m,3], m >= 0 (NULL allowed for m == 0).  cost = GS_GEO_INF everywhere, then 0 at every
 *   seed that is inside the lattice and passable (others are ignored, duplicates are harmless); both flag buffers
 *   cleared, then the bricks that hold such a seed marked in buffer 0.
 * gs_geodesic_relax, and gs_frontier_relax below on its labels: sweeps sweep0 .. sweep0 + k - 1, k >= 1, sweep0 >= 0
 *   the number of sweeps enqueued on this field so far (it selects the flag buffer: sweep s reads buffer s & 1 and
 *   writes the other).  changed u32 [k]: entry s is non-zero iff sweep sweep0 + s lowered any cell.  One zero entry
 *   proves the fixed point; sweeps after it do nothing.  The number of sweeps a field needs may differ between runs;
 *   the field does not.
 * gs_geodesic_path: start i32[3] by value, max_len >= 1, out_cells i32 [max_len,3], out_n i32 [1].  out_n = 0 when
 *   start lies outside the lattice or holds GS_GEO_INF.  Otherwise out_cells[0] = start, and each step goes to the allowed
 *   neighbour with the smallest cost[n] + w among those with cost[n] < GS_GEO_INF, ties to the lowest move index (at the
 *   fixed point that smallest value is cost[cur]).  The walk ends on a cell of cost 0, which is included; out_n is the
 *   number of cells.  out_n = -1 when max_len cells do not suffice or no such neighbour exists (a field off its fixed
 *   point).  At the fixed point a finite non-zero cell has a neighbour at least 1000 lower: cost / 1000 + 1 cells
 *   suffice.                                                                                                      */
#define GS_GEO_INF 0x3fffffff
#define GS_GEO_MAX_COST (GS_GEO_INF - 1732)
int gs_geodesic_brick(int* b0, int* b1, int* b2);
size_t gs_geodesic_flags_bytes(int n0, int n1, int n2);
int gs_geodesic_init(const unsigned char* passable, int n0, int n1, int n2, const int* seeds, int m, int* cost,
                     unsigned char* flags, gs_stream_t stream);
int gs_geodesic_relax(const unsigned char* passable, int n0, int n1, int n2, int max_cost, int* cost,
                      unsigned char* flags, int sweep0, int k, unsigned int* changed, gs_stream_t stream);
int gs_geodesic_path(const int* cost, const unsigned char* passable, int n0, int n1, int n2, int start0, int start1,
                     int start2, int max_len, int* out_cells, int* out_n, gs_stream_t stream);

/* ---- Frontiers of a state lattice: free cells next to never-observed space, their clusters and one table row per
 *      cluster (no counterpart in the reference), csrc/frontier.hip; tests/frontier_restatement.py restates it serially
 *       ----
 *
 * The lattice is n0 x n1 x n2, the last axis contiguous, each size in [1, 1024] (a 2-D map [n_u,n_v] is the lattice
 * [1,n_u,n_v]): a linear index ((c0 * n1) + c1) * n2 + c2 fits in 30 bits.  state u8: 0 unknown, 1 free, any other value
 * solid (gs_esdf_build writes 2).  open u8 or NULL: non-zero where a frontier cell may be (NULL: everywhere).  cost i32 or
 * NULL: a gs_geodesic_* field over the same lattice, GS_GEO_INF where unreachable.  Everything is integer.  Bad sizes,
 * ranges or NULL where a pointer is needed return GS_ERR_INVALID_ARG before anything is launched; every entry point
 * enqueues on the stream and reads nothing back.
 *
 * Frontier cell: state == 1, open == NULL || open != 0, and at least one of the 6 face neighbours lies inside the lattice
 *   and has state == 0.  The lattice's own border is not unknown.
 * Clusters: the connected components of the frontier cells under 26-connectivity (the neighbours (d0,d1,d2) in
 *   {-1,0,1}^3 without 0).  label i32: -1 off the frontier, else the smallest linear index in the cell's component.  It is
 *   the fixed point of label[c] = min(label[c], label[n]) over frontier neighbours n, started from label = own index,
 *   and it is unique: the result does not depend on the order or the number of relaxations, only that none is left.
 * Table: K rows, one per cluster, ascending root; the row number is the cluster's id.
 *     root i32 [K]      the cluster's label
 *     size i32 [K]      its number of cells
 *     faces i32 [K]     the number of pairs (cell of the cluster, face neighbour inside the lattice with state == 0)
 *     sum i64 [K,3]     the sums of the cells' coordinates (c0, c1, c2)
 *     bbox i32 [K,6]    (min c0, min c1, min c2, max c0, max c1, max c2)
 *     best i32 [K,2]    8-byte aligned; row r read as one little-endian u64 is the minimum over the cluster's cells of
 *                       (cost << 32) | linear index, so [r][0] = best_cell, the cheapest cell, ties to the lowest index,
 *                       and [r][1] = best_cost.  cost == NULL counts as GS_GEO_INF everywhere: best_cell is the root.
 *
 * gs_frontier_brick: the relaxation's brick (b0, b1, b2); flags are u8 [2][ceil(n0/b0) * ceil(n1/b1) * ceil(n2/b2)],
 *   gs_frontier_flags_bytes gives that size (0 for sizes outside [1, 1024]).  The flags belong to the library between
 *   gs_frontier_mark and the last gs_frontier_relax of a lattice.
 * gs_frontier_mark: frontier u8 (0 / 1) and label (own index / -1), every element written; counts u32 [4] = the number
 *   of unknown, free, solid and frontier cells; both flag buffers cleared, then the bricks that hold a frontier cell
 *   marked in buffer 0.
 * gs_frontier_relax: sweep0, k, the flag buffers and changed as for gs_geodesic_relax, with "label" for "cell".
 * gs_frontier_roots: counts the roots (label == own index) per block of cells and scans the counts into the workspace
 *   (gs_frontier_workspace_bytes; 0 for sizes outside [1, 1024]); n_roots i32 [1] = K, which the caller reads to size the
 *   table.
 * gs_frontier_table: rows = K as read from gs_frontier_roots of the same labels and workspace, capacity = the number of
 *   rows the table's arrays hold; 0 <= rows <= capacity, else GS_ERR_INVALID_ARG.  rows == 0 launches nothing.  Rows
 *   [0, rows) of every column are written.  (With rows below the true K the roots past the table and their clusters are
 *   left out; nothing is written outside [0, rows).)                                                                  */
int gs_frontier_brick(int* b0, int* b1, int* b2);
size_t gs_frontier_flags_bytes(int n0, int n1, int n2);
size_t gs_frontier_workspace_bytes(int n0, int n1, int n2);
int gs_frontier_mark(const unsigned char* state, const unsigned char* open, int n0, int n1, int n2,
                     unsigned char* frontier, int* label, unsigned int* counts, unsigned char* flags, gs_stream_t stream);
int gs_frontier_relax(int n0, int n1, int n2, int* label, unsigned char* flags, int sweep0, int k, unsigned int* changed,
                      gs_stream_t stream);
int gs_frontier_roots(const int* label, int n0, int n1, int n2, void* workspace, size_t workspace_bytes, int* n_roots,
                      gs_stream_t stream);
int gs_frontier_table(const unsigned char* state, const int* label, const int* cost, int n0, int n1, int n2,
                      const void* workspace, size_t workspace_bytes, int rows, int capacity, int* root, int* size,
                      int* faces, long long* sum, int* bbox, int* best, gs_stream_t stream);

/* ---- Objects: the surface samples of a TSDF lattice that lie on none of the given structure planes, their clusters and
 *      one table row per cluster (no counterpart in the reference), csrc/tsdf_objects.hip;
 *      tests/tsdf_objects_restatement.py restates it ----
 *
 * tsdf, weight, the lattice, lo, voxel, min_weight, the surface sample (p, g, gg) of a cell, "agrees" and the fp32
 * operation order are those of the plane block above (gs_tsdf_plane_*).  The cell lattice is (cx, cy, cz) = (nx - 1, ny -
 * 1, nz - 1), cell s = (a * cy + b) * cz + c; kind, label and every "cell" below are indexed by s.  Sizes outside [2, 1024]
 * (cell lattices outside [1, 1024]), a NULL pointer, n_planes outside [0, 16], a voxel that is not positive and finite, a lo
 * or min_weight that is not finite, cos2 outside [0, 1], band < 0 or not finite, rows < 0 or above capacity, a workspace
 * that is too small return GS_ERR_INVALID_ARG before anything is launched or written.
 *
 * gs_tsdf_object_mark: planes f64 [n_planes,4] = (n, o) on the device, each entry rounded to fp32.  kind u8 [cells] and
 *   label i32 [cells], every element written; counts u32 [4]; flags as gs_frontier_flags_bytes(cx, cy, cz) sizes them.
 *     no sample                     kind = 0, label = -1
 *     for a sample and plane j      r_j = ((n.x * p.x + n.y * p.y) + n.z * p.z) - o ; near_j = fabsf(r_j) <= band ;
 *                                   on_j = near_j and the sample agrees with n_j
 *     structure                     some on_j, or near_j for at least two j (a crease between two planes):
 *                                   kind = 2 + j*, label = -1, j* the lowest j with on_j, else the lowest j with near_j
 *     otherwise an object cell      kind = 1, label = s
 *   counts = samples, object cells, structure cells, crease cells (structure without any on_j).  n_planes == 0: every
 *   sample is an object cell.  Both flag buffers are cleared and the bricks (gs_frontier_brick) that hold an object cell
 *   marked in buffer 0, as gs_frontier_mark does: gs_frontier_relax(cx, cy, cz, label, flags, ...) and gs_frontier_roots
 *   run on the result as they are, and the labels' fixed point is the smallest cell index of each 26-connected cluster.
 * gs_tsdf_object_table: workspace as filled by gs_frontier_roots of these labels; rows, capacity and what is written as
 *   for gs_frontier_table.  One row per cluster, ascending root:
 *     root i32 [K], size i32 [K]
 *     sum i64 [K,3]     the sums of the cells' coordinates (c0, c1, c2); 8-byte aligned
 *     sum2 i64 [K,6]    the sums of their products 00 01 02 11 12 22; 8-byte aligned.  Below 2^30 * 2^20.
 *     bbox i32 [K,6]    mins, then maxes
 *     touch u32 [K]     bit j set iff some cell of the cluster has a 26-neighbour inside the cell lattice with kind == 2 + j
 *   Integer add, min, max and or: the rows do not depend on any order.
 * gs_tsdf_object_extents: label at its fixed point, root and rows of the table; axes f64 [rows,3,3] on the device, each
 *   entry rounded to fp32; ext u32 [rows,3,2], every entry written; rows == 0 launches nothing.  Every cell with label >= 0
 *   whose label is one of root[0 .. rows) and which is a sample adds t_m = (a.x * p.x + a.y * p.y) + a.z * p.z for the
 *   three axes a = axes[row, m] of its row: ext[row, m, 0] is the minimum and ext[row, m, 1] the maximum of e(t_m) as
 *   unsigned integers, e(x) = bits(x) ^ (bits(x) >> 31 ? 0xffffffff : 0x80000000), which orders as the floats do.  A row
 *   without such a cell holds e(+inf) = 0xff800000 and e(-inf) = 0x007fffff.                                          */
int gs_tsdf_object_mark(const float* tsdf, const float* weight, int nx, int ny, int nz, float lo_x, float lo_y, float lo_z,
                        float voxel, float min_weight, const double* planes, int n_planes, float cos2, float band,
                        unsigned char* kind, int* label, unsigned int* counts, unsigned char* flags, gs_stream_t stream);
int gs_tsdf_object_table(const unsigned char* kind, const int* label, int cx, int cy, int cz, const void* workspace,
                         size_t workspace_bytes, int rows, int capacity, int* root, int* size, long long* sum,
                         long long* sum2, int* bbox, unsigned int* touch, gs_stream_t stream);
int gs_tsdf_object_extents(const float* tsdf, const float* weight, int nx, int ny, int nz, float lo_x, float lo_y,
                           float lo_z, float voxel, float min_weight, const int* label, const int* root, int rows,
                           const double* axes, unsigned int* ext, gs_stream_t stream);

/* ---- Rooms: the free space of a passability lattice split by clearance, the doorways between the parts and one table
 *      row per room and per doorway (no counterpart in the reference), csrc/rooms.hip; tests/rooms_restatement.py restates
 *      it serially ----
 *
 * The lattice, its linear index p, the 26 moves with weights 1000 / 1414 / 1732, "allowed move" (every cell of the box
 * the move's two ends span is inside the lattice and open) and GS_GEO_INF are those of the geodesic block above.  open u8:
 * non-zero where the robot's centre may be.  core u8: non-zero where it has room to spare.  d2 i32 or NULL: the squared
 * clearance in voxels (gs_esdf_build's d2); NULL and negative values count as 0.  Everything is integer.
 *
 * 1. Core cell: open != 0 && core != 0.  Core components: the 26-connected components of the core cells under plain
 *    adjacency (gs_frontier_relax's rule).  A component's root is its smallest linear index.  A component is kept when the
 *    caller's keep byte of its row is non-zero (the caller keeps those of at least min_core_cells cells); the cells of a
 *    dropped component are ordinary open cells from there on.
 * 2. cost: the gs_geodesic_* field over open seeded at every kept core cell.
 * 3. Room label R(p): a kept core cell holds its component's root; an open cell with 0 < cost[p] < GS_GEO_INF holds the
 *    smallest R(p + m) over its parents, the allowed moves m with cost[p + m] + w(m) == cost[p] (at the cost's fixed point
 *    there is at least one); every other cell holds -1.  Equivalently R(p) is the smallest root among the kept cores whose
 *    distance to p equals cost[p].  It is the unique fixed point of label[p] = min(label[p], label[p + m]) over parents.
 * 4. Boundary cell: R(p) >= 0 and some allowed move m with R(p + m) >= 0 and R(p + m) != R(p).
 * 5. Doorways: the 26-connected components of the boundary cells under plain adjacency; door_label i32: -1 off them, else
 *    the component's smallest linear index.
 * 6. Room table, one row per kept core by ascending root, the row number is the room's id:
 *      root i32 [K], size i32 [K] (cells with R == root), core_size i32 [K] (those of them with cost 0: the kept core),
 *      sum i64 [K,3] (8-byte aligned), bbox i32 [K,6] (mins, then maxes), reach i32 [K] (the largest cost in the room)
 * 7. Door table, one row per doorway by ascending root:
 *      root, size, sum, bbox as above over the doorway's cells
 *      room_lo, room_hi i32 [D]   the smallest and largest label found on the doorway's cells and across their allowed
 *                                 moves to a differing label (at a junction of three rooms: only the extremes)
 *      widest u64 [D]             8-byte aligned; the maximum over the doorway's cells of (d2 << 32) | (0xffffffff - p):
 *                                 the cell with the largest d2, ties to the lowest index
 *
 * Sizes outside [1, 1024], a NULL pointer where one is needed, rows < 0 or above capacity, a workspace that is too small
 * or a misaligned 64-bit column return GS_ERR_INVALID_ARG before anything is launched or written.  Every entry enqueues
 * on the stream and reads nothing back.  flags are gs_frontier_flags_bytes' two buffers (the brick is gs_frontier_brick's),
 * the workspace is gs_frontier_workspace_bytes'.
 *
 * gs_room_mark: label = own index on a core cell, -1 elsewhere, every element written; counts u32 [2] = open cells, core
 *   cells; both flag buffers cleared, then the bricks that hold a core cell marked in buffer 0: gs_frontier_relax and
 *   gs_frontier_roots run on the result as they are.
 * gs_room_cores: workspace as filled by gs_frontier_roots of `label` at its fixed point, rows = its K.  root [rows]
 *   ascending and size [rows] (or NULL: not wanted), the components' numbers of cells.  rows == 0 launches nothing.
 *   (Any label lattice of gs_frontier_relax serves: the doorways' too.)
 * gs_room_seed: root, keep u8 [rows]; label = -1 on every cell whose label is no root with a non-zero keep byte; both flag
 *   buffers cleared, then every brick that holds an open cell marked in buffer 0, which contains every brick in which
 *   a cell can be the first to take a label.
 * gs_room_relax: cost at its fixed point over `open` seeded at the cells label >= 0; sweep0, k, the flag buffers and
 *   changed as for gs_geodesic_relax, with "label" for "cell".
 * gs_room_door_mark: label at gs_room_relax's fixed point; door_label = own index on a boundary cell, -1 elsewhere, every
 *   element written; count u32 [1] = boundary cells; flags as gs_room_mark leaves them, for the boundary cells.
 * gs_room_table / gs_room_door_table: root [rows] ascending, as gs_room_cores wrote it (for the rooms: its kept rows);
 *   rows [0, rows) of every other column are written; rows == 0 launches nothing.  Integer add, min and max: the rows do
 *   not depend on any order.                                                                                           */
int gs_room_mark(const unsigned char* open, const unsigned char* core, int n0, int n1, int n2, int* label,
                 unsigned int* counts, unsigned char* flags, gs_stream_t stream);
int gs_room_cores(const int* label, int n0, int n1, int n2, const void* workspace, size_t workspace_bytes, int rows,
                  int capacity, int* root, int* size, gs_stream_t stream);
int gs_room_seed(const unsigned char* open, int n0, int n1, int n2, const int* root, const unsigned char* keep, int rows,
                 int* label, unsigned char* flags, gs_stream_t stream);
int gs_room_relax(const unsigned char* open, const int* cost, int n0, int n1, int n2, int* label, unsigned char* flags,
                  int sweep0, int k, unsigned int* changed, gs_stream_t stream);
int gs_room_door_mark(const unsigned char* open, const int* label, int n0, int n1, int n2, int* door_label,
                      unsigned int* count, unsigned char* flags, gs_stream_t stream);
int gs_room_table(const int* label, const int* cost, int n0, int n1, int n2, const int* root, int rows, int* size,
                  int* core_size, long long* sum, int* bbox, int* reach, gs_stream_t stream);
int gs_room_door_table(const unsigned char* open, const int* label, const int* door_label, const int* d2, int n0, int n1,
                       int n2, const int* root, int rows, int* size, long long* sum, int* bbox, int* room_lo, int* room_hi,
                       unsigned long long* widest, gs_stream_t stream);

/* ---- Line of sight over a passability lattice and the shortest shortcut of a path (no counterpart in the reference),
 *      csrc/sight_walk.h and csrc/sight.hip; tests/sight_restatement.py restates it serially ----
 *
 * The lattice, its linear index and passable u8 are those of the geodesic block above (each size in [1, 1024]).  A cell is
 * three i32 (c0, c1, c2); a segment is six, a then b.  Everything is integer apart from one fp64 sqrt per leg length.
 *
 * Supercover of the cells a and b: the cells whose closed unit cube, centred on the lattice point, meets the closed
 *   segment between the two centres.  a sees b over passable when both lie inside the lattice and every cell of the
 *   supercover is passable.  The walk that lists it (sight_walk.h), d = b - a, w_k = |d_k|, g_k = sign(d_k), one counter
 *   k_k per axis from 0 and the offset f from a, f = 0 at first:
 *     a is visited first.  While some k_k < w_k: the axes with k_k < w_k cross next at (2 k_k + 1) / (2 w_k), compared
 *     exactly by cross-multiplying (products below 2^21); S is the set of axes that hold the smallest crossing; the cells
 *     a + f + sum_{k in T} g_k e_k are visited for every non-empty T within S (1, 3 or 7 cells: a segment through an edge
 *     or a corner touches every cube around it, and a robot does not slip between two cells that touch there); then f
 *     and k advance along every axis of S.  At most w_0 + w_1 + w_2 steps, no cell twice, every cell inside the box the
 *     two ends span, the same set from b to a.  For a and b one move apart it is the box of the geodesic block's move
 *     rule.
 * len(a, b) = floor(sqrt(1000000 * |b - a|^2)), the leg's length in milli-voxels, in 64-bit integers (an fp64 sqrt and a
 *   correction by one): 1000, 1414, 1732 for the 26 moves, at most 1771887.
 *
 * gs_segment_sight: segs i32 [n,6], n >= 0 (n == 0 launches nothing); out u8 [n], every element written: 1 when a sees
 *   b, else 0 (an end outside the lattice: 0).
 * gs_segment_min: field i32 [n0,n1,n2]; out_value i32 [n] the smallest field value over the supercover, out_cell i32
 *   [n] the lowest linear index that holds it; an end outside the lattice: INT32_MIN and -1.
 * gs_path_sight: cells i32 [L,3], 1 <= L <= GS_PATH_MAX_CELLS; window W with 1 <= W <= L - 1, or W == 1 when L == 1;
 *   sight u64 [L, ceil(W / 64)], 8-byte aligned, every word written: bit (b & 63) of word b / 64 of row j is set iff
 *   0 <= b < min(W, j) and cell j - 1 - b sees cell j; every other bit is 0.  A path cell outside the lattice or not
 *   passable sees nothing and is seen by nothing.
 * gs_path_shortcut: sight and cells as gs_path_sight wrote and read them, the same L and W.  The shortest route from
 *   cell 0 to cell L - 1 over the path's own cells whose legs see: dp[0] = 0, dp[j] = the minimum over the i with bit
 *   j - 1 - i of row j set and dp[i] reached of dp[i] + len(i, j), ties to the lowest i; a sum of 2^31 - 1 or more
 *   counts as not reached (a path of adjacent cells stays below 2^25).  n_out i32 [1] = K, the number of cells kept,
 *   index i32 [L] of which [0, K) are written, ascending, index[0] = 0 and index[K - 1] = L - 1, and length i32 [1] =
 *   dp[L - 1].  When cell L - 1 is not reached n_out = -1 and nothing else is written.  One workgroup; dp and the
 *   predecessors take 6 L bytes of LDS.
 * A NULL pointer, a size outside [1, 1024], n < 0, L or W outside the ranges above or a misaligned sight return
 * GS_ERR_INVALID_ARG before anything is launched or written; every entry enqueues on the stream and reads nothing back. */
#define GS_PATH_MAX_CELLS 16384
int gs_segment_sight(const unsigned char* passable, int n0, int n1, int n2, const int* segs, int n, unsigned char* out,
                     gs_stream_t stream);
int gs_segment_min(const int* field, int n0, int n1, int n2, const int* segs, int n, int* out_value, int* out_cell,
                   gs_stream_t stream);
int gs_path_sight(const unsigned char* passable, int n0, int n1, int n2, const int* cells, int L, int window,
                  unsigned long long* sight, gs_stream_t stream);
int gs_path_shortcut(const unsigned long long* sight, const int* cells, int L, int window, int* index, int* n_out,
                     int* length, gs_stream_t stream);

/* ---- Following a route: a sampled-rollout (model-predictive path-integral) controller of a differential-drive base over
 *      the distance field and a cost-to-go field (no counterpart in the reference), csrc/follow.hip;
 *      tests/follow_restatement.py restates it serially ----
 *
 * The lattice is gs_esdf_query's (n0 x n1 x n2, the last axis contiguous, each size in [2, 1024], lo, voxel).  dist f32
 * [n0,n1,n2] is gs_esdf_build's; togo i32 [n0,n1,n2] is a gs_geodesic_* cost field seeded at the goal, in milli-voxels,
 * >= INF = 0x3fffffff where the robot's centre may not be.  The robot moves in the plane perpendicular to up_axis in
 * {0, 1, 2} at the world coordinate `height` on it; the two other axes, in increasing order, are (u, v), as in
 * gs_esdf_slice.  State (x, y, c, s): the position on (u, v) in metres and the heading as a unit vector.  Controls (v, w):
 * speed in m/s and yaw rate in rad/s, 0 <= v <= v_max, |w| <= w_max.  K rollouts, 1 <= K <= GS_FOLLOW_MAX_ROLLOUTS, of
 * T steps, 1 <= T <= GS_FOLLOW_MAX_STEPS; U f32 [T,2] the nominal controls, noise f32 [T,K,2], both 8-byte aligned.
 *
 * Everything of a rollout is fp32, one rounding per operation, no fma, in exactly this order.
 *   control(U[t], noise[t,k]): per component a = U + noise, a = U when a is NaN or +-inf; then
 *     v = a_v < 0 ? 0 : (a_v > v_max ? v_max : a_v) ; w = a_w < -w_max ? -w_max : (a_w > w_max ? w_max : a_w)
 *   step: h = (0.5 * dt) * w ; den = 1 + h * h ; cr = (1 - h * h) / den ; sr = (2 * h) / den
 *         c' = c * cr - s * sr ; s' = s * cr + c * sr ; x' = x + (dt * v) * c' ; y' = y + (dt * v) * s'
 *     (Cayley's form of a rotation: exactly one by 2 atan(h), which is w dt up to (w dt)^3 / 12, and no transcendental.)
 *   sample(x, y): the world point p with p[up_axis] = height, p[u] = x, p[v] = y; per axis g = (p - lo) / voxel and
 *     a = floorf(g).  It is a collision when not 0 <= a < float(n - 1) on every axis (compared as floats; NaN fails) or
 *     when togo at the nearest lattice point (int)floorf(g + 0.5) is >= INF.  Otherwise
 *       d = gs_esdf_query's out_dist, the lerps z, then y, then x of the cell's corners of dist at g - a
 *       togo_term = w_togo * (float(togo) * (voxel / 1000)) ; cost = togo_term
 *       cost = cost + (w_clear * ((robot_radius + margin) - d)) / margin        only when d < robot_radius + margin
 *   rollout k: state = the start; frozen = sample(start).cost and last = its togo_term, both 0 when the start collides;
 *     S = 0 ; hit = T ; closest = +inf.  For t = 0 .. T - 1, while hit == T: the control, the step, the sample of the
 *     stepped point.  Live: the state moves there, frozen = cost + w_turn * (w * w), last = togo_term, closest = d where
 *     d < closest, S = S + frozen.  A collision: hit = t, S = S + collision_cost, then S = S + frozen, and the state
 *     stays.  Every later step: S = S + frozen.  After the loop S = S + w_end * last when hit == T.
 * gs_follow_rollouts: outputs S f32 [K], end f32 [K,4] the last state, hit_step i32 [K] (T: never collided), min_dist f32
 *   [K] (closest), every element written.  One lane per rollout.
 * gs_follow_weights: S f32 [K] without NaN -> s_min f32 [1] the smallest S, best i32 [1] the lowest k that holds it,
 *   omega f64 [K] = exp(-(double(S[k]) - double(s_min)) / double(lambda)), stats f64 [2] = (eta, ess) with eta = sum omega
 *   and ess = eta * eta / sum omega^2.  One workgroup.
 * gs_follow_update: per step t, delta[t,k] = control(U[t], noise[t,k]) - U[t] per component in fp32, the perturbation the
 *   rollout applied (recomputed, nothing [T,K,2] is stored), mean = sum_k omega[k] * double(delta[t,k]) / stats[0] in
 *   fp64, row = U[t] + float(mean) clamped as the control is.  shift == 0: U_new[t] = row.  shift == 1: U_new[t - 1] = row
 *   for t >= 1 and U_new[T - 1] = row of T - 1 as well (the last row is repeated).  u_exec f32 [2] gets row 0 (needed with
 *   shift == 1; may be NULL without).  U_new f32 [T,2] is another buffer than U.  One workgroup per step.
 * Sums over k: a thread adds the elements k = tid, tid + threads, ... in that order, a wave adds by the xor butterfly
 *   (offsets 32 .. 1), thread 0 adds the waves' sums in increasing order; no atomics, so the same inputs give the same
 *   bits, and any order is within K * 2^-52 relative of the exact sum since every term of eta is positive.
 * Bad sizes, a NULL or misaligned pointer, a parameter that is not finite, dt, v_max, w_max, margin, voxel or lambda that
 * is not positive, a negative weight, radius or collision_cost return GS_ERR_INVALID_ARG before anything is launched or
 * written; every entry enqueues on the stream and reads nothing back.                                                  */
#define GS_FOLLOW_MAX_ROLLOUTS 65536
#define GS_FOLLOW_MAX_STEPS 256
int gs_follow_rollouts(const float* dist, const int* togo, int n0, int n1, int n2, float lo_x, float lo_y, float lo_z,
                       float voxel, int up_axis, float height, float x, float y, float c, float s, const float* U,
                       const float* noise, int K, int T, float dt, float v_max, float w_max, float robot_radius,
                       float margin, float w_togo, float w_clear, float w_turn, float w_end, float collision_cost,
                       float* S, float* end, int* hit_step, float* min_dist, gs_stream_t stream);
int gs_follow_weights(const float* S, int K, float lambda, float* s_min, int* best, double* omega, double* stats,
                      gs_stream_t stream);
int gs_follow_update(const float* U, const float* noise, const double* omega, const double* stats, int K, int T,
                     float v_max, float w_max, int shift, float* U_new, float* u_exec, gs_stream_t stream);

/* ---- Drivable floor: an elevation map of a state lattice and the map of where a ground robot's base can stand and roll
 *      on it (no counterpart in the reference), csrc/floor.hip; tests/floor_restatement.py restates it serially
 *       ----
 *
 * state u8 [nx,ny,nz] is gs_esdf_build's (0 unseen, 1 free, 2 solid), each size in [2, 1024].  up_axis in {0, 1, 2},
 * up_sign in {+1, -1}.  The position p along up of the lattice index k is k for up_sign = +1 and n_a - 1 - k for -1, n_a
 * the size along up_axis; "above" is a larger p; a position beyond the lattice counts as unseen.  The two other axes, in
 * increasing order, are (u, v) and index every image [n_u,n_v], as in gs_esdf_slice.  Integers only, no atomics: the same
 * inputs give the same bits for every up_axis.
 *
 * gs_floor_columns: the band 0 <= p0 <= p1 < n_a of positions the robot's base may rest at, the headroom H >= 1 in cells.
 *   Per column a position p is a stand when p >= 1, state[p - 1] == 2 (seen support directly beneath) and state[j] != 2
 *   for every j in p .. p + H - 1; it is strict when all those cells lie inside the lattice and are free (== 1).  With F
 *   the lowest stand in p0 <= p <= p1, floor i16 [n_u,n_v] and kind u8 [n_u,n_v], every element written:
 *     F strict                      floor = the lattice index k of F (not p), kind = 1
 *     F not strict ("maybe")        floor = the lattice index k of F,         kind = 2
 *     no stand, no cell at a position in [max(p0 - 1, 0), min(p1 + H - 1, n_a - 1)] is solid and at least one of them is
 *       unseen (the floor was never observed)                                 floor = -1, kind = 0
 *     anything else (a wall, too low, a hole seen free to the bottom)         floor = -1, kind = 3
 *   One walk per column over exactly those positions.
 * gs_floor_footprint: floor, kind [n_u,n_v] as above, n_u and n_v in [2, 1024]; the robot's disc is the offsets (du, dv)
 *   with du * du + dv * dv <= R2, 2 <= R2 <= 1024 (the eight neighbours always belong to it, so a move between two
 *   drivable neighbours never climbs more than S); S >= 0 the largest height difference in cells inside the disc.  A
 *   column q of the disc outside the map counts as kind 0.  Per column c, cells u8 (254 free, 0 occupied, 205 unknown: a
 *   map_server PGM's values), why u8 and rough i16, all [n_u,n_v], every element written, rules in this order:
 *     kind[c] == 3                                                      cells = 0,   why = 1
 *     kind[c] == 0                                                      cells = 205, why = 0
 *     some q of the disc has kind 3                                     cells = 0,   why = 2
 *     some q of kind 1 or 2 has |floor[q] - floor[c]| > S               cells = 0,   why = 3
 *     kind[c] == 2 or some q has kind 0 or 2                            cells = 205, why = 0
 *     otherwise                                                         cells = 254, why = 0
 *   rough[c] = the largest |floor[q] - floor[c]| over the disc's columns of kind 1 or 2; 0 when kind[c] is 0 or 3.
 * A NULL pointer, a size outside [2, 1024], a bad axis or sign, an empty or out-of-range band, H < 1, S < 0 or R2 outside
 * its range return GS_ERR_INVALID_ARG before anything is launched or written; both entries enqueue on the stream and read
 * nothing back.                                                                                                        */
int gs_floor_columns(const unsigned char* state, int nx, int ny, int nz, int up_axis, int up_sign, int p0, int p1, int H,
                     short* floor, unsigned char* kind, gs_stream_t stream);
int gs_floor_footprint(const short* floor, const unsigned char* kind, int n_u, int n_v, int R2, int S,
                       unsigned char* cells, unsigned char* why, short* rough, gs_stream_t stream);

/* ---- View gain: the cells of a state lattice that a camera's rays cross from a candidate pose (no counterpart in the
 *      reference), csrc/view_gain.hip; tests/view_gain_restatement.py restates it serially ----
 *
 * The lattice and state are those of the frontier block above (each size in [1, 1024]; 0 unknown, 1 free, any other value
 * solid).  origins i32 [V,3] in cells, V >= 0 (V == 0 launches nothing).  dirs i32 [R,3], 1 <= R <= 65536, the same rays
 * for every view of the call, every component in [-GS_VIEW_MAX_DIR, GS_VIEW_MAX_DIR]; an all-zero direction casts nothing
 * (nor does one with a component outside that range: the caller's mistake, made harmless).  range2 in [1, 3 * 1023^2], the
 * squared range in cells.  max_unknown >= 0, 0 for no limit.  box: six HOST ints lo0, lo1, lo2, hi0, hi1, hi2, offsets
 * from a view's origin with lo <= 0 <= hi on every axis and at most GS_VIEW_MAX_BOX_CELLS cells prod(hi - lo + 1).
 * Everything is integer.  Bad sizes, ranges, NULL where a pointer is needed or such a box return GS_ERR_INVALID_ARG
 * before anything is launched or written; the call enqueues on the stream and reads nothing back.
 *
 * The walk of one ray, origin o, direction d, s_a = sign(d_a), w_a = |d_a|, one step counter k_a per axis from 0:
 *   the ray visits o first.  The next cell lies one step along s_a on the axis a with w_a != 0 that minimises the time
 *   (2 k_a + 1) / (2 w_a) at which a ray from the cell's centre crosses into it, compared exactly: a beats b when
 *   (2 k_a + 1) * w_b < (2 k_b + 1) * w_a, a tie goes to the lower axis (both products stay below 2^31).  The ray ends,
 *   without visiting that cell, when it lies outside the lattice, outside o + [lo, hi], or at a squared distance from o
 *   above range2; else k_a goes up by one and the cell is visited.  After visiting a solid cell the ray ends.  After
 *   visiting its max_unknown-th unknown cell (counted per ray, over every unknown cell it crosses) it ends, when
 *   max_unknown > 0.  The offsets never shrink, so a ray takes at most floor(sqrt(3 * range2)) steps.
 * A view whose origin lies outside the lattice casts nothing.
 * gain u32 [V,4]: per view the number of distinct unknown, free and solid cells visited by any of its rays, and their
 *   sum, the distinct cells in all.  A set has no order: the counts do not depend on the order of rays or lanes.
 * gs_view_gain_lds_bytes: the dynamic LDS one workgroup (one view) takes for this box, one bit per cell plus the
 *   reduction's words; 0 for a box the call refuses.                                                                  */
#define GS_VIEW_MAX_BOX_CELLS 1048576        /* one bit per cell: 128 KiB of the CU's 160 KiB of LDS */
#define GS_VIEW_MAX_DIR 32767
size_t gs_view_gain_lds_bytes(const int* box);
int gs_view_gain(const unsigned char* state, int n0, int n1, int n2, const int* origins, int n_views, const int* dirs,
                 int n_rays, int range2, int max_unknown, const int* box, unsigned int* gain, gs_stream_t stream);

/* ---- Range scans on a 2-D occupancy map and the exhaustive correlative scan match (no counterpart in the reference),
 *      csrc/scan.hip; tests/scan_restatement.py restates it serially ----
 *
 * A map is cells u8 [n_u,n_v], n_u and n_v in [1, 1024], a map_server PGM's values read conservatively: 254 is free, 205
 * is unknown, every other value is occupied.  A position is a cell (u, v), the cell's centre; the linear index of a cell
 * is u * n_v + v.  Everything is integer.  All three entries return GS_ERR_INVALID_ARG for a size or a range outside what
 * is stated here, a flag that is neither 0 nor 1 or a NULL pointer, before anything is launched or written; they enqueue
 * on the stream and read nothing back.
 *
 * gs_scan_cast: a virtual range scanner, one ray per (pose, beam).  poses i32 [P,2] in cells, P >= 0 (P == 0 launches
 *   nothing); dirs i32 [P,B,2], 1 <= B <= 4096, P * B <= 2^28, every component in [-GS_VIEW_MAX_DIR, GS_VIEW_MAX_DIR];
 *   range2 in [1, 2 * 1023^2], the squared range in cells; stop_unknown 0 or 1.
 *   The walk of one ray is the view-gain walk above on two axes: origin o, direction d, s_a = sign(d_a), w_a = |d_a|, one
 *   step counter k_a per axis from 0.  The ray visits o first.  The next cell lies one step along s_a on the axis a with
 *   w_a != 0 that minimises (2 k_a + 1) / (2 w_a), compared exactly: axis 1 beats axis 0 when
 *   (2 k_1 + 1) * w_0 < (2 k_0 + 1) * w_1, a tie goes to axis 0 (both products stay below 2^31).  The ray ends, without
 *   visiting that cell, when it lies outside the map or at a squared distance from o above range2; else k_a goes up by
 *   one and the cell is visited.  A visited occupied cell ends the ray as a hit (kind 1); a visited unknown cell ends it
 *   with kind 2 when stop_unknown is set and is passed through otherwise.  An occupied origin is a hit at range 0.  A
 *   pose outside the map, an all-zero direction and a direction with a component out of range cast nothing (kind 0).
 *   kind u8 [P,B]: 0 no return, 1 hit, 2 stopped at unknown.  hit i32 [P,B]: the linear index of the cell that ended the
 *   ray (kind 1 or 2), else -1.  range_mc i32 [P,B]: floor(1000 * sqrt(du^2 + dv^2)) of that cell's offset (du, dv) from
 *   the origin, in milli-cells, else -1.  Every element is written.
 * gs_scan_field: the likelihood field of a map, cost u8 [n_u,n_v] = min(d2, cap), cap = R * R + 1, 1 <= R <= 15 (cap <=
 *   226), d2 the exact squared cell distance to the nearest occupied cell of the map (unknown cells are no sites; a map
 *   without an occupied cell is all cap).  Two separable band-limited passes, out[i] = min over |k| <= R of in[i + k] +
 *   k * k, first along v from 0 at a site and cap elsewhere, then along u, each kept at min(., cap); a site further than
 *   R cells along either axis is beyond the cap, so the result is exact.  Every element is written; no atomics.
 * gs_scan_match: cost and cells [n_u,n_v] as above; offsets i32 [Y,B,2], 1 <= Y <= 1024, 1 <= B <= 4096: per yaw
 *   hypothesis the cell offset (du, dv) of every beam's end point from the robot's cell; the translation window u0 <= u <
 *   u0 + w_u, v0 <= v < v0 + w_v inside the map, w_u, w_v >= 1, Y * w_u * w_v <= 2^28; cap in [1, 226]; allow_unknown 0
 *   or 1.  score u32 [Y,w_u,w_v], every element written: 0xffffffff when the robot's cell (u, v) is not free (with
 *   allow_unknown an unknown cell counts as free), else the sum over the beams of cost[u + du, v + dv], where an end
 *   point outside the map costs cap and an offset with a component outside [-32768, 32767] counts as outside the map.
 *   best u64 [1]: the call resets it to all ones on the stream; it ends as the minimum, over the candidates whose score
 *   is not 0xffffffff, of (score << 32) | linear index, linear index (y * w_u + i) * w_v + j for (y, u0 + i, v0 + j) --
 *   reduced per wave, then by one 64-bit integer atomic min.  A minimum has no order: ties go to the lowest index and
 *   every run gives the same bits.  All ones: no candidate may stand anywhere.                                          */
int gs_scan_cast(const unsigned char* cells, int n_u, int n_v, const int* poses, int n_poses, const int* dirs, int n_beams,
                 int range2, int stop_unknown, unsigned char* kind, int* hit, int* range_mc, gs_stream_t stream);
int gs_scan_field(const unsigned char* cells, int n_u, int n_v, int R, unsigned char* cost, gs_stream_t stream);
int gs_scan_match(const unsigned char* cost, const unsigned char* cells, int n_u, int n_v, const int* offsets, int n_yaws,
                  int n_beams, int u0, int v0, int w_u, int w_v, int cap, int allow_unknown, unsigned int* score,
                  unsigned long long* best, gs_stream_t stream);

/* ---- Monte Carlo localisation on a 2-D occupancy map: particles moved by odometry, weighed against a range scan on the
 *      likelihood field of gs_scan_field, resampled (no counterpart in the reference), csrc/mcl.hip;
 *      tests/mcl_restatement.py restates it serially ----
 *
 * The map is the scan block's: cells and cost u8 [n_u,n_v], n_u and n_v in [1, 1024], 254 free, 205 unknown, anything else
 * occupied.  Everything is integer.  particles i32 [N,3], 0 <= N <= GS_MCL_MAX_PARTICLES (N == 0 launches nothing), one
 * row (x, y, h) per particle -- interleaved, because the weigh kernel gives a wave to a particle and reads the row as three
 * consecutive scalars: x, y in milli-cells, 0 <= x < 1000 n_u, 0 <= y < 1000 n_v, the particle's cell is (x / 1000,
 * y / 1000); h a heading index in [0, H), 1 <= H <= 1024, for the yaw 2 pi h / H (yaw 0 along +u, positive toward +v).
 * rot i32 [H,2]: rint(2^14 (cos, sin)(2 pi h / H)), every |component| <= 2^14.  All four entries return
 * GS_ERR_INVALID_ARG for a size or a value outside what is stated here, a flag that is neither 0 nor 1, a NULL pointer, a
 * 64-bit array that is not 8-byte aligned or outputs that alias inputs where that is refused, before anything is launched
 * or written; they enqueue on the stream and read nothing back.
 *
 * gs_mcl_move: the odometry step (df, dl, dh) -- forward and left in milli-cells, heading steps, each |.| <= 2^20 -- plus
 *   the particle's own noise i32 [N,3] (each |.| <= 2^20).  With f = df + n0, l = dl + n1, (c, s) = rot[h] of the old
 *   heading, in i64 (|f c| <= 2^21 * 2^14: far inside):
 *     x' = clamp(x + ((f c - l s + 8192) >> 14), 0, 1000 n_u - 1),  y' = clamp(y + ((f s + l c + 8192) >> 14), 0, 1000 n_v - 1)
 *     h' = (h + dh + n2) mod H, non-negative;  >> is the arithmetic shift (floor).
 *   out i32 [N,3] may be the particles themselves; any other overlap is refused.  An h outside [0, H) (outside the
 *   contract) is wrapped into it for the table read.
 * gs_mcl_weigh: ends i32 [H,B,2], 1 <= B <= 4096, 8-byte aligned: per heading the end point (ex, ey) of every beam in
 *   milli-cells from the robot; cap in [1, 226]; allow_unknown 0 or 1.  S u32 [N], every element written: 0xffffffff when
 *   the particle's cell is not free (with allow_unknown an unknown cell counts as free; so does a particle outside the
 *   map or with h outside [0, H)), else the sum over the beams of cost[floor((x + ex) / 1000), floor((y + ey) / 1000)] --
 *   the floor of a negative sum goes down, not toward zero --, where an end point outside the map or with |ex| or |ey| >
 *   4 000 000 costs cap.  S <= 4096 * 226 < 2^20.  best u64 [1]: the call resets it to all ones on the stream; it ends as
 *   the minimum over the standing particles of (S << 32) | p, all ones when none stands -- reduced per workgroup, then by
 *   one 64-bit integer atomic min.  A minimum has no order: ties go to the lowest p and every run gives the same bits.
 * gs_mcl_estimate: S as above, lut u32 [L], 1 <= L <= 65536, every entry <= 2^20.  With S_min the smallest S that is not
 *   0xffffffff: w u32 [N] = lut[S - S_min] where the particle stands and S - S_min < L, else 0; cum u64 [N] the inclusive
 *   prefix sum of w; stats u64 [GS_MCL_STATS]:
 *     0 W = sum w    1 sum w^2    2 the particles standing    3 those with w > 0    4 the key `best` of gs_mcl_weigh
 *     5 sum w x      6 sum w y    7 sum w c    8 sum w s  (c, s) = rot[h], two's complement i64
 *     9, 10 sum w (x^2 >> 20), sum w (x^2 & 0xfffff)    11, 12 the same of y^2    13, 14 the same of x y    15 zero
 *   so that sum w x^2 = (stats[9] << 20) + stats[10] exactly.  Bounds: w <= 2^20, N <= 2^16, x, y < 1 024 000 < 2^20,
 *   |c|, |s| <= 2^14: W <= 2^36; sum w^2, sum w x, sum w y < 2^56; |sum w c| <= 2^50; x^2 < 2^40, so both of its parts
 *   are below 2^20 and each of the six sums is below 2^56: every word stays below 2^57.  Integer sums have no order:
 *   every run gives the same bits.  One workgroup.  N == 0 writes nothing.
 * gs_mcl_resample: systematic resampling.  cum u64 [N] as above with W = cum[N - 1] in [1, 2^36] and 0 <= q < W given by
 *   the host (W == 0 is refused).  New particle j is a copy of the old particle i, the smallest i with cum[i] * N >
 *   j * W + q (both sides below 2^52); i = N - 1 when a cum that does not end in W leaves none.  out i32 [N,3] must share
 *   no byte with the particles.                                                                                        */
#define GS_MCL_MAX_PARTICLES 65536
#define GS_MCL_STATS 16
int gs_mcl_move(const int* particles, int n, const int* rot, int n_headings, const int* noise, int df, int dl, int dh,
                int n_u, int n_v, int* out, gs_stream_t stream);
int gs_mcl_weigh(const unsigned char* cost, const unsigned char* cells, int n_u, int n_v, const int* particles, int n,
                 const int* ends, int n_headings, int n_beams, int cap, int allow_unknown, unsigned int* S,
                 unsigned long long* best, gs_stream_t stream);
int gs_mcl_estimate(const unsigned int* S, const int* particles, int n, const int* rot, int n_headings,
                    const unsigned int* lut, int n_lut, unsigned int* w, unsigned long long* cum,
                    unsigned long long* stats, gs_stream_t stream);
int gs_mcl_resample(const unsigned long long* cum, const int* particles, int n, unsigned long long W, unsigned long long q,
                    int* out, gs_stream_t stream);

/* ---- frame preprocessing of the dataset readers (src/datasets.py:96-143, 565-605), csrc/frame_prep.hip ----
 *
 * Semantics: tests/frame_prep_restatement.py, bit for bit (cv2.remap / cv2.resize INTER_LINEAR on 8-bit data,
 * F.interpolate nearest on depth).  Every view is resized to the full frame (H_out + 2 H_edge) x (W_out + 2 W_edge) and
 * only the window [H_edge, H_edge + H_out) x [W_edge, W_edge + W_out) is computed.
 *
 * gs_frame_prep_color: n views, each its own size.  src uint8 [h,w,c] (c = 1: grey, written to all three planes; c = 3:
 *   RGB, plane k from channel k: the decoder's RGB is the reference's BGR image reversed).  With map_x / map_y f32
 *   [mh,mw] (both or neither) the view is first remapped (BORDER_CONSTANT 0) into tmp uint8 [mh,mw,c], which is then
 *   resized.  dst f32 [3,H_out,W_out] = level / 255.0f.
 *   src and tmp start 4-byte aligned; rows need not.  One launch per GS_FRAME_PREP_MAX_VIEWS views, plus one remap
 *   launch per such chunk that holds a mapped view.  h, w, mh, mw in [1, 16384], w * c and mw * c at most 16384.
 * gs_frame_prep_depth: src uint16 [h,w] (4-byte aligned) -> dst f32 [H_out,W_out] = float(level) / scale, nearest
 *   resize.  One launch per GS_FRAME_PREP_MAX_VIEWS views; w at most 8192.                                          */
#define GS_FRAME_PREP_MAX_VIEWS 32
typedef struct {
  const uint8_t* src;
  const float* map_x;    /* NULL: no remap */
  const float* map_y;
  uint8_t* tmp;          /* [mh,mw,c] when mapped */
  float* dst;
  int h, w, c, mh, mw;
} gs_color_view;
typedef struct {
  const uint16_t* src;
  float* dst;
  int h, w;
} gs_depth_view;
int gs_frame_prep_color(const gs_color_view* views_host, int n, int H_out, int W_out, int H_edge, int W_edge,
                        gs_stream_t stream);
int gs_frame_prep_depth(const gs_depth_view* views_host, int n, float scale, int H_out, int W_out, int H_edge,
                        int W_edge, gs_stream_t stream);

/* ------------------------------------------- update-operator gate fusions ---- */

/* ConvGRU gates of src/modules/gru.py:20-33 around MIOpen's convolutions; all NHWC fp16.
 * gs_gru_gate_zr: zr_pre f16 [n,hw,256] = fused convz|convr output WITHOUT bias, bias_zr f32 [256],
 *   glo_zr f32 [n,256] (the 1x1 global-context terms), hx f16 [n,hw,ldx] whose first 128 channels
 *   hold `net` on entry and r*net on exit, z_out f16 [n,hw,128].
 * gs_gru_gate_q : q_pre f16 [n,hw,128] (convq output without bias), bias_q f32 [128], glo_q f32
 *   [n,128], z / net f16 [n,hw,128] -> net_out = (1-z)*net + z*tanh(q_pre + bias + glo).
 * inp_pre (may be NULL): f16 [n,hw,384] = the z | r | q convolutions restricted to the context
 *   features `inp`, which are constant while an edge lives; by linearity they are hoisted out of the
 *   update loop and added to the pre-activations here (zr_pre / q_pre then cover net, corr, flow).  */
int gs_gru_gate_zr(const void* zr_pre, const float* bias_zr, const float* glo_zr, const void* inp_pre, void* hx,
                   void* z_out, int n, int hw, int ldx, gs_stream_t stream);
int gs_gru_gate_q(const void* q_pre, const float* bias_q, const float* glo_q, const void* inp_pre, const void* z,
                  const void* net, void* net_out, int n, int hw, gs_stream_t stream);
/* y[row, 0:channels] = act(x[row, 0:channels] + bias) for NHWC fp16 data viewed as [rows, channels]
 * (channels % 8 == 0); x / y rows are x_stride / y_stride elements apart, so y may be x itself (in
 * place) and either side may be a channel slice of a wider NHWC tensor (replaces torch.cat / split).  bias may be
 * NULL (plain strided copy when act == 0).  act: 0 none, 1 ReLU (a NaN stays a NaN, as torch.relu), 2 sigmoid.
 * fp32 arithmetic, one rounding to fp16: y = half(act(float(x) + bias)).
 * Epilogue of the bias-free MIOpen convolutions of src/droid_net.py:69-140.                       */
int gs_bias_act(const void* x, const float* bias, void* y, int rows, int channels, int x_stride, int y_stride,
                int act, gs_stream_t stream);
/* FactorGraph.update glue (src/factor_graph.py:201-207): out [n,h,w,4] fp16 (NHWC; logical [n,4,h,w]) =
 * clamp([coords1 - pixel grid, target - coords1], -64, 64), coords1 / target f32 [n,h,w,2].            */
int gs_motion_features(const float* coords1, const float* target, void* out, int n, int h, int w,
                       gs_stream_t stream);
/* The per-chunk glue of FactorGraph.update_lowmem (src/factor_graph.py:283-312), one launch each instead of ~11 torch
 * launches per chunk of 13 source keyframes:
 *   gs_lowmem_gather: rows sel[r] (i64 [n_sel], edge indices) of coords1 / target f32 [E,h,w,2] and net f16 [E,h,w,128]
 *     (NHWC) -> coords_out f32 [n_sel,h,w,2] (= coords1[:, v]), motion_out f16 [n_sel,h,w,4] (= clamp([coords1 - grid,
 *     target - coords1], +-64): gs_motion_features of the chunk), net_out f16 [n_sel,h,w,128] (= self.net[:, v]).
 *   gs_lowmem_scatter: target[sel[r]] = coords + delta, weight_all[sel[r]] = weight (all f32 [.,h,w,2]),
 *     net[sel[r]] = net_new (f16 NHWC) -- the three masked assignments of :308-310.  sel must not repeat an index.     */
int gs_lowmem_gather(const float* coords1, const float* target, const void* net, const int64_t* sel,
                     float* coords_out, void* motion_out, void* net_out, int n_sel, int h, int w, gs_stream_t stream);
int gs_lowmem_scatter(const float* coords, const float* delta, const float* weight, const void* net_new,
                      const int64_t* sel, float* target, float* weight_all, void* net, int n_sel, int h, int w,
                      gs_stream_t stream);

/* FactorGraph.update glue (src/factor_graph.py:222-223,244-247): target [n,h,w,2] = coords1 + delta, plus
 * the [n,2,h,w] copies of target and weight that droid_backends.ba takes (ba_target / ba_weight point at
 * the first of these n edges inside the caller's [E_all,2,h,w] buffers).  All f32.                    */
int gs_ba_inputs(const float* coords1, const float* delta, const float* weight, float* target,
                 float* ba_target, float* ba_weight, int n, int h, int w, gs_stream_t stream);
/* 1x1 convolution + bias + activation as one memory-bound MFMA GEMM: y[p, 0:n_out] = act(W x[p, 0:k_in] + b)
 * over `rows` NHWC fp16 pixels (corr_encoder[0] 196->128 ReLU, src/droid_net.py:75; GraphAgg upmask
 * 128->576, src/droid_net.py:45).  x / y rows are x_stride / y_stride elements apart.  k_in % 4 == 0,
 * k_in <= 208; n_out % 32 == 0.  wpack: fp16 [n_out/32][KS][64][8] A-fragments with KS = 8 (k_in <= 128)
 * or 13, wpack[nb][ks][l][e] = W[32 nb + (l & 31)][16 ks + 8 (l >> 5) + e] (0 for k >= k_in).
 * bias may be NULL; act: 0 none, 1 ReLU.                                                            */
int gs_conv1x1(const void* x, int x_stride, int k_in, const void* wpack, const float* bias, int act, void* y,
               int y_stride, int n_out, long long rows, gs_stream_t stream);
/* act(conv7x7(x) + bias), padding 3, stride 1, for a FOUR-channel NHWC fp16 map [n,h,w,4] -> 128 channels (pixels of
 * y `ys` halves apart, 128 written): the flow encoder's first layer over the motion features (reference
 * src/droid_net.py:79 `Conv2d(4, 128, 7, padding=3)` + ReLU).  fp32 accumulation starting from the bias, one rounding to
 * fp16, then ReLU if `relu`.  K is laid out as 7 kernel rows x 8 taps x 4 channels (the 8th tap is zero) = 14 MFMA
 * k-steps; wpack: fp16 [2][2][14][64][8],
 * wpack[nh][t][s][l][e] = Wk[64 nh + 32 t + (l & 31)][16 s + 8 (l >> 5) + e] with Wk[o][32 ky + 4 kx + c] = W[o][c][ky][kx]
 * (0 for kx = 7).  rt = image rows per workgroup (0: chosen from the map size); w <= 1024.              */
int gs_conv7x7_c4(const void* x, const void* wpack, const float* bias, void* y, int ys, int n, int h, int w, int relu,
                  int rt, gs_stream_t stream);
/* 3x3 convolution, padding 1, stride 1, no bias: NHWC fp16 [n,h,w,c_in] (pixels x_stride elements apart) ->
 * NHWC fp16 [n,h,w,n_out] (y_stride apart), fp32 accumulation, as an implicit GEMM on MFMA.  Covers the large
 * convolutions of the update operator: ConvGRU convz|convr and convq (src/modules/gru.py:10-12), the first layers of
 * the delta / weight / agg heads (src/droid_net.py:83,88,40), corr_encoder[2] and flow_encoder[2] (:76,:80).
 * Row-stacked tiling: the n images are tiled as one image of n*h rows, tiles of 512 / tw rows x tw columns (tw in
 * {8, 16}: pick the width that divides w best, 40 -> 8, 80 -> 16) run across image boundaries and the vertical taps
 * are masked per pixel at y == 0 / y == h-1, so no tile padding is spent on h; the images must be contiguous (image
 * stride = h * w * x_stride resp. y_stride).  512-thread workgroups whose two wave groups alternate a fragment-read
 * phase and an MFMA phase one phase apart ("ping-pong"), all staging by LDS-DMA (global_load_lds) with counted waits
 * across raw barriers, an XOR-swizzled bank-conflict-free patch layout.  xcd_order != 0: workgroup ids are decoded so
 * that the output-channel blocks of a tile run on one XCD (shared L2).
 * n_out % 64 == 0 (BN = 128 output channels per workgroup, or 64 when n_out is only a multiple of 64), c_in % 32 == 0.
 * wpack: fp16 [n_out/BN][c_in/32][9][4][BN][8],
 * wpack[nb][ck][3 ky + kx][kg][r][e] = W[BN nb + r][32 ck + 8 kg + e][ky][kx] (gs_conv3x3_wpack_elems halves). */
size_t gs_conv3x3_wpack_elems(int c_in, int n_out);
int gs_conv3x3_pp(const void* x, int x_stride, int c_in, const void* wpack, int tw, void* y, int y_stride, int n_out,
                  int n, int h, int w, int xcd_order, gs_stream_t stream);
/* ConvGRU (src/modules/gru.py:20-33) with the gate arithmetic fused into the 3x3 convolutions' epilogues
 * (results equal gs_conv3x3_pp + gs_gru_gate_zr / gs_gru_gate_q to one fp16 ulp on < 1e-4 of the elements; the 256 + 128
 * channels of pre-activations never travel to HBM and back).
 *   gs_conv3x3_gru_zr: hx [n,h,w,hx_stride] fp16, first c_in channels = [net(128) | rest]; wpack = gs_conv3x3_pp image of
 *     the fused convz|convr weight [256, c_in, 3, 3]; bias_zr f32 [256]; glo_zr f32 [n,256]; inp_pre fp16
 *     [n,h,w,384] or NULL.  Writes z_out = sigmoid(.) [n,h,w,128] and rnet_out = r * net [n,h,w,128]; hx is not modified.
 *   gs_conv3x3_gru_q: input [rnet (128 ch, dense) | x_rest (c_rest channels, pixels x_rest_stride apart)]; wpack = image
 *     of convq [128, 128 + c_rest, 3, 3] (c_rest % 32 == 0); writes net_out = (1 - z) net + z tanh(.).   */
/* gs_conv3x3_pp + bias + ReLU in one kernel; y / y_stride may address a channel slice of a wider NHWC tensor
 * (corr_encoder[2] / flow_encoder[2] -> the GRU input buffer, src/droid_net.py:76,80; agg.conv2, :41).             */
int gs_conv3x3_bias_relu(const void* x, int x_stride, int c_in, const void* wpack, const float* bias, void* y,
                         int y_stride, int n_out, int n, int h, int w, gs_stream_t stream);
/* gs_conv3x3_gru_zr2: the same with the input given as [net (128 channels, dense rows) | x_rest (c_rest channels, pixels
 * x_rest_stride apart)] -- no copy of net into the input buffer before the step (as gs_conv3x3_gru_q).          */
int gs_conv3x3_gru_zr2(const void* net, const void* x_rest, int x_rest_stride, int c_rest, const void* wpack,
                       const float* bias_zr, const float* glo_zr, const void* inp_pre, void* z_out, void* rnet_out,
                       int n, int h, int w, gs_stream_t stream);
int gs_conv3x3_gru_zr(const void* hx, int hx_stride, int c_in, const void* wpack, const float* bias_zr,
                      const float* glo_zr, const void* inp_pre, void* z_out, void* rnet_out, int n, int h, int w,
                      gs_stream_t stream);
int gs_conv3x3_gru_q(const void* rnet, const void* x_rest, int x_rest_stride, int c_rest, const void* wpack,
                     const float* bias_q, const float* glo_q, const void* inp_pre, const void* z, const void* net,
                     void* net_out, int n, int h, int w, gs_stream_t stream);
/* 3x3 convolution (padding 1) from 128 channels to n_out in {1,2} channels, NHWC fp16 in, fp32 out
 * [n,h,w,n_out]: the flow-revision / confidence heads delta[2], weight[2] (src/droid_net.py:83-92) and
 * GraphAgg's eta[0] (src/droid_net.py:43).  x rows are x_stride elements apart (a channel slice of a
 * wider tensor is fine).  If in_bias != NULL or in_relu, the operand is relu?(x + in_bias) applied on
 * the fly (the producer convolution's epilogue).  wpack: fp16 [8][64][8] MFMA A-fragments,
 * wpack[ks][l][e] = W[o][16 ks + 8 (l>>5) + e][ky][kx] with (l & 31) = (3 ky + kx) n_out + o (0 beyond
 * 9 n_out).  out = out_scale * epi(half(conv + bias)); epilogue: 0 none, 1 sigmoid (rounded to fp16),
 * 2 softplus (fp32).                                                                              */
int gs_conv3x3_head(const void* x, int x_stride, const float* in_bias, int in_relu, const void* wpack,
                    const float* bias, int n_out, int epilogue, float out_scale, float* out, int n, int h, int w,
                    gs_stream_t stream);
/* The merged head convolution delta[0] | weight[0] | agg.conv1 (src/droid_net.py:83,88,40) with the 128 -> 2 heads that
 * read its first blocks finished in its epilogue: gs_conv3x3_pp's kernel, arguments and weight image; the first
 * n_tap_blocks 128-channel blocks are never written as fp16 -- each pixel's relu(pre + in_bias) (fp16) is multiplied with
 * that block's head weights (tap_wpack: [n_tap_blocks] gs_conv3x3_head images, fp16 [8][64][8] each; in_bias f32
 * [128 n_tap_blocks]) in gs_conv3x3_head's operand arithmetic and accumulation order, and the 18 products go to
 * tap_out f32 [n_tap_blocks][n*h*w][18], column (3 ky + kx) 2 + o.  The remaining n_out / 128 - n_tap_blocks blocks are
 * stored without bias as gs_conv3x3_pp does, into y [n*h*w, y_stride] from channel 0 (y may be NULL when there are none).
 * gs_conv3x3_heads_finish: out_k[n,h,w,2] = out_scale_k * epi_k(half(sum over the 9 in-image taps of
 * tap[k][neighbour][tap column] + bias_k)) for the two heads k = 0, 1 -- gs_conv3x3_head's gather and epilogue, so the
 * pair equals gs_conv3x3_pp + 2 x gs_conv3x3_head(in_bias, in_relu = 1) bit for bit.                              */
int gs_conv3x3_heads(const void* x, int x_stride, int c_in, const void* wpack, int tw, const void* tap_wpack,
                     const float* in_bias, int n_tap_blocks, float* tap_out, void* y, int y_stride, int n_out, int n,
                     int h, int w, gs_stream_t stream);
int gs_conv3x3_heads_finish(const float* tap, const float* bias0, const float* bias1, int epilogue0, int epilogue1,
                            float out_scale0, float out_scale1, float* out0, float* out1, int n, int h, int w,
                            gs_stream_t stream);
/* GraphAgg's scatter_mean over source keyframes (src/droid_net.py:57-60, torch_scatter):
 * out[s, p, :] = mean over k in [seg_offsets[s], seg_offsets[s+1]) of act(x[seg_edges[k], p, :]), NHWC
 * fp16 [*, hw, channels] (channels % 8 == 0, x rows x_stride elements apart), fp32 accumulation.
 * act = relu?(. + in_bias) rounded to fp16 when in_bias != NULL or in_relu (the producer
 * convolution's epilogue applied on the fly), identity otherwise; the ReLU keeps a NaN (torch.relu).  The fp32 sum
 * runs over the segment's edges in seg_edges order, is multiplied by fp32(1 / count) and rounded once to fp16.
 * seg_edges need not be sorted, may name an edge in several segments and may leave edges unused.  An empty
 * segment (seg_offsets[s] == seg_offsets[s+1]) is written as zeros.                                  */
int gs_segment_mean(const void* x, int x_stride, const float* in_bias, int in_relu, const int* seg_offsets,
                    const int* seg_edges, void* out, int n_seg, int hw, int channels, gs_stream_t stream);
/* Frame encoders (src/modules/extractor.py:27-57 ResidualBlock.forward, :113-126 BasicEncoder.forward): the
 * elementwise tail of every convolution of `fnet` (norm_fn='instance') / `cnet` (norm_fn='none') in three launches
 * (one without the norm) instead of torch's batch_norm_collect_statistics + calc_invstd + transform_input + clamp
 * + add + clamp (and the bias add of the convolution before them).  x, skip, y: NHWC fp16 [n, hw, channels], y may
 * alias x or skip; bias: fp16 [channels] or NULL.
 *   x = bias ? half(x + bias_c) : x                           the convolution's bias, added to its fp16 output
 *   t = instance_norm ? half((x - mean_c) * invstd_c) : x     InstanceNorm2d(affine=False): per image and channel,
 *                                                             biased variance, fp32 statistics, eps inside the sqrt
 *   t = relu_in  ? max(t, 0) : t
 *   t = skip     ? half(skip + t) : t
 *   y = relu_out ? max(t, 0) : t
 * workspace: gs_norm_act_workspace_bytes bytes (not needed when instance_norm == 0).  stat_chunks > 0: the statistics pass
 * is skipped -- gs_enc_conv, given the same workspace as `stats_ws`, already wrote stat_chunks = gs_enc_conv_stat_chunks
 * (h_out, w_out, c_out) moment slabs per image in its epilogue (workspace: gs_norm_act_workspace_bytes_chunks).    */
size_t gs_norm_act_workspace_bytes(int n, int hw, int channels);
size_t gs_norm_act_workspace_bytes_chunks(int n, int chunks, int channels);
/* The frame encoders' convolutions (src/modules/extractor.py:61-126: BasicEncoder.conv1 7x7 / stride 2, the residual
 * blocks' 3x3 convolutions with stride 1 / 2, their strided 1x1 skips, conv2 1x1), NHWC fp16 -> NHWC fp16 with fp32
 * accumulation and ONE fp16 rounding (+ a second one after the fp16 bias add when `bias` f16 [c_out] is given -- the
 * rounding points of a library convolution followed by its bias kernel).  Built shapes (ksize, c_in, c_out, stride):
 * (7,4,32,2) -- the stem on a dense 4-channel RGB0 image --, (3,32,32,1), (3,32,64,2), (3,64,64,1), (3,64,128,2),
 * (3,128,128,1), (1,32,64,2), (1,64,128,2), (1,128,128,1), (1,128,256,1); padding = ksize / 2; anything else returns
 * GS_ERR_UNSUPPORTED.  wpack: MFMA A-fragments in lane order, f16 [ksize^2][c_in/16][c_out/32][64][8] with element
 * [t][s][m][l][e] = W[32 m + (l & 31)][16 s + 8 (l >> 5) + e][t / ksize][t % ksize]; the stem: [7][2][64][8] with
 * [dy][s][l][e] = W[l & 31][e % 4][dy][4 s + 2 (l >> 5) + e / 4] (0 for channel 3 and tap 7).
 * stats_ws (optional): the gs_norm_act workspace of the InstanceNorm that follows -- the epilogue leaves per workgroup
 * and channel the count, mean and M2 (sums shifted by each wave's first pixel) of v = half(half(conv) + stat_bias)
 * (stat_bias f16 [c_out], optional) there, and
 * gs_norm_act is then called with the SAME bias and stat_chunks = gs_enc_conv_stat_chunks(h_out, w_out, c_out).     */
size_t gs_enc_conv_wpack_elems(int ksize, int c_in, int c_out);
int gs_enc_conv_stat_chunks(int h_out, int w_out, int c_out);
int gs_enc_conv(const void* x, int x_stride, int c_in, const void* wpack, const void* bias, void* y, int y_stride,
                int c_out, int ksize, int stride, int n, int h, int w, const void* stat_bias, void* stats_ws,
                gs_stream_t stream);
int gs_norm_act(const void* x, const void* bias, const void* skip, void* y, int n, int hw, int channels,
                int instance_norm, int relu_in, int relu_out, float eps, void* workspace, size_t workspace_bytes,
                int stat_chunks, gs_stream_t stream);
/* ConvGRU global context (src/modules/gru.py:22-27): glo = mean_hw(sigmoid(w_pre + w_bias) * net),
 * then the three 1x1 convolutions convz_glo | convr_glo (-> gzr [n,256]) and convq_glo (-> gq [n,128]).
 * w_pre = bias-free 1x1 conv of net, NHWC fp16 [n,hw,128]; wz/wr/wq fp16 [128 out,128 in]; outputs f32
 * holding fp16-rounded values (what autocast produces).  Rounding points: g = half(sigmoid(half(w_pre + w_bias))),
 * t = half(g * net), fp32 sum of t over the pixels (fixed order: deterministic) times fp32(1 / hw) rounded to fp16, then
 * per head half(b + sum_k W[o][k] glo[k]) with fp32 accumulation starting from the bias.              */
size_t gs_gru_glo_workspace_bytes(int n);
int gs_gru_glo(const void* w_pre, const float* w_bias, const void* net, const void* wz, const void* wr,
               const void* wq, const float* bz, const float* br, const float* bq, float* gzr, float* gq,
               int n, int hw, void* workspace, size_t workspace_bytes, gs_stream_t stream);

/* The same with the 1x1 convolution w(net) inside (MFMA; gru.py:22 `self.w`): w_pre never exists in memory, net is
 * read once.  net: NHWC fp16 [n,hw,*] with pixels net_stride halves apart (first 128 channels used); w_pack = gs_conv1x1's
 * weight image of w ([4][8][64][8] halves); the pre-activation is rounded once, fp16(conv + w_bias).  Deterministic.  */
size_t gs_gru_glo_fused_workspace_bytes(int n, int hw);
int gs_gru_glo_fused(const void* net, int net_stride, const void* w_pack, const float* w_bias, const void* wz,
                     const void* wr, const void* wq, const float* bz, const float* br, const float* bq, float* gzr,
                     float* gq, int n, int hw, void* workspace, size_t workspace_bytes, gs_stream_t stream);

/* FactorGraph.update's damping rows (src/factor_graph.py:228,244): damping_buf[index[k]] = eta[inv[k]] where
 * inv[k] >= 0, then out[k] = scale * damping_buf[index[k]] + eps, rows of hw floats; eta [*,hw] (may be NULL when no
 * inv[k] >= 0), inv int32 [n_rows], index int64 [n_rows] (distinct frames), out [n_rows,hw].                  */
int gs_damping_rows(const float* eta, const int* inv, const int64_t* index, float* damping_buf, float* out,
                    int n_rows, int hw, float scale, float eps, gs_stream_t stream);

/* DepthVideo.upsample -> cvx_upsample (src/depth_video.py:194-196, src/droid_net.py:9-23):
 * out[ix[n]] (f32 [*,8h,8w]) = convex 8x upsampling of disps[ix[n]] (f32 [*,h,w]) with the softmax
 * of mask f16 [m,576,h,w] (logical NCHW; mask_channels_last != 0: NHWC strides).  ix i64 [m] or
 * NULL (identity).                                                                            */
int gs_cvx_upsample(const float* disps, const void* mask, const int64_t* ix, float* out,
                    int m, int h, int w, int mask_channels_last, gs_stream_t stream);
/* GraphAgg's upmask convolution (Conv2d(128, 576, 1), src/droid_net.py:45,62) fused with the convex upsampling above:
 * x fp16 [m*h*w, x_stride] (NHWC agg features, first 128 channels), weight fp16 [576][128], bias f32 [576];
 * out[ix[n]] = cvx_upsample(disps[ix[n]], half(W x + b)).  The 576-channel mask is never materialised.              */
int gs_upmask_upsample(const void* x, int x_stride, const void* weight, const float* bias, const float* disps,
                       const int64_t* ix, float* out, int m, int h, int w, gs_stream_t stream);

/* ------------------------------------------------------ dense bundle adjustment ---- */

/* Workspace size for gs_ba (bytes).  n_edges = len(ii), n_poses = t1-t0, n_depth = rows of
 * eta (= |unique(cat(arange(t0,t1), ii))|; pass an upper bound when unknown), nbuf = poses
 * rows, hw = h*w.                                                                           */
size_t gs_ba_workspace_bytes(int n_edges, int n_poses, int n_depth, int nbuf, int hw);

/* droid_backends.ba (droid.cpp:88-117, droid_kernels.cu:1314-1434 incl. the host-side
 * SparseBlock / schur_block / Eigen LLT of :1117-1311, all on the device here).
 *   poses f32 [nbuf,7] (in/out), disps f32 [nbuf,h,w] (in/out), intrinsics f32 [4],
 *   disps_sens f32 [nbuf,h,w], targets/weights f32 [n_edges,2,h,w], eta f32 [n_depth,h,w]
 *   (ignored when motion_only), ii/jj i64 [n_edges];
 *   dx f32 [t1-t0,6] and dz f32 [n_depth,h*w] receive the last iteration's update.
 * A Cholesky failure leaves dx = 0 for that iteration as the reference does (:1202-1210).
 * status_out (optional, device int32[4]): [0] = #depth keyframes found, [1] = 1 if it
 * differs from n_depth, [2] = #Cholesky failures, [3] reserved.                             */
int gs_ba(float* poses, float* disps, const float* intrinsics, const float* disps_sens,
          const float* targets, const float* weights, const float* eta,
          const int64_t* ii, const int64_t* jj,
          int t0, int t1, int iterations, float lm, float ep, int motion_only,
          int n_edges, int n_depth, int nbuf, int h, int w,
          float* dx, float* dz, int32_t* status_out,
          void* workspace, size_t workspace_bytes, gs_stream_t stream);

/* gs_ba with flags.  GS_BA_REUSE_TABLES (1): `workspace` still holds the index tables (unique keyframes, CSR of
 * out-edges, Schur entry lists) an earlier call built for the SAME ii / jj / t0 / t1 / n_depth / nbuf / map size and
 * nothing has written to it since -- they depend on nothing else, so the one-workgroup table kernel (26 us, once per
 * call) is skipped.  FactorGraph.update issues 6 calls per keyframe on one edge set.                       */
#define GS_BA_REUSE_TABLES 1
int gs_ba_ex(float* poses, float* disps, const float* intrinsics, const float* disps_sens,
             const float* targets, const float* weights, const float* eta,
             const int64_t* ii, const int64_t* jj,
             int t0, int t1, int iterations, float lm, float ep, int motion_only,
             int n_edges, int n_depth, int nbuf, int h, int w,
             float* dx, float* dz, int32_t* status_out,
             void* workspace, size_t workspace_bytes, int flags, gs_stream_t stream);

/* The damped fp64 Cholesky solve of gs_ba's reduced camera system on its own (Eigen SimplicialLLT, droid_kernels.cu:
 * 1192-1213): x = (A + diag(ep + lm * diag(A)))^-1 b, dx = float(x); a pivot <= 0 gives dx = 0 (a NaN pivot does not).
 *   H f64 [n,n] row-major, only its LOWER triangle is read; b f64 [n].  Both are device buffers and both may be
 *     overwritten (the mid and blocked paths work in place; the blocked path leaves L in H's lower triangle and uses
 *     b for y = L^-1 b and the backward substitution's partial sums); dx f32 [n].
 *   path: 0 = gs_ba's own choice by n, 1 = the one-workgroup LDS path (n <= 192, n % 6 == 0), 2 = the one-workgroup
 *     path with global head stages (n % 6 == 0, n <= 300), 3 = the blocked multi-launch path (any n >= 1).  A forced
 *     path whose limits n does not meet is refused with GS_ERR_UNSUPPORTED before anything is enqueued.
 *   status: device int32[4]; [0] = 1 if this solve failed, else 0; [1] += 1 per failed solve; [2..3] reserved.      */
int gs_chol_solve(double* H, double* b, int n, float lm, float ep, int path, float* dx, int32_t* status,
                  gs_stream_t stream);

/* Edge proposal with greedy non-maximum suppression on the device: FactorGraph.add_proximity_factors
 * (src/factor_graph.py:384-450) and Backend.ba's selection incl. the loop-closure rule (src/backend.py:31-94), in two
 * launches around a device-side stable sort; the frame-distance matrix never leaves HBM.
 *   raw f32 [(t-i0) x (t-j0)]: frame distances of keyframe pairs (i0 + row, j0 + col).
 *   gs_edge_prep: d_work = raw with the non-candidates (i - rad < j, raw > cut) at +inf, +inf in the (2 nms + 1)^2
 *     windows of the existing edges ex_i / ex_j (i64, n_existing; pairs outside the window are ignored) and of the
 *     local-window edges (i, j), (j, i) for j in [max(i - rad, jmin), i) -- which are written to es (i64 [cap,2], with
 *     (i, i) first per keyframe if `stereo`) in the reference's order; count[0] = number of edges written.
 *   (the caller sorts d_work ascending, stable: sorted_vals f32, order i64)
 *   gs_edge_greedy: visits the candidates with sorted value <= thresh in order; a candidate that an earlier pick has
 *     not suppressed appends (i, j), (j, i) -- in `loop` mode instead the members (si != sj) of its 3x3 neighbourhood
 *     with raw <= thresh, and only if more than 4 of the 9 are -- and suppresses its window; stops as soon as
 *     count > max_factors.  count[0] is updated.  At most 512 x 512 candidate pairs.                       */
int gs_edge_prep(const float* raw, float* d_work, const long long* ex_i, const long long* ex_j, int n_existing,
                 long long* es, int* count, int cap, int i0, int j0, int t, int rad, int nms, float cut, int stereo,
                 int jmin, gs_stream_t stream);
int gs_edge_greedy(const float* raw, const float* sorted_vals, const long long* order, long long* es, int* count,
                   int cap, int i0, int j0, int t, int nms, float thresh, int max_factors, int loop, gs_stream_t stream);

/* End-of-run trajectory evaluation on the device, fp64 (src/slam.py:313-365).  Every reduction below has one fixed
 * order -- frame 256 b + t belongs to thread t of block b, an LDS tree (stride 128 .. 1) inside the block, then one
 * block that adds the block results b = t, t + 256, ... in ascending order and runs the same tree -- and uses no
 * float atomics: two runs give identical bits.  workspace: gs_traj_eval_workspace_bytes(n) for both reductions.
 *
 * gs_traj_world (replaces src/slam.py:315-318, `SE3(pose_compensate) * traj.inv()`, `.data` and `.matrix()`):
 *   w2c f32 [n,7] world-to-camera (t, q), compensate f32 [7]; tq f64 [n,7] = compensate * inv(w2c) as (t, q) and
 *   mat f64 [n,4,4] the same pose as a camera-to-world matrix (rotation = the quaternion's action on the basis, not
 *   normalised, as lietorch's matrix()).  fp32 inputs are widened first; one thread per frame.
 *
 * gs_ape_moments (replaces the sums inside evo's umeyama_alignment, reached from src/slam.py:359-360):
 *   est, ref f64 [n,3]; mask u8 [n] (NULL = every frame), a frame with mask 0 is never read.  moments f64 [17]:
 *   [0] valid count, [1..3] mean of est, [4..6] mean of ref, [7..15] the 3x3 cross-covariance
 *   sum (ref - mean_ref)(est - mean_est)^T / count row-major with ref along the rows, [16] the variance of est
 *   sum |est - mean_est|^2 / count.  Two passes: the means, then the centred sums.  count == 0 gives zeros.
 *
 * gs_ape_stats (replaces evo's APE translation part and its statistics, src/slam.py:359-364):
 *   sim f64 [12] on the device: c R row-major [9] then t [3].  err f64 [n]: |ref - (cR est + t)| per frame, -1 for a
 *   frame outside the mask.  stats f64 [7] = rmse, mean, median, min, max, sse, std (population) over the valid
 *   frames.  The median is taken by rank counting (rank = #{j: e_j < e_i or e_j == e_i and j < i}): the frames of
 *   rank (count - 1) / 2 and count / 2 are averaged.  count == 0 gives NaN statistics (sse 0).                 */
size_t gs_traj_eval_workspace_bytes(int n);
int gs_traj_world(const float* w2c, const float* compensate, int n, double* tq, double* mat, gs_stream_t stream);
int gs_ape_moments(const double* est, const double* ref, const unsigned char* mask, int n, double* moments,
                   void* workspace, size_t workspace_bytes, gs_stream_t stream);
int gs_ape_stats(const double* est, const double* ref, const unsigned char* mask, const double* sim, int n,
                 double* err, double* stats, void* workspace, size_t workspace_bytes, gs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GOSLAM_HIP_H */
