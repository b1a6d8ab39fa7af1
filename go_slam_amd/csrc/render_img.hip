// Renderer.render_img / Visualizer.vis (reference src/render.py:177-236, src/image_visualization.py:32-83): a whole
// frame of the map from one camera pose.
//
//   batch_max_kernel        one workgroup per ray batch: gt_depth.max() of the batch (render.py:121,140), NaN
//                           propagated as torch.max does -- the n^2 re-reads of gs_render_sample's in-launch maximum
//                           (every workgroup reduces its whole batch) become one pass over the image
//   img_sample_kernel       one wave per pixel: the ray from the pose (build_all_rays, nerf_coordinate = False), written
//                           out for the forward, and the batch's sample placement by gs_place_ray_wave (neus_common.h,
//                           the very code of gs_render_sample's wave kernel) with the batch's maximum and perturbation row
//   img_metrics_kernel      camera-frame normals, residual images and fp64 per-workgroup partial sums of the metrics
//   img_metrics_final_kernel   one workgroup: the partials in a fixed order -> MSE, PSNR, MAE, RMSE, S0.01, S0.02
// The forward between sampling and metrics is gs_neus_forward_segmented (neus.hip).
#include "common.h"
#include "neus_common.h"
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void batch_max_kernel(const float* __restrict__ gt, int n, int batch,
                                                        float* __restrict__ out) {
  __shared__ float smax[4];
  __shared__ int snan[4];
  const int b0 = blockIdx.x * batch;
  const int b1 = b0 + batch < n ? b0 + batch : n;
  float m = -INFINITY;
  int isnan_ = 0;
  for (int i = b0 + (int)threadIdx.x; i < b1; i += 256) {
    const float v = gt[i];
    m = fmaxf(m, v);
    isnan_ |= (v != v) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m = fmaxf(m, __shfl_xor(m, o));
    isnan_ |= __shfl_xor(isnan_, o);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { smax[wave] = m; snan[wave] = isnan_; }
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    out[blockIdx.x] = (snan[0] | snan[1] | snan[2] | snan[3]) ? NAN : m;
  }
}

__global__ __launch_bounds__(256) void img_sample_kernel(
    const float* __restrict__ c2w, int H, int W, float fx, float fy, float cx, float cy, const float* __restrict__ gt_depth,
    const float* __restrict__ bound, const float* __restrict__ t_samples, const float* __restrict__ t_surface,
    const float* __restrict__ perturb, int batch, const float* __restrict__ batch_max, float* __restrict__ rays_o,
    float* __restrict__ rays_d, float* __restrict__ z_vals, float* __restrict__ dists, int ns, int nsurf) {
  __shared__ float sa[4][64], sb[4][64], sz[4][128];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = H * W;
  const int r = blockIdx.x * 4 + wave;
  if (r >= n) return;
  // build_all_rays (nerf_func.py:184-221, nerf_coordinate = False): dirs = ((x-cx)/fx, (y-cy)/fy, 1), rays_d = dirs R^T
  typedef const __attribute__((address_space(4))) float* cfp;    // uniform, unchanged during the launch -> s_load
  cfp P = (cfp)(uintptr_t)c2w;
  const int y = r / W, x = r - y * W;
  const float u = ((float)x - cx) / fx, v = ((float)y - cy) / fy;
  float o[3], d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = P[4 * k + 3];
    d[k] = (u * P[4 * k + 0] + v * P[4 * k + 1]) + 1.0f * P[4 * k + 2];
  }
  if (lane < 3) {
    rays_o[(size_t)r * 3 + lane] = o[lane];
    rays_d[(size_t)r * 3 + lane] = d[lane];
  }
  const int b = r / batch;
  const bool has_depth = gt_depth != nullptr;
  const int total = ns + (has_depth ? nsurf : 0);
  gs_place_ray_wave(o, d, bound, has_depth, has_depth ? gt_depth[r] : 0.0f, has_depth ? batch_max[b] : 0.0f, t_samples,
                    t_surface, perturb ? perturb + (size_t)b * ns : nullptr, ns, nsurf, sa[wave], sb[wave], sz[wave],
                    z_vals + (size_t)r * total, dists + (size_t)r * total, lane);
}

// metrics partials: [sum (gt_c - c)^2, sum |gt - d|, sum (gt - d)^2, k, #|sdf| < 0.01, #|sdf| < 0.02]
constexpr int kMetricBlocks = 512;
constexpr int kMetricTerms = 6;

__device__ __forceinline__ void block_sum(double (&v)[kMetricTerms], double (*sh)[256]) {
#pragma unroll
  for (int t = 0; t < kMetricTerms; ++t) sh[t][threadIdx.x] = v[t];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
#pragma unroll
      for (int t = 0; t < kMetricTerms; ++t) sh[t][threadIdx.x] += sh[t][threadIdx.x + h];
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < kMetricTerms; ++t) v[t] = sh[t][0];
}

__global__ __launch_bounds__(256) void img_metrics_kernel(
    const float* __restrict__ color, const float* __restrict__ depth, const float* __restrict__ normal,
    const float* __restrict__ sdf, const float* __restrict__ gt_depth, const float* __restrict__ gt_color,
    const float* __restrict__ c2w, int n, int s, float* __restrict__ normal_cam, float* __restrict__ depth_res,
    float* __restrict__ color_res, double* __restrict__ partial) {
  __shared__ double sh[kMetricTerms][256];
  typedef const __attribute__((address_space(4))) float* cfp;
  cfp P = (cfp)(uintptr_t)c2w;
  double acc[kMetricTerms] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int stride = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float g = gt_depth[i];
    const float de = fabsf(g - depth[i]);
    const bool zero = g < 1e-3f, in = g > 1e-3f;     // (a depth of exactly 1e-3 is in the images, not in the metrics)
    if (depth_res) depth_res[i] = zero ? 0.0f : de;
    float cn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float ce = fabsf(gt_color[(size_t)i * 3 + c] - color[(size_t)i * 3 + c]);
      if (color_res) color_res[(size_t)i * 3 + c] = zero ? 0.0f : ce;
      if (in) acc[0] += (double)ce * (double)ce;
    }
    if (normal_cam) {
      const float nx = normal[(size_t)i * 3 + 0], ny = normal[(size_t)i * 3 + 1], nz = normal[(size_t)i * 3 + 2];
#pragma unroll
      for (int c = 0; c < 3; ++c) cn[c] = (P[c] * nx + P[4 + c] * ny) + P[8 + c] * nz;    // R^T n
#pragma unroll
      for (int c = 0; c < 3; ++c) normal_cam[(size_t)i * 3 + c] = cn[c];
    }
    if (in) {
      acc[1] += (double)de;
      acc[2] += (double)de * (double)de;
      acc[3] += 1.0;
    }
  }
  const long long ns_total = (long long)n * s;
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < ns_total; j += stride) {
    const float a = fabsf(sdf[j]);
    acc[4] += a < 0.01f ? 1.0 : 0.0;
    acc[5] += a < 0.02f ? 1.0 : 0.0;
  }
  block_sum(acc, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int t = 0; t < kMetricTerms; ++t) partial[(size_t)blockIdx.x * kMetricTerms + t] = acc[t];
  }
}

__global__ __launch_bounds__(256) void img_metrics_final_kernel(const double* __restrict__ partial, int blocks, int n,
                                                                int s, double* __restrict__ metrics) {
  __shared__ double sh[kMetricTerms][256];
  double acc[kMetricTerms] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < blocks; b += 256) {
#pragma unroll
    for (int t = 0; t < kMetricTerms; ++t) acc[t] += partial[(size_t)b * kMetricTerms + t];
  }
  block_sum(acc, sh);
  if (threadIdx.x == 0) {
    const double k = acc[3], all = (double)n * (double)s;
    const double mse = acc[0] / (3.0 * k);          // 0 / 0 = NaN for an empty mask, as numpy's mean of nothing
    metrics[0] = mse;
    metrics[1] = -10.0 * log10(mse);
    metrics[2] = acc[1] / k;
    metrics[3] = sqrt(acc[2] / k);
    metrics[4] = acc[4] / all;
    metrics[5] = acc[5] / all;
    metrics[6] = k;
    metrics[7] = all;
  }
}

}  // namespace

extern "C" int gs_render_img_sample(const float* c2w, int H, int W, float fx, float fy, float cx, float cy,
                                    const float* gt_depth, const float* bound, const float* t_samples,
                                    const float* t_surface, const float* perturb, int ray_batch, float* rays_o,
                                    float* rays_d, float* batch_max, float* z_vals, float* dists, int n_samples,
                                    int n_surface, gs_stream_t stream) {
  GS_REQUIRE(c2w && bound && t_samples && rays_o && rays_d && z_vals && dists, "render_img_sample: null pointer");
  GS_REQUIRE(H >= 0 && W >= 0 && (long long)H * W < (1ll << 31) && ray_batch > 0, "render_img_sample: bad shape");
  GS_REQUIRE(n_samples > 0 && n_samples <= 64 && n_surface >= 0 && n_surface <= 64,
             "render_img_sample: n_samples in [1, 64] and n_surface in [0, 64]");
  GS_REQUIRE(!gt_depth || ((n_surface == 0 || t_surface) && batch_max), "render_img_sample: t_surface / batch_max required");
  const int n = H * W;
  if (n == 0) return GS_OK;
  hipStream_t st = (hipStream_t)stream;
  GS_TIMING_PRE();
  if (gt_depth) {
    batch_max_kernel<<<gs_cdiv(n, ray_batch), 256, 0, st>>>(gt_depth, n, ray_batch, batch_max);
    GS_CHECK_LAUNCH("render_img_batch_max");
  }
  img_sample_kernel<<<gs_cdiv(n, 4), 256, 0, st>>>(c2w, H, W, fx, fy, cx, cy, gt_depth, bound, t_samples, t_surface,
                                                   perturb, ray_batch, batch_max, rays_o, rays_d, z_vals, dists, n_samples,
                                                   gt_depth ? n_surface : 0);
  GS_CHECK_LAUNCH("render_img_sample");
  return GS_OK;
}

extern "C" size_t gs_render_img_metrics_workspace_bytes(void) {
  return (size_t)kMetricBlocks * kMetricTerms * sizeof(double) + 256;
}

extern "C" int gs_render_img_metrics(const float* color, const float* depth, const float* normal, const float* sdf,
                                     const float* gt_depth, const float* gt_color, const float* c2w, int n, int s,
                                     float* normal_cam, float* depth_res, float* color_res, double* metrics,
                                     void* workspace, size_t workspace_bytes, gs_stream_t stream) {
  GS_REQUIRE(color && depth && sdf && gt_depth && gt_color && metrics, "render_img_metrics: null pointer");
  GS_REQUIRE(!normal_cam || (normal && c2w), "render_img_metrics: normal_cam needs normal and c2w");
  GS_REQUIRE(n >= 0 && s >= 0, "render_img_metrics: bad shape");
  if (!workspace || workspace_bytes < gs_render_img_metrics_workspace_bytes()) {
    gs_set_error("render_img_metrics: workspace too small (%zu < %zu)", workspace_bytes,
                 gs_render_img_metrics_workspace_bytes());
    return GS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)gs_align((size_t)workspace);
  // a fixed grid: the partials, and so the rounding of every sum, do not depend on anything but n and s
  const long long work = (long long)n * (s > 1 ? s : 1);
  const long long want = (work + 255) / 256;
  const int blocks = want < 1 ? 1 : (want > kMetricBlocks ? kMetricBlocks : (int)want);
  GS_TIMING_PRE();
  img_metrics_kernel<<<blocks, 256, 0, st>>>(color, depth, normal, sdf, gt_depth, gt_color, c2w, n, s, normal_cam,
                                             depth_res, color_res, partial);
  GS_CHECK_LAUNCH("render_img_metrics");
  img_metrics_final_kernel<<<1, 256, 0, st>>>(partial, blocks, n, s, metrics);
  GS_CHECK_LAUNCH("render_img_metrics_final");
  return GS_OK;
}
