// Reversible TSDF fusion: integer sums and counts on the lattice of tsdf.hip, so that a keyframe fused at a pose that
// bundle adjustment later moves can be taken out again bit for bit (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_tsdf_accumulate, gs_tsdf_resolve, gs_tsdf_frame_change);
// tests/tsdf_live_restatement.py restates the three serially.
//
// tsdf_accumulate_kernel is the sweep of tsdf_common.h (tsdf_fuse), the one tsdf_integrate_kernel is, with SumRule: a
// point's state is two i32, with images six.  An observation is quantised once and added with its frame's sign (at a
// wave-uniform address: a scalar load), so the state is a sum over frames that commutes and has an exact inverse.
//
// tsdf_resolve_kernel: one lane per point, the state turned into the fp32 lattices TSDFVolume's consumers read.
// tsdf_frame_change_kernel: one workgroup per frame, fp64 partial sums over the pixels a lane strides over, a butterfly
// within the wave, then the four waves' totals through LDS in wave order: a fixed order, so two runs agree bitwise.
// Compiled with -ffp-contract=off.
#include "tsdf_common.h"

namespace {

struct SumRule {
  int* sum_s;
  int* count;
  int* sum_rgb;            // planar [3,npoints], and count_rgb: touched only by the COLOR kernel
  int* count_rgb;
  const int* sign;         // [nframes] of the batch, +1 or -1
  struct State { int ss, cn, sr, sg, sb, cc; };

  __device__ __forceinline__ void load(State& p, size_t at, size_t npoints, bool color) const {
    p.ss = sum_s[at];
    p.cn = count[at];
    p.sr = p.sg = p.sb = p.cc = 0;
    if (color) {
      p.sr = sum_rgb[at];
      p.sg = sum_rgb[npoints + at];
      p.sb = sum_rgb[2 * npoints + at];
      p.cc = count_rgb[at];
    }
  }
  __device__ __forceinline__ void fold(State& p, int f, float s, const float* img, size_t hw) const {
    const int sn = sign[f];
    p.ss += sn * (int)rintf(s * 16384.0f);
    p.cn += sn;
    if (img) {
      p.sr += sn * (int)rintf(fminf(fmaxf(img[0], 0.0f), 1.0f) * 255.0f);
      p.sg += sn * (int)rintf(fminf(fmaxf(img[hw], 0.0f), 1.0f) * 255.0f);
      p.sb += sn * (int)rintf(fminf(fmaxf(img[2 * hw], 0.0f), 1.0f) * 255.0f);
      p.cc += sn;
    }
  }
  __device__ __forceinline__ void store(const State& p, size_t at, size_t npoints, bool color) const {
    sum_s[at] = p.ss;
    count[at] = p.cn;
    if (color) {
      sum_rgb[at] = p.sr;
      sum_rgb[npoints + at] = p.sg;
      sum_rgb[2 * npoints + at] = p.sb;
      count_rgb[at] = p.cc;
    }
  }
};

template <bool COLOR>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_accumulate_kernel(SumRule rule, TsdfSweep sw) {
  tsdf_fuse<COLOR>(rule, sw);
}

template <bool COLOR>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_resolve_kernel(
    const int* __restrict__ sum_s, const int* __restrict__ count, const int* __restrict__ sum_rgb,
    const int* __restrict__ count_rgb, float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ colors,
    long long npoints) {
  const long long at = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (at >= npoints) return;
  const int cn = count[at];
  weight[at] = (float)max(cn, 0);
  tsdf[at] = cn > 0 ? (float)((double)sum_s[at] / ((double)cn * 16384.0)) : 1.0f;
  if (COLOR) {
    const int cc = count_rgb[at];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t o = (size_t)c * npoints + at;
      colors[o] = cc > 0 ? (float)((double)sum_rgb[o] / ((double)cc * 255.0)) : 0.0f;
    }
  }
}

// c = -R^T t and p = R^T (ref e_z - t) of a [3,4] fp32 matrix, in fp64: column j of R against v, as (a + b) + c
__device__ __forceinline__ void tsdf_pose_points(const float* __restrict__ m, double ref, double* c, double* p) {
  const double t0 = (double)m[3], t1 = (double)m[7], t2 = (double)m[11];
  const double v2 = ref - t2;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double r0 = (double)m[j], r1 = (double)m[4 + j], r2 = (double)m[8 + j];
    c[j] = -((r0 * t0 + r1 * t1) + r2 * t2);
    p[j] = (r0 * (-t0) + r1 * (-t1)) + r2 * v2;
  }
}

__device__ __forceinline__ double tsdf_dist3(const double* a, const double* b) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_frame_change_kernel(
    const float* __restrict__ old_depth, const float* __restrict__ cur_depth, const float* __restrict__ w2c_old,
    const float* __restrict__ w2c_new, int hw, double ref, double* __restrict__ out) {
  __shared__ double part[TSDF_WAVES][2];
  const int f = blockIdx.x;
  const float* __restrict__ a = old_depth + (size_t)f * hw;
  const float* __restrict__ b = cur_depth + (size_t)f * hw;
  double n = 0.0, sum = 0.0;
  for (int p = threadIdx.x; p < hw; p += TSDF_THREADS) {
    const float o = a[p], c = b[p];
    if (o > 0.0f && c > 0.0f) {
      n += 1.0;
      sum += (double)fabsf(c - o);
    }
  }
  n = gs_wave_sum_f64(n);
  sum = gs_wave_sum_f64(sum);
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = n;
    part[threadIdx.x >> 6][1] = sum;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* __restrict__ o = out + (size_t)f * 4;
  o[0] = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0];
  o[1] = ((part[0][1] + part[1][1]) + part[2][1]) + part[3][1];
  double c0[3], p0[3], c1[3], p1[3];
  tsdf_pose_points(w2c_old + f * 12, ref, c0, p0);
  tsdf_pose_points(w2c_new + f * 12, ref, c1, p1);
  o[2] = tsdf_dist3(c1, c0);
  o[3] = tsdf_dist3(p1, p0);
}

}  // namespace

extern "C" int gs_tsdf_accumulate(int* sum_s, int* count, int* sum_rgb, int* count_rgb, int nx, int ny, int nz,
                                  const float* depth, const float* mask, const float* images, const float* w2c,
                                  const int* sign, int k, int h, int w, float fx, float fy, float cx, float cy,
                                  float lo_x, float lo_y, float lo_z, float voxel, float trunc, gs_stream_t stream) {
  GS_REQUIRE(sum_s && count && depth && w2c && sign, "tsdf_accumulate: null pointer");
  GS_REQUIRE(!images || (sum_rgb && count_rgb), "tsdf_accumulate: images without the colour sums and their count");
  GS_REQUIRE(fx > 0.0f && fy > 0.0f && voxel > 0.0f && trunc > 0.0f, "tsdf_accumulate: fx=%g fy=%g voxel=%g trunc=%g",
             fx, fy, voxel, trunc);
  return tsdf_fuse_enqueue("tsdf_accumulate", tsdf_accumulate_kernel<true>, tsdf_accumulate_kernel<false>, nx, ny, nz,
                           depth, mask, images, w2c, k, h, w, fx, fy, cx, cy, lo_x, lo_y, lo_z, voxel, trunc, stream,
                           [=](int f0) { return SumRule{sum_s, count, sum_rgb, count_rgb, sign + f0}; });
}

extern "C" int gs_tsdf_resolve(const int* sum_s, const int* count, const int* sum_rgb, const int* count_rgb, int nx,
                               int ny, int nz, float* tsdf, float* weight, float* colors, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_resolve: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(sum_s && count && tsdf && weight, "tsdf_resolve: null pointer");
  GS_REQUIRE((colors && sum_rgb && count_rgb) || (!colors && !sum_rgb && !count_rgb),
             "tsdf_resolve: colors, sum_rgb and count_rgb go together");
  const long long npoints = (long long)nx * ny * nz;
  const unsigned blocks = (unsigned)((npoints + TSDF_THREADS - 1) / TSDF_THREADS);
  GS_TIMING_PRE();
  if (colors)
    tsdf_resolve_kernel<true><<<blocks, TSDF_THREADS, 0, (hipStream_t)stream>>>(sum_s, count, sum_rgb, count_rgb, tsdf,
                                                                                weight, colors, npoints);
  else
    tsdf_resolve_kernel<false><<<blocks, TSDF_THREADS, 0, (hipStream_t)stream>>>(sum_s, count, nullptr, nullptr, tsdf,
                                                                                 weight, nullptr, npoints);
  GS_CHECK_LAUNCH("tsdf_resolve");
  return GS_OK;
}

extern "C" int gs_tsdf_frame_change(const float* old_depth, const float* cur_depth, const float* w2c_old,
                                    const float* w2c_new, int k, int h, int w, float ref_depth, double* out,
                                    gs_stream_t stream) {
  GS_REQUIRE(k >= 0 && h > 0 && w > 0 && (long long)h * w <= (1LL << 30), "tsdf_frame_change: k=%d h=%d w=%d", k, h, w);
  if (k == 0) return GS_OK;
  GS_REQUIRE(old_depth && cur_depth && w2c_old && w2c_new && out, "tsdf_frame_change: null pointer");
  GS_TIMING_PRE();
  tsdf_frame_change_kernel<<<(unsigned)k, TSDF_THREADS, 0, (hipStream_t)stream>>>(old_depth, cur_depth, w2c_old, w2c_new,
                                                                                 h * w, (double)ref_depth, out);
  GS_CHECK_LAUNCH("tsdf_frame_change");
  return GS_OK;
}
