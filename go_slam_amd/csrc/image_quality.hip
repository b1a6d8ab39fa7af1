// Quality of a rendered frame against the input frame (no counterpart in the reference, whose image_visualization.py
// stops at a per-frame MAE / PSNR over the pixels with depth): colour MSE and PSNR over the whole image, SSIM after
// Wang et al. 2004 (11 x 11 Gaussian window, sigma 1.5, valid windows only, per channel) and the depth L1 over the
// pixels with a measurement.  Contract: include/goslam_neus.h (gs_image_quality); tests/image_quality_restatement.py
// restates it on the CPU by direct 121-tap sums.
//
// iq_tile_kernel: one 256-thread workgroup per tile of GS_IQ_TILE_H x GS_IQ_TILE_W (16 x 32) window positions, all three
// channels.  The tile and its 10-pixel apron, 26 x 42 pixels of both images, are fetched from global memory once as
// interleaved fp32 rows (126 consecutive floats per row) into LDS, zeros outside the image.  Per channel the separable
// filter runs in fp64: the horizontal pass turns 26 x 42 staged values into the five moments x, y, x^2, y^2, xy at
// 26 x 32 positions (lanes 3 floats apart: no bank conflict), the vertical pass reads those (lanes 8 B apart) and
// finishes 16 x 32 windows, two per thread.  The colour error comes from the same staged values: a tile owns the pixels
// of its 16 x 32 corner, the last tile of a row or column also its apron, so every pixel is owned once.  The depth pair
// is read straight from global memory for the owned pixels.
//   LDS 59 616 B: 2 x 26 x 126 fp32 staged + 5 x 26 x 32 fp64 moments + 4 x 4 fp64 wave sums: two workgroups per CU,
//   two waves per SIMD.  As compiled for gfx950: iq_tile_kernel 128 VGPRs (the 11 taps unrolled, which that occupancy
//   leaves room for), iq_final_kernel 36 VGPRs, no scratch.
//
// Reductions, no float atomics: a thread adds its own terms in program order, the 64 lanes of a wave meet in an xor
// butterfly (32, 16, ... 1), lane 0 of each wave leaves its sum in LDS and thread 0 adds the four in wave order: one
// fp64 partial per sum and workgroup.  iq_final_kernel, one workgroup: thread t adds the partials t, t + 256, ... in
// ascending order, then the same butterfly and wave order.  Two runs give identical bits; a NaN input reaches every sum
// it is a term of.  Compiled with -ffp-contract=off, and the fp64 arithmetic is written with the rounded intrinsics.
#include "common.h"
#include "../../include/goslam_neus.h"

#include <math.h>

namespace {

constexpr int IQ_THREADS = 256;
constexpr int IQ_TH = GS_IQ_TILE_H, IQ_TW = GS_IQ_TILE_W;
constexpr int IQ_TAPS = 11, IQ_APRON = IQ_TAPS - 1;
constexpr int IQ_SH = IQ_TH + IQ_APRON, IQ_SW = IQ_TW + IQ_APRON;     // staged pixels: 26 x 42
constexpr int IQ_ROW = IQ_SW * 3;                                     // staged floats per row, channels interleaved
constexpr int IQ_NV = 4;                                              // sum d^2 | sum s | sum |dz| | depth count
constexpr double IQ_C1 = 0.01 * 0.01, IQ_C2 = 0.03 * 0.03;

struct IqWindow { double g[IQ_TAPS]; };      // by-value kernel argument (SGPRs)

// -> red[a] (a < IQ_NV) on thread 0; every thread must call
__device__ __forceinline__ void iq_block_sum(double (&v)[IQ_NV], double (*wsum)[IQ_NV]) {
#pragma unroll
  for (int a = 0; a < IQ_NV; ++a)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[a] = __dadd_rn(v[a], __shfl_xor(v[a], off, 64));
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < IQ_NV; ++a) wsum[threadIdx.x >> 6][a] = v[a];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int a = 0; a < IQ_NV; ++a)
      v[a] = __dadd_rn(__dadd_rn(__dadd_rn(wsum[0][a], wsum[1][a]), wsum[2][a]), wsum[3][a]);
}

__global__ __launch_bounds__(IQ_THREADS) void iq_tile_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                             const float* __restrict__ pred_depth,
                                                             const float* __restrict__ gt_depth, int H, int W,
                                                             IqWindow win, double* __restrict__ part) {
  __shared__ float sx[IQ_SH][IQ_ROW];
  __shared__ float sy[IQ_SH][IQ_ROW];
  __shared__ double hm[5][IQ_SH][IQ_TW];
  __shared__ double wsum[IQ_THREADS / 64][IQ_NV];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * IQ_TW, y0 = blockIdx.y * IQ_TH;
  const int row_floats = 3 * W;

  // stage: rows y0 .. y0 + 25, floats 3 x0 .. 3 x0 + 125 of each, zeros past the image
  for (int i = t; i < IQ_SH * IQ_ROW; i += IQ_THREADS) {
    const int r = i / IQ_ROW, e = i - r * IQ_ROW;
    const int gy = y0 + r, ge = 3 * x0 + e;
    float a = 0.0f, b = 0.0f;
    if (gy < H && ge < row_floats) {
      const size_t at = (size_t)gy * row_floats + ge;
      a = pred[at];
      b = gt[at];
    }
    sx[r][e] = a;
    sy[r][e] = b;
  }
  __syncthreads();

  double v[IQ_NV] = {0.0, 0.0, 0.0, 0.0};
  // the pixels this tile owns: its corner, and in the last tile of a row / column everything up to the image's edge
  const int own_h = (int)blockIdx.y == (int)gridDim.y - 1 ? H - y0 : IQ_TH;
  const int own_w = (int)blockIdx.x == (int)gridDim.x - 1 ? W - x0 : IQ_TW;
  const int own_floats = 3 * own_w;
  for (int i = t; i < own_h * own_floats; i += IQ_THREADS) {
    const int r = i / own_floats, e = i - r * own_floats;
    const double d = __dsub_rn((double)sx[r][e], (double)sy[r][e]);
    v[0] = __dadd_rn(v[0], __dmul_rn(d, d));
  }
  if (gt_depth) {
    for (int i = t; i < own_h * own_w; i += IQ_THREADS) {
      const int r = i / own_w, c = i - r * own_w;
      const size_t at = (size_t)(y0 + r) * W + (x0 + c);
      const float g = gt_depth[at];
      if (g > 0.0f) {
        v[2] = __dadd_rn(v[2], fabs(__dsub_rn((double)pred_depth[at], (double)g)));
        v[3] = __dadd_rn(v[3], 1.0);
      }
    }
  }

  const int wins_y = H - IQ_APRON, wins_x = W - IQ_APRON;             // valid window positions of the image
  for (int ch = 0; ch < 3; ++ch) {
    // horizontal pass: moments at staged row r, window column c
    for (int i = t; i < IQ_SH * IQ_TW; i += IQ_THREADS) {
      const int r = i / IQ_TW, c = i - r * IQ_TW;
      double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
      for (int k = 0; k < IQ_TAPS; ++k) {
        const double x = (double)sx[r][3 * (c + k) + ch], y = (double)sy[r][3 * (c + k) + ch];
        const double g = win.g[k];
        m0 = __dadd_rn(m0, __dmul_rn(g, x));
        m1 = __dadd_rn(m1, __dmul_rn(g, y));
        m2 = __dadd_rn(m2, __dmul_rn(g, __dmul_rn(x, x)));
        m3 = __dadd_rn(m3, __dmul_rn(g, __dmul_rn(y, y)));
        m4 = __dadd_rn(m4, __dmul_rn(g, __dmul_rn(x, y)));
      }
      hm[0][r][c] = m0;
      hm[1][r][c] = m1;
      hm[2][r][c] = m2;
      hm[3][r][c] = m3;
      hm[4][r][c] = m4;
    }
    __syncthreads();
    // vertical pass and the index of one window
    for (int i = t; i < IQ_TH * IQ_TW; i += IQ_THREADS) {
      const int r = i / IQ_TW, c = i - r * IQ_TW;
      if (y0 + r >= wins_y || x0 + c >= wins_x) continue;
      double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < IQ_TAPS; ++k) {
        const double g = win.g[k];
#pragma unroll
        for (int a = 0; a < 5; ++a) m[a] = __dadd_rn(m[a], __dmul_rn(g, hm[a][r + k][c]));
      }
      const double mxx = __dmul_rn(m[0], m[0]), myy = __dmul_rn(m[1], m[1]), mxy = __dmul_rn(m[0], m[1]);
      const double vx = __dsub_rn(m[2], mxx), vy = __dsub_rn(m[3], myy), cov = __dsub_rn(m[4], mxy);
      const double num = __dmul_rn(__dadd_rn(__dadd_rn(mxy, mxy), IQ_C1), __dadd_rn(__dadd_rn(cov, cov), IQ_C2));
      const double den = __dmul_rn(__dadd_rn(__dadd_rn(mxx, myy), IQ_C1), __dadd_rn(__dadd_rn(vx, vy), IQ_C2));
      v[1] = __dadd_rn(v[1], __ddiv_rn(num, den));
    }
    __syncthreads();                         // hm is rewritten for the next channel
  }

  iq_block_sum(v, wsum);
  if (t == 0) {
    const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    for (int a = 0; a < IQ_NV; ++a) part[b * IQ_NV + a] = v[a];
  }
}

// out = mse, psnr, ssim, depth_l1, n_depth, n_windows, 0, 0
__global__ __launch_bounds__(IQ_THREADS) void iq_final_kernel(const double* __restrict__ part, int nblk, int H, int W,
                                                              double* __restrict__ out) {
  __shared__ double wsum[IQ_THREADS / 64][IQ_NV];
  double v[IQ_NV] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += IQ_THREADS)
    for (int a = 0; a < IQ_NV; ++a) v[a] = __dadd_rn(v[a], part[(size_t)b * IQ_NV + a]);
  iq_block_sum(v, wsum);
  if (threadIdx.x != 0) return;
  const double n_values = 3.0 * (double)H * (double)W;
  const double n_windows = 3.0 * (double)(H - IQ_APRON) * (double)(W - IQ_APRON);
  const double mse = __ddiv_rn(v[0], n_values);
  out[0] = mse;
  out[1] = __dmul_rn(-10.0, log10(mse));     // +inf at mse == 0
  out[2] = __ddiv_rn(v[1], n_windows);
  out[3] = v[3] > 0.0 ? __ddiv_rn(v[2], v[3]) : __builtin_nan("");
  out[4] = v[3];
  out[5] = n_windows;
  out[6] = 0.0;
  out[7] = 0.0;
}

bool iq_tiles(int H, int W, int* tx, int* ty) {
  if (H < IQ_TAPS || W < IQ_TAPS) return false;
  *tx = gs_cdiv(W - IQ_APRON, IQ_TW);
  *ty = gs_cdiv(H - IQ_APRON, IQ_TH);
  return true;
}

// g_k = exp(-(k - 5)^2 / 4.5) / sum, the sum taken in ascending k; mirrored, so exactly symmetric
IqWindow iq_window() {
  IqWindow w;
  double e[IQ_TAPS], s = 0.0;
  for (int k = 0; k <= IQ_APRON / 2; ++k) e[k] = e[IQ_APRON - k] = exp(-(double)((k - 5) * (k - 5)) / 4.5);
  for (int k = 0; k < IQ_TAPS; ++k) s += e[k];
  for (int k = 0; k < IQ_TAPS; ++k) w.g[k] = e[k] / s;
  return w;
}

}  // namespace

extern "C" int gs_image_quality_tile(int* tile_h, int* tile_w) {
  GS_REQUIRE(tile_h && tile_w, "image_quality_tile: null pointer");
  *tile_h = IQ_TH;
  *tile_w = IQ_TW;
  return GS_OK;
}

extern "C" size_t gs_image_quality_workspace_bytes(int H, int W) {
  int tx, ty;
  if (!iq_tiles(H, W, &tx, &ty)) return 0;
  return (size_t)tx * ty * IQ_NV * sizeof(double);
}

extern "C" int gs_image_quality(const float* pred_rgb, const float* gt_rgb, const float* pred_depth,
                                const float* gt_depth, int H, int W, double* out, void* workspace,
                                size_t workspace_bytes, gs_stream_t stream) {
  int tx, ty;
  GS_REQUIRE(iq_tiles(H, W, &tx, &ty), "image_quality: %d x %d is smaller than the 11 x 11 window", H, W);
  GS_REQUIRE(pred_rgb && gt_rgb && out && workspace, "image_quality: null pointer");
  GS_REQUIRE((pred_depth == nullptr) == (gt_depth == nullptr), "image_quality: the depth pair is both or neither");
  GS_REQUIRE(ty <= 65535 && W <= (1 << 24), "image_quality: %d x %d is too large", H, W);
  if (workspace_bytes < gs_image_quality_workspace_bytes(H, W)) {
    gs_set_error("image_quality: workspace %zu < %zu bytes", workspace_bytes, gs_image_quality_workspace_bytes(H, W));
    return GS_ERR_WORKSPACE;
  }
  static const IqWindow win = iq_window();
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  GS_TIMING_PRE();
  iq_tile_kernel<<<dim3(tx, ty), IQ_THREADS, 0, st>>>(pred_rgb, gt_rgb, pred_depth, gt_depth, H, W, win, part);
  GS_CHECK_LAUNCH("image_quality_tiles");
  iq_final_kernel<<<1, IQ_THREADS, 0, st>>>(part, tx * ty, H, W, out);
  GS_CHECK_LAUNCH("image_quality_final");
  return GS_OK;
}
