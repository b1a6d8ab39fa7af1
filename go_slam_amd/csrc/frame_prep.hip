// Frame preprocessing of the dataset readers (src/datasets.py:96-143, 565-605): cv2.remap and cv2.resize INTER_LINEAR
// on 8-bit frames, planar RGB, / 255, the edge crop; depth / png_depth_scale and F.interpolate(mode='nearest').  The
// semantics are tests/frame_prep_restatement.py's, bit for bit; contract in include/goslam_hip.h.
//
// Resize and depth: a workgroup owns one output row of one view (grid = (H_out, views)).  The one or two source rows
// it needs are staged into LDS with coalesced dword loads (rows need not start dword-aligned: the load starts at the
// aligned dword below and the row begins `lead` bytes into the copy), then each lane computes output pixels of the
// cropped window from LDS and writes the three float planes, coalesced.  The remap is a launch of its own, one lane
// per mapped pixel, into a uint8 intermediate: its four taps are gathers wherever the maps point.  Compiled with
// -ffp-contract=off: the tap positions are computed in double and float exactly as cv::resize computes them.
#include "common.h"

namespace {

constexpr int FP_THREADS = 256;
constexpr int FP_MAX_BYTES = 16384;                     // longest staged row: w * c (colour), 2 * w (depth)
constexpr int FP_ONE = 2048;                            // INTER_RESIZE_COEF_SCALE

struct FpColorItem {
  const uint8_t* src;
  float* dst;
  int h, w, c, pad;
};
struct FpColorArgs {
  FpColorItem it[GS_FRAME_PREP_MAX_VIEWS];
  int H_out, W_out, H_edge, W_edge, row_dw;
};
struct FpRemapItem {
  const uint8_t* src;
  const float* map_x;
  const float* map_y;
  uint8_t* tmp;
  int h, w, c, mh, mw, pad;
};
struct FpRemapArgs {
  FpRemapItem it[GS_FRAME_PREP_MAX_VIEWS];
};
struct FpDepthItem {
  const uint16_t* src;
  float* dst;
  int h, w;
};
struct FpDepthArgs {
  FpDepthItem it[GS_FRAME_PREP_MAX_VIEWS];
  int H_out, W_out, H_edge, W_edge, row_dw;
  float scale;
};

// Bytes [off, off + n) of a buffer of `total` bytes (base dword-aligned) into lds; returns where the row starts in the
// copy.  The one dword that would cross the end of the buffer is assembled from bytes.
__device__ __forceinline__ int fp_stage(const uint8_t* __restrict__ base, size_t total, size_t off, int n,
                                        uint32_t* __restrict__ lds) {
  const size_t a = off & ~(size_t)3;
  const int lead = (int)(off - a);
  const int nd = (lead + n + 3) >> 2;
  for (int i = threadIdx.x; i < nd; i += FP_THREADS) {
    const size_t p = a + 4 * (size_t)i;
    uint32_t v = 0;
    if (p + 4 <= total) {
      v = *(const uint32_t*)(base + p);
    } else {
      for (int k = 0; k < 4; ++k)
        if (p + k < total) v |= (uint32_t)base[p + k] << (8 * k);
    }
    lds[i] = v;
  }
  return lead;
}

// One axis of cv::resize's INTER_LINEAR table: source index and fraction of destination index d.
__device__ __forceinline__ void fp_tap(int d, double scale, int& s, float& f) {
  f = (float)(((double)d + 0.5) * scale - 0.5);
  const float fl = floorf(f);
  s = (int)fl;
  f = f - fl;
}

__device__ __forceinline__ int fp_weight(float v) { return (int)rintf(v * (float)FP_ONE); }

__device__ __forceinline__ int fp_sat16(int v) { return min(max(v, -32768), 32767); }

// VResizeLinearVec_32s8u: ((S0 >> 4) * b0 >> 16) + ((S1 >> 4) * b1 >> 16), saturated to int16, then (s + 2) >> 2
__device__ __forceinline__ int fp_vresize(int S0, int S1, int b0, int b1) {
  const int t = fp_sat16(((fp_sat16(S0 >> 4) * b0) >> 16) + ((fp_sat16(S1 >> 4) * b1) >> 16));
  return min(max((t + 2) >> 2, 0), 255);
}

__global__ __launch_bounds__(FP_THREADS) void fp_color_kernel(FpColorArgs args) {
  extern __shared__ uint32_t fp_lds[];
  const FpColorItem it = args.it[blockIdx.y];
  const int y = blockIdx.x;
  const int Hf = args.H_out + 2 * args.H_edge, Wf = args.W_out + 2 * args.W_edge;
  const int h = it.h, w = it.w, c = it.c;
  const int dy = y + args.H_edge;
  const bool area = h == 2 * Hf && w == 2 * Wf;
  int r0, r1, b0 = FP_ONE, b1 = 0;
  if (area) {
    r0 = 2 * dy;
    r1 = r0 + 1;
  } else {
    int sy;
    float fy;
    fp_tap(dy, 1.0 / ((double)Hf / (double)h), sy, fy);
    b0 = fp_weight(1.0f - fy);
    b1 = fp_weight(fy);
    r0 = min(max(sy, 0), h - 1);
    r1 = min(max(sy + 1, 0), h - 1);
  }
  const size_t total = (size_t)h * w * c;
  const int wc = w * c;
  uint32_t* lds0 = fp_lds;
  uint32_t* lds1 = fp_lds + args.row_dw;
  const int lead0 = fp_stage(it.src, total, (size_t)r0 * wc, wc, lds0);
  const int lead1 = fp_stage(it.src, total, (size_t)r1 * wc, wc, lds1);
  __syncthreads();
  const uint8_t* row0 = (const uint8_t*)lds0 + lead0;
  const uint8_t* row1 = (const uint8_t*)lds1 + lead1;
  const double scale_x = 1.0 / ((double)Wf / (double)w);
  const size_t plane = (size_t)args.H_out * args.W_out;
  float* out = it.dst + (size_t)y * args.W_out;
  for (int x = threadIdx.x; x < args.W_out; x += FP_THREADS) {
    const int dx = x + args.W_edge;
    int v[3];
    if (area) {
      const int i0 = 2 * dx * c, i1 = i0 + c;
      for (int ch = 0; ch < c; ++ch)
        v[ch] = ((int)row0[i0 + ch] + (int)row0[i1 + ch] + (int)row1[i0 + ch] + (int)row1[i1 + ch] + 2) >> 2;
    } else {
      int sx;
      float fx;
      fp_tap(dx, scale_x, sx, fx);
      if (sx < 0) { fx = 0.0f; sx = 0; }
      if (sx >= w - 1) { fx = 0.0f; sx = w - 1; }
      const int a0 = fp_weight(1.0f - fx), a1 = fp_weight(fx);
      const int i0 = sx * c, i1 = min(sx + 1, w - 1) * c;
      for (int ch = 0; ch < c; ++ch) {
        const int S0 = (int)row0[i0 + ch] * a0 + (int)row0[i1 + ch] * a1;
        const int S1 = (int)row1[i0 + ch] * a0 + (int)row1[i1 + ch] * a1;
        v[ch] = fp_vresize(S0, S1, b0, b1);
      }
    }
    if (c == 1) v[1] = v[2] = v[0];
    // planes in the source's channel order (RGB as decoded), IEEE division as the reference's float32 tensor / 255.0
    out[x] = (float)v[0] / 255.0f;
    out[plane + x] = (float)v[1] / 255.0f;
    out[2 * plane + x] = (float)v[2] / 255.0f;
  }
}

__global__ __launch_bounds__(FP_THREADS) void fp_remap_kernel(FpRemapArgs args) {
  const FpRemapItem it = args.it[blockIdx.y];
  if (it.map_x == nullptr) return;
  const int p = blockIdx.x * FP_THREADS + threadIdx.x;
  if (p >= it.mh * it.mw) return;
  const float mx = fminf(fmaxf(it.map_x[p] * 32.0f, -1073741824.0f), 1073741824.0f);
  const float my = fminf(fmaxf(it.map_y[p] * 32.0f, -1073741824.0f), 1073741824.0f);
  const int ix = (int)rintf(mx), iy = (int)rintf(my);
  const int tx = ix & 31, ty = iy & 31;
  const int sx = min(max(ix >> 5, -32768), 32767), sy = min(max(iy >> 5, -32768), 32767);
  const int w00 = (32 - ty) * (32 - tx) * 32, w01 = (32 - ty) * tx * 32;
  const int w10 = ty * (32 - tx) * 32, w11 = ty * tx * 32;
  const int h = it.h, w = it.w, c = it.c;
  const bool x0 = sx >= 0 && sx < w, x1 = sx + 1 >= 0 && sx + 1 < w;
  const bool y0 = sy >= 0 && sy < h, y1 = sy + 1 >= 0 && sy + 1 < h;
  const uint8_t* s00 = it.src + ((size_t)sy * w + sx) * c;      // dereferenced only where in bounds
  for (int ch = 0; ch < c; ++ch) {
    const int v00 = (y0 && x0) ? s00[ch] : 0;
    const int v01 = (y0 && x1) ? s00[c + ch] : 0;
    const int v10 = (y1 && x0) ? s00[(size_t)w * c + ch] : 0;
    const int v11 = (y1 && x1) ? s00[(size_t)w * c + c + ch] : 0;
    const int acc = v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11;
    it.tmp[(size_t)p * c + ch] = (uint8_t)min(max((acc + (1 << 14)) >> 15, 0), 255);
  }
}

__global__ __launch_bounds__(FP_THREADS) void fp_depth_kernel(FpDepthArgs args) {
  extern __shared__ uint32_t fp_lds[];
  const FpDepthItem it = args.it[blockIdx.y];
  const int y = blockIdx.x;
  const int Hf = args.H_out + 2 * args.H_edge, Wf = args.W_out + 2 * args.W_edge;
  const int h = it.h, w = it.w;
  // torch's nearest_idx: min(floor(d * (float)in / out), in - 1), in float
  const float sh = (float)h / (float)Hf, sw = (float)w / (float)Wf;
  const int sy = min((int)floorf((float)(y + args.H_edge) * sh), h - 1);
  const int lead = fp_stage((const uint8_t*)it.src, (size_t)h * w * 2, (size_t)sy * w * 2, w * 2, fp_lds);
  __syncthreads();
  const uint16_t* row = (const uint16_t*)((const uint8_t*)fp_lds + lead);   // lead is 0 or 2
  float* out = it.dst + (size_t)y * args.W_out;
  for (int x = threadIdx.x; x < args.W_out; x += FP_THREADS) {
    const int sx = min((int)floorf((float)(x + args.W_edge) * sw), w - 1);
    out[x] = (float)row[sx] / args.scale;
  }
}

bool fp_aligned(const void* p) { return ((uintptr_t)p & 3) == 0; }

int fp_check_out(int H_out, int W_out, int H_edge, int W_edge, const char* name) {
  GS_REQUIRE(H_out >= 1 && W_out >= 1 && H_edge >= 0 && W_edge >= 0, "%s: bad output %d x %d, edges %d %d", name, H_out,
             W_out, H_edge, W_edge);
  GS_REQUIRE(H_out + 2 * (long long)H_edge <= FP_MAX_BYTES && W_out + 2 * (long long)W_edge <= FP_MAX_BYTES,
             "%s: output frame larger than %d", name, FP_MAX_BYTES);
  return GS_OK;
}

}  // namespace

extern "C" int gs_frame_prep_color(const gs_color_view* views, int n, int H_out, int W_out, int H_edge, int W_edge,
                                   gs_stream_t stream) {
  GS_REQUIRE(n >= 0 && (n == 0 || views), "frame_prep_color: n=%d", n);
  int rc = fp_check_out(H_out, W_out, H_edge, W_edge, "frame_prep_color");
  if (rc != GS_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const gs_color_view& v = views[i];
    GS_REQUIRE(v.src && v.dst, "frame_prep_color: view %d: null pointer", i);
    GS_REQUIRE(fp_aligned(v.src), "frame_prep_color: view %d: src not 4-byte aligned", i);
    GS_REQUIRE(v.c == 1 || v.c == 3, "frame_prep_color: view %d: %d channels", i, v.c);
    GS_REQUIRE(v.h >= 1 && v.w >= 1 && v.h <= FP_MAX_BYTES && (long long)v.w * v.c <= FP_MAX_BYTES,
               "frame_prep_color: view %d: unsupported size %d x %d x %d", i, v.h, v.w, v.c);
    GS_REQUIRE((v.map_x == nullptr) == (v.map_y == nullptr), "frame_prep_color: view %d: one map only", i);
    if (v.map_x) {
      GS_REQUIRE(v.tmp && fp_aligned(v.tmp), "frame_prep_color: view %d: remap needs a 4-byte aligned tmp", i);
      GS_REQUIRE(v.mh >= 1 && v.mw >= 1 && v.mh <= FP_MAX_BYTES && (long long)v.mw * v.c <= FP_MAX_BYTES,
                 "frame_prep_color: view %d: unsupported map size %d x %d", i, v.mh, v.mw);
    }
  }
  for (int lo = 0; lo < n; lo += GS_FRAME_PREP_MAX_VIEWS) {
    const int m = min(n - lo, GS_FRAME_PREP_MAX_VIEWS);
    FpRemapArgs ra = {};
    FpColorArgs ca = {};
    int remap_px = 0, max_wc = 0;
    for (int k = 0; k < m; ++k) {
      const gs_color_view& v = views[lo + k];
      FpColorItem& ci = ca.it[k];
      ci.dst = v.dst;
      ci.c = v.c;
      if (v.map_x) {
        ra.it[k] = FpRemapItem{v.src, v.map_x, v.map_y, v.tmp, v.h, v.w, v.c, v.mh, v.mw, 0};
        remap_px = max(remap_px, v.mh * v.mw);
        ci.src = v.tmp;
        ci.h = v.mh;
        ci.w = v.mw;
      } else {
        ci.src = v.src;
        ci.h = v.h;
        ci.w = v.w;
      }
      max_wc = max(max_wc, ci.w * ci.c);
    }
    if (remap_px > 0) {
      GS_TIMING_PRE();
      fp_remap_kernel<<<dim3(gs_cdiv(remap_px, FP_THREADS), m), FP_THREADS, 0, (hipStream_t)stream>>>(ra);
      GS_CHECK_LAUNCH("frame_prep_remap");
    }
    ca.H_out = H_out;
    ca.W_out = W_out;
    ca.H_edge = H_edge;
    ca.W_edge = W_edge;
    ca.row_dw = (max_wc + 3) / 4 + 1;
    GS_TIMING_PRE();
    fp_color_kernel<<<dim3(H_out, m), FP_THREADS, 2 * ca.row_dw * sizeof(uint32_t), (hipStream_t)stream>>>(ca);
    GS_CHECK_LAUNCH("frame_prep_color");
  }
  return GS_OK;
}

extern "C" int gs_frame_prep_depth(const gs_depth_view* views, int n, float scale, int H_out, int W_out, int H_edge,
                                   int W_edge, gs_stream_t stream) {
  GS_REQUIRE(n >= 0 && (n == 0 || views), "frame_prep_depth: n=%d", n);
  int rc = fp_check_out(H_out, W_out, H_edge, W_edge, "frame_prep_depth");
  if (rc != GS_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const gs_depth_view& v = views[i];
    GS_REQUIRE(v.src && v.dst, "frame_prep_depth: view %d: null pointer", i);
    GS_REQUIRE(fp_aligned(v.src), "frame_prep_depth: view %d: src not 4-byte aligned", i);
    GS_REQUIRE(v.h >= 1 && v.w >= 1 && v.h <= FP_MAX_BYTES && 2LL * v.w <= FP_MAX_BYTES,
               "frame_prep_depth: view %d: unsupported size %d x %d", i, v.h, v.w);
  }
  for (int lo = 0; lo < n; lo += GS_FRAME_PREP_MAX_VIEWS) {
    const int m = min(n - lo, GS_FRAME_PREP_MAX_VIEWS);
    FpDepthArgs da = {};
    int max_w = 0;
    for (int k = 0; k < m; ++k) {
      const gs_depth_view& v = views[lo + k];
      da.it[k] = FpDepthItem{v.src, v.dst, v.h, v.w};
      max_w = max(max_w, v.w);
    }
    da.H_out = H_out;
    da.W_out = W_out;
    da.H_edge = H_edge;
    da.W_edge = W_edge;
    da.row_dw = (2 * max_w + 3) / 4 + 1;
    da.scale = scale;
    GS_TIMING_PRE();
    fp_depth_kernel<<<dim3(H_out, m), FP_THREADS, da.row_dw * sizeof(uint32_t), (hipStream_t)stream>>>(da);
    GS_CHECK_LAUNCH("frame_prep_depth");
  }
  return GS_OK;
}
