// TSDF fusion of keyframe depth on a dense lattice (no counterpart in the reference: surfaces without the mapper).
// Contract: include/goslam_hip.h (gs_tsdf_*); tests/tsdf_restatement.py restates it serially.
//
// tsdf_integrate_kernel is the sweep of tsdf_common.h (tsdf_fuse) with MeanRule: a point's state is tsdf, weight and
// with images the three colours, each a running mean over the observations in frame order.
// Compiled with -ffp-contract=off.
#include "tsdf_common.h"

namespace {

struct MeanRule {
  float* tsdf;
  float* weight;
  float* colors;           // planar [3,npoints]; touched only by the COLOR kernel
  float max_weight;
  struct State { float t, w0, cr, cg, cb; };

  __device__ __forceinline__ void load(State& p, size_t at, size_t npoints, bool color) const {
    p.t = tsdf[at];
    p.w0 = weight[at];
    p.cr = p.cg = p.cb = 0.0f;
    if (color) {
      p.cr = colors[at];
      p.cg = colors[npoints + at];
      p.cb = colors[2 * npoints + at];
    }
  }
  __device__ __forceinline__ void fold(State& p, int, float s, const float* img, size_t hw) const {
    const float w1 = p.w0 + 1.0f;
    p.t = (p.t * p.w0 + s) / w1;
    if (img) {
      p.cr = (p.cr * p.w0 + img[0]) / w1;
      p.cg = (p.cg * p.w0 + img[hw]) / w1;
      p.cb = (p.cb * p.w0 + img[2 * hw]) / w1;
    }
    p.w0 = fminf(w1, max_weight);
  }
  __device__ __forceinline__ void store(const State& p, size_t at, size_t npoints, bool color) const {
    tsdf[at] = p.t;
    weight[at] = p.w0;
    if (color) {
      colors[at] = p.cr;
      colors[npoints + at] = p.cg;
      colors[2 * npoints + at] = p.cb;
    }
  }
};

template <bool COLOR>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(MeanRule rule, TsdfSweep sw) {
  tsdf_fuse<COLOR>(rule, sw);
}

// One lane per vertex.  A vertex lies on a lattice edge: at most one coordinate is fractional.
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_vertex_attr_kernel(
    const float* __restrict__ verts, int nv, const float* __restrict__ weight, const float* __restrict__ colors,
    int nx, int ny, int nz, float min_weight, unsigned char* __restrict__ keep, float* __restrict__ rgb) {
  const int v = blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (v >= nv) return;
  const int n[3] = {nx, ny, nz};
  int a[3], b[3];
  float t = 0.0f;
  bool found = false;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float c = verts[(size_t)v * 3 + d];
    const float fl = floorf(c);
    // clamped into the lattice (NaN -> 0): a vertex of marching cubes is inside, this only bounds the loads
    a[d] = (fl >= 0.0f) ? ((fl < (float)(n[d] - 1)) ? (int)fl : n[d] - 1) : 0;
    b[d] = a[d];
    const float fr = c - fl;
    if (!found && fr > 0.0f) {
      found = true;
      t = fr;
      b[d] = min(a[d] + 1, n[d] - 1);
    }
  }
  const size_t np = (size_t)nx * ny * nz;
  const size_t ia = ((size_t)a[0] * ny + a[1]) * nz + a[2];
  const size_t ib = ((size_t)b[0] * ny + b[1]) * nz + b[2];
  keep[v] = (weight[ia] >= min_weight && weight[ib] >= min_weight) ? 1 : 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float ca = colors[c * np + ia], cb = colors[c * np + ib];
    rgb[(size_t)v * 3 + c] = ca + t * (cb - ca);
  }
}

}  // namespace

extern "C" int gs_tsdf_batch(void) { return GS_TSDF_BATCH; }

extern "C" int gs_tsdf_integrate(float* tsdf, float* weight, float* colors, int nx, int ny, int nz, const float* depth,
                                 const float* mask, const float* images, const float* w2c, int k, int h, int w,
                                 float fx, float fy, float cx, float cy, float lo_x, float lo_y, float lo_z,
                                 float voxel, float trunc, float max_weight, gs_stream_t stream) {
  GS_REQUIRE(tsdf && weight && depth && w2c, "tsdf_integrate: null pointer");
  GS_REQUIRE(!images || colors, "tsdf_integrate: images without a colour lattice");
  GS_REQUIRE(fx > 0.0f && fy > 0.0f && voxel > 0.0f && trunc > 0.0f && max_weight >= 1.0f,
             "tsdf_integrate: fx=%g fy=%g voxel=%g trunc=%g max_weight=%g", fx, fy, voxel, trunc, max_weight);
  return tsdf_fuse_enqueue("tsdf_integrate", tsdf_integrate_kernel<true>, tsdf_integrate_kernel<false>, nx, ny, nz,
                           depth, mask, images, w2c, k, h, w, fx, fy, cx, cy, lo_x, lo_y, lo_z, voxel, trunc, stream,
                           [=](int) { return MeanRule{tsdf, weight, colors, max_weight}; });
}

extern "C" int gs_tsdf_vertex_attr(const float* vertices, int n_vertices, const float* weight, const float* colors,
                                   int nx, int ny, int nz, float min_weight, unsigned char* keep, float* rgb,
                                   gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_vertex_attr: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(n_vertices >= 0, "tsdf_vertex_attr: n_vertices=%d", n_vertices);
  if (n_vertices == 0) return GS_OK;
  GS_REQUIRE(vertices && weight && colors && keep && rgb, "tsdf_vertex_attr: null pointer");
  GS_TIMING_PRE();
  tsdf_vertex_attr_kernel<<<gs_cdiv(n_vertices, TSDF_THREADS), TSDF_THREADS, 0, (hipStream_t)stream>>>(
      vertices, n_vertices, weight, colors, nx, ny, nz, min_weight, keep, rgb);
  GS_CHECK_LAUNCH("tsdf_vertex_attr");
  return GS_OK;
}
