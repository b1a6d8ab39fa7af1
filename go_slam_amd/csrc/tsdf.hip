// TSDF fusion of keyframe depth on a dense lattice (no counterpart in the reference: surfaces without the mapper).
// Contract: include/goslam_hip.h (gs_tsdf_*); tests/tsdf_restatement.py restates it serially.
//
// tsdf_integrate_kernel: one lane per lattice point, the 64 lanes of a wave along z (a wave's state loads and stores
// are 256 B runs), four waves per workgroup on consecutive runs.  A launch takes a batch of up to GS_TSDF_BATCH frames:
// the point's state (tsdf, weight, and with images the three colour sums) is loaded once, carried in registers over the
// batch in frame order and stored once.  A frame's matrix sits at a wave-uniform address, so it is read by scalar loads
// into SGPRs; the intrinsics and the lattice origin are kernel arguments.  Every point is owned by one lane: no atomics,
// and the result does not depend on the launch geometry.
//
// The skip: before any state is touched a wave tests each frame's frustum against the segment its 64-point run spans
// and keeps a bit per frame; frames without a bit are not evaluated, and a wave without any bit neither loads nor
// stores.  See tsdf_run_may_hit for why the test cannot change a result.  Compiled with -ffp-contract=off.
#include "tsdf_common.h"

namespace {

template <bool COLOR>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(
    float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ colors,
    const float* __restrict__ depth, const float* __restrict__ mask, const float* __restrict__ images,
    const float* __restrict__ w2c, int nframes, TsdfCam cam, float lox, float loy, float loz, float voxel, float trunc,
    float max_weight, int ny, int nz, int zchunks, long long nruns, long long npoints) {
  // the wave's run: wave-uniform, so everything derived from it lives in SGPRs and the frame branches are scalar
  const long long run = (long long)blockIdx.x * TSDF_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (run >= nruns) return;
  const int lane = threadIdx.x & 63;
  const long long row = run / zchunks;
  const int zc = (int)(run - row * zchunks);
  const int i = (int)(row / ny), j = (int)(row - (long long)i * ny);
  const float px = lox + (float)i * voxel;
  const float py = loy + (float)j * voxel;

  // bit f set: frame f may touch this run (its 64 points, whether or not the lattice ends inside it)
  const float pz0 = loz + (float)(zc * 64) * voxel, pz1 = loz + (float)(zc * 64 + 63) * voxel;
  unsigned live = 0;
  for (int f = 0; f < nframes; ++f)
    if (tsdf_run_may_hit(w2c + f * 12, cam, px, py, pz0, pz1, voxel)) live |= 1u << f;
  if (live == 0) return;

  const int k = zc * 64 + lane;
  if (k >= nz) return;
  const float pz = loz + (float)k * voxel;
  const size_t at = (size_t)row * nz + k;
  const size_t hw = (size_t)cam.h * cam.w;
  float t = tsdf[at], w0 = weight[at];
  float cr = 0.0f, cg = 0.0f, cb = 0.0f;
  if (COLOR) {
    cr = colors[at];
    cg = colors[(size_t)npoints + at];
    cb = colors[(size_t)2 * npoints + at];
  }
  for (int f = 0; f < nframes; ++f) {
    if (!((live >> f) & 1u)) continue;
    const float* __restrict__ m = w2c + f * 12;
    const float z = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
    if (!(z > 1e-3f)) continue;
    const float x = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
    const float y = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
    const float u = cam.fx * (x / z) + cam.cx;
    const float v = cam.fy * (y / z) + cam.cy;
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    if (!(fu >= 0.0f && fu < (float)cam.w && fv >= 0.0f && fv < (float)cam.h)) continue;
    const size_t pix = (size_t)f * hw + (size_t)((int)fv * cam.w + (int)fu);
    const float d = depth[pix];
    if (!(d > 0.0f)) continue;
    if (mask && mask[pix] == 0.0f) continue;
    const float sdf = d - z;
    if (sdf < -trunc) continue;
    const float s = fminf(1.0f, sdf / trunc);
    const float w1 = w0 + 1.0f;
    t = (t * w0 + s) / w1;
    if (COLOR && sdf <= trunc) {
      const float* __restrict__ img = images + (size_t)f * 3 * hw + (pix - (size_t)f * hw);
      cr = (cr * w0 + img[0]) / w1;
      cg = (cg * w0 + img[hw]) / w1;
      cb = (cb * w0 + img[2 * hw]) / w1;
    }
    w0 = fminf(w1, max_weight);
  }
  tsdf[at] = t;
  weight[at] = w0;
  if (COLOR) {
    colors[at] = cr;
    colors[(size_t)npoints + at] = cg;
    colors[(size_t)2 * npoints + at] = cb;
  }
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
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_integrate: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(tsdf && weight && depth && w2c, "tsdf_integrate: null pointer");
  GS_REQUIRE(!images || colors, "tsdf_integrate: images without a colour lattice");
  GS_REQUIRE(k >= 0 && h > 0 && w > 0 && (long long)h * w <= (1LL << 30), "tsdf_integrate: k=%d h=%d w=%d", k, h, w);
  GS_REQUIRE(fx > 0.0f && fy > 0.0f && voxel > 0.0f && trunc > 0.0f && max_weight >= 1.0f,
             "tsdf_integrate: fx=%g fy=%g voxel=%g trunc=%g max_weight=%g", fx, fy, voxel, trunc, max_weight);
  const TsdfCam cam = tsdf_cam(fx, fy, cx, cy, h, w);
  const int zchunks = gs_cdiv(nz, 64);
  const long long nruns = (long long)nx * ny * zchunks;
  const long long npoints = (long long)nx * ny * nz;
  const unsigned blocks = (unsigned)((nruns + TSDF_WAVES - 1) / TSDF_WAVES);
  const size_t hw = (size_t)h * w;
  for (int f0 = 0; f0 < k; f0 += GS_TSDF_BATCH) {
    const int nb = (k - f0 < GS_TSDF_BATCH) ? k - f0 : GS_TSDF_BATCH;
    const float* d = depth + (size_t)f0 * hw;
    const float* mk = mask ? mask + (size_t)f0 * hw : nullptr;
    const float* m = w2c + (size_t)f0 * 12;
    GS_TIMING_PRE();
    if (images)
      tsdf_integrate_kernel<true><<<blocks, TSDF_THREADS, 0, (hipStream_t)stream>>>(
          tsdf, weight, colors, d, mk, images + (size_t)f0 * 3 * hw, m, nb, cam, lo_x, lo_y, lo_z, voxel, trunc,
          max_weight, ny, nz, zchunks, nruns, npoints);
    else
      tsdf_integrate_kernel<false><<<blocks, TSDF_THREADS, 0, (hipStream_t)stream>>>(
          tsdf, weight, colors, d, mk, nullptr, m, nb, cam, lo_x, lo_y, lo_z, voxel, trunc, max_weight, ny, nz,
          zchunks, nruns, npoints);
    GS_CHECK_LAUNCH("tsdf_integrate");
  }
  return GS_OK;
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
