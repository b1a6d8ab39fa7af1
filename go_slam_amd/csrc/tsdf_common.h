// What tsdf.hip (running-mean fusion) and tsdf_live.hip (reversible integer fusion) share: the sweep that both fusion
// kernels are (tsdf_fuse), its per-run frustum test, the camera arguments and the host side of the two entry points
// (tsdf_fuse_enqueue).  A file adds only its rule: what a lattice point holds and what one observation does to it.
//
// The sweep: one lane per lattice point, the 64 lanes of a wave along z (a wave's state loads and stores are 256 B
// runs), four waves per workgroup on consecutive runs.  A launch takes a batch of up to GS_TSDF_BATCH frames: the
// point's state is loaded once, carried in registers over the batch in frame order and stored once.  A frame's matrix
// sits at a wave-uniform address, so it is read by scalar loads into SGPRs; the rule, the intrinsics and the lattice are
// by-value kernel arguments.  Every point is owned by one lane: no LDS, no atomics, and the result does not depend on
// the launch geometry.  The skip: before any state is touched a wave tests each frame's frustum against the segment its
// 64-point run spans and keeps a bit per frame; frames without a bit are not evaluated, and a wave without any bit
// neither loads nor stores.  See tsdf_run_may_hit for why the test cannot change a result.
#pragma once
#include "tsdf_cell.h"      // tsdf_dims_ok

namespace {

constexpr int TSDF_THREADS = 256;
constexpr int TSDF_WAVES = TSDF_THREADS / 64;

struct TsdfCam {           // by-value kernel arguments (SGPRs)
  float fx, fy, cx, cy;
  float nl, nr, nt, nb;    // norms of the four side planes' normals (left, right, top, bottom), host fp64 rounded up
  int h, w;
};

// Can any point of the segment e0..e1 (world coordinates; a wave's z-run, so x and y are shared) pass the kernel's
// per-point tests pc.z > 1e-3, -0.5 <= u < W - 0.5, -0.5 <= v < H - 0.5 for the frame with matrix m?  Those tests are half
// spaces of the camera frame: z > 1e-3 and, for z > 0, fx x + (cx + 0.5) z >= 0, -fx x + (W - 0.5 - cx) z > 0 and the
// same two in y.  Each left side is linear along the segment, so it is largest at an end: the segment lies outside a
// half space when both ends do.  "Outside" is taken with a margin rr in distance (times the normal's length, rounded
// up): half a voxel plus 2^-10 of the magnitudes involved.  The per-point fp32 arithmetic (a dozen roundings of relative
// size 2^-24) moves a point by about 2^-20 of them, a thousand times less.  So "false" is only returned when every point
// of the run fails its own test.
__device__ __forceinline__ bool tsdf_run_may_hit(const float* __restrict__ m, const TsdfCam cam, float pxw, float pyw,
                                                 float pz0, float pz1, float voxel) {
  const float bx = m[0] * pxw + m[1] * pyw, by = m[4] * pxw + m[5] * pyw, bz = m[8] * pxw + m[9] * pyw;
  const float x0 = (bx + m[2] * pz0) + m[3], x1 = (bx + m[2] * pz1) + m[3];
  const float y0 = (by + m[6] * pz0) + m[7], y1 = (by + m[6] * pz1) + m[7];
  const float z0 = (bz + m[10] * pz0) + m[11], z1 = (bz + m[10] * pz1) + m[11];
  const float mag = ((fabsf(m[3]) + fabsf(m[7])) + (fabsf(m[11]) + fabsf(pxw))) + ((fabsf(pyw) + fabsf(pz0)) + (fabsf(pz1) + 1.0f));
  const float rr = 0.5f * voxel + 0.0009765625f * mag;
  if (!(fmaxf(z0, z1) + rr > 1e-3f)) return false;
  const float a = cam.cx + 0.5f, b = ((float)cam.w - 0.5f) - cam.cx;
  const float c = cam.cy + 0.5f, d = ((float)cam.h - 0.5f) - cam.cy;
  if (fmaxf(cam.fx * x0 + a * z0, cam.fx * x1 + a * z1) < -(rr * cam.nl)) return false;
  if (fmaxf(b * z0 - cam.fx * x0, b * z1 - cam.fx * x1) < -(rr * cam.nr)) return false;
  if (fmaxf(cam.fy * y0 + c * z0, cam.fy * y1 + c * z1) < -(rr * cam.nt)) return false;
  if (fmaxf(d * z0 - cam.fy * y0, d * z1 - cam.fy * y1) < -(rr * cam.nb)) return false;
  return true;
}

struct TsdfSweep {         // by-value kernel argument (SGPRs): a batch of frames and the lattice they are fused into
  const float* depth;      // [nframes,h,w]
  const float* mask;       // [nframes,h,w] or NULL
  const float* images;     // [nframes,3,h,w]; read only by the COLOR kernels
  const float* w2c;        // [nframes,3,4]
  int nframes;
  TsdfCam cam;
  float lox, loy, loz, voxel, trunc;
  int ny, nz, zchunks;
  long long nruns, npoints;
};

// The body of both fusion kernels.  The rule, a plain struct passed by value, supplies State, a point's state, and
//   load(state, at, npoints, COLOR)    from offset `at` of the lattice; the colour part only with COLOR
//   fold(state, f, s, img, hw)         one observation of frame f of the batch: s = fminf(1, sdf / trunc) and, unless
//                                      img is NULL (no COLOR, or sdf > trunc), the pixel's img[0], img[hw], img[2 hw]
//   store(state, at, npoints, COLOR)   once, after the batch
// Which (point, frame) pairs reach fold, and with what s and pixel, is decided here alone, so every rule sees the same
// observations: what LiveFusion.finish() relies on when it promises the state of a fresh fusion.
template <bool COLOR, class Rule>
__device__ __forceinline__ void tsdf_fuse(const Rule rule, const TsdfSweep sw) {
  const TsdfCam cam = sw.cam;
  const float voxel = sw.voxel, trunc = sw.trunc;
  // the wave's run: wave-uniform, so everything derived from it lives in SGPRs and the frame branches are scalar
  const long long run = (long long)blockIdx.x * TSDF_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (run >= sw.nruns) return;
  const int lane = threadIdx.x & 63;
  const long long row = run / sw.zchunks;
  const int zc = (int)(run - row * sw.zchunks);
  const int i = (int)(row / sw.ny), j = (int)(row - (long long)i * sw.ny);
  const float px = sw.lox + (float)i * voxel;
  const float py = sw.loy + (float)j * voxel;

  // bit f set: frame f may touch this run (its 64 points, whether or not the lattice ends inside it)
  const float pz0 = sw.loz + (float)(zc * 64) * voxel, pz1 = sw.loz + (float)(zc * 64 + 63) * voxel;
  unsigned live = 0;
  for (int f = 0; f < sw.nframes; ++f)
    if (tsdf_run_may_hit(sw.w2c + f * 12, cam, px, py, pz0, pz1, voxel)) live |= 1u << f;
  if (live == 0) return;

  const int k = zc * 64 + lane;
  if (k >= sw.nz) return;
  const float pz = sw.loz + (float)k * voxel;
  const size_t at = (size_t)row * sw.nz + k;
  const size_t hw = (size_t)cam.h * cam.w;
  typename Rule::State state;
  rule.load(state, at, (size_t)sw.npoints, COLOR);
  for (int f = 0; f < sw.nframes; ++f) {
    if (!((live >> f) & 1u)) continue;
    const float* __restrict__ m = sw.w2c + f * 12;
    const float z = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
    if (!(z > 1e-3f)) continue;
    const float x = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
    const float y = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
    const float u = cam.fx * (x / z) + cam.cx;
    const float v = cam.fy * (y / z) + cam.cy;
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    if (!(fu >= 0.0f && fu < (float)cam.w && fv >= 0.0f && fv < (float)cam.h)) continue;
    const size_t pix = (size_t)f * hw + (size_t)((int)fv * cam.w + (int)fu);
    const float d = sw.depth[pix];
    if (!(d > 0.0f)) continue;
    if (sw.mask && sw.mask[pix] == 0.0f) continue;
    const float sdf = d - z;
    if (sdf < -trunc) continue;
    const float s = fminf(1.0f, sdf / trunc);
    rule.fold(state, f, s, COLOR && sdf <= trunc ? sw.images + (size_t)f * 3 * hw + (pix - (size_t)f * hw) : nullptr, hw);
  }
  rule.store(state, at, (size_t)sw.npoints, COLOR);
}

// |(fx, 0, a)| in double, rounded up to float: a larger norm only widens the skip test's margin
float tsdf_norm_up(double f, double a) {
  const double n = sqrt(f * f + a * a);
  float r = (float)n;
  if ((double)r < n) r = nextafterf(r, INFINITY);
  return r;
}

TsdfCam tsdf_cam(float fx, float fy, float cx, float cy, int h, int w) {
  TsdfCam cam;
  cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy;
  cam.h = h; cam.w = w;
  cam.nl = tsdf_norm_up(fx, (double)cx + 0.5);
  cam.nr = tsdf_norm_up(fx, ((double)w - 0.5) - cx);
  cam.nt = tsdf_norm_up(fy, (double)cy + 0.5);
  cam.nb = tsdf_norm_up(fy, ((double)h - 0.5) - cy);
  return cam;
}

// gs_tsdf_integrate and gs_tsdf_accumulate after the checks of their own arguments (`name`: the entry point's, for the
// error texts and the timer): the lattice's and the frames' checks, then a launch per batch of GS_TSDF_BATCH frames,
// `coloured` with images and `plain` without, with rule_at(f0), the rule of the batch that begins at frame f0.
template <class Rule, class RuleAt>
int tsdf_fuse_enqueue(const char* name, void (*coloured)(Rule, TsdfSweep), void (*plain)(Rule, TsdfSweep), int nx,
                      int ny, int nz, const float* depth, const float* mask, const float* images, const float* w2c, int k,
                      int h, int w, float fx, float fy, float cx, float cy, float lo_x, float lo_y, float lo_z,
                      float voxel, float trunc, gs_stream_t stream, RuleAt rule_at) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "%s: lattice %d x %d x %d outside [2, 1024]", name, nx, ny, nz);
  GS_REQUIRE(k >= 0 && h > 0 && w > 0 && (long long)h * w <= (1LL << 30), "%s: k=%d h=%d w=%d", name, k, h, w);
  TsdfSweep sw;
  sw.cam = tsdf_cam(fx, fy, cx, cy, h, w);
  sw.lox = lo_x; sw.loy = lo_y; sw.loz = lo_z; sw.voxel = voxel; sw.trunc = trunc;
  sw.ny = ny; sw.nz = nz; sw.zchunks = gs_cdiv(nz, 64);
  sw.nruns = (long long)nx * ny * sw.zchunks;
  sw.npoints = (long long)nx * ny * nz;
  const unsigned blocks = (unsigned)((sw.nruns + TSDF_WAVES - 1) / TSDF_WAVES);
  const size_t hw = (size_t)h * w;
  for (int f0 = 0; f0 < k; f0 += GS_TSDF_BATCH) {
    sw.nframes = (k - f0 < GS_TSDF_BATCH) ? k - f0 : GS_TSDF_BATCH;
    sw.depth = depth + (size_t)f0 * hw;
    sw.mask = mask ? mask + (size_t)f0 * hw : nullptr;
    sw.images = images ? images + (size_t)f0 * 3 * hw : nullptr;
    sw.w2c = w2c + (size_t)f0 * 12;
    GS_TIMING_PRE();
    (images ? coloured : plain)<<<blocks, TSDF_THREADS, 0, (hipStream_t)stream>>>(rule_at(f0), sw);
    GS_CHECK_LAUNCH(name);
  }
  return GS_OK;
}

}  // namespace
