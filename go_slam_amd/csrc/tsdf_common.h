// What tsdf.hip (running-mean fusion) and tsdf_live.hip (reversible integer fusion) share: the camera arguments, the
// conservative per-run frustum test and the host helpers of their entry points.  Both kernels evaluate the same geometry
// operation for operation; this file holds the parts that are literally the same text.
#pragma once
#include "common.h"

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

bool tsdf_dims_ok(int nx, int ny, int nz) {
  return nx >= 2 && nx <= 1024 && ny >= 2 && ny <= 1024 && nz >= 2 && nz <= 1024;
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

}  // namespace
