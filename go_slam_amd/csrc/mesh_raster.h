// The triangle rasteriser shared by the depth maps of cull.hip (gs_mesh_depth) and the visibility buffer of mesh_shade.hip
// (gs_mesh_visbuf): camera-space set-up, the watertight fp64 edge functions, the ray-plane depth, and the two walks (one
// thread per small face, one workgroup per large (face, pose)).  Both entry points cover the same pixels at the same fp64
// depth by construction; they differ in what a fragment stores.  Contract: include/goslam_neus.h (gs_mesh_depth).
#pragma once
#include "neus_common.h"

namespace {

constexpr int MD_BLOCK = 256;
constexpr int MD_LARGE_PIXELS = 256;   // bounding boxes above this many pixels go to the tiled (workgroup) path

struct Tri {
  double P[3][3];   // camera-space vertices, fp64
  double C[3][3];   // canonical edge cross products Plo x Phi for edges (0,1), (1,2), (2,0)
  double s[3];      // +1 if the edge runs lo -> hi in the face's order, else -1
  double det;       // P0 . (P1 x P2)
  int c0, c1, r0, r1;   // inclusive pixel range to test (empty when c0 > c1 or r0 > r1)
};

__device__ __forceinline__ void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = __dmul_rn(a[1], b[2]) - __dmul_rn(a[2], b[1]);
  o[1] = __dmul_rn(a[2], b[0]) - __dmul_rn(a[0], b[2]);
  o[2] = __dmul_rn(a[0], b[1]) - __dmul_rn(a[1], b[0]);
}

// Camera-space vertices of the face (fp64, every product and sum rounded on its own) and their z range.
__device__ __forceinline__ void tri_camera(const float* __restrict__ V, const int vid[3], const float* __restrict__ w2c,
                                           Tri& t, double& zmin, double& zmax) {
  double M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = (double)w2c[i];
  zmin = 1e300, zmax = -1e300;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double x = V[3 * (size_t)vid[j]], y = V[3 * (size_t)vid[j] + 1], z = V[3 * (size_t)vid[j] + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
      t.P[j][r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[4 * r], x), __dmul_rn(M[4 * r + 1], y)),
                                      __dmul_rn(M[4 * r + 2], z)), M[4 * r + 3]);
    zmin = fmin(zmin, t.P[j][2]);
    zmax = fmax(zmax, t.P[j][2]);
  }
}

// The canonical edge cross products, their signs and det from t.P; n = the face's camera-space normal
// s0 C0 + s1 C1 + s2 C2.  Returns false for a degenerate or non-finite face.
__device__ __forceinline__ bool tri_edges(const int vid[3], Tri& t, double n[3]) {
  const int e0[3] = {0, 1, 2}, e1[3] = {1, 2, 0};
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int a = e0[e], b = e1[e];
    const bool fwd = vid[a] <= vid[b];
    cross3(fwd ? t.P[a] : t.P[b], fwd ? t.P[b] : t.P[a], t.C[e]);
    t.s[e] = fwd ? 1.0 : -1.0;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) n[r] = t.s[0] * t.C[0][r] + t.s[1] * t.C[1][r] + t.s[2] * t.C[2][r];
  t.det = t.P[0][0] * n[0] + t.P[0][1] * n[1] + t.P[0][2] * n[2];
  return (n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0) && isfinite(t.det);
}

// Camera-space triangle of face `f` at pose `k` and the pixel range its near-clipped projection may cover.  Returns false
// when the face renders nothing at this pose (non-finite or degenerate, wholly in front of znear, wholly beyond far, or
// projecting onto no pixel).
__device__ bool tri_setup(const float* __restrict__ V, const int vid[3], const float* __restrict__ w2c, double fx,
                          double fy, double cx, double cy, int H, int W, double znear, double zfar, Tri& t) {
  double zmin, zmax;
  tri_camera(V, vid, w2c, t, zmin, zmax);
  if (!(zmax >= znear) || !(zmin <= zfar)) return false;   // also rejects NaN
  double n[3];
  if (!tri_edges(vid, t, n)) return false;
  const int e0[3] = {0, 1, 2}, e1[3] = {1, 2, 0};
  // screen bounds of the part with z >= znear: its vertices, and the edges' crossings of the near plane
  double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300;
  auto add = [&](double X, double Y, double Z) {
    const double u = fx * X / Z + cx, v = fy * Y / Z + cy;
    umin = fmin(umin, u); umax = fmax(umax, u); vmin = fmin(vmin, v); vmax = fmax(vmax, v);
  };
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const double* A = t.P[e0[e]];
    const double* B = t.P[e1[e]];
    if (A[2] >= znear) add(A[0], A[1], A[2]);
    if ((A[2] < znear) != (B[2] < znear)) {
      const double a = (znear - A[2]) / (B[2] - A[2]);
      add(A[0] + a * (B[0] - A[0]), A[1] + a * (B[1] - A[1]), znear);
    }
  }
  // pixel centre of column c is c + 0.5; widen by a pixel so rounding of the bounds never loses one
  const double cl = fmax(ceil(umin - 0.5) - 1.0, 0.0), ch = fmin(floor(umax - 0.5) + 1.0, (double)(W - 1));
  const double rl = fmax(ceil(vmin - 0.5) - 1.0, 0.0), rh = fmin(floor(vmax - 0.5) + 1.0, (double)(H - 1));
  if (!(cl <= ch) || !(rl <= rh)) return false;
  t.c0 = (int)cl; t.c1 = (int)ch; t.r0 = (int)rl; t.r1 = (int)rh;
  return true;
}

// The signed edge functions of the ray through the pixel centre (c + 0.5, r + 0.5); d = (dx, dy, 1).
__device__ __forceinline__ void tri_edge_functions(const Tri& t, int r, int c, double fx, double fy, double cx, double cy,
                                                   double e[3], double& dx, double& dy) {
  dx = ((double)c + 0.5 - cx) / fx, dy = ((double)r + 0.5 - cy) / fy;
#pragma unroll
  for (int k = 0; k < 3; ++k) e[k] = t.s[k] * (__dadd_rn(__dadd_rn(__dmul_rn(dx, t.C[k][0]), __dmul_rn(dy, t.C[k][1])),
                                                         t.C[k][2]));
}

// Depth of the pixel centre (c + 0.5, r + 0.5) on triangle t, or a negative value when not covered / clipped / too far.
__device__ __forceinline__ double tri_depth(const Tri& t, int r, int c, double fx, double fy, double cx, double cy,
                                            double znear, double zfar) {
  double e[3], dx, dy;
  tri_edge_functions(t, r, c, fx, fy, cx, cy, e, dx, dy);
  const bool in = (e[0] >= 0.0 && e[1] >= 0.0 && e[2] >= 0.0) || (e[0] <= 0.0 && e[1] <= 0.0 && e[2] <= 0.0);
  const double den = e[0] + e[1] + e[2];
  if (!in || den == 0.0) return -1.0;
  const double z = t.det / den;
  return (z >= znear && z <= zfar) ? z : -1.0;
}

// One thread per face, all K poses: small pixel ranges are walked here, the others queued for raster_large_faces.
// `frag(k, pixel, z, f)` stores one fragment: pose, r * W + c, fp64 depth, face.
template <class Frag>
__device__ __forceinline__ void raster_faces(const float* __restrict__ V, const int* __restrict__ Fc, int nf, int nv,
                                             const float* __restrict__ w2c, int K, double fx, double fy, double cx,
                                             double cy, int H, int W, double znear, double zfar,
                                             int2* __restrict__ large, int large_cap, int* __restrict__ large_count,
                                             Frag frag) {
  const int f = blockIdx.x * MD_BLOCK + threadIdx.x;
  if (f >= nf) return;
  const int vid[3] = {Fc[3 * (size_t)f], Fc[3 * (size_t)f + 1], Fc[3 * (size_t)f + 2]};
  if (vid[0] < 0 || vid[1] < 0 || vid[2] < 0 || vid[0] >= nv || vid[1] >= nv || vid[2] >= nv) return;
  if (vid[0] == vid[1] || vid[1] == vid[2] || vid[2] == vid[0]) return;
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    Tri t;
    if (!tri_setup(V, vid, w2c + 12 * (size_t)k, fx, fy, cx, cy, H, W, znear, zfar, t)) continue;
    const long long npx = (long long)(t.c1 - t.c0 + 1) * (t.r1 - t.r0 + 1);
    if (npx > MD_LARGE_PIXELS) {
      const int slot = atomicAdd(large_count, 1);
      if (slot < large_cap) {
        large[slot] = make_int2(f, k);
        continue;
      }                                             // list full: walk it here (slow, still correct)
    }
    for (int r = t.r0; r <= t.r1; ++r)
      for (int c = t.c0; c <= t.c1; ++c) {
        const double z = tri_depth(t, r, c, fx, fy, cx, cy, znear, zfar);
        if (z > 0.0) frag(k, (size_t)r * W + c, z, f);
      }
  }
}

// The large triangles: one workgroup per (face, pose), its threads striding over the pixel range.
template <class Frag>
__device__ __forceinline__ void raster_large_faces(const float* __restrict__ V, const int* __restrict__ Fc,
                                                   const float* __restrict__ w2c, double fx, double fy, double cx,
                                                   double cy, int H, int W, double znear, double zfar,
                                                   const int2* __restrict__ large, int large_cap,
                                                   const int* __restrict__ large_count, Frag frag) {
  const int n = min(*large_count, large_cap);
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int2 fk = large[i];
    const int vid[3] = {Fc[3 * (size_t)fk.x], Fc[3 * (size_t)fk.x + 1], Fc[3 * (size_t)fk.x + 2]};
    Tri t;
    if (!tri_setup(V, vid, w2c + 12 * (size_t)fk.y, fx, fy, cx, cy, H, W, znear, zfar, t)) continue;
    const int bw = t.c1 - t.c0 + 1;
    const int npx = bw * (t.r1 - t.r0 + 1);
    for (int p = threadIdx.x; p < npx; p += MD_BLOCK) {
      const int r = t.r0 + p / bw, c = t.c0 + p % bw;
      const double z = tri_depth(t, r, c, fx, fy, cx, cy, znear, zfar);
      if (z > 0.0) frag(fk.y, (size_t)r * W + c, z, fk.x);
    }
  }
}

}  // namespace
