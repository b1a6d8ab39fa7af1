// Per-pixel geometry shared by geom.hip (iproj, depth_filter) and pointcloud.hip (the keyframe point cloud), so that
// the fused point-cloud path counts and back-projects with the very same instructions.  Both translation units are
// compiled with -ffp-contract=off.
#pragma once
#include "common.h"

__device__ __forceinline__ void gs_load_pose(const float* poses, int k, float* t, float* q) {
  const float* p = poses + (size_t)k * 7;
  t[0] = p[0]; t[1] = p[1]; t[2] = p[2];
  q[0] = p[3]; q[1] = p[4]; q[2] = p[5]; q[3] = p[6];
}

// iproj (droid_kernels.cu:779-850): pixel (u, v) of inverse depth d through pose (t, q), divided by its last
// homogeneous coordinate.
__device__ __forceinline__ void gs_iproj_point(const float* t, const float* q, float fx, float fy, float cx, float cy,
                                               float u, float v, float d, float* out) {
  float Xi[4] = {(u - cx) / fx, (v - cy) / fy, 1.0f, d};
  float Xj[4];
  gs_act_se3(t, q, Xi, Xj);
  out[0] = Xj[0] / Xj[3];
  out[1] = Xj[1] / Xj[3];
  out[2] = Xj[2] / Xj[3];
}

// One neighbour's vote of depth_filter (droid_kernels.cu:661-775): pixel (ui, vi) of frame ix (pose ti, qi, inverse
// depth di) projected into frame jx; 1 when one of the four corners of the cell it lands in (strictly inside the
// image: u0 < wd-1, v0 < ht-1) has an inverse depth within th, compared in double.  The caller checks 0 <= jx < num.
__device__ __forceinline__ float gs_depth_filter_vote(const float* __restrict__ poses, const float* __restrict__ disps,
                                                      const float* ti, const float* qi, int jx, float fx, float fy,
                                                      float cx, float cy, float ui, float vi, float di, float th,
                                                      int hw, int ht, int wd) {
  float tj[3], qj[4], tij[3], qij[4];
  gs_load_pose(poses, jx, tj, qj);
  gs_rel_se3(ti, qi, tj, qj, tij, qij);
  float Xi[4] = {(ui - cx) / fx, (vi - cy) / fy, 1.0f, di};
  float Xj[4];
  gs_act_se3(tij, qij, Xi, Xj);
  const float uj = fx * (Xj[0] / Xj[2]) + cx;
  const float vj = fy * (Xj[1] / Xj[2]) + cy;
  const float dj = Xj[3] / Xj[2];
  const float fu = floorf(uj), fv = floorf(vj);
  if (fu >= 0.f && fv >= 0.f && fu < (float)(wd - 1) && fv < (float)(ht - 1)) {
    const int u0 = (int)fu, v0 = (int)fv;
    const float* dj_map = disps + (size_t)jx * hw + (size_t)v0 * wd + u0;
    const double inv = 1.0 / (double)dj;
    const double t = (double)th;
    if (fabs(inv - 1.0 / (double)dj_map[0]) < t) return 1.0f;
    else if (fabs(inv - 1.0 / (double)dj_map[1]) < t) return 1.0f;
    else if (fabs(inv - 1.0 / (double)dj_map[wd]) < t) return 1.0f;
    else if (fabs(inv - 1.0 / (double)dj_map[wd + 1]) < t) return 1.0f;
  }
  return 0.0f;
}

// depth_filter's count for pixel p of frame ix: the votes of neighbours ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 that lie in
// [0, num), summed in the reference's order.
__device__ __forceinline__ float gs_depth_filter_count(const float* __restrict__ poses, const float* __restrict__ disps,
                                                       int ix, int p, float fx, float fy, float cx, float cy, float th,
                                                       int num, int hw, int ht, int wd) {
  const float ui = (float)(p % wd), vi = (float)(p / wd);
  const float di = disps[(size_t)ix * hw + p];
  float ti[3], qi[4];
  gs_load_pose(poses, ix, ti, qi);
  float count = 0.f;
#pragma unroll
  for (int neigh = 0; neigh < 6; ++neigh) {
    const int jx = (neigh < 3) ? ix - neigh - 1 : ix + neigh;
    if (jx < 0 || jx >= num) continue;
    count += gs_depth_filter_vote(poses, disps, ti, qi, jx, fx, fy, cx, cy, ui, vi, di, th, hw, ht, wd);
  }
  return count;
}
