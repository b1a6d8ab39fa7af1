// The surface sample of a cell of a TSDF lattice, once for every kernel that takes one (tsdf_planes.hip, tsdf_objects.hip):
// a point on the zero set one Newton step from the cell's centre, with the gradient there as its normal direction
// (include/goslam_hip.h, "the surface sample of a cell").  Most cells have none: they leave after the eight weights or the
// eight values.  Compiled with -ffp-contract=off; everything is inlined.
#pragma once
#include "tsdf_cell.h"

namespace {

struct PlaneField {        // by-value kernel argument (SGPRs)
  const float* tsdf;
  const float* weight;
  TsdfLattice l;
  int cy, cz;              // cells along y and z
  int n_cells;
  float min_weight;
};

struct PlaneSample { float g[3], p[3], gg; };

__device__ __forceinline__ bool plane_unsaturated(const TsdfCorners& c) {          // a NaN fails
  return fabsf(c.v000) < 1.0f && fabsf(c.v001) < 1.0f && fabsf(c.v010) < 1.0f && fabsf(c.v011) < 1.0f &&
         fabsf(c.v100) < 1.0f && fabsf(c.v101) < 1.0f && fabsf(c.v110) < 1.0f && fabsf(c.v111) < 1.0f;
}

__device__ __forceinline__ bool plane_sign_change(const TsdfCorners& c) {
  const bool neg = c.v000 < 0.0f || c.v001 < 0.0f || c.v010 < 0.0f || c.v011 < 0.0f || c.v100 < 0.0f || c.v101 < 0.0f ||
                   c.v110 < 0.0f || c.v111 < 0.0f;
  const bool pos = c.v000 >= 0.0f || c.v001 >= 0.0f || c.v010 >= 0.0f || c.v011 >= 0.0f || c.v100 >= 0.0f ||
                   c.v101 >= 0.0f || c.v110 >= 0.0f || c.v111 >= 0.0f;
  return neg && pos;
}

// The surface sample of cell s (row-major over the cells), or false.  s < d.n_cells: every corner is a lattice point.
__device__ __forceinline__ bool plane_sample(const PlaneField& d, int s, PlaneSample& o) {
  const int cyz = d.cy * d.cz;
  const int a = s / cyz, rem = s - a * cyz;
  const int b = rem / d.cz, c = rem - b * d.cz;
  const unsigned at = tsdf_cell_at<unsigned>(d.l, a, b, c);
  const TsdfCorners wc = tsdf_corners_load(d.weight, at, d.l.ny, d.l.nz);
  if (!tsdf_corners_at_least(wc, d.min_weight)) return false;
  const TsdfCorners v = tsdf_corners_load(d.tsdf, at, d.l.ny, d.l.nz);
  if (!plane_unsaturated(v) || !plane_sign_change(v)) return false;
  const float f = tsdf_corners_value(v, 0.5f, 0.5f, 0.5f);
  tsdf_corners_gradient(v, 0.5f, 0.5f, 0.5f, o.g);
  const float gg = (o.g[0] * o.g[0] + o.g[1] * o.g[1]) + o.g[2] * o.g[2];
  if (!(gg > 0.0f && f * f <= gg)) return false;
  const float t = f / gg;
  o.gg = gg;
  o.p[0] = d.l.lox + (((float)a + 0.5f) - t * o.g[0]) * d.l.voxel;
  o.p[1] = d.l.loy + (((float)b + 0.5f) - t * o.g[1]) * d.l.voxel;
  o.p[2] = d.l.loz + (((float)c + 0.5f) - t * o.g[2]) * d.l.voxel;
  return true;
}

// does the sample's normal direction lie in the cone about n?
__device__ __forceinline__ bool plane_agrees(const PlaneSample& s, float n0, float n1, float n2, float cos2) {
  const float d = (n0 * s.g[0] + n1 * s.g[1]) + n2 * s.g[2];
  return d > 0.0f && d * d >= cos2 * s.gg;
}

__device__ __forceinline__ float plane_dot(const PlaneSample& s, float n0, float n1, float n2) {
  return (n0 * s.p[0] + n1 * s.p[1]) + n2 * s.p[2];
}

bool plane_finite(float v) { return fabsf(v) < INFINITY; }

int plane_cells(int nx, int ny, int nz) { return (nx - 1) * (ny - 1) * (nz - 1); }      // < 2^30

PlaneField plane_field(const float* tsdf, const float* weight, int nx, int ny, int nz, float lo_x, float lo_y, float lo_z,
                       float voxel, float min_weight) {
  PlaneField d;
  d.tsdf = tsdf; d.weight = weight;
  d.l = tsdf_lattice(nx, ny, nz, lo_x, lo_y, lo_z, voxel);
  d.cy = ny - 1; d.cz = nz - 1;
  d.n_cells = plane_cells(nx, ny, nz);
  d.min_weight = min_weight;
  return d;
}

}  // namespace
