// A point in a TSDF lattice, once for every kernel that gathers one: the lattice as a kernel argument, the cell under a
// point, its eight corners and the trilinear value and gradient.  tsdf_raycast.hip, tsdf_align.hip, tsdf_merge.hip and
// esdf.hip's query promise the same operation sequences (include/goslam_hip.h), one rounding per operation: they are
// these functions.  Compiled with -ffp-contract=off; everything is inlined, so a caller's code is what it wrote out before.
#pragma once
#include "common.h"

namespace {

constexpr int TSDF_DIM_MAX = 1024;          // lattice points per axis

bool tsdf_dims_ok(int nx, int ny, int nz) {
  return nx >= 2 && nx <= TSDF_DIM_MAX && ny >= 2 && ny <= TSDF_DIM_MAX && nz >= 2 && nz <= TSDF_DIM_MAX;
}

struct TsdfLattice {       // by-value kernel argument (SGPRs)
  int ny, nz;
  float topx, topy, topz;  // float(n - 1)
  float lox, loy, loz, voxel;
};

TsdfLattice tsdf_lattice(int nx, int ny, int nz, float lo_x, float lo_y, float lo_z, float voxel) {
  TsdfLattice l;
  l.ny = ny; l.nz = nz;
  l.topx = (float)(nx - 1); l.topy = (float)(ny - 1); l.topz = (float)(nz - 1);
  l.lox = lo_x; l.loy = lo_y; l.loz = lo_z; l.voxel = voxel;
  return l;
}

// Has the point with the floors (ax, ay, az) of its lattice coordinates a cell?  0 <= a < n - 1 on every axis; a NaN
// fails, and the comparison comes before any cast.
__device__ __forceinline__ bool tsdf_cell_inside(const TsdfLattice& l, float ax, float ay, float az) {
  return ax >= 0.0f && ax < l.topx && ay >= 0.0f && ay < l.topy && az >= 0.0f && az < l.topz;
}

// The offset of a cell's corner (0,0,0).  Off is the caller's offset type: unsigned where 32 bits are known to do (the
// largest lattice has 2^30 points), size_t elsewhere.
template <class Off>
__device__ __forceinline__ Off tsdf_cell_at(const TsdfLattice& l, int ax, int ay, int az) {
  return ((Off)ax * (Off)l.ny + (Off)ay) * (Off)l.nz + (Off)az;
}

__device__ __forceinline__ float tsdf_lerp(float p, float q, float s) { return p + s * (q - p); }

struct TsdfCorners { float v000, v001, v010, v011, v100, v101, v110, v111; };   // v[x][y][z]

template <class Off>
__device__ __forceinline__ TsdfCorners tsdf_corners_load(const float* __restrict__ p, Off at, int ny, int nz) {
  const Off sy = (Off)nz, sx = (Off)ny * (Off)nz;
  TsdfCorners c;
  c.v000 = p[at];           c.v001 = p[at + 1];
  c.v010 = p[at + sy];      c.v011 = p[at + sy + 1];
  c.v100 = p[at + sx];      c.v101 = p[at + sx + 1];
  c.v110 = p[at + sx + sy]; c.v111 = p[at + sx + sy + 1];
  return c;
}

__device__ __forceinline__ bool tsdf_corners_at_least(const TsdfCorners& c, float m) {
  return c.v000 >= m && c.v001 >= m && c.v010 >= m && c.v011 >= m && c.v100 >= m && c.v101 >= m && c.v110 >= m && c.v111 >= m;
}

// the value: lerps along z (four), then y (two), then x (one)
__device__ __forceinline__ float tsdf_corners_value(const TsdfCorners& c, float sx, float sy, float sz) {
  const float z00 = tsdf_lerp(c.v000, c.v001, sz), z01 = tsdf_lerp(c.v010, c.v011, sz);
  const float z10 = tsdf_lerp(c.v100, c.v101, sz), z11 = tsdf_lerp(c.v110, c.v111, sz);
  return tsdf_lerp(tsdf_lerp(z00, z01, sy), tsdf_lerp(z10, z11, sy), sx);
}

// The gradient in lattice units, from the z-lerps of the four z-edges and the y-lerps of the four y-edges: g[0] is the
// difference of the value's two y-lerps, g[1] and g[2] the differences of the x-lerps of the z-lerps and of the y-lerps.
// A caller that also takes the value shares its z-lerps and y-lerps: the same operations on the same operands.
__device__ __forceinline__ void tsdf_corners_gradient(const TsdfCorners& c, float sx, float sy, float sz, float g[3]) {
  const float z00 = tsdf_lerp(c.v000, c.v001, sz), z01 = tsdf_lerp(c.v010, c.v011, sz);
  const float z10 = tsdf_lerp(c.v100, c.v101, sz), z11 = tsdf_lerp(c.v110, c.v111, sz);
  const float y00 = tsdf_lerp(c.v000, c.v010, sy), y01 = tsdf_lerp(c.v001, c.v011, sy);
  const float y10 = tsdf_lerp(c.v100, c.v110, sy), y11 = tsdf_lerp(c.v101, c.v111, sy);
  g[0] = tsdf_lerp(z10, z11, sy) - tsdf_lerp(z00, z01, sy);
  g[1] = tsdf_lerp(z01, z11, sx) - tsdf_lerp(z00, z10, sx);
  g[2] = tsdf_lerp(y01, y11, sx) - tsdf_lerp(y00, y10, sx);
}

}  // namespace
