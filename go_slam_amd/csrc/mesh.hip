// Mesh extraction (InstantNeuS.extract_geometry, reference src/InstantNeuS.py:457-497): the -sdf lattice straight from the
// hash grid (one fused launch instead of encode + addmm + select per chunk) and marching cubes over any float32 volume in
// launches that never wait on another workgroup -- count, scan, emit.  Contract and ordering: include/goslam_neus.h.
#include "neus_common.h"

namespace {

// ---------------------------------------------------------------------------------------
// fused SDF lattice
// ---------------------------------------------------------------------------------------
// One level's two interpolated features -- the value half of neus.hip's grid_level, op for op (same corner order, weight
// products and fmaf chain), so the features equal gs_grid_encode's bit for bit.
__device__ __forceinline__ void lattice_level(const gs_grid_meta& m, int l, const _Float16* __restrict__ grid,
                                              const float x[3], float val[2]) {
  const float scale = m.scale[l];
  float f[3];
  uint32_t g[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float pos = fmaf(scale, x[d], 0.5f);
    const float fl = floorf(pos);
    g[d] = (uint32_t)(int)fl;
    f[d] = pos - fl;
  }
  const _Float16* tab = grid + (size_t)m.offset[l] * 2;
  uint32_t cidx[8];
  grid_corners(m, l, g, cidx);
  float v[8][2];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint32_t raw = *reinterpret_cast<const uint32_t*>(tab + (size_t)cidx[c] * 2);
    v[c][0] = (float)__builtin_bit_cast(_Float16, (uint16_t)(raw & 0xffffu));
    v[c][1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(raw >> 16));
  }
  val[0] = 0.f; val[1] = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float w = 1.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) w = w * (((c >> d) & 1) ? f[d] : (1.0f - f[d]));
    val[0] = fmaf(w, v[c][0], val[0]);
    val[1] = fmaf(w, v[c][1], val[1]);
  }
}

// u[i,j,k] = -(b0 + W0 . [p, enc(p)]) at (xs[i], ys[j], zs[k]); -100 unless strictly inside the realtime bound.  The
// normalisation is SDFNetwork._query's op by op: p = clamp((x - b0) / span * 2 - 1, -1, 1), grid input (p + 1) / 2.
__global__ __launch_bounds__(256) void sdf_lattice_kernel(const float* __restrict__ xs, const float* __restrict__ ys,
                                                          const float* __restrict__ zs, int nx, int ny, int nz,
                                                          const float* __restrict__ bound, const float* __restrict__ rt,
                                                          const _Float16* __restrict__ grid, const float* __restrict__ w0,
                                                          const float* __restrict__ b0, float* __restrict__ u,
                                                          gs_grid_meta m) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nx * ny * nz) return;
  const int k = p % nz, j = (p / nz) % ny, i = p / (nz * ny);
  const float pt[3] = {xs[i], ys[j], zs[k]};
  bool inside = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) inside = inside && (pt[d] > rt[2 * d]) && (pt[d] < rt[2 * d + 1]);
  if (!inside) {                     // InstantNeuS.in_bound is strict; outside: no gathers at all
    u[p] = -100.0f;
    return;
  }
  float q[3], x[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float lo = bound[2 * d], span = bound[2 * d + 1] - bound[2 * d];
    float v = (pt[d] - lo) / span;
    v = v * 2.0f;
    v = v - 1.0f;
    v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);      // torch.clamp (a NaN stays a NaN)
    q[d] = v;
    x[d] = (v + 1.0f) / 2.0f;
  }
  float acc = 0.0f;
#pragma unroll
  for (int d = 0; d < 3; ++d) acc = fmaf(w0[d], q[d], acc);
#pragma unroll 1
  for (int l = 0; l < GS_GRID_LEVELS; ++l) {
    float val[2];
    lattice_level(m, l, grid, x, val);
    // the fp32 value first, then the fp16 rounding, as gs_grid_encode stores it: without this barrier the compiler folds
    // the last interpolation fmaf and the conversion into one v_fma_mixlo_f16 -- a single rounding to fp16, which
    // differs from the double rounding now and then
    asm volatile("" : "+v"(val[0]), "+v"(val[1]));
    acc = fmaf(w0[3 + 2 * l], (float)(_Float16)val[0], acc);       // features rounded to fp16 (tcnn's output type)
    acc = fmaf(w0[4 + 2 * l], (float)(_Float16)val[1], acc);
  }
  u[p] = -(acc + b0[0]);
}

// ---------------------------------------------------------------------------------------
// marching cubes
// ---------------------------------------------------------------------------------------
constexpr int MC_BLOCK = 256;        // lattice points per count / emit workgroup
constexpr int MC_CHUNK = 1024;       // workgroup totals per scan_a workgroup
constexpr int MC_MAX_CHUNKS = 4096;  // 1024^3 / (MC_BLOCK * MC_CHUNK): scan_b's single workgroup covers them all

// Cube corners: 0 (0,0,0) 1 (1,0,0) 2 (1,1,0) 3 (0,1,0) 4 (0,0,1) 5 (1,0,1) 6 (1,1,1) 7 (0,1,1); case bit c set iff
// corner c is below.  Cube edge -> (offset of its lower corner, axis).
__constant__ int8_t kEdgeGeom[12][4] = {
    {0, 0, 0, 0},
    {1, 0, 0, 1},
    {0, 1, 0, 0},
    {0, 0, 0, 1},
    {0, 0, 1, 0},
    {1, 0, 1, 1},
    {0, 1, 1, 0},
    {0, 0, 1, 1},
    {0, 0, 0, 2},
    {1, 0, 0, 2},
    {1, 1, 0, 2},
    {0, 1, 0, 2},
};
// Triangles per case as cube-edge triples, -1 terminated.  Generated by resolving every cube face from its own four corner
// classes (below corners that meet only diagonally on a face stay separated), chaining the faces' oriented segments into
// loops and fanning every loop from a vertex that shares no cube face with the loop's non-adjacent vertices; wound so that
// (v1 - v0) x (v2 - v0) points toward decreasing u.  At most five triangles per case; case 1 is (0, 8, 3), as in the
// commonly circulated table.
__constant__ int8_t kTriTable[256][16] = {
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  8,  1,  8,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  1,  2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  2, 10,  0, 10,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2, 10,  9,  2,  9,  8,  2,  8,  3, -1, -1, -1, -1, -1, -1, -1},
    { 2,  3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8, 11,  0, 11,  2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  2,  3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  8,  1,  8, 11,  1, 11,  2, -1, -1, -1, -1, -1, -1, -1},
    { 1,  3, 11,  1, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8, 11,  0, 11, 10,  0, 10,  1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  3, 11,  0, 11, 10,  0, 10,  9, -1, -1, -1, -1, -1, -1, -1},
    { 8, 11, 10,  8, 10,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 4,  7,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  7,  0,  7,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  4,  7,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  4,  1,  4,  7,  1,  7,  3, -1, -1, -1, -1, -1, -1, -1},
    { 1,  2, 10,  4,  7,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  7,  0,  7,  3,  1,  2, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  2, 10,  0, 10,  9,  4,  7,  8, -1, -1, -1, -1, -1, -1, -1},
    { 2, 10,  9,  2,  9,  4,  2,  4,  7,  2,  7,  3, -1, -1, -1, -1},
    { 2,  3, 11,  4,  7,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  7,  0,  7, 11,  0, 11,  2, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  2,  3, 11,  4,  7,  8, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  4,  1,  4,  7,  1,  7, 11,  1, 11,  2, -1, -1, -1, -1},
    { 1,  3, 11,  1, 11, 10,  4,  7,  8, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  7,  0,  7, 11,  0, 11, 10,  0, 10,  1, -1, -1, -1, -1},
    { 0,  3, 11,  0, 11, 10,  0, 10,  9,  4,  7,  8, -1, -1, -1, -1},
    { 4,  7, 11,  4, 11, 10,  4, 10,  9, -1, -1, -1, -1, -1, -1, -1},
    { 4,  9,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  4,  9,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  5,  0,  5,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  5,  4,  1,  4,  8,  1,  8,  3, -1, -1, -1, -1, -1, -1, -1},
    { 1,  2, 10,  4,  9,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  1,  2, 10,  4,  9,  5, -1, -1, -1, -1, -1, -1, -1},
    { 0,  2, 10,  0, 10,  5,  0,  5,  4, -1, -1, -1, -1, -1, -1, -1},
    { 2, 10,  5,  2,  5,  4,  2,  4,  8,  2,  8,  3, -1, -1, -1, -1},
    { 2,  3, 11,  4,  9,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8, 11,  0, 11,  2,  4,  9,  5, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  5,  0,  5,  4,  2,  3, 11, -1, -1, -1, -1, -1, -1, -1},
    { 1,  5,  4,  1,  4,  8,  1,  8, 11,  1, 11,  2, -1, -1, -1, -1},
    { 1,  3, 11,  1, 11, 10,  4,  9,  5, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8, 11,  0, 11, 10,  0, 10,  1,  4,  9,  5, -1, -1, -1, -1},
    { 0,  3, 11,  0, 11, 10,  0, 10,  5,  0,  5,  4, -1, -1, -1, -1},
    { 4,  8, 11,  4, 11, 10,  4, 10,  5, -1, -1, -1, -1, -1, -1, -1},
    { 5,  7,  8,  5,  8,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  0,  5,  7,  0,  7,  3, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  5,  0,  5,  7,  0,  7,  8, -1, -1, -1, -1, -1, -1, -1},
    { 1,  5,  7,  1,  7,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  2, 10,  5,  7,  8,  5,  8,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  0,  5,  7,  0,  7,  3,  1,  2, 10, -1, -1, -1, -1},
    { 0,  2, 10,  0, 10,  5,  0,  5,  7,  0,  7,  8, -1, -1, -1, -1},
    { 2, 10,  5,  2,  5,  7,  2,  7,  3, -1, -1, -1, -1, -1, -1, -1},
    { 2,  3, 11,  5,  7,  8,  5,  8,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  0,  5,  7,  0,  7, 11,  0, 11,  2, -1, -1, -1, -1},
    { 0,  1,  5,  0,  5,  7,  0,  7,  8,  2,  3, 11, -1, -1, -1, -1},
    { 1,  5,  7,  1,  7, 11,  1, 11,  2, -1, -1, -1, -1, -1, -1, -1},
    { 1,  3, 11,  1, 11, 10,  5,  7,  8,  5,  8,  9, -1, -1, -1, -1},
    { 0,  9,  5,  0,  5,  7,  0,  7, 11,  0, 11, 10,  0, 10,  1, -1},
    { 0,  3, 11,  0, 11, 10,  0, 10,  5,  0,  5,  7,  0,  7,  8, -1},
    { 5,  7, 11,  5, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 5, 10,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  5, 10,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  5, 10,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  8,  1,  8,  3,  5, 10,  6, -1, -1, -1, -1, -1, -1, -1},
    { 1,  2,  6,  1,  6,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  1,  2,  6,  1,  6,  5, -1, -1, -1, -1, -1, -1, -1},
    { 0,  2,  6,  0,  6,  5,  0,  5,  9, -1, -1, -1, -1, -1, -1, -1},
    { 2,  6,  5,  2,  5,  9,  2,  9,  8,  2,  8,  3, -1, -1, -1, -1},
    { 2,  3, 11,  5, 10,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8, 11,  0, 11,  2,  5, 10,  6, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  2,  3, 11,  5, 10,  6, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  8,  1,  8, 11,  1, 11,  2,  5, 10,  6, -1, -1, -1, -1},
    { 1,  3, 11,  1, 11,  6,  1,  6,  5, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8, 11,  0, 11,  6,  0,  6,  5,  0,  5,  1, -1, -1, -1, -1},
    { 0,  3, 11,  0, 11,  6,  0,  6,  5,  0,  5,  9, -1, -1, -1, -1},
    { 5,  9,  8,  5,  8, 11,  5, 11,  6, -1, -1, -1, -1, -1, -1, -1},
    { 4,  7,  8,  5, 10,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  7,  0,  7,  3,  5, 10,  6, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  4,  7,  8,  5, 10,  6, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  4,  1,  4,  7,  1,  7,  3,  5, 10,  6, -1, -1, -1, -1},
    { 1,  2,  6,  1,  6,  5,  4,  7,  8, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  7,  0,  7,  3,  1,  2,  6,  1,  6,  5, -1, -1, -1, -1},
    { 0,  2,  6,  0,  6,  5,  0,  5,  9,  4,  7,  8, -1, -1, -1, -1},
    { 2,  6,  5,  2,  5,  9,  2,  9,  4,  2,  4,  7,  2,  7,  3, -1},
    { 2,  3, 11,  4,  7,  8,  5, 10,  6, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  7,  0,  7, 11,  0, 11,  2,  5, 10,  6, -1, -1, -1, -1},
    { 0,  1,  9,  2,  3, 11,  4,  7,  8,  5, 10,  6, -1, -1, -1, -1},
    { 1,  9,  4,  1,  4,  7,  1,  7, 11,  1, 11,  2,  5, 10,  6, -1},
    { 1,  3, 11,  1, 11,  6,  1,  6,  5,  4,  7,  8, -1, -1, -1, -1},
    { 0,  4,  7,  0,  7, 11,  0, 11,  6,  0,  6,  5,  0,  5,  1, -1},
    { 0,  3, 11,  0, 11,  6,  0,  6,  5,  0,  5,  9,  4,  7,  8, -1},
    {11,  6,  5, 11,  5,  9, 11,  9,  4, 11,  4,  7, -1, -1, -1, -1},
    { 4,  9, 10,  4, 10,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  4,  9, 10,  4, 10,  6, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1, 10,  0, 10,  6,  0,  6,  4, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10,  6,  1,  6,  4,  1,  4,  8,  1,  8,  3, -1, -1, -1, -1},
    { 1,  2,  6,  1,  6,  4,  1,  4,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  1,  2,  6,  1,  6,  4,  1,  4,  9, -1, -1, -1, -1},
    { 0,  2,  6,  0,  6,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  6,  4,  2,  4,  8,  2,  8,  3, -1, -1, -1, -1, -1, -1, -1},
    { 2,  3, 11,  4,  9, 10,  4, 10,  6, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8, 11,  0, 11,  2,  4,  9, 10,  4, 10,  6, -1, -1, -1, -1},
    { 0,  1, 10,  0, 10,  6,  0,  6,  4,  2,  3, 11, -1, -1, -1, -1},
    { 1, 10,  6,  1,  6,  4,  1,  4,  8,  1,  8, 11,  1, 11,  2, -1},
    { 1,  3, 11,  1, 11,  6,  1,  6,  4,  1,  4,  9, -1, -1, -1, -1},
    {11,  6,  4, 11,  4,  9, 11,  9,  1, 11,  1,  0, 11,  0,  8, -1},
    { 0,  3, 11,  0, 11,  6,  0,  6,  4, -1, -1, -1, -1, -1, -1, -1},
    { 4,  8, 11,  4, 11,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 6,  7,  8,  6,  8,  9,  6,  9, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9, 10,  0, 10,  6,  0,  6,  7,  0,  7,  3, -1, -1, -1, -1},
    { 0,  1, 10,  0, 10,  6,  0,  6,  7,  0,  7,  8, -1, -1, -1, -1},
    { 1, 10,  6,  1,  6,  7,  1,  7,  3, -1, -1, -1, -1, -1, -1, -1},
    { 1,  2,  6,  1,  6,  7,  1,  7,  8,  1,  8,  9, -1, -1, -1, -1},
    { 9,  1,  2,  9,  2,  6,  9,  6,  7,  9,  7,  3,  9,  3,  0, -1},
    { 0,  2,  6,  0,  6,  7,  0,  7,  8, -1, -1, -1, -1, -1, -1, -1},
    { 2,  6,  7,  2,  7,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  3, 11,  6,  7,  8,  6,  8,  9,  6,  9, 10, -1, -1, -1, -1},
    { 0,  9, 10,  0, 10,  6,  0,  6,  7,  0,  7, 11,  0, 11,  2, -1},
    { 0,  1, 10,  0, 10,  6,  0,  6,  7,  0,  7,  8,  2,  3, 11, -1},
    { 1, 10,  6,  1,  6,  7,  1,  7, 11,  1, 11,  2, -1, -1, -1, -1},
    { 1,  3, 11,  1, 11,  6,  1,  6,  7,  1,  7,  8,  1,  8,  9, -1},
    { 0,  9,  1,  6,  7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  3, 11,  0, 11,  6,  0,  6,  7,  0,  7,  8, -1, -1, -1, -1},
    { 6,  7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 6, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  6, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  6, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  8,  1,  8,  3,  6, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 1,  2, 10,  6, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  1,  2, 10,  6, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  2, 10,  0, 10,  9,  6, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 2, 10,  9,  2,  9,  8,  2,  8,  3,  6, 11,  7, -1, -1, -1, -1},
    { 2,  3,  7,  2,  7,  6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  7,  0,  7,  6,  0,  6,  2, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  2,  3,  7,  2,  7,  6, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  8,  1,  8,  7,  1,  7,  6,  1,  6,  2, -1, -1, -1, -1},
    { 1,  3,  7,  1,  7,  6,  1,  6, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  7,  0,  7,  6,  0,  6, 10,  0, 10,  1, -1, -1, -1, -1},
    { 0,  3,  7,  0,  7,  6,  0,  6, 10,  0, 10,  9, -1, -1, -1, -1},
    { 6, 10,  9,  6,  9,  8,  6,  8,  7, -1, -1, -1, -1, -1, -1, -1},
    { 4,  6, 11,  4, 11,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  6,  0,  6, 11,  0, 11,  3, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  4,  6, 11,  4, 11,  8, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  4,  1,  4,  6,  1,  6, 11,  1, 11,  3, -1, -1, -1, -1},
    { 1,  2, 10,  4,  6, 11,  4, 11,  8, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  6,  0,  6, 11,  0, 11,  3,  1,  2, 10, -1, -1, -1, -1},
    { 0,  2, 10,  0, 10,  9,  4,  6, 11,  4, 11,  8, -1, -1, -1, -1},
    { 9,  4,  6,  9,  6, 11,  9, 11,  3,  9,  3,  2,  9,  2, 10, -1},
    { 2,  3,  8,  2,  8,  4,  2,  4,  6, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  6,  0,  6,  2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  2,  3,  8,  2,  8,  4,  2,  4,  6, -1, -1, -1, -1},
    { 1,  9,  4,  1,  4,  6,  1,  6,  2, -1, -1, -1, -1, -1, -1, -1},
    { 1,  3,  8,  1,  8,  4,  1,  4,  6,  1,  6, 10, -1, -1, -1, -1},
    { 0,  4,  6,  0,  6, 10,  0, 10,  1, -1, -1, -1, -1, -1, -1, -1},
    { 3,  8,  4,  3,  4,  6,  3,  6, 10,  3, 10,  9,  3,  9,  0, -1},
    { 4,  6, 10,  4, 10,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 4,  9,  5,  6, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  4,  9,  5,  6, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  5,  0,  5,  4,  6, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 1,  5,  4,  1,  4,  8,  1,  8,  3,  6, 11,  7, -1, -1, -1, -1},
    { 1,  2, 10,  4,  9,  5,  6, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  1,  2, 10,  4,  9,  5,  6, 11,  7, -1, -1, -1, -1},
    { 0,  2, 10,  0, 10,  5,  0,  5,  4,  6, 11,  7, -1, -1, -1, -1},
    { 2, 10,  5,  2,  5,  4,  2,  4,  8,  2,  8,  3,  6, 11,  7, -1},
    { 2,  3,  7,  2,  7,  6,  4,  9,  5, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  7,  0,  7,  6,  0,  6,  2,  4,  9,  5, -1, -1, -1, -1},
    { 0,  1,  5,  0,  5,  4,  2,  3,  7,  2,  7,  6, -1, -1, -1, -1},
    { 1,  5,  4,  1,  4,  8,  1,  8,  7,  1,  7,  6,  1,  6,  2, -1},
    { 1,  3,  7,  1,  7,  6,  1,  6, 10,  4,  9,  5, -1, -1, -1, -1},
    { 0,  8,  7,  0,  7,  6,  0,  6, 10,  0, 10,  1,  4,  9,  5, -1},
    { 0,  3,  7,  0,  7,  6,  0,  6, 10,  0, 10,  5,  0,  5,  4, -1},
    { 8,  7,  6,  8,  6, 10,  8, 10,  5,  8,  5,  4, -1, -1, -1, -1},
    { 5,  6, 11,  5, 11,  8,  5,  8,  9, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  5,  0,  5,  6,  0,  6, 11,  0, 11,  3, -1, -1, -1, -1},
    { 0,  1,  5,  0,  5,  6,  0,  6, 11,  0, 11,  8, -1, -1, -1, -1},
    { 1,  5,  6,  1,  6, 11,  1, 11,  3, -1, -1, -1, -1, -1, -1, -1},
    { 1,  2, 10,  5,  6, 11,  5, 11,  8,  5,  8,  9, -1, -1, -1, -1},
    { 0,  9,  5,  0,  5,  6,  0,  6, 11,  0, 11,  3,  1,  2, 10, -1},
    { 0,  2, 10,  0, 10,  5,  0,  5,  6,  0,  6, 11,  0, 11,  8, -1},
    { 5,  6, 11,  5, 11,  3,  5,  3,  2,  5,  2, 10, -1, -1, -1, -1},
    { 2,  3,  8,  2,  8,  9,  2,  9,  5,  2,  5,  6, -1, -1, -1, -1},
    { 0,  9,  5,  0,  5,  6,  0,  6,  2, -1, -1, -1, -1, -1, -1, -1},
    { 5,  6,  2,  5,  2,  3,  5,  3,  8,  5,  8,  0,  5,  0,  1, -1},
    { 1,  5,  6,  1,  6,  2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 3,  8,  9,  3,  9,  5,  3,  5,  6,  3,  6, 10,  3, 10,  1, -1},
    { 0,  9,  5,  0,  5,  6,  0,  6, 10,  0, 10,  1, -1, -1, -1, -1},
    { 0,  3,  8,  5,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 5,  6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 5, 10, 11,  5, 11,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  5, 10, 11,  5, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  5, 10, 11,  5, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 1,  9,  8,  1,  8,  3,  5, 10, 11,  5, 11,  7, -1, -1, -1, -1},
    { 1,  2, 11,  1, 11,  7,  1,  7,  5, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  1,  2, 11,  1, 11,  7,  1,  7,  5, -1, -1, -1, -1},
    { 0,  2, 11,  0, 11,  7,  0,  7,  5,  0,  5,  9, -1, -1, -1, -1},
    { 2, 11,  7,  2,  7,  5,  2,  5,  9,  2,  9,  8,  2,  8,  3, -1},
    { 2,  3,  7,  2,  7,  5,  2,  5, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  7,  0,  7,  5,  0,  5, 10,  0, 10,  2, -1, -1, -1, -1},
    { 0,  1,  9,  2,  3,  7,  2,  7,  5,  2,  5, 10, -1, -1, -1, -1},
    { 8,  7,  5,  8,  5, 10,  8, 10,  2,  8,  2,  1,  8,  1,  9, -1},
    { 1,  3,  7,  1,  7,  5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  7,  0,  7,  5,  0,  5,  1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  3,  7,  0,  7,  5,  0,  5,  9, -1, -1, -1, -1, -1, -1, -1},
    { 5,  9,  8,  5,  8,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 4,  5, 10,  4, 10, 11,  4, 11,  8, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  5,  0,  5, 10,  0, 10, 11,  0, 11,  3, -1, -1, -1, -1},
    { 0,  1,  9,  4,  5, 10,  4, 10, 11,  4, 11,  8, -1, -1, -1, -1},
    { 4,  5, 10,  4, 10, 11,  4, 11,  3,  4,  3,  1,  4,  1,  9, -1},
    { 1,  2, 11,  1, 11,  8,  1,  8,  4,  1,  4,  5, -1, -1, -1, -1},
    { 4,  5,  1,  4,  1,  2,  4,  2, 11,  4, 11,  3,  4,  3,  0, -1},
    { 2, 11,  8,  2,  8,  4,  2,  4,  5,  2,  5,  9,  2,  9,  0, -1},
    { 2, 11,  3,  4,  5,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  3,  8,  2,  8,  4,  2,  4,  5,  2,  5, 10, -1, -1, -1, -1},
    { 0,  4,  5,  0,  5, 10,  0, 10,  2, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1,  9,  2,  3,  8,  2,  8,  4,  2,  4,  5,  2,  5, 10, -1},
    { 4,  5, 10,  4, 10,  2,  4,  2,  1,  4,  1,  9, -1, -1, -1, -1},
    { 1,  3,  8,  1,  8,  4,  1,  4,  5, -1, -1, -1, -1, -1, -1, -1},
    { 0,  4,  5,  0,  5,  1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 3,  8,  4,  3,  4,  5,  3,  5,  9,  3,  9,  0, -1, -1, -1, -1},
    { 4,  5,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 4,  9, 10,  4, 10, 11,  4, 11,  7, -1, -1, -1, -1, -1, -1, -1},
    { 0,  8,  3,  4,  9, 10,  4, 10, 11,  4, 11,  7, -1, -1, -1, -1},
    { 0,  1, 10,  0, 10, 11,  0, 11,  7,  0,  7,  4, -1, -1, -1, -1},
    { 1, 10, 11,  1, 11,  7,  1,  7,  4,  1,  4,  8,  1,  8,  3, -1},
    { 1,  2, 11,  1, 11,  7,  1,  7,  4,  1,  4,  9, -1, -1, -1, -1},
    { 0,  8,  3,  1,  2, 11,  1, 11,  7,  1,  7,  4,  1,  4,  9, -1},
    { 0,  2, 11,  0, 11,  7,  0,  7,  4, -1, -1, -1, -1, -1, -1, -1},
    { 2, 11,  7,  2,  7,  4,  2,  4,  8,  2,  8,  3, -1, -1, -1, -1},
    { 2,  3,  7,  2,  7,  4,  2,  4,  9,  2,  9, 10, -1, -1, -1, -1},
    { 7,  4,  9,  7,  9, 10,  7, 10,  2,  7,  2,  0,  7,  0,  8, -1},
    {10,  2,  3, 10,  3,  7, 10,  7,  4, 10,  4,  0, 10,  0,  1, -1},
    { 1, 10,  2,  4,  8,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  3,  7,  1,  7,  4,  1,  4,  9, -1, -1, -1, -1, -1, -1, -1},
    { 7,  4,  9,  7,  9,  1,  7,  1,  0,  7,  0,  8, -1, -1, -1, -1},
    { 0,  3,  7,  0,  7,  4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 4,  8,  7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 8,  9, 10,  8, 10, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9, 10,  0, 10, 11,  0, 11,  3, -1, -1, -1, -1, -1, -1, -1},
    { 0,  1, 10,  0, 10, 11,  0, 11,  8, -1, -1, -1, -1, -1, -1, -1},
    { 1, 10, 11,  1, 11,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  2, 11,  1, 11,  8,  1,  8,  9, -1, -1, -1, -1, -1, -1, -1},
    { 9,  1,  2,  9,  2, 11,  9, 11,  3,  9,  3,  0, -1, -1, -1, -1},
    { 0,  2, 11,  0, 11,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2, 11,  3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 2,  3,  8,  2,  8,  9,  2,  9, 10, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9, 10,  0, 10,  2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {10,  2,  3, 10,  3,  8, 10,  8,  0, 10,  0,  1, -1, -1, -1, -1},
    { 1, 10,  2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 1,  3,  8,  1,  8,  9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  9,  1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    { 0,  3,  8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
};
__constant__ uint8_t kTriCount[256] = {
    0, 1, 1, 2, 1, 2, 2, 3, 1, 2, 2, 3, 2, 3, 3, 2, 1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 2, 3, 4, 4, 3, 3, 4, 4, 3, 4, 5, 5, 2,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 4, 5, 5, 4,
    2, 3, 3, 4, 3, 4, 2, 3, 3, 4, 4, 5, 4, 5, 3, 2, 3, 4, 4, 3, 4, 5, 3, 2, 4, 5, 5, 4, 5, 2, 4, 1,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 4, 3, 4, 4, 5, 3, 2, 4, 3, 4, 3, 5, 2,
    2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 4, 5, 5, 4, 3, 4, 4, 3, 4, 5, 5, 4, 4, 3, 5, 2, 5, 4, 2, 1,
    2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 2, 3, 3, 2, 3, 4, 4, 5, 4, 5, 5, 2, 4, 3, 5, 4, 3, 2, 4, 1,
    3, 4, 4, 5, 4, 5, 3, 4, 4, 5, 5, 2, 3, 4, 2, 1, 2, 3, 3, 2, 3, 4, 2, 1, 3, 2, 4, 1, 2, 1, 1, 0,
};

struct McLayout {                    // workspace carve-up (gs_mcubes_workspace_bytes)
  uint16_t* rec;                     // per point: owned crossing edges (bits 0-2) | in-workgroup vertex offset << 3
  unsigned long long* blk;           // per workgroup: V | F << 32; after scan_a the exclusive prefix inside its chunk
  unsigned long long* chunk;         // per chunk: V | F << 32 (scan_a)
  unsigned long long* base;          // per chunk: [V base, F base] (scan_b), 64-bit
  size_t bytes;
};

McLayout mc_layout(void* ws, int nx, int ny, int nz) {
  const size_t n = (size_t)nx * ny * nz;
  const size_t nblk = (n + MC_BLOCK - 1) / MC_BLOCK, nch = (nblk + MC_CHUNK - 1) / MC_CHUNK;
  char* b = (char*)ws;
  McLayout L;
  size_t o = 0;
  L.rec = (uint16_t*)(b + o);             o += gs_align(n * 2);
  L.blk = (unsigned long long*)(b + o);   o += gs_align(nblk * 8);
  L.chunk = (unsigned long long*)(b + o); o += gs_align(nch * 8);
  L.base = (unsigned long long*)(b + o);  o += gs_align(nch * 16);
  L.bytes = o;
  return L;
}

// Exclusive prefix over the workgroup (NT threads) and the workgroup total; `lds` holds NT / 64 values.
template <typename T, int NT>
__device__ __forceinline__ T block_exclusive_scan(T v, T* lds, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T s = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(s, off, 64);
    if (lane >= off) s += o;
  }
  if (lane == 63) lds[wave] = s;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const T t = lds[w];
    before += (w < wave) ? t : (T)0;
    all += t;
  }
  __syncthreads();                   // lds may be reused by the caller
  total = all;
  return before + s - v;
}

// A lattice point's crossing edges (+x, +y, +z that exist and cross: bits 0..2) and, when it is the lowest corner of a
// cube, that cube's case (else -1).
__device__ __forceinline__ void mc_point(const float* __restrict__ u, int p, int i, int j, int k, int nx, int ny, int nz,
                                         float level, unsigned& edges, int& cube_case) {
  const int sy = nz, sx = ny * nz;
  const bool hx = i + 1 < nx, hy = j + 1 < ny, hz = k + 1 < nz;
  const bool cube = hx && hy && hz;
  float c[8];                        // every load in flight before the first compare
  c[0] = u[p];
  c[1] = hx ? u[p + sx] : 0.0f;
  c[3] = hy ? u[p + sy] : 0.0f;
  c[4] = hz ? u[p + 1] : 0.0f;
  c[2] = cube ? u[p + sx + sy] : 0.0f;
  c[5] = cube ? u[p + sx + 1] : 0.0f;
  c[6] = cube ? u[p + sx + sy + 1] : 0.0f;
  c[7] = cube ? u[p + sy + 1] : 0.0f;
  unsigned b = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) b |= (c[q] < level ? 1u : 0u) << q;     // NaN is not below
  const unsigned b0 = b & 1u;
  edges = (hx && ((b >> 1) & 1u) != b0 ? 1u : 0u) | (hy && ((b >> 3) & 1u) != b0 ? 2u : 0u) |
          (hz && ((b >> 4) & 1u) != b0 ? 4u : 0u);
  cube_case = cube ? (int)b : -1;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_count_kernel(const float* __restrict__ u, int nx, int ny, int nz,
                                                            float level, uint16_t* __restrict__ rec,
                                                            unsigned long long* __restrict__ blk) {
  __shared__ unsigned lds[MC_BLOCK / 64];
  const int n = nx * ny * nz;
  const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
  unsigned edges = 0;
  int cube_case = -1;
  if (p < n) mc_point(u, p, p / (ny * nz), (p / nz) % ny, p % nz, nx, ny, nz, level, edges, cube_case);
  const unsigned nv = __builtin_popcount(edges), nf = cube_case >= 0 ? kTriCount[cube_case] : 0u;
  unsigned total;
  // V and F packed in one word: a workgroup holds at most 3 * 256 vertices and 5 * 256 faces
  const unsigned ex = block_exclusive_scan<unsigned, MC_BLOCK>(nv | (nf << 16), lds, total);
  if (p < n) rec[p] = (uint16_t)(edges | ((ex & 0xffffu) << 3));
  if (threadIdx.x == 0) blk[blockIdx.x] = (unsigned long long)(total & 0xffffu) | ((unsigned long long)(total >> 16) << 32);
}

// In-chunk exclusive prefix of the workgroup totals (in place) and the chunk totals.  Each half of a packed word stays
// below 2^32 (a chunk holds at most 1024 * 1280 faces), so one 64-bit scan carries both.
__global__ __launch_bounds__(MC_CHUNK) void mc_scan_a_kernel(unsigned long long* __restrict__ blk, int nblk,
                                                             unsigned long long* __restrict__ chunk) {
  __shared__ unsigned long long lds[MC_CHUNK / 64];
  const int b = blockIdx.x * MC_CHUNK + threadIdx.x;
  const unsigned long long v = b < nblk ? blk[b] : 0ull;
  unsigned long long total;
  const unsigned long long ex = block_exclusive_scan<unsigned long long, MC_CHUNK>(v, lds, total);
  if (b < nblk) blk[b] = ex;
  if (threadIdx.x == 0) chunk[blockIdx.x] = total;
}

// One workgroup: 64-bit exclusive prefix of the chunk totals (<= 4096 chunks, four per thread) and the grand totals.
__global__ __launch_bounds__(1024) void mc_scan_b_kernel(const unsigned long long* __restrict__ chunk, int nch,
                                                         unsigned long long* __restrict__ base,
                                                         long long* __restrict__ totals) {
  __shared__ unsigned long long lds[1024 / 64];
  constexpr int PER = MC_MAX_CHUNKS / 1024;
  unsigned long long cv[PER], cf[PER], sv = 0, sf = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int c = threadIdx.x * PER + q;
    const unsigned long long w = c < nch ? chunk[c] : 0ull;
    cv[q] = w & 0xffffffffull;
    cf[q] = w >> 32;
    sv += cv[q];
    sf += cf[q];
  }
  unsigned long long tv, tf;
  unsigned long long ev = block_exclusive_scan<unsigned long long, 1024>(sv, lds, tv);
  unsigned long long ef = block_exclusive_scan<unsigned long long, 1024>(sf, lds, tf);
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int c = threadIdx.x * PER + q;
    if (c < nch) {
      base[2 * c] = ev;
      base[2 * c + 1] = ef;
    }
    ev += cv[q];
    ef += cf[q];
  }
  if (threadIdx.x == 0) {
    totals[0] = (long long)tv;
    totals[1] = (long long)tf;
  }
}

// First vertex of lattice point q: its chunk's base + its workgroup's in-chunk prefix + its in-workgroup offset.
__device__ __forceinline__ long long mc_vertex_base(const McLayout& L, int q, unsigned rec) {
  const int b = q / MC_BLOCK, c = b / MC_CHUNK;
  return (long long)L.base[2 * c] + (long long)(L.blk[b] & 0xffffffffull) + (long long)(rec >> 3);
}

// Vertices, then faces, of the workgroup's points.  Every offset another workgroup contributes was written by an earlier
// launch, so no workgroup waits for another.  Every store is bounded by the caller's n_vertices / n_faces.
__global__ __launch_bounds__(MC_BLOCK) void mc_emit_kernel(const float* __restrict__ u, int nx, int ny, int nz,
                                                           float level, McLayout L, long long n_vertices,
                                                           long long n_faces, float* __restrict__ vertices,
                                                           int* __restrict__ faces) {
  __shared__ unsigned lds[MC_BLOCK / 64];
  const int n = nx * ny * nz;
  const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
  const int i = p / (ny * nz), j = (p / nz) % ny, k = p % nz;
  unsigned edges = 0;
  int cube_case = -1;
  if (p < n) mc_point(u, p, i, j, k, nx, ny, nz, level, edges, cube_case);
  const unsigned nf = cube_case >= 0 ? kTriCount[cube_case] : 0u;
  unsigned total;
  const unsigned fex = block_exclusive_scan<unsigned, MC_BLOCK>(nf, lds, total);
  if (p >= n) return;
  const unsigned my_rec = L.rec[p];
  if (edges) {
    long long v = mc_vertex_base(L, p, my_rec);
    const int a0[3] = {i, j, k};
    const int stride[3] = {ny * nz, nz, 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!((edges >> a) & 1u)) continue;
      const float u0 = u[p], u1 = u[p + stride[a]];
      const float t = (level - u0) / (u1 - u0);
      const float lo = (float)a0[a], hi = (float)(a0[a] + 1);
      float pos[3] = {(float)i, (float)j, (float)k};
      pos[a] = lo + t * (hi - lo);
      if (v < n_vertices) {
        vertices[v * 3 + 0] = pos[0];
        vertices[v * 3 + 1] = pos[1];
        vertices[v * 3 + 2] = pos[2];
      }
      ++v;
    }
  }
  if (nf) {
    const int b = p / MC_BLOCK, c = b / MC_CHUNK;
    long long f = (long long)L.base[2 * c + 1] + (long long)(L.blk[b] >> 32) + (long long)fex;
    const int8_t* tri = kTriTable[cube_case];
    for (int t = 0; t < (int)nf; ++t, ++f) {
      int idx[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int e = tri[3 * t + s];
        const int q = p + kEdgeGeom[e][0] * ny * nz + kEdgeGeom[e][1] * nz + kEdgeGeom[e][2];
        const unsigned axis = (unsigned)kEdgeGeom[e][3];
        const unsigned r = q == p ? my_rec : (unsigned)L.rec[q];
        idx[s] = (int)(mc_vertex_base(L, q, r) + __builtin_popcount(r & ((1u << axis) - 1u)));
      }
      if (f < n_faces) {
        faces[f * 3 + 0] = idx[0];
        faces[f * 3 + 1] = idx[1];
        faces[f * 3 + 2] = idx[2];
      }
    }
  }
}

bool mc_dims_ok(int nx, int ny, int nz) {
  return nx >= 1 && ny >= 1 && nz >= 1 && nx <= 1024 && ny <= 1024 && nz <= 1024;
}

}  // namespace

extern "C" int gs_sdf_lattice(const float* xs, const float* ys, const float* zs, int nx, int ny, int nz,
                              const float* bound, const float* realtime_bound, const void* grid, const float* sdf_w0,
                              const float* sdf_b0, float* u, gs_stream_t stream) {
  GS_REQUIRE(xs && ys && zs && bound && realtime_bound && grid && sdf_w0 && sdf_b0 && u, "sdf_lattice: null pointer");
  GS_REQUIRE(mc_dims_ok(nx, ny, nz), "sdf_lattice: sizes must be in [1, 1024] (got %d x %d x %d)", nx, ny, nz);
  gs_grid_meta m;
  gs_grid_meta_default(&m);
  GS_TIMING_PRE();
  sdf_lattice_kernel<<<gs_cdiv(nx * ny * nz, 256), 256, 0, (hipStream_t)stream>>>(
      xs, ys, zs, nx, ny, nz, bound, realtime_bound, (const _Float16*)grid, sdf_w0, sdf_b0, u, m);
  GS_CHECK_LAUNCH("sdf_lattice");
  return GS_OK;
}

extern "C" size_t gs_mcubes_workspace_bytes(int nx, int ny, int nz) {
  if (!mc_dims_ok(nx, ny, nz)) return 0;
  return mc_layout(nullptr, nx, ny, nz).bytes;
}

extern "C" int gs_mcubes_count(const float* u, int nx, int ny, int nz, float level, void* workspace,
                               size_t workspace_bytes, gs_stream_t stream) {
  GS_REQUIRE(u && workspace, "mcubes_count: null pointer");
  GS_REQUIRE(mc_dims_ok(nx, ny, nz), "mcubes_count: sizes must be in [1, 1024] (got %d x %d x %d)", nx, ny, nz);
  const McLayout L = mc_layout(workspace, nx, ny, nz);
  if (workspace_bytes < L.bytes) {
    gs_set_error("mcubes_count: workspace %zu < %zu bytes", workspace_bytes, L.bytes);
    return GS_ERR_WORKSPACE;
  }
  GS_TIMING_PRE();
  mc_count_kernel<<<gs_cdiv(nx * ny * nz, MC_BLOCK), MC_BLOCK, 0, (hipStream_t)stream>>>(u, nx, ny, nz, level, L.rec,
                                                                                       L.blk);
  GS_CHECK_LAUNCH("mcubes_count");
  return GS_OK;
}

extern "C" int gs_mcubes_scan(int nx, int ny, int nz, void* workspace, size_t workspace_bytes, long long* totals,
                              gs_stream_t stream) {
  GS_REQUIRE(workspace && totals, "mcubes_scan: null pointer");
  GS_REQUIRE(mc_dims_ok(nx, ny, nz), "mcubes_scan: sizes must be in [1, 1024] (got %d x %d x %d)", nx, ny, nz);
  const McLayout L = mc_layout(workspace, nx, ny, nz);
  if (workspace_bytes < L.bytes) {
    gs_set_error("mcubes_scan: workspace %zu < %zu bytes", workspace_bytes, L.bytes);
    return GS_ERR_WORKSPACE;
  }
  const int nblk = gs_cdiv(nx * ny * nz, MC_BLOCK), nch = gs_cdiv(nblk, MC_CHUNK);
  GS_TIMING_PRE();
  mc_scan_a_kernel<<<nch, MC_CHUNK, 0, (hipStream_t)stream>>>(L.blk, nblk, L.chunk);
  GS_CHECK_LAUNCH("mcubes_scan_a");
  mc_scan_b_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(L.chunk, nch, L.base, totals);
  GS_CHECK_LAUNCH("mcubes_scan_b");
  return GS_OK;
}

extern "C" int gs_mcubes_emit(const float* u, int nx, int ny, int nz, float level, const void* workspace,
                              size_t workspace_bytes, long long n_vertices, long long n_faces, float* vertices,
                              int* faces, gs_stream_t stream) {
  GS_REQUIRE(u && workspace, "mcubes_emit: null pointer");
  GS_REQUIRE(mc_dims_ok(nx, ny, nz), "mcubes_emit: sizes must be in [1, 1024] (got %d x %d x %d)", nx, ny, nz);
  GS_REQUIRE(n_vertices >= 0 && n_faces >= 0, "mcubes_emit: negative output size");
  GS_REQUIRE(n_vertices == 0 || vertices, "mcubes_emit: null vertices");
  GS_REQUIRE(n_faces == 0 || faces, "mcubes_emit: null faces");
  if (n_vertices > 2147483647LL || n_faces > 2147483647LL) {
    gs_set_error("mcubes_emit: %lld vertices / %lld faces exceed int32 indexing", n_vertices, n_faces);
    return GS_ERR_UNSUPPORTED;
  }
  const McLayout L = mc_layout(const_cast<void*>(workspace), nx, ny, nz);
  if (workspace_bytes < L.bytes) {
    gs_set_error("mcubes_emit: workspace %zu < %zu bytes", workspace_bytes, L.bytes);
    return GS_ERR_WORKSPACE;
  }
  if (n_vertices == 0 && n_faces == 0) return GS_OK;
  GS_TIMING_PRE();
  mc_emit_kernel<<<gs_cdiv(nx * ny * nz, MC_BLOCK), MC_BLOCK, 0, (hipStream_t)stream>>>(
      u, nx, ny, nz, level, L, n_vertices, n_faces, vertices, faces);
  GS_CHECK_LAUNCH("mcubes_emit");
  return GS_OK;
}
