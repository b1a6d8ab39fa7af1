// One cell of the tiny-cuda-nn HashGrid encoding (3-D input, 2 fp16 features per entry, trilinear interpolation), in the
// pieces every kernel that touches the encoding composes in its own order: the cell of a level, the corner indices, the
// corner gather, the trilinear weights, the value, and the corner enumerations of the first and the mixed second derivative.
// The arithmetic of each piece -- product order, fmaf chain, where nothing is rounded to fp16 -- is the contract: the
// forward, the lattice, the fused backward and the autograd kernels agree bit for bit because they call the same piece.
#pragma once
#include "common.h"
#include "../../include/goslam_neus.h"

namespace {

__device__ __forceinline__ uint32_t grid_index(const gs_grid_meta& m, int l, uint32_t cx, uint32_t cy, uint32_t cz) {
  const uint32_t size = m.size[l];
  uint32_t idx;
  if (m.hashed[l]) {
    idx = (cx * 1u) ^ (cy * 2654435761u) ^ (cz * 805459861u);
  } else {
    const uint32_t res = m.resolution[l];
    idx = cx + cy * res + cz * res * res;
  }
  // tcnn: `index % hashmap_size`.  A hashed level holds 2^19 entries (a mask), and a dense level's index is below its
  // size except at the far corner of the box -- the generic 32-bit modulo (~30 VALU instructions, 8 per level and
  // point, a third of a level's arithmetic) only runs when it has to.  Same result in every case.
  if ((size & (size - 1u)) == 0u) return idx & (size - 1u);
  return idx < size ? idx : idx % size;
}

// The 8 corner indices of one cell, corner c = (c & 1, (c >> 1) & 1, (c >> 2) & 1) -- the same values as eight
// grid_index calls (uint32 arithmetic is a ring: (cy + 1) * P == cy * P + P), with the level's kind decided ONCE instead of
// inside every corner: a hashed level costs 2 multiplications + 2 additions + 12 xors + 8 masks instead of 16
// multiplications (v_mul_lo_u32 is a quarter-rate instruction) + 16 xors + 8 masks + 12 corner additions and five uniform
// branches per corner; a dense level is the base index plus the uniform strides 1 / res / res^2.
__device__ __forceinline__ void grid_corners(const gs_grid_meta& m, int l, const uint32_t (&g)[3], uint32_t (&cidx)[8]) {
  const uint32_t size = m.size[l];
  if (m.hashed[l]) {
    const uint32_t y0 = g[1] * 2654435761u, y1 = y0 + 2654435761u;
    const uint32_t z0 = g[2] * 805459861u, z1 = z0 + 805459861u;
    const uint32_t x0 = g[0], x1 = g[0] + 1u;
    const uint32_t yz[4] = {y0 ^ z0, y1 ^ z0, y0 ^ z1, y1 ^ z1};
#pragma unroll
    for (int c = 0; c < 8; ++c) cidx[c] = ((c & 1) ? x1 : x0) ^ yz[c >> 1];
  } else {
    const uint32_t res = m.resolution[l], res2 = res * res;
    const uint32_t base = g[0] + g[1] * res + g[2] * res2;
#pragma unroll
    for (int c = 0; c < 8; ++c) cidx[c] = base + (uint32_t)(c & 1) + (((c >> 1) & 1) ? res : 0u) + (((c >> 2) & 1) ? res2 : 0u);
  }
  // tcnn: `index % hashmap_size` (see grid_index)
  if ((size & (size - 1u)) == 0u) {
#pragma unroll
    for (int c = 0; c < 8; ++c) cidx[c] &= size - 1u;
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) cidx[c] = cidx[c] < size ? cidx[c] : cidx[c] % size;
  }
}

// The cell of level l that holds x (the grid's [0, 1] input): integer corner gi, fraction f; returns the level's scale.
__device__ __forceinline__ float grid_cell(const gs_grid_meta& m, int l, const float x[3], uint32_t (&gi)[3], float (&f)[3]) {
  const float scale = m.scale[l];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float pos = fmaf(scale, x[d], 0.5f);
    const float fl = floorf(pos);
    gi[d] = (uint32_t)(int)fl;
    f[d] = pos - fl;
  }
  return scale;
}

// The 8 corner entries of a cell, `tab` = the level's first entry: one 4-byte load per corner (both fp16 features); the
// loads are independent, so the compiler issues all 8 before the first is unpacked.
__device__ __forceinline__ void grid_gather(const _Float16* __restrict__ tab, const uint32_t (&cidx)[8], float (&v)[8][2]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint32_t raw = *reinterpret_cast<const uint32_t*>(tab + (size_t)cidx[c] * 2);
    v[c][0] = (float)__builtin_bit_cast(_Float16, (uint16_t)(raw & 0xffffu));
    v[c][1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(raw >> 16));
  }
}

// cell, corner indices and corner values of level l at x in one call (the sites that gather at once); returns the scale
__device__ __forceinline__ float grid_cell_gather(const gs_grid_meta& m, int l, const _Float16* __restrict__ grid,
                                                  const float x[3], uint32_t (&gi)[3], float (&f)[3], uint32_t (&cidx)[8],
                                                  float (&v)[8][2]) {
  const float scale = grid_cell(m, l, x, gi, f);
  const _Float16* tab = grid + (size_t)m.offset[l] * 2;
  grid_corners(m, l, gi, cidx);
  grid_gather(tab, cidx, v);
  return scale;
}

// trilinear corner weights, tcnn's product order
__device__ __forceinline__ void grid_weights(const float (&f)[3], float (&wc)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float w = 1.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) w = w * (((c >> d) & 1) ? f[d] : (1.0f - f[d]));
    wc[c] = w;
  }
}

// the interpolated features (fp32: the caller rounds to fp16 where tcnn's output type applies), tcnn's accumulation order
__device__ __forceinline__ void grid_value(const float (&wc)[8], const float (&v)[8][2], float (&val)[2]) {
  val[0] = 0.f; val[1] = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    val[0] = fmaf(wc[c], v[c][0], val[0]);
    val[1] = fmaf(wc[c], v[c][1], val[1]);
  }
}

// First derivative along axis gd: term k (0..3) runs over the two other axes (ascending, k's bit 0 the lower one); its
// weight is scale * (f or 1 - f)[o0] * (f or 1 - f)[o1] and it differences the corner pair (cl, cr) along gd.  Needs no
// corner values, so the fused backward uses the same terms for its second-order scatter.
struct GridD1 { float w; int cl, cr; };
__device__ __forceinline__ GridD1 grid_d1(float scale, const float (&f)[3], int gd, int k) {
  const int o0 = (gd == 0) ? 1 : 0, o1 = (gd == 2) ? 1 : 2;
  GridD1 t;
  t.w = scale;
  t.w = t.w * ((k & 1) ? f[o0] : (1.0f - f[o0]));
  t.w = t.w * ((k & 2) ? f[o1] : (1.0f - f[o1]));
  t.cl = ((k & 1) << o0) | (((k >> 1) & 1) << o1);
  t.cr = t.cl | (1 << gd);
  return t;
}

// d value / d x (3 x 2), tcnn accumulation order
__device__ __forceinline__ void grid_dvalue(float scale, const float (&f)[3], const float (&v)[8][2], float (&dv)[3][2]) {
#pragma unroll
  for (int gd = 0; gd < 3; ++gd) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const GridD1 t = grid_d1(scale, f, gd, k);
      a0 = fmaf(t.w, v[t.cr][0] - v[t.cl][0], a0);
      a1 = fmaf(t.w, v[t.cr][1] - v[t.cl][1], a1);
    }
    dv[gd][0] = a0;
    dv[gd][1] = a1;
  }
}

// The forward of one level: value (2 features) and, if wanted, d value / d x (3 x 2).
__device__ __forceinline__ void grid_encode_level(const gs_grid_meta& m, int l, const _Float16* __restrict__ grid,
                                                  const float x[3], float (&val)[2], float (&dv)[3][2], bool want_grad) {
  uint32_t gi[3], cidx[8];
  float f[3], v[8][2], wc[8];
  const float scale = grid_cell_gather(m, l, grid, x, gi, f, cidx, v);
  grid_weights(f, wc);
  grid_value(wc, v, val);
  if (want_grad) grid_dvalue(scale, f, v, dv);
}

// Mixed second derivative along axes a < b: term k (0, 1) sits at bit k of the third axis t, carries the weight
// (k ? f[t] : 1 - f[t]) and combines v[c11] - v[c10] - v[c01] + v[c00].  Indices only: the two users round that
// four-term sum differently (neus_bwd.hip, grid_autograd.hip) and each keeps its own form.
struct GridD2 { int c11, c10, c01, c00, t; };
__device__ __forceinline__ GridD2 grid_d2(int a, int b, int k) {
  GridD2 q;
  q.t = 3 - a - b;
  q.c00 = k << q.t;
  q.c10 = q.c00 | (1 << a);
  q.c01 = q.c00 | (1 << b);
  q.c11 = q.c10 | (1 << b);
  return q;
}

}  // namespace
