// Two TSDF lattices of tsdf.hip put together: where does volume S sit in volume D, and S fused into D.  (No counterpart
// in the reference.)  Contract: include/goslam_hip.h (gs_tsdf_register_workspace_bytes, gs_tsdf_register_system,
// gs_tsdf_merge); tests/tsdf_merge_restatement.py restates the three with one rounding per operation and the summation
// order written out.  Compiled with -ffp-contract=off.
//
// tsdf_register_system_kernel: tsdf_align.hip's system kernel with lattice points of S in the place of pixels.  One
// workgroup of 256 threads per (pose, chunk of gs_tsdf_align_chunk() strided lattice points of S); a lane walks its
// samples t, t + 256, ... of the chunk.  A wave's 64 samples are neighbours along S's z axis (stride apart), so the two
// loads of S share cache lines and the sixteen corner loads of D fall into neighbouring cells.  As there, the contract's
// early-outs are one predicate (a skipped sample reads D's cell 0 and drops it), the 29 fp64 sums live in registers, the
// chunk ends with gs_wave_sum_f64 per value and the four waves' totals through 1 KiB of LDS as ((w0 + w1) + w2) + w3.
// tsdf_register_sum_kernel adds the chunks' totals in increasing order, sixteen loads in flight.  No atomics.  The rows
// have gs_tsdf_align_system's layout and feed gs_tsdf_align_step unchanged.  The gather is written out here a second
// time on purpose: tsdf_align.hip's kernels stay the code they were.
//   gfx950, -O3: tsdf_register_system_kernel 128 VGPRs, no scratch, 1 KiB LDS: 4 waves per SIMD (amdgpu_waves_per_eu
//   4, 4; the 29 fp64 accumulators are 58 of them); tsdf_register_sum_kernel 38 VGPRs, no scratch, no LDS.
//
// tsdf_merge_kernel: one lane per lattice point of D, the 64 lanes of a wave along z (D's loads and stores are 256 B
// runs), the four waves of a workgroup on four neighbouring y: a tile of 1 x 4 x 64 points.  The transform D-world ->
// S-world and both lattices are by-value kernel arguments (SGPRs).  Before any load a workgroup maps its tile's eight
// corners into S's index space: a rigid map sends the tile into the hull of the eight images, so when all eight lie
// below 0 or at or beyond n_S - 1 on one axis -- by a margin of half a cell plus 2^-10 of the magnitudes involved, a
// thousand times the per-point fp32 rounding -- no point of the tile has a cell in S, and the workgroup leaves without
// a load (tsdf_common.h's frustum skip, for a box).  A lane that passes gathers the cell's eight weights, and only a
// cell seen at all eight corners loads its eight tsdf values (and 24 colours): 8 to 40 gathers of S per point against
// 2 to 5 streamed loads and stores of D, which is where the time goes.  Every point is owned by one lane: no LDS, no
// atomics, and the result does not depend on the launch geometry.
//   gfx950, -O3: tsdf_merge_kernel<true> 58 VGPRs, <false> 50 VGPRs, no scratch, no LDS: 8 waves per SIMD.
#include "common.h"

namespace {

constexpr int REG_THREADS = 256;
constexpr int REG_WAVES = REG_THREADS / GS_WAVE;
constexpr int REG_ROW = 32;                 // doubles per row of out and of a chunk's partial: gs_tsdf_align_system's
constexpr int REG_SUMS = 29;                // H 21, b 6, cost, sq
constexpr int REG_SUM_BATCH = 16;           // chunk totals the sum kernel loads before it adds them
constexpr int MERGE_THREADS = 256;
constexpr int MERGE_TILE_Y = MERGE_THREADS / GS_WAVE;

struct Lattice {           // by-value kernel argument (SGPRs)
  int ny, nz;
  float topx, topy, topz;  // float(n - 1)
  float lox, loy, loz, voxel;
};

struct RegisterArgs {      // by-value kernel argument (SGPRs)
  const float* tsdf_d;
  const float* weight_d;
  const float* tsdf_s;
  const float* weight_s;
  const double* pose;      // [B,3,4], S-world to D-world
  double* partial;         // [B,n_chunks,32]
  Lattice d, s;
  int stride, chunk;
  int sny, snz;            // strided lattice points of S along y and z
  int n_samples, n_chunks;
  float ratio;             // trunc_S / trunc_D
  float min_weight, huber;
};

__device__ __forceinline__ float merge_lerp(float p, float q, float s) { return p + s * (q - p); }

struct Corners { float v000, v001, v010, v011, v100, v101, v110, v111; };   // v[x][y][z]

// 32-bit offsets: the largest lattice has 2^30 points
__device__ __forceinline__ Corners corners_load(const float* __restrict__ p, unsigned at, int ny, int nz) {
  const unsigned sy = (unsigned)nz, sx = (unsigned)ny * (unsigned)nz;
  Corners c;
  c.v000 = p[at];           c.v001 = p[at + 1];
  c.v010 = p[at + sy];      c.v011 = p[at + sy + 1];
  c.v100 = p[at + sx];      c.v101 = p[at + sx + 1];
  c.v110 = p[at + sx + sy]; c.v111 = p[at + sx + sy + 1];
  return c;
}

__device__ __forceinline__ bool corners_at_least(const Corners& c, float m) {
  return c.v000 >= m && c.v001 >= m && c.v010 >= m && c.v011 >= m && c.v100 >= m && c.v101 >= m && c.v110 >= m && c.v111 >= m;
}

// the value by lerps z, y, x: gs_tsdf_raycast's sequence
__device__ __forceinline__ float corners_value(const Corners& c, float sx, float sy, float sz) {
  const float z00 = merge_lerp(c.v000, c.v001, sz), z01 = merge_lerp(c.v010, c.v011, sz);
  const float z10 = merge_lerp(c.v100, c.v101, sz), z11 = merge_lerp(c.v110, c.v111, sz);
  return merge_lerp(merge_lerp(z00, z01, sy), merge_lerp(z10, z11, sy), sx);
}

// four waves per SIMD: at most 128 VGPRs (tests/test_tsdf_merge_cpu.py holds the budget)
__global__ __launch_bounds__(REG_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
void tsdf_register_system_kernel(const RegisterArgs a) {
  __shared__ double part[REG_WAVES][REG_ROW];
  const int b = blockIdx.x / a.n_chunks;
  const int chunk = blockIdx.x - b * a.n_chunks;

  double acc[REG_SUMS];
#pragma unroll
  for (int i = 0; i < REG_SUMS; ++i) acc[i] = 0.0;
  int count = 0, considered = 0;

  {
    const double* __restrict__ m = a.pose + (size_t)b * 12;
    // (float) of the fp64 pose; the conversion is a vector instruction, so the uniform results are moved back to SGPRs
    float pm[12];
#pragma unroll
    for (int i = 0; i < 12; ++i)
      pm[i] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, (float)m[i])));
    const float r00 = pm[0], r01 = pm[1], r02 = pm[2], ox = pm[3];
    const float r10 = pm[4], r11 = pm[5], r12 = pm[6], oy = pm[7];
    const float r20 = pm[8], r21 = pm[9], r22 = pm[10], oz = pm[11];
    const int syz = a.sny * a.snz;
    const int s_end = min((chunk + 1) * a.chunk, a.n_samples);
#pragma nounroll
    for (int s = chunk * a.chunk + (int)threadIdx.x; s < s_end; s += REG_THREADS) {
      const int si = s / syz, rem = s - si * syz;
      const int sj = rem / a.snz, sk = rem - sj * a.snz;
      const int ii = si * a.stride, jj = sj * a.stride, kk = sk * a.stride;
      const unsigned at_s = ((unsigned)ii * a.s.ny + (unsigned)jj) * a.s.nz + (unsigned)kk;
      const float ws = a.weight_s[at_s], fs = a.tsdf_s[at_s];
      const float fr = fs * a.ratio;                           // the source's value in units of D's truncation
      bool valid = ws >= a.min_weight && fabsf(fs) < 1.0f && fabsf(fr) < 1.0f;
      if (valid) ++considered;
      const float px = a.s.lox + (float)ii * a.s.voxel, py = a.s.loy + (float)jj * a.s.voxel, pz = a.s.loz + (float)kk * a.s.voxel;
      const float qx = (r00 * px + r01 * py) + r02 * pz;
      const float qy = (r10 * px + r11 * py) + r12 * pz;
      const float qz = (r20 * px + r21 * py) + r22 * pz;
      const float gx = ((qx + ox) - a.d.lox) / a.d.voxel, gy = ((qy + oy) - a.d.loy) / a.d.voxel, gz = ((qz + oz) - a.d.loz) / a.d.voxel;
      const float ax = floorf(gx), ay = floorf(gy), az = floorf(gz);
      valid = valid && ax >= 0.0f && ax < a.d.topx && ay >= 0.0f && ay < a.d.topy && az >= 0.0f && az < a.d.topz;
      // a skipped sample reads D's cell 0 and drops what it read: sixteen loads in flight per lane instead of a branch each
      const unsigned at = valid ? ((unsigned)(int)ax * a.d.ny + (unsigned)(int)ay) * a.d.nz + (unsigned)(int)az : 0u;
      const Corners wc = corners_load(a.weight_d, at, a.d.ny, a.d.nz);
      const Corners c = corners_load(a.tsdf_d, at, a.d.ny, a.d.nz);
      valid = valid && corners_at_least(wc, a.min_weight);
      const float sx = gx - ax, sy = gy - ay, sz = gz - az;
      // gs_tsdf_align_system's sequences: the value by lerps z, y, x; the gradient from the z-lerps and the y-lerps
      const float z00 = merge_lerp(c.v000, c.v001, sz), z01 = merge_lerp(c.v010, c.v011, sz);
      const float z10 = merge_lerp(c.v100, c.v101, sz), z11 = merge_lerp(c.v110, c.v111, sz);
      const float x0 = merge_lerp(z00, z01, sy), x1 = merge_lerp(z10, z11, sy);
      const float f = merge_lerp(x0, x1, sx);
      valid = valid && fabsf(f) < 1.0f;
      if (!valid) continue;
      const float y00 = merge_lerp(c.v000, c.v010, sy), y01 = merge_lerp(c.v001, c.v011, sy);
      const float y10 = merge_lerp(c.v100, c.v110, sy), y11 = merge_lerp(c.v101, c.v111, sy);
      const float nx = x1 - x0;
      const float ny = merge_lerp(z01, z11, sx) - merge_lerp(z00, z10, sx);
      const float nz = merge_lerp(y01, y11, sx) - merge_lerp(y00, y10, sx);
      const float wx = nx / a.d.voxel, wy = ny / a.d.voxel, wz = nz / a.d.voxel;
      float J[6];
      J[0] = wx; J[1] = wy; J[2] = wz;
      J[3] = qy * wz - qz * wy;
      J[4] = qz * wx - qx * wz;
      J[5] = qx * wy - qy * wx;
      const float r = f - fr;
      const float ar = fabsf(r);
      const float wt = ar <= a.huber ? 1.0f : a.huber / ar;
      const double rd = (double)r, wd = (double)wt;
      int at_h = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double wj = wd * (double)J[i];
#pragma unroll
        for (int j = i; j < 6; ++j) {
          acc[at_h] += wj * (double)J[j];
          ++at_h;
        }
        acc[21 + i] += wj * rd;
      }
      acc[27] += (wd * rd) * rd;
      acc[28] += rd * rd;
      ++count;
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < REG_SUMS; ++i) {
    const double v = gs_wave_sum_f64(acc[i]);
    if (lane == 0) part[wave][i == 28 ? 29 : i] = v;         // a row is H, b, cost, count, sq, considered, 0
    __builtin_amdgcn_sched_barrier(0);                       // one value's exchanges at a time: they need no more registers
  }
  {
    const int cn = gs_wave_sum_i32(count), cs = gs_wave_sum_i32(considered);     // integers: any order gives the sum
    if (lane == 0) {
      part[wave][28] = (double)cn;
      part[wave][30] = (double)cs;
      part[wave][31] = 0.0;
    }
  }
  __syncthreads();
  if (threadIdx.x < REG_ROW) {
    const int i = threadIdx.x;
    a.partial[((size_t)b * a.n_chunks + chunk) * REG_ROW + i] = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i];
  }
}

__global__ __launch_bounds__(GS_WAVE) void tsdf_register_sum_kernel(const double* __restrict__ partial, int n_chunks,
                                                                    double* __restrict__ out) {
  const int i = threadIdx.x;
  if (i >= REG_ROW) return;
  const double* __restrict__ p = partial + (size_t)blockIdx.x * n_chunks * REG_ROW + i;
  double t = p[0];
  int c = 1;
  for (; c + REG_SUM_BATCH <= n_chunks; c += REG_SUM_BATCH) {       // the loads of a batch in flight together, the adds in order
    double v[REG_SUM_BATCH];
#pragma unroll
    for (int j = 0; j < REG_SUM_BATCH; ++j) v[j] = p[(size_t)(c + j) * REG_ROW];
#pragma unroll
    for (int j = 0; j < REG_SUM_BATCH; ++j) t = t + v[j];
  }
  for (; c < n_chunks; ++c) t = t + p[(size_t)c * REG_ROW];
  out[(size_t)blockIdx.x * REG_ROW + i] = t;
}

struct MergeArgs {         // by-value kernel argument (SGPRs)
  float* tsdf_d;
  float* weight_d;
  float* colors_d;         // [3,nx,ny,nz]; touched only by the COLOR kernel
  const float* tsdf_s;
  const float* weight_s;
  const float* colors_s;
  Lattice d, s;
  int nx_d;
  unsigned np_d, np_s;     // points per lattice: the stride of a colour plane
  float m[12];             // D-world to S-world, rows (r0 r1 r2 t)
  float ratio;             // trunc_S / trunc_D >= 1
  float min_weight, max_weight;
};

// One corner of the tile in S's index space, folded into the running extremes of the three axes.
__device__ __forceinline__ void merge_corner(const MergeArgs& a, float px, float py, float pz, float* lo, float* hi) {
  const float* m = a.m;
  const float x = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
  const float y = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
  const float z = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
  const float g[3] = {(x - a.s.lox) / a.s.voxel, (y - a.s.loy) / a.s.voxel, (z - a.s.loz) / a.s.voxel};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    // a NaN would fail every comparison below and skip a tile it says nothing about: it counts as "may hit"
    lo[k] = g[k] == g[k] ? fminf(lo[k], g[k]) : -INFINITY;
    hi[k] = g[k] == g[k] ? fmaxf(hi[k], g[k]) : INFINITY;
  }
}

// Can any point of the tile i, [j0, j0 + 3], [k0, k0 + 63] of D have a cell in S?  A point passes the kernel's own test
// when 0 <= floorf(g) < n_S - 1, i.e. 0 <= g < n_S - 1, on every axis.  g is an affine function of the point, so over
// the tile (a box) it lies between the smallest and the largest of the eight corners' values.  "Outside" is taken with
// a margin rr in cells: half a cell plus 2^-10 of the magnitudes that enter g, in cells.  The per-point fp32 arithmetic
// (a dozen roundings of relative size 2^-24) moves g by about 2^-20 of them, a thousand times less.  So "false" is only
// returned when every point of the tile fails its own test.
__device__ __forceinline__ bool merge_tile_may_hit(const MergeArgs& a, int i, int j0, int k0) {
  const float x0 = a.d.lox + (float)i * a.d.voxel;
  const float y0 = a.d.loy + (float)j0 * a.d.voxel, y1 = a.d.loy + (float)(j0 + MERGE_TILE_Y - 1) * a.d.voxel;
  const float z0 = a.d.loz + (float)k0 * a.d.voxel, z1 = a.d.loz + (float)(k0 + GS_WAVE - 1) * a.d.voxel;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  merge_corner(a, x0, y0, z0, lo, hi); merge_corner(a, x0, y0, z1, lo, hi);
  merge_corner(a, x0, y1, z0, lo, hi); merge_corner(a, x0, y1, z1, lo, hi);
  const float mag = ((fabsf(a.m[3]) + fabsf(a.m[7])) + (fabsf(a.m[11]) + fabsf(x0))) +
                    ((fmaxf(fabsf(y0), fabsf(y1)) + fmaxf(fabsf(z0), fabsf(z1))) +
                     ((fabsf(a.s.lox) + fabsf(a.s.loy)) + (fabsf(a.s.loz) + 1.0f)));
  const float rr = 0.5f + 0.0009765625f * (mag / a.s.voxel);
  const float top[3] = {a.s.topx, a.s.topy, a.s.topz};
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (hi[k] < -rr || lo[k] > top[k] + rr) return false;
  return true;
}

template <bool COLOR>
__global__ __launch_bounds__(MERGE_THREADS) void tsdf_merge_kernel(const MergeArgs a) {
  // the tile: x = blockIdx.z, four y from blockIdx.y * 4 (one per wave), 64 z from blockIdx.x * 64 (one per lane); the
  // tile has one x, so its box has four distinct corners
  const int i = blockIdx.z, j0 = blockIdx.y * MERGE_TILE_Y, k0 = blockIdx.x * GS_WAVE;
  if (!merge_tile_may_hit(a, i, j0, k0)) return;
  const int j = j0 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int k = k0 + (int)(threadIdx.x & 63);
  if (j >= a.d.ny || k >= a.d.nz) return;

  const float px = a.d.lox + (float)i * a.d.voxel, py = a.d.loy + (float)j * a.d.voxel, pz = a.d.loz + (float)k * a.d.voxel;
  const float* m = a.m;
  const float x = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
  const float y = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
  const float z = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
  const float gx = (x - a.s.lox) / a.s.voxel, gy = (y - a.s.loy) / a.s.voxel, gz = (z - a.s.loz) / a.s.voxel;
  const float ax = floorf(gx), ay = floorf(gy), az = floorf(gz);
  if (!(ax >= 0.0f && ax < a.s.topx && ay >= 0.0f && ay < a.s.topy && az >= 0.0f && az < a.s.topz)) return;   // a NaN fails
  const unsigned at_s = ((unsigned)(int)ax * a.s.ny + (unsigned)(int)ay) * a.s.nz + (unsigned)(int)az;
  const Corners wc = corners_load(a.weight_s, at_s, a.s.ny, a.s.nz);
  if (!corners_at_least(wc, a.min_weight)) return;
  const float sx = gx - ax, sy = gy - ay, sz = gz - az;
  const float fs = corners_value(corners_load(a.tsdf_s, at_s, a.s.ny, a.s.nz), sx, sy, sz);
  const float ws = corners_value(wc, sx, sy, sz);
  float s = fs * a.ratio;
  if (s < -1.0f) return;
  s = fminf(1.0f, s);

  const unsigned at = ((unsigned)i * a.d.ny + (unsigned)j) * a.d.nz + (unsigned)k;
  const float w0 = a.weight_d[at];
  const float w1 = w0 + ws;
  a.tsdf_d[at] = (a.tsdf_d[at] * w0 + s * ws) / w1;
  if (COLOR) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float cs = corners_value(corners_load(a.colors_s + (size_t)ch * a.np_s, at_s, a.s.ny, a.s.nz), sx, sy, sz);
      float* __restrict__ cd = a.colors_d + (size_t)ch * a.np_d;
      cd[at] = (cd[at] * w0 + cs * ws) / w1;
    }
  }
  a.weight_d[at] = fminf(w1, a.max_weight);
}

bool merge_dims_ok(int nx, int ny, int nz) {
  return nx >= 2 && nx <= 1024 && ny >= 2 && ny <= 1024 && nz >= 2 && nz <= 1024;
}

bool merge_finite(float v) { return fabsf(v) < INFINITY; }

// strided lattice points of an nx x ny x nz lattice, or -1 for sizes the entry points refuse
long long register_samples(int nx, int ny, int nz, int stride) {
  if (!merge_dims_ok(nx, ny, nz) || stride < 1) return -1;
  return (long long)gs_cdiv(nx, stride) * gs_cdiv(ny, stride) * gs_cdiv(nz, stride);
}

Lattice merge_lattice(int nx, int ny, int nz, float lo_x, float lo_y, float lo_z, float voxel) {
  Lattice l;
  l.ny = ny; l.nz = nz;
  l.topx = (float)(nx - 1); l.topy = (float)(ny - 1); l.topz = (float)(nz - 1);
  l.lox = lo_x; l.loy = lo_y; l.loz = lo_z; l.voxel = voxel;
  return l;
}

}  // namespace

extern "C" int gs_tsdf_align_chunk(void);

extern "C" size_t gs_tsdf_register_workspace_bytes(int n_poses, int nx_s, int ny_s, int nz_s, int stride) {
  const long long n = register_samples(nx_s, ny_s, nz_s, stride);
  if (n_poses < 0 || n < 0) return 0;
  const long long c = gs_tsdf_align_chunk();
  const long long chunks = (n + c - 1) / c;
  if ((long long)n_poses * chunks > 0x7fffffffLL) return 0;
  return (size_t)n_poses * (size_t)chunks * REG_ROW * sizeof(double);
}

extern "C" int gs_tsdf_register_system(const float* tsdf_d, const float* weight_d, int nx_d, int ny_d, int nz_d,
                                       float lo_dx, float lo_dy, float lo_dz, float voxel_d, float trunc_d,
                                       const float* tsdf_s, const float* weight_s, int nx_s, int ny_s, int nz_s,
                                       float lo_sx, float lo_sy, float lo_sz, float voxel_s, float trunc_s,
                                       const double* pose, int n_poses, int stride, float min_weight, float huber,
                                       void* workspace, double* out, gs_stream_t stream) {
  GS_REQUIRE(merge_dims_ok(nx_d, ny_d, nz_d), "tsdf_register_system: destination lattice %d x %d x %d outside [2, 1024]", nx_d,
             ny_d, nz_d);
  GS_REQUIRE(merge_dims_ok(nx_s, ny_s, nz_s), "tsdf_register_system: source lattice %d x %d x %d outside [2, 1024]", nx_s,
             ny_s, nz_s);
  const long long n = register_samples(nx_s, ny_s, nz_s, stride);
  GS_REQUIRE(n_poses >= 0 && n >= 0, "tsdf_register_system: n_poses=%d stride=%d", n_poses, stride);
  GS_REQUIRE(voxel_d > 0.0f && voxel_d < INFINITY && voxel_s > 0.0f && voxel_s < INFINITY,
             "tsdf_register_system: voxel_d=%g voxel_s=%g", voxel_d, voxel_s);
  GS_REQUIRE(trunc_d > 0.0f && trunc_d < INFINITY && trunc_s > 0.0f && trunc_s < INFINITY,
             "tsdf_register_system: trunc_d=%g trunc_s=%g", trunc_d, trunc_s);
  GS_REQUIRE(merge_finite(lo_dx) && merge_finite(lo_dy) && merge_finite(lo_dz) && merge_finite(lo_sx) && merge_finite(lo_sy) &&
                 merge_finite(lo_sz),
             "tsdf_register_system: lo_d=(%g, %g, %g) lo_s=(%g, %g, %g)", lo_dx, lo_dy, lo_dz, lo_sx, lo_sy, lo_sz);
  GS_REQUIRE(huber > 0.0f, "tsdf_register_system: huber=%g (need > 0)", huber);
  GS_REQUIRE(min_weight == min_weight, "tsdf_register_system: min_weight is NaN");
  if (n_poses == 0) return GS_OK;
  const int chunk = gs_tsdf_align_chunk();
  const long long chunks = (n + chunk - 1) / chunk;
  GS_REQUIRE((long long)n_poses * chunks <= 0x7fffffffLL,
             "tsdf_register_system: %d poses of %lld chunks are too many for one launch", n_poses, chunks);
  GS_REQUIRE(tsdf_d && weight_d && tsdf_s && weight_s && pose && workspace && out, "tsdf_register_system: null pointer");
  RegisterArgs a;
  a.tsdf_d = tsdf_d; a.weight_d = weight_d; a.tsdf_s = tsdf_s; a.weight_s = weight_s;
  a.pose = pose; a.partial = (double*)workspace;
  a.d = merge_lattice(nx_d, ny_d, nz_d, lo_dx, lo_dy, lo_dz, voxel_d);
  a.s = merge_lattice(nx_s, ny_s, nz_s, lo_sx, lo_sy, lo_sz, voxel_s);
  a.stride = stride; a.chunk = chunk;
  a.sny = gs_cdiv(ny_s, stride); a.snz = gs_cdiv(nz_s, stride);
  a.n_samples = (int)n; a.n_chunks = (int)chunks;
  a.ratio = trunc_s / trunc_d;
  a.min_weight = min_weight; a.huber = huber;
  GS_TIMING_PRE();
  tsdf_register_system_kernel<<<(unsigned)(n_poses * chunks), REG_THREADS, 0, (hipStream_t)stream>>>(a);
  GS_CHECK_LAUNCH("tsdf_register_system");
  tsdf_register_sum_kernel<<<(unsigned)n_poses, GS_WAVE, 0, (hipStream_t)stream>>>(a.partial, a.n_chunks, out);
  GS_CHECK_LAUNCH("tsdf_register_sum");
  return GS_OK;
}

extern "C" int gs_tsdf_merge(float* tsdf_d, float* weight_d, float* colors_d, int nx_d, int ny_d, int nz_d, float lo_dx,
                             float lo_dy, float lo_dz, float voxel_d, float trunc_d, float max_weight, const float* tsdf_s,
                             const float* weight_s, const float* colors_s, int nx_s, int ny_s, int nz_s, float lo_sx,
                             float lo_sy, float lo_sz, float voxel_s, float trunc_s, const float* d2s, float min_weight,
                             gs_stream_t stream) {
  GS_REQUIRE(merge_dims_ok(nx_d, ny_d, nz_d), "tsdf_merge: destination lattice %d x %d x %d outside [2, 1024]", nx_d, ny_d, nz_d);
  GS_REQUIRE(merge_dims_ok(nx_s, ny_s, nz_s), "tsdf_merge: source lattice %d x %d x %d outside [2, 1024]", nx_s, ny_s, nz_s);
  GS_REQUIRE(voxel_d > 0.0f && voxel_d < INFINITY && voxel_s > 0.0f && voxel_s < INFINITY, "tsdf_merge: voxel_d=%g voxel_s=%g",
             voxel_d, voxel_s);
  GS_REQUIRE(trunc_d > 0.0f && trunc_d < INFINITY && trunc_s > 0.0f && trunc_s < INFINITY, "tsdf_merge: trunc_d=%g trunc_s=%g",
             trunc_d, trunc_s);
  GS_REQUIRE(trunc_s >= trunc_d,
             "tsdf_merge: trunc_s=%g < trunc_d=%g (a source that saturates earlier than the destination knows only \"free\" "
             "where the destination wants a distance)", trunc_s, trunc_d);
  GS_REQUIRE(merge_finite(lo_dx) && merge_finite(lo_dy) && merge_finite(lo_dz) && merge_finite(lo_sx) && merge_finite(lo_sy) &&
                 merge_finite(lo_sz),
             "tsdf_merge: lo_d=(%g, %g, %g) lo_s=(%g, %g, %g)", lo_dx, lo_dy, lo_dz, lo_sx, lo_sy, lo_sz);
  GS_REQUIRE(max_weight >= 1.0f, "tsdf_merge: max_weight=%g (need >= 1)", max_weight);
  GS_REQUIRE(min_weight > 0.0f, "tsdf_merge: min_weight=%g (need > 0: a cell no frame saw has nothing to add)", min_weight);
  GS_REQUIRE(tsdf_d && weight_d && tsdf_s && weight_s && d2s, "tsdf_merge: null pointer");
  GS_REQUIRE(tsdf_d != tsdf_s && weight_d != weight_s && (!colors_d || colors_d != colors_s),
             "tsdf_merge: source and destination are the same lattice");
  MergeArgs a;
  for (int i = 0; i < 12; ++i) {
    GS_REQUIRE(merge_finite(d2s[i]), "tsdf_merge: transform entry %d is %g", i, d2s[i]);
    a.m[i] = d2s[i];
  }
  a.tsdf_d = tsdf_d; a.weight_d = weight_d; a.colors_d = colors_d;
  a.tsdf_s = tsdf_s; a.weight_s = weight_s; a.colors_s = colors_s;
  a.d = merge_lattice(nx_d, ny_d, nz_d, lo_dx, lo_dy, lo_dz, voxel_d);
  a.s = merge_lattice(nx_s, ny_s, nz_s, lo_sx, lo_sy, lo_sz, voxel_s);
  a.nx_d = nx_d;
  a.np_d = (unsigned)nx_d * (unsigned)ny_d * (unsigned)nz_d;
  a.np_s = (unsigned)nx_s * (unsigned)ny_s * (unsigned)nz_s;
  a.ratio = trunc_s / trunc_d;
  a.min_weight = min_weight; a.max_weight = max_weight;
  const dim3 grid((unsigned)gs_cdiv(nz_d, GS_WAVE), (unsigned)gs_cdiv(ny_d, MERGE_TILE_Y), (unsigned)nx_d);
  GS_TIMING_PRE();
  if (colors_d && colors_s)
    tsdf_merge_kernel<true><<<grid, MERGE_THREADS, 0, (hipStream_t)stream>>>(a);
  else
    tsdf_merge_kernel<false><<<grid, MERGE_THREADS, 0, (hipStream_t)stream>>>(a);
  GS_CHECK_LAUNCH("tsdf_merge");
  return GS_OK;
}
