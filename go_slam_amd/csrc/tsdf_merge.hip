// Two TSDF lattices of tsdf.hip put together: where does volume S sit in volume D, and S fused into D.  (No counterpart
// in the reference.)  Contract: include/goslam_hip.h (gs_tsdf_register_workspace_bytes, gs_tsdf_register_system,
// gs_tsdf_merge); tests/tsdf_merge_restatement.py restates the three with one rounding per operation and the summation
// order written out.  Compiled with -ffp-contract=off.
//
// tsdf_register_system_kernel: tsdf_gn.h's system kernel (the gather of D, the 29 fp64 sums and their order are there,
// shared with tsdf_align.hip) with strided lattice points of S as samples: one workgroup per (pose, chunk of
// gs_tsdf_align_chunk() of them).  A wave's 64 samples are neighbours along S's z axis (stride apart), so the two loads of
// S share cache lines and the sixteen corner loads of D fall into neighbouring cells.  A sample that S saw and that is
// unsaturated in both truncations is considered; the reference value is S's in units of D's truncation.
// tsdf_register_sum_kernel: tsdf_gn.h's chunk sum.  The rows have gs_tsdf_align_system's layout and feed
// gs_tsdf_align_step unchanged.
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
#include "tsdf_gn.h"

namespace {

constexpr int MERGE_THREADS = 256;
constexpr int MERGE_TILE_Y = MERGE_THREADS / GS_WAVE;

struct RegisterArgs {      // by-value kernel argument (SGPRs)
  GnField d;
  const float* tsdf_s;
  const float* weight_s;
  const double* pose;      // [B,3,4], S-world to D-world
  double* partial;         // [B,n_chunks,32]
  TsdfLattice s;
  int stride, chunk;
  int sny, snz;            // strided lattice points of S along y and z
  int n_samples, n_chunks;
  float ratio;             // trunc_S / trunc_D
};

// four waves per SIMD: at most 128 VGPRs (tests/test_tsdf_merge_cpu.py holds the budget)
__global__ __launch_bounds__(GN_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
void tsdf_register_system_kernel(const RegisterArgs a) {
  const int b = blockIdx.x / a.n_chunks;
  const int chunk = blockIdx.x - b * a.n_chunks;
  GnSums sums;
  const GnPose p = gn_pose(a.pose + (size_t)b * 12);
  const int syz = a.sny * a.snz;
  const int s_end = min((chunk + 1) * a.chunk, a.n_samples);
#pragma nounroll
  for (int s = chunk * a.chunk + (int)threadIdx.x; s < s_end; s += GN_THREADS) {
    const int si = s / syz, rem = s - si * syz;
    const int sj = rem / a.snz, sk = rem - sj * a.snz;
    const int ii = si * a.stride, jj = sj * a.stride, kk = sk * a.stride;
    const unsigned at_s = tsdf_cell_at<unsigned>(a.s, ii, jj, kk);
    const float ws = a.weight_s[at_s], fs = a.tsdf_s[at_s];
    const float fr = fs * a.ratio;                             // the source's value in units of D's truncation
    const bool valid = ws >= a.d.min_weight && fabsf(fs) < 1.0f && fabsf(fr) < 1.0f;
    if (valid) ++sums.considered;
    const float px = a.s.lox + (float)ii * a.s.voxel, py = a.s.loy + (float)jj * a.s.voxel, pz = a.s.loz + (float)kk * a.s.voxel;
    const float qx = (p.r00 * px + p.r01 * py) + p.r02 * pz;
    const float qy = (p.r10 * px + p.r11 * py) + p.r12 * pz;
    const float qz = (p.r20 * px + p.r21 * py) + p.r22 * pz;
    gn_fold<false>(sums, a.d, p, qx, qy, qz, valid, fr);
  }
  gn_store_row(sums, a.partial + ((size_t)b * a.n_chunks + chunk) * GN_ROW);
}

__global__ __launch_bounds__(GS_WAVE) void tsdf_register_sum_kernel(const double* __restrict__ partial, int n_chunks,
                                                                    double* __restrict__ out) {
  gn_sum_chunks(partial, n_chunks, out);
}

struct MergeArgs {         // by-value kernel argument (SGPRs)
  float* tsdf_d;
  float* weight_d;
  float* colors_d;         // [3,nx,ny,nz]; touched only by the COLOR kernel
  const float* tsdf_s;
  const float* weight_s;
  const float* colors_s;
  TsdfLattice d, s;
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
  if (!tsdf_cell_inside(a.s, ax, ay, az)) return;
  const unsigned at_s = tsdf_cell_at<unsigned>(a.s, (int)ax, (int)ay, (int)az);
  const TsdfCorners wc = tsdf_corners_load(a.weight_s, at_s, a.s.ny, a.s.nz);
  if (!tsdf_corners_at_least(wc, a.min_weight)) return;
  const float sx = gx - ax, sy = gy - ay, sz = gz - az;
  const float fs = tsdf_corners_value(tsdf_corners_load(a.tsdf_s, at_s, a.s.ny, a.s.nz), sx, sy, sz);
  const float ws = tsdf_corners_value(wc, sx, sy, sz);
  float s = fs * a.ratio;
  if (s < -1.0f) return;
  s = fminf(1.0f, s);

  const unsigned at = tsdf_cell_at<unsigned>(a.d, i, j, k);
  const float w0 = a.weight_d[at];
  const float w1 = w0 + ws;
  a.tsdf_d[at] = (a.tsdf_d[at] * w0 + s * ws) / w1;
  if (COLOR) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float cs = tsdf_corners_value(tsdf_corners_load(a.colors_s + (size_t)ch * a.np_s, at_s, a.s.ny, a.s.nz), sx, sy, sz);
      float* __restrict__ cd = a.colors_d + (size_t)ch * a.np_d;
      cd[at] = (cd[at] * w0 + cs * ws) / w1;
    }
  }
  a.weight_d[at] = fminf(w1, a.max_weight);
}

bool merge_finite(float v) { return fabsf(v) < INFINITY; }

// strided lattice points of an nx x ny x nz lattice, or -1 for sizes the entry points refuse
long long register_samples(int nx, int ny, int nz, int stride) {
  if (!tsdf_dims_ok(nx, ny, nz) || stride < 1) return -1;
  return (long long)gs_cdiv(nx, stride) * gs_cdiv(ny, stride) * gs_cdiv(nz, stride);
}

}  // namespace

extern "C" int gs_tsdf_align_chunk(void);

extern "C" size_t gs_tsdf_register_workspace_bytes(int n_poses, int nx_s, int ny_s, int nz_s, int stride) {
  return gn_workspace_bytes(n_poses, register_samples(nx_s, ny_s, nz_s, stride), gs_tsdf_align_chunk());
}

extern "C" int gs_tsdf_register_system(const float* tsdf_d, const float* weight_d, int nx_d, int ny_d, int nz_d,
                                       float lo_dx, float lo_dy, float lo_dz, float voxel_d, float trunc_d,
                                       const float* tsdf_s, const float* weight_s, int nx_s, int ny_s, int nz_s,
                                       float lo_sx, float lo_sy, float lo_sz, float voxel_s, float trunc_s,
                                       const double* pose, int n_poses, int stride, float min_weight, float huber,
                                       void* workspace, double* out, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx_d, ny_d, nz_d), "tsdf_register_system: destination lattice %d x %d x %d outside [2, 1024]", nx_d,
             ny_d, nz_d);
  GS_REQUIRE(tsdf_dims_ok(nx_s, ny_s, nz_s), "tsdf_register_system: source lattice %d x %d x %d outside [2, 1024]", nx_s,
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
  const long long chunks = gn_chunks(n, chunk);
  GS_REQUIRE(gn_fits(n_poses, chunks), "tsdf_register_system: %d poses of %lld chunks are too many for one launch", n_poses,
             chunks);
  GS_REQUIRE(tsdf_d && weight_d && tsdf_s && weight_s && pose && workspace && out, "tsdf_register_system: null pointer");
  RegisterArgs a;
  a.d = GnField{tsdf_d, weight_d, tsdf_lattice(nx_d, ny_d, nz_d, lo_dx, lo_dy, lo_dz, voxel_d), min_weight, huber};
  a.tsdf_s = tsdf_s; a.weight_s = weight_s;
  a.pose = pose; a.partial = (double*)workspace;
  a.s = tsdf_lattice(nx_s, ny_s, nz_s, lo_sx, lo_sy, lo_sz, voxel_s);
  a.stride = stride; a.chunk = chunk;
  a.sny = gs_cdiv(ny_s, stride); a.snz = gs_cdiv(nz_s, stride);
  a.n_samples = (int)n; a.n_chunks = (int)chunks;
  a.ratio = trunc_s / trunc_d;
  return gn_enqueue("tsdf_register_system", "tsdf_register_sum", tsdf_register_system_kernel, tsdf_register_sum_kernel, a,
                    n_poses, out, stream);
}

extern "C" int gs_tsdf_merge(float* tsdf_d, float* weight_d, float* colors_d, int nx_d, int ny_d, int nz_d, float lo_dx,
                             float lo_dy, float lo_dz, float voxel_d, float trunc_d, float max_weight, const float* tsdf_s,
                             const float* weight_s, const float* colors_s, int nx_s, int ny_s, int nz_s, float lo_sx,
                             float lo_sy, float lo_sz, float voxel_s, float trunc_s, const float* d2s, float min_weight,
                             gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx_d, ny_d, nz_d), "tsdf_merge: destination lattice %d x %d x %d outside [2, 1024]", nx_d, ny_d, nz_d);
  GS_REQUIRE(tsdf_dims_ok(nx_s, ny_s, nz_s), "tsdf_merge: source lattice %d x %d x %d outside [2, 1024]", nx_s, ny_s, nz_s);
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
  a.d = tsdf_lattice(nx_d, ny_d, nz_d, lo_dx, lo_dy, lo_dz, voxel_d);
  a.s = tsdf_lattice(nx_s, ny_s, nz_s, lo_sx, lo_sy, lo_sz, voxel_s);
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
