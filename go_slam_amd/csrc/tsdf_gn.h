// The Gauss-Newton system of a pose against a TSDF lattice, once for tsdf_align.hip (samples are pixels of a depth map)
// and tsdf_merge.hip (samples are lattice points of a second volume): what include/goslam_hip.h fixes for both, above all
// the summation order, is here; a file adds its args struct, its sample loop (where a sample comes from, what
// "considered" means, the reference value) and its two __global__ kernels.
//
// A system kernel is one workgroup of GN_THREADS per (pose, chunk of samples); a lane walks its samples t, t + 256, ... of
// the chunk and hands each to gn_fold.  The contract's early-outs are folded into one predicate: a skipped sample loads
// cell 0 and drops it, so the 29 accumulators are not carried through a nest of branches and the sums sit behind one.
// In what order the sixteen corner loads (weight and tsdf) are issued and waited for is gn_fold's WEIGHTS_FIRST.  The 29
// fp64 sums (21 of H's upper triangle, 6 of b, cost, sq) live in registers and the two counts in
// integers (exact: their order is free).  gn_store_row ends the chunk: gs_wave_sum_f64 per value (v += v[lane ^ m], m =
// 32 .. 1) and the four waves' totals through 1 KiB of LDS as ((w0 + w1) + w2) + w3, gs_tsdf_frame_change's order.  No
// atomics.  A sum kernel (gn_sum_chunks) has one lane per (pose, value) add the chunks' totals in increasing chunk order.
#pragma once
#include "tsdf_cell.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_WAVES = GN_THREADS / GS_WAVE;
constexpr int GN_ROW = 32;                  // doubles per row of out and of a chunk's partial
constexpr int GN_SUMS = 29;                 // H 21, b 6, cost, sq
constexpr int GN_SUM_BATCH = 16;            // chunk totals the sum kernel loads before it adds them

struct GnField {           // the volume the samples are gathered from; part of a by-value kernel argument (SGPRs)
  const float* tsdf;
  const float* weight;
  TsdfLattice l;
  float min_weight, huber;
};

struct GnSums {
  double acc[GN_SUMS] = {};
  int count = 0, considered = 0;
};

struct GnPose { float r00, r01, r02, ox, r10, r11, r12, oy, r20, r21, r22, oz; };

// (float) of the fp64 pose m[3][4]; the conversion is a vector instruction, so the uniform results are moved back to SGPRs
__device__ __forceinline__ GnPose gn_pose(const double* __restrict__ m) {
  float pm[12];
#pragma unroll
  for (int i = 0; i < 12; ++i)
    pm[i] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, (float)m[i])));
  return GnPose{pm[0], pm[1], pm[2], pm[3], pm[4], pm[5], pm[6], pm[7], pm[8], pm[9], pm[10], pm[11]};
}

// One sample: q is its point rotated by the pose (the translation is added here), `valid` what the caller's own tests
// left of it, ref the value the field's is compared with (the residual is f - ref).
// WEIGHTS_FIRST changes no result, only how `valid` joins the weight test, and with it what hipcc makes of the sixteen
// loads.  true (tsdf_align.hip): every lane loads the eight weights, waits for them and branches, and only a lane that
// passes loads the eight values; the launches of a tracking call (one pose, a few short chains) are 2 us of 26 faster
// this way than with all sixteen in flight, the wide ones up to 16 % slower.  false (tsdf_merge.hip): every lane loads
// the eight weights, a lane with a cell loads the eight values behind a branch that does not wait, and the sixteen are
// waited for together; with `true` that kernel no longer fits its 128 VGPRs (20 B of scratch).  Both are the schedules
// the two kernels had when each wrote the gather out itself.
template <bool WEIGHTS_FIRST>
__device__ __forceinline__ void gn_fold(GnSums& s, const GnField& d, const GnPose& p, float qx, float qy, float qz,
                                        bool valid, float ref) {
  const TsdfLattice& l = d.l;
  const float gx = ((qx + p.ox) - l.lox) / l.voxel, gy = ((qy + p.oy) - l.loy) / l.voxel, gz = ((qz + p.oz) - l.loz) / l.voxel;
  const float ax = floorf(gx), ay = floorf(gy), az = floorf(gz);
  valid = valid && tsdf_cell_inside(l, ax, ay, az);
  // a skipped sample reads cell 0 and drops what it read, instead of a branch per early-out
  const unsigned at = valid ? tsdf_cell_at<unsigned>(l, (int)ax, (int)ay, (int)az) : 0u;
  const TsdfCorners wc = tsdf_corners_load(d.weight, at, l.ny, l.nz);
  const TsdfCorners c = tsdf_corners_load(d.tsdf, at, l.ny, l.nz);
  if constexpr (WEIGHTS_FIRST)
    valid = valid & tsdf_corners_at_least(wc, d.min_weight);
  else
    valid = valid && tsdf_corners_at_least(wc, d.min_weight);
  const float sx = gx - ax, sy = gy - ay, sz = gz - az;
  const float f = tsdf_corners_value(c, sx, sy, sz);
  valid = valid && fabsf(f) < 1.0f;
  if (!valid) return;
  float g[3];
  tsdf_corners_gradient(c, sx, sy, sz, g);
  const float wx = g[0] / l.voxel, wy = g[1] / l.voxel, wz = g[2] / l.voxel;
  float J[6];
  J[0] = wx; J[1] = wy; J[2] = wz;
  J[3] = qy * wz - qz * wy;
  J[4] = qz * wx - qx * wz;
  J[5] = qx * wy - qy * wx;
  const float r = f - ref;
  const float ar = fabsf(r);
  const float wt = ar <= d.huber ? 1.0f : d.huber / ar;
  const double rd = (double)r, wd = (double)wt;
  int at_h = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wj = wd * (double)J[i];
#pragma unroll
    for (int j = i; j < 6; ++j) {
      s.acc[at_h] += wj * (double)J[j];
      ++at_h;
    }
    s.acc[21 + i] += wj * rd;
  }
  s.acc[27] += (wd * rd) * rd;
  s.acc[28] += rd * rd;
  ++s.count;
}

// The workgroup's sums as the chunk's row: H, b, cost, count, sq, considered, 0.  Every thread of the workgroup calls it.
__device__ __forceinline__ void gn_store_row(const GnSums& s, double* __restrict__ row) {
  __shared__ double part[GN_WAVES][GN_ROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < GN_SUMS; ++i) {
    const double v = gs_wave_sum_f64(s.acc[i]);
    if (lane == 0) part[wave][i == 28 ? 29 : i] = v;
    __builtin_amdgcn_sched_barrier(0);                       // one value's exchanges at a time: they need no more registers
  }
  {
    const int cn = gs_wave_sum_i32(s.count), cs = gs_wave_sum_i32(s.considered);   // integers: any order gives the sum
    if (lane == 0) {
      part[wave][28] = (double)cn;
      part[wave][30] = (double)cs;
      part[wave][31] = 0.0;
    }
  }
  __syncthreads();
  if (threadIdx.x < GN_ROW) {
    const int i = threadIdx.x;
    row[i] = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i];
  }
}

// The body of a sum kernel, one wave per pose: out's row is the sum of the pose's chunk rows in increasing chunk order.
// A lane loads sixteen of them at a time, so that the sum is not a chain of as many memory latencies as there are chunks.
__device__ __forceinline__ void gn_sum_chunks(const double* __restrict__ partial, int n_chunks, double* __restrict__ out) {
  const int i = threadIdx.x;
  if (i >= GN_ROW) return;
  const double* __restrict__ p = partial + (size_t)blockIdx.x * n_chunks * GN_ROW + i;
  double t = p[0];
  int c = 1;
  for (; c + GN_SUM_BATCH <= n_chunks; c += GN_SUM_BATCH) {         // the loads of a batch in flight together, the adds in order
    double v[GN_SUM_BATCH];
#pragma unroll
    for (int j = 0; j < GN_SUM_BATCH; ++j) v[j] = p[(size_t)(c + j) * GN_ROW];
#pragma unroll
    for (int j = 0; j < GN_SUM_BATCH; ++j) t = t + v[j];
  }
  for (; c < n_chunks; ++c) t = t + p[(size_t)c * GN_ROW];
  out[(size_t)blockIdx.x * GN_ROW + i] = t;
}

// ---- the host side of gs_tsdf_align_system and gs_tsdf_register_system ---------------------------------------------------
long long gn_chunks(long long n_samples, int chunk) { return (n_samples + chunk - 1) / chunk; }

// one launch has a workgroup per (pose, chunk)
bool gn_fits(int n_poses, long long chunks) { return (long long)n_poses * chunks <= 0x7fffffffLL; }

// bytes of the chunks' rows, 0 for what an entry point refuses (n_samples < 0 stands for refused sizes)
size_t gn_workspace_bytes(int n_poses, long long n_samples, int chunk) {
  if (n_poses < 0 || n_samples < 0) return 0;
  const long long chunks = gn_chunks(n_samples, chunk);
  if (!gn_fits(n_poses, chunks)) return 0;
  return (size_t)n_poses * (size_t)chunks * GN_ROW * sizeof(double);
}

// The two launches, after the entry point's checks: a.n_chunks rows per pose into a.partial, their sums into out.  The
// names are the timer's.
template <class Args>
int gn_enqueue(const char* system_name, const char* sum_name, void (*system)(Args), void (*sum)(const double*, int, double*),
               const Args& a, int n_poses, double* out, gs_stream_t stream) {
  GS_TIMING_PRE();
  system<<<(unsigned)((long long)n_poses * a.n_chunks), GN_THREADS, 0, (hipStream_t)stream>>>(a);
  GS_CHECK_LAUNCH(system_name);
  sum<<<(unsigned)n_poses, GS_WAVE, 0, (hipStream_t)stream>>>(a.partial, a.n_chunks, out);
  GS_CHECK_LAUNCH(sum_name);
  return GS_OK;
}

}  // namespace
