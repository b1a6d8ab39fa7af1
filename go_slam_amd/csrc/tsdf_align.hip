// Direct SDF alignment of depth images to the TSDF lattice of tsdf.hip: where is this camera in the volume that is
// already there?  (No counterpart in the reference.)  Contract: include/goslam_hip.h (gs_tsdf_align_chunk,
// gs_tsdf_align_workspace_bytes, gs_tsdf_align_system, gs_tsdf_align_step); tests/tsdf_align_restatement.py restates
// the four with one rounding per operation and the summation order written out.  Compiled with -ffp-contract=off.
//
// tsdf_align_system_kernel: tsdf_gn.h's system kernel (the gather, the 29 fp64 sums and their order are there) with
// sampled pixels of a depth map as samples: one workgroup per (pose, chunk of TSDF_ALIGN_CHUNK of them).  The pose and
// its depth map's index sit at wave-uniform addresses (scalar loads); the lattice, the intrinsics and the thresholds are
// by-value kernel arguments.  A wave's 64 samples are neighbours in an image row, so their back-projections fall into
// neighbouring cells and the sixteen corner loads of a wave share cache lines.  A pixel with a depth is considered, the
// reference value is 0: the residual is the TSDF value itself.
// tsdf_align_sum_kernel: tsdf_gn.h's chunk sum.
// tsdf_align_step_kernel: one lane per pose; the damped 6 x 6 Cholesky solve and the quaternion retraction in fp64.
#include "tsdf_gn.h"

#ifndef TSDF_ALIGN_CHUNK
#define TSDF_ALIGN_CHUNK 2048        // sampled pixels per workgroup: a contract constant (gs_tsdf_align_chunk), DESIGN 28
#endif

namespace {

constexpr int ALIGN_CHUNK = TSDF_ALIGN_CHUNK;
static_assert(ALIGN_CHUNK % GN_THREADS == 0 && ALIGN_CHUNK >= GN_THREADS, "a chunk is whole rounds of the workgroup");

struct AlignArgs {         // by-value kernel argument (SGPRs)
  GnField vol;
  const float* depth;      // [k,h,w]
  const int* frame;        // [B]
  const double* pose;      // [B,3,4]
  double* partial;         // [B,n_chunks,32]
  int k, h, w, stride;
  int sw;                  // sampled pixels per image row
  int n_samples, n_chunks;
  float fx, fy, cx, cy;
  float max_depth;
};

// four waves per SIMD: at most 128 VGPRs (tests/test_tsdf_align_cpu.py holds the budget: 111, no scratch)
__global__ __launch_bounds__(GN_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
void tsdf_align_system_kernel(const AlignArgs a) {
  const int b = blockIdx.x / a.n_chunks;
  const int chunk = blockIdx.x - b * a.n_chunks;
  const int fr = a.frame[b];
  GnSums sums;
  if (fr >= 0 && fr < a.k) {                                 // else: a row of zeros, and nothing of depth is read
    const GnPose p = gn_pose(a.pose + (size_t)b * 12);
    const float* __restrict__ dmap = a.depth + (size_t)fr * a.h * a.w;
    const int s_end = min((chunk + 1) * ALIGN_CHUNK, a.n_samples);
#pragma nounroll
    for (int s = chunk * ALIGN_CHUNK + (int)threadIdx.x; s < s_end; s += GN_THREADS) {
      const int sv = s / a.sw, su = s - sv * a.sw;
      const int iu = su * a.stride, iv = sv * a.stride;
      const float d = dmap[(size_t)iv * a.w + iu];
      if (d > 0.0f) ++sums.considered;
      const float px = ((float)iu - a.cx) / a.fx * d, py = ((float)iv - a.cy) / a.fy * d;
      const float qx = (p.r00 * px + p.r01 * py) + p.r02 * d;
      const float qy = (p.r10 * px + p.r11 * py) + p.r12 * d;
      const float qz = (p.r20 * px + p.r21 * py) + p.r22 * d;
      gn_fold<true>(sums, a.vol, p, qx, qy, qz, d > 0.0f && d <= a.max_depth, 0.0f);
    }
  }
  gn_store_row(sums, a.partial + ((size_t)b * a.n_chunks + chunk) * GN_ROW);
}

__global__ __launch_bounds__(GS_WAVE) void tsdf_align_sum_kernel(const double* __restrict__ partial, int n_chunks,
                                                                 double* __restrict__ out) {
  gn_sum_chunks(partial, n_chunks, out);
}

__global__ __launch_bounds__(GS_WAVE) void tsdf_align_step_kernel(const double* __restrict__ out, double* __restrict__ pose,
                                                                  int B, double lam_rel, double lam_abs, double min_count,
                                                                  double* __restrict__ trace) {
  const int b = blockIdx.x * GS_WAVE + threadIdx.x;
  if (b >= B) return;
  const double* __restrict__ row = out + (size_t)b * GN_ROW;
  double A[6][6], L[6][6], g[6];
  {
    int at = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) {
        const double hij = row[at++];
        A[i][j] = hij;
        A[j][i] = hij;
      }
      g[i] = row[21 + i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) A[i][i] = (A[i][i] + lam_rel * A[i][i]) + lam_abs;
  }
  const double cost = row[27], count = row[28], considered = row[30];
  bool ok = !(count < min_count);
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
    if (!(s > 0.0)) ok = false;
    const double ljj = sqrt(s);
    L[j][j] = ljj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k];
      L[i][j] = t / ljj;
    }
  }
  if (trace) {
    double* __restrict__ tr = trace + (size_t)b * 4;
    tr[0] = cost; tr[1] = count; tr[2] = considered; tr[3] = ok ? 1.0 : 0.0;
  }
  if (!ok) return;
  double y[6], x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double t = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t = t - L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int k = 5; k > i; --k) t = t - L[k][i] * x[k];
    x[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = -x[i];

  double* __restrict__ m = pose + (size_t)b * 12;
  const double hx = x[3] * 0.5, hy = x[4] * 0.5, hz = x[5] * 0.5;
  const double len = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
  const double qa = 1.0 / len, qb = hx / len, qc = hy / len, qd = hz / len;
  const double aa = qa * qa, bb = qb * qb, cc = qc * qc, dd = qd * qd;
  double dR[3][3];
  dR[0][0] = ((aa + bb) - cc) - dd;       dR[0][1] = 2.0 * (qb * qc - qa * qd);  dR[0][2] = 2.0 * (qb * qd + qa * qc);
  dR[1][0] = 2.0 * (qb * qc + qa * qd);   dR[1][1] = ((aa - bb) + cc) - dd;      dR[1][2] = 2.0 * (qc * qd - qa * qb);
  dR[2][0] = 2.0 * (qb * qd - qa * qc);   dR[2][1] = 2.0 * (qc * qd + qa * qb);  dR[2][2] = ((aa - bb) - cc) + dd;
  double R[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i][j] = m[i * 4 + j];
  double P[3][3], E[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) P[i][j] = (dR[i][0] * R[0][j] + dR[i][1] * R[1][j]) + dR[i][2] * R[2][j];
  // One Newton step toward the nearest rotation, P (I - E / 2) with E = P^T P - I.  A product of fp64 rotations leaves
  // the rotations by a few 1e-16 per step and the departures add up (1e-14 after 100 steps); with this step they do
  // not: |R^T R - I| stays below 5e-16 however many steps a pose has been through.
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      E[i][j] = ((P[0][i] * P[0][j] + P[1][i] * P[1][j]) + P[2][i] * P[2][j]) - (i == j ? 1.0 : 0.0);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) m[i * 4 + j] = P[i][j] - 0.5 * ((P[i][0] * E[0][j] + P[i][1] * E[1][j]) + P[i][2] * E[2][j]);
    m[i * 4 + 3] = m[i * 4 + 3] + x[i];
  }
}

// sampled pixels of an h x w image at `stride`, or -1 for sizes the entry points refuse
long long align_samples(int h, int w, int stride) {
  if (h < 1 || w < 1 || stride < 1 || (long long)h * w > (1LL << 30)) return -1;
  return (long long)gs_cdiv(h, stride) * gs_cdiv(w, stride);
}

}  // namespace

extern "C" int gs_tsdf_align_chunk(void) { return ALIGN_CHUNK; }

extern "C" size_t gs_tsdf_align_workspace_bytes(int n_poses, int h, int w, int stride) {
  return gn_workspace_bytes(n_poses, align_samples(h, w, stride), ALIGN_CHUNK);
}

extern "C" int gs_tsdf_align_system(const float* tsdf, const float* weight, int nx, int ny, int nz, const float* depth,
                                    const int* frame, const double* pose, int n_poses, int k, int h, int w, int stride,
                                    float fx, float fy, float cx, float cy, float lo_x, float lo_y, float lo_z,
                                    float voxel, float max_depth, float min_weight, float huber, void* workspace,
                                    double* out, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_align_system: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  const long long n = align_samples(h, w, stride);
  GS_REQUIRE(n_poses >= 0 && k >= 0 && n >= 0, "tsdf_align_system: n_poses=%d k=%d h=%d w=%d stride=%d", n_poses, k, h, w,
             stride);
  GS_REQUIRE(fx != 0.0f && fy != 0.0f && fabsf(fx) < INFINITY && fabsf(fy) < INFINITY && fabsf(cx) < INFINITY &&
                 fabsf(cy) < INFINITY,
             "tsdf_align_system: fx=%g fy=%g cx=%g cy=%g", fx, fy, cx, cy);
  GS_REQUIRE(voxel > 0.0f && voxel < INFINITY, "tsdf_align_system: voxel=%g", voxel);
  GS_REQUIRE(fabsf(lo_x) < INFINITY && fabsf(lo_y) < INFINITY && fabsf(lo_z) < INFINITY, "tsdf_align_system: lo=(%g, %g, %g)",
             lo_x, lo_y, lo_z);
  GS_REQUIRE(huber > 0.0f, "tsdf_align_system: huber=%g (need > 0)", huber);
  GS_REQUIRE(max_depth > 0.0f, "tsdf_align_system: max_depth=%g (need > 0; +inf keeps every depth)", max_depth);
  GS_REQUIRE(min_weight == min_weight, "tsdf_align_system: min_weight is NaN");
  if (n_poses == 0) return GS_OK;
  GS_REQUIRE(k >= 1, "tsdf_align_system: %d poses without a depth map", n_poses);
  const long long chunks = gn_chunks(n, ALIGN_CHUNK);
  GS_REQUIRE(gn_fits(n_poses, chunks), "tsdf_align_system: %d poses of %lld chunks are too many for one launch", n_poses,
             chunks);
  GS_REQUIRE(tsdf && weight && depth && frame && pose && workspace && out, "tsdf_align_system: null pointer");
  AlignArgs a;
  a.vol = GnField{tsdf, weight, tsdf_lattice(nx, ny, nz, lo_x, lo_y, lo_z, voxel), min_weight, huber};
  a.depth = depth; a.frame = frame; a.pose = pose; a.partial = (double*)workspace;
  a.k = k; a.h = h; a.w = w; a.stride = stride;
  a.sw = gs_cdiv(w, stride);
  a.n_samples = (int)n; a.n_chunks = (int)chunks;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
  a.max_depth = max_depth;
  return gn_enqueue("tsdf_align_system", "tsdf_align_sum", tsdf_align_system_kernel, tsdf_align_sum_kernel, a, n_poses, out,
                    stream);
}

extern "C" int gs_tsdf_align_step(const double* out, double* pose, int n_poses, double lam_rel, double lam_abs,
                                  int min_count, double* trace, gs_stream_t stream) {
  GS_REQUIRE(n_poses >= 0, "tsdf_align_step: n_poses=%d", n_poses);
  GS_REQUIRE(lam_rel >= 0.0 && lam_rel < (double)INFINITY && lam_abs >= 0.0 && lam_abs < (double)INFINITY,
             "tsdf_align_step: lam_rel=%g lam_abs=%g (need finite, >= 0)", lam_rel, lam_abs);
  GS_REQUIRE(min_count >= 1, "tsdf_align_step: min_count=%d (need >= 1)", min_count);
  if (n_poses == 0) return GS_OK;
  GS_REQUIRE(out && pose, "tsdf_align_step: null pointer");
  GS_TIMING_PRE();
  tsdf_align_step_kernel<<<(unsigned)gs_cdiv(n_poses, GS_WAVE), GS_WAVE, 0, (hipStream_t)stream>>>(
      out, pose, n_poses, lam_rel, lam_abs, (double)min_count, trace);
  GS_CHECK_LAUNCH("tsdf_align_step");
  return GS_OK;
}
