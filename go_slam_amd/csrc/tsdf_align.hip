// Direct SDF alignment of depth images to the TSDF lattice of tsdf.hip: where is this camera in the volume that is
// already there?  (No counterpart in the reference.)  Contract: include/goslam_hip.h (gs_tsdf_align_chunk,
// gs_tsdf_align_workspace_bytes, gs_tsdf_align_system, gs_tsdf_align_step); tests/tsdf_align_restatement.py restates
// the four with one rounding per operation and the summation order written out.  Compiled with -ffp-contract=off.
//
// tsdf_align_system_kernel: one workgroup of 256 threads per (pose, chunk of TSDF_ALIGN_CHUNK sampled pixels).  The
// pose and its depth map's index sit at wave-uniform addresses (scalar loads); the lattice, the intrinsics and the
// thresholds are by-value kernel arguments.  A lane walks its samples t, t + 256, ... of the chunk: a wave's 64 samples
// are neighbours in an image row, so their back-projections fall into neighbouring cells and the sixteen corner loads
// (weight and tsdf) of a wave share cache lines.  The contract's early-outs are folded into one predicate: a skipped
// pixel loads cell 0 and drops it, so a lane has its sixteen loads in flight at once and the sums sit behind one branch.
// The 29 fp64 sums (21 of H's upper triangle, 6 of b, cost, sq) live in registers and the two counts in integers
// (exact: their order is free); the chunk ends with gs_wave_sum_f64 per value (v += v[lane ^ m], m = 32 .. 1) and the
// four waves' totals through 1 KiB of LDS as ((w0 + w1) + w2) + w3, gs_tsdf_frame_change's order.  No atomics.
// tsdf_align_sum_kernel: one lane per (pose, value) adds the chunks' totals in increasing chunk order into out; it
// loads sixteen of them at a time, so that the sum is not a chain of as many memory latencies as there are chunks.
// tsdf_align_step_kernel: one lane per pose; the damped 6 x 6 Cholesky solve and the quaternion retraction in fp64.
#include "common.h"

#ifndef TSDF_ALIGN_CHUNK
#define TSDF_ALIGN_CHUNK 2048        // sampled pixels per workgroup: a contract constant (gs_tsdf_align_chunk), DESIGN 28
#endif

namespace {

constexpr int ALIGN_THREADS = 256;
constexpr int ALIGN_WAVES = ALIGN_THREADS / GS_WAVE;
constexpr int ALIGN_CHUNK = TSDF_ALIGN_CHUNK;
constexpr int ALIGN_ROW = 32;               // doubles per row of out and of a chunk's partial
constexpr int ALIGN_SUMS = 29;              // H 21, b 6, cost, sq
constexpr int ALIGN_SUM_BATCH = 16;         // chunk totals the sum kernel loads before it adds them
static_assert(ALIGN_CHUNK % ALIGN_THREADS == 0 && ALIGN_CHUNK >= ALIGN_THREADS, "a chunk is whole rounds of the workgroup");

struct AlignArgs {         // by-value kernel argument (SGPRs)
  const float* tsdf;
  const float* weight;
  const float* depth;      // [k,h,w]
  const int* frame;        // [B]
  const double* pose;      // [B,3,4]
  double* partial;         // [B,n_chunks,32]
  int ny, nz;
  float topx, topy, topz;  // float(n - 1)
  float lox, loy, loz, voxel;
  int k, h, w, stride;
  int sw;                  // sampled pixels per image row
  int n_samples, n_chunks;
  float fx, fy, cx, cy;
  float max_depth, min_weight, huber;
};

__device__ __forceinline__ float align_lerp(float p, float q, float s) { return p + s * (q - p); }

struct AlignCorners { float v000, v001, v010, v011, v100, v101, v110, v111; };   // v[x][y][z]

// 32-bit offsets: the largest lattice has 2^30 points
__device__ __forceinline__ AlignCorners align_load(const float* __restrict__ p, unsigned at, int ny, int nz) {
  const unsigned sy = (unsigned)nz, sx = (unsigned)ny * (unsigned)nz;
  AlignCorners c;
  c.v000 = p[at];           c.v001 = p[at + 1];
  c.v010 = p[at + sy];      c.v011 = p[at + sy + 1];
  c.v100 = p[at + sx];      c.v101 = p[at + sx + 1];
  c.v110 = p[at + sx + sy]; c.v111 = p[at + sx + sy + 1];
  return c;
}

// four waves per SIMD: at most 128 VGPRs (tests/test_tsdf_align_cpu.py holds the budget: 111, no scratch)
__global__ __launch_bounds__(ALIGN_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
void tsdf_align_system_kernel(const AlignArgs a) {
  __shared__ double part[ALIGN_WAVES][ALIGN_ROW];
  const int b = blockIdx.x / a.n_chunks;
  const int chunk = blockIdx.x - b * a.n_chunks;
  const int fr = a.frame[b];

  double acc[ALIGN_SUMS];
#pragma unroll
  for (int i = 0; i < ALIGN_SUMS; ++i) acc[i] = 0.0;
  int count = 0, considered = 0;

  if (fr >= 0 && fr < a.k) {                                 // else: a row of zeros, and nothing of depth is read
    const double* __restrict__ m = a.pose + (size_t)b * 12;
    // (float) of the fp64 pose; the conversion is a vector instruction, so the uniform results are moved back to SGPRs
    float pm[12];
#pragma unroll
    for (int i = 0; i < 12; ++i)
      pm[i] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, (float)m[i])));
    const float r00 = pm[0], r01 = pm[1], r02 = pm[2], ox = pm[3];
    const float r10 = pm[4], r11 = pm[5], r12 = pm[6], oy = pm[7];
    const float r20 = pm[8], r21 = pm[9], r22 = pm[10], oz = pm[11];
    const float* __restrict__ dmap = a.depth + (size_t)fr * a.h * a.w;
    const int s_end = min((chunk + 1) * ALIGN_CHUNK, a.n_samples);
#pragma nounroll
    for (int s = chunk * ALIGN_CHUNK + (int)threadIdx.x; s < s_end; s += ALIGN_THREADS) {
      const int sv = s / a.sw, su = s - sv * a.sw;
      const int iu = su * a.stride, iv = sv * a.stride;
      const float d = dmap[(size_t)iv * a.w + iu];
      if (d > 0.0f) ++considered;
      bool valid = d > 0.0f && d <= a.max_depth;
      const float px = ((float)iu - a.cx) / a.fx * d, py = ((float)iv - a.cy) / a.fy * d;
      const float qx = (r00 * px + r01 * py) + r02 * d;
      const float qy = (r10 * px + r11 * py) + r12 * d;
      const float qz = (r20 * px + r21 * py) + r22 * d;
      const float gx = ((qx + ox) - a.lox) / a.voxel, gy = ((qy + oy) - a.loy) / a.voxel, gz = ((qz + oz) - a.loz) / a.voxel;
      const float ax = floorf(gx), ay = floorf(gy), az = floorf(gz);
      valid = valid && ax >= 0.0f && ax < a.topx && ay >= 0.0f && ay < a.topy && az >= 0.0f && az < a.topz;
      // a skipped pixel reads cell 0 and drops what it read: sixteen loads in flight per lane instead of a branch each
      const unsigned at = valid ? ((unsigned)(int)ax * a.ny + (unsigned)(int)ay) * a.nz + (unsigned)(int)az : 0u;
      const AlignCorners wc = align_load(a.weight, at, a.ny, a.nz);
      const AlignCorners c = align_load(a.tsdf, at, a.ny, a.nz);
      const float mw = a.min_weight;
      valid = valid && wc.v000 >= mw && wc.v001 >= mw && wc.v010 >= mw && wc.v011 >= mw && wc.v100 >= mw && wc.v101 >= mw &&
              wc.v110 >= mw && wc.v111 >= mw;
      const float sx = gx - ax, sy = gy - ay, sz = gz - az;
      // gs_tsdf_raycast's sequences: the value by lerps z, y, x; the gradient from the z-lerps and the y-lerps
      const float z00 = align_lerp(c.v000, c.v001, sz), z01 = align_lerp(c.v010, c.v011, sz);
      const float z10 = align_lerp(c.v100, c.v101, sz), z11 = align_lerp(c.v110, c.v111, sz);
      const float x0 = align_lerp(z00, z01, sy), x1 = align_lerp(z10, z11, sy);
      const float f = align_lerp(x0, x1, sx);
      valid = valid && fabsf(f) < 1.0f;
      if (!valid) continue;
      const float y00 = align_lerp(c.v000, c.v010, sy), y01 = align_lerp(c.v001, c.v011, sy);
      const float y10 = align_lerp(c.v100, c.v110, sy), y11 = align_lerp(c.v101, c.v111, sy);
      const float nx = x1 - x0;
      const float ny = align_lerp(z01, z11, sx) - align_lerp(z00, z10, sx);
      const float nz = align_lerp(y01, y11, sx) - align_lerp(y00, y10, sx);
      const float wx = nx / a.voxel, wy = ny / a.voxel, wz = nz / a.voxel;
      float J[6];
      J[0] = wx; J[1] = wy; J[2] = wz;
      J[3] = qy * wz - qz * wy;
      J[4] = qz * wx - qx * wz;
      J[5] = qx * wy - qy * wx;
      const float af = fabsf(f);
      const float wt = af <= a.huber ? 1.0f : a.huber / af;
      const double fd = (double)f, wd = (double)wt;
      int at_h = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double wj = wd * (double)J[i];
#pragma unroll
        for (int j = i; j < 6; ++j) {
          acc[at_h] += wj * (double)J[j];
          ++at_h;
        }
        acc[21 + i] += wj * fd;
      }
      acc[27] += (wd * fd) * fd;
      acc[28] += fd * fd;
      ++count;
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < ALIGN_SUMS; ++i) {
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
  if (threadIdx.x < ALIGN_ROW) {
    const int i = threadIdx.x;
    a.partial[((size_t)b * a.n_chunks + chunk) * ALIGN_ROW + i] = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i];
  }
}

__global__ __launch_bounds__(GS_WAVE) void tsdf_align_sum_kernel(const double* __restrict__ partial, int n_chunks,
                                                                 double* __restrict__ out) {
  const int i = threadIdx.x;
  if (i >= ALIGN_ROW) return;
  const double* __restrict__ p = partial + (size_t)blockIdx.x * n_chunks * ALIGN_ROW + i;
  double t = p[0];
  int c = 1;
  for (; c + ALIGN_SUM_BATCH <= n_chunks; c += ALIGN_SUM_BATCH) {     // the loads of a batch in flight together, the adds in order
    double v[ALIGN_SUM_BATCH];
#pragma unroll
    for (int j = 0; j < ALIGN_SUM_BATCH; ++j) v[j] = p[(size_t)(c + j) * ALIGN_ROW];
#pragma unroll
    for (int j = 0; j < ALIGN_SUM_BATCH; ++j) t = t + v[j];
  }
  for (; c < n_chunks; ++c) t = t + p[(size_t)c * ALIGN_ROW];
  out[(size_t)blockIdx.x * ALIGN_ROW + i] = t;
}

__global__ __launch_bounds__(GS_WAVE) void tsdf_align_step_kernel(const double* __restrict__ out, double* __restrict__ pose,
                                                                  int B, double lam_rel, double lam_abs, double min_count,
                                                                  double* __restrict__ trace) {
  const int b = blockIdx.x * GS_WAVE + threadIdx.x;
  if (b >= B) return;
  const double* __restrict__ row = out + (size_t)b * ALIGN_ROW;
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

bool align_dims_ok(int nx, int ny, int nz) {
  return nx >= 2 && nx <= 1024 && ny >= 2 && ny <= 1024 && nz >= 2 && nz <= 1024;
}

// sampled pixels of an h x w image at `stride`, or -1 for sizes the entry points refuse
long long align_samples(int h, int w, int stride) {
  if (h < 1 || w < 1 || stride < 1 || (long long)h * w > (1LL << 30)) return -1;
  return (long long)gs_cdiv(h, stride) * gs_cdiv(w, stride);
}

}  // namespace

extern "C" int gs_tsdf_align_chunk(void) { return ALIGN_CHUNK; }

extern "C" size_t gs_tsdf_align_workspace_bytes(int n_poses, int h, int w, int stride) {
  const long long n = align_samples(h, w, stride);
  if (n_poses < 0 || n < 0) return 0;
  const long long chunks = (n + ALIGN_CHUNK - 1) / ALIGN_CHUNK;
  if ((long long)n_poses * chunks > 0x7fffffffLL) return 0;
  return (size_t)n_poses * (size_t)chunks * ALIGN_ROW * sizeof(double);
}

extern "C" int gs_tsdf_align_system(const float* tsdf, const float* weight, int nx, int ny, int nz, const float* depth,
                                    const int* frame, const double* pose, int n_poses, int k, int h, int w, int stride,
                                    float fx, float fy, float cx, float cy, float lo_x, float lo_y, float lo_z,
                                    float voxel, float max_depth, float min_weight, float huber, void* workspace,
                                    double* out, gs_stream_t stream) {
  GS_REQUIRE(align_dims_ok(nx, ny, nz), "tsdf_align_system: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
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
  const long long chunks = (n + ALIGN_CHUNK - 1) / ALIGN_CHUNK;
  GS_REQUIRE((long long)n_poses * chunks <= 0x7fffffffLL, "tsdf_align_system: %d poses of %lld chunks are too many for one launch",
             n_poses, chunks);
  GS_REQUIRE(tsdf && weight && depth && frame && pose && workspace && out, "tsdf_align_system: null pointer");
  AlignArgs a;
  a.tsdf = tsdf; a.weight = weight; a.depth = depth; a.frame = frame; a.pose = pose; a.partial = (double*)workspace;
  a.ny = ny; a.nz = nz;
  a.topx = (float)(nx - 1); a.topy = (float)(ny - 1); a.topz = (float)(nz - 1);
  a.lox = lo_x; a.loy = lo_y; a.loz = lo_z; a.voxel = voxel;
  a.k = k; a.h = h; a.w = w; a.stride = stride;
  a.sw = gs_cdiv(w, stride);
  a.n_samples = (int)n; a.n_chunks = (int)chunks;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
  a.max_depth = max_depth; a.min_weight = min_weight; a.huber = huber;
  GS_TIMING_PRE();
  tsdf_align_system_kernel<<<(unsigned)(n_poses * chunks), ALIGN_THREADS, 0, (hipStream_t)stream>>>(a);
  GS_CHECK_LAUNCH("tsdf_align_system");
  tsdf_align_sum_kernel<<<(unsigned)n_poses, GS_WAVE, 0, (hipStream_t)stream>>>(a.partial, a.n_chunks, out);
  GS_CHECK_LAUNCH("tsdf_align_sum");
  return GS_OK;
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
