// End-of-run trajectory evaluation in fp64 (reference src/slam.py:313-365): the camera-to-world poses of every frame
// from the filled world-to-camera trajectory, the moments of the Umeyama Sim(3) alignment and the APE statistics of the
// translation part.  Contracts: include/goslam_hip.h (gs_traj_world, gs_ape_moments, gs_ape_stats);
// tests/traj_eval_restatement.py restates them on the CPU in the same order.
//
// Every reduction has one fixed order, no float atomics: thread t of block b owns frame 256 b + t; the block's 256
// values meet in an LDS tree (stride 128, 64, ... 1); a single-block kernel then adds the block results b = t, t + 256,
// ... in ascending order per thread and runs the same tree.  Two runs give identical bits.
#include "common.h"

#include <math.h>

namespace {

constexpr int TE_BLOCK = 256;
constexpr int TE_NV = 10;                    // widest reduction: 9 cross products + the variance sum

enum { TE_ADD = 0, TE_MIN = 1, TE_MAX = 2 };

__device__ __forceinline__ double te_op(int op, double a, double b) {
  return op == TE_ADD ? __dadd_rn(a, b) : (op == TE_MIN ? fmin(a, b) : fmax(a, b));
}

// slots [0, n_add) are sums, slot n_add a minimum, slot n_add + 1 a maximum (when nv reaches that far)
template <int NV>
__device__ __forceinline__ void te_block_tree(double (*red)[TE_BLOCK], const double (&v)[NV], int n_add) {
  for (int a = 0; a < NV; ++a) red[a][threadIdx.x] = v[a];
  __syncthreads();
  for (int w = TE_BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int a = 0; a < NV; ++a) {
        const int op = a < n_add ? TE_ADD : (a == n_add ? TE_MIN : TE_MAX);
        red[a][threadIdx.x] = te_op(op, red[a][threadIdx.x], red[a][threadIdx.x + w]);
      }
    __syncthreads();
  }
}

template <int NV>
__device__ __forceinline__ void te_gather_parts(const double* __restrict__ part, int nblk, double (&v)[NV], int n_add) {
  for (int a = 0; a < NV; ++a) v[a] = a < n_add ? 0.0 : (a == n_add ? INFINITY : -INFINITY);
  for (int b = threadIdx.x; b < nblk; b += TE_BLOCK)
    for (int a = 0; a < NV; ++a) {
      const int op = a < n_add ? TE_ADD : (a == n_add ? TE_MIN : TE_MAX);
      v[a] = te_op(op, v[a], part[(size_t)b * NV + a]);
    }
}

// p + w uv + q x uv with uv = 2 (q x p): the rotation lietorch applies (not normalised), every operation rounded
__device__ __forceinline__ void te_qrot(const double q[4], const double p[3], double o[3]) {
  double c[3] = {__dsub_rn(__dmul_rn(q[1], p[2]), __dmul_rn(q[2], p[1])),
                 __dsub_rn(__dmul_rn(q[2], p[0]), __dmul_rn(q[0], p[2])),
                 __dsub_rn(__dmul_rn(q[0], p[1]), __dmul_rn(q[1], p[0]))};
  double uv[3] = {__dadd_rn(c[0], c[0]), __dadd_rn(c[1], c[1]), __dadd_rn(c[2], c[2])};
  double x[3] = {__dsub_rn(__dmul_rn(q[1], uv[2]), __dmul_rn(q[2], uv[1])),
                 __dsub_rn(__dmul_rn(q[2], uv[0]), __dmul_rn(q[0], uv[2])),
                 __dsub_rn(__dmul_rn(q[0], uv[1]), __dmul_rn(q[1], uv[0]))};
  for (int a = 0; a < 3; ++a) o[a] = __dadd_rn(__dadd_rn(p[a], __dmul_rn(q[3], uv[a])), x[a]);
}

// ------------------------------------------------------------------------------------------- gs_traj_world -------
__global__ __launch_bounds__(TE_BLOCK) void te_world_kernel(const float* __restrict__ w2c, const float* __restrict__ comp,
                                                            int n, double* __restrict__ tq, double* __restrict__ mat) {
  const int i = blockIdx.x * TE_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float* p = w2c + (size_t)i * 7;
  const double t[3] = {(double)p[0], (double)p[1], (double)p[2]};
  const double qi[4] = {-(double)p[3], -(double)p[4], -(double)p[5], (double)p[6]};   // inverse rotation
  double r[3];
  te_qrot(qi, t, r);
  const double ti[3] = {-r[0], -r[1], -r[2]};                                        // inverse translation
  const double ct[3] = {(double)comp[0], (double)comp[1], (double)comp[2]};
  const double a[4] = {(double)comp[3], (double)comp[4], (double)comp[5], (double)comp[6]};
  double rt[3];
  te_qrot(a, ti, rt);
  double o[7];
  for (int k = 0; k < 3; ++k) o[k] = __dadd_rn(ct[k], rt[k]);
  const double* b = qi;
  o[3] = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[3], b[0]), __dmul_rn(a[0], b[3])), __dmul_rn(a[1], b[2])),
                   __dmul_rn(a[2], b[1]));
  o[4] = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[3], b[1]), __dmul_rn(a[1], b[3])), __dmul_rn(a[2], b[0])),
                   __dmul_rn(a[0], b[2]));
  o[5] = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[3], b[2]), __dmul_rn(a[2], b[3])), __dmul_rn(a[0], b[1])),
                   __dmul_rn(a[1], b[0]));
  o[6] = __dsub_rn(__dsub_rn(__dsub_rn(__dmul_rn(a[3], b[3]), __dmul_rn(a[0], b[0])), __dmul_rn(a[1], b[1])),
                   __dmul_rn(a[2], b[2]));
  for (int k = 0; k < 7; ++k) tq[(size_t)i * 7 + k] = o[k];
  double* m = mat + (size_t)i * 16;
  for (int col = 0; col < 3; ++col) {
    const double e[3] = {col == 0 ? 1.0 : 0.0, col == 1 ? 1.0 : 0.0, col == 2 ? 1.0 : 0.0};
    double c[3];
    te_qrot(o + 3, e, c);
    for (int row = 0; row < 3; ++row) m[4 * row + col] = c[row];
  }
  for (int row = 0; row < 3; ++row) m[4 * row + 3] = o[row];
  m[12] = 0.0; m[13] = 0.0; m[14] = 0.0; m[15] = 1.0;
}

// ------------------------------------------------------------------------------------------- gs_ape_moments ------
// second == 0: (count, sum est xyz, sum ref xyz); second == 1: the centred products (ref - mr)(est - me)^T, row-major
// with the reference along the rows, and sum |est - me|^2.  means = me then mr.
__global__ __launch_bounds__(TE_BLOCK) void te_moment_sums_kernel(const double* __restrict__ est,
                                                                  const double* __restrict__ ref,
                                                                  const unsigned char* __restrict__ mask, int n,
                                                                  const double* __restrict__ means,
                                                                  double* __restrict__ part) {
  __shared__ double red[TE_NV][TE_BLOCK];
  double v[TE_NV] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int i = blockIdx.x * TE_BLOCK + threadIdx.x;
  if (i < n && (!mask || mask[i])) {
    const double e[3] = {est[3 * (size_t)i], est[3 * (size_t)i + 1], est[3 * (size_t)i + 2]};
    const double r[3] = {ref[3 * (size_t)i], ref[3 * (size_t)i + 1], ref[3 * (size_t)i + 2]};
    if (!means) {
      v[0] = 1.0;
      for (int a = 0; a < 3; ++a) {
        v[1 + a] = e[a];
        v[4 + a] = r[a];
      }
    } else {
      double ec[3], rc[3];
      for (int a = 0; a < 3; ++a) {
        ec[a] = __dsub_rn(e[a], means[a]);
        rc[a] = __dsub_rn(r[a], means[3 + a]);
      }
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) v[3 * a + b] = __dmul_rn(rc[a], ec[b]);
      v[9] = __dadd_rn(__dadd_rn(__dmul_rn(ec[0], ec[0]), __dmul_rn(ec[1], ec[1])), __dmul_rn(ec[2], ec[2]));
    }
  }
  te_block_tree<TE_NV>(red, v, TE_NV);
  if (threadIdx.x == 0)
    for (int a = 0; a < TE_NV; ++a) part[(size_t)blockIdx.x * TE_NV + a] = red[a][0];
}

__global__ __launch_bounds__(TE_BLOCK) void te_moment_final_kernel(const double* __restrict__ part, int nblk, int second,
                                                                   double* __restrict__ out) {
  __shared__ double red[TE_NV][TE_BLOCK];
  double v[TE_NV];
  te_gather_parts<TE_NV>(part, nblk, v, TE_NV);
  te_block_tree<TE_NV>(red, v, TE_NV);
  if (threadIdx.x != 0) return;
  if (!second) {
    const double cnt = red[0][0];
    out[0] = cnt;
    for (int a = 0; a < 6; ++a) out[1 + a] = cnt > 0.0 ? __ddiv_rn(red[1 + a][0], cnt) : 0.0;
  } else {
    const double cnt = out[0];
    for (int a = 0; a < 10; ++a) out[7 + a] = cnt > 0.0 ? __ddiv_rn(red[a][0], cnt) : 0.0;
  }
}

// ------------------------------------------------------------------------------------------- gs_ape_stats --------
constexpr int TS_NV = 5;                     // count, sum e, sum e^2 | min | max

__global__ __launch_bounds__(TE_BLOCK) void te_error_kernel(const double* __restrict__ est, const double* __restrict__ ref,
                                                            const unsigned char* __restrict__ mask,
                                                            const double* __restrict__ sim, int n,
                                                            double* __restrict__ err, double* __restrict__ part) {
  __shared__ double red[TS_NV][TE_BLOCK];
  double v[TS_NV] = {0.0, 0.0, 0.0, INFINITY, -INFINITY};
  const int i = blockIdx.x * TE_BLOCK + threadIdx.x;
  if (i < n) {
    double e = -1.0;                         // frames outside the mask carry -1
    if (!mask || mask[i]) {
      const double x[3] = {est[3 * (size_t)i], est[3 * (size_t)i + 1], est[3 * (size_t)i + 2]};
      double d[3];
      for (int a = 0; a < 3; ++a) {
        const double p = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(sim[3 * a], x[0]), __dmul_rn(sim[3 * a + 1], x[1])),
                                             __dmul_rn(sim[3 * a + 2], x[2])), sim[9 + a]);
        d[a] = __dsub_rn(ref[3 * (size_t)i + a], p);
      }
      e = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1])), __dmul_rn(d[2], d[2])));
      v[0] = 1.0;
      v[1] = e;
      v[2] = __dmul_rn(e, e);
      v[3] = e;
      v[4] = e;
    }
    err[i] = e;
  }
  te_block_tree<TS_NV>(red, v, 3);
  if (threadIdx.x == 0)
    for (int a = 0; a < TS_NV; ++a) part[(size_t)blockIdx.x * TS_NV + a] = red[a][0];
}

// stats = [rmse, mean, median, min, max, sse, std]; scratch = [count, lower middle, upper middle]
__global__ __launch_bounds__(TE_BLOCK) void te_stats_mid_kernel(const double* __restrict__ part, int nblk,
                                                                double* __restrict__ stats, double* __restrict__ scratch) {
  __shared__ double red[TS_NV][TE_BLOCK];
  double v[TS_NV];
  te_gather_parts<TS_NV>(part, nblk, v, 3);
  te_block_tree<TS_NV>(red, v, 3);
  if (threadIdx.x != 0) return;
  const double cnt = red[0][0];
  const double nan = __builtin_nan("");
  scratch[0] = cnt;
  scratch[1] = nan;
  scratch[2] = nan;
  stats[0] = cnt > 0.0 ? __dsqrt_rn(__ddiv_rn(red[2][0], cnt)) : nan;
  stats[1] = cnt > 0.0 ? __ddiv_rn(red[1][0], cnt) : nan;
  stats[2] = nan;
  stats[3] = cnt > 0.0 ? red[3][0] : nan;
  stats[4] = cnt > 0.0 ? red[4][0] : nan;
  stats[5] = red[2][0];
  stats[6] = nan;
}

// rank of frame i among the valid errors = #{j : e_j < e_i, or e_j == e_i and j < i}: a permutation of 0 .. count - 1,
// so exactly one frame owns each of the two middle ranks.  Also the centred squares for the standard deviation.
__global__ __launch_bounds__(TE_BLOCK) void te_rank_kernel(const double* __restrict__ err, int n,
                                                           const double* __restrict__ stats, double* __restrict__ scratch,
                                                           double* __restrict__ part) {
  __shared__ double red[1][TE_BLOCK];
  __shared__ double tile[TE_BLOCK];
  const int i = blockIdx.x * TE_BLOCK + threadIdx.x;
  const double e = i < n ? err[i] : -1.0;
  const bool valid = e >= 0.0;
  int rank = 0;
  for (int base = 0; base < n; base += TE_BLOCK) {
    const int j = base + threadIdx.x;
    tile[threadIdx.x] = j < n ? err[j] : -1.0;
    __syncthreads();
    const int m = min(TE_BLOCK, n - base);
    for (int k = 0; k < m; ++k) {
      const double f = tile[k];
      rank += (f >= 0.0 && (f < e || (f == e && base + k < i))) ? 1 : 0;
    }
    __syncthreads();
  }
  double v[1] = {0.0};
  if (valid && i < n) {
    const long long cnt = (long long)scratch[0];
    if (rank == (int)((cnt - 1) / 2)) scratch[1] = e;
    if (rank == (int)(cnt / 2)) scratch[2] = e;
    const double c = __dsub_rn(e, stats[1]);
    v[0] = __dmul_rn(c, c);
  }
  te_block_tree<1>(red, v, 1);
  if (threadIdx.x == 0) part[blockIdx.x] = red[0][0];
}

__global__ __launch_bounds__(TE_BLOCK) void te_stats_final_kernel(const double* __restrict__ part, int nblk,
                                                                  const double* __restrict__ scratch,
                                                                  double* __restrict__ stats) {
  __shared__ double red[1][TE_BLOCK];
  double v[1];
  te_gather_parts<1>(part, nblk, v, 1);
  te_block_tree<1>(red, v, 1);
  if (threadIdx.x != 0) return;
  const double cnt = scratch[0];
  if (cnt > 0.0) {
    stats[2] = __dmul_rn(0.5, __dadd_rn(scratch[1], scratch[2]));
    stats[6] = __dsqrt_rn(__ddiv_rn(red[0][0], cnt));
  }
}

}  // namespace

extern "C" size_t gs_traj_eval_workspace_bytes(int n) {
  if (n < 0) return 0;
  return ((size_t)(n > 0 ? gs_cdiv(n, TE_BLOCK) : 1) * TE_NV + 4) * sizeof(double);
}

extern "C" int gs_traj_world(const float* w2c, const float* compensate, int n, double* tq, double* mat,
                             gs_stream_t stream) {
  GS_REQUIRE(n >= 0, "traj_world: bad frame count");
  if (n == 0) return GS_OK;
  GS_REQUIRE(w2c && compensate && tq && mat, "traj_world: null pointer");
  GS_TIMING_PRE();
  te_world_kernel<<<gs_cdiv(n, TE_BLOCK), TE_BLOCK, 0, (hipStream_t)stream>>>(w2c, compensate, n, tq, mat);
  GS_CHECK_LAUNCH("traj_world");
  return GS_OK;
}

extern "C" int gs_ape_moments(const double* est, const double* ref, const unsigned char* mask, int n, double* moments,
                              void* workspace, size_t workspace_bytes, gs_stream_t stream) {
  GS_REQUIRE(n >= 0, "ape_moments: bad frame count");
  GS_REQUIRE(moments && workspace && (n == 0 || (est && ref)), "ape_moments: null pointer");
  if (workspace_bytes < gs_traj_eval_workspace_bytes(n)) {
    gs_set_error("ape_moments: workspace %zu < %zu bytes", workspace_bytes, gs_traj_eval_workspace_bytes(n));
    return GS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const int nblk = n > 0 ? gs_cdiv(n, TE_BLOCK) : 0;
  GS_TIMING_PRE();
  if (nblk > 0) {
    te_moment_sums_kernel<<<nblk, TE_BLOCK, 0, st>>>(est, ref, mask, n, nullptr, part);
    GS_CHECK_LAUNCH("ape_sums");
  }
  te_moment_final_kernel<<<1, TE_BLOCK, 0, st>>>(part, nblk, 0, moments);
  GS_CHECK_LAUNCH("ape_means");
  if (nblk > 0) {
    te_moment_sums_kernel<<<nblk, TE_BLOCK, 0, st>>>(est, ref, mask, n, moments + 1, part);
    GS_CHECK_LAUNCH("ape_cross");
  }
  te_moment_final_kernel<<<1, TE_BLOCK, 0, st>>>(part, nblk, 1, moments);
  GS_CHECK_LAUNCH("ape_cross_final");
  return GS_OK;
}

extern "C" int gs_ape_stats(const double* est, const double* ref, const unsigned char* mask, const double* sim, int n,
                            double* err, double* stats, void* workspace, size_t workspace_bytes, gs_stream_t stream) {
  GS_REQUIRE(n >= 0, "ape_stats: bad frame count");
  GS_REQUIRE(sim && stats && workspace && (n == 0 || (est && ref && err)), "ape_stats: null pointer");
  if (workspace_bytes < gs_traj_eval_workspace_bytes(n)) {
    gs_set_error("ape_stats: workspace %zu < %zu bytes", workspace_bytes, gs_traj_eval_workspace_bytes(n));
    return GS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nblk = n > 0 ? gs_cdiv(n, TE_BLOCK) : 0;
  double* scratch = (double*)workspace;      // [count, lower middle, upper middle, pad]
  double* part = scratch + 4;
  GS_TIMING_PRE();
  if (nblk > 0) {
    te_error_kernel<<<nblk, TE_BLOCK, 0, st>>>(est, ref, mask, sim, n, err, part);
    GS_CHECK_LAUNCH("ape_errors");
  }
  te_stats_mid_kernel<<<1, TE_BLOCK, 0, st>>>(part, nblk, stats, scratch);
  GS_CHECK_LAUNCH("ape_stats_mid");
  if (nblk > 0) {
    te_rank_kernel<<<nblk, TE_BLOCK, 0, st>>>(err, n, stats, scratch, part);
    GS_CHECK_LAUNCH("ape_rank");
  }
  te_stats_final_kernel<<<1, TE_BLOCK, 0, st>>>(part, nblk, scratch, stats);
  GS_CHECK_LAUNCH("ape_stats_final");
  return GS_OK;
}
