// Dense fp64 Cholesky solve of the reduced camera system, on the device.
// Stands in for Eigen::SimplicialLLT on the host (reference: src/lib/droid_kernels.cu:1192-1213):
//   L = A;  diag(L) += ep + lm * diag(L);  LLT;  x = solve(b);  failure (pivot <= 0) => x = 0.
//
// Three paths, chosen by n (chol_dispatch; gs_chol_solve can force any of them):
//   chol_small_kernel (n <= 192)   : one launch of one workgroup, the packed lower triangle of [A; b^T] in LDS
//   chol_mid_kernel   (n <= MID_N) : one launch of one workgroup, the head stages' trailing matrix in HBM / L2, the last
//                                    <= 192 columns in LDS
//   blocked (any n)                : the (n x n) matrix in HBM / L2 as a dense row-major fp64 array whose LOWER triangle is
//                                    valid; right-looking, NB = 32, one launch per panel:
//     chol_panel_kernel   : panel 0, with the damping folded in -- every workgroup (one wave) re-factors the 32x32 diagonal
//                           block (cheaper than a dependent launch) and solves 64 rows of the panel
//     chol_step_kernel    : panel k + 1 AND the trailing update of panel k in the same launch: the panel workgroups apply
//                           panel k's rank-32 update to their own 32 columns themselves (v_mfma_f64_16x16x4), the tile
//                           workgroups update what lies beyond those columns (64x64 tiles, operands in LDS)
//     chol_back_pair_kernel / chol_back_block_kernel : backward substitution, two 64-wide blocks per launch, one for an odd
//                           last block (b rides along as row n of the factorisation, so the forward substitution is free);
//                           writes fp32 dx
//   1 launch per panel + 1 per 128 unknowns; 6P = 1194 (global BA) is 38 + 10 launches, 0.85 ms.  tools/chol_bench.hip
//   times the dispatched path against the blocked one and reads the phase stamps (CHOL_TIMING).
#include "common.h"

namespace {

constexpr int NB = 32;     // panel width
constexpr int PR = 64;     // panel rows per workgroup (one wave)
constexpr int TT = 64;     // trailing tile edge
constexpr int SB = 64;     // substitution block

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned int lo = __builtin_amdgcn_readlane((int)(u & 0xffffffffu), lane);
  const unsigned int hi = __builtin_amdgcn_readlane((int)(u >> 32), lane);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// sqrt and reciprocal sqrt of a pivot from v_rsq_f64 + two coupled Goldschmidt steps (full fp64
// accuracy, ~12 dependent FMAs instead of the ~35-instruction sqrt + divide sequences).
__device__ __forceinline__ void sqrt_rsqrt(double x, double& s, double& rs) {
  const double r = __builtin_amdgcn_rsq(x);
  double g = x * r, h = 0.5 * r;
  double e = fma(-g, h, 0.5);
  g = fma(g, e, g); h = fma(h, e, h);
  e = fma(-g, h, 0.5);
  g = fma(g, e, g); h = fma(h, e, h);
  s = g; rs = h + h;
}

constexpr int DS = NB + 2;  // row stride of the factored diagonal block in LDS: even, so that a row's entries can be read in
                            // 16-byte pairs (every read of it is a broadcast: the stride needs no bank padding)

// The 32x32 diagonal factorisation of a panel by ONE wave, lane i = row i (32 doubles in registers), LEFT-looking:
//   step j:  s_i = a_i[j] - sum_{t<j} L[i][t] L[j][t]   (the lane's own finished entries x row j of L)
//            L[j][j] = sqrt(s_j),  L[i][j] = s_i / L[j][j]  (i > j)
// Row j of L is read from LDS as broadcasts, two entries per ds_read_b128 -- every lane files L[i][j] there as soon as it
// has it -- and only the pivot and the newest entry of the row travel through v_readlane.  The right-looking form this
// replaces (rounds 3-5) updated every remaining column after every pivot with the column entry fetched by two v_readlane
// per (pivot, column): 496 x (2 readlane + multiply-add + lane mask) = ~3000 instructions behind each other, ~10 us of the
// panel kernel's 21.5 and, 38 panels deep, the longest link of the 6P = 1194 solve's dependency chain; here ~500
// multiply-adds and ~250 LDS reads.
// Lanes >= nb carry identity rows.  Leaves L11 in D (lower triangle; lanes >= NB store nothing) and 1 / diag in Dinv.
__device__ __forceinline__ void panel_diag_factor(double (&a)[NB], int nb, int lane, bool& bad, double (*D)[DS],
                                                  double* Dinv) {
  typedef double double2v __attribute__((ext_vector_type(2)));
  double mydiag = 1.0;
  // Row j's entries L[j][t], t <= j - 2, are requested one step AHEAD (they were all filed by step j - 2), and the one entry
  // step j - 1 has just produced, L[j][j-1], comes from lane j through v_readlane: read where it is used, every step waited
  // an LDS round trip for a row whose last entry had only just been written (32 exposed round trips of a lone wave).
  // (One wave: its LDS operations retire in order, and every access goes through D with a lane-dependent index, so the
  // compiler keeps the stores of a step in front of the later steps' reads.)
  double2v cur[NB / 2], nxt[NB / 2];
#pragma unroll
  for (int q = 0; q < NB / 2; ++q) nxt[q] = double2v{0.0, 0.0};
#pragma unroll
  for (int j = 0; j < NB; ++j) {
#pragma unroll
    for (int q = 0; q < NB / 2; ++q) cur[q] = nxt[q];
    if (j + 1 < NB) {                       // row j + 1, entries t <= j - 1 (columns filed by the steps before this one)
#pragma unroll
      for (int q = 0; 2 * q <= j - 1; ++q) nxt[q] = *reinterpret_cast<const double2v*>(&D[j + 1][2 * q]);
    }
    double s0 = a[j], s1 = 0.0;
#pragma unroll
    for (int t = 0; t + 1 <= j - 2; t += 2) {
      s0 = fma(-a[t], cur[t >> 1][0], s0);
      s1 = fma(-a[t + 1], cur[t >> 1][1], s1);
    }
    if (j >= 2 && ((j - 2) & 1) == 0) s0 = fma(-a[j - 2], cur[(j - 2) >> 1][0], s0);   // (an unpaired last entry t = j - 2)
    if (j >= 1) s1 = fma(-a[j - 1], readlane_f64(a[j - 1], j), s1);                    // L[j][j-1], from lane j itself
    const double s = s0 + s1;
    const double piv = readlane_f64(s, j);
    if (j < nb && !(piv > 0.0) && piv == piv) bad = true;   // pivot <= 0 (NaN falls through like Eigen)
    double dj, rdj;                         // (rsq + two Goldschmidt steps: ~12 dependent FMAs instead of sqrt + divide)
    sqrt_rsqrt(piv, dj, rdj);
    a[j] = lane == j ? dj : (lane > j ? s * rdj : 0.0);
    if (lane == j) mydiag = dj;
    if (lane < NB) D[lane][j] = a[j];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < NB) Dinv[lane] = 1.0 / mydiag;
}

// one panel row: x = a L11^-T (forward substitution against the factored diagonal block in LDS): two partial sums per
// entry and row c of L read as 16-byte broadcasts, like the diagonal factor's inner loop (one sum fed by one 8-byte read
// per term was a dependent chain of 2 c instructions per entry: 6.5 us of a 22 us panel step in tools/chol_bench's stamps)
__device__ __forceinline__ void panel_row_solve(double (&x)[NB], int nb, double (*D)[DS], const double* Dinv) {
  typedef double double2v __attribute__((ext_vector_type(2)));
  // row c + 1 of L is requested BEFORE entry c's arithmetic (its reads depend on nothing the solve computes): consumed where
  // they are read, every entry waited one LDS round trip for its own row -- 32 exposed round trips of a lone wave
  double2v cur[NB / 2], nxt[NB / 2];
#pragma unroll
  for (int q = 0; q < NB / 2; ++q) nxt[q] = double2v{0.0, 0.0};           // (row 0: entry 0 has no terms)
#pragma unroll
  for (int c = 0; c < NB; ++c) {
#pragma unroll
    for (int q = 0; q < NB / 2; ++q) cur[q] = nxt[q];
    if (c + 1 < NB) {
#pragma unroll
      for (int q = 0; 2 * q < c + 1; ++q) nxt[q] = *reinterpret_cast<const double2v*>(&D[c + 1][2 * q]);
    }
    if (c < nb) {
      double s0 = x[c], s1 = 0.0;
#pragma unroll
      for (int t = 0; t + 1 < c; t += 2) {
        s0 = fma(-x[t], cur[t >> 1][0], s0);
        s1 = fma(-x[t + 1], cur[t >> 1][1], s1);
      }
      if (c & 1) s0 = fma(-x[c - 1], cur[c >> 1][0], s0);
      x[c] = (s0 + s1) * Dinv[c];
    }
  }
}

// Factor the diagonal block [k0,k0+nb) (every workgroup redundantly -- cheaper than a dependent
// launch) and compute L21 = A21 * L11^-T for this workgroup's PR rows.
// `damp` (panel 0): the solve's damping, diag += ep + lm * diag, applied on the way -- by lane r to the diagonal block's
// entry it holds, by every row's lane to its own diagonal entry further down (nothing else in this launch touches those) --
// and the failure flag reset (chol_step_kernel only ever raises it).
__global__ __launch_bounds__(64) void chol_panel_kernel(double* __restrict__ A, double* __restrict__ bvec, int n, int k0,
                                                        int32_t* fail_flag, int damp = 0, double lm = 0.0, double ep = 0.0) {
  __shared__ __attribute__((aligned(16))) double D[NB][DS];
  __shared__ double Dinv[NB];
  const int lane = threadIdx.x;
  const int nb = min(NB, n - k0);
  double a[NB];
  {
    const int r = lane & (NB - 1);
    const bool live = (lane < NB) && (r < nb);
    const double* Ar = A + (size_t)(k0 + (live ? r : 0)) * n + k0;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      double v = (live && c <= r && c < nb) ? Ar[c] : 0.0;
      if (damp && live && c == r) v = v + (ep + lm * v);
      if (!live && c == r) v = 1.0;            // identity padding keeps the recurrence well-defined
      a[c] = v;
    }
  }
  const int row = k0 + nb + blockIdx.x * PR + lane;
  double own_diag = 0.0;
  if (damp && row < n) own_diag = A[(size_t)row * n + row];
  bool bad = false;
  panel_diag_factor(a, nb, lane, bad, D, Dinv);
  __syncthreads();
  if (blockIdx.x == 0) {
    if (lane < nb) {
      double* Ar = A + (size_t)(k0 + lane) * n + k0;
#pragma unroll
      for (int c = 0; c < NB; ++c)
        if (c <= lane) Ar[c] = a[c];
    }
    if (lane == 0 && (bad || damp)) *fail_flag = bad ? 1 : 0;
  }
  if (damp && row < n) A[(size_t)row * n + row] = own_diag + (ep + lm * own_diag);
  // panel rows; row n is b^T (round 4: b rides along as an extra row of the matrix, so the forward substitution
  // L y = b falls out of the factorisation -- the single-workgroup forward sweep cost 0.75 ms at 6P = 1194)
  if (row <= n) {
    double x[NB];
    double* Ar = row < n ? A + (size_t)row * n + k0 : bvec + k0;
#pragma unroll
    for (int c = 0; c < NB; ++c) x[c] = (c < nb) ? Ar[c] : 0.0;
    panel_row_solve(x, nb, D, Dinv);
#pragma unroll
    for (int c = 0; c < NB; ++c)
      if (c < nb) Ar[c] = x[c];
  }
}

// A22[r][c] -= sum_k L21[r][k] L21[c][k] over ONE 64x64 lower tile `t` of the matrix that starts at row / column s0 (the
// b row, row n, included), L21 = columns [k0, k0 + nb); operands staged in LDS (Lr, Lc: [TT][NB + 1] each).
__device__ __forceinline__ void trail_tile(double* __restrict__ A, double* __restrict__ bvec, int n, int k0, int nb, int s0,
                                           int t, double (*Lr)[NB + 1], double (*Lc)[NB + 1]) {
  // decode (ti,tj), tj <= ti, from the flat lower-triangular tile index
  int ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  while (ti * (ti + 1) / 2 > t) --ti;
  const int tj = t - ti * (ti + 1) / 2;
  const int r0 = s0 + ti * TT, c0 = s0 + tj * TT;
  const int tid = threadIdx.x;
  // operands: all sixteen loads of a thread requested before the first LDS write (one load, one wait, one write per
  // element was 16 dependent round trips at the head of every tile); rows past the end read a valid address and are
  // zeroed by a select; row n = b^T lives in bvec
  {
    constexpr int PER = TT * NB / 256;
    double vr[PER], vc[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = tid + 256 * u, r = idx / NB, k = idx % NB;
      const int rr = r0 + r, cc = c0 + r;
      const double* pr = rr < n ? A + (size_t)rr * n + (k0 + k) : bvec + (k0 + k);
      const double* pc = A + (size_t)min(cc, n - 1) * n + (k0 + k);
      vr[u] = *pr;
      vc[u] = *pc;
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = tid + 256 * u, r = idx / NB, k = idx % NB;
      Lr[r][k] = (r0 + r <= n && k < nb) ? vr[u] : 0.0;
      Lc[r][k] = (c0 + r < n && k < nb) ? vc[u] : 0.0;
    }
  }
  __syncthreads();
  const int tr = (tid / 16) * 4, tc = (tid % 16) * 4;
  // the tile's current values are requested before the products (they were 16 load - wait - store round trips behind them)
  double old[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = min(r0 + tr + i, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = min(c0 + tc + j, n - 1);
      old[i][j] = r < n ? A[(size_t)r * n + c] : bvec[c];
    }
  }
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
#pragma unroll 4
  for (int k = 0; k < NB; ++k) {
    double a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { a[i] = Lr[tr + i][k]; b[i] = Lc[tc + i][k]; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + tr + i;
    if (r > n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + tc + j;
      if (c <= r && c < n) {
        if (r < n) A[(size_t)r * n + c] = old[i][j] - acc[i][j];
        else bvec[c] = old[i][j] - acc[i][j];
      }
    }
  }
}

#ifdef CHOL_TIMING   // tools/chol_bench.hip: where a step's panel wave spends its time (workgroup 0, summed over the steps)
__device__ long long g_step_t[8];
#define STEP_T0() long long st_last = wall_clock64()
#define STEP_T(i) do { const long long t_now = wall_clock64(); if (blockIdx.x == 0 && threadIdx.x == 0) g_step_t[i] += t_now - st_last; st_last = t_now; } while (0)
#else
#define STEP_T0() do { } while (0)
#define STEP_T(i) do { } while (0)
#endif

// ONE launch per panel step (round 6): the trailing update of panel kp and the factorisation of panel kp + NB side by
// side.  Panel and trailing update as two launches (38 times at 6P = 1194) were a chain of 76 kernels each bound by
// its own latency (launch, a dependent load round trip, the 32-pivot chain, a store round trip); but panel kp + NB only
// needs panel kp's rank-32 update on ITS OWN 32 columns, so:
//   workgroups [0, n_panel)        factor panel c1 = kp + NB after applying that PENDING update to the diagonal block and to
//                                  their own 64 rows themselves (Lp Lp^T and Lr Lp^T on v_mfma_f64_16x16x4, operands and
//                                  results through LDS: lane = row layouts on both sides of the matrix cores), one wave each;
//   workgroups [n_panel, ...)      the trailing update of panel kp on what lies right of / below panel c1 (origin s1 = c1 +
//                                  nb1): tiles that neither read nor write panel c1's columns.
// Nothing in one role depends on the other inside the launch; the kernel boundary orders step kp after step kp - NB.
__global__ __launch_bounds__(256) void chol_step_kernel(double* __restrict__ A, double* __restrict__ bvec, int n, int kp,
                                                        int n_panel, int32_t* fail_flag) {
  extern __shared__ __attribute__((aligned(16))) double step_lds[];
  const int c1 = kp + NB, nb1 = min(NB, n - c1), s1 = c1 + nb1;
  if ((int)blockIdx.x >= n_panel) {
    double (*Lr)[NB + 1] = reinterpret_cast<double (*)[NB + 1]>(step_lds);
    double (*Lc)[NB + 1] = Lr + TT;
    trail_tile(A, bvec, n, kp, NB, s1, (int)blockIdx.x - n_panel, Lr, Lc);
    return;
  }
  // the panel role: wave 0 owns the rows (lane = row); waves 1-3 only help with the pending-update products
  const int wv = threadIdx.x >> 6;
  STEP_T0();
  typedef double double4v __attribute__((ext_vector_type(4)));
  double (*D)[DS] = reinterpret_cast<double (*)[DS]>(step_lds);                // [NB]  (first: 16-byte aligned rows)
  double (*Lp)[NB + 1] = reinterpret_cast<double (*)[NB + 1]>(D + NB);          // [NB]  rows c1 .. of panel kp's L21
  double (*Lr)[NB + 1] = Lp + NB;                                               // [PR]  this workgroup's rows of it
  double (*U)[NB + 1] = Lr + PR;                                                // [PR]  products, lane = row on the way out
  double (*UD)[NB + 1] = U + PR;                                                // [NB]  ... of the diagonal block
  double* Dinv = reinterpret_cast<double*>(UD + NB);                            // [NB]
  const int lane = threadIdx.x & 63;
  auto lds_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // ---- everything this wave reads from memory is requested up front: diagonal block row + its L21 row (lanes < NB), own
  // row of the panel's columns + its L21 row
  double a[NB], lp[NB], x[NB], lr[NB];
  const int row = s1 + (int)blockIdx.x * PR + lane;
  const bool has_row = row <= n;
  double* Xr = row < n ? A + (size_t)row * n + c1 : bvec + c1;
  if (wv == 0) {
    const int r = lane & (NB - 1);
    const bool live = (lane < NB) && (r < nb1);
    const double* Ar = A + (size_t)(c1 + (live ? r : 0)) * n;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      double v = (live && c <= r && c < nb1) ? Ar[c1 + c] : 0.0;
      if (!live && c == r) v = 1.0;            // identity padding keeps the recurrence well-defined
      a[c] = v;
      lp[c] = live ? Ar[kp + c] : 0.0;
    }
    const double* Lrow = row < n ? A + (size_t)row * n + kp : bvec + kp;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      x[c] = (has_row && c < nb1) ? Xr[c] : 0.0;
      lr[c] = has_row ? Lrow[c] : 0.0;
    }
    if (lane < NB) {
#pragma unroll
      for (int c = 0; c < NB; ++c) Lp[lane][c] = lp[c];
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) Lr[lane][c] = lr[c];
  }
  __syncthreads();
  STEP_T(0);                                      // loads arrived + staged
  // ---- the pending rank-32 update, eleven 16 x 16 x 32 products dealt to the workgroup's four waves (the fp64 matrix rate of
  // this part equals its vector rate: one wave alone spent 2.7 of the step's 21 us here):
  //   wave 0: the diagonal block's lower tiles (0,0) (1,0) (1,1), sum_k Lp[i][k] Lp[c][k] -> UD
  //   waves 1-3: the rows' eight tiles, sum_k Lr[row][k] Lp[c][k] -> U, three / three / two each
  const int m16 = lane & 15, k4 = lane >> 4;
  if (wv == 0) {
    double4v acc00 = {0.0, 0.0, 0.0, 0.0}, acc10 = acc00, acc11 = acc00;
#pragma unroll
    for (int kb = 0; kb < NB / 4; ++kb) {
      const double p0 = Lp[m16][4 * kb + k4], p1 = Lp[16 + m16][4 * kb + k4];
      acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(p0, p0, acc00, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(p1, p0, acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(p1, p1, acc11, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      UD[k4 + 4 * q][m16] = acc00[q];
      UD[16 + k4 + 4 * q][m16] = acc10[q];
      UD[16 + k4 + 4 * q][16 + m16] = acc11[q];
    }
  } else {
    const int first = 3 * (wv - 1), count = wv == 3 ? 2 : 3;      // tile id = 2 ti + tj
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      if (u < count) {
        const int id = first + u, ti = id >> 1, tj = id & 1;
        double4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kb = 0; kb < NB / 4; ++kb)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Lr[16 * ti + m16][4 * kb + k4], Lp[16 * tj + m16][4 * kb + k4], acc, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) U[16 * ti + k4 + 4 * q][16 * tj + m16] = acc[q];
      }
    }
  }
  __syncthreads();
  if (wv != 0) return;
  if (lane < NB) {
#pragma unroll
    for (int c = 0; c < NB; ++c)
      if (c <= lane) a[c] -= UD[lane][c];
  }
#pragma unroll
  for (int c = 0; c < NB; ++c) x[c] -= U[lane][c];
  STEP_T(1);                                      // pending updates
  // ---- the panel itself, as chol_panel_kernel
  bool bad = false;
  panel_diag_factor(a, nb1, lane, bad, D, Dinv);
  lds_sync();
  STEP_T(2);                                      // diagonal factor
  if (blockIdx.x == 0) {
    if (lane < nb1) {
      double* Ar = A + (size_t)(c1 + lane) * n + c1;
#pragma unroll
      for (int c = 0; c < NB; ++c)
        if (c <= lane) Ar[c] = a[c];
    }
    if (lane == 0 && bad) *fail_flag = 1;
  }
  if (has_row) {
    panel_row_solve(x, nb1, D, Dinv);
    STEP_T(3);                                    // row solve
#pragma unroll
    for (int c = 0; c < NB; ++c)
      if (c < nb1) Xr[c] = x[c];
  }
  STEP_T(4);                                      // stores issued
}

// Backward substitution L^T x = y of ONE 64-wide block at k0 (y = L^-1 b is already in b: it rode along as row n of the
// factorisation): every workgroup solves the block's triangle redundantly in wave 0 (registers, v_readlane broadcasts:
// lane j holds COLUMN j), then the workgroups share the update of the columns left of the block, y[c] -= sum_r
// L[k0 + r][c] x[r] -- consecutive threads read consecutive c, so the loads coalesce.  The blocked path launches it on one
// workgroup for the block at 0 that chol_back_pair_kernel leaves when the number of blocks is odd.
__global__ __launch_bounds__(256) void chol_back_block_kernel(const double* __restrict__ L, double* __restrict__ b, int n,
                                                              int k0, float* __restrict__ dx, const int32_t* fail_flag,
                                                              int32_t* fail_count) {
  __shared__ double xs[SB];
  const int tid = threadIdx.x;
  const int nb = min(SB, n - k0);
  if (*fail_flag) {   // reference: zero update on failure (droid_kernels.cu:1207-1210)
    if (blockIdx.x == 0) {
      for (int i = tid; i < nb; i += 256) dx[k0 + i] = 0.0f;
      if (tid == 0 && k0 == 0) *fail_count += 1;
    }
    return;
  }
  // Everything is requested before anything is computed, the triangle first (the memory counter retires in order: what is
  // waited for first must be asked for first): column j = lane of the block for the solve -- every wave asks, only wave 0
  // solves; a load behind the `tid < 64` branch would be issued after the update's -- then this thread's column of the
  // update, y[c] -= sum_r L[k0 + r][c] x[r], which needs nothing of x (behind the solve and the barrier it was a second
  // exposed round trip of every launch).
  const int j = tid & 63;
  const bool live = j < nb;
  const double dg = L[(size_t)(k0 + min(j, nb - 1)) * n + k0 + min(j, nb - 1)];
  double yv = b[k0 + min(j, nb - 1)];
  double c_[SB];                          // column j of the block: L[k0+i][k0+j], i > j
#pragma unroll
  for (int i = 0; i < SB; ++i) c_[i] = L[(size_t)(k0 + min(i, nb - 1)) * n + k0 + min(j, nb - 1)];
  const int c = blockIdx.x * 256 + tid;
  const int cc = min(c, max(k0 - 1, 0));
  double v[SB];
#pragma unroll
  for (int u = 0; u < SB; ++u) v[u] = L[(size_t)(k0 + min(u, nb - 1)) * n + cc];
  const double bc = b[cc];
  if (tid < 64) {
    if (!live) yv = 0.0;
#pragma unroll
    for (int i = 0; i < SB; ++i)
      if (!(live && i > j && i < nb)) c_[i] = 0.0;
    const double inv_dg = live ? 1.0 / dg : 1.0;
#pragma unroll
    for (int i = SB - 1; i >= 0; --i) {
      const double xi = readlane_f64(yv * inv_dg, i);
      if (j == i) yv = xi;
      else if (j < i) yv -= c_[i] * xi;
    }
    xs[j] = yv;
    if (live && blockIdx.x == 0) dx[k0 + j] = (float)yv;      // (b[k0 ..] keeps y: the other workgroups still read it)
  }
  __syncthreads();
  if (c < k0) {
    // (a rolled two-row loop was 32 dependent round trips: most of this kernel's 15 us until round 6); the sums are formed in
    // the same order as before -- even rows, odd rows, then both
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int u = 0; u < SB; u += 2) {
      if (u < nb) s0 = fma(v[u], xs[u], s0);
      if (u + 1 < nb) s1 = fma(v[u + 1], xs[u + 1], s1);
    }
    b[c] = bc - (s0 + s1);
  }
}


// TWO 64-wide blocks per launch (round 6): the block at k_hi = k_lo + 64 (nb_hi <= 64 unknowns) and the full block at k_lo.
// Wave 0 of every workgroup solves the upper triangle, takes its solution out of the lower block's right-hand side
// (y_lo[j] -= sum_r L[k_hi + r][k_lo + j] x_hi[r], a 64 x 64 product: lane j = column, coalesced) and solves the lower
// triangle -- redundantly per workgroup, as the single-block kernel does; waves 1-3 then update the columns left of k_lo
// with both blocks' rows, 192 columns per workgroup.  Half the launches of the substitution, i.e. half of its kernel
// boundaries (each a launch gap and a first-touch round trip).
__global__ __launch_bounds__(256) void chol_back_pair_kernel(const double* __restrict__ L, double* __restrict__ b, int n,
                                                             int k_lo, float* __restrict__ dx, const int32_t* fail_flag,
                                                             int32_t* fail_count) {
  __shared__ double xs[2 * SB];                       // x of [k_lo, k_lo + 64 + nb_hi)
  const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
  const int k_hi = k_lo + SB, nb_hi = min(SB, n - k_hi);
  if (*fail_flag) {   // reference: zero update on failure (droid_kernels.cu:1207-1210)
    if (blockIdx.x == 0) {
      for (int i = tid; i < SB + nb_hi; i += 256) dx[k_lo + i] = 0.0f;
      if (tid == 0 && k_lo == 0) *fail_count += 1;
    }
    return;
  }
  if (wv == 0) {
    const bool live = j < nb_hi;
    const int jc = min(j, nb_hi - 1);
    // everything wave 0 needs, requested before anything is computed: upper triangle column j, the 64 x nb_hi block
    // between the two (column k_lo + j of rows k_hi ..), lower triangle column j, both right-hand sides
    const double dg_hi = L[(size_t)(k_hi + jc) * n + k_hi + jc], dg_lo = L[(size_t)(k_lo + j) * n + k_lo + j];
    double y_hi = b[k_hi + jc], y_lo = b[k_lo + j];
    double c_hi[SB], g[SB], c_lo[SB];
#pragma unroll
    for (int i = 0; i < SB; ++i) c_hi[i] = L[(size_t)(k_hi + min(i, nb_hi - 1)) * n + k_hi + jc];
#pragma unroll
    for (int i = 0; i < SB; ++i) g[i] = L[(size_t)(k_hi + min(i, nb_hi - 1)) * n + k_lo + j];
#pragma unroll
    for (int i = 0; i < SB; ++i) c_lo[i] = L[(size_t)(k_lo + i) * n + k_lo + j];
    if (!live) y_hi = 0.0;
    const double inv_hi = live ? 1.0 / dg_hi : 1.0, inv_lo = 1.0 / dg_lo;
#pragma unroll
    for (int i = SB - 1; i >= 0; --i) {               // upper triangle; x_hi[i] also leaves the lower right-hand side
      const double xi = readlane_f64(y_hi * inv_hi, i);
      if (j == i) y_hi = xi;
      else if (live && j < i && i < nb_hi) y_hi -= c_hi[i] * xi;
      if (i < nb_hi) y_lo -= g[i] * xi;
    }
#pragma unroll
    for (int i = SB - 1; i >= 0; --i) {               // lower triangle
      const double xi = readlane_f64(y_lo * inv_lo, i);
      if (j == i) y_lo = xi;
      else if (j < i) y_lo -= c_lo[i] * xi;
    }
    xs[j] = y_lo;
    xs[SB + j] = live ? y_hi : 0.0;
    if (blockIdx.x == 0) {
      dx[k_lo + j] = (float)y_lo;                     // (b keeps y: the other workgroups still read it)
      if (live) dx[k_hi + j] = (float)y_hi;
    }
  }
  // waves 1-3: this thread's column of the update, requested before the barrier (it needs nothing of x)
  const int c = blockIdx.x * 192 + (tid - 64);
  const int cc = min(max(c, 0), max(k_lo - 1, 0));
  double v[2 * SB];
  double bc = 0.0;
  if (wv != 0) {
#pragma unroll
    for (int u = 0; u < 2 * SB; ++u) v[u] = L[(size_t)(k_lo + min(u, SB + nb_hi - 1)) * n + cc];
    bc = b[cc];
  }
  __syncthreads();
  if (wv != 0 && c < k_lo) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int u = 0; u < 2 * SB; u += 2) {
      if (u < SB + nb_hi) s0 = fma(v[u], xs[u], s0);
      if (u + 1 < SB + nb_hi) s1 = fma(v[u + 1], xs[u + 1], s1);
    }
    b[c] = bc - (s0 + s1);
  }
}

#ifdef CHOL_TIMING   // tools/chol_bench.hip only: per-phase wall-clock stamps (100 MHz)
__device__ long long g_chol_t[64];
#define CHOL_STAMP(i) do { if (threadIdx.x == 0) g_chol_t[i] = wall_clock64(); } while (0)
#define CHOL_ACC_DECL long long t_acc[5] = {0, 0, 0, 0, 0}; long long t_last = wall_clock64()
#define CHOL_ACC(i) do { const long long t_now = wall_clock64(); t_acc[i] += t_now - t_last; t_last = t_now; } while (0)
#define CHOL_ACC_DUMP do { if (threadIdx.x == 0) for (int q = 0; q < 5; ++q) g_chol_t[10 + q] = t_acc[q]; } while (0)
#else
#define CHOL_STAMP(i) do { } while (0)
#define CHOL_ACC_DECL do { } while (0)
#define CHOL_ACC(i) do { } while (0)
#define CHOL_ACC_DUMP do { } while (0)
#endif

// ---- single-launch path for the frontend window (6P <= 192) -------------------------------
// The multi-kernel path above spends its time in launch-to-launch dependencies: 6P = 150 is 5 panel
// + 4 trailing launches + the solve, ~230 us for 1.1 MFLOP.  Here ONE workgroup keeps the packed
// lower triangle in LDS (90 KB at n = 150; CDNA4's 160 KB holds n <= 192) and does damping, the
// factorisation, both substitutions and the failure fallback in one launch; the only global traffic
// is one read of H and b and the fp32 dx.
//
// Two-level right-looking factorisation.  Inner step = one camera block (6 pivots): the 6x6 diagonal
// block is factored REDUNDANTLY by every thread in registers (no broadcast step), each thread solves
// its own panel row and applies the rank-6 update to that row's remaining columns of the current
// 30-wide panel only.  Once per panel the rank-30 update of the rest of the matrix runs on 4x4
// register tiles -- the LDS read-modify-write traffic of the far matrix is paid 5x, not 25x.
// b rides along as row n of the matrix, so the forward substitution L y = b falls out of the panel
// steps for free; the backward substitution is column-oriented (x block known -> every remaining
// y[c] is updated independently, no reductions).
constexpr int SMALL_N = 192;
constexpr int CB = 6;      // camera block
#ifndef GS_CHOL_NT
#define GS_CHOL_NT 1024
#endif
constexpr int SMALL_NT = GS_CHOL_NT;   // one workgroup, 16 waves: latency hiding for the LDS-resident steps (tools/chol_bench.hip
                                       // builds other sizes with -DGS_CHOL_NT=...; 512 and 768 solve correctly but
                                       // slower, 256 does not: the work splits below assume >= 8 waves)
static_assert(SMALL_NT >= 512 && SMALL_NT % 64 == 0 && SMALL_NT <= 1024, "chol: 512 .. 1024 threads");
constexpr int PW = 30;     // panel width (5 camera blocks): far updates are deferred per panel


__device__ __forceinline__ int tri(int r, int c) { return ((r * (r + 1)) >> 1) + c; }

// ---- the LDS-resident core, shared by chol_small_kernel (6P <= 192) and the tail of chol_mid_kernel ------------------
// Lp: packed lower triangle of [A; b^T] (n + 1 rows, already damped), invd: n reciprocals of the diagonal of L.
// Factorises in place (b rides along as row n: forward substitution for free) and reports a non-positive pivot.
__device__ __forceinline__ void lds_factor(double* Lp, double* invd, const int n, bool& bad) {
  const int tid = threadIdx.x;
  CHOL_ACC_DECL;
  for (int p0 = 0; p0 < n; p0 += PW) {
    const int pend = min(p0 + PW, n);                 // panel = columns [p0, pend)
    for (int k0 = p0; k0 < pend; k0 += CB) {
      const int s0 = k0 + CB;
      const int rows = n + 1 - s0;                    // rows below the diagonal block (the b row included)
      // (0) LEFT-LOOKING inside the panel (round 4): bring this block column (columns k0 .. k0+5, rows k0 .. n) up to
      // date with the panel's earlier blocks, A[r][k0+c] -= sum_{k in [p0,k0)} L[r][k] L[k0+c][k].  A thread owns one
      // row and two of the six columns: it reads its row's <= 24 panel entries once and the pivot rows' entries as LDS
      // multicasts (lanes of a wave share them).  The right-looking form this replaces updated ALL remaining panel
      // columns after every block and re-read 7 doubles per (row, column): 168 LDS accesses per row and step against
      // ~30 here -- that pass was LDS-bandwidth bound (19 of the 51 us of the factorisation at n = 150).
      const int kw = k0 - p0;                         // panel columns already factored (0, 6, .. 24)
      if (kw > 0) {
        const int rr = tid / 3, cg = tid - 3 * rr;    // row k0 + rr, columns k0 + 2 cg, k0 + 2 cg + 1
        if (rr < rows + CB) {
          const int r = k0 + rr;
          const double* Xr = Lp + tri(r, p0);
          const int c0 = 2 * cg, c1 = c0 + 1;
          const bool ok0 = k0 + c0 <= r && k0 + c0 < n, ok1 = k0 + c1 <= r && k0 + c1 < n;   // lower triangle only
          const double* L0 = Lp + tri(min(k0 + c0, n - 1), p0);
          const double* L1 = Lp + tri(min(k0 + c1, n - 1), p0);
          double a0 = 0.0, a1 = 0.0;
#pragma unroll 6
          for (int k = 0; k < kw; ++k) {
            const double x = Xr[k];
            a0 = fma(x, L0[k], a0);
            a1 = fma(x, L1[k], a1);
          }
          if (ok0) Lp[tri(r, k0 + c0)] -= a0;
          if (ok1) Lp[tri(r, k0 + c1)] -= a1;
        }
        __syncthreads();
      }
      CHOL_ACC(2);
      // (1) 6x6 diagonal block, redundantly in every wave that owns panel rows, registers
      const bool need = tid < ((max(rows, CB) + 63) & ~63);
      double l[CB][CB], inv[CB];
      if (need) {
#pragma unroll
        for (int i = 0; i < CB; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) l[i][j] = Lp[tri(k0 + i, k0 + j)];
#pragma unroll
        for (int j = 0; j < CB; ++j) {
          double piv = l[j][j];
#pragma unroll
          for (int t = 0; t < j; ++t) piv = fma(-l[j][t], l[j][t], piv);
          if (!(piv > 0.0) && piv == piv) bad = true; // pivot <= 0 (NaN falls through like Eigen)
          sqrt_rsqrt(piv, l[j][j], inv[j]);
#pragma unroll
          for (int i = j + 1; i < CB; ++i) {
            double sacc = l[i][j];
#pragma unroll
            for (int t = 0; t < j; ++t) sacc = fma(-l[i][t], l[j][t], sacc);
            l[i][j] = sacc * inv[j];
          }
        }
      }
      CHOL_ACC(0);
      // (2) rows below the block (the b row included): x = a L11^-T
      if (tid < rows) {                               // rows <= 187: one thread per row
        double* Ar = Lp + tri(s0 + tid, k0);
        double x[CB];
#pragma unroll
        for (int j = 0; j < CB; ++j) {
          double s = Ar[j];
#pragma unroll
          for (int u = 0; u < j; ++u) s = fma(-x[u], l[j][u], s);
          x[j] = s * inv[j];
        }
#pragma unroll
        for (int j = 0; j < CB; ++j) Ar[j] = x[j];
      }
      CHOL_ACC(1);
      __syncthreads();                                // x is visible; all reads of the old diagonal block are done
      if (tid < CB) {                                 // ... so its factor can replace it (only the backward pass reads it)
#pragma unroll
        for (int i = 0; i < CB; ++i)
          if (i == tid) {
#pragma unroll
            for (int j = 0; j <= i; ++j) Lp[tri(k0 + i, k0 + j)] = l[i][j];
            invd[k0 + i] = inv[i];
          }
      }
      CHOL_ACC(3);
    }
    // (4) rank-PW update of everything right of / below the panel on the fp64 matrix cores: one wave per 16x16
    // tile of the lower triangle, v_mfma_f64_16x16x4_f64 over 8 k-steps (A[i][k] = L[r0+i][p0+k] and B[k][j] =
    // L[c0+j][p0+k], one double per lane: row/column = lane & 15, k = lane >> 4; D: column = lane & 15, row =
    // (lane >> 4) + 4 * reg).  16 LDS reads per lane per tile instead of 240 for the same 7 680 multiply-adds: the
    // 4x4 register tiles this replaces were bound by LDS bandwidth (18 of the 60 us of the factorisation at n = 150).
    const int s1 = pend;
    const int rows1 = n + 1 - s1;                     // rows s1..n (b row included)
    const int pw = pend - p0;
    if (rows1 > 1) {
      typedef double double4v __attribute__((ext_vector_type(4)));
      const int T = (rows1 + 15) >> 4, ntile = (T * (T + 1)) >> 1;
      const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;
      for (int t = wv; t < ntile; t += SMALL_NT / 64) {
        int ti = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
        while (((ti + 1) * (ti + 2)) >> 1 <= t) ++ti;
        while ((ti * (ti + 1)) >> 1 > t) --ti;
        const int tj = t - ((ti * (ti + 1)) >> 1);
        const int r0 = s1 + 16 * ti, c0 = s1 + 16 * tj;
        const double* pa = Lp + tri(min(r0 + (ln & 15), n), p0);
        const double* pb = Lp + tri(min(c0 + (ln & 15), n), p0);
        double4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kb = 0; kb < (PW + 3) / 4; ++kb) {
          const int k = 4 * kb + (ln >> 4);
          const double a = k < pw ? pa[k] : 0.0, b = k < pw ? pb[k] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        const int c = c0 + (ln & 15);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int rr = r0 + (ln >> 4) + 4 * q;
          if (rr <= n && c < n && c <= rr) Lp[tri(rr, c)] -= acc[q];   // column n (the b row's own diagonal) is unused
        }
      }
    }
    __syncthreads();
    CHOL_ACC(4);
  }
  CHOL_ACC_DUMP;
}

// backward substitution L^T x = y (y sits in row n of Lp), column-oriented, 6 unknowns per step; dx[i] = (float) x[i],
// and the solved x replaces y in LDS (row n), which the mid-size kernel's head stages read afterwards.
// ONE wave does it (round 6).  A step is a 6-pivot dependent chain + 6 multiply-adds per remaining column: nothing for
// 16 waves to share, and in the 1024-thread form every step paid two workgroup barriers -- 25 steps x 2 barriers were
// ~10 of the backward's 15 us at n = 150.  Inside a wave the LDS is in order: a step's writes to y are visible to the
// next step's reads with no barrier at all.  The columns are dealt from k0 - 1 downwards, so the six entries the NEXT
// step's chain starts from are updated in the first trip.  Ends with a workgroup barrier (x is in row n for everyone).
__device__ __forceinline__ void lds_backward(double* Lp, const double* invd, const int n, float* __restrict__ dx) {
  const int npk = (n * (n + 1)) >> 1;
  double* y = Lp + npk;
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    for (int k0 = n - CB; k0 >= 0; k0 -= CB) {
      double l[CB][CB], x[CB];
#pragma unroll
      for (int i = 0; i < CB; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) l[i][j] = Lp[tri(k0 + i, k0 + j)];
#pragma unroll
      for (int i = CB - 1; i >= 0; --i) {
        double sacc = y[k0 + i];
#pragma unroll
        for (int t = i + 1; t < CB; ++t) sacc = fma(-l[t][i], x[t], sacc);
        x[i] = sacc * invd[k0 + i];
      }
      for (int c = k0 - 1 - lane; c >= 0; c -= 64) {
        double s = y[c];
#pragma unroll
        for (int i = 0; i < CB; ++i) s = fma(-Lp[tri(k0 + i, c)], x[i], s);
        y[c] = s;
      }
      if (lane < CB) {
        double xl = x[0];
#pragma unroll
        for (int i = 1; i < CB; ++i) xl = (i == lane) ? x[i] : xl;
        dx[k0 + lane] = (float)xl;
        y[k0 + lane] = xl;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  __syncthreads();
}

// packed lower triangle of [A; b^T] from global memory (rows / columns [c0, n) of the dense n x n array H, b from bg),
// diagonal damped on the way in: 4 independent loads in flight per thread (x 1024 threads) -- a lone workgroup is bound
// by global-load latency, not bandwidth
__device__ __forceinline__ void lds_load_packed(double* Lp, const double* __restrict__ H, const double* __restrict__ bg,
                                                const int n, const int c0, const double lm, const double ep) {
  const int tid = threadIdx.x;
  const int m = n - c0;
  const int npk = (m * (m + 1)) >> 1;
  for (int base = 0; base < npk; base += SMALL_NT * 4) {
    double v[4];
    int dg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * SMALL_NT + tid;
      int r = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
      while (((r + 1) * (r + 2)) >> 1 <= idx) ++r;
      while ((r * (r + 1)) >> 1 > idx) --r;
      const int c = idx - ((r * (r + 1)) >> 1);
      dg[u] = (c == r) ? 1 : 0;
      v[u] = idx < npk ? H[(size_t)(c0 + r) * n + (c0 + c)] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * SMALL_NT + tid;
      if (idx < npk) Lp[idx] = dg[u] ? v[u] + (ep + lm * v[u]) : v[u];
    }
  }
  for (int i = tid; i <= m; i += SMALL_NT) Lp[npk + i] = (i < m) ? bg[c0 + i] : 0.0;    // row m = b^T
}

__global__ __launch_bounds__(SMALL_NT) void chol_small_kernel(const double* __restrict__ H, const double* __restrict__ bg,
                                                         int n, double lm, double ep, float* __restrict__ dx,
                                                         int32_t* fail_flag, int32_t* fail_count) {
  extern __shared__ double sm[];
  double* Lp = sm;                                   // packed lower triangle of [A; b^T], n+1 rows
  double* invd = sm + (((n + 1) * (n + 2)) >> 1);    // 1 / L[j][j]
  const int tid = threadIdx.x;
  CHOL_STAMP(0);
  lds_load_packed(Lp, H, bg, n, 0, lm, ep);
  __syncthreads();
  CHOL_STAMP(1);

  __shared__ int s_bad;
  bool bad = false;                                   // thread 0 takes part in every diagonal block
  lds_factor(Lp, invd, n, bad);
  CHOL_STAMP(2);

  if (tid == 0) s_bad = bad ? 1 : 0;
  __syncthreads();
  if (s_bad) {   // reference: zero update on failure (droid_kernels.cu:1207-1210)
    for (int i = tid; i < n; i += SMALL_NT) dx[i] = 0.0f;
    if (tid == 0) { *fail_flag = 1; *fail_count += 1; }
    return;
  }
  if (tid == 0) *fail_flag = 0;
  lds_backward(Lp, invd, n, dx);
  CHOL_STAMP(3);
}

// ---- single-launch path for the MONOCULAR frontend window (192 < 6P <= 612; replica_mono.yaml:29: window 50 -> 294) ----
// The packed fp64 triangle of 6P = 294 takes 349 KB: it does not fit the CU's 160 KB of LDS, and the multi-kernel path
// above costs ~0.39 ms per solve at that size (10 panel + 9 trailing launches + solve, each a dependent launch).  Here
// ONE workgroup does the whole solve in one launch with the trailing matrix in HBM / L2 until it is small enough:
//   * HEAD STAGES (while more than 192 columns remain): the stage's SW = 60 (or 30) columns of ALL remaining rows -- a
//     TALL panel [n + 1 - c0][SW], b^T as its last row -- are loaded into LDS and factored exactly like the panels of
//     the LDS-resident kernel (6x6 diagonal blocks in registers, one thread per row, per-30-column far updates on the
//     fp64 matrix cores); then the rank-SW update of the trailing matrix is applied IN GLOBAL MEMORY (read-modify-write
//     of the lower triangle by the same workgroup, 16x16 tiles on v_mfma_f64_16x16x4; b's trailing part too) and the
//     stage's columns of L go back to H for the backward substitution;
//   * TAIL: the remaining <= 192 columns are loaded as a packed triangle and handled by lds_factor / lds_backward;
//   * backward substitution of the head columns: y -= L21^T x_tail from global memory, then stage by stage in reverse.
// Same arithmetic as the blocked path: fp64 throughout, pivot <= 0 anywhere => dx = 0 (droid_kernels.cu:1202-1210).
#ifndef CHOL_TB
#define CHOL_TB 2                  // tiles per wave in flight in the head stages' global trailing update
#endif
constexpr int MID_N = 300;      // beyond this the multi-kernel path (whole chip on the trailing updates) wins: 201 vs 231 us at
                                // 6P = 294, 243 vs 227 at 306, 306 vs 249 at 342, 556 vs 419 at 450 (tools/chol_bench.hip;
                                // until the round-6 one-launch-per-panel form the two met at 450)
constexpr int MID_SW60_N = 300; // up to here a 60-column stage fits: (n + 1) x 61 doubles + vectors <= 160 KB

// 16x16 tile of A B^T over KS k-steps of 4 on the fp64 matrix cores; the operands of five k-steps are requested from LDS
// before their products are issued (a rolled loop pays an LDS round trip + a dependent MFMA per k-step)
template <int KS>
__device__ __forceinline__ __attribute__((ext_vector_type(4))) double mid_tile_product(const double* pa, const double* pb,
                                                                                      int ln, int SW) {
  typedef double double4v __attribute__((ext_vector_type(4)));
  double4v acc = {0.0, 0.0, 0.0, 0.0};
  constexpr int G = 5;
#pragma unroll
  for (int g0 = 0; g0 < KS; g0 += G) {
    double a[G], b[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int k = 4 * (g0 + u) + (ln >> 4);
      a[u] = (g0 + u < KS && k < SW) ? pa[k] : 0.0;
      b[u] = (g0 + u < KS && k < SW) ? pb[k] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < G; ++u)
      if (g0 + u < KS) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
  }
  return acc;
}

__global__ __launch_bounds__(SMALL_NT) void chol_mid_kernel(double* __restrict__ H, double* __restrict__ bg, int n,
                                                       double lm, double ep, int SW, float* __restrict__ dx,
                                                       int32_t* fail_flag, int32_t* fail_count) {
  extern __shared__ double sm[];
  typedef double double4v __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;
  double* invd = sm;                 // [n]  1 / L[j][j] of every column
  double* yv = sm + n;               // [n]  forward-substituted b of the head columns, then x of every column
  double* T = sm + 2 * n;            // tall panel [rows][SWP] / packed tail triangle
  const int SWP = SW + 1;            // odd row stride (in doubles): rows hit different banks
  __shared__ int s_bad;
  bool bad = false;
  // damping once, on the original diagonal (the trailing updates below then act on the damped matrix, as in LLT(A + D))
  for (int i = tid; i < n; i += SMALL_NT) {
    const double d = H[(size_t)i * n + i];
    H[(size_t)i * n + i] = d + (ep + lm * d);
  }
  __syncthreads();
  int c0 = 0;
  CHOL_STAMP(20);
  for (; n - c0 > SMALL_N; c0 += SW) {
    const int R = n + 1 - c0;                         // rows of the tall panel (b^T last)
    const int stg_ = (c0 / SW) < 4 ? 21 + 4 * (c0 / SW) : 56;
    (void)stg_;
    // ---- load: row r (global row c0 + r), columns c0 .. c0 + min(SW - 1, r)
    for (int base = 0; base < R * SW; base += 4 * SMALL_NT) {     // 4 independent loads in flight per thread
      double v[4];
      int at[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = base + u * SMALL_NT + tid;
        const int r = idx / SW, k = idx - r * SW;
        v[u] = 0.0;
        at[u] = idx < R * SW ? r * SWP + k : -1;
        if (idx < R * SW) {
          if (r == R - 1) v[u] = bg[c0 + k];
          else if (k <= r) v[u] = H[(size_t)(c0 + r) * n + (c0 + k)];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (at[u] >= 0) T[at[u]] = v[u];
    }
    __syncthreads();
    CHOL_STAMP(stg_ + 0);
    // ---- factor the SW columns (local indices: column k, row r of T)
    for (int p0 = 0; p0 < SW; p0 += PW) {
      const int pend = p0 + PW;
      for (int k0 = p0; k0 < pend; k0 += CB) {
        const int s0 = k0 + CB;
        const int rows = R - s0;                      // rows below the diagonal block (>= 1: the b row)
        // left-looking inside the panel, as lds_factor: block column k0 .. k0+5 of rows k0 .. R-1 catches up with the
        // panel's earlier blocks before it is factored
        const int kw = k0 - p0;
        if (kw > 0) {
          const int cg = tid % 3;
          for (int rr = tid < 3 * (SMALL_NT / 3) ? tid / 3 : R; rr < rows + CB; rr += SMALL_NT / 3) {   // (341 x 3 threads)
            const int r = k0 + rr;
            const double* Xr = T + r * SWP + p0;
            const int c0 = 2 * cg, c1 = c0 + 1;
            const bool ok0 = k0 + c0 <= r, ok1 = k0 + c1 <= r;
            const double* L0 = T + (k0 + c0) * SWP + p0;
            const double* L1 = T + (k0 + c1) * SWP + p0;
            double a0 = 0.0, a1 = 0.0;
#pragma unroll 6
            for (int k = 0; k < kw; ++k) {
              const double x = Xr[k];
              a0 = fma(x, L0[k], a0);
              a1 = fma(x, L1[k], a1);
            }
            if (ok0) T[r * SWP + k0 + c0] -= a0;
            if (ok1) T[r * SWP + k0 + c1] -= a1;
          }
          __syncthreads();
        }
        const bool need = tid < ((max(rows, CB) + 63) & ~63);
        double l[CB][CB], inv[CB];
        if (need) {
#pragma unroll
          for (int i = 0; i < CB; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) l[i][j] = T[(k0 + i) * SWP + (k0 + j)];
#pragma unroll
          for (int j = 0; j < CB; ++j) {
            double piv = l[j][j];
#pragma unroll
            for (int t = 0; t < j; ++t) piv = fma(-l[j][t], l[j][t], piv);
            if (!(piv > 0.0) && piv == piv) bad = true;
            sqrt_rsqrt(piv, l[j][j], inv[j]);
#pragma unroll
            for (int i = j + 1; i < CB; ++i) {
              double sacc = l[i][j];
#pragma unroll
              for (int t = 0; t < j; ++t) sacc = fma(-l[i][t], l[j][t], sacc);
              l[i][j] = sacc * inv[j];
            }
          }
        }
        if (tid < rows) {                             // one thread per row: x = a L11^-T
          double* Ar = T + (s0 + tid) * SWP + k0;
          double x[CB];
#pragma unroll
          for (int j = 0; j < CB; ++j) {
            double s = Ar[j];
#pragma unroll
            for (int u = 0; u < j; ++u) s = fma(-x[u], l[j][u], s);
            x[j] = s * inv[j];
          }
#pragma unroll
          for (int j = 0; j < CB; ++j) Ar[j] = x[j];
        }
        __syncthreads();
        if (tid < CB) {
#pragma unroll
          for (int i = 0; i < CB; ++i)
            if (i == tid) {
#pragma unroll
              for (int j = 0; j <= i; ++j) T[(k0 + i) * SWP + (k0 + j)] = l[i][j];
              invd[c0 + k0 + i] = inv[i];
            }
        }
      }
      // rank-30 update of the stage's remaining columns [pend, SW) for rows >= pend (matrix cores, 16x16 tiles)
      if (pend < SW) {
        const int rows1 = R - pend, cols1 = SW - pend;
        const int TR = (rows1 + 15) >> 4, TC = (cols1 + 15) >> 4;
        for (int t = wv; t < TR * TC; t += SMALL_NT / 64) {
          const int ti = t / TC, tj = t - ti * TC;
          const int r0 = pend + 16 * ti, q0 = pend + 16 * tj;
          if (q0 > r0 + 15) continue;                 // tile wholly above the diagonal
          const double* pa = T + min(r0 + (ln & 15), R - 1) * SWP + p0;
          const double* pb = T + min(q0 + (ln & 15), SW - 1) * SWP + p0;
          double4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int kb = 0; kb < (PW + 3) / 4; ++kb) {
            const int k = 4 * kb + (ln >> 4);
            const double a = k < PW ? pa[k] : 0.0, b = k < PW ? pb[k] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
          }
          const int c = q0 + (ln & 15);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int rr = r0 + (ln >> 4) + 4 * q;
            if (rr < R && c < SW && (c <= rr || rr == R - 1)) T[rr * SWP + c] -= acc[q];
          }
        }
        __syncthreads();
      }
    }
    CHOL_STAMP(stg_ + 1);
    // ---- rank-SW update of the trailing matrix in global memory: rows / columns [c1, n], the b row included
    {
      const int R1 = n + 1 - (c0 + SW);
      const int TT1 = (R1 + 15) >> 4, ntile = (TT1 * (TT1 + 1)) >> 1;
      constexpr int TB = CHOL_TB;                         // tiles in flight per wave: their 16 global loads per lane are
      for (int tb = wv * TB; tb < ntile; tb += (SMALL_NT / 64) * TB) {   // issued before the first product
        double cur[TB][4];
        bool ok[TB][4];
        int r0s[TB], q0s[TB];
#pragma unroll
        for (int u = 0; u < TB; ++u) {
          const int t = min(tb + u, ntile - 1);
          int ti = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
          while (((ti + 1) * (ti + 2)) >> 1 <= t) ++ti;
          while ((ti * (ti + 1)) >> 1 > t) --ti;
          const int tj = t - ((ti * (ti + 1)) >> 1);
          r0s[u] = SW + 16 * ti;                      // local rows of T
          q0s[u] = SW + 16 * tj;
          const int cl = q0s[u] + (ln & 15);          // local column index (= local row index of the other operand)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int rl = r0s[u] + (ln >> 4) + 4 * q;
            ok[u][q] = (tb + u < ntile) && rl < R && cl < R - 1 && cl <= rl;   // column n does not exist; lower triangle
            cur[u][q] = 0.0;
            if (ok[u][q]) cur[u][q] = (rl == R - 1) ? bg[c0 + cl] : H[(size_t)(c0 + rl) * n + (c0 + cl)];
          }
        }
#pragma unroll
        for (int u = 0; u < TB; ++u) {
          if (tb + u >= ntile) break;
          const double* pa = T + min(r0s[u] + (ln & 15), R - 1) * SWP;
          const double* pb = T + min(q0s[u] + (ln & 15), R - 1) * SWP;
          const double4v acc = SW == 60 ? mid_tile_product<15>(pa, pb, ln, SW) : mid_tile_product<8>(pa, pb, ln, SW);
          const int cl = q0s[u] + (ln & 15);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int rl = r0s[u] + (ln >> 4) + 4 * q;
            if (ok[u][q]) {
              const double v = cur[u][q] - acc[q];
              if (rl == R - 1) bg[c0 + cl] = v;
              else H[(size_t)(c0 + rl) * n + (c0 + cl)] = v;
            }
          }
        }
      }
    }
    CHOL_STAMP(stg_ + 2);
    // ---- the stage's columns of L back to H (backward substitution reads them), y of these columns to LDS
    for (int idx = tid; idx < (R - 1) * SW; idx += SMALL_NT) {
      const int r = idx / SW, k = idx - r * SW;
      if (k <= r) H[(size_t)(c0 + r) * n + (c0 + k)] = T[r * SWP + k];
    }
    for (int k = tid; k < SW; k += SMALL_NT) yv[c0 + k] = T[(R - 1) * SWP + k];
    __threadfence_block();
    __syncthreads();                                  // global writes of this workgroup are visible to its next loads
    CHOL_STAMP(stg_ + 3);
  }
  // ---- tail: the remaining m <= 192 columns, LDS-resident (already damped)
  const int m = n - c0;
  double* Lp = T;
  lds_load_packed(Lp, H, bg, n, c0, 0.0, 0.0);
  __syncthreads();
  CHOL_STAMP(40);
  lds_factor(Lp, invd + c0, m, bad);
  CHOL_STAMP(41);
  if (tid == 0) s_bad = 0;
  __syncthreads();
  if (bad) s_bad = 1;                                 // every diagonal block was factored by (at least) wave 0
  __syncthreads();
  if (s_bad) {
    for (int i = tid; i < n; i += SMALL_NT) dx[i] = 0.0f;
    if (tid == 0) { *fail_flag = 1; *fail_count += 1; }
    return;
  }
  if (tid == 0) *fail_flag = 0;
  lds_backward(Lp, invd + c0, m, dx + c0);
  CHOL_STAMP(42);
  {                                                   // x of the tail -> yv[c0 .. n)
    const double* xt = Lp + ((m * (m + 1)) >> 1);
    for (int i = tid; i < m; i += SMALL_NT) yv[c0 + i] = xt[i];
  }
  __syncthreads();
  // ---- head columns: y[c] -= sum_{r >= c0} L[r][c] x[r] (L21 from global), 8 row groups per column, merged in LDS
  {
    double* part = T;                                 // [8][c0] partial sums (the tail triangle is no longer needed)
    const int ng = 8;
    for (int idx = tid; idx < ng * c0; idx += SMALL_NT) {
      const int g = idx / c0, c = idx - g * c0;
      double s = 0.0;
      for (int r = c0 + g; r < n; r += ng) s = fma(H[(size_t)r * n + c], yv[r], s);
      part[g * c0 + c] = s;
    }
    __syncthreads();
    for (int c = tid; c < c0; c += SMALL_NT) {
      double s = yv[c];
#pragma unroll
      for (int g = 0; g < 8; ++g) s -= part[g * c0 + c];
      yv[c] = s;
    }
    __syncthreads();
  }
  CHOL_STAMP(43);
  // ---- the head stages in reverse: solve the stage's SW x SW triangle (from global into T), then propagate to the left
  for (int a = c0 - SW; a >= 0; a -= SW) {
    for (int idx = tid; idx < SW * SW; idx += SMALL_NT) {
      const int r = idx / SW, k = idx - r * SW;
      T[r * SWP + k] = (k <= r) ? H[(size_t)(a + r) * n + (a + k)] : 0.0;
    }
    __syncthreads();
    for (int k0 = SW - CB; k0 >= 0; k0 -= CB) {
      double x[CB];
      if (tid < ((max(k0, CB) + 63) & ~63)) {         // (only the waves that update a y[c], c < k0, or write x)
        double l[CB][CB];
#pragma unroll
        for (int i = 0; i < CB; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) l[i][j] = T[(k0 + i) * SWP + (k0 + j)];
#pragma unroll
        for (int i = CB - 1; i >= 0; --i) {
          double sacc = yv[a + k0 + i];
#pragma unroll
          for (int t = i + 1; t < CB; ++t) sacc = fma(-l[t][i], x[t], sacc);
          x[i] = sacc * invd[a + k0 + i];
        }
      }
      __syncthreads();                                // everyone has read y[a + k0 .. +5]
      if (tid < CB) {
#pragma unroll
        for (int i = 0; i < CB; ++i)
          if (i == tid) { dx[a + k0 + i] = (float)x[i]; yv[a + k0 + i] = x[i]; }
      }
      for (int c = tid; c < k0; c += SMALL_NT) {
        double s = yv[a + c];
#pragma unroll
        for (int i = 0; i < CB; ++i) s = fma(-T[(k0 + i) * SWP + c], x[i], s);
        yv[a + c] = s;
      }
      __syncthreads();
    }
    // columns left of the stage: y[c] -= sum_{r in stage} L[a + r][c] x[a + r]; row groups in parallel, merged in LDS
    if (a > 0) {
      double* part = T;                               // (the stage's triangle is no longer needed)
      const int ng = min(16, SMALL_NT / a);
      for (int idx = tid; idx < ng * a; idx += SMALL_NT) {
        const int g = idx / a, c = idx - g * a;
        double s = 0.0;
        for (int r = g; r < SW; r += ng) s = fma(H[(size_t)(a + r) * n + c], yv[a + r], s);
        part[g * a + c] = s;
      }
      __syncthreads();
      for (int c = tid; c < a; c += SMALL_NT) {
        double s = yv[c];
        for (int g = 0; g < ng; ++g) s -= part[g * a + c];
        yv[c] = s;
      }
      __syncthreads();
    }
  }
  CHOL_STAMP(44);
}

enum { CHOL_PATH_DISPATCH = 0, CHOL_PATH_SMALL = 1, CHOL_PATH_MID = 2, CHOL_PATH_BLOCKED = 3 };

// dynamic LDS of chol_mid_kernel at n (SW = 60 or 30 column stages, then the <= 192-column packed tail)
size_t chol_mid_lds(int n) {
  const int SW = n <= MID_SW60_N ? 60 : 30;
  const size_t tall = (size_t)(n + 1) * (SW + 1);
  const size_t tail = (size_t)(SMALL_N + 1) * (SMALL_N + 2) / 2 + SMALL_N;
  return ((size_t)2 * n + (tall > tail ? tall : tail)) * sizeof(double);
}

bool chol_small_fits(int n) { return n >= 1 && n <= SMALL_N && n % CB == 0; }
bool chol_mid_fits(int n) {                           // (the kernel also has a few bytes of static LDS)
  return n >= 1 && n <= MID_N && n % CB == 0 && chol_mid_lds(n) <= 160 * 1024 - 256;
}

// the product's choice of path for n unknowns
int chol_dispatch(int n) {
  if (chol_small_fits(n)) return CHOL_PATH_SMALL;
  if (chol_mid_fits(n)) return CHOL_PATH_MID;
  return CHOL_PATH_BLOCKED;
}

// the three paths; `path` is CHOL_PATH_SMALL / _MID / _BLOCKED and its preconditions hold (chol_small_fits / chol_mid_fits)
int chol_solve_path(double* H, double* b, int n, float lm, float ep, int path, float* dx_out, int32_t* fail_flag,
                    int32_t* fail_count, hipStream_t st) {
  if (path == CHOL_PATH_SMALL) {
    const size_t lds = ((size_t)(n + 1) * (n + 2) / 2 + (size_t)n) * sizeof(double);
    static GsLdsLimit limit;
    const size_t cap = ((size_t)(SMALL_N + 1) * (SMALL_N + 2) / 2 + SMALL_N) * sizeof(double);
    if (int rc = limit.raise((const void*)chol_small_kernel, cap, "chol")) return rc;
    chol_small_kernel<<<1, SMALL_NT, lds, st>>>(H, b, n, (double)lm, (double)ep, dx_out, fail_flag, fail_count);
    GS_CHECK_LAUNCH("chol_small");
    return GS_OK;
  }
  if (path == CHOL_PATH_MID) {                        // the monocular window: one launch, trailing matrix in HBM / L2
    const int SW = n <= MID_SW60_N ? 60 : 30;
    const size_t lds = chol_mid_lds(n);
    static GsLdsLimit limit;
    if (int rc = limit.raise((const void*)chol_mid_kernel, lds, "chol_mid")) return rc;
    chol_mid_kernel<<<1, SMALL_NT, lds, st>>>(H, b, n, (double)lm, (double)ep, SW, dx_out, fail_flag, fail_count);
    GS_CHECK_LAUNCH("chol_mid");
    return GS_OK;
  }
  // panel 0 on its own (rows NB .. n: the matrix rows below the panel AND the b row, which rides along), then ONE launch
  // per further panel: its factorisation beside the previous panel's trailing update (chol_step_kernel)
  const int nb0 = n < NB ? n : NB;
  chol_panel_kernel<<<gs_cdiv(n - nb0 + 1, PR), 64, 0, st>>>(H, b, n, 0, fail_flag, 1, (double)lm, (double)ep);
  GS_CHECK_LAUNCH("chol_panel");
  constexpr size_t step_lds = ((size_t)NB * DS + (size_t)(2 * NB + 2 * PR) * (NB + 1) + NB) * sizeof(double);   // 59.6 KB
  static_assert(step_lds >= (size_t)2 * TT * (NB + 1) * sizeof(double), "chol_step: the trailing role's operands fit");
  for (int kp = 0; kp + NB < n; kp += NB) {
    const int c1 = kp + NB, nb1 = (n - c1 < NB) ? (n - c1) : NB, rem1 = n - c1 - nb1;
    const int n_panel = gs_cdiv(rem1 + 1, PR);
    const int T = rem1 > 0 ? gs_cdiv(rem1 + 1, TT) : 0;
    chol_step_kernel<<<n_panel + T * (T + 1) / 2, 256, step_lds, st>>>(H, b, n, kp, n_panel, fail_flag);
    GS_CHECK_LAUNCH("chol_step");
  }
  // b now holds y = L^-1 b; backward substitution from the last block up, two 64-wide blocks per launch (a single block is
  // left when their number is odd)
  int k0 = ((n - 1) / SB) * SB;
  for (; k0 >= SB; k0 -= 2 * SB) {
    const int k_lo = k0 - SB;
    chol_back_pair_kernel<<<gs_cdiv(k_lo, 192) + 1, 256, 0, st>>>(H, b, n, k_lo, dx_out, fail_flag, fail_count);
    GS_CHECK_LAUNCH("chol_back_pair");
  }
  if (k0 == 0) {
    chol_back_block_kernel<<<1, 256, 0, st>>>(H, b, n, 0, dx_out, fail_flag, fail_count);
    GS_CHECK_LAUNCH("chol_back_block");
  }
  return GS_OK;
}

}  // namespace

int gs_chol_solve_launch(double* H, double* b, int n, float lm, float ep, float* dx_out, int32_t* fail_flag,
                         int32_t* fail_count, hipStream_t st) {
  return chol_solve_path(H, b, n, lm, ep, chol_dispatch(n), dx_out, fail_flag, fail_count, st);
}

extern "C" int gs_chol_solve(double* H, double* b, int n, float lm, float ep, int path, float* dx, int32_t* status,
                             gs_stream_t stream) {
  GS_REQUIRE(n >= 1, "chol_solve: n = %d < 1", n);
  GS_REQUIRE(path >= CHOL_PATH_DISPATCH && path <= CHOL_PATH_BLOCKED, "chol_solve: unknown path %d (0 .. 3)", path);
  if (path == CHOL_PATH_SMALL && !chol_small_fits(n)) {
    gs_set_error("chol_solve: the small path needs n <= %d and n %% %d == 0 (n = %d)", SMALL_N, CB, n);
    return GS_ERR_UNSUPPORTED;
  }
  if (path == CHOL_PATH_MID && !chol_mid_fits(n)) {
    gs_set_error("chol_solve: the mid path needs n <= %d, n %% %d == 0 and %zu B of LDS to fit (n = %d)", MID_N, CB,
                 chol_mid_lds(n), n);
    return GS_ERR_UNSUPPORTED;
  }
  GS_REQUIRE(H && b && dx && status, "chol_solve: null pointer");
  if (path == CHOL_PATH_DISPATCH) path = chol_dispatch(n);
  return chol_solve_path(H, b, n, lm, ep, path, dx, status, status + 1, (hipStream_t)stream);
}
