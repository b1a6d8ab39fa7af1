// Monte Carlo localisation on a 2-D occupancy map: particles moved by odometry, weighed against a range scan on the
// likelihood field of gs_scan_field, and resampled (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_mcl_*); tests/mcl_restatement.py restates it serially; DESIGN.md section 38.
// Integer arithmetic only: every output equals the restatement bit for bit and two runs give the same bits.
//
// mcl_move_kernel      one lane per particle: the Q14 rotation of the odometry step in i64, the clamps, the heading wrap.
// mcl_weigh_kernel     the hot path, one wave per particle and lanes over the beams.  The particle is wave-uniform (scalar
//                      loads), so the wave reads the row ends[h] in runs of 64 consecutive int2 (512 bytes per instruction)
//                      and gathers one byte of `cost` per lane and beam; one integer butterfly per particle.  A particle
//                      that may not stand skips its beams.  The workgroup's four keys (S << 32 | p) go through LDS, one
//                      gs_wave_min_u64 and, when the result beats what `best` holds at that moment, one 64-bit atomic min.
//                      The other shape, one lane per particle, would read `ends` at 64 unrelated rows per instruction; it
//                      was not built or measured.
// mcl_estimate_kernel  one workgroup of 1024 threads: the minimum key, then chunks of 1024 particles -- the weight from the
//                      table, an inclusive scan per wave (__shfl_up), the waves' totals through LDS, a carry from chunk to
//                      chunk -- and 14 sums kept per thread across the chunks, reduced once at the end.  Integer sums have
//                      no order: any tree gives the same bits.
// mcl_resample_kernel  one lane per new particle: a binary search in `cum`, then a gather of three words.
// No inline assembly, no scratch, no dynamic LDS.
#include "common.h"

namespace {

constexpr int MCL_MAX = 1024;                               // cells per side
constexpr int MCL_MILLI = 1000;                             // milli-cells per cell
constexpr int MCL_MAX_PARTICLES = GS_MCL_MAX_PARTICLES;
constexpr int MCL_MAX_HEADINGS = 1024;
constexpr int MCL_MAX_BEAMS = 4096;
constexpr int MCL_MAX_LUT = 65536;
constexpr int MCL_MAX_STEP = 1 << 20;                       // |df|, |dl|, |dh|, |noise|
constexpr int MCL_MAX_END = 4000000;                        // |end point component| in milli-cells
constexpr int MCL_MAX_CAP = 15 * 15 + 1;
constexpr unsigned long long MCL_MAX_W = 1ull << 36;        // 2^16 particles of weight 2^20
constexpr int MCL_THREADS = 256;
constexpr int MCL_WAVES = MCL_THREADS / GS_WAVE;
constexpr int MCL_EST_THREADS = 1024;
constexpr int MCL_EST_WAVES = MCL_EST_THREADS / GS_WAVE;
constexpr int MCL_SUMS = 14;                                // stats words that are sums: 0-3 and 5-14 (4 is the key)
constexpr int MCL_FREE = 254, MCL_UNKNOWN = 205;
constexpr unsigned MCL_NO_SCORE = 0xffffffffu;

__device__ __forceinline__ int mcl_wrap(long long v, int H) {
  const int r = (int)(v % H);
  return r < 0 ? r + H : r;
}

// floor(t / 1000), written out for negative t (C's division rounds toward zero)
__device__ __forceinline__ int mcl_cell(int t) { return t >= 0 ? t / MCL_MILLI : -((MCL_MILLI - 1 - t) / MCL_MILLI); }

__global__ __launch_bounds__(MCL_THREADS) void mcl_move_kernel(const int* particles, int N, const int* __restrict__ rot,
                                                               int H, const int* __restrict__ noise, int df, int dl,
                                                               int dh, int n_u, int n_v, int* out) {
  const int p = blockIdx.x * MCL_THREADS + threadIdx.x;
  if (p >= N) return;
  const int x = particles[3 * p], y = particles[3 * p + 1], h = particles[3 * p + 2];
  const int n0 = noise[3 * p], n1 = noise[3 * p + 1], n2 = noise[3 * p + 2];
  const int at = mcl_wrap(h, H);                            // h itself inside the contract; never a read outside rot
  const long long c = rot[2 * at], s = rot[2 * at + 1];
  const long long f = (long long)df + n0, l = (long long)dl + n1;
  long long xn = x + ((f * c - l * s + 8192) >> 14);        // >> of a negative i64 is arithmetic
  long long yn = y + ((f * s + l * c + 8192) >> 14);
  const long long x_hi = (long long)MCL_MILLI * n_u - 1, y_hi = (long long)MCL_MILLI * n_v - 1;
  xn = xn < 0 ? 0 : (xn > x_hi ? x_hi : xn);
  yn = yn < 0 ? 0 : (yn > y_hi ? y_hi : yn);
  out[3 * p] = (int)xn;
  out[3 * p + 1] = (int)yn;
  out[3 * p + 2] = mcl_wrap((long long)h + dh + n2, H);
}

__global__ __launch_bounds__(MCL_THREADS) void mcl_weigh_kernel(
    const unsigned char* __restrict__ cost, const unsigned char* __restrict__ cells, int n_u, int n_v,
    const int* __restrict__ particles, int N, const int2* __restrict__ ends, int H, int B, int cap, int allow_unknown,
    unsigned* __restrict__ S, unsigned long long* __restrict__ best) {
  __shared__ unsigned long long keys[MCL_WAVES];
  const int lane = threadIdx.x & (GS_WAVE - 1), wave = threadIdx.x / GS_WAVE;
  const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * MCL_WAVES + wave));   // the wave's particle
  unsigned long long key = ~0ull;
  if (p < N) {
    const int x = particles[3 * p], y = particles[3 * p + 1], h = particles[3 * p + 2];
    // a particle outside the map or with a heading outside [0, H) stands nowhere: no read outside cells or ends
    bool stands = x >= 0 && x < MCL_MILLI * n_u && y >= 0 && y < MCL_MILLI * n_v && h >= 0 && h < H;
    if (stands) {
      const int c = cells[(x / MCL_MILLI) * n_v + y / MCL_MILLI];
      stands = c == MCL_FREE || (allow_unknown && c == MCL_UNKNOWN);
    }
    unsigned sum = MCL_NO_SCORE;
    if (stands) {                                           // wave-uniform
      const int2* __restrict__ row = ends + (size_t)h * B;
      unsigned acc = 0u;
      for (int b = lane; b < B; b += GS_WAVE) {
        const int2 e = row[b];
        const bool near = e.x >= -MCL_MAX_END && e.x <= MCL_MAX_END && e.y >= -MCL_MAX_END && e.y <= MCL_MAX_END;
        const int cu = mcl_cell(x + (near ? e.x : 0)), cv = mcl_cell(y + (near ? e.y : 0));   // |sum| < 2^23
        const bool in = near && cu >= 0 && cu < n_u && cv >= 0 && cv < n_v;
        const unsigned c = cost[in ? cu * n_v + cv : 0];    // always a load from inside the map: nothing to branch around
        acc += in ? c : (unsigned)cap;
      }
      sum = (unsigned)gs_wave_sum_i32((int)acc);            // <= 4096 * 226 < 2^20
      key = ((unsigned long long)sum << 32) | (unsigned)p;
    }
    if (lane == 0) S[p] = sum;
  }
  if (lane == 0) keys[wave] = key;
  __syncthreads();
  if (wave != 0) return;
  key = gs_wave_min_u64(lane < MCL_WAVES ? keys[lane] : ~0ull);
  // a minimum has no order: `best` ends as the smallest key whichever workgroup gets here first.  The plain read only
  // spares the atomic when it cannot change anything (a stale, larger value costs one atomic more, never a wrong result)
  if (lane == 0 && key != ~0ull && key < __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    __hip_atomic_fetch_min(best, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(MCL_EST_THREADS) void mcl_estimate_kernel(
    const unsigned* __restrict__ S, const int* __restrict__ particles, int N, const int* __restrict__ rot, int H,
    const unsigned* __restrict__ lut, int L, unsigned* __restrict__ w, unsigned long long* __restrict__ cum,
    unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long wave_word[MCL_EST_WAVES];
  __shared__ unsigned long long sums[MCL_SUMS][MCL_EST_WAVES];
  const int tid = threadIdx.x, lane = tid & (GS_WAVE - 1), wave = tid / GS_WAVE;
  unsigned long long key = ~0ull;
  for (int p = tid; p < N; p += MCL_EST_THREADS) {
    const unsigned s = S[p];
    const unsigned long long cand = s != MCL_NO_SCORE ? ((unsigned long long)s << 32) | (unsigned)p : ~0ull;
    key = cand < key ? cand : key;
  }
  key = gs_wave_min_u64(key);
  if (lane == 0) wave_word[wave] = key;
  __syncthreads();
  key = wave_word[0];
#pragma unroll
  for (int k = 1; k < MCL_EST_WAVES; ++k) key = wave_word[k] < key ? wave_word[k] : key;
  __syncthreads();                                          // wave_word is written again below
  const unsigned s_min = (unsigned)(key >> 32);
  // W, sum w^2, standing, w > 0, sum w x, w y, w c, w s, then w times the high and the low 20 bits of x^2, y^2 and x y
  unsigned long long acc[MCL_SUMS];
#pragma unroll
  for (int k = 0; k < MCL_SUMS; ++k) acc[k] = 0ull;
  unsigned long long carry = 0ull;                          // the weights of the chunks before this one
  for (int base = 0; base < N; base += MCL_EST_THREADS) {
    const int p = base + tid;
    unsigned wt = 0u;
    if (p < N) {
      const unsigned s = S[p];
      if (s != MCL_NO_SCORE) {
        const unsigned d = s - s_min;
        wt = d < (unsigned)L ? lut[d] : 0u;
        acc[2] += 1ull;
      }
      w[p] = wt;
      if (wt != 0u) {
        const int x = particles[3 * p], y = particles[3 * p + 1], h = particles[3 * p + 2];
        const bool turned = h >= 0 && h < H;                // outside the contract: no read outside rot
        const long long c = turned ? rot[2 * h] : 0, sn = turned ? rot[2 * h + 1] : 0;
        const unsigned long long wl = wt, ux = (unsigned)x, uy = (unsigned)y;
        const unsigned long long xx = ux * ux, yy = uy * uy, xy = ux * uy;      // < 2^40 inside the contract
        acc[0] += wl;
        acc[1] += wl * wl;
        acc[3] += 1ull;
        acc[4] += wl * ux;
        acc[5] += wl * uy;
        acc[6] += (unsigned long long)((long long)wl * c);  // two's complement: the i64 sum, read back signed
        acc[7] += (unsigned long long)((long long)wl * sn);
        acc[8] += wl * (xx >> 20);
        acc[9] += wl * (xx & 0xfffffull);
        acc[10] += wl * (yy >> 20);
        acc[11] += wl * (yy & 0xfffffull);
        acc[12] += wl * (xy >> 20);
        acc[13] += wl * (xy & 0xfffffull);
      }
    }
    unsigned long long v = wt;                              // inclusive scan over the wave's 64 particles
#pragma unroll
    for (int off = 1; off < GS_WAVE; off <<= 1) {
      const unsigned long long u = __shfl_up(v, off, GS_WAVE);
      if (lane >= off) v += u;
    }
    if (lane == GS_WAVE - 1) wave_word[wave] = v;
    __syncthreads();
    unsigned long long before = carry, total = 0ull;
#pragma unroll
    for (int k = 0; k < MCL_EST_WAVES; ++k) {
      const unsigned long long t = wave_word[k];
      before += k < wave ? t : 0ull;
      total += t;
    }
    if (p < N) cum[p] = before + v;
    carry += total;
    __syncthreads();                                        // every wave has read wave_word before the next chunk writes it
  }
#pragma unroll
  for (int k = 0; k < MCL_SUMS; ++k) {
    const unsigned long long t = (unsigned long long)gs_wave_sum_i64((long long)acc[k]);
    if (lane == 0) sums[k][wave] = t;
  }
  __syncthreads();
  if (tid >= GS_MCL_STATS) return;
  // word tid of stats: 0-3 the sums 0-3, 4 the key, 5-14 the sums 4-13, 15 zero
  unsigned long long out = 0ull;
  if (tid == 4) {
    out = key;
  } else if (tid < 15) {
    const int k = tid < 4 ? tid : tid - 1;
    for (int v = 0; v < MCL_EST_WAVES; ++v) out += sums[k][v];
  }
  stats[tid] = out;
}

__global__ __launch_bounds__(MCL_THREADS) void mcl_resample_kernel(const unsigned long long* __restrict__ cum,
                                                                   const int* __restrict__ particles, int N,
                                                                   unsigned long long W, unsigned long long q,
                                                                   int* __restrict__ out) {
  const int j = blockIdx.x * MCL_THREADS + threadIdx.x;
  if (j >= N) return;
  const unsigned long long t = (unsigned long long)j * W + q;      // < 2^52
  int lo = 0, hi = N - 1;                                   // cum[N - 1] * N = W * N > t: the answer lies in [0, N - 1]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] * (unsigned long long)N > t) hi = mid; else lo = mid + 1;
  }
  out[3 * j] = particles[3 * lo];
  out[3 * j + 1] = particles[3 * lo + 1];
  out[3 * j + 2] = particles[3 * lo + 2];
}

bool mcl_map_ok(int n_u, int n_v) { return n_u >= 1 && n_u <= MCL_MAX && n_v >= 1 && n_v <= MCL_MAX; }
bool mcl_step_ok(int v) { return v >= -MCL_MAX_STEP && v <= MCL_MAX_STEP; }
// do the n * 12 bytes at a and at b share a byte
bool mcl_overlap(const void* a, const void* b, int n) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, bytes = (uintptr_t)n * 12u;
  return pa < pb + bytes && pb < pa + bytes;
}

}  // namespace

extern "C" int gs_mcl_move(const int* particles, int n, const int* rot, int n_headings, const int* noise, int df, int dl,
                           int dh, int n_u, int n_v, int* out, gs_stream_t stream) {
  GS_REQUIRE(mcl_map_ok(n_u, n_v), "mcl_move: map %d x %d outside [1, 1024]", n_u, n_v);
  GS_REQUIRE(n >= 0 && n <= MCL_MAX_PARTICLES, "mcl_move: %d particles (0 .. %d)", n, MCL_MAX_PARTICLES);
  GS_REQUIRE(n_headings >= 1 && n_headings <= MCL_MAX_HEADINGS, "mcl_move: %d headings (1 .. %d)", n_headings,
             MCL_MAX_HEADINGS);
  GS_REQUIRE(mcl_step_ok(df) && mcl_step_ok(dl) && mcl_step_ok(dh), "mcl_move: odometry (%d, %d, %d) beyond 2^20", df, dl, dh);
  GS_REQUIRE(particles && rot && noise && out, "mcl_move: null pointer");
  GS_REQUIRE(out == particles || !mcl_overlap(particles, out, n),
             "mcl_move: out must be the particles themselves or share no byte with them");
  if (n == 0) return GS_OK;
  GS_TIMING_PRE();
  mcl_move_kernel<<<gs_cdiv(n, MCL_THREADS), MCL_THREADS, 0, (hipStream_t)stream>>>(particles, n, rot, n_headings, noise, df,
                                                                                   dl, dh, n_u, n_v, out);
  GS_CHECK_LAUNCH("mcl_move");
  return GS_OK;
}

extern "C" int gs_mcl_weigh(const unsigned char* cost, const unsigned char* cells, int n_u, int n_v, const int* particles,
                            int n, const int* ends, int n_headings, int n_beams, int cap, int allow_unknown,
                            unsigned int* S, unsigned long long* best, gs_stream_t stream) {
  GS_REQUIRE(mcl_map_ok(n_u, n_v), "mcl_weigh: map %d x %d outside [1, 1024]", n_u, n_v);
  GS_REQUIRE(n >= 0 && n <= MCL_MAX_PARTICLES, "mcl_weigh: %d particles (0 .. %d)", n, MCL_MAX_PARTICLES);
  GS_REQUIRE(n_headings >= 1 && n_headings <= MCL_MAX_HEADINGS && n_beams >= 1 && n_beams <= MCL_MAX_BEAMS,
             "mcl_weigh: %d headings (1 .. %d), %d beams (1 .. %d)", n_headings, MCL_MAX_HEADINGS, n_beams, MCL_MAX_BEAMS);
  GS_REQUIRE(cap >= 1 && cap <= MCL_MAX_CAP, "mcl_weigh: cap=%d outside [1, %d]", cap, MCL_MAX_CAP);
  GS_REQUIRE(allow_unknown == 0 || allow_unknown == 1, "mcl_weigh: allow_unknown=%d is not 0 or 1", allow_unknown);
  GS_REQUIRE(cost && cells && particles && ends && S && best, "mcl_weigh: null pointer");
  GS_REQUIRE((uintptr_t)ends % 8 == 0 && (uintptr_t)best % 8 == 0, "mcl_weigh: ends or best is not 8-byte aligned");
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(best, 0xff, sizeof(unsigned long long), s) != hipSuccess) {
    gs_set_error("mcl_weigh: cannot reset best");
    return GS_ERR_LAUNCH;
  }
  if (n == 0) return GS_OK;
  GS_TIMING_PRE();
  mcl_weigh_kernel<<<gs_cdiv(n, MCL_WAVES), MCL_THREADS, 0, s>>>(cost, cells, n_u, n_v, particles, n, (const int2*)ends,
                                                                 n_headings, n_beams, cap, allow_unknown, S, best);
  GS_CHECK_LAUNCH("mcl_weigh");
  return GS_OK;
}

extern "C" int gs_mcl_estimate(const unsigned int* S, const int* particles, int n, const int* rot, int n_headings,
                               const unsigned int* lut, int n_lut, unsigned int* w, unsigned long long* cum,
                               unsigned long long* stats, gs_stream_t stream) {
  GS_REQUIRE(n >= 0 && n <= MCL_MAX_PARTICLES, "mcl_estimate: %d particles (0 .. %d)", n, MCL_MAX_PARTICLES);
  GS_REQUIRE(n_headings >= 1 && n_headings <= MCL_MAX_HEADINGS, "mcl_estimate: %d headings (1 .. %d)", n_headings,
             MCL_MAX_HEADINGS);
  GS_REQUIRE(n_lut >= 1 && n_lut <= MCL_MAX_LUT, "mcl_estimate: a table of %d weights (1 .. %d)", n_lut, MCL_MAX_LUT);
  GS_REQUIRE(S && particles && rot && lut && w && cum && stats, "mcl_estimate: null pointer");
  GS_REQUIRE((uintptr_t)cum % 8 == 0 && (uintptr_t)stats % 8 == 0, "mcl_estimate: cum or stats is not 8-byte aligned");
  if (n == 0) return GS_OK;
  GS_TIMING_PRE();
  mcl_estimate_kernel<<<1, MCL_EST_THREADS, 0, (hipStream_t)stream>>>(S, particles, n, rot, n_headings, lut, n_lut, w, cum,
                                                                      stats);
  GS_CHECK_LAUNCH("mcl_estimate");
  return GS_OK;
}

extern "C" int gs_mcl_resample(const unsigned long long* cum, const int* particles, int n, unsigned long long W,
                               unsigned long long q, int* out, gs_stream_t stream) {
  GS_REQUIRE(n >= 0 && n <= MCL_MAX_PARTICLES, "mcl_resample: %d particles (0 .. %d)", n, MCL_MAX_PARTICLES);
  GS_REQUIRE(W >= 1 && W <= MCL_MAX_W && q < W, "mcl_resample: W=%llu (1 .. 2^36), q=%llu (below W)", W, q);
  GS_REQUIRE(cum && particles && out, "mcl_resample: null pointer");
  GS_REQUIRE((uintptr_t)cum % 8 == 0, "mcl_resample: cum is not 8-byte aligned");
  GS_REQUIRE(!mcl_overlap(particles, out, n > 0 ? n : 1), "mcl_resample: out shares memory with the particles it reads");
  if (n == 0) return GS_OK;
  GS_TIMING_PRE();
  mcl_resample_kernel<<<gs_cdiv(n, MCL_THREADS), MCL_THREADS, 0, (hipStream_t)stream>>>(cum, particles, n, W, q, out);
  GS_CHECK_LAUNCH("mcl_resample");
  return GS_OK;
}
