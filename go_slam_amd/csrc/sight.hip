// Line of sight over a passability lattice and the shortest shortcut of a planned path (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_segment_* / gs_path_*); tests/sight_restatement.py restates it serially.  Integer
// apart from the fp64 sqrt of a leg's length (sight_walk.h).
//
// segment_sight_kernel / segment_min_kernel: one lane per segment, the walk of sight_walk.h with a visitor that stops at
//   the first blocked cell, or keeps the smallest (value, index).
// path_sight_kernel: one wave per (path cell j, 64 consecutive earlier cells): lane b walks from cell j - 1 - b to cell j,
//   neighbouring lanes nearly the same direction and length; the wave's ballot is the row's word, one 8-byte store by
//   lane 0.  Every word of the matrix is written, so the caller clears nothing.
// path_shortcut_kernel: one workgroup, sequential in j: the lanes stride over the window, the minimum of the key
//   (dp[i] + len) << 32 | i goes by a wave butterfly and then across the waves through two alternating rows of LDS
//   slots, so a step costs one barrier.  Lane b = 0 is always thread 0's, which wrote dp[j - 1] itself; every other
//   dp[i] a thread reads was written before the barrier of the step before.  Thread 0 then walks the predecessors back.
// No global atomics, no inline assembly, no scratch.
#include "common.h"
#include "sight_walk.h"

namespace {

constexpr int SIGHT_THREADS = 256;
constexpr int SIGHT_WAVES = SIGHT_THREADS / GS_WAVE;
constexpr int SIGHT_MAX = 1024;                             // cells per axis
constexpr int SIGHT_INF = 0x7fffffff;                       // dp of a cell no route reaches

__device__ __forceinline__ bool sight_inside(int c0, int c1, int c2, int n0, int n1, int n2) {
  return c0 >= 0 && c0 < n0 && c1 >= 0 && c1 < n1 && c2 >= 0 && c2 < n2;
}

__device__ __forceinline__ bool sight_sees(const unsigned char* __restrict__ passable, int a0, int a1, int a2, int b0,
                                           int b1, int b2, int n1, int n2) {
  return sight_walk(a0, a1, a2, b0, b1, b2, n1, n2, [&](int at) { return passable[at] != 0; });
}

__global__ __launch_bounds__(SIGHT_THREADS) void segment_sight_kernel(const unsigned char* __restrict__ passable, int n0,
                                                                      int n1, int n2, const int* __restrict__ segs, int n,
                                                                      unsigned char* __restrict__ out) {
  const int p = blockIdx.x * SIGHT_THREADS + threadIdx.x;
  if (p >= n) return;
  const int* s = segs + (size_t)p * 6;
  const int a0 = s[0], a1 = s[1], a2 = s[2], b0 = s[3], b1 = s[4], b2 = s[5];
  bool sees = sight_inside(a0, a1, a2, n0, n1, n2) && sight_inside(b0, b1, b2, n0, n1, n2);
  if (sees) sees = sight_sees(passable, a0, a1, a2, b0, b1, b2, n1, n2);
  out[p] = sees ? 1 : 0;
}

__global__ __launch_bounds__(SIGHT_THREADS) void segment_min_kernel(const int* __restrict__ field, int n0, int n1, int n2,
                                                                    const int* __restrict__ segs, int n,
                                                                    int* __restrict__ out_value,
                                                                    int* __restrict__ out_cell) {
  const int p = blockIdx.x * SIGHT_THREADS + threadIdx.x;
  if (p >= n) return;
  const int* s = segs + (size_t)p * 6;
  const int a0 = s[0], a1 = s[1], a2 = s[2], b0 = s[3], b1 = s[4], b2 = s[5];
  int value = (int)0x80000000, cell = -1;
  if (sight_inside(a0, a1, a2, n0, n1, n2) && sight_inside(b0, b1, b2, n0, n1, n2)) {
    value = 0x7fffffff;
    cell = 0x7fffffff;
    sight_walk(a0, a1, a2, b0, b1, b2, n1, n2, [&](int at) {
      const int v = field[at];
      if (v < value || (v == value && at < cell)) {
        value = v;
        cell = at;
      }
      return true;
    });
  }
  out_value[p] = value;
  out_cell[p] = cell;
}

__global__ __launch_bounds__(SIGHT_THREADS) void path_sight_kernel(const unsigned char* __restrict__ passable, int n0,
                                                                   int n1, int n2, const int* __restrict__ cells, int L,
                                                                   int window, int words,
                                                                   unsigned long long* __restrict__ sight) {
  const int lane = threadIdx.x & (GS_WAVE - 1);
  const long long row_word = (long long)blockIdx.x * SIGHT_WAVES + threadIdx.x / GS_WAVE;      // wave-uniform
  if (row_word >= (long long)L * words) return;
  const int j = (int)(row_word / words), word = (int)(row_word % words);
  const int b = word * GS_WAVE + lane;
  const int reach = window < j ? window : j;                // bits [0, reach) of row j exist
  bool sees = false;
  if (word * GS_WAVE < reach) {
    const int j0 = cells[(size_t)j * 3 + 0], j1 = cells[(size_t)j * 3 + 1], j2 = cells[(size_t)j * 3 + 2];
    if (b < reach && sight_inside(j0, j1, j2, n0, n1, n2)) {
      const int i = j - 1 - b;
      const int i0 = cells[(size_t)i * 3 + 0], i1 = cells[(size_t)i * 3 + 1], i2 = cells[(size_t)i * 3 + 2];
      // the walk visits both ends, so a blocked path cell sees nothing
      if (sight_inside(i0, i1, i2, n0, n1, n2)) sees = sight_sees(passable, i0, i1, i2, j0, j1, j2, n1, n2);
    }
  }
  const unsigned long long bits = __ballot(sees);
  if (lane == 0) sight[row_word] = bits;
}

// dynamic LDS: dp i32 [L], then the predecessors u16 [L]
__global__ __launch_bounds__(SIGHT_THREADS) void path_shortcut_kernel(const unsigned long long* __restrict__ sight,
                                                                      const int* __restrict__ cells, int L, int window,
                                                                      int words, int* __restrict__ index,
                                                                      int* __restrict__ n_out, int* __restrict__ length) {
  extern __shared__ __attribute__((aligned(16))) int sc_lds[];
  __shared__ unsigned long long slots[2][SIGHT_WAVES];
  int* dp = sc_lds;
  unsigned short* pred = reinterpret_cast<unsigned short*>(sc_lds + L);
  const int tid = threadIdx.x, lane = tid & (GS_WAVE - 1), wave = tid / GS_WAVE;
  const unsigned long long none = ~0ull;
  if (tid == 0) {
    dp[0] = 0;
    pred[0] = 0;
  }
  for (int j = 1; j < L; ++j) {
    const int reach = window < j ? window : j;
    const int j0 = cells[(size_t)j * 3 + 0], j1 = cells[(size_t)j * 3 + 1], j2 = cells[(size_t)j * 3 + 2];
    unsigned long long key = none;
    for (int b = tid; b < reach; b += SIGHT_THREADS) {
      if ((sight[(size_t)j * words + (b >> 6)] >> (b & 63) & 1ull) == 0) continue;
      const int i = j - 1 - b;
      const int before = dp[i];
      if (before == SIGHT_INF) continue;
      const long long cand = (long long)before + sight_leg_length(j0 - cells[(size_t)i * 3 + 0],
                                                                  j1 - cells[(size_t)i * 3 + 1],
                                                                  j2 - cells[(size_t)i * 3 + 2]);
      if (cand >= SIGHT_INF) continue;
      const unsigned long long k = (unsigned long long)cand << 32 | (unsigned)i;
      key = k < key ? k : key;
    }
    key = gs_wave_min_u64(key);
    if (lane == 0) slots[j & 1][wave] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < SIGHT_WAVES; ++w) key = slots[j & 1][w] < key ? slots[j & 1][w] : key;
      dp[j] = key == none ? SIGHT_INF : (int)(key >> 32);
      pred[j] = key == none ? 0 : (unsigned short)(key & 0xffffu);
    }
  }
  if (tid != 0) return;
  if (dp[L - 1] == SIGHT_INF) {
    n_out[0] = -1;
    return;
  }
  int kept = 1;
  for (int j = L - 1; j > 0; j = pred[j]) ++kept;           // pred[j] < j: at most L steps
  int at = kept;
  for (int j = L - 1; j > 0; j = pred[j]) index[--at] = j;
  index[0] = 0;
  n_out[0] = kept;
  length[0] = dp[L - 1];
}

bool sight_dims_ok(int n0, int n1, int n2) {
  return n0 >= 1 && n0 <= SIGHT_MAX && n1 >= 1 && n1 <= SIGHT_MAX && n2 >= 1 && n2 <= SIGHT_MAX;
}
bool sight_window_ok(int L, int window) {
  return L >= 1 && L <= GS_PATH_MAX_CELLS && window >= 1 && window <= (L > 1 ? L - 1 : 1);
}

}  // namespace

extern "C" int gs_segment_sight(const unsigned char* passable, int n0, int n1, int n2, const int* segs, int n,
                                unsigned char* out, gs_stream_t stream) {
  GS_REQUIRE(sight_dims_ok(n0, n1, n2), "segment_sight: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(n >= 0 && n <= (1 << 30), "segment_sight: n=%d outside [0, 2^30]", n);
  GS_REQUIRE(passable && segs && out, "segment_sight: null pointer");
  if (n == 0) return GS_OK;
  GS_TIMING_PRE();
  segment_sight_kernel<<<gs_cdiv(n, SIGHT_THREADS), SIGHT_THREADS, 0, (hipStream_t)stream>>>(passable, n0, n1, n2, segs,
                                                                                            n, out);
  GS_CHECK_LAUNCH("segment_sight");
  return GS_OK;
}

extern "C" int gs_segment_min(const int* field, int n0, int n1, int n2, const int* segs, int n, int* out_value,
                              int* out_cell, gs_stream_t stream) {
  GS_REQUIRE(sight_dims_ok(n0, n1, n2), "segment_min: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(n >= 0 && n <= (1 << 30), "segment_min: n=%d outside [0, 2^30]", n);
  GS_REQUIRE(field && segs && out_value && out_cell, "segment_min: null pointer");
  if (n == 0) return GS_OK;
  GS_TIMING_PRE();
  segment_min_kernel<<<gs_cdiv(n, SIGHT_THREADS), SIGHT_THREADS, 0, (hipStream_t)stream>>>(field, n0, n1, n2, segs, n,
                                                                                          out_value, out_cell);
  GS_CHECK_LAUNCH("segment_min");
  return GS_OK;
}

extern "C" int gs_path_sight(const unsigned char* passable, int n0, int n1, int n2, const int* cells, int L, int window,
                             unsigned long long* sight, gs_stream_t stream) {
  GS_REQUIRE(sight_dims_ok(n0, n1, n2), "path_sight: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(sight_window_ok(L, window), "path_sight: L=%d (1 .. %d), window=%d (1 .. max(L - 1, 1))", L,
             GS_PATH_MAX_CELLS, window);
  GS_REQUIRE(passable && cells && sight, "path_sight: null pointer");
  GS_REQUIRE((uintptr_t)sight % 8 == 0, "path_sight: sight is not 8-byte aligned");
  const int words = gs_cdiv(window, GS_WAVE);
  const long long waves = (long long)L * words;             // at most 16384 * 256
  GS_TIMING_PRE();
  path_sight_kernel<<<(unsigned)((waves + SIGHT_WAVES - 1) / SIGHT_WAVES), SIGHT_THREADS, 0, (hipStream_t)stream>>>(
      passable, n0, n1, n2, cells, L, window, words, sight);
  GS_CHECK_LAUNCH("path_sight");
  return GS_OK;
}

extern "C" int gs_path_shortcut(const unsigned long long* sight, const int* cells, int L, int window, int* index,
                                int* n_out, int* length, gs_stream_t stream) {
  GS_REQUIRE(sight_window_ok(L, window), "path_shortcut: L=%d (1 .. %d), window=%d (1 .. max(L - 1, 1))", L,
             GS_PATH_MAX_CELLS, window);
  GS_REQUIRE(sight && cells && index && n_out && length, "path_shortcut: null pointer");
  GS_REQUIRE((uintptr_t)sight % 8 == 0, "path_shortcut: sight is not 8-byte aligned");
  const size_t lds = gs_align((size_t)L * (sizeof(int) + sizeof(unsigned short)), 16);     // at most 96 KiB
  static GsLdsLimit limit;
  if (int rc = limit.raise((const void*)path_shortcut_kernel, lds, "path_shortcut")) return rc;
  GS_TIMING_PRE();
  path_shortcut_kernel<<<1, SIGHT_THREADS, lds, (hipStream_t)stream>>>(sight, cells, L, window, gs_cdiv(window, GS_WAVE),
                                                                      index, n_out, length);
  GS_CHECK_LAUNCH("path_shortcut");
  return GS_OK;
}
