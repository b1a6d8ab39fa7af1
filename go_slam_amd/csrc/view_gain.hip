// View gain: the distinct unknown, free and solid cells of a state lattice that the rays of a camera cross from a
// candidate pose before something solid stops them (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_view_gain*); tests/view_gain_restatement.py restates it serially.  Integer only.
//
// view_gain_kernel: one workgroup per view.  The visited set is one bit per cell of the box around the origin, in dynamic
//   LDS sized by the box (a small box lets several workgroups share a CU; the largest takes 128 KiB and the CU alone).
//   The lanes zero the mask, meet at a barrier and stride over the rays.  A ray walks cell by cell: the next axis is the
//   one whose crossing time (2 k + 1) / (2 w) is smallest, compared by cross-multiplying in i32.  Every visited cell costs
//   one byte load of `state` -- each ray needs it, a solid cell ends the ray and an unknown one counts toward max_unknown
//   -- and one returning LDS atomic OR on the cell's word; the two do not depend on each other and are in flight together.
//   The lane whose OR set the bit counts the cell in registers, so every cell is counted exactly once whatever the order
//   in which rays and lanes arrive.  The counts are summed per wave by butterflies, then through LDS, and lane 0 stores
//   the four words.  No global atomics, no floating point, no scratch.
// VIEW_READ_FIRST=1 (measurement builds only): read the word first and skip the atomic when the bit is already set.  Near
//   the origin every ray crosses the same cells, so most ORs set nothing -- yet it measured 2.2 % slower (DESIGN.md
//   section 27, profiles/view_gain.json), so every visit issues the atomic.  (Likely, not isolated: the returning OR costs
//   the LDS what the read costs it, and a first visit then pays for both, one after the other.)
// VIEW_PACKED (measurement builds only): the walk reads a 2-bit copy of `state`, 16 cells to a word, that a pre-pass
//   writes into a buffer the build keeps for the life of the process.
// `make view_variants` (csrc/Makefile) builds the measurement libraries that tools/view_gain_bench.py --also takes.
#include "common.h"

namespace {

#ifndef VIEW_THREADS          // 16 waves: the largest box leaves one workgroup per CU, and the walk is a chain of latencies
#define VIEW_THREADS 1024
#endif
#ifndef VIEW_READ_FIRST
#define VIEW_READ_FIRST 0
#endif
#ifndef VIEW_PACKED
#define VIEW_PACKED 0
#endif
constexpr int VG_THREADS = VIEW_THREADS;
constexpr int VG_WAVES = VG_THREADS / GS_WAVE;
constexpr int VG_MAX = 1024;                                // cells per axis
constexpr int VG_MAX_RAYS = 65536;
constexpr int VG_MAX_RANGE2 = 3 * 1023 * 1023;

struct VgBox { int lo0, lo1, lo2, hi0, hi1, hi2; };

// words of the bit mask, rounded so that the reduction area behind it starts 16-byte aligned
__host__ __device__ inline unsigned vg_mask_words(unsigned cells) { return ((cells + 31u) / 32u + 3u) & ~3u; }

// the cells of a box the call accepts, or 0: lo <= 0 <= hi on every axis and at most GS_VIEW_MAX_BOX_CELLS cells
long long vg_box_cells(const int* box) {
  if (!box) return 0;
  long long cells = 1;
  for (int a = 0; a < 3; ++a) {
    if (box[a] > 0 || box[3 + a] < 0) return 0;
    cells *= (long long)box[3 + a] - (long long)box[a] + 1;          // each factor < 2^32, the running product <= 2^20
    if (cells > GS_VIEW_MAX_BOX_CELLS) return 0;
  }
  return cells;
}

int vg_isqrt(long long v) {
  long long r = 0;
  while ((r + 1) * (r + 1) <= v) ++r;                       // v <= 3 * GS_VIEW max range2: a few thousand steps, on the host
  return (int)r;
}

#if VIEW_PACKED
constexpr int VG_PACK_THREADS = 256;
__global__ __launch_bounds__(VG_PACK_THREADS) void view_pack_kernel(const unsigned char* __restrict__ state, int n,
                                                                    unsigned* __restrict__ packed) {
  const int w = blockIdx.x * VG_PACK_THREADS + threadIdx.x;
  if (w * 16 >= n) return;
  unsigned v = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = w * 16 + i;
    const unsigned s = p < n ? state[p] : 2u;
    v |= (s > 2u ? 2u : s) << (2 * i);
  }
  packed[w] = v;
}
#endif

// the state of cell p: a byte of `state`, or in a VIEW_PACKED build two bits of the pre-pass's copy
__device__ __forceinline__ unsigned vg_state(const unsigned char* __restrict__ cells, int p) {
#if VIEW_PACKED
  return (((const unsigned*)cells)[p >> 4] >> (2 * (p & 15))) & 3u;
#else
  return cells[p];
#endif
}

__global__ __launch_bounds__(VG_THREADS) void view_gain_kernel(const unsigned char* __restrict__ cells, int n0, int n1, int n2,
                                                               const int* __restrict__ origins,
                                                               const int* __restrict__ dirs, int n_rays, int range2,
                                                               int max_unknown, VgBox box, int max_steps,
                                                               unsigned* __restrict__ gain) {
  extern __shared__ __attribute__((aligned(16))) unsigned vg_lds[];
  const int tid = threadIdx.x;
  const int lane = tid & (GS_WAVE - 1), wave = tid / GS_WAVE;
  const int v = blockIdx.x;
  const int s1 = box.hi1 - box.lo1 + 1, s2 = box.hi2 - box.lo2 + 1;
  const unsigned words = vg_mask_words((unsigned)((box.hi0 - box.lo0 + 1) * s1 * s2));
  unsigned* mask = vg_lds;
  unsigned* red = vg_lds + words;                           // [VG_WAVES][3]
  for (unsigned i = tid; i < words; i += VG_THREADS) mask[i] = 0u;
  __syncthreads();

  const int o0 = origins[3 * v], o1 = origins[3 * v + 1], o2 = origins[3 * v + 2];
  const bool inside = o0 >= 0 && o0 < n0 && o1 >= 0 && o1 < n1 && o2 >= 0 && o2 < n2;
  int cnt_u = 0, cnt_f = 0, cnt_s = 0;
  for (int r = tid; inside && r < n_rays; r += VG_THREADS) {
    const int d0 = dirs[3 * r], d1 = dirs[3 * r + 1], d2 = dirs[3 * r + 2];
    // an all-zero direction casts nothing; neither does one outside the contract, whose products would leave i32 (the
    // signed values are tested: the most negative int has no absolute value)
    if ((d0 | d1 | d2) == 0 || d0 < -GS_VIEW_MAX_DIR || d0 > GS_VIEW_MAX_DIR || d1 < -GS_VIEW_MAX_DIR ||
        d1 > GS_VIEW_MAX_DIR || d2 < -GS_VIEW_MAX_DIR || d2 > GS_VIEW_MAX_DIR)
      continue;
    const int w0 = d0 < 0 ? -d0 : d0, w1 = d1 < 0 ? -d1 : d1, w2 = d2 < 0 ? -d2 : d2;
    const int g0 = d0 < 0 ? -1 : 1, g1 = d1 < 0 ? -1 : 1, g2 = d2 < 0 ? -1 : 1;
    int f0 = 0, f1 = 0, f2 = 0;                             // the offset from the origin; |f_a| is the step counter k_a
    int m0 = 1, m1 = 1, m2 = 1;                             // 2 k_a + 1
    int unknown = 0;
    for (int step = 0;; ++step) {
      // visit o + f: inside the lattice, the box and the range
      const int p = ((o0 + f0) * n1 + (o1 + f1)) * n2 + (o2 + f2);
      const int bit = ((f0 - box.lo0) * s1 + (f1 - box.lo1)) * s2 + (f2 - box.lo2);
      const unsigned m = 1u << (bit & 31);
      const unsigned st = vg_state(cells, p);
#if VIEW_READ_FIRST
      unsigned old = mask[bit >> 5];
      if (!(old & m)) old = atomicOr(&mask[bit >> 5], m);
#else
      const unsigned old = atomicOr(&mask[bit >> 5], m);
#endif
      if (!(old & m)) {
        cnt_u += st == 0u;
        cnt_f += st == 1u;
        cnt_s += st > 1u;
      }
      if (st > 1u) break;
      if (st == 0u && ++unknown == max_unknown) break;      // max_unknown == 0: never equal, no limit
      if (step >= max_steps) break;                         // never taken before the range ends the ray; bounds the loop
      // the next cell: the axis with the smallest (2 k + 1) / (2 w), ties to the lower axis.  An axis with w == 0 never
      // beats another and is beaten by every axis with w > 0; products stay below 3545 * 32767 < 2^31
      const bool b1 = m1 * w0 < m0 * w1;
      const int mb = b1 ? m1 : m0, wb = b1 ? w1 : w0;
      const bool b2 = m2 * wb < mb * w2;
      const int e0 = f0 + ((!b1 && !b2) ? g0 : 0), e1 = f1 + ((b1 && !b2) ? g1 : 0), e2 = f2 + (b2 ? g2 : 0);
      const int c0 = o0 + e0, c1 = o1 + e1, c2 = o2 + e2;
      if (c0 < 0 || c0 >= n0 || c1 < 0 || c1 >= n1 || c2 < 0 || c2 >= n2) break;
      if (e0 < box.lo0 || e0 > box.hi0 || e1 < box.lo1 || e1 > box.hi1 || e2 < box.lo2 || e2 > box.hi2) break;
      if (e0 * e0 + e1 * e1 + e2 * e2 > range2) break;
      f0 = e0, f1 = e1, f2 = e2;
      m0 += (!b1 && !b2) ? 2 : 0, m1 += (b1 && !b2) ? 2 : 0, m2 += b2 ? 2 : 0;
    }
  }
  cnt_u = gs_wave_sum_i32(cnt_u);
  cnt_f = gs_wave_sum_i32(cnt_f);
  cnt_s = gs_wave_sum_i32(cnt_s);
  if (lane == 0) {
    red[3 * wave] = (unsigned)cnt_u;
    red[3 * wave + 1] = (unsigned)cnt_f;
    red[3 * wave + 2] = (unsigned)cnt_s;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned u = 0, f = 0, s = 0;
    for (int i = 0; i < VG_WAVES; ++i) u += red[3 * i], f += red[3 * i + 1], s += red[3 * i + 2];
    gain[4 * (size_t)v] = u;
    gain[4 * (size_t)v + 1] = f;
    gain[4 * (size_t)v + 2] = s;
    gain[4 * (size_t)v + 3] = u + f + s;
  }
}

}  // namespace

extern "C" size_t gs_view_gain_lds_bytes(const int* box) {
  const long long cells = vg_box_cells(box);
  if (cells == 0) return 0;
  return sizeof(unsigned) * ((size_t)vg_mask_words((unsigned)cells) + 3 * VG_WAVES);
}

extern "C" int gs_view_gain(const unsigned char* state, int n0, int n1, int n2, const int* origins, int n_views,
                            const int* dirs, int n_rays, int range2, int max_unknown, const int* box, unsigned int* gain,
                            gs_stream_t stream) {
  GS_REQUIRE(n0 >= 1 && n0 <= VG_MAX && n1 >= 1 && n1 <= VG_MAX && n2 >= 1 && n2 <= VG_MAX,
             "view_gain: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(n_views >= 0 && n_rays >= 1 && n_rays <= VG_MAX_RAYS, "view_gain: %d views, %d rays (1 .. %d)", n_views,
             n_rays, VG_MAX_RAYS);
  GS_REQUIRE(range2 >= 1 && range2 <= VG_MAX_RANGE2 && max_unknown >= 0, "view_gain: range2=%d (1 .. %d) max_unknown=%d",
             range2, VG_MAX_RANGE2, max_unknown);
  GS_REQUIRE(state && origins && dirs && box && gain, "view_gain: null pointer");
  const size_t lds = gs_view_gain_lds_bytes(box);
  GS_REQUIRE(lds != 0, "view_gain: box [%d..%d] x [%d..%d] x [%d..%d] must hold offset 0 on every axis and at most %d cells",
             box[0], box[3], box[1], box[4], box[2], box[5], GS_VIEW_MAX_BOX_CELLS);
  if (n_views == 0) return GS_OK;
  const hipStream_t s = (hipStream_t)stream;
  const VgBox b = {box[0], box[1], box[2], box[3], box[4], box[5]};
  const int steps = vg_isqrt(3LL * range2);                 // the offsets never shrink: |f|_1 <= sqrt(3) |f|_2
  const int max_steps = steps < n0 + n1 + n2 ? steps : n0 + n1 + n2;
  const unsigned char* cells = state;
#if VIEW_PACKED
  // measurement build: one buffer for the largest lattice a process has asked for, kept until the process ends
  static unsigned* pack_buf = nullptr;
  static size_t pack_words = 0;
  const size_t need = ((size_t)n0 * n1 * n2 + 15) / 16;
  if (need > pack_words) {
    if (pack_buf) (void)hipFree(pack_buf);                  // synchronises: no launch still reads it
    pack_buf = nullptr, pack_words = 0;
    if (hipMalloc((void**)&pack_buf, sizeof(unsigned) * need) != hipSuccess) {
      gs_set_error("view_gain: no memory for the packed state");
      return GS_ERR_LAUNCH;
    }
    pack_words = need;
  }
  cells = (const unsigned char*)pack_buf;
#endif
  static GsLdsLimit limit;
  if (int rc = limit.raise((const void*)view_gain_kernel, lds, "view_gain")) return rc;
  GS_TIMING_PRE();
#if VIEW_PACKED
  view_pack_kernel<<<gs_cdiv(gs_cdiv(n0 * n1 * n2, 16), VG_PACK_THREADS), VG_PACK_THREADS, 0, s>>>(state, n0 * n1 * n2,
                                                                                                 pack_buf);
  GS_CHECK_LAUNCH("view_pack");
#endif
  view_gain_kernel<<<(unsigned)n_views, VG_THREADS, lds, s>>>(cells, n0, n1, n2, origins, dirs, n_rays, range2, max_unknown,
                                                             b, max_steps, gain);
  GS_CHECK_LAUNCH("view_gain");
  return GS_OK;
}
