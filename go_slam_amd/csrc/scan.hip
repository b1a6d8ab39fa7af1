// Planar range scans on a 2-D occupancy map and the exhaustive correlative scan match (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_scan_*); tests/scan_restatement.py restates it serially; DESIGN.md section 36.
// Integer arithmetic only (the one fp64 sqrt of sight_leg_length is corrected to the exact floor).
//
// scan_cast_kernel   one lane per (pose, beam): the two-axis form of view-gain's walk, restated here -- view_gain.hip's
//                    loop carries the box, the bit mask and the unknown counter of its three-axis walk, and a shared
//                    header would not leave it the same kernel.  A chain of dependent byte loads per lane.
// scan_field_kernel  one launch: a 16 x 64 tile of cells per workgroup, the site flags of the tile and a halo of R cells
//                    in LDS, the band-limited minimum along v for every row of tile and halo, a barrier, the one along u.
//                    Both passes keep min(., cap): a site more than R cells away along either axis is beyond the cap.
// scan_match_kernel  four consecutive translations along v per lane, a wave per 256 consecutive v of one (yaw, u): per
//                    beam one unaligned dword load per lane where its four end points lie inside the row (256 consecutive
//                    bytes of one row of `cost` per wave), else four guarded byte loads.  The beam offsets are read at
//                    wave-uniform addresses (scalar loads).  The wave's best (score << 32 | index) goes through a
//                    butterfly and, when it beats the value `best` holds at that moment, one 64-bit atomic min.
// SCAN_MATCH_V4=0 (measurement builds only): the form this kernel started as, one translation and one byte load per lane
//                    and beam, 64 consecutive v per wave; it measured 2.4 times slower on a 400 x 400 map (DESIGN.md
//                    section 36, profiles/scan.json).
#include "common.h"
#include "sight_walk.h"

namespace {

#ifndef SCAN_MATCH_V4
#define SCAN_MATCH_V4 1
#endif
constexpr int SCAN_MAX = 1024;                              // cells per side
constexpr int SCAN_MAX_BEAMS = 4096;
constexpr int SCAN_MAX_YAWS = 1024;
constexpr int SCAN_MAX_RANGE2 = 2 * 1023 * 1023;
constexpr long long SCAN_MAX_LANES = 1ll << 28;             // (pose, beam) pairs of a cast, candidates of a match
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_FREE = 254, SCAN_UNKNOWN = 205;
constexpr int SCAN_R_MAX = 15;
constexpr int FIELD_TU = 16, FIELD_TV = 64;
constexpr int FIELD_SPAN_U = FIELD_TU + 2 * SCAN_R_MAX, FIELD_SPAN_V = FIELD_TV + 2 * SCAN_R_MAX;
constexpr int MATCH_V = SCAN_MATCH_V4 ? 4 : 1;              // consecutive v per lane
constexpr int MATCH_CHUNK = GS_WAVE * MATCH_V;              // consecutive v per wave

int scan_isqrt(long long v) {
  long long r = 0;
  while ((r + 1) * (r + 1) <= v) ++r;                       // v <= 2 * SCAN_MAX_RANGE2: a few thousand steps, on the host
  return (int)r;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_cast_kernel(const unsigned char* __restrict__ cells, int n_u, int n_v,
                                                                 const int* __restrict__ poses,
                                                                 const int* __restrict__ dirs, int n_lanes, int n_beams,
                                                                 int range2, int stop_unknown, int max_steps,
                                                                 unsigned char* __restrict__ kind, int* __restrict__ hit,
                                                                 int* __restrict__ range_mc) {
  const int idx = blockIdx.x * SCAN_THREADS + threadIdx.x;
  if (idx >= n_lanes) return;
  const int p = idx / n_beams;
  const int o0 = poses[2 * p], o1 = poses[2 * p + 1];
  const int d0 = dirs[2 * (size_t)idx], d1 = dirs[2 * (size_t)idx + 1];
  int out_kind = 0, out_hit = -1, out_range = -1;
  // a pose outside the map, an all-zero direction and one outside the contract (whose products would leave i32) cast nothing
  const bool casts = o0 >= 0 && o0 < n_u && o1 >= 0 && o1 < n_v && (d0 | d1) != 0 && d0 >= -GS_VIEW_MAX_DIR &&
                     d0 <= GS_VIEW_MAX_DIR && d1 >= -GS_VIEW_MAX_DIR && d1 <= GS_VIEW_MAX_DIR;
  if (casts) {
    const int w0 = d0 < 0 ? -d0 : d0, w1 = d1 < 0 ? -d1 : d1;
    const int g0 = d0 < 0 ? -1 : 1, g1 = d1 < 0 ? -1 : 1;
    int f0 = 0, f1 = 0;                                     // the offset from the origin; |f_a| is the step counter k_a
    int m0 = 1, m1 = 1;                                     // 2 k_a + 1
    for (int step = 0;; ++step) {
      const int at = (o0 + f0) * n_v + (o1 + f1);           // inside the map: the origin was tested, a step below
      const int c = cells[at];
      const bool unknown = c == SCAN_UNKNOWN;
      if ((c != SCAN_FREE && !unknown) || (unknown && stop_unknown)) {
        out_kind = unknown ? 2 : 1;
        out_hit = at;
        out_range = sight_leg_length(f0, f1, 0);
        break;
      }
      if (step >= max_steps) break;                         // never taken before the map or the range ends the ray
      // axis 1 only by a strictly earlier crossing; w_a == 0 never beats the other axis.  Products < 4099 * 32767 < 2^31
      const bool b1 = m1 * w0 < m0 * w1;
      const int e0 = f0 + (b1 ? 0 : g0), e1 = f1 + (b1 ? g1 : 0);
      const int c0 = o0 + e0, c1 = o1 + e1;
      if (c0 < 0 || c0 >= n_u || c1 < 0 || c1 >= n_v) break;
      if (e0 * e0 + e1 * e1 > range2) break;
      f0 = e0, f1 = e1;
      m0 += b1 ? 0 : 2, m1 += b1 ? 2 : 0;
    }
  }
  kind[idx] = (unsigned char)out_kind;
  hit[idx] = out_hit;
  range_mc[idx] = out_range;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_field_kernel(const unsigned char* __restrict__ cells, int n_u, int n_v,
                                                                  int R, unsigned char* __restrict__ cost) {
  __shared__ unsigned char site[FIELD_SPAN_U * FIELD_SPAN_V];        // 1 where an occupied cell of the map lies
  __shared__ unsigned char row_min[FIELD_SPAN_U * FIELD_TV];         // min(cap, squared distance along v) per row
  const int cap = R * R + 1;
  const int span_u = FIELD_TU + 2 * R, span_v = FIELD_TV + 2 * R;
  const int u0 = blockIdx.y * FIELD_TU - R, v0 = blockIdx.x * FIELD_TV - R;
  for (int i = threadIdx.x; i < span_u * span_v; i += SCAN_THREADS) {
    const int hu = i / span_v, hv = i - hu * span_v;
    const int u = u0 + hu, v = v0 + hv;
    int s = 0;
    if (u >= 0 && u < n_u && v >= 0 && v < n_v) {
      const int c = cells[(size_t)u * n_v + v];
      s = c != SCAN_FREE && c != SCAN_UNKNOWN;
    }
    site[i] = (unsigned char)s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < span_u * FIELD_TV; i += SCAN_THREADS) {
    const int hu = i / FIELD_TV, tv = i - hu * FIELD_TV;
    const unsigned char* at = site + hu * span_v + tv + R;
    int best = cap;
    for (int k = -R; k <= R; ++k) best = at[k] ? min(best, k * k) : best;
    row_min[i] = (unsigned char)best;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < FIELD_TU * FIELD_TV; i += SCAN_THREADS) {
    const int tu = i / FIELD_TV, tv = i - tu * FIELD_TV;
    const int u = u0 + R + tu, v = v0 + R + tv;
    if (u >= n_u || v >= n_v) continue;
    const unsigned char* at = row_min + (tu + R) * FIELD_TV + tv;
    int best = cap;
    for (int k = -R; k <= R; ++k) best = min(best, (int)at[k * FIELD_TV] + k * k);
    cost[(size_t)u * n_v + v] = (unsigned char)best;
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_match_kernel(
    const unsigned char* __restrict__ cost, const unsigned char* __restrict__ cells, int n_u, int n_v,
    const int* __restrict__ offsets, int n_beams, int u0, int v0, int w_u, int w_v, int chunks, int cap, int allow_unknown,
    unsigned* __restrict__ score, unsigned long long* __restrict__ best) {
  const int lane = threadIdx.x & (GS_WAVE - 1);
  // the wave's (u, chunk of v): the same for its 64 lanes, and known to be
  const int wid = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (SCAN_THREADS / GS_WAVE) + threadIdx.x / GS_WAVE));
  if (wid >= w_u * chunks) return;
  const int y = blockIdx.y;
  const int i = wid / chunks, j0 = (wid - i * chunks) * MATCH_CHUNK + lane * MATCH_V;
  const int u = u0 + i;
  const int* __restrict__ off = offsets + 2 * (size_t)y * n_beams;
  unsigned acc[MATCH_V];
#pragma unroll
  for (int q = 0; q < MATCH_V; ++q) acc[q] = 0u;
  const int v = v0 + j0;                                    // lanes past the window's end compute and store nothing
#pragma unroll 8
  for (int b = 0; b < n_beams; ++b) {
    const int du = off[2 * b], dv = off[2 * b + 1];
    const int uu = u + du;
    // an offset outside 16 bits counts as outside the map, so the sums below stay far inside i32
    const bool row_in = du >= -32768 && du <= 32767 && dv >= -32768 && dv <= 32767 && uu >= 0 && uu < n_u;
    const int vv = v + dv;
    const unsigned char* row = cost + (row_in ? uu * n_v : 0);
#if SCAN_MATCH_V4
    if (row_in && vv >= 0 && vv + 3 < n_v) {
      unsigned word;
      __builtin_memcpy(&word, row + vv, 4);                 // one unaligned dword
      acc[0] += word & 255u, acc[1] += (word >> 8) & 255u, acc[2] += (word >> 16) & 255u, acc[3] += word >> 24;
      continue;
    }
#endif
#pragma unroll
    for (int q = 0; q < MATCH_V; ++q) {
      const bool in = row_in && vv + q >= 0 && vv + q < n_v;
      const unsigned c = row[in ? vv + q : 0];              // always a load from inside the map: nothing to branch around
      acc[q] += in ? c : (unsigned)cap;
    }
  }
  unsigned long long key = ~0ull;
#pragma unroll
  for (int q = 0; q < MATCH_V; ++q) {
    const int j = j0 + q;
    if (j >= w_v) break;
    const int c = cells[u * n_v + v + q];
    const bool stands = c == SCAN_FREE || (allow_unknown && c == SCAN_UNKNOWN);
    const unsigned index = (unsigned)((y * w_u + i) * w_v + j);       // < 2^28
    const unsigned s = stands ? acc[q] : 0xffffffffu;
    score[index] = s;
    const unsigned long long k = stands ? ((unsigned long long)s << 32) | index : ~0ull;
    key = k < key ? k : key;
  }
  key = gs_wave_min_u64(key);
  // a minimum has no order: whichever waves get here first, `best` ends as the smallest key.  The plain read only spares
  // the atomic when it cannot change anything (a stale, larger value costs one atomic more, never a wrong result)
  if (lane == 0 && key != ~0ull && key < __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    __hip_atomic_fetch_min(best, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" int gs_scan_cast(const unsigned char* cells, int n_u, int n_v, const int* poses, int n_poses, const int* dirs,
                            int n_beams, int range2, int stop_unknown, unsigned char* kind, int* hit, int* range_mc,
                            gs_stream_t stream) {
  GS_REQUIRE(n_u >= 1 && n_u <= SCAN_MAX && n_v >= 1 && n_v <= SCAN_MAX, "scan_cast: map %d x %d outside [1, 1024]", n_u, n_v);
  GS_REQUIRE(n_poses >= 0 && n_beams >= 1 && n_beams <= SCAN_MAX_BEAMS && (long long)n_poses * n_beams <= SCAN_MAX_LANES,
             "scan_cast: %d poses, %d beams (1 .. %d, at most 2^28 rays in all)", n_poses, n_beams, SCAN_MAX_BEAMS);
  GS_REQUIRE(range2 >= 1 && range2 <= SCAN_MAX_RANGE2, "scan_cast: range2=%d (1 .. %d)", range2, SCAN_MAX_RANGE2);
  GS_REQUIRE(stop_unknown == 0 || stop_unknown == 1, "scan_cast: stop_unknown=%d is not 0 or 1", stop_unknown);
  GS_REQUIRE(cells && poses && dirs && kind && hit && range_mc, "scan_cast: null pointer");
  if (n_poses == 0) return GS_OK;
  const int steps = scan_isqrt(2LL * range2);               // the offsets never shrink: |f|_1 <= sqrt(2) |f|_2
  const int max_steps = steps < n_u + n_v ? steps : n_u + n_v;
  const int n_lanes = n_poses * n_beams;
  GS_TIMING_PRE();
  scan_cast_kernel<<<gs_cdiv(n_lanes, SCAN_THREADS), SCAN_THREADS, 0, (hipStream_t)stream>>>(
      cells, n_u, n_v, poses, dirs, n_lanes, n_beams, range2, stop_unknown, max_steps, kind, hit, range_mc);
  GS_CHECK_LAUNCH("scan_cast");
  return GS_OK;
}

extern "C" int gs_scan_field(const unsigned char* cells, int n_u, int n_v, int R, unsigned char* cost, gs_stream_t stream) {
  GS_REQUIRE(n_u >= 1 && n_u <= SCAN_MAX && n_v >= 1 && n_v <= SCAN_MAX, "scan_field: map %d x %d outside [1, 1024]", n_u, n_v);
  GS_REQUIRE(R >= 1 && R <= SCAN_R_MAX, "scan_field: R=%d outside [1, %d]", R, SCAN_R_MAX);
  GS_REQUIRE(cells && cost, "scan_field: null pointer");
  GS_TIMING_PRE();
  scan_field_kernel<<<dim3(gs_cdiv(n_v, FIELD_TV), gs_cdiv(n_u, FIELD_TU)), SCAN_THREADS, 0, (hipStream_t)stream>>>(
      cells, n_u, n_v, R, cost);
  GS_CHECK_LAUNCH("scan_field");
  return GS_OK;
}

extern "C" int gs_scan_match(const unsigned char* cost, const unsigned char* cells, int n_u, int n_v, const int* offsets,
                             int n_yaws, int n_beams, int u0, int v0, int w_u, int w_v, int cap, int allow_unknown,
                             unsigned int* score, unsigned long long* best, gs_stream_t stream) {
  GS_REQUIRE(n_u >= 1 && n_u <= SCAN_MAX && n_v >= 1 && n_v <= SCAN_MAX, "scan_match: map %d x %d outside [1, 1024]", n_u, n_v);
  GS_REQUIRE(n_yaws >= 1 && n_yaws <= SCAN_MAX_YAWS && n_beams >= 1 && n_beams <= SCAN_MAX_BEAMS,
             "scan_match: %d yaws (1 .. %d), %d beams (1 .. %d)", n_yaws, SCAN_MAX_YAWS, n_beams, SCAN_MAX_BEAMS);
  GS_REQUIRE(u0 >= 0 && v0 >= 0 && w_u >= 1 && w_v >= 1 && u0 <= n_u - w_u && v0 <= n_v - w_v,
             "scan_match: window [%d, %d) x [%d, %d) outside the map %d x %d or empty", u0, u0 + w_u, v0, v0 + w_v, n_u, n_v);
  GS_REQUIRE((long long)n_yaws * w_u * w_v <= SCAN_MAX_LANES, "scan_match: %d x %d x %d candidates, at most 2^28", n_yaws,
             w_u, w_v);
  GS_REQUIRE(cap >= 1 && cap <= SCAN_R_MAX * SCAN_R_MAX + 1, "scan_match: cap=%d outside [1, %d]", cap,
             SCAN_R_MAX * SCAN_R_MAX + 1);
  GS_REQUIRE(allow_unknown == 0 || allow_unknown == 1, "scan_match: allow_unknown=%d is not 0 or 1", allow_unknown);
  GS_REQUIRE(cost && cells && offsets && score && best, "scan_match: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(best, 0xff, sizeof(unsigned long long), s) != hipSuccess) {
    gs_set_error("scan_match: cannot reset best");
    return GS_ERR_LAUNCH;
  }
  const int chunks = gs_cdiv(w_v, MATCH_CHUNK);
  GS_TIMING_PRE();
  scan_match_kernel<<<dim3(gs_cdiv(w_u * chunks, SCAN_THREADS / GS_WAVE), n_yaws), SCAN_THREADS, 0, s>>>(
      cost, cells, n_u, n_v, offsets, n_beams, u0, v0, w_u, w_v, chunks, cap, allow_unknown, score, best);
  GS_CHECK_LAUNCH("scan_match");
  return GS_OK;
}
