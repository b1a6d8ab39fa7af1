// Cost-to-go field over a passability lattice and the path walked down it (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_geodesic_*); tests/geodesic_restatement.py restates it serially.  Integer only.
//
// gs_geodesic_relax enqueues k launches of geodesic_relax_kernel, the brick sweep of brick_relax.h with GeoRule: beside
//   the costs a brick loads the passability of its tile, derives each cell's 26 allowed-move bits from it, and lowers
//   a cell to the smallest cost + weight over its allowed moves that stays within max_cost.
// Every stored cost is the length of a real path: a seed holds 0, and a cell is only ever given a neighbour's stored
// cost plus the weight of an allowed move to it, old or new, both of which are lengths of paths from a seed.  Costs only
// fall, so the fixed point, which is unique, is reached whatever the order (brick_relax.h).
// geodesic_path_kernel is one wave: lanes 0..25 evaluate the moves, a butterfly takes the minimum of (cost + w, move),
// the steps run serially.  No atomics, no scratch.
#include "brick_relax.h"
#include "geo_moves.h"

namespace {

#ifndef GEO_B0           // the brick; tools/geodesic_bench.py measures other shapes through a library built with these set
#define GEO_B0 4
#define GEO_B1 4
#define GEO_B2 32
#endif
#ifndef GEO_ROUNDS_MAX   // rounds inside LDS per sweep
#define GEO_ROUNDS_MAX 64
#endif
using GeoBrick = Brick<GEO_B0, GEO_B1, GEO_B2, GEO_ROUNDS_MAX>;
constexpr int B0 = GeoBrick::B0, B1 = GeoBrick::B1, B2 = GeoBrick::B2;
constexpr int GEO_THREADS = GeoBrick::THREADS;
constexpr int GEO_INF = GS_GEO_INF;

static_assert(geo_nb(12) == GeoBrick::nb(12) && geo_nb(13) == GeoBrick::nb(13), "geo_moves.h numbers the moves as the brick");

__global__ __launch_bounds__(GEO_THREADS) void geodesic_fill_kernel(int* __restrict__ cost, long long ncells,
                                                                    unsigned char* __restrict__ flags,
                                                                    long long nflags) {
  const long long p = (long long)blockIdx.x * GEO_THREADS + threadIdx.x;
  if (p < ncells) cost[p] = GEO_INF;
  if (p < nflags) flags[p] = 0;
}

__global__ __launch_bounds__(GEO_THREADS) void geodesic_seed_kernel(const unsigned char* __restrict__ passable, int n0,
                                                                    int n1, int n2, const int* __restrict__ seeds, int m,
                                                                    int* __restrict__ cost,
                                                                    unsigned char* __restrict__ flags) {
  const int p = blockIdx.x * GEO_THREADS + threadIdx.x;
  if (p >= m) return;
  const int s0 = seeds[(size_t)p * 3 + 0], s1 = seeds[(size_t)p * 3 + 1], s2 = seeds[(size_t)p * 3 + 2];
  if (s0 < 0 || s0 >= n0 || s1 < 0 || s1 >= n1 || s2 < 0 || s2 >= n2) return;
  const size_t at = ((size_t)s0 * n1 + s1) * n2 + s2;
  if (passable[at] == 0) return;
  cost[at] = 0;                                             // duplicates store the same values
  const int nb1 = (n1 + B1 - 1) / B1, nb2 = (n2 + B2 - 1) / B2;
  flags[((size_t)(s0 / B0) * nb1 + s1 / B1) * nb2 + s2 / B2] = 1;
}

struct GeoRule {
  using Value = int;
  struct Cell { unsigned moves; };                          // bit m: move m is allowed
  const unsigned char* passable;
  int* cost;
  int max_cost;
  unsigned char* pass;                                      // LDS [TILE]: 1 where the tile's cell is inside and passable
  __device__ __forceinline__ int load(size_t at, bool inside, int q) const {
    const int c = cost[at];
    const unsigned char p = passable[at];
    pass[q] = inside && p != 0 ? 1 : 0;
    return inside ? c : GEO_INF;
  }
  __device__ __forceinline__ int prepare(const int* tile, int at, int v, Cell& cell) const {
    unsigned around = 0;
#pragma unroll
    for (int e = 0; e < 27; ++e)
      around |= (unsigned)pass[at + GeoBrick::tile_offset(e / 9 - 1, e / 3 % 3 - 1, e % 3 - 1)] << e;
    unsigned ok = 0;
#pragma unroll
    for (int m = 0; m < 26; ++m) ok |= (around & geo_box(m)) == geo_box(m) ? 1u << m : 0u;
    cell.moves = ok;
    return v;
  }
  // not blocked, outside the lattice or walled in
  __device__ __forceinline__ bool active(int, const Cell& cell) const { return cell.moves != 0; }
  __device__ __forceinline__ int lower(const int* tile, int at, int v, const Cell& cell) const {
    int best = v;
#pragma unroll
    for (int m = 0; m < 26; ++m) {
      const int cand = tile[at + GeoBrick::nb_offset(m)] + geo_weight(m);
      if ((cell.moves >> m & 1u) != 0 && cand <= max_cost && cand < best) best = cand;
    }
    return best;
  }
  __device__ __forceinline__ void store(size_t at, int v) const { cost[at] = v; }
};

__global__ __launch_bounds__(GEO_THREADS) void geodesic_relax_kernel(
    const unsigned char* __restrict__ passable, int* cost, int n0, int n1, int n2, int nb0, int nb1, int nb2,
    int max_cost, unsigned char* cur, unsigned char* next, unsigned int* changed) {
  __shared__ unsigned char pass[GeoBrick::TILE];
  brick_relax<GeoBrick>(GeoRule{passable, cost, max_cost, pass}, n0, n1, n2, nb0, nb1, nb2, cur, next, changed);
}

__global__ __launch_bounds__(64) void geodesic_path_kernel(const int* __restrict__ cost,
                                                           const unsigned char* __restrict__ passable, int n0, int n1,
                                                           int n2, int s0, int s1, int s2, int max_len,
                                                           int* __restrict__ out_cells, int* __restrict__ out_n) {
  const int lane = threadIdx.x;
  if (s0 < 0 || s0 >= n0 || s1 < 0 || s1 >= n1 || s2 < 0 || s2 >= n2) {
    if (lane == 0) out_n[0] = 0;
    return;
  }
  const int nb = geo_nb(lane < 26 ? lane : 0);
  const int d0 = nb / 9 - 1, d1 = nb / 3 % 3 - 1, d2 = nb % 3 - 1;
  const int nz = (d0 != 0) + (d1 != 0) + (d2 != 0);
  const int w = nz == 1 ? 1000 : (nz == 2 ? 1414 : 1732);
  int c0 = s0, c1 = s1, c2 = s2;
  int c = cost[((size_t)c0 * n1 + c1) * n2 + c2];
  if (c >= GEO_INF) {
    if (lane == 0) out_n[0] = 0;
    return;
  }
  const unsigned long long none = ~0ull;
  for (int n = 0; n < max_len; ++n) {
    if (lane == 0) {
      out_cells[(size_t)n * 3 + 0] = c0;
      out_cells[(size_t)n * 3 + 1] = c1;
      out_cells[(size_t)n * 3 + 2] = c2;
    }
    if (c == 0) {
      if (lane == 0) out_n[0] = n + 1;
      return;
    }
    unsigned long long key = none;
    const int t0 = c0 + d0, t1 = c1 + d1, t2 = c2 + d2;
    if (lane < 26 && t0 >= 0 && t0 < n0 && t1 >= 0 && t1 < n1 && t2 >= 0 && t2 < n2) {
      bool ok = true;                                       // the box of c and t: inside the lattice since both ends are
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
          for (int e = 0; e < 2; ++e)
            ok = ok && passable[((size_t)(c0 + a * d0) * n1 + (c1 + b * d1)) * n2 + (c2 + e * d2)] != 0;
      const int v = cost[((size_t)t0 * n1 + t1) * n2 + t2];
      if (ok && v < GEO_INF) key = (unsigned long long)(unsigned)(v + w) << 5 | (unsigned)lane;
    }
    key = gs_wave_min_u64(key);
    if (key == none) break;
    const int m = geo_nb((int)(key & 31u));
    c0 += m / 9 - 1;
    c1 += m / 3 % 3 - 1;
    c2 += m % 3 - 1;
    c = cost[((size_t)c0 * n1 + c1) * n2 + c2];
  }
  if (lane == 0) out_n[0] = -1;
}

}  // namespace

extern "C" int gs_geodesic_brick(int* b0, int* b1, int* b2) {
  GS_REQUIRE(b0 && b1 && b2, "geodesic_brick: null pointer");
  *b0 = B0;
  *b1 = B1;
  *b2 = B2;
  return GS_OK;
}

extern "C" size_t gs_geodesic_flags_bytes(int n0, int n1, int n2) {
  return brick_flags_bytes<GeoBrick>(n0, n1, n2);
}

extern "C" int gs_geodesic_init(const unsigned char* passable, int n0, int n1, int n2, const int* seeds, int m, int* cost,
                                unsigned char* flags, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "geodesic_init: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(m >= 0, "geodesic_init: m=%d", m);
  GS_REQUIRE(passable && cost && flags && (seeds || m == 0), "geodesic_init: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  const long long ncells = (long long)n0 * n1 * n2, nflags = (long long)gs_geodesic_flags_bytes(n0, n1, n2);
  const long long most = ncells > nflags ? ncells : nflags;
  GS_TIMING_PRE();
  geodesic_fill_kernel<<<(unsigned)((most + GEO_THREADS - 1) / GEO_THREADS), GEO_THREADS, 0, s>>>(cost, ncells, flags,
                                                                                                   nflags);
  GS_CHECK_LAUNCH("geodesic_fill");
  if (m > 0) {
    geodesic_seed_kernel<<<gs_cdiv(m, GEO_THREADS), GEO_THREADS, 0, s>>>(passable, n0, n1, n2, seeds, m, cost, flags);
    GS_CHECK_LAUNCH("geodesic_seed");
  }
  return GS_OK;
}

extern "C" int gs_geodesic_relax(const unsigned char* passable, int n0, int n1, int n2, int max_cost, int* cost,
                                 unsigned char* flags, int sweep0, int k, unsigned int* changed, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "geodesic_relax: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(max_cost >= 0 && max_cost <= GS_GEO_MAX_COST, "geodesic_relax: max_cost %d outside [0, %d]", max_cost,
             GS_GEO_MAX_COST);
  GS_REQUIRE(k >= 1 && sweep0 >= 0 && sweep0 <= 0x7fffffff - k, "geodesic_relax: sweep0=%d k=%d", sweep0, k);
  GS_REQUIRE(passable && cost && flags && changed, "geodesic_relax: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  const int nb0 = gs_cdiv(n0, B0), nb1 = gs_cdiv(n1, B1), nb2 = gs_cdiv(n2, B2);
  const size_t nbricks = (size_t)nb0 * nb1 * nb2;           // at most 128 * 128 * 64 = 2^20 workgroups
  return brick_relax_enqueue("geodesic_relax", nbricks, flags, sweep0, k, changed, s,
                             [&](unsigned char* cur, unsigned char* next, unsigned int* ch) {
                               geodesic_relax_kernel<<<(unsigned)nbricks, GEO_THREADS, 0, s>>>(
                                   passable, cost, n0, n1, n2, nb0, nb1, nb2, max_cost, cur, next, ch);
                             });
}

extern "C" int gs_geodesic_path(const int* cost, const unsigned char* passable, int n0, int n1, int n2, int start0,
                                int start1, int start2, int max_len, int* out_cells, int* out_n, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "geodesic_path: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(max_len >= 1, "geodesic_path: max_len=%d", max_len);
  GS_REQUIRE(cost && passable && out_cells && out_n, "geodesic_path: null pointer");
  GS_TIMING_PRE();
  geodesic_path_kernel<<<1, 64, 0, (hipStream_t)stream>>>(cost, passable, n0, n1, n2, start0, start1, start2, max_len,
                                                          out_cells, out_n);
  GS_CHECK_LAUNCH("geodesic_path");
  return GS_OK;
}
