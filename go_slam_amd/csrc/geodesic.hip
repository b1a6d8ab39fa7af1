// Cost-to-go field over a passability lattice and the path walked down it (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_geodesic_*); tests/geodesic_restatement.py restates it serially.  Integer only.
//
// gs_geodesic_relax enqueues k launches of geodesic_relax_kernel, one workgroup per brick of B0 x B1 x B2 cells:
//   a brick whose dirty flag is clear leaves after one byte load.  A dirty one loads cost and passability of the brick
//   and a one-cell halo into LDS, derives each cell's 26 allowed-move bits from the tile, and relaxes its cells inside
//   LDS (every cell owned by one lane, GEO_PER cells per lane, one barrier per round) until a round lowers nothing or
//   GEO_ROUNDS rounds have run.  Only lowered cells are written back.  A brick that lowered a cell on a face, edge or
//   corner marks the bricks behind it in the next sweep's flag buffer, marks itself when it ran out of rounds, and
//   stores 1 to changed[s].  Every such store writes the same value, so none is atomic.  A dirty brick clears its own
//   byte of the buffer it read, which makes that buffer the clean "next" buffer of the following sweep.
// Cost is relaxed in place and nothing waits for another workgroup: a halo value read while its owner lowers it is
// stale, which only postpones that improvement to the next sweep -- the owner marks this brick, and the kernel boundary
// makes the value visible.  Values only fall and every stored value is the length of a real path, so the fixed point,
// which is unique, is reached whatever the order.
// geodesic_path_kernel is one wave: lanes 0..25 evaluate the moves, a butterfly takes the minimum of (cost + w, move),
// the steps run serially.  No atomics, no scratch.
#include "common.h"

namespace {

#ifndef GEO_B0           // the brick; tools/geodesic_bench.py measures other shapes through a library built with these set
#define GEO_B0 4
#define GEO_B1 4
#define GEO_B2 32
#endif
#ifndef GEO_ROUNDS_MAX   // rounds inside LDS per sweep
#define GEO_ROUNDS_MAX 64
#endif
constexpr int B0 = GEO_B0, B1 = GEO_B1, B2 = GEO_B2;
constexpr int GEO_THREADS = 256;
constexpr int GEO_CELLS = B0 * B1 * B2;
constexpr int GEO_PER = GEO_CELLS / GEO_THREADS;           // cells per lane
constexpr int T0 = B0 + 2, T1 = B1 + 2, T2 = B2 + 2;       // the tile: the brick and its halo
constexpr int GEO_TILE = T0 * T1 * T2;
constexpr int GEO_ROUNDS = GEO_ROUNDS_MAX;
constexpr int GEO_MAX = 1024;                              // cells per axis
constexpr int GEO_INF = GS_GEO_INF;
static_assert(GEO_CELLS % GEO_THREADS == 0, "a lane owns a whole number of cells");

// move m of 26 -> index 0..26 of the 3 x 3 x 3 neighbourhood (the centre, 13, is skipped), its components and weight
__host__ __device__ constexpr int geo_nb(int m) { return m < 13 ? m : m + 1; }
__host__ __device__ constexpr int geo_d0(int m) { return geo_nb(m) / 9 - 1; }
__host__ __device__ constexpr int geo_d1(int m) { return geo_nb(m) / 3 % 3 - 1; }
__host__ __device__ constexpr int geo_d2(int m) { return geo_nb(m) % 3 - 1; }
__host__ __device__ constexpr int geo_weight(int m) {
  const int nz = (geo_d0(m) != 0) + (geo_d1(m) != 0) + (geo_d2(m) != 0);
  return nz == 1 ? 1000 : (nz == 2 ? 1414 : 1732);
}
// the cells of the box spanned by the centre and move m, as bits of the 3 x 3 x 3 neighbourhood
__host__ __device__ constexpr unsigned geo_box(int m) {
  unsigned bits = 0;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < 2; ++c)
        bits |= 1u << ((a * geo_d0(m) + 1) * 9 + (b * geo_d1(m) + 1) * 3 + (c * geo_d2(m) + 1));
  return bits;
}
__host__ __device__ constexpr int geo_tile_offset(int e0, int e1, int e2) { return (e0 * T1 + e1) * T2 + e2; }

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

__global__ __launch_bounds__(GEO_THREADS) void geodesic_relax_kernel(
    const unsigned char* __restrict__ passable, int* cost, int n0, int n1, int n2, int nb0, int nb1, int nb2,
    int max_cost, unsigned char* cur, unsigned char* next, unsigned int* changed) {
  __shared__ int tile[GEO_TILE];
  __shared__ unsigned char pass[GEO_TILE];
  __shared__ int lowered[3];                                // round r stores to [r % 3]
  __shared__ int face[6];                                   // a cell with index 0 / B - 1 along axis a fell: [2a] / [2a + 1]
  const int tid = threadIdx.x;
  const int brick = blockIdx.x;
  if (cur[brick] == 0) return;                              // written before this launch: every lane reads the same
  const int i2 = brick % nb2, i1 = brick / nb2 % nb1, i0 = brick / nb2 / nb1;
  const int base0 = i0 * B0 - 1, base1 = i1 * B1 - 1, base2 = i2 * B2 - 1;     // the tile's corner, a halo cell

  if (tid < 3) lowered[tid] = 0;
  if (tid < 6) face[tid] = 0;
  for (int q = tid; q < GEO_TILE; q += GEO_THREADS) {
    const int t0 = q / (T1 * T2), r = q - t0 * (T1 * T2), t1 = r / T2, t2 = r - t1 * T2;
    const int g0 = base0 + t0, g1 = base1 + t1, g2 = base2 + t2;
    const bool inside = g0 >= 0 && g0 < n0 && g1 >= 0 && g1 < n1 && g2 >= 0 && g2 < n2;
    const size_t at = inside ? ((size_t)g0 * n1 + g1) * n2 + g2 : 0;
    const int c = cost[at];
    const unsigned char p = passable[at];
    tile[q] = inside ? c : GEO_INF;
    pass[q] = inside && p != 0 ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0) cur[brick] = 0;                             // after the barrier: every wave has read the flag

  int at[GEO_PER], val[GEO_PER], was[GEO_PER];
  unsigned moves[GEO_PER];
#pragma unroll
  for (int j = 0; j < GEO_PER; ++j) {
    const int q = tid + GEO_THREADS * j;
    const int z = q % B2, y = q / B2 % B1, x = q / (B1 * B2);
    at[j] = geo_tile_offset(x + 1, y + 1, z + 1);
    unsigned around = 0;
#pragma unroll
    for (int e = 0; e < 27; ++e)
      around |= (unsigned)pass[at[j] + geo_tile_offset(e / 9 - 1, e / 3 % 3 - 1, e % 3 - 1)] << e;
    unsigned ok = 0;
#pragma unroll
    for (int m = 0; m < 26; ++m) ok |= (around & geo_box(m)) == geo_box(m) ? 1u << m : 0u;
    moves[j] = ok;
    val[j] = was[j] = tile[at[j]];
  }

  int round = 0;
  bool more;
  do {
    bool fell = false;
#pragma unroll
    for (int j = 0; j < GEO_PER; ++j) {
      if (moves[j] == 0) continue;
      int best = val[j];
#pragma unroll
      for (int m = 0; m < 26; ++m) {
        const int cand = tile[at[j] + geo_tile_offset(geo_d0(m), geo_d1(m), geo_d2(m))] + geo_weight(m);
        if ((moves[j] >> m & 1u) != 0 && cand <= max_cost && cand < best) best = cand;
      }
      if (best < val[j]) {
        val[j] = best;
        tile[at[j]] = best;                                 // a neighbour reads the old or the new value: both are path lengths
        fell = true;
      }
    }
    if (fell) lowered[round % 3] = 1;
    __syncthreads();
    more = lowered[round % 3] != 0;
    if (tid == 0) lowered[(round + 2) % 3] = 0;             // last read before this barrier, next written after the next
    ++round;
  } while (more && round < GEO_ROUNDS);

  bool any = false;
#pragma unroll
  for (int j = 0; j < GEO_PER; ++j) {
    if (val[j] >= was[j]) continue;
    const int q = tid + GEO_THREADS * j;
    const int z = q % B2, y = q / B2 % B1, x = q / (B1 * B2);
    cost[((size_t)(base0 + 1 + x) * n1 + (base1 + 1 + y)) * n2 + (base2 + 1 + z)] = val[j];      // inside: it has moves
    any = true;
    if (x == 0) face[0] = 1;
    if (x == B0 - 1) face[1] = 1;
    if (y == 0) face[2] = 1;
    if (y == B1 - 1) face[3] = 1;
    if (z == 0) face[4] = 1;
    if (z == B2 - 1) face[5] = 1;
  }
  if (any) lowered[round % 3] = 1;                          // zero since the barrier before last, not read since
  __syncthreads();
  if (lowered[round % 3] == 0) return;
  if (tid == 0) changed[0] = 1;
  if (tid < 27) {
    const int d0 = tid / 9 - 1, d1 = tid / 3 % 3 - 1, d2 = tid % 3 - 1;
    const int j0 = i0 + d0, j1 = i1 + d1, j2 = i2 + d2;
    // a lowered cell that the brick at +d reads lies on every face d names, so all of them are set (the converse need
    // not hold: a brick marked in vain loads its tile, lowers nothing and marks nobody)
    bool mark = (d0 == 0 || face[d0 < 0 ? 0 : 1] != 0) && (d1 == 0 || face[d1 < 0 ? 2 : 3] != 0) &&
                (d2 == 0 || face[d2 < 0 ? 4 : 5] != 0);
    if (tid == 13) mark = more;                             // itself: only when the rounds ran out
    if (mark && j0 >= 0 && j0 < nb0 && j1 >= 0 && j1 < nb1 && j2 >= 0 && j2 < nb2)
      next[((size_t)j0 * nb1 + j1) * nb2 + j2] = 1;
  }
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
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long other = __shfl_xor(key, off, 64);
      key = other < key ? other : key;
    }
    if (key == none) break;
    const int m = geo_nb((int)(key & 31u));
    c0 += m / 9 - 1;
    c1 += m / 3 % 3 - 1;
    c2 += m % 3 - 1;
    c = cost[((size_t)c0 * n1 + c1) * n2 + c2];
  }
  if (lane == 0) out_n[0] = -1;
}

bool geo_dims_ok(int n0, int n1, int n2) {
  return n0 >= 1 && n0 <= GEO_MAX && n1 >= 1 && n1 <= GEO_MAX && n2 >= 1 && n2 <= GEO_MAX;
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
  if (!geo_dims_ok(n0, n1, n2)) return 0;
  return (size_t)2 * gs_cdiv(n0, B0) * gs_cdiv(n1, B1) * gs_cdiv(n2, B2);
}

extern "C" int gs_geodesic_init(const unsigned char* passable, int n0, int n1, int n2, const int* seeds, int m, int* cost,
                                unsigned char* flags, gs_stream_t stream) {
  GS_REQUIRE(geo_dims_ok(n0, n1, n2), "geodesic_init: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
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
  GS_REQUIRE(geo_dims_ok(n0, n1, n2), "geodesic_relax: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(max_cost >= 0 && max_cost <= GS_GEO_MAX_COST, "geodesic_relax: max_cost %d outside [0, %d]", max_cost,
             GS_GEO_MAX_COST);
  GS_REQUIRE(k >= 1 && sweep0 >= 0 && sweep0 <= 0x7fffffff - k, "geodesic_relax: sweep0=%d k=%d", sweep0, k);
  GS_REQUIRE(passable && cost && flags && changed, "geodesic_relax: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  const int nb0 = gs_cdiv(n0, B0), nb1 = gs_cdiv(n1, B1), nb2 = gs_cdiv(n2, B2);
  const size_t nbricks = (size_t)nb0 * nb1 * nb2;           // at most 128 * 128 * 64 = 2^20 workgroups
  if (hipMemsetAsync(changed, 0, sizeof(unsigned int) * (size_t)k, s) != hipSuccess) {
    gs_set_error("geodesic_relax: clearing changed[%d] failed", k);
    return GS_ERR_LAUNCH;
  }
  GS_TIMING_PRE();
  for (int i = 0; i < k; ++i) {
    const int parity = (sweep0 + i) & 1;
    geodesic_relax_kernel<<<(unsigned)nbricks, GEO_THREADS, 0, s>>>(passable, cost, n0, n1, n2, nb0, nb1, nb2, max_cost,
                                                                    flags + parity * nbricks,
                                                                    flags + (parity ^ 1) * nbricks, changed + i);
    GS_CHECK_LAUNCH("geodesic_relax");
  }
  return GS_OK;
}

extern "C" int gs_geodesic_path(const int* cost, const unsigned char* passable, int n0, int n1, int n2, int start0,
                                int start1, int start2, int max_len, int* out_cells, int* out_n, gs_stream_t stream) {
  GS_REQUIRE(geo_dims_ok(n0, n1, n2), "geodesic_path: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(max_len >= 1, "geodesic_path: max_len=%d", max_len);
  GS_REQUIRE(cost && passable && out_cells && out_n, "geodesic_path: null pointer");
  GS_TIMING_PRE();
  geodesic_path_kernel<<<1, 64, 0, (hipStream_t)stream>>>(cost, passable, n0, n1, n2, start0, start1, start2, max_len,
                                                          out_cells, out_n);
  GS_CHECK_LAUNCH("geodesic_path");
  return GS_OK;
}
