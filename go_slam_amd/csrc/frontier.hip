// Frontiers of a state lattice: free cells that border never-observed space, their 26-connected clusters and one table
// row per cluster (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_frontier_*); tests/frontier_restatement.py restates it serially.  Integer only.
//
// frontier_mark_kernel: one lane per cell, FR_PER cells per lane, runs along the last axis coalesced.  Writes frontier,
//   label (own index on the frontier, -1 off it) and the four counts (ballots per wave, LDS per workgroup, at most four
//   integer atomics per workgroup), and sets the dirty byte, in flag buffer 0, of every brick that holds a frontier cell.
// gs_frontier_relax enqueues k launches of frontier_relax_kernel, the brick sweep of brick_relax.h with FrRule: a tile
//   entry is the label as unsigned (-1, the largest value, where there is no frontier cell or no lattice), a cell first
//   takes label[label[c]] where that is lower (FRONTIER_SHORTCUT), and is lowered to the smallest of its 26 neighbours.
// Every stored label is the index of a cell of the same component: a cell starts with its own index and is only ever
// given a label that a neighbour, or the cell its label names, holds or held -- a stale one included.  Labels only
// fall, so the fixed point -- every cell holds its component's smallest index -- is reached whatever the order
// (brick_relax.h).
// Table: the roots (label == own index) are compacted in ascending order by count / scan / emit launches over blocks of
// FR_THREADS * FR_PER cells; emit also clears the row.  frontier_table_kernel passes over the cells once: a frontier
// cell finds its row by binary search of its label among the roots, the lanes of a wave that share a row reduce their
// contributions by butterflies, and one lane per (wave, row) issues the integer atomics.  No scratch, no floating point.
#include "frontier_rows.h"

namespace {

#ifndef FRONTIER_SHORTCUT     // 0: neighbour relaxation alone (tools/frontier_bench.py counts the sweeps of both)
#define FRONTIER_SHORTCUT 1
#endif
constexpr int FR_SCAN_THREADS = 1024;
constexpr unsigned FR_NONE = 0xffffffffu;                  // label -1

// the number of face neighbours of cell p = (c0, c1, c2) that lie inside the lattice and are unknown
__device__ __forceinline__ int fr_unknown_faces(const unsigned char* __restrict__ state, int p, int c0, int c1, int c2,
                                                int n0, int n1, int n2) {
  int f = 0;
  if (c2 > 0) f += state[p - 1] == 0;
  if (c2 + 1 < n2) f += state[p + 1] == 0;
  if (c1 > 0) f += state[p - n2] == 0;
  if (c1 + 1 < n1) f += state[p + n2] == 0;
  if (c0 > 0) f += state[p - n1 * n2] == 0;
  if (c0 + 1 < n0) f += state[p + n1 * n2] == 0;
  return f;
}

__global__ __launch_bounds__(FR_THREADS) void frontier_mark_kernel(const unsigned char* __restrict__ state,
                                                                   const unsigned char* __restrict__ open, int n0,
                                                                   int n1, int n2, int nb1, int nb2,
                                                                   unsigned char* __restrict__ frontier,
                                                                   int* __restrict__ label, unsigned int* counts,
                                                                   unsigned char* flags) {
  __shared__ unsigned part[FR_WAVES][4];
  const int tid = threadIdx.x, lane = tid % GS_WAVE, wave = tid / GS_WAVE;
  const int ncells = n0 * n1 * n2;                          // at most 2^30
  const int base = blockIdx.x * FR_BLOCK;
  unsigned n[4] = {0u, 0u, 0u, 0u};                         // wave totals: unknown, free, solid, frontier
#pragma unroll
  for (int i = 0; i < FR_PER; ++i) {
    const int p = base + i * FR_THREADS + tid;
    const bool in = p < ncells;
    const int s = in ? state[p] : 0;
    bool fr = false;
    if (in && s == 1 && (open == nullptr || open[p] != 0)) {
      const int c2 = p % n2, c1 = p / n2 % n1, c0 = p / n2 / n1;
      fr = fr_unknown_faces(state, p, c0, c1, c2, n0, n1, n2) != 0;
      if (fr) flags[((size_t)(c0 / B0) * nb1 + c1 / B1) * nb2 + c2 / B2] = 1;      // buffer 0; every store writes 1
    }
    if (in) {
      frontier[p] = fr ? 1 : 0;
      label[p] = fr ? p : -1;
    }
    n[0] += fr_popc(__ballot(in && s == 0));
    n[1] += fr_popc(__ballot(in && s == 1));
    n[2] += fr_popc(__ballot(in && s > 1));
    n[3] += fr_popc(__ballot(fr));
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) part[wave][c] = n[c];
  }
  __syncthreads();
  if (tid < 4) {
    unsigned total = 0;
#pragma unroll
    for (int w = 0; w < FR_WAVES; ++w) total += part[w][tid];
    if (total != 0) atomicAdd(&counts[tid], total);
  }
}

struct FrRule {
  using Value = unsigned;
  struct Cell {};
  int* label;
  unsigned ncells;
  __device__ __forceinline__ unsigned load(size_t at, bool inside, int) const {
    const unsigned v = (unsigned)label[at];
    return inside ? v : FR_NONE;
  }
  __device__ __forceinline__ unsigned prepare(unsigned* tile, int at, unsigned v, Cell&) const {
#if FRONTIER_SHORTCUT
    if (v < ncells) {
      // the label of the cell this one points at: possibly stale, always an index of this component at most v
      const unsigned far = (unsigned)label[v];
      if (far < v) {
        tile[at] = far;                                     // a neighbour reads the old or the new value: both are valid
        return far;
      }
    }
#endif
    return v;                                               // FR_NONE off the frontier and outside the lattice
  }
  __device__ __forceinline__ bool active(unsigned v, const Cell&) const { return v != FR_NONE; }
  __device__ __forceinline__ unsigned lower(const unsigned* tile, int at, unsigned v, const Cell&) const {
    unsigned best = v;
#pragma unroll
    for (int m = 0; m < 26; ++m) {
      const unsigned cand = tile[at + FrBrick::nb_offset(m)];
      best = cand < best ? cand : best;                     // FR_NONE never wins
    }
    return best;
  }
  __device__ __forceinline__ void store(size_t at, unsigned v) const { label[at] = (int)v; }
};

__global__ __launch_bounds__(FR_THREADS) void frontier_relax_kernel(int* label, int n0, int n1, int n2, int nb0, int nb1,
                                                                    int nb2, unsigned char* cur, unsigned char* next,
                                                                    unsigned int* changed) {
  brick_relax<FrBrick>(FrRule{label, (unsigned)(n0 * n1 * n2)}, n0, n1, n2, nb0, nb1, nb2, cur, next, changed);
}

__global__ __launch_bounds__(FR_THREADS) void frontier_count_kernel(const int* __restrict__ label, int ncells,
                                                                    unsigned* __restrict__ count) {
  __shared__ unsigned wcount[FR_PER * FR_WAVES];
  bool is[FR_PER];
  unsigned rank[FR_PER];
  const unsigned total = fr_rank_roots(label, ncells, blockIdx.x * FR_BLOCK, wcount, is, rank);
  if (threadIdx.x == 0) count[blockIdx.x] = total;
}

// one workgroup: first[b] = the number of roots in the blocks before b, n_roots[0] = their total
__global__ __launch_bounds__(FR_SCAN_THREADS) void frontier_scan_kernel(const unsigned* __restrict__ count, int nblk,
                                                                        int iters, unsigned* __restrict__ first,
                                                                        int* __restrict__ n_roots) {
  constexpr int W = FR_SCAN_THREADS / GS_WAVE;
  __shared__ unsigned wsum[W];
  const int tid = threadIdx.x, lane = tid % GS_WAVE, wave = tid / GS_WAVE;
  unsigned carry = 0;
  for (int it = 0; it < iters; ++it) {
    const int e = it * FR_SCAN_THREADS + tid;
    const unsigned v = e < nblk ? count[e] : 0u;
    unsigned incl = v;
#pragma unroll
    for (int off = 1; off < GS_WAVE; off <<= 1) {
      const unsigned up = __shfl_up(incl, off, GS_WAVE);
      if (lane >= off) incl += up;
    }
    if (lane == GS_WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const unsigned s = wsum[w];
      if (w < wave) before += s;
      total += s;
    }
    if (e < nblk) first[e] = carry + before + incl - v;
    carry += total;
    __syncthreads();                                        // wsum is rewritten by the next iteration
  }
  if (tid == 0) n_roots[0] = (int)carry;
}

__global__ __launch_bounds__(FR_THREADS) void frontier_emit_kernel(const int* __restrict__ label, int ncells,
                                                                   const unsigned* __restrict__ first, int rows,
                                                                   int* __restrict__ root, int* __restrict__ size,
                                                                   int* __restrict__ faces,
                                                                   unsigned long long* __restrict__ sum,
                                                                   int* __restrict__ bbox,
                                                                   unsigned long long* __restrict__ best) {
  __shared__ unsigned wcount[FR_PER * FR_WAVES];
  bool is[FR_PER];
  unsigned rank[FR_PER];
  const int base = blockIdx.x * FR_BLOCK;
  fr_rank_roots(label, ncells, base, wcount, is, rank);
  const unsigned start = first[blockIdx.x];
#pragma unroll
  for (int i = 0; i < FR_PER; ++i) {
    const unsigned slot = start + rank[i];
    if (!is[i] || slot >= (unsigned)rows) continue;         // a caller that named fewer rows than there are roots
    root[slot] = base + i * FR_THREADS + (int)threadIdx.x;
    size[slot] = 0;
    faces[slot] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sum[(size_t)slot * 3 + a] = 0ull;
      bbox[(size_t)slot * 6 + a] = FR_MAX;
      bbox[(size_t)slot * 6 + 3 + a] = -1;
    }
    best[slot] = ~0ull;
  }
}

__global__ __launch_bounds__(FR_THREADS) void frontier_table_kernel(
    const unsigned char* __restrict__ state, const int* __restrict__ label, const int* __restrict__ cost, int n0, int n1,
    int n2, const int* __restrict__ root, int rows, int* size, int* faces, unsigned long long* sum, int* bbox,
    unsigned long long* best) {
  const int tid = threadIdx.x, lane = tid % GS_WAVE;
  const int ncells = n0 * n1 * n2;
  const int base = blockIdx.x * FR_BLOCK;
  for (int i = 0; i < FR_PER; ++i) {
    const int p = base + i * FR_THREADS + tid;
    const int l = p < ncells ? label[p] : -1;
    unsigned long long todo = __ballot(l >= 0);
    if (todo == 0) continue;                                // the wave's 64 cells hold no frontier cell: most do not
    int id = -1, c0 = 0, c1 = 0, c2 = 0, nf = 0;
    unsigned long long key = ~0ull;
    if (l >= 0) {
      int lo = 0, hi = rows;                                // the first row whose root is >= l
      for (int s = 0; s < 31 && lo < hi; ++s) {
        const int mid = lo + (hi - lo) / 2;
        if (root[mid] < l) lo = mid + 1; else hi = mid;
      }
      if (lo < rows && root[lo] == l) id = lo;              // else: a table that does not belong to these labels
      c2 = p % n2, c1 = p / n2 % n1, c0 = p / n2 / n1;
      nf = fr_unknown_faces(state, p, c0, c1, c2, n0, n1, n2);
      const unsigned c = cost != nullptr ? (unsigned)cost[p] : (unsigned)GS_GEO_INF;
      key = (unsigned long long)c << 32 | (unsigned)p;
    }
    todo = __ballot(id >= 0);
    for (int it = 0; it < GS_WAVE && todo != 0; ++it) {     // one turn per distinct row among the wave's cells
      const int leader = __ffsll((long long)todo) - 1;
      const int row = __shfl(id, leader, GS_WAVE);
      const bool mine = id == row;
      const unsigned long long members = __ballot(mine);
      todo &= ~members;
      const int f = gs_wave_sum_i32(mine ? nf : 0);
      const int s0 = gs_wave_sum_i32(mine ? c0 : 0), s1 = gs_wave_sum_i32(mine ? c1 : 0);
      const int s2 = gs_wave_sum_i32(mine ? c2 : 0);
      const int lo0 = gs_wave_min_i32(mine ? c0 : FR_MAX), lo1 = gs_wave_min_i32(mine ? c1 : FR_MAX);
      const int lo2 = gs_wave_min_i32(mine ? c2 : FR_MAX);
      const int hi0 = -gs_wave_min_i32(mine ? -c0 : 1), hi1 = -gs_wave_min_i32(mine ? -c1 : 1);
      const int hi2 = -gs_wave_min_i32(mine ? -c2 : 1);
      const unsigned long long k = gs_wave_min_u64(mine ? key : ~0ull);
      if (lane == leader) {
        atomicAdd(&size[row], fr_popc(members));
        atomicAdd(&faces[row], f);
        atomicAdd(&sum[(size_t)row * 3 + 0], (unsigned long long)s0);
        atomicAdd(&sum[(size_t)row * 3 + 1], (unsigned long long)s1);
        atomicAdd(&sum[(size_t)row * 3 + 2], (unsigned long long)s2);
        atomicMin(&bbox[(size_t)row * 6 + 0], lo0);
        atomicMin(&bbox[(size_t)row * 6 + 1], lo1);
        atomicMin(&bbox[(size_t)row * 6 + 2], lo2);
        atomicMax(&bbox[(size_t)row * 6 + 3], hi0);
        atomicMax(&bbox[(size_t)row * 6 + 4], hi1);
        atomicMax(&bbox[(size_t)row * 6 + 5], hi2);
        atomicMin(&best[row], k);
      }
    }
  }
}

}  // namespace

extern "C" int gs_frontier_brick(int* b0, int* b1, int* b2) {
  GS_REQUIRE(b0 && b1 && b2, "frontier_brick: null pointer");
  *b0 = B0;
  *b1 = B1;
  *b2 = B2;
  return GS_OK;
}

extern "C" size_t gs_frontier_flags_bytes(int n0, int n1, int n2) {
  return brick_flags_bytes<FrBrick>(n0, n1, n2);
}

extern "C" size_t gs_frontier_workspace_bytes(int n0, int n1, int n2) {
  if (!brick_dims_ok(n0, n1, n2)) return 0;
  return fr_workspace_bytes(fr_blocks(n0, n1, n2));
}

extern "C" int gs_frontier_mark(const unsigned char* state, const unsigned char* open, int n0, int n1, int n2,
                                unsigned char* frontier, int* label, unsigned int* counts, unsigned char* flags,
                                gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "frontier_mark: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(state && frontier && label && counts && flags, "frontier_mark: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(unsigned int) * 4, s) != hipSuccess ||
      hipMemsetAsync(flags, 0, gs_frontier_flags_bytes(n0, n1, n2), s) != hipSuccess) {
    gs_set_error("frontier_mark: clearing counts and flags failed");
    return GS_ERR_LAUNCH;
  }
  GS_TIMING_PRE();
  frontier_mark_kernel<<<fr_blocks(n0, n1, n2), FR_THREADS, 0, s>>>(state, open, n0, n1, n2, gs_cdiv(n1, B1),
                                                                    gs_cdiv(n2, B2), frontier, label, counts, flags);
  GS_CHECK_LAUNCH("frontier_mark");
  return GS_OK;
}

extern "C" int gs_frontier_relax(int n0, int n1, int n2, int* label, unsigned char* flags, int sweep0, int k,
                                 unsigned int* changed, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "frontier_relax: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(k >= 1 && sweep0 >= 0 && sweep0 <= 0x7fffffff - k, "frontier_relax: sweep0=%d k=%d", sweep0, k);
  GS_REQUIRE(label && flags && changed, "frontier_relax: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  const int nb0 = gs_cdiv(n0, B0), nb1 = gs_cdiv(n1, B1), nb2 = gs_cdiv(n2, B2);
  const size_t nbricks = (size_t)nb0 * nb1 * nb2;           // at most 2^20 workgroups for the shipped brick
  return brick_relax_enqueue("frontier_relax", nbricks, flags, sweep0, k, changed, s,
                             [&](unsigned char* cur, unsigned char* next, unsigned int* ch) {
                               frontier_relax_kernel<<<(unsigned)nbricks, FR_THREADS, 0, s>>>(label, n0, n1, n2, nb0, nb1,
                                                                                             nb2, cur, next, ch);
                             });
}

extern "C" int gs_frontier_roots(const int* label, int n0, int n1, int n2, void* workspace, size_t workspace_bytes,
                                 int* n_roots, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "frontier_roots: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(label && workspace && n_roots, "frontier_roots: null pointer");
  GS_REQUIRE(workspace_bytes >= gs_frontier_workspace_bytes(n0, n1, n2), "frontier_roots: workspace of %zu bytes, %zu needed",
             workspace_bytes, gs_frontier_workspace_bytes(n0, n1, n2));
  const hipStream_t s = (hipStream_t)stream;
  const int nblk = fr_blocks(n0, n1, n2);
  unsigned* count = (unsigned*)workspace;
  unsigned* first = fr_workspace_first(workspace, nblk);
  GS_TIMING_PRE();
  frontier_count_kernel<<<nblk, FR_THREADS, 0, s>>>(label, n0 * n1 * n2, count);
  GS_CHECK_LAUNCH("frontier_count");
  frontier_scan_kernel<<<1, FR_SCAN_THREADS, 0, s>>>(count, nblk, gs_cdiv(nblk, FR_SCAN_THREADS), first, n_roots);
  GS_CHECK_LAUNCH("frontier_scan");
  return GS_OK;
}

extern "C" int gs_frontier_table(const unsigned char* state, const int* label, const int* cost, int n0, int n1, int n2,
                                 const void* workspace, size_t workspace_bytes, int rows, int capacity, int* root,
                                 int* size, int* faces, long long* sum, int* bbox, int* best, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "frontier_table: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(rows >= 0 && capacity >= rows, "frontier_table: %d rows do not fit a table of capacity %d", rows, capacity);
  GS_REQUIRE(state && label && workspace && root && size && faces && sum && bbox && best, "frontier_table: null pointer");
  GS_REQUIRE(((uintptr_t)best & 7u) == 0, "frontier_table: best is not 8-byte aligned");
  GS_REQUIRE(workspace_bytes >= gs_frontier_workspace_bytes(n0, n1, n2), "frontier_table: workspace of %zu bytes, %zu needed",
             workspace_bytes, gs_frontier_workspace_bytes(n0, n1, n2));
  if (rows == 0) return GS_OK;
  const hipStream_t s = (hipStream_t)stream;
  const int nblk = fr_blocks(n0, n1, n2);
  const unsigned* first = fr_workspace_first(workspace, nblk);
  GS_TIMING_PRE();
  frontier_emit_kernel<<<nblk, FR_THREADS, 0, s>>>(label, n0 * n1 * n2, first, rows, root, size, faces,
                                                   (unsigned long long*)sum, bbox, (unsigned long long*)best);
  GS_CHECK_LAUNCH("frontier_emit");
  frontier_table_kernel<<<nblk, FR_THREADS, 0, s>>>(state, label, cost, n0, n1, n2, root, rows, size, faces,
                                                    (unsigned long long*)sum, bbox, (unsigned long long*)best);
  GS_CHECK_LAUNCH("frontier_table");
  return GS_OK;
}
