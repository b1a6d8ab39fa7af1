// What the kernels that make one table row per component of a label lattice share (frontier.hip, tsdf_objects.hip): the
// brick of the relaxation, the geometry of the lattice-wide passes, the rank of a block's roots and the layout of the
// workspace gs_frontier_roots fills.
#pragma once
#include "brick_relax.h"

namespace {

#ifndef FRONTIER_B0      // the brick; tools/frontier_bench.py measures other shapes through a library built with these set
#define FRONTIER_B0 4
#define FRONTIER_B1 4
#define FRONTIER_B2 32
#endif
#ifndef FRONTIER_ROUNDS_MAX   // rounds inside LDS per sweep
#define FRONTIER_ROUNDS_MAX 64
#endif
using FrBrick = Brick<FRONTIER_B0, FRONTIER_B1, FRONTIER_B2, FRONTIER_ROUNDS_MAX>;
constexpr int B0 = FrBrick::B0, B1 = FrBrick::B1, B2 = FrBrick::B2;
constexpr int FR_THREADS = FrBrick::THREADS;
constexpr int FR_WAVES = FR_THREADS / GS_WAVE;
constexpr int FR_MAX = BRICK_MAX_CELLS;                    // cells per axis
constexpr int FR_PER = 8;                                  // cells per lane of the lattice-wide passes
constexpr int FR_BLOCK = FR_THREADS * FR_PER;              // cells per workgroup of those passes

__device__ __forceinline__ int fr_popc(unsigned long long b) { return __popcll(b); }

// Which of this lane's FR_PER cells of block `base` are roots, each one's rank among the block's roots in ascending cell
// order, and the block's number of roots.  wcount is LDS [FR_PER * FR_WAVES]; holds a barrier.
__device__ __forceinline__ unsigned fr_rank_roots(const int* __restrict__ label, int ncells, int base, unsigned* wcount,
                                                  bool (&is)[FR_PER], unsigned (&rank)[FR_PER]) {
  const int tid = threadIdx.x, lane = tid % GS_WAVE, wave = tid / GS_WAVE;
#pragma unroll
  for (int i = 0; i < FR_PER; ++i) {
    const int p = base + i * FR_THREADS + tid;
    is[i] = p < ncells && label[p] == p;
    const unsigned long long b = __ballot(is[i]);
    rank[i] = fr_popc(b & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[i * FR_WAVES + wave] = fr_popc(b);
  }
  __syncthreads();
  unsigned run = 0;
#pragma unroll
  for (int i = 0; i < FR_PER; ++i) {
#pragma unroll
    for (int w = 0; w < FR_WAVES; ++w) {
      if (w == wave) rank[i] += run;
      run += wcount[i * FR_WAVES + w];
    }
  }
  return run;
}

// The pass that folds labelled cells into table rows (tsdf_objects.hip, rooms.hip), over blocks of FR_BLOCK cells: a cell
// finds its row by binary search of its label among the ascending roots; the lanes of a wave that share a row take one
// turn together.  Fold: int load(p, id) forms what cell p adds to row id (id < 0: nothing; it may drop the cell by
// returning -1); fold(row, mine, members, leader) reduces over the lanes with `mine` and has the lane with `leader`
// issue the atomics.
template <class Fold>
__device__ __forceinline__ void fr_fold_rows(const int* __restrict__ label, int ncells, const int* __restrict__ root,
                                             int rows, Fold& f) {
  const int tid = threadIdx.x, lane = tid % GS_WAVE;
  const int base = blockIdx.x * FR_BLOCK;
  for (int i = 0; i < FR_PER; ++i) {
    const int p = base + i * FR_THREADS + tid;
    const int l = p < ncells ? label[p] : -1;
    if (__ballot(l >= 0) == 0) continue;                    // the wave's 64 cells hold no labelled cell: most do not
    int id = -1;
    if (l >= 0) {
      int lo = 0, hi = rows;                                // the first row whose root is >= l
      for (int s = 0; s < 31 && lo < hi; ++s) {
        const int mid = lo + (hi - lo) / 2;
        if (root[mid] < l) lo = mid + 1; else hi = mid;
      }
      if (lo < rows && root[lo] == l) id = lo;              // else: a table that does not hold this cluster
    }
    id = f.load(p, id);
    unsigned long long todo = __ballot(id >= 0);
    for (int it = 0; it < GS_WAVE && todo != 0; ++it) {     // one turn per distinct row among the wave's cells
      const int leader = __ffsll((long long)todo) - 1;
      const int row = __shfl(id, leader, GS_WAVE);
      const bool mine = id == row;
      const unsigned long long members = __ballot(mine);
      todo &= ~members;
      f.fold(row, mine, members, lane == leader);
    }
  }
}

int fr_blocks(int n0, int n1, int n2) { return (int)(((long long)n0 * n1 * n2 + FR_BLOCK - 1) / FR_BLOCK); }     // <= 2^19

// the workspace: count and first, u32 per block each
size_t fr_workspace_bytes(int nblk) { return 2 * gs_align(sizeof(unsigned) * (size_t)nblk); }
unsigned* fr_workspace_first(const void* workspace, int nblk) {
  return (unsigned*)((char*)workspace + gs_align(sizeof(unsigned) * (size_t)nblk));
}

}  // namespace
