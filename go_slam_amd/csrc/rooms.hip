// Rooms and doorways of a passability lattice: the free space split by clearance into one region per wide place, the
// cells where two regions meet, and one table row per room and per doorway (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_room_*); tests/rooms_restatement.py restates it serially.  Integer only.
//
// The host runs three relaxations one after the other, each to its fixed point before the next begins:
//   1. the core components: room_mark_kernel writes label (own index on a core cell, -1 elsewhere), the counts and the
//      dirty bytes, gs_frontier_relax / gs_frontier_roots label and rank the components as they stand, gs_room_cores emits
//      the roots and sizes and gs_room_seed takes the dropped components' labels away;
//   2. the cost to the nearest kept core cell: gs_geodesic_init / gs_geodesic_relax, unchanged;
//   3. the room labels: gs_room_relax, k launches of room_relax_kernel, the brick sweep of brick_relax.h with RoomRule.
// RoomRule: a tile entry is the label as unsigned (-1, the largest value, where a cell holds none or there is no lattice);
//   beside the labels a brick loads its tile's costs and passability into LDS.  prepare derives, once per cell, the 26-bit
//   mask of the cell's parents on the shortest-route graph: move m is a parent when it is allowed (the box it spans is
//   passable, geo_moves.h) and cost[p + m] + w(m) == cost[p].  The mask stays in a register; lower is the minimum of the
//   tile's labels over it.  Only passable cells with 0 < cost < INF and a parent are active: a kept core cell (cost 0)
//   keeps the root it holds, a cell no route reaches keeps -1.
// Why the fixed point is reached whatever the order (the argument brick_relax.h asks of every rule), given that cost and
// the core labels are at their own fixed points, which the order of the three relaxations guarantees:
//   every stored label other than -1 is the root of a kept core at distance exactly cost[p] from p.  A kept core cell
//     holds its component's root at distance 0.  A cell p is only ever given the label r that a parent q holds or held,
//     a stale one included; r's core lies at distance cost[q] from q, the move from q to p is allowed, so it lies at most
//     cost[q] + w = cost[p] from p, and no core lies nearer than cost[p];
//   labels only fall, and a cell's parents all hold a smaller cost than the cell (every weight is positive), so the
//     shortest-route graph has no cycle and "the smallest label among my parents" has exactly one solution: by induction
//     over ascending cost, the smallest root among the kept cores at distance cost[p].  At the cost's fixed point every
//     cell with 0 < cost < INF has a parent, so every such cell ends labelled.
//   Were cost not at its fixed point, a cell could have no parent yet or a parent set that later changes, and a label
//   already stored could name a core that is not nearest: labels never rise, so that would stay wrong.
// gs_room_seed's first dirty bytes: every brick that holds a passable cell.  What is needed is that every brick holding
//   a passable non-core cell with a labelled 26-neighbour is swept first -- those are the only cells that can fall before
//   a neighbour has -- and the chosen set contains these bricks; it costs one flag store per passable cell and no
//   neighbour reads, and a brick marked in vain loads its tile once, lowers nothing and marks nobody.
// room_door_mark_kernel: a labelled cell is a boundary cell when an allowed move leads to a cell with another label
//   (room_across: 27 passability bytes, then the labels across the allowed moves).  Boundary cells get their own index in
//   door_label, and gs_frontier_relax / gs_frontier_roots / gs_room_cores label, rank and emit the doorways as they did the
//   cores.
// Tables: the rooms, and the cores' sizes, by room_fold_lanes below (a lane adds up its own cells first: rooms are few and
//   large), the doorways by fr_fold_rows (frontier_rows.h); integer atomics only, one lane per (wave, row) and turn; a
//   doorway's widest cell is one 64-bit atomic max of d2 << 32 | ~cell.  No scratch, no floating point, and no kernel
//   waits for another workgroup.
#include "frontier_rows.h"
#include "geo_moves.h"

namespace {

constexpr unsigned ROOM_NONE = 0xffffffffu;                // label -1
constexpr int ROOM_INF = GS_GEO_INF;

// ---- marking ------------------------------------------------------------------------------------------------------------
// counts[0 .. NC): each the number of this workgroup's lanes-and-cells for which the flag was set; one atomic per count
template <int NC>
__device__ __forceinline__ void room_add_counts(const unsigned (&n)[NC], unsigned (*part)[NC], unsigned* counts) {
  const int tid = threadIdx.x, lane = tid % GS_WAVE, wave = tid / GS_WAVE;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) part[wave][c] = n[c];
  }
  __syncthreads();
  if (tid < NC) {
    unsigned total = 0;
#pragma unroll
    for (int w = 0; w < FR_WAVES; ++w) total += part[w][tid];
    if (total != 0) atomicAdd(&counts[tid], total);
  }
}

__device__ __forceinline__ size_t room_brick_of(int p, int n1, int n2, int nb1, int nb2) {
  const int c2 = p % n2, c1 = p / n2 % n1, c0 = p / n2 / n1;
  return ((size_t)(c0 / B0) * nb1 + c1 / B1) * nb2 + c2 / B2;
}

__global__ __launch_bounds__(FR_THREADS) void room_mark_kernel(const unsigned char* __restrict__ open,
                                                               const unsigned char* __restrict__ core, int ncells, int n1,
                                                               int n2, int nb1, int nb2, int* __restrict__ label,
                                                               unsigned int* counts, unsigned char* flags) {
  __shared__ unsigned part[FR_WAVES][2];
  const int tid = threadIdx.x;
  const int base = blockIdx.x * FR_BLOCK;
  unsigned n[2] = {0u, 0u};                                 // wave totals: open cells, core cells
#pragma unroll
  for (int i = 0; i < FR_PER; ++i) {
    const int p = base + i * FR_THREADS + tid;
    const bool in = p < ncells;
    const bool is_open = in && open[p] != 0;
    const bool is_core = is_open && core[p] != 0;
    if (in) label[p] = is_core ? p : -1;
    if (is_core) flags[room_brick_of(p, n1, n2, nb1, nb2)] = 1;               // buffer 0; every store writes 1
    n[0] += fr_popc(__ballot(is_open));
    n[1] += fr_popc(__ballot(is_core));
  }
  room_add_counts<2>(n, part, counts);
}

// the roots in ascending order into the first `rows` rows, each row's size (if asked for) cleared
__global__ __launch_bounds__(FR_THREADS) void room_emit_kernel(const int* __restrict__ label, int ncells,
                                                               const unsigned* __restrict__ first, int rows,
                                                               int* __restrict__ root, int* __restrict__ size) {
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
    if (size != nullptr) size[slot] = 0;
  }
}

// The pass that folds the cells of a few large components into rows.  fr_fold_rows takes a wave's turns once per 64 cells;
// with rooms of millions of cells every one of those turns ends in atomics on the same few rows.  Here a lane first adds
// up its own FR_PER cells for as long as they share a row, and the wave takes its turns over the lanes' sums: where a
// wave's 512 cells lie in one room, one turn instead of eight.  Every operation is exact and commutes, so the rows are
// the same.  Fold: reset() empties what the lane holds, add(p) adds cell p to it, fold(row, mine, leader) reduces over the
// lanes with `mine` and has the lane with `leader` issue the atomics.
template <class Fold>
__device__ __forceinline__ void room_fold_lanes(const int* __restrict__ label, int ncells, const int* __restrict__ root,
                                                int rows, Fold& f) {
  const int tid = threadIdx.x, lane = tid % GS_WAVE;
  const int base = blockIdx.x * FR_BLOCK;
  int held = -1;                                            // the row of what this lane holds
  f.reset();
  for (int i = 0; i <= FR_PER; ++i) {                       // the last pass only hands over what is held
    const int p = base + i * FR_THREADS + tid;
    const int l = i < FR_PER && p < ncells ? label[p] : -1;
    int id = -1;
    if (l >= 0) {
      int lo = 0, hi = rows;                                // the first row whose root is >= l
      for (int s = 0; s < 31 && lo < hi; ++s) {
        const int mid = lo + (hi - lo) / 2;
        if (root[mid] < l) lo = mid + 1; else hi = mid;
      }
      if (lo < rows && root[lo] == l) id = lo;              // else: a table that does not hold this component
    }
    const bool flush = held >= 0 && (i == FR_PER || (id >= 0 && id != held));
    unsigned long long todo = __ballot(flush);
    for (int it = 0; it < GS_WAVE && todo != 0; ++it) {     // one turn per distinct row among the lanes that hand over
      const int leader = __ffsll((long long)todo) - 1;
      const int row = __shfl(held, leader, GS_WAVE);
      const bool mine = flush && held == row;
      todo &= ~__ballot(mine);
      f.fold(row, mine, lane == leader);
    }
    if (flush) {
      held = -1;
      f.reset();
    }
    if (id >= 0) {
      held = id;
      f.add(p);
    }
  }
}

struct SizeFold {
  int* size;
  int n;
  __device__ __forceinline__ void reset() { n = 0; }
  __device__ __forceinline__ void add(int) { ++n; }
  __device__ __forceinline__ void fold(int row, bool mine, bool leader) {
    const int total = gs_wave_sum_i32(mine ? n : 0);
    if (leader) atomicAdd(&size[row], total);
  }
};

__global__ __launch_bounds__(FR_THREADS) void room_sizes_kernel(const int* __restrict__ label, int ncells,
                                                                const int* __restrict__ root, int rows, SizeFold f) {
  room_fold_lanes(label, ncells, root, rows, f);
}

// label = -1 on the cells of the components whose keep byte is 0; flag buffer 0 set for every brick with an open cell
__global__ __launch_bounds__(FR_THREADS) void room_seed_kernel(const unsigned char* __restrict__ open, int ncells, int n1,
                                                               int n2, int nb1, int nb2, const int* __restrict__ root,
                                                               const unsigned char* __restrict__ keep, int rows,
                                                               int* __restrict__ label, unsigned char* flags) {
  const int tid = threadIdx.x;
  const int base = blockIdx.x * FR_BLOCK;
#pragma unroll
  for (int i = 0; i < FR_PER; ++i) {
    const int p = base + i * FR_THREADS + tid;
    if (p >= ncells) continue;
    const int l = label[p];
    if (l >= 0) {
      int lo = 0, hi = rows;                                // the first row whose root is >= l
      for (int s = 0; s < 31 && lo < hi; ++s) {
        const int mid = lo + (hi - lo) / 2;
        if (root[mid] < l) lo = mid + 1; else hi = mid;
      }
      if (!(lo < rows && root[lo] == l && keep[lo] != 0)) label[p] = -1;      // dropped, or not of this table
    }
    if (open[p] != 0) flags[room_brick_of(p, n1, n2, nb1, nb2)] = 1;          // buffer 0; every store writes 1
  }
}

// ---- the room relaxation ------------------------------------------------------------------------------------------------
struct RoomRule {
  using Value = unsigned;
  struct Cell { unsigned parents; };                        // bit m: move m is allowed and cost[p + m] + w(m) == cost[p]
  const unsigned char* open;
  const int* cost;
  int* label;
  int* costs;                                               // LDS [TILE]: the tile's costs, INF outside the lattice
  unsigned char* pass;                                      // LDS [TILE]: 1 where the tile's cell is inside and passable
  __device__ __forceinline__ unsigned load(size_t at, bool inside, int q) const {
    const unsigned v = (unsigned)label[at];
    const int c = cost[at];
    const unsigned char o = open[at];
    costs[q] = inside ? c : ROOM_INF;
    pass[q] = inside && o != 0 ? 1 : 0;
    return inside ? v : ROOM_NONE;
  }
  __device__ __forceinline__ unsigned prepare(const unsigned*, int at, unsigned v, Cell& cell) const {
    cell.parents = 0u;
    const int c = costs[at];
    if (pass[at] == 0 || c <= 0 || c >= ROOM_INF) return v; // a wall, a kept core cell, a cell no route reaches
    unsigned around = 0;
#pragma unroll
    for (int e = 0; e < 27; ++e)
      around |= (unsigned)pass[at + FrBrick::tile_offset(e / 9 - 1, e / 3 % 3 - 1, e % 3 - 1)] << e;
    unsigned parents = 0;
#pragma unroll
    for (int m = 0; m < 26; ++m) {
      const bool from = costs[at + FrBrick::nb_offset(m)] + geo_weight(m) == c;
      parents |= (around & geo_box(m)) == geo_box(m) && from ? 1u << m : 0u;
    }
    cell.parents = parents;
    return v;
  }
  __device__ __forceinline__ bool active(unsigned, const Cell& cell) const { return cell.parents != 0u; }
  __device__ __forceinline__ unsigned lower(const unsigned* tile, int at, unsigned v, const Cell& cell) const {
    unsigned best = v;
#pragma unroll
    for (int m = 0; m < 26; ++m) {
      const unsigned cand = tile[at + FrBrick::nb_offset(m)];
      if ((cell.parents >> m & 1u) != 0 && cand < best) best = cand;          // ROOM_NONE never wins
    }
    return best;
  }
  __device__ __forceinline__ void store(size_t at, unsigned v) const { label[at] = (int)v; }
};

__global__ __launch_bounds__(FR_THREADS) void room_relax_kernel(const unsigned char* __restrict__ open,
                                                                const int* __restrict__ cost, int* label, int n0, int n1,
                                                                int n2, int nb0, int nb1, int nb2, unsigned char* cur,
                                                                unsigned char* next, unsigned int* changed) {
  __shared__ int costs[FrBrick::TILE];
  __shared__ unsigned char pass[FrBrick::TILE];
  brick_relax<FrBrick>(RoomRule{open, cost, label, costs, pass}, n0, n1, n2, nb0, nb1, nb2, cur, next, changed);
}

// ---- doorways -----------------------------------------------------------------------------------------------------------
// The labels across the allowed moves of the labelled cell p = (c0, c1, c2) with label l that differ from l: whether there
// is one; lo / hi: the smallest and largest of l and them.
__device__ __forceinline__ bool room_across(const unsigned char* __restrict__ open, const int* __restrict__ label, int p,
                                            int c0, int c1, int c2, int n0, int n1, int n2, int l, int& lo, int& hi) {
  unsigned around = 0;
  for (int d0 = -1; d0 <= 1; ++d0)
    for (int d1 = -1; d1 <= 1; ++d1)
#pragma unroll
      for (int d2 = -1; d2 <= 1; ++d2) {
        const int q0 = c0 + d0, q1 = c1 + d1, q2 = c2 + d2;
        if (q0 < 0 || q0 >= n0 || q1 < 0 || q1 >= n1 || q2 < 0 || q2 >= n2) continue;
        if (open[p + (d0 * n1 + d1) * n2 + d2] != 0) around |= 1u << ((d0 + 1) * 9 + (d1 + 1) * 3 + d2 + 1);
      }
  lo = l, hi = l;
  bool any = false;
#pragma unroll
  for (int m = 0; m < 26; ++m) {
    if ((around & geo_box(m)) != geo_box(m)) continue;      // the far end's bit is one of the box's: it is inside
    const int q = label[p + (geo_d0(m) * n1 + geo_d1(m)) * n2 + geo_d2(m)];
    if (q < 0 || q == l) continue;
    any = true;
    lo = q < lo ? q : lo;
    hi = q > hi ? q : hi;
  }
  return any;
}

__global__ __launch_bounds__(FR_THREADS) void room_door_mark_kernel(const unsigned char* __restrict__ open,
                                                                    const int* __restrict__ label, int n0, int n1, int n2,
                                                                    int nb1, int nb2, int* __restrict__ door_label,
                                                                    unsigned int* count, unsigned char* flags) {
  __shared__ unsigned part[FR_WAVES][1];
  const int tid = threadIdx.x;
  const int ncells = n0 * n1 * n2;
  const int base = blockIdx.x * FR_BLOCK;
  unsigned n[1] = {0u};                                     // wave total: boundary cells
  for (int i = 0; i < FR_PER; ++i) {
    const int p = base + i * FR_THREADS + tid;
    const bool in = p < ncells;
    const int l = in ? label[p] : -1;
    bool edge = false;
    if (l >= 0) {
      const int c2 = p % n2, c1 = p / n2 % n1, c0 = p / n2 / n1;
      int lo, hi;
      edge = room_across(open, label, p, c0, c1, c2, n0, n1, n2, l, lo, hi);
      if (edge) flags[((size_t)(c0 / B0) * nb1 + c1 / B1) * nb2 + c2 / B2] = 1;      // buffer 0; every store writes 1
    }
    if (in) door_label[p] = edge ? p : -1;
    n[0] += fr_popc(__ballot(edge));
  }
  room_add_counts<1>(n, part, count);
}

// ---- tables -------------------------------------------------------------------------------------------------------------
// what both tables hold of a row's cells: their number, coordinate sums and box; a lane's share of them between calls
struct CellsFold {
  int n1, n2;
  int* size;
  unsigned long long* sum;
  int* bbox;
  int n, s0, s1, s2, lo0, lo1, lo2, hi0, hi1, hi2;
  __device__ __forceinline__ void reset() {
    n = 0, s0 = 0, s1 = 0, s2 = 0;
    lo0 = FR_MAX, lo1 = FR_MAX, lo2 = FR_MAX, hi0 = -1, hi1 = -1, hi2 = -1;
  }
  __device__ __forceinline__ void add(int p) {
    const int c2 = p % n2, c1 = p / n2 % n1, c0 = p / n2 / n1;
    ++n;
    s0 += c0, s1 += c1, s2 += c2;                           // at most FR_PER * 1023
    lo0 = c0 < lo0 ? c0 : lo0, lo1 = c1 < lo1 ? c1 : lo1, lo2 = c2 < lo2 ? c2 : lo2;
    hi0 = c0 > hi0 ? c0 : hi0, hi1 = c1 > hi1 ? c1 : hi1, hi2 = c2 > hi2 ? c2 : hi2;
  }
  __device__ __forceinline__ void fold_cells(int row, bool mine, bool leader) {
    const int total = gs_wave_sum_i32(mine ? n : 0);
    const int t0 = gs_wave_sum_i32(mine ? s0 : 0), t1 = gs_wave_sum_i32(mine ? s1 : 0);
    const int t2 = gs_wave_sum_i32(mine ? s2 : 0);          // at most 64 * FR_PER * 1023
    const int a0 = gs_wave_min_i32(mine ? lo0 : FR_MAX), a1 = gs_wave_min_i32(mine ? lo1 : FR_MAX);
    const int a2 = gs_wave_min_i32(mine ? lo2 : FR_MAX);
    const int b0 = -gs_wave_min_i32(mine ? -hi0 : 1), b1 = -gs_wave_min_i32(mine ? -hi1 : 1);
    const int b2 = -gs_wave_min_i32(mine ? -hi2 : 1);
    if (!leader) return;
    atomicAdd(&size[row], total);
    atomicAdd(&sum[(size_t)row * 3 + 0], (unsigned long long)t0);
    atomicAdd(&sum[(size_t)row * 3 + 1], (unsigned long long)t1);
    atomicAdd(&sum[(size_t)row * 3 + 2], (unsigned long long)t2);
    atomicMin(&bbox[(size_t)row * 6 + 0], a0);
    atomicMin(&bbox[(size_t)row * 6 + 1], a1);
    atomicMin(&bbox[(size_t)row * 6 + 2], a2);
    atomicMax(&bbox[(size_t)row * 6 + 3], b0);
    atomicMax(&bbox[(size_t)row * 6 + 4], b1);
    atomicMax(&bbox[(size_t)row * 6 + 5], b2);
  }
};

struct RoomFold {                                           // on room_fold_lanes
  CellsFold cells;
  const int* cost;
  int* core_size;
  int* reach;
  int n_core, far;                                          // a kept core cell is a labelled cell at cost 0
  __device__ __forceinline__ void reset() {
    cells.reset();
    n_core = 0, far = 0;
  }
  __device__ __forceinline__ void add(int p) {
    cells.add(p);
    const int c = cost[p];
    n_core += c == 0;
    far = c > far ? c : far;
  }
  __device__ __forceinline__ void fold(int row, bool mine, bool leader) {
    cells.fold_cells(row, mine, leader);
    const int cores = gs_wave_sum_i32(mine ? n_core : 0);
    const int furthest = -gs_wave_min_i32(mine ? -far : 1);
    if (!leader) return;
    if (cores != 0) atomicAdd(&core_size[row], cores);
    atomicMax(&reach[row], furthest);
  }
};

struct DoorFold {                                           // on fr_fold_rows: doorways are few cells
  CellsFold cells;
  const unsigned char* open;
  const int* label;                                         // the rooms'
  const int* d2;                                            // or nullptr
  int n0;
  int* room_lo;
  int* room_hi;
  unsigned long long* widest;
  int lo, hi;
  unsigned long long key;
  __device__ __forceinline__ int load(int p, int id) {
    cells.reset();
    lo = 0x7fffffff, hi = -1, key = 0ull;
    const int l = id >= 0 ? label[p] : -1;
    if (l < 0) return -1;                                   // door labels that are not these rooms'
    cells.add(p);
    const int c2 = p % cells.n2, c1 = p / cells.n2 % cells.n1, c0 = p / cells.n2 / cells.n1;
    room_across(open, label, p, c0, c1, c2, n0, cells.n1, cells.n2, l, lo, hi);
    const int w = d2 != nullptr ? d2[p] : 0;
    key = (unsigned long long)(unsigned)(w > 0 ? w : 0) << 32 | (0xffffffffu - (unsigned)p);
    return id;
  }
  __device__ __forceinline__ void fold(int row, bool mine, unsigned long long, bool leader) {
    cells.fold_cells(row, mine, leader);
    const int l = gs_wave_min_i32(mine ? lo : 0x7fffffff);
    const int h = -gs_wave_min_i32(mine ? -hi : 1);
    const unsigned long long k = ~gs_wave_min_u64(mine ? ~key : ~0ull);       // the largest key
    if (!leader) return;
    atomicMin(&room_lo[row], l);
    atomicMax(&room_hi[row], h);
    atomicMax(&widest[row], k);
  }
};

__global__ __launch_bounds__(FR_THREADS) void room_table_init_kernel(int rows, int* __restrict__ size,
                                                                     unsigned long long* __restrict__ sum,
                                                                     int* __restrict__ bbox, int* __restrict__ core_size,
                                                                     int* __restrict__ reach, int* __restrict__ room_lo,
                                                                     int* __restrict__ room_hi,
                                                                     unsigned long long* __restrict__ widest) {
  const int r = blockIdx.x * FR_THREADS + threadIdx.x;
  if (r >= rows) return;
  size[r] = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    sum[(size_t)r * 3 + a] = 0ull;
    bbox[(size_t)r * 6 + a] = FR_MAX;
    bbox[(size_t)r * 6 + 3 + a] = -1;
  }
  if (core_size != nullptr) {                               // a room
    core_size[r] = 0;
    reach[r] = 0;
  } else {                                                  // a doorway
    room_lo[r] = 0x7fffffff;
    room_hi[r] = -1;
    widest[r] = 0ull;
  }
}

__global__ __launch_bounds__(FR_THREADS) void room_table_kernel(const int* __restrict__ label, int ncells,
                                                                const int* __restrict__ root, int rows, RoomFold f) {
  room_fold_lanes(label, ncells, root, rows, f);
}

__global__ __launch_bounds__(FR_THREADS) void room_door_table_kernel(const int* __restrict__ label, int ncells,
                                                                     const int* __restrict__ root, int rows, DoorFold f) {
  fr_fold_rows(label, ncells, root, rows, f);
}

}  // namespace

extern "C" size_t gs_frontier_flags_bytes(int n0, int n1, int n2);
extern "C" size_t gs_frontier_workspace_bytes(int n0, int n1, int n2);

extern "C" int gs_room_mark(const unsigned char* open, const unsigned char* core, int n0, int n1, int n2, int* label,
                            unsigned int* counts, unsigned char* flags, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "room_mark: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(open && core && label && counts && flags, "room_mark: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(unsigned int) * 2, s) != hipSuccess ||
      hipMemsetAsync(flags, 0, gs_frontier_flags_bytes(n0, n1, n2), s) != hipSuccess) {
    gs_set_error("room_mark: clearing counts and flags failed");
    return GS_ERR_LAUNCH;
  }
  GS_TIMING_PRE();
  room_mark_kernel<<<fr_blocks(n0, n1, n2), FR_THREADS, 0, s>>>(open, core, n0 * n1 * n2, n1, n2, gs_cdiv(n1, B1),
                                                                gs_cdiv(n2, B2), label, counts, flags);
  GS_CHECK_LAUNCH("room_mark");
  return GS_OK;
}

extern "C" int gs_room_cores(const int* label, int n0, int n1, int n2, const void* workspace, size_t workspace_bytes,
                             int rows, int capacity, int* root, int* size, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "room_cores: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(rows >= 0 && capacity >= rows, "room_cores: %d rows do not fit a table of capacity %d", rows, capacity);
  GS_REQUIRE(label && workspace && root, "room_cores: null pointer");
  GS_REQUIRE(workspace_bytes >= gs_frontier_workspace_bytes(n0, n1, n2), "room_cores: workspace of %zu bytes, %zu needed",
             workspace_bytes, gs_frontier_workspace_bytes(n0, n1, n2));
  if (rows == 0) return GS_OK;
  const hipStream_t s = (hipStream_t)stream;
  const int nblk = fr_blocks(n0, n1, n2), ncells = n0 * n1 * n2;
  GS_TIMING_PRE();
  room_emit_kernel<<<nblk, FR_THREADS, 0, s>>>(label, ncells, fr_workspace_first(workspace, nblk), rows, root, size);
  GS_CHECK_LAUNCH("room_emit");
  if (size == nullptr) return GS_OK;                        // the caller's table counts the cells itself
  room_sizes_kernel<<<nblk, FR_THREADS, 0, s>>>(label, ncells, root, rows, SizeFold{size, 0});
  GS_CHECK_LAUNCH("room_sizes");
  return GS_OK;
}

extern "C" int gs_room_seed(const unsigned char* open, int n0, int n1, int n2, const int* root, const unsigned char* keep,
                            int rows, int* label, unsigned char* flags, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "room_seed: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(rows >= 0, "room_seed: rows=%d", rows);
  GS_REQUIRE(open && label && flags && ((root && keep) || rows == 0), "room_seed: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(flags, 0, gs_frontier_flags_bytes(n0, n1, n2), s) != hipSuccess) {
    gs_set_error("room_seed: clearing flags failed");
    return GS_ERR_LAUNCH;
  }
  GS_TIMING_PRE();
  room_seed_kernel<<<fr_blocks(n0, n1, n2), FR_THREADS, 0, s>>>(open, n0 * n1 * n2, n1, n2, gs_cdiv(n1, B1),
                                                                gs_cdiv(n2, B2), root, keep, rows, label, flags);
  GS_CHECK_LAUNCH("room_seed");
  return GS_OK;
}

extern "C" int gs_room_relax(const unsigned char* open, const int* cost, int n0, int n1, int n2, int* label,
                             unsigned char* flags, int sweep0, int k, unsigned int* changed, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "room_relax: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(k >= 1 && sweep0 >= 0 && sweep0 <= 0x7fffffff - k, "room_relax: sweep0=%d k=%d", sweep0, k);
  GS_REQUIRE(open && cost && label && flags && changed, "room_relax: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  const int nb0 = gs_cdiv(n0, B0), nb1 = gs_cdiv(n1, B1), nb2 = gs_cdiv(n2, B2);
  const size_t nbricks = (size_t)nb0 * nb1 * nb2;           // at most 2^20 workgroups for the shipped brick
  return brick_relax_enqueue("room_relax", nbricks, flags, sweep0, k, changed, s,
                             [&](unsigned char* cur, unsigned char* next, unsigned int* ch) {
                               room_relax_kernel<<<(unsigned)nbricks, FR_THREADS, 0, s>>>(open, cost, label, n0, n1, n2, nb0,
                                                                                         nb1, nb2, cur, next, ch);
                             });
}

extern "C" int gs_room_door_mark(const unsigned char* open, const int* label, int n0, int n1, int n2, int* door_label,
                                 unsigned int* count, unsigned char* flags, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "room_door_mark: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(open && label && door_label && count && flags, "room_door_mark: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(count, 0, sizeof(unsigned int), s) != hipSuccess ||
      hipMemsetAsync(flags, 0, gs_frontier_flags_bytes(n0, n1, n2), s) != hipSuccess) {
    gs_set_error("room_door_mark: clearing count and flags failed");
    return GS_ERR_LAUNCH;
  }
  GS_TIMING_PRE();
  room_door_mark_kernel<<<fr_blocks(n0, n1, n2), FR_THREADS, 0, s>>>(open, label, n0, n1, n2, gs_cdiv(n1, B1),
                                                                     gs_cdiv(n2, B2), door_label, count, flags);
  GS_CHECK_LAUNCH("room_door_mark");
  return GS_OK;
}

extern "C" int gs_room_table(const int* label, const int* cost, int n0, int n1, int n2, const int* root, int rows, int* size,
                             int* core_size, long long* sum, int* bbox, int* reach, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "room_table: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(rows >= 0, "room_table: rows=%d", rows);
  GS_REQUIRE(label && cost && root && size && core_size && sum && bbox && reach, "room_table: null pointer");
  GS_REQUIRE(((uintptr_t)sum & 7u) == 0, "room_table: sum is not 8-byte aligned");
  if (rows == 0) return GS_OK;
  const hipStream_t s = (hipStream_t)stream;
  RoomFold f = {};
  f.cells.n1 = n1; f.cells.n2 = n2; f.cells.size = size; f.cells.sum = (unsigned long long*)sum; f.cells.bbox = bbox;
  f.cost = cost; f.core_size = core_size; f.reach = reach;
  GS_TIMING_PRE();
  room_table_init_kernel<<<gs_cdiv(rows, FR_THREADS), FR_THREADS, 0, s>>>(rows, size, f.cells.sum, bbox, core_size, reach,
                                                                          nullptr, nullptr, nullptr);
  GS_CHECK_LAUNCH("room_table_init");
  room_table_kernel<<<fr_blocks(n0, n1, n2), FR_THREADS, 0, s>>>(label, n0 * n1 * n2, root, rows, f);
  GS_CHECK_LAUNCH("room_table");
  return GS_OK;
}

extern "C" int gs_room_door_table(const unsigned char* open, const int* label, const int* door_label, const int* d2, int n0,
                                  int n1, int n2, const int* root, int rows, int* size, long long* sum, int* bbox,
                                  int* room_lo, int* room_hi, unsigned long long* widest, gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(n0, n1, n2), "room_door_table: lattice %d x %d x %d outside [1, 1024]", n0, n1, n2);
  GS_REQUIRE(rows >= 0, "room_door_table: rows=%d", rows);
  GS_REQUIRE(open && label && door_label && root && size && sum && bbox && room_lo && room_hi && widest,
             "room_door_table: null pointer");
  GS_REQUIRE((((uintptr_t)sum | (uintptr_t)widest) & 7u) == 0, "room_door_table: sum or widest is not 8-byte aligned");
  if (rows == 0) return GS_OK;
  const hipStream_t s = (hipStream_t)stream;
  DoorFold f = {};
  f.cells.n1 = n1; f.cells.n2 = n2; f.cells.size = size; f.cells.sum = (unsigned long long*)sum; f.cells.bbox = bbox;
  f.open = open; f.label = label; f.d2 = d2; f.n0 = n0;
  f.room_lo = room_lo; f.room_hi = room_hi; f.widest = widest;
  GS_TIMING_PRE();
  room_table_init_kernel<<<gs_cdiv(rows, FR_THREADS), FR_THREADS, 0, s>>>(rows, size, f.cells.sum, bbox, nullptr, nullptr,
                                                                          room_lo, room_hi, widest);
  GS_CHECK_LAUNCH("room_door_table_init");
  room_door_table_kernel<<<fr_blocks(n0, n1, n2), FR_THREADS, 0, s>>>(door_label, n0 * n1 * n2, root, rows, f);
  GS_CHECK_LAUNCH("room_door_table");
  return GS_OK;
}
