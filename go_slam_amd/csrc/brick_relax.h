// What geodesic.hip (cost to go) and frontier.hip (component labels) share: one value per cell of a lattice, lowered in
// place to the fixed point of "a cell takes the best its 26 neighbours offer", brick by brick.
//
// A sweep is one launch, one workgroup per brick of B0 x B1 x B2 cells; the host enqueues sweeps until one lowers
// nothing (brick_relax_enqueue).  A brick whose dirty flag is clear leaves after one byte load.  A dirty one loads its
// values and a one-cell halo into LDS (the tile), prepares its cells, and lowers them inside LDS -- every cell owned by
// one lane, Brick::PER cells per lane, one barrier per round -- until a round lowers nothing or Brick::ROUNDS rounds
// have run.  Only lowered cells are written back.  A brick that lowered a cell marks, in the next sweep's flag buffer,
// the bricks that read that cell, marks itself when it ran out of rounds, and stores 1 to changed[s].  It clears its
// own byte of the buffer it read, which makes that buffer the clean "next" buffer of the following sweep.
//
// Why the fixed point is reached whatever the order, given a rule whose stored values are all valid (each file says why
// its own are):
//   values only fall -- a cell is written by its owner alone and only with a smaller value -- so a value read late or
//     twice is an upper bound of the one it would read now, and lowering from it is lowering from a valid value;
//   nothing waits for another workgroup.  A halo value read while its owner lowers it is stale, which only postpones
//     that improvement: the owner lowered a cell this brick reads, so it marks this brick for the next sweep, and the
//     kernel boundary between the sweeps makes the stored value visible;
//   inside a brick a neighbour reads the old or the new value of a cell lowered in the same round; a round that lowered
//     something is followed by another, and a brick whose rounds ran out marks itself, so no improvement is dropped;
//   the marks, written by lanes 0..26, one per brick of the 3 x 3 x 3 neighbourhood: the brick at +d reads, of this
//     one, the cells that lie on every face d names.  face[] records on which of the six faces a lowered cell lies, so
//     a lowered cell among those cells has set all of d's faces and that brick is marked.  The converse need not hold
//     (different cells may have set the faces): a brick marked in vain loads its tile, lowers nothing, marks nobody;
//   a sweep that lowers nothing has found every dirty brick at rest and marks none: changed[s] == 0 is the fixed point.
// lowered[], "did round r lower anything", takes one barrier per round with three slots: round r stores 1 to slot r % 3
// before barrier r and reads that slot after it; lane 0 then clears slot (r + 2) % 3, which was last read between
// barriers r - 1 and r and is next written in round r + 2, after barrier r + 1, which lane 0 reaches after its clear.
// With two slots that clear would fall between the same two barriers as round r + 1's stores to the slot.
// Every store to a flag, to changed[s], to lowered[] and to face[] writes the same value as every other store to that
// byte or word in the launch, so none is atomic.
#pragma once
#include "common.h"

namespace {

constexpr int BRICK_MAX_CELLS = 1024;                      // cells per axis of a lattice

template <int B0_, int B1_, int B2_, int ROUNDS_, int THREADS_ = 256>
struct Brick {
  static constexpr int B0 = B0_, B1 = B1_, B2 = B2_;
  static constexpr int ROUNDS = ROUNDS_;                   // rounds inside LDS per sweep
  static constexpr int THREADS = THREADS_;
  static constexpr int CELLS = B0 * B1 * B2;
  static constexpr int PER = CELLS / THREADS;              // cells per lane
  static constexpr int T0 = B0 + 2, T1 = B1 + 2, T2 = B2 + 2;      // the tile: the brick and its halo
  static constexpr int TILE = T0 * T1 * T2;
  static_assert(CELLS % THREADS == 0, "a lane owns a whole number of cells");
  __host__ __device__ static constexpr int tile_offset(int e0, int e1, int e2) { return (e0 * T1 + e1) * T2 + e2; }
  // neighbour m of 26 -> index 0..26 of the 3 x 3 x 3 neighbourhood (the centre, 13, is skipped), and its tile offset
  __host__ __device__ static constexpr int nb(int m) { return m < 13 ? m : m + 1; }
  __host__ __device__ static constexpr int nb_offset(int m) {
    return tile_offset(nb(m) / 9 - 1, nb(m) / 3 % 3 - 1, nb(m) % 3 - 1);
  }
};

// One sweep's work on brick blockIdx.x.  cur / next: this sweep's and the next sweep's flag buffer.  The rule, a plain
// struct passed by value, supplies what a cell holds and how it falls:
//   Value                          the unsigned or signed 32-bit type of a cell; smaller is better
//   Cell                           what a lane keeps per cell between prepare and lower (may be empty)
//   Value load(at, inside, q)      tile entry q from global offset `at` (0 when !inside: readable, to be ignored); the
//                                  value outside the lattice is one that never lowers a neighbour
//   Value prepare(tile, at, v, cell)  after the tile is complete: the value the cell at tile offset `at` starts with
//                                  (v or lower; a lower one is also stored to the tile) and its Cell
//   bool active(v, cell)           whether the cell can fall at all (the skeleton skips the others: their 26 tile reads
//                                  and, in the compiled code, a second pass through the execution mask per cell)
//   Value lower(tile, at, v, cell) one relaxation of an active cell from the tile: the new value, or v if nothing fell
//   void store(at, v)              the global store of a lowered cell
template <class Brick, class Rule>
__device__ __forceinline__ void brick_relax(Rule rule, int n0, int n1, int n2, int nb0, int nb1, int nb2,
                                            unsigned char* cur, unsigned char* next, unsigned int* changed) {
  using Value = typename Rule::Value;
  constexpr int B0 = Brick::B0, B1 = Brick::B1, B2 = Brick::B2, T1 = Brick::T1, T2 = Brick::T2;
  constexpr int PER = Brick::PER, THREADS = Brick::THREADS;
  __shared__ Value tile[Brick::TILE];
  __shared__ int lowered[3];                                // round r stores to [r % 3]
  __shared__ int face[6];                                   // a cell with index 0 / B - 1 along axis a fell: [2a] / [2a + 1]
  const int tid = threadIdx.x;
  const int brick = blockIdx.x;
  if (cur[brick] == 0) return;                              // written before this launch: every lane reads the same
  const int i2 = brick % nb2, i1 = brick / nb2 % nb1, i0 = brick / nb2 / nb1;
  const int base0 = i0 * B0 - 1, base1 = i1 * B1 - 1, base2 = i2 * B2 - 1;     // the tile's corner, a halo cell

  if (tid < 3) lowered[tid] = 0;
  if (tid < 6) face[tid] = 0;
  for (int q = tid; q < Brick::TILE; q += THREADS) {
    const int t0 = q / (T1 * T2), r = q - t0 * (T1 * T2), t1 = r / T2, t2 = r - t1 * T2;
    const int g0 = base0 + t0, g1 = base1 + t1, g2 = base2 + t2;
    const bool inside = g0 >= 0 && g0 < n0 && g1 >= 0 && g1 < n1 && g2 >= 0 && g2 < n2;
    const size_t at = inside ? ((size_t)g0 * n1 + g1) * n2 + g2 : 0;
    tile[q] = rule.load(at, inside, q);
  }
  __syncthreads();
  if (tid == 0) cur[brick] = 0;                             // after the barrier: every wave has read the flag

  int at[PER];
  Value val[PER], was[PER];
  typename Rule::Cell cell[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int q = tid + THREADS * j;
    const int z = q % B2, y = q / B2 % B1, x = q / (B1 * B2);
    at[j] = Brick::tile_offset(x + 1, y + 1, z + 1);
    was[j] = tile[at[j]];
    val[j] = rule.prepare(tile, at[j], was[j], cell[j]);
  }

  int round = 0;
  bool more;
  do {
    bool fell = false;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (!rule.active(val[j], cell[j])) continue;
      const Value best = rule.lower(tile, at[j], val[j], cell[j]);
      if (best < val[j]) {
        val[j] = best;
        tile[at[j]] = best;                                 // a neighbour reads the old or the new value: both are valid
        fell = true;
      }
    }
    if (fell) lowered[round % 3] = 1;
    __syncthreads();
    more = lowered[round % 3] != 0;
    if (tid == 0) lowered[(round + 2) % 3] = 0;             // last read before this barrier, next written after the next
    ++round;
  } while (more && round < Brick::ROUNDS);

  bool any = false;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (val[j] >= was[j]) continue;
    const int q = tid + THREADS * j;
    const int z = q % B2, y = q / B2 % B1, x = q / (B1 * B2);
    // inside the lattice: an outside cell holds a value that nothing lowers
    rule.store(((size_t)(base0 + 1 + x) * n1 + (base1 + 1 + y)) * n2 + (base2 + 1 + z), val[j]);
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
    bool mark = (d0 == 0 || face[d0 < 0 ? 0 : 1] != 0) && (d1 == 0 || face[d1 < 0 ? 2 : 3] != 0) &&
                (d2 == 0 || face[d2 < 0 ? 4 : 5] != 0);
    if (tid == 13) mark = more;                             // itself: only when the rounds ran out
    if (mark && j0 >= 0 && j0 < nb0 && j1 >= 0 && j1 < nb1 && j2 >= 0 && j2 < nb2)
      next[((size_t)j0 * nb1 + j1) * nb2 + j2] = 1;
  }
}

bool brick_dims_ok(int n0, int n1, int n2) {
  return n0 >= 1 && n0 <= BRICK_MAX_CELLS && n1 >= 1 && n1 <= BRICK_MAX_CELLS && n2 >= 1 && n2 <= BRICK_MAX_CELLS;
}

// the two flag buffers, one byte per brick each; 0 for sizes outside [1, 1024]
template <class Brick>
size_t brick_flags_bytes(int n0, int n1, int n2) {
  if (!brick_dims_ok(n0, n1, n2)) return 0;
  return (size_t)2 * gs_cdiv(n0, Brick::B0) * gs_cdiv(n1, Brick::B1) * gs_cdiv(n2, Brick::B2);
}

// Sweeps sweep0 .. sweep0 + k - 1: changed[0..k) cleared, then launch(cur, next, changed + i) once per sweep, sweep s
// reading flag buffer s & 1 and writing the other.  `name` is the timer's and the error texts' name of the launch.
template <class Launch>
int brick_relax_enqueue(const char* name, size_t nbricks, unsigned char* flags, int sweep0, int k,
                        unsigned int* changed, hipStream_t s, Launch launch) {
  if (hipMemsetAsync(changed, 0, sizeof(unsigned int) * (size_t)k, s) != hipSuccess) {
    gs_set_error("%s: clearing changed[%d] failed", name, k);
    return GS_ERR_LAUNCH;
  }
  GS_TIMING_PRE();
  for (int i = 0; i < k; ++i) {
    const int parity = (sweep0 + i) & 1;
    launch(flags + parity * nbricks, flags + (parity ^ 1) * nbricks, changed + i);
    GS_CHECK_LAUNCH(name);
  }
  return GS_OK;
}

}  // namespace
