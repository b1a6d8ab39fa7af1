// Elevation and traversability map of the state lattice of esdf.hip: where a ground robot can stand and roll (no
// counterpart in the reference).  Contract: include/goslam_hip.h (gs_floor_*); tests/floor_restatement.py restates it
// serially; DESIGN.md section 35.  Integer arithmetic only, no atomics, no waiting between workgroups: every column of
// either map is owned by one lane, so nothing depends on the launch geometry.
//
// gs_floor_columns is one launch, one walk per column from the cell under the band to the top of the headroom over it:
//   floor_columns_kernel<false>  up_axis 0 or 1: one lane per column, v along z, so the 64 lanes of a wave read a 64 B run
//                                per position; four positions are loaded before the first is looked at.
//   floor_columns_kernel<true>   up_axis 2: a column is a run along z and 64 columns are 64 rows nz bytes apart.  A wave
//                                takes 64 columns and brings 64 positions of each through LDS, one 64 B row per load with
//                                the lanes along z, then walks them with a lane per column (rows 68 B apart: the lanes'
//                                bytes lie on 17-dword strides, all banks differ).
// gs_floor_footprint is one launch: a 16 x 16 tile of columns per workgroup, floor and kind staged in LDS with a halo of
// floor(sqrt(R2)) cells (at most 80 x 80 x 3 bytes), the disc walked row by row.
#include "tsdf_cell.h"

namespace {

constexpr int FLOOR_THREADS = 256;
constexpr int FLOOR_CHUNK = 64;                      // positions per LDS tile row
constexpr int FLOOR_PITCH = FLOOR_CHUNK + 4;         // 17 dwords
constexpr int FLOOR_TILE = 16;
constexpr int FLOOR_R2_MAX = 32 * 32;
constexpr int FLOOR_HALO_MAX = 32;
constexpr int FLOOR_SPAN_MAX = FLOOR_TILE + 2 * FLOOR_HALO_MAX;

// The walk of one column, positions in increasing order from max(p0 - 1, 0).
struct FloorWalk {
  int cand = -1;        // the position over the last solid cell when it lies in the band, else -1
  int run = 0;          // non-solid cells seen from cand on
  int found = 0;        // 0 none yet, 1 strict, 2 maybe
  bool all_free = true, any_solid = false, any_unseen = false;
};

__device__ __forceinline__ void floor_step(FloorWalk& w, int s, int j, int p0, int p1, int H) {
  if (s == 2) {
    w.any_solid = true;
    w.cand = (j + 1 >= p0 && j + 1 <= p1) ? j + 1 : -1;
    w.run = 0;
    w.all_free = true;
    return;
  }
  w.any_unseen = w.any_unseen || s == 0;
  if (w.cand < 0) return;
  w.all_free = w.all_free && s == 1;
  if (++w.run >= H) w.found = w.all_free ? 1 : 2;      // run counts at most jend - jstart + 1 <= 1024 cells
}

// After the last position jend = min(p1 + H - 1, n_a - 1): a candidate that is still open ran into the lattice's top,
// whose cells beyond count as unseen.
__device__ __forceinline__ void floor_store(const FloorWalk& w, int n_a, int up_sign, short* __restrict__ floor,
                                            unsigned char* __restrict__ kind, int col) {
  int k = -1, kd;
  if (w.found != 0 || w.cand >= 0) {
    k = up_sign > 0 ? w.cand : n_a - 1 - w.cand;
    kd = w.found != 0 ? w.found : 2;
  } else {
    kd = (!w.any_solid && w.any_unseen) ? 0 : 3;
  }
  floor[col] = (short)k;
  kind[col] = (unsigned char)kd;
}

template <bool ALONG_Z>
__global__ __launch_bounds__(FLOOR_THREADS) void floor_columns_kernel(
    const unsigned char* __restrict__ state, int n_u, int n_v, int n_a, long long stride_u, long long stride_v,
    long long stride_a, int up_sign, int p0, int p1, int H, int jstart, int jend, short* __restrict__ floor,
    unsigned char* __restrict__ kind) {
  const int ncols = n_u * n_v;                                    // <= 2^20
  FloorWalk w;
  if (!ALONG_Z) {
    const int col = blockIdx.x * FLOOR_THREADS + threadIdx.x;
    if (col >= ncols) return;
    const int u = col / n_v, v = col - u * n_v;
    const unsigned char* at = state + (size_t)(u * stride_u + v * stride_v);
    for (int j = jstart; j <= jend && w.found == 0; j += 4) {
      int s[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int jj = min(j + i, jend);                          // a repeated load, never stepped
        s[i] = at[(size_t)((up_sign > 0 ? jj : n_a - 1 - jj) * stride_a)];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (j + i <= jend && w.found == 0) floor_step(w, s[i], j + i, p0, p1, H);
    }
    floor_store(w, n_a, up_sign, floor, kind, col);
  } else {
    // stride_a == 1 and column c is the n_a bytes at c * n_a
    __shared__ unsigned char tile[FLOOR_THREADS / 64][64 * FLOOR_PITCH];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col0 = blockIdx.x * FLOOR_THREADS + wave * 64;      // this wave's first column
    const int col = col0 + lane;
    const int rows = min(64, ncols - col0);                       // <= 0 for a wave past the end: it keeps the barriers
    unsigned char* mine = tile[wave];
    for (int jb = jstart; jb <= jend; jb += FLOOR_CHUNK) {
      const int jl = jb + lane;
      if (jl <= jend) {
        const int k = up_sign > 0 ? jl : n_a - 1 - jl;
        for (int r = 0; r < rows; ++r) mine[r * FLOOR_PITCH + lane] = state[(size_t)(col0 + r) * n_a + k];
      }
      __syncthreads();
      if (col < ncols) {
        const int top = min(FLOOR_CHUNK, jend - jb + 1);
        for (int i = 0; i < top && w.found == 0; ++i) floor_step(w, mine[lane * FLOOR_PITCH + i], jb + i, p0, p1, H);
      }
      // every column of the workgroup has its stand: nothing further up can change it
      if (__syncthreads_and(col >= ncols || w.found != 0)) break;
    }
    if (col < ncols) floor_store(w, n_a, up_sign, floor, kind, col);
  }
}

__global__ __launch_bounds__(FLOOR_THREADS) void floor_footprint_kernel(
    const short* __restrict__ floor, const unsigned char* __restrict__ kind, int n_u, int n_v, int R2, int r, int S,
    unsigned char* __restrict__ cells, unsigned char* __restrict__ why, short* __restrict__ rough) {
  __shared__ short fl[FLOOR_SPAN_MAX * FLOOR_SPAN_MAX];
  __shared__ unsigned char kd[FLOOR_SPAN_MAX * FLOOR_SPAN_MAX];
  const int span = FLOOR_TILE + 2 * r;                            // r <= FLOOR_HALO_MAX
  const int u0 = blockIdx.y * FLOOR_TILE - r, v0 = blockIdx.x * FLOOR_TILE - r;
  for (int i = threadIdx.x; i < span * span; i += FLOOR_THREADS) {
    const int hu = i / span, hv = i - hu * span;
    const int u = u0 + hu, v = v0 + hv;
    const bool in = u >= 0 && u < n_u && v >= 0 && v < n_v;       // a column outside the map is kind 0
    fl[i] = in ? floor[(size_t)u * n_v + v] : (short)-1;
    kd[i] = in ? kind[(size_t)u * n_v + v] : (unsigned char)0;
  }
  __syncthreads();
  const int tu = threadIdx.x >> 4, tv = threadIdx.x & 15;
  const int u = u0 + r + tu, v = v0 + r + tv;
  if (u >= n_u || v >= n_v) return;
  const int centre = (tu + r) * span + tv + r;
  const int kc = kd[centre], fc = fl[centre];
  int out_cells, out_why = 0, worst = 0;
  if (kc == 3) {
    out_cells = 0; out_why = 1;
  } else if (kc == 0) {
    out_cells = 205;
  } else {
    bool any_blocked = false, any_unsure = kc == 2;
    for (int du = -r; du <= r; ++du) {
      const int rem = R2 - du * du;                               // >= 0 since r * r <= R2
      int wd = r;
      while (wd * wd > rem) --wd;
      const int row = centre + du * span;
      for (int dv = -wd; dv <= wd; ++dv) {
        const int kq = kd[row + dv];
        any_blocked = any_blocked || kq == 3;
        any_unsure = any_unsure || kq == 0 || kq == 2;
        if (kq == 1 || kq == 2) {
          const int d = fl[row + dv] - fc;
          worst = max(worst, d < 0 ? -d : d);
        }
      }
    }
    if (any_blocked) { out_cells = 0; out_why = 2; }
    else if (worst > S) { out_cells = 0; out_why = 3; }
    else out_cells = any_unsure ? 205 : 254;
  }
  const size_t at = (size_t)u * n_v + v;
  cells[at] = (unsigned char)out_cells;
  why[at] = (unsigned char)out_why;
  rough[at] = (short)worst;
}

}  // namespace

extern "C" int gs_floor_columns(const unsigned char* state, int nx, int ny, int nz, int up_axis, int up_sign, int p0,
                                int p1, int H, short* floor, unsigned char* kind, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "floor_columns: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(up_axis >= 0 && up_axis <= 2, "floor_columns: up_axis=%d outside 0..2", up_axis);
  GS_REQUIRE(up_sign == 1 || up_sign == -1, "floor_columns: up_sign=%d is not +1 or -1", up_sign);
  const int n[3] = {nx, ny, nz};
  const long long stride[3] = {(long long)ny * nz, (long long)nz, 1};
  const int n_a = n[up_axis];
  GS_REQUIRE(p0 >= 0 && p0 <= p1 && p1 < n_a, "floor_columns: band [%d, %d] outside [0, %d) of axis %d", p0, p1, n_a,
             up_axis);
  GS_REQUIRE(H >= 1, "floor_columns: headroom H=%d cells is below 1", H);
  GS_REQUIRE(state && floor && kind, "floor_columns: null pointer");
  const int au = up_axis == 0 ? 1 : 0, av = up_axis == 2 ? 1 : 2;
  const int jstart = p0 > 0 ? p0 - 1 : 0;
  const long long top = (long long)p1 + H - 1;
  const int jend = top < n_a - 1 ? (int)top : n_a - 1;
  const int blocks = gs_cdiv(n[au] * n[av], FLOOR_THREADS);
  GS_TIMING_PRE();
  if (up_axis == 2)
    floor_columns_kernel<true><<<blocks, FLOOR_THREADS, 0, (hipStream_t)stream>>>(
        state, n[au], n[av], n_a, stride[au], stride[av], stride[up_axis], up_sign, p0, p1, H, jstart, jend, floor, kind);
  else
    floor_columns_kernel<false><<<blocks, FLOOR_THREADS, 0, (hipStream_t)stream>>>(
        state, n[au], n[av], n_a, stride[au], stride[av], stride[up_axis], up_sign, p0, p1, H, jstart, jend, floor, kind);
  GS_CHECK_LAUNCH("floor_columns");
  return GS_OK;
}

extern "C" int gs_floor_footprint(const short* floor, const unsigned char* kind, int n_u, int n_v, int R2, int S,
                                  unsigned char* cells, unsigned char* why, short* rough, gs_stream_t stream) {
  GS_REQUIRE(n_u >= 2 && n_u <= TSDF_DIM_MAX && n_v >= 2 && n_v <= TSDF_DIM_MAX, "floor_footprint: map %d x %d outside [2, 1024]",
             n_u, n_v);
  GS_REQUIRE(R2 >= 2 && R2 <= FLOOR_R2_MAX, "floor_footprint: R2=%d outside [2, %d]", R2, FLOOR_R2_MAX);
  GS_REQUIRE(S >= 0, "floor_footprint: S=%d is negative", S);
  GS_REQUIRE(floor && kind && cells && why && rough, "floor_footprint: null pointer");
  int r = 1;
  while ((r + 1) * (r + 1) <= R2) ++r;                            // floor(sqrt(R2)) <= FLOOR_HALO_MAX
  GS_TIMING_PRE();
  floor_footprint_kernel<<<dim3(gs_cdiv(n_v, FLOOR_TILE), gs_cdiv(n_u, FLOOR_TILE)), FLOOR_THREADS, 0,
                           (hipStream_t)stream>>>(floor, kind, n_u, n_v, R2, r, S, cells, why, rough);
  GS_CHECK_LAUNCH("floor_footprint");
  return GS_OK;
}
