// Exact nearest neighbours between fp64 point clouds and the ICP moments over their correspondences: the KD-tree
// queries of eval_mesh (reference src/mesher.py:390-421, scipy cKDTree) and the hybrid search inside Open3D's
// registration_icp (align_mesh, src/mesher.py:339-357).  Contracts: include/goslam_neus.h (gs_nn_*, gs_icp_moments).
#include "neus_common.h"

#include <math.h>

namespace {

constexpr int NN_BLOCK = 256;
constexpr int NN_TILE = 256;                 // reference points per LDS tile of the brute-force fallback
constexpr int MOM_BLOCK = 256;
constexpr int MOM_ITEMS = 8;                 // correspondences per thread per moment tile
constexpr int MOM_TILE = MOM_BLOCK * MOM_ITEMS;

struct NNGrid {
  double lo[3];
  double h;
  double scale;                              // max |coordinate| of the box + h: sets the bound's slack
  int n[3];
};

__device__ __forceinline__ void xform(const double* __restrict__ T, const double p[3], double o[3]) {
  for (int r = 0; r < 3; ++r)
    o[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T[4 * r], p[0]), __dmul_rn(T[4 * r + 1], p[1])),
                               __dmul_rn(T[4 * r + 2], p[2])), T[4 * r + 3]);
}

// the contract's d2: dx*dx + dy*dy + dz*dz, left to right, every operation rounded
__device__ __forceinline__ double dist2(const double a[3], double x, double y, double z) {
  const double dx = __dsub_rn(a[0], x), dy = __dsub_rn(a[1], y), dz = __dsub_rn(a[2], z);
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

__device__ __forceinline__ void load_query(const double* __restrict__ q, int i, const double* __restrict__ T,
                                           double p[3]) {
  const double a[3] = {q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2]};
  if (T) {
    xform(T, a, p);
  } else {
    p[0] = a[0]; p[1] = a[1]; p[2] = a[2];
  }
}

__device__ __forceinline__ double cell_coord(const NNGrid& g, double p, int d) {
  return floor(__ddiv_rn(__dsub_rn(p, g.lo[d]), g.h));
}

__global__ __launch_bounds__(NN_BLOCK) void nn_keys_kernel(const double* __restrict__ pts, int n, NNGrid g,
                                                           int* __restrict__ keys) {
  const int i = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i >= n) return;
  int c[3];
  for (int d = 0; d < 3; ++d) {
    const double f = cell_coord(g, pts[3 * (size_t)i + d], d);
    c[d] = f <= 0.0 ? 0 : (f >= (double)(g.n[d] - 1) ? g.n[d] - 1 : (int)f);   // NaN lands in cell 0
  }
  keys[i] = (c[2] * g.n[1] + c[1]) * g.n[0] + c[0];
}

// cell_start[c] = the first sorted position whose key is >= c, for c in [0, n_cells]
__global__ __launch_bounds__(NN_BLOCK) void nn_cell_start_kernel(const int* __restrict__ skeys, int n, int n_cells,
                                                                 int* __restrict__ cell_start) {
  const int c = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (c > n_cells) return;
  int a = 0, b = n;
  while (a < b) {
    const int m = (a + b) >> 1;
    if (skeys[m] < c) a = m + 1; else b = m;
  }
  cell_start[c] = a;
}

__global__ __launch_bounds__(NN_BLOCK) void nn_gather_kernel(const double* __restrict__ pts, const int64_t* __restrict__ perm,
                                                             int n, double* __restrict__ spts, int* __restrict__ sidx) {
  const int i = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int j = (int)perm[i];
  spts[3 * (size_t)i] = pts[3 * (size_t)j];
  spts[3 * (size_t)i + 1] = pts[3 * (size_t)j + 1];
  spts[3 * (size_t)i + 2] = pts[3 * (size_t)j + 2];
  sidx[i] = j;
}

__device__ __forceinline__ long long clip_len(long long a, long long b) { return b >= a ? b - a + 1 : 0; }

// One lane per query: rings of growing Chebyshev radius k around the query's (unclamped) cell, starting at the first
// ring that meets the grid.  After ring k every unvisited point lies outside the block [c - k, c + k] (clipped to the
// grid), so its distance is at least the distance from the query to the nearest block face that has cells beyond it;
// that bound, shrunk by a slack far above fp64 rounding, ends the search once best d2 < bound^2.  A query whose next
// ring would take it past `budget` visited cells is appended to the fallback list.
__global__ __launch_bounds__(NN_BLOCK) void nn_grid_query_kernel(
    const double* __restrict__ spts, const int* __restrict__ sidx, const int* __restrict__ cell_start, NNGrid g,
    const double* __restrict__ q, int m, const double* __restrict__ T, double r2, long long budget,
    double* __restrict__ out_d2, int* __restrict__ out_idx, int* __restrict__ fb_list, int* __restrict__ fb_count) {
  const int i = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i >= m) return;
  double p[3];
  load_query(q, i, T, p);
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
    out_d2[i] = INFINITY;
    out_idx[i] = -1;
    return;
  }
  constexpr double CMAX = 1099511627776.0;     // 2^40: keeps far-away cell coordinates exact in int64
  long long c[3], k0 = 0;
  for (int d = 0; d < 3; ++d) {
    const double f = fmin(fmax(cell_coord(g, p[d], d), -CMAX), CMAX);
    c[d] = (long long)f;
    const long long out = c[d] < 0 ? -c[d] : (c[d] > g.n[d] - 1 ? c[d] - (g.n[d] - 1) : 0);
    k0 = out > k0 ? out : k0;
  }
  const double slack = 1e-9 * (g.scale + fabs(p[0]) + fabs(p[1]) + fabs(p[2]));
  double best = INFINITY;
  int bi = -1;
  long long visited = 0;
  for (long long k = k0;; ++k) {
    long long bl[3], bh[3], inner = 1, outer = 1;
    for (int d = 0; d < 3; ++d) {
      bl[d] = c[d] - k > 0 ? c[d] - k : 0;
      bh[d] = c[d] + k < g.n[d] - 1 ? c[d] + k : g.n[d] - 1;
      outer *= clip_len(bl[d], bh[d]);
      const long long il = c[d] - k + 1 > 0 ? c[d] - k + 1 : 0;
      const long long ih = c[d] + k - 1 < g.n[d] - 1 ? c[d] + k - 1 : g.n[d] - 1;
      inner *= k > 0 ? clip_len(il, ih) : 0;
    }
    if (visited + (outer - inner) > budget) {
      fb_list[atomicAdd(fb_count, 1)] = i;
      return;
    }
    visited += outer - inner;
    for (long long z = bl[2]; z <= bh[2]; ++z) {
      for (long long y = bl[1]; y <= bh[1]; ++y) {
        const bool shell = (z == c[2] - k || z == c[2] + k || y == c[1] - k || y == c[1] + k);
        const int row = (int)((z * g.n[1] + y) * g.n[0]);
        // a shell row is one contiguous run of cells; an interior row has only its two end cells on the ring
        for (int part = 0; part < (shell ? 1 : 2); ++part) {
          long long x0, x1;
          if (shell) {
            x0 = bl[0]; x1 = bh[0];
          } else {
            x0 = x1 = part == 0 ? c[0] - k : c[0] + k;
            if (x0 < 0 || x0 > g.n[0] - 1) continue;
          }
          const int s = cell_start[row + (int)x0], e = cell_start[row + (int)x1 + 1];
          for (int j = s; j < e; ++j) {
            const double d2 = dist2(p, spts[3 * (size_t)j], spts[3 * (size_t)j + 1], spts[3 * (size_t)j + 2]);
            const int id = sidx[j];
            if (d2 < best || (d2 == best && id < bi)) {
              best = d2;
              bi = id;
            }
          }
        }
      }
    }
    double lb = INFINITY;
    for (int d = 0; d < 3; ++d) {
      if (c[d] - k > 0) lb = fmin(lb, __dsub_rn(p[d], __dadd_rn(g.lo[d], __dmul_rn((double)(c[d] - k), g.h))));
      if (c[d] + k < g.n[d] - 1) lb = fmin(lb, __dsub_rn(__dadd_rn(g.lo[d], __dmul_rn((double)(c[d] + k + 1), g.h)), p[d]));
    }
    if (lb == INFINITY) break;                     // the block covers the whole grid
    const double l = __dsub_rn(lb, slack);
    const double lb2 = l > 0.0 ? __dmul_rn(__dmul_rn(l, l), 1.0 - 1e-12) : 0.0;
    if (best < lb2) break;
    if (r2 >= 0.0 && lb2 >= r2) break;             // nothing unvisited can be within range
  }
  if (r2 >= 0.0 && !(best < r2)) {
    best = INFINITY;
    bi = -1;
  }
  out_d2[i] = best;
  out_idx[i] = bi;
}

// The fallback: each listed query scans every reference point in ascending index order (strict < keeps the smallest
// index of a tie), the points streamed through LDS in tiles shared by the workgroup's 256 queries.  Launched over the
// worst-case list length; workgroups past the device-side count return at once.
__global__ __launch_bounds__(NN_BLOCK) void nn_brute_kernel(const double* __restrict__ ref, int n,
                                                            const double* __restrict__ q, const double* __restrict__ T,
                                                            const int* __restrict__ fb_list, const int* __restrict__ fb_count,
                                                            double r2, double* __restrict__ out_d2, int* __restrict__ out_idx) {
  __shared__ double tx[NN_TILE], ty[NN_TILE], tz[NN_TILE];
  const int cnt = *fb_count;
  const int base = blockIdx.x * NN_BLOCK;
  if (base >= cnt) return;                         // uniform across the workgroup
  const int slot = base + threadIdx.x;
  const bool act = slot < cnt;
  const int qi = act ? fb_list[slot] : 0;
  double p[3] = {0.0, 0.0, 0.0};
  if (act) load_query(q, qi, T, p);
  double best = INFINITY;
  int bi = -1;
  for (int t0 = 0; t0 < n; t0 += NN_TILE) {
    const int j = t0 + threadIdx.x;
    if (j < n) {
      tx[threadIdx.x] = ref[3 * (size_t)j];
      ty[threadIdx.x] = ref[3 * (size_t)j + 1];
      tz[threadIdx.x] = ref[3 * (size_t)j + 2];
    }
    __syncthreads();
    const int len = n - t0 < NN_TILE ? n - t0 : NN_TILE;
    for (int jj = 0; jj < len; ++jj) {
      const double d2 = dist2(p, tx[jj], ty[jj], tz[jj]);
      if (d2 < best) {
        best = d2;
        bi = t0 + jj;
      }
    }
    __syncthreads();
  }
  if (!act) return;
  if (r2 >= 0.0 && !(best < r2)) {
    best = INFINITY;
    bi = -1;
  }
  out_d2[qi] = best;
  out_idx[qi] = bi;
}

// ------------------------------------------------------------------------------------------- ICP moments -----------
// Pass 1 sums (count, d2, source xyz, target xyz) over the correspondences (index >= 0) of each MOM_TILE tile; pass 2
// adds the tiles' sums in tile order and writes count, sum d2 and both centroids; pass 3 sums the centred products
// (t - t_mean)(s - s_mean)^T per tile; pass 4 adds those in tile order.  Within a tile: each thread sums its items in
// ascending order, then a fixed tree over the 256 threads.
template <int NV>
__device__ __forceinline__ void block_tree(double (*red)[MOM_BLOCK], double v[NV]) {
  for (int a = 0; a < NV; ++a) red[a][threadIdx.x] = v[a];
  __syncthreads();
  for (int w = MOM_BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int a = 0; a < NV; ++a) red[a][threadIdx.x] += red[a][threadIdx.x + w];
    __syncthreads();
  }
}

__global__ __launch_bounds__(MOM_BLOCK) void icp_sums_kernel(const double* __restrict__ src, int n,
                                                             const double* __restrict__ T, const double* __restrict__ tgt,
                                                             const int* __restrict__ idx, const double* __restrict__ d2,
                                                             const double* __restrict__ means, double* __restrict__ part) {
  // means == NULL: the first-order sums (8 values); otherwise the centred cross products (9 values), means = the source
  // centroid then the target centroid
  __shared__ double red[9][MOM_BLOCK];
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int base = blockIdx.x * MOM_TILE;
  for (int it = 0; it < MOM_ITEMS; ++it) {
    const int i = base + it * MOM_BLOCK + threadIdx.x;
    if (i >= n) break;
    const int j = idx[i];
    if (j < 0) continue;
    double s[3];
    load_query(src, i, T, s);
    const double t[3] = {tgt[3 * (size_t)j], tgt[3 * (size_t)j + 1], tgt[3 * (size_t)j + 2]};
    if (!means) {
      v[0] += 1.0;
      v[1] += d2[i];
      for (int a = 0; a < 3; ++a) {
        v[2 + a] += s[a];
        v[5 + a] += t[a];
      }
    } else {
      for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc)
          v[3 * r + cc] += __dmul_rn(__dsub_rn(t[r], means[3 + r]), __dsub_rn(s[cc], means[cc]));
    }
  }
  block_tree<9>(red, v);
  if (threadIdx.x == 0)
    for (int a = 0; a < (means ? 9 : 8); ++a) part[(size_t)blockIdx.x * 9 + a] = red[a][0];
}

__global__ __launch_bounds__(MOM_BLOCK) void icp_final_kernel(const double* __restrict__ part, int nblk, int second,
                                                              double* __restrict__ out) {
  __shared__ double red[9][MOM_BLOCK];
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nblk; b += MOM_BLOCK)
    for (int a = 0; a < 9; ++a) v[a] += part[(size_t)b * 9 + a];
  block_tree<9>(red, v);
  if (threadIdx.x != 0) return;
  if (!second) {
    const double cnt = red[0][0];
    out[0] = cnt;
    out[1] = red[1][0];
    for (int a = 0; a < 6; ++a) out[2 + a] = cnt > 0.0 ? red[2 + a][0] / cnt : 0.0;
  } else {
    for (int a = 0; a < 9; ++a) out[8 + a] = red[a][0];
  }
}

NNGrid make_grid(const double* grid_host, const int* dims_host) {
  NNGrid g;
  for (int d = 0; d < 3; ++d) {
    g.lo[d] = grid_host[d];
    g.n[d] = dims_host[d];
  }
  g.h = grid_host[3];
  g.scale = grid_host[4];
  return g;
}

bool grid_ok(const double* grid_host, const int* dims_host, long long* cells) {
  if (!grid_host || !dims_host) return false;
  long long c = 1;
  for (int d = 0; d < 3; ++d) {
    if (dims_host[d] < 1 || !isfinite(grid_host[d])) return false;
    c *= dims_host[d];
    if (c > GS_NN_MAX_CELLS) return false;
  }
  *cells = c;
  return isfinite(grid_host[3]) && grid_host[3] > 0.0 && isfinite(grid_host[4]) && grid_host[4] >= 0.0;
}

}  // namespace

extern "C" int gs_nn_cell_keys(const double* points, int n_points, const double* grid_host, const int* dims_host,
                               int* keys, gs_stream_t stream) {
  long long cells = 0;
  GS_REQUIRE(n_points >= 0 && grid_ok(grid_host, dims_host, &cells), "nn_cell_keys: bad grid or point count");
  if (n_points == 0) return GS_OK;
  GS_REQUIRE(points && keys, "nn_cell_keys: null pointer");
  GS_TIMING_PRE();
  nn_keys_kernel<<<gs_cdiv(n_points, NN_BLOCK), NN_BLOCK, 0, (hipStream_t)stream>>>(points, n_points,
                                                                                   make_grid(grid_host, dims_host), keys);
  GS_CHECK_LAUNCH("nn_cell_keys");
  return GS_OK;
}

extern "C" int gs_nn_grid_build(const double* points, int n_points, const int* sorted_keys, const int64_t* perm,
                                const int* dims_host, int* cell_start, double* sorted_points, int* sorted_index,
                                gs_stream_t stream) {
  GS_REQUIRE(n_points >= 0 && dims_host, "nn_grid_build: bad arguments");
  long long cells = 1;
  for (int d = 0; d < 3; ++d) {
    GS_REQUIRE(dims_host[d] >= 1, "nn_grid_build: bad grid dimensions");
    cells *= dims_host[d];
  }
  GS_REQUIRE(cells <= GS_NN_MAX_CELLS, "nn_grid_build: %lld cells exceed %d", cells, GS_NN_MAX_CELLS);
  GS_REQUIRE(cell_start && (n_points == 0 || (points && sorted_keys && perm && sorted_points && sorted_index)),
             "nn_grid_build: null pointer");
  hipStream_t st = (hipStream_t)stream;
  GS_TIMING_PRE();
  nn_cell_start_kernel<<<gs_cdiv((int)cells + 1, NN_BLOCK), NN_BLOCK, 0, st>>>(sorted_keys, n_points, (int)cells,
                                                                               cell_start);
  GS_CHECK_LAUNCH("nn_cell_start");
  if (n_points > 0) {
    nn_gather_kernel<<<gs_cdiv(n_points, NN_BLOCK), NN_BLOCK, 0, st>>>(points, perm, n_points, sorted_points,
                                                                       sorted_index);
    GS_CHECK_LAUNCH("nn_gather");
  }
  return GS_OK;
}

extern "C" size_t gs_nn_query_workspace_bytes(int n_queries) {
  if (n_queries < 0) return 0;
  return (size_t)(n_queries + 1) * sizeof(int);
}

extern "C" int gs_nn_query(const double* points, const double* sorted_points, const int* sorted_index,
                           const int* cell_start, int n_points, const double* grid_host, const int* dims_host,
                           const double* queries, int n_queries, const double* transform, double max_distance,
                           double* d2, int* index, void* workspace, size_t workspace_bytes, gs_stream_t stream) {
  long long cells = 0;
  GS_REQUIRE(n_points >= 0 && n_queries >= 0 && grid_ok(grid_host, dims_host, &cells),
             "nn_query: bad grid or point counts");
  GS_REQUIRE(!(max_distance >= 0.0) || isfinite(max_distance), "nn_query: max_distance must be finite");
  if (n_queries == 0) return GS_OK;
  GS_REQUIRE(cell_start && queries && d2 && index && workspace &&
                 (n_points == 0 || (points && sorted_points && sorted_index)),
             "nn_query: null pointer");
  if (workspace_bytes < gs_nn_query_workspace_bytes(n_queries)) {
    gs_set_error("nn_query: workspace %zu < %zu bytes", workspace_bytes, gs_nn_query_workspace_bytes(n_queries));
    return GS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int* fb_count = (int*)workspace;
  int* fb_list = fb_count + 1;
  const double r2 = max_distance >= 0.0 ? max_distance * max_distance : -1.0;
  if (hipMemsetAsync(fb_count, 0, sizeof(int), st) != hipSuccess) {
    gs_set_error("nn_query: memset failed");
    return GS_ERR_LAUNCH;
  }
  const int nb = gs_cdiv(n_queries, NN_BLOCK);
  GS_TIMING_PRE();
  nn_grid_query_kernel<<<nb, NN_BLOCK, 0, st>>>(sorted_points, sorted_index, cell_start, make_grid(grid_host, dims_host),
                                                queries, n_queries, transform, r2, (long long)GS_NN_CELL_BUDGET, d2,
                                                index, fb_list, fb_count);
  GS_CHECK_LAUNCH("nn_grid_query");
  nn_brute_kernel<<<nb, NN_BLOCK, 0, st>>>(points, n_points, queries, transform, fb_list, fb_count, r2, d2, index);
  GS_CHECK_LAUNCH("nn_brute");
  return GS_OK;
}

extern "C" size_t gs_icp_moments_workspace_bytes(int n_source) {
  if (n_source < 0) return 0;
  return (size_t)(n_source > 0 ? gs_cdiv(n_source, MOM_TILE) : 1) * 9 * sizeof(double);
}

extern "C" int gs_icp_moments(const double* source, int n_source, const double* transform, const double* target,
                              const int* index, const double* d2, double* moments, void* workspace,
                              size_t workspace_bytes, gs_stream_t stream) {
  GS_REQUIRE(n_source >= 0, "icp_moments: bad point count");
  GS_REQUIRE(moments && workspace && (n_source == 0 || (source && target && index && d2)), "icp_moments: null pointer");
  if (workspace_bytes < gs_icp_moments_workspace_bytes(n_source)) {
    gs_set_error("icp_moments: workspace %zu < %zu bytes", workspace_bytes, gs_icp_moments_workspace_bytes(n_source));
    return GS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const int nblk = n_source > 0 ? gs_cdiv(n_source, MOM_TILE) : 0;
  GS_TIMING_PRE();
  if (nblk > 0) {
    icp_sums_kernel<<<nblk, MOM_BLOCK, 0, st>>>(source, n_source, transform, target, index, d2, nullptr, part);
    GS_CHECK_LAUNCH("icp_sums");
  }
  icp_final_kernel<<<1, MOM_BLOCK, 0, st>>>(part, nblk, 0, moments);
  GS_CHECK_LAUNCH("icp_means");
  if (nblk > 0) {
    icp_sums_kernel<<<nblk, MOM_BLOCK, 0, st>>>(source, n_source, transform, target, index, d2, moments + 2, part);
    GS_CHECK_LAUNCH("icp_cross");
  }
  icp_final_kernel<<<1, MOM_BLOCK, 0, st>>>(part, nblk, 1, moments);
  GS_CHECK_LAUNCH("icp_cross_final");
  return GS_OK;
}
