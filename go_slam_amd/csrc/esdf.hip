// Euclidean distance field and 2-D occupancy map of the TSDF lattice of tsdf.hip (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_esdf_*); tests/esdf_restatement.py restates it serially.  Integer arithmetic except
// for one sqrtf and one multiply per point; compiled with -ffp-contract=off.
//
// gs_esdf_build is four launches:
//   esdf_sites_z_kernel   one wave per z line (four lines per workgroup).  The line's states go to LDS and to `state`;
//                         the site stencil reads the z neighbours from LDS and the x / y neighbours' tsdf and weight
//                         from global memory (256 B runs); the start values (0 / INF) go to LDS and the z pass runs over
//                         them there.
//   esdf_pass_kernel      the y pass, then the x pass: one lane per lattice point, the 64 lanes of a wave along z as in
//                         tsdf.hip, so the loads at offset +-k along the axis are 256 B runs.  The x pass applies the FAR
//                         rule.
//   esdf_finish_kernel    dist from d2 and state, one lane per point.
// Every pass is the header's early-exit loop: bounded by R <= 1023 whatever the data holds.  `dist` is the int32
// ping-pong buffer (z -> d2, y -> dist, x -> d2, finish -> dist).  No atomics, no scratch; every point, query and map
// column is owned by one lane, so nothing depends on the launch geometry.
#include "tsdf_cell.h"

namespace {

constexpr int ESDF_THREADS = 256;
constexpr int ESDF_WAVES = ESDF_THREADS / 64;
constexpr int ESDF_MAX = 1024;              // lattice points per axis: sizes the LDS lines of esdf_sites_z_kernel
static_assert(ESDF_MAX == TSDF_DIM_MAX, "tsdf_dims_ok admits the lattices whose lines fit");
constexpr int ESDF_INF = 0x3fffffff;
constexpr int ESDF_FAR = 0x7fffffff;

__device__ __forceinline__ int esdf_state(float t, float w, float min_weight) {
  if (!(w >= min_weight)) return 0;
  return t < 0.0f ? 2 : 1;
}

// out[i] = min over |k| <= R, 0 <= i + k < n of in[i + k] + k * k, for the point at `idx` of a line of n values that
// are `stride` apart around `at`.  A term with k * k >= best cannot lower best, and best only falls: the loop may stop.
template <typename T>
__device__ __forceinline__ int esdf_line_min(const T* __restrict__ at, long long stride, int idx, int n, int radius) {
  int best = at[0];
  const int reach = max(idx, n - 1 - idx);                  // beyond it both i - k and i + k lie outside the line
  const int kmax = radius < reach ? radius : reach;
  for (int k = 1; k <= kmax && k * k < best; ++k) {
    const int kk = k * k;
    if (idx - k >= 0) best = min(best, at[-(long long)k * stride] + kk);
    if (idx + k < n) best = min(best, at[(long long)k * stride] + kk);
  }
  return best;
}

__global__ __launch_bounds__(ESDF_THREADS) void esdf_sites_z_kernel(
    const float* __restrict__ tsdf, const float* __restrict__ weight, int nx, int ny, int nz, float min_weight,
    int radius, unsigned char* __restrict__ state, int* __restrict__ out) {
  __shared__ int line[ESDF_WAVES][ESDF_MAX];
  __shared__ unsigned char st[ESDF_WAVES][ESDF_MAX];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * ESDF_WAVES + wave;            // nx * ny <= 2^20
  const bool live = row < nx * ny;                           // a dead wave only keeps the barriers' count
  const int i = row / ny, j = row - i * ny;
  const size_t base = (size_t)row * nz;
  const size_t sy = (size_t)nz, sx = (size_t)ny * nz;

  for (int k = lane; k < nz; k += 64) {
    if (!live) continue;
    const int s = esdf_state(tsdf[base + k], weight[base + k], min_weight);
    st[wave][k] = (unsigned char)s;
    state[base + k] = (unsigned char)s;
  }
  __syncthreads();
  for (int k = lane; k < nz; k += 64) {
    if (!live) continue;
    const int s = st[wave][k];
    bool site = false;
    if (s != 0) {
      int o;
      if (k > 0) { o = st[wave][k - 1]; site = site || (o != 0 && o != s); }
      if (k < nz - 1) { o = st[wave][k + 1]; site = site || (o != 0 && o != s); }
      const size_t at = base + k;
      if (j > 0) { o = esdf_state(tsdf[at - sy], weight[at - sy], min_weight); site = site || (o != 0 && o != s); }
      if (j < ny - 1) { o = esdf_state(tsdf[at + sy], weight[at + sy], min_weight); site = site || (o != 0 && o != s); }
      if (i > 0) { o = esdf_state(tsdf[at - sx], weight[at - sx], min_weight); site = site || (o != 0 && o != s); }
      if (i < nx - 1) { o = esdf_state(tsdf[at + sx], weight[at + sx], min_weight); site = site || (o != 0 && o != s); }
    }
    line[wave][k] = site ? 0 : ESDF_INF;
  }
  __syncthreads();
  for (int k = lane; k < nz; k += 64) {
    if (!live) continue;
    out[base + k] = esdf_line_min(&line[wave][k], 1, k, nz, radius);
  }
}

// AXIS 1: along y (stride nz), AXIS 0: along x (stride ny * nz) and the FAR rule
template <int AXIS>
__global__ __launch_bounds__(ESDF_THREADS) void esdf_pass_kernel(const int* __restrict__ in, int* __restrict__ out,
                                                                 int nx, int ny, int nz, int zchunks, long long nruns,
                                                                 int radius) {
  const long long run = (long long)blockIdx.x * ESDF_WAVES + (threadIdx.x >> 6);
  if (run >= nruns) return;
  const long long row = run / zchunks;
  const int zc = (int)(run - row * zchunks);
  const int k = zc * 64 + (threadIdx.x & 63);
  if (k >= nz) return;
  const int i = (int)(row / ny), j = (int)(row - (long long)i * ny);
  const size_t at = (size_t)row * nz + k;
  int best;
  if (AXIS == 1) {
    best = esdf_line_min(in + at, (long long)nz, j, ny, radius);
  } else {
    best = esdf_line_min(in + at, (long long)ny * nz, i, nx, radius);
    if (best > radius * radius) best = ESDF_FAR;
  }
  out[at] = best;
}

__global__ __launch_bounds__(ESDF_THREADS) void esdf_finish_kernel(const int* __restrict__ d2,
                                                                   const unsigned char* __restrict__ state,
                                                                   long long npoints, int radius, float voxel,
                                                                   float* __restrict__ dist) {
  const long long p = (long long)blockIdx.x * ESDF_THREADS + threadIdx.x;
  if (p >= npoints) return;
  const int v = d2[p];
  const float d = voxel * (v == ESDF_FAR ? (float)radius : sqrtf((float)v));
  dist[p] = state[p] == 2 ? -d : d;
}

__global__ __launch_bounds__(ESDF_THREADS) void esdf_query_kernel(
    const float* __restrict__ dist, const unsigned char* __restrict__ state, int nx, int ny, int nz, float lox, float loy,
    float loz, float voxel, const float* __restrict__ points, int n, float* __restrict__ out_dist,
    float* __restrict__ out_grad, unsigned char* __restrict__ out_flags) {
  const int p = blockIdx.x * ESDF_THREADS + threadIdx.x;
  if (p >= n) return;
  const float gx = (points[(size_t)p * 3 + 0] - lox) / voxel;
  const float gy = (points[(size_t)p * 3 + 1] - loy) / voxel;
  const float gz = (points[(size_t)p * 3 + 2] - loz) / voxel;
  const float ax = floorf(gx), ay = floorf(gy), az = floorf(gz);
  float d = 0.0f, g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
  unsigned char flags = 0;
  // NaN fails every comparison, +inf the upper and -inf the lower one: only a finite g inside the lattice is cast
  if (ax >= 0.0f && ax < (float)(nx - 1) && ay >= 0.0f && ay < (float)(ny - 1) && az >= 0.0f && az < (float)(nz - 1)) {
    const size_t at = ((size_t)(int)ax * ny + (int)ay) * nz + (int)az;
    const size_t sy = (size_t)nz, sx = (size_t)ny * nz;
    const float fx = gx - ax, fy = gy - ay, fz = gz - az;
    const TsdfCorners c = tsdf_corners_load(dist, at, ny, nz);
    const bool known = state[at] != 0 && state[at + 1] != 0 && state[at + sy] != 0 && state[at + sy + 1] != 0 &&
                       state[at + sx] != 0 && state[at + sx + 1] != 0 && state[at + sx + sy] != 0 &&
                       state[at + sx + sy + 1] != 0;
    float g[3];
    d = tsdf_corners_value(c, fx, fy, fz);
    tsdf_corners_gradient(c, fx, fy, fz, g);
    g0 = g[0] / voxel; g1 = g[1] / voxel; g2 = g[2] / voxel;
    flags = known ? 3 : 1;
  }
  out_dist[p] = d;
  out_grad[(size_t)p * 3 + 0] = g0;
  out_grad[(size_t)p * 3 + 1] = g1;
  out_grad[(size_t)p * 3 + 2] = g2;
  out_flags[p] = flags;
}

// One lane per column of the slab; v is the fastest image index and, unless z is up, runs along z.
__global__ __launch_bounds__(ESDF_THREADS) void esdf_slice_kernel(
    const unsigned char* __restrict__ state, const int* __restrict__ d2, const float* __restrict__ dist, int n_u, int n_v,
    long long stride_u, long long stride_v, long long stride_a, int k0, int k1, int occ_d2, int min_known,
    unsigned char* __restrict__ cells, float* __restrict__ clearance) {
  const int p = blockIdx.x * ESDF_THREADS + threadIdx.x;
  if (p >= n_u * n_v) return;
  const int u = p / n_v, v = p - u * n_v;
  const size_t col = (size_t)(u * stride_u + v * stride_v);
  bool occupied = false;
  int known = 0;
  float c = 0.0f;
  for (int k = k0; k <= k1; ++k) {
    const size_t at = col + (size_t)(k * stride_a);
    const int s = state[at];
    occupied = occupied || s == 2 || d2[at] <= occ_d2;
    known += s != 0 ? 1 : 0;
    const float d = dist[at];
    c = (k == k0 || d < c) ? d : c;
  }
  cells[p] = occupied ? 0 : (known >= min_known ? 254 : 205);
  clearance[p] = c;
}

}  // namespace

extern "C" int gs_esdf_build(const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight,
                             int radius, float voxel, unsigned char* state, int* d2, float* dist, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "esdf_build: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(radius >= 1 && radius <= ESDF_MAX - 1, "esdf_build: radius %d outside [1, 1023] voxels", radius);
  GS_REQUIRE(voxel > 0.0f && voxel < INFINITY, "esdf_build: voxel=%g", voxel);
  GS_REQUIRE(min_weight == min_weight, "esdf_build: min_weight is NaN");
  GS_REQUIRE(tsdf && weight && state && d2 && dist, "esdf_build: null pointer");
  const hipStream_t s = (hipStream_t)stream;
  const int rows = nx * ny, zchunks = gs_cdiv(nz, 64);
  const long long nruns = (long long)rows * zchunks, npoints = (long long)rows * nz;
  const unsigned run_blocks = (unsigned)((nruns + ESDF_WAVES - 1) / ESDF_WAVES);
  int* tmp = (int*)dist;
  GS_TIMING_PRE();
  esdf_sites_z_kernel<<<gs_cdiv(rows, ESDF_WAVES), ESDF_THREADS, 0, s>>>(tsdf, weight, nx, ny, nz, min_weight, radius,
                                                                         state, d2);
  GS_CHECK_LAUNCH("esdf_sites_z");
  esdf_pass_kernel<1><<<run_blocks, ESDF_THREADS, 0, s>>>(d2, tmp, nx, ny, nz, zchunks, nruns, radius);
  GS_CHECK_LAUNCH("esdf_pass_y");
  esdf_pass_kernel<0><<<run_blocks, ESDF_THREADS, 0, s>>>(tmp, d2, nx, ny, nz, zchunks, nruns, radius);
  GS_CHECK_LAUNCH("esdf_pass_x");
  esdf_finish_kernel<<<(unsigned)((npoints + ESDF_THREADS - 1) / ESDF_THREADS), ESDF_THREADS, 0, s>>>(
      d2, state, npoints, radius, voxel, dist);
  GS_CHECK_LAUNCH("esdf_finish");
  return GS_OK;
}

extern "C" int gs_esdf_query(const float* dist, const unsigned char* state, int nx, int ny, int nz, float lo_x,
                             float lo_y, float lo_z, float voxel, const float* points, int n, float* out_dist,
                             float* out_grad, unsigned char* out_flags, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "esdf_query: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(voxel > 0.0f && voxel < INFINITY, "esdf_query: voxel=%g", voxel);
  GS_REQUIRE(n >= 0, "esdf_query: n=%d", n);
  if (n == 0) return GS_OK;
  GS_REQUIRE(dist && state && points && out_dist && out_grad && out_flags, "esdf_query: null pointer");
  GS_TIMING_PRE();
  esdf_query_kernel<<<gs_cdiv(n, ESDF_THREADS), ESDF_THREADS, 0, (hipStream_t)stream>>>(
      dist, state, nx, ny, nz, lo_x, lo_y, lo_z, voxel, points, n, out_dist, out_grad, out_flags);
  GS_CHECK_LAUNCH("esdf_query");
  return GS_OK;
}

extern "C" int gs_esdf_slice(const unsigned char* state, const int* d2, const float* dist, int nx, int ny, int nz,
                             int up_axis, int k0, int k1, int occ_d2, int min_known, unsigned char* cells,
                             float* clearance, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "esdf_slice: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(up_axis >= 0 && up_axis <= 2, "esdf_slice: up_axis=%d outside 0..2", up_axis);
  const int n[3] = {nx, ny, nz};
  const long long stride[3] = {(long long)ny * nz, (long long)nz, 1};
  GS_REQUIRE(k0 >= 0 && k0 <= k1 && k1 < n[up_axis], "esdf_slice: layers [%d, %d] outside [0, %d) of axis %d", k0, k1,
             n[up_axis], up_axis);
  GS_REQUIRE(occ_d2 >= 0 && min_known >= 0, "esdf_slice: occ_d2=%d min_known=%d", occ_d2, min_known);
  GS_REQUIRE(state && d2 && dist && cells && clearance, "esdf_slice: null pointer");
  const int au = up_axis == 0 ? 1 : 0, av = up_axis == 2 ? 1 : 2;
  GS_TIMING_PRE();
  esdf_slice_kernel<<<gs_cdiv(n[au] * n[av], ESDF_THREADS), ESDF_THREADS, 0, (hipStream_t)stream>>>(
      state, d2, dist, n[au], n[av], stride[au], stride[av], stride[up_axis], k0, k1, occ_d2, min_known, cells,
      clearance);
  GS_CHECK_LAUNCH("esdf_slice");
  return GS_OK;
}
