// What stands in the room: the surface samples of a TSDF lattice of tsdf.hip that lie on none of the given structure
// planes (floor, walls), their 26-connected clusters and one table row per cluster.  (No counterpart in the reference.)
// Contract: include/goslam_hip.h (gs_tsdf_object_mark, gs_tsdf_object_table, gs_tsdf_object_extents);
// tests/tsdf_objects_restatement.py restates it with one rounding per operation.  Compiled with -ffp-contract=off.
//
// All kernels walk the lattice's cells ((nx - 1)(ny - 1)(nz - 1) of them, row-major, neighbouring lanes along z: the
// numbering of tsdf_surface.h's plane_sample) in frontier_rows.h's blocks of FR_THREADS * FR_PER cells, so that the labels
// tsdf_object_mark_kernel writes are relaxed by gs_frontier_relax and ranked by gs_frontier_roots as they stand.  (A
// measurement build of frontier.hip with another brick compiles this file with the same -D.)
//
// tsdf_object_mark_kernel: one lane per cell, FR_PER cells per lane.  The planes, rounded to fp32, lie in LDS and are read
//   by every lane at the same address (a broadcast).  Writes kind and label, the four counts (ballots per wave, LDS per
//   workgroup, at most four integer atomics per workgroup) and the dirty byte, in flag buffer 0, of every brick that holds
//   an object cell.
// fr_fold_rows (frontier_rows.h): the skeleton of the two passes that fold cells into table rows.  A labelled cell finds
//   its row by binary search of its label among the roots and forms what it adds; the lanes of a wave that share a row reduce by
//   butterflies and one lane per (wave, row) issues the integer atomics: add, min, max, or.  Each is exact and commutes,
//   so the rows do not depend on the order of arrival.
// tsdf_object_table_kernel: size, the first and second moments of the cell coordinates, the box, and the structure planes
//   among the 26 neighbours' kinds.  tsdf_object_extents_kernel: the sample point again (plane_sample) along the row's
//   three axes, minimum and maximum in an order-preserving integer encoding of the float.
#include "frontier_rows.h"
#include "tsdf_surface.h"

namespace {

constexpr int OB_MAX_PLANES = 16;
constexpr unsigned OB_EXT_EMPTY_MIN = 0xff800000u;         // e(+inf)
constexpr unsigned OB_EXT_EMPTY_MAX = 0x007fffffu;         // e(-inf)

struct MarkArgs {          // by-value kernel argument (SGPRs)
  PlaneField d;
  const double* planes;    // [n_planes,4]: n, o
  int n_planes;
  float cos2, band;
  unsigned char* kind;
  int* label;
  unsigned* counts;
  unsigned char* flags;    // buffer 0
  int nb1, nb2;            // bricks along y and z
};

__global__ __launch_bounds__(FR_THREADS) void tsdf_object_mark_kernel(const MarkArgs a) {
  __shared__ float pl[OB_MAX_PLANES][4];
  __shared__ unsigned part[FR_WAVES][4];
  const int tid = threadIdx.x, lane = tid % GS_WAVE, wave = tid / GS_WAVE;
  if (tid < a.n_planes * 4) pl[tid >> 2][tid & 3] = (float)a.planes[tid];
  __syncthreads();
  const int base = blockIdx.x * FR_BLOCK;
  const int cyz = a.d.cy * a.d.cz;
  unsigned n[4] = {0u, 0u, 0u, 0u};                         // wave totals: samples, object, structure, crease cells
#pragma nounroll
  for (int i = 0; i < FR_PER; ++i) {
    const int p = base + i * FR_THREADS + tid;
    const bool in = p < a.d.n_cells;
    PlaneSample sm;
    const bool is = in && plane_sample(a.d, p, sm);
    int on = -1, near = -1, n_near = 0;                     // the lowest plane the sample is on / near; how many it is near
    if (is) {
      for (int j = 0; j < a.n_planes; ++j) {
        const float n0 = pl[j][0], n1 = pl[j][1], n2 = pl[j][2];
        const float r = plane_dot(sm, n0, n1, n2) - pl[j][3];
        if (!(fabsf(r) <= a.band)) continue;                // a NaN is not near
        ++n_near;
        if (near < 0) near = j;
        if (on < 0 && plane_agrees(sm, n0, n1, n2, a.cos2)) on = j;
      }
    }
    const bool structure = on >= 0 || n_near >= 2;          // on a plane, or in the crease of two
    const bool object = is && !structure;
    if (in) {
      a.kind[p] = (unsigned char)(!is ? 0 : (structure ? 2 + (on >= 0 ? on : near) : 1));
      a.label[p] = object ? p : -1;
    }
    if (object) {
      const int c0 = p / cyz, rem = p - c0 * cyz;
      const int c1 = rem / a.d.cz, c2 = rem - c1 * a.d.cz;
      a.flags[((size_t)(c0 / B0) * a.nb1 + c1 / B1) * a.nb2 + c2 / B2] = 1;       // buffer 0; every store writes 1
    }
    n[0] += fr_popc(__ballot(is));
    n[1] += fr_popc(__ballot(object));
    n[2] += fr_popc(__ballot(structure));
    n[3] += fr_popc(__ballot(structure && on < 0));
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
    if (total != 0) atomicAdd(&a.counts[tid], total);
  }
}

// ---- cells into rows ----------------------------------------------------------------------------------------------------
template <class T, class Op>
__device__ __forceinline__ T ob_wave(T v, Op op) {          // every lane returns op over the wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, GS_WAVE));
  return v;
}
__device__ __forceinline__ unsigned ob_wave_min(unsigned v) {
  return ob_wave(v, [](unsigned x, unsigned y) { return y < x ? y : x; });
}
__device__ __forceinline__ unsigned ob_wave_max(unsigned v) {
  return ob_wave(v, [](unsigned x, unsigned y) { return y > x ? y : x; });
}
__device__ __forceinline__ unsigned ob_wave_or(unsigned v) {
  return ob_wave(v, [](unsigned x, unsigned y) { return x | y; });
}

struct TableFold {
  const unsigned char* kind;
  int n0, n1, n2;
  int* size;
  unsigned long long* sum;
  unsigned long long* sum2;
  int* bbox;
  unsigned* touch;
  int c0, c1, c2;
  unsigned bits;

  __device__ __forceinline__ int load(int p, int id) {
    c0 = 0, c1 = 0, c2 = 0, bits = 0u;
    if (id < 0) return id;
    c2 = p % n2, c1 = p / n2 % n1, c0 = p / n2 / n1;
    for (int d0 = -1; d0 <= 1; ++d0)
      for (int d1 = -1; d1 <= 1; ++d1)
#pragma unroll
        for (int d2 = -1; d2 <= 1; ++d2) {
          const int q0 = c0 + d0, q1 = c1 + d1, q2 = c2 + d2;
          if (q0 < 0 || q0 >= n0 || q1 < 0 || q1 >= n1 || q2 < 0 || q2 >= n2) continue;
          const int k = kind[((size_t)q0 * n1 + q1) * n2 + q2];   // the cell itself holds 1
          if (k >= 2 && k < 2 + OB_MAX_PLANES) bits |= 1u << (k - 2);
        }
    return id;
  }

  __device__ __forceinline__ void fold(int row, bool mine, unsigned long long members, bool leader) {
    const int m0 = mine ? c0 : 0, m1 = mine ? c1 : 0, m2 = mine ? c2 : 0;
    const int s0 = gs_wave_sum_i32(m0), s1 = gs_wave_sum_i32(m1), s2 = gs_wave_sum_i32(m2);
    const long long q00 = gs_wave_sum_i64((long long)m0 * m0), q01 = gs_wave_sum_i64((long long)m0 * m1);
    const long long q02 = gs_wave_sum_i64((long long)m0 * m2), q11 = gs_wave_sum_i64((long long)m1 * m1);
    const long long q12 = gs_wave_sum_i64((long long)m1 * m2), q22 = gs_wave_sum_i64((long long)m2 * m2);
    const int lo0 = gs_wave_min_i32(mine ? c0 : FR_MAX), lo1 = gs_wave_min_i32(mine ? c1 : FR_MAX);
    const int lo2 = gs_wave_min_i32(mine ? c2 : FR_MAX);
    const int hi0 = -gs_wave_min_i32(mine ? -c0 : 1), hi1 = -gs_wave_min_i32(mine ? -c1 : 1);
    const int hi2 = -gs_wave_min_i32(mine ? -c2 : 1);
    const unsigned t = ob_wave_or(mine ? bits : 0u);
    if (!leader) return;
    atomicAdd(&size[row], fr_popc(members));
    atomicAdd(&sum[(size_t)row * 3 + 0], (unsigned long long)s0);
    atomicAdd(&sum[(size_t)row * 3 + 1], (unsigned long long)s1);
    atomicAdd(&sum[(size_t)row * 3 + 2], (unsigned long long)s2);
    atomicAdd(&sum2[(size_t)row * 6 + 0], (unsigned long long)q00);
    atomicAdd(&sum2[(size_t)row * 6 + 1], (unsigned long long)q01);
    atomicAdd(&sum2[(size_t)row * 6 + 2], (unsigned long long)q02);
    atomicAdd(&sum2[(size_t)row * 6 + 3], (unsigned long long)q11);
    atomicAdd(&sum2[(size_t)row * 6 + 4], (unsigned long long)q12);
    atomicAdd(&sum2[(size_t)row * 6 + 5], (unsigned long long)q22);
    atomicMin(&bbox[(size_t)row * 6 + 0], lo0);
    atomicMin(&bbox[(size_t)row * 6 + 1], lo1);
    atomicMin(&bbox[(size_t)row * 6 + 2], lo2);
    atomicMax(&bbox[(size_t)row * 6 + 3], hi0);
    atomicMax(&bbox[(size_t)row * 6 + 4], hi1);
    atomicMax(&bbox[(size_t)row * 6 + 5], hi2);
    if (t != 0u) atomicOr(&touch[row], t);
  }
};

// the roots in ascending order into the table's first `rows` rows, each row cleared
__global__ __launch_bounds__(FR_THREADS) void tsdf_object_emit_kernel(const int* __restrict__ label, int ncells,
                                                                      const unsigned* __restrict__ first, int rows,
                                                                      int* __restrict__ root, int* __restrict__ size,
                                                                      unsigned long long* __restrict__ sum,
                                                                      unsigned long long* __restrict__ sum2,
                                                                      int* __restrict__ bbox, unsigned* __restrict__ touch) {
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
    touch[slot] = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sum[(size_t)slot * 3 + a] = 0ull;
      sum2[(size_t)slot * 6 + a] = 0ull;
      sum2[(size_t)slot * 6 + 3 + a] = 0ull;
      bbox[(size_t)slot * 6 + a] = FR_MAX;
      bbox[(size_t)slot * 6 + 3 + a] = -1;
    }
  }
}

__global__ __launch_bounds__(FR_THREADS) void tsdf_object_table_kernel(const int* __restrict__ label,
                                                                       const int* __restrict__ root, int rows, TableFold f) {
  fr_fold_rows(label, f.n0 * f.n1 * f.n2, root, rows, f);
}

// e(x): unsigned integers in the order of the floats they encode
__device__ __forceinline__ unsigned ob_encode(float x) {
  const unsigned b = __float_as_uint(x);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

struct ExtentFold {
  PlaneField d;
  const double* axes;      // [rows,3,3]
  unsigned* ext;           // [rows,3,2]
  unsigned e[3];

  __device__ __forceinline__ int load(int p, int id) {
    e[0] = 0u, e[1] = 0u, e[2] = 0u;
    if (id < 0) return id;
    PlaneSample sm;
    if (!plane_sample(d, p, sm)) return -1;                 // labels that are not this lattice's
    const double* __restrict__ ax = axes + (size_t)id * 9;
#pragma unroll
    for (int m = 0; m < 3; ++m)
      e[m] = ob_encode(plane_dot(sm, (float)ax[m * 3 + 0], (float)ax[m * 3 + 1], (float)ax[m * 3 + 2]));
    return id;
  }

  __device__ __forceinline__ void fold(int row, bool mine, unsigned long long, bool leader) {
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const unsigned lo = ob_wave_min(mine ? e[m] : 0xffffffffu), hi = ob_wave_max(mine ? e[m] : 0u);
      if (leader) {
        atomicMin(&ext[((size_t)row * 3 + m) * 2 + 0], lo);
        atomicMax(&ext[((size_t)row * 3 + m) * 2 + 1], hi);
      }
    }
  }
};

__global__ __launch_bounds__(FR_THREADS) void tsdf_object_extents_init_kernel(unsigned* __restrict__ ext, size_t n) {
  const size_t i = (size_t)blockIdx.x * FR_THREADS + threadIdx.x;
  if (i < n) ext[i] = (i & 1) ? OB_EXT_EMPTY_MAX : OB_EXT_EMPTY_MIN;
}

__global__ __launch_bounds__(FR_THREADS) void tsdf_object_extents_kernel(const int* __restrict__ label,
                                                                         const int* __restrict__ root, int rows,
                                                                         ExtentFold f) {
  fr_fold_rows(label, f.d.n_cells, root, rows, f);
}

}  // namespace

extern "C" size_t gs_frontier_flags_bytes(int n0, int n1, int n2);

extern "C" int gs_tsdf_object_mark(const float* tsdf, const float* weight, int nx, int ny, int nz, float lo_x, float lo_y,
                                   float lo_z, float voxel, float min_weight, const double* planes, int n_planes, float cos2,
                                   float band, unsigned char* kind, int* label, unsigned int* counts, unsigned char* flags,
                                   gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_object_mark: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(n_planes >= 0 && n_planes <= OB_MAX_PLANES, "tsdf_object_mark: n_planes=%d outside [0, %d]", n_planes,
             OB_MAX_PLANES);
  GS_REQUIRE(voxel > 0.0f && voxel < INFINITY, "tsdf_object_mark: voxel=%g", voxel);
  GS_REQUIRE(plane_finite(lo_x) && plane_finite(lo_y) && plane_finite(lo_z), "tsdf_object_mark: lo=(%g, %g, %g)", lo_x, lo_y,
             lo_z);
  GS_REQUIRE(plane_finite(min_weight), "tsdf_object_mark: min_weight=%g", min_weight);
  GS_REQUIRE(cos2 >= 0.0f && cos2 <= 1.0f, "tsdf_object_mark: cos2=%g outside [0, 1]", cos2);
  GS_REQUIRE(band >= 0.0f && band < INFINITY, "tsdf_object_mark: band=%g", band);
  GS_REQUIRE(tsdf && weight && planes && kind && label && counts && flags, "tsdf_object_mark: null pointer");
  const int cx = nx - 1, cy = ny - 1, cz = nz - 1;
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(unsigned int) * 4, s) != hipSuccess ||
      hipMemsetAsync(flags, 0, gs_frontier_flags_bytes(cx, cy, cz), s) != hipSuccess) {
    gs_set_error("tsdf_object_mark: clearing counts and flags failed");
    return GS_ERR_LAUNCH;
  }
  MarkArgs a;
  a.d = plane_field(tsdf, weight, nx, ny, nz, lo_x, lo_y, lo_z, voxel, min_weight);
  a.planes = planes; a.n_planes = n_planes; a.cos2 = cos2; a.band = band;
  a.kind = kind; a.label = label; a.counts = counts; a.flags = flags;
  a.nb1 = gs_cdiv(cy, B1); a.nb2 = gs_cdiv(cz, B2);
  GS_TIMING_PRE();
  tsdf_object_mark_kernel<<<fr_blocks(cx, cy, cz), FR_THREADS, 0, s>>>(a);
  GS_CHECK_LAUNCH("tsdf_object_mark");
  return GS_OK;
}

extern "C" int gs_tsdf_object_table(const unsigned char* kind, const int* label, int cx, int cy, int cz,
                                    const void* workspace, size_t workspace_bytes, int rows, int capacity, int* root,
                                    int* size, long long* sum, long long* sum2, int* bbox, unsigned int* touch,
                                    gs_stream_t stream) {
  GS_REQUIRE(brick_dims_ok(cx, cy, cz), "tsdf_object_table: lattice %d x %d x %d outside [1, 1024]", cx, cy, cz);
  GS_REQUIRE(rows >= 0 && capacity >= rows, "tsdf_object_table: %d rows do not fit a table of capacity %d", rows, capacity);
  GS_REQUIRE(kind && label && workspace && root && size && sum && sum2 && bbox && touch, "tsdf_object_table: null pointer");
  GS_REQUIRE((((uintptr_t)sum | (uintptr_t)sum2) & 7u) == 0, "tsdf_object_table: sum or sum2 is not 8-byte aligned");
  const int nblk = fr_blocks(cx, cy, cz);
  GS_REQUIRE(workspace_bytes >= fr_workspace_bytes(nblk), "tsdf_object_table: workspace of %zu bytes, %zu needed",
             workspace_bytes, fr_workspace_bytes(nblk));
  if (rows == 0) return GS_OK;
  const hipStream_t s = (hipStream_t)stream;
  TableFold f;
  f.kind = kind; f.n0 = cx; f.n1 = cy; f.n2 = cz;
  f.size = size; f.sum = (unsigned long long*)sum; f.sum2 = (unsigned long long*)sum2; f.bbox = bbox; f.touch = touch;
  f.c0 = f.c1 = f.c2 = 0; f.bits = 0u;
  GS_TIMING_PRE();
  tsdf_object_emit_kernel<<<nblk, FR_THREADS, 0, s>>>(label, cx * cy * cz, fr_workspace_first(workspace, nblk), rows, root,
                                                      size, f.sum, f.sum2, bbox, touch);
  GS_CHECK_LAUNCH("tsdf_object_emit");
  tsdf_object_table_kernel<<<nblk, FR_THREADS, 0, s>>>(label, root, rows, f);
  GS_CHECK_LAUNCH("tsdf_object_table");
  return GS_OK;
}

extern "C" int gs_tsdf_object_extents(const float* tsdf, const float* weight, int nx, int ny, int nz, float lo_x, float lo_y,
                                      float lo_z, float voxel, float min_weight, const int* label, const int* root, int rows,
                                      const double* axes, unsigned int* ext, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_object_extents: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(rows >= 0 && rows <= plane_cells(nx, ny, nz), "tsdf_object_extents: rows=%d outside [0, the number of cells]",
             rows);
  GS_REQUIRE(voxel > 0.0f && voxel < INFINITY, "tsdf_object_extents: voxel=%g", voxel);
  GS_REQUIRE(plane_finite(lo_x) && plane_finite(lo_y) && plane_finite(lo_z), "tsdf_object_extents: lo=(%g, %g, %g)", lo_x,
             lo_y, lo_z);
  GS_REQUIRE(plane_finite(min_weight), "tsdf_object_extents: min_weight=%g", min_weight);
  GS_REQUIRE(tsdf && weight && label && root && axes && ext, "tsdf_object_extents: null pointer");
  if (rows == 0) return GS_OK;
  const hipStream_t s = (hipStream_t)stream;
  ExtentFold f;
  f.d = plane_field(tsdf, weight, nx, ny, nz, lo_x, lo_y, lo_z, voxel, min_weight);
  f.axes = axes; f.ext = ext;
  f.e[0] = f.e[1] = f.e[2] = 0u;
  GS_TIMING_PRE();
  const size_t entries = (size_t)rows * 6;                  // < 2^33
  tsdf_object_extents_init_kernel<<<(unsigned)((entries + FR_THREADS - 1) / FR_THREADS), FR_THREADS, 0, s>>>(ext, entries);
  GS_CHECK_LAUNCH("tsdf_object_extents_init");
  tsdf_object_extents_kernel<<<fr_blocks(nx - 1, ny - 1, nz - 1), FR_THREADS, 0, s>>>(label, root, rows, f);
  GS_CHECK_LAUNCH("tsdf_object_extents");
  return GS_OK;
}
