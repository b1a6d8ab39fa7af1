// The dominant planes of a TSDF lattice of tsdf.hip: where is the floor, where are the walls?  (No counterpart in the
// reference.)  Contract: include/goslam_hip.h (gs_tsdf_plane_votes, gs_tsdf_plane_offsets, gs_tsdf_plane_workspace_bytes,
// gs_tsdf_plane_moments); tests/tsdf_planes_restatement.py restates the three with one rounding per operation and the
// summation order written out.  Compiled with -ffp-contract=off.
//
// All three kernels walk the lattice's cells ((nx - 1)(ny - 1)(nz - 1) of them, row-major, neighbouring lanes along z) and
// share tsdf_surface.h's plane_sample: the cell's surface sample, a point on the zero set one Newton step from the cell's
// centre, with the gradient there as its normal direction.  Most cells have none.
//
// tsdf_plane_votes_kernel / tsdf_plane_offsets_kernel: histograms of integers.  A workgroup of 1024 lanes keeps a private
// histogram of up to 16384 bins (64 KiB, two workgroups per CU) in LDS, counts into it with non-returning ds_add_u32 and
// adds its non-zero bins to the output with one global integer atomic each; a launch has at most 512 workgroups that stride
// over the cells.  A histogram with more bins (B = 64: 24576; 16 directions of 2048 bins) is cut into launches over bin
// ranges (the offsets kernel keeps its directions in the last 256 B of the 64 KiB).  Integer sums: the result does not depend on the launch geometry or on the order of arrival.
//
// tsdf_plane_moments_kernel: tsdf_gn.h's reduction order (a thread's samples t, t + 256, ... of a chunk of
// gs_tsdf_align_chunk() cells, the wave butterfly, the four waves as ((w0 + w1) + w2) + w3, the chunks in increasing order
// by tsdf_plane_sum_kernel) written out for rows of 16 values.  One workgroup per (group of up to four planes, chunk): a
// lane computes its sample once for the group, so sixteen planes cost four gathers of the lattice, not sixteen; a plane's
// ten fp64 sums never meet another plane's, so its row does not depend on which planes share the call.  No atomics.
#include "tsdf_surface.h"

namespace {

constexpr int PL_HIST_THREADS = 1024;
constexpr int PL_HIST_BINS = 16384;          // u32 bins of a workgroup's LDS histogram
constexpr int PL_OFFSET_BINS = PL_HIST_BINS - 64;      // beside the 16 directions' 64 floats: 64 KiB together
constexpr int PL_HIST_GRID = 512;            // two workgroups per CU
constexpr int PL_MAX_B = 64, PL_MAX_PLANES = 16, PL_MAX_BINS = 2048;
constexpr int PL_THREADS = 256;
constexpr int PL_WAVES = PL_THREADS / GS_WAVE;
constexpr int PL_ROW = 16;                   // doubles per row of out and of a chunk's partial
constexpr int PL_SUMS = 10;                  // q 3, q q^T 6, r^2
constexpr int PL_GROUP = 4;                  // planes a workgroup of the moments kernel carries
constexpr int PL_SUM_BATCH = 16;             // chunk totals the sum kernel loads before it adds them

// The workgroup's histogram over the bins [0, span) of this launch, zeroed / added to out[0 .. span).
__device__ __forceinline__ void plane_hist_zero(unsigned* hist, int span) {
  for (int i = threadIdx.x; i < span; i += PL_HIST_THREADS) hist[i] = 0u;
  __syncthreads();
}

__device__ __forceinline__ void plane_hist_flush(const unsigned* hist, int span, unsigned* __restrict__ out) {
  __syncthreads();
  for (int i = threadIdx.x; i < span; i += PL_HIST_THREADS) {
    const unsigned v = hist[i];
    if (v) atomicAdd(out + i, v);
  }
}

struct VotesArgs {         // by-value kernel argument (SGPRs)
  PlaneField d;
  unsigned* votes;         // [6,B,B]
  int B;
  int bin_lo, span;        // the bins [bin_lo, bin_lo + span) of this launch
};

__global__ __launch_bounds__(PL_HIST_THREADS) void tsdf_plane_votes_kernel(const VotesArgs a) {
  __shared__ unsigned hist[PL_HIST_BINS];
  plane_hist_zero(hist, a.span);
  const float half = (float)(a.B / 2);
  for (int s = blockIdx.x * PL_HIST_THREADS + threadIdx.x; s < a.d.n_cells; s += gridDim.x * PL_HIST_THREADS) {
    PlaneSample sm;
    if (!plane_sample(a.d, s, sm)) continue;
    const float a0 = fabsf(sm.g[0]), a1 = fabsf(sm.g[1]), a2 = fabsf(sm.g[2]);
    int m = a1 > a0 ? 1 : 0;                                  // the largest |g_m|; a tie keeps the lower axis
    if (a2 > (m ? a1 : a0)) m = 2;
    const float gm = m == 0 ? sm.g[0] : (m == 1 ? sm.g[1] : sm.g[2]);
    const float gb = m == 0 ? sm.g[1] : sm.g[0], gc = m == 2 ? sm.g[1] : sm.g[2];
    const float am = fabsf(gm);
    const float u = gb / am, v = gc / am;
    const int iu = min(a.B - 1, (int)floorf((u + 1.0f) * half)), iv = min(a.B - 1, (int)floorf((v + 1.0f) * half));
    const int face = 2 * m + (gm < 0.0f ? 1 : 0);
    const int idx = (face * a.B + iu) * a.B + iv - a.bin_lo;
    if ((unsigned)idx < (unsigned)a.span) atomicAdd(&hist[idx], 1u);
  }
  plane_hist_flush(hist, a.span, a.votes + a.bin_lo);
}

struct OffsetsArgs {       // by-value kernel argument (SGPRs)
  PlaneField d;
  const double* n;         // [P,3]
  const double* o0;        // [P]
  unsigned* hist;          // [P,n_bins]
  int j_lo, count;         // the directions [j_lo, j_lo + count) of this launch: count * n_bins <= PL_OFFSET_BINS
  int n_bins;
  float cos2, bin;
};

__global__ __launch_bounds__(PL_HIST_THREADS) void tsdf_plane_offsets_kernel(const OffsetsArgs a) {
  __shared__ unsigned hist[PL_OFFSET_BINS];
  __shared__ float dir[PL_MAX_PLANES][4];
  if ((int)threadIdx.x < a.count) {
    const int j = a.j_lo + threadIdx.x;
    dir[threadIdx.x][0] = (float)a.n[j * 3 + 0];
    dir[threadIdx.x][1] = (float)a.n[j * 3 + 1];
    dir[threadIdx.x][2] = (float)a.n[j * 3 + 2];
    dir[threadIdx.x][3] = (float)a.o0[j];
  }
  const int span = a.count * a.n_bins;
  plane_hist_zero(hist, span);
  const float top = (float)a.n_bins;
  for (int s = blockIdx.x * PL_HIST_THREADS + threadIdx.x; s < a.d.n_cells; s += gridDim.x * PL_HIST_THREADS) {
    PlaneSample sm;
    if (!plane_sample(a.d, s, sm)) continue;
    for (int j = 0; j < a.count; ++j) {
      const float n0 = dir[j][0], n1 = dir[j][1], n2 = dir[j][2];
      if (!plane_agrees(sm, n0, n1, n2, a.cos2)) continue;
      const float kf = floorf((plane_dot(sm, n0, n1, n2) - dir[j][3]) / a.bin);
      if (kf >= 0.0f && kf < top) atomicAdd(&hist[j * a.n_bins + (int)kf], 1u);      // a NaN fails; compared before the cast
    }
  }
  plane_hist_flush(hist, span, a.hist + (size_t)a.j_lo * a.n_bins);
}

struct MomentsArgs {       // by-value kernel argument (SGPRs)
  PlaneField d;
  const double* planes;    // [P,4]: n, o
  double* partial;         // [P,n_chunks,16]
  int n_planes, chunk, n_chunks;
  float cos2, band;
  float rx, ry, rz;        // ref
};

__global__ __launch_bounds__(PL_THREADS) void tsdf_plane_moments_kernel(const MomentsArgs a) {
  __shared__ double part[PL_WAVES][PL_GROUP][PL_ROW];
  const int group = blockIdx.x / a.n_chunks;
  const int chunk = blockIdx.x - group * a.n_chunks;
  const int j0 = group * PL_GROUP;
  const int count = min(PL_GROUP, a.n_planes - j0);
  float pl[PL_GROUP][4];
#pragma unroll
  for (int j = 0; j < PL_GROUP; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // (float) of the fp64 plane; the conversion is a vector instruction, so the uniform result is moved back to an SGPR
      const float v = j < count ? (float)a.planes[(size_t)(j0 + j) * 4 + k] : 0.0f;
      pl[j][k] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
    }
  double acc[PL_GROUP][PL_SUMS] = {};
  int inliers[PL_GROUP] = {}, agreeing[PL_GROUP] = {};
  const int s_end = min((chunk + 1) * a.chunk, a.d.n_cells);
#pragma nounroll
  for (int s = chunk * a.chunk + (int)threadIdx.x; s < s_end; s += PL_THREADS) {
    PlaneSample sm;
    if (!plane_sample(a.d, s, sm)) continue;
    const double q0 = (double)(sm.p[0] - a.rx), q1 = (double)(sm.p[1] - a.ry), q2 = (double)(sm.p[2] - a.rz);
#pragma unroll
    for (int j = 0; j < PL_GROUP; ++j) {
      if (j >= count || !plane_agrees(sm, pl[j][0], pl[j][1], pl[j][2], a.cos2)) continue;
      ++agreeing[j];
      const float r = plane_dot(sm, pl[j][0], pl[j][1], pl[j][2]) - pl[j][3];
      if (!(fabsf(r) <= a.band)) continue;
      ++inliers[j];
      const double rd = (double)r;
      acc[j][0] += q0; acc[j][1] += q1; acc[j][2] += q2;
      acc[j][3] += q0 * q0; acc[j][4] += q0 * q1; acc[j][5] += q0 * q2;
      acc[j][6] += q1 * q1; acc[j][7] += q1 * q2; acc[j][8] += q2 * q2;
      acc[j][9] += rd * rd;
    }
  }
  // the chunk's rows: sums 0 .. 9, inliers, agreeing samples, 0 0 0 0
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < PL_GROUP; ++j) {
#pragma unroll
    for (int i = 0; i < PL_SUMS; ++i) {
      const double v = gs_wave_sum_f64(acc[j][i]);
      if (lane == 0) part[wave][j][i] = v;
    }
    const int ci = gs_wave_sum_i32(inliers[j]), ca = gs_wave_sum_i32(agreeing[j]);     // integers: any order gives the sum
    if (lane == 0) {
      part[wave][j][10] = (double)ci;
      part[wave][j][11] = (double)ca;
      part[wave][j][12] = 0.0; part[wave][j][13] = 0.0; part[wave][j][14] = 0.0; part[wave][j][15] = 0.0;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < count * PL_ROW) {
    const int j = threadIdx.x / PL_ROW, i = threadIdx.x - j * PL_ROW;
    a.partial[((size_t)(j0 + j) * a.n_chunks + chunk) * PL_ROW + i] =
        ((part[0][j][i] + part[1][j][i]) + part[2][j][i]) + part[3][j][i];
  }
}

// One wave per plane: out's row is the sum of the plane's chunk rows in increasing chunk order.  A lane loads sixteen of
// them at a time, so that the sum is not a chain of as many memory latencies as there are chunks.
__global__ __launch_bounds__(GS_WAVE) void tsdf_plane_sum_kernel(const double* __restrict__ partial, int n_chunks,
                                                                 double* __restrict__ out) {
  const int i = threadIdx.x;
  if (i >= PL_ROW) return;
  const double* __restrict__ p = partial + (size_t)blockIdx.x * n_chunks * PL_ROW + i;
  double t = p[0];
  int c = 1;
  for (; c + PL_SUM_BATCH <= n_chunks; c += PL_SUM_BATCH) {
    double v[PL_SUM_BATCH];
#pragma unroll
    for (int j = 0; j < PL_SUM_BATCH; ++j) v[j] = p[(size_t)(c + j) * PL_ROW];
#pragma unroll
    for (int j = 0; j < PL_SUM_BATCH; ++j) t = t + v[j];
  }
  for (; c < n_chunks; ++c) t = t + p[(size_t)c * PL_ROW];
  out[(size_t)blockIdx.x * PL_ROW + i] = t;
}

int plane_min(int a, int b) { return a < b ? a : b; }

unsigned plane_hist_grid(int n_cells) { return (unsigned)plane_min(gs_cdiv(n_cells, PL_HIST_THREADS), PL_HIST_GRID); }

}  // namespace

extern "C" int gs_tsdf_align_chunk(void);

extern "C" int gs_tsdf_plane_votes(const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight, int bins,
                                   unsigned* votes, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_plane_votes: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(bins >= 2 && bins <= PL_MAX_B && bins % 2 == 0, "tsdf_plane_votes: bins=%d (need an even number in [2, %d])", bins,
             PL_MAX_B);
  GS_REQUIRE(plane_finite(min_weight), "tsdf_plane_votes: min_weight=%g", min_weight);
  GS_REQUIRE(tsdf && weight && votes, "tsdf_plane_votes: null pointer");
  VotesArgs a;
  a.d = plane_field(tsdf, weight, nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f, min_weight);
  a.votes = votes; a.B = bins;
  const int total = 6 * bins * bins;
  GS_TIMING_PRE();
  for (int lo = 0; lo < total; lo += PL_HIST_BINS) {
    a.bin_lo = lo; a.span = plane_min(PL_HIST_BINS, total - lo);
    tsdf_plane_votes_kernel<<<plane_hist_grid(a.d.n_cells), PL_HIST_THREADS, 0, (hipStream_t)stream>>>(a);
    GS_CHECK_LAUNCH("tsdf_plane_votes");
  }
  return GS_OK;
}

extern "C" int gs_tsdf_plane_offsets(const float* tsdf, const float* weight, int nx, int ny, int nz, float lo_x, float lo_y,
                                     float lo_z, float voxel, float min_weight, const double* normals, const double* o0,
                                     int n_planes, float cos2, float bin, int n_bins, unsigned* hist, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_plane_offsets: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(n_planes >= 0 && n_planes <= PL_MAX_PLANES, "tsdf_plane_offsets: n_planes=%d outside [0, %d]", n_planes,
             PL_MAX_PLANES);
  GS_REQUIRE(n_bins >= 1 && n_bins <= PL_MAX_BINS, "tsdf_plane_offsets: n_bins=%d outside [1, %d]", n_bins, PL_MAX_BINS);
  GS_REQUIRE(voxel > 0.0f && voxel < INFINITY, "tsdf_plane_offsets: voxel=%g", voxel);
  GS_REQUIRE(plane_finite(lo_x) && plane_finite(lo_y) && plane_finite(lo_z), "tsdf_plane_offsets: lo=(%g, %g, %g)", lo_x, lo_y,
             lo_z);
  GS_REQUIRE(plane_finite(min_weight), "tsdf_plane_offsets: min_weight=%g", min_weight);
  GS_REQUIRE(cos2 >= 0.0f && cos2 <= 1.0f, "tsdf_plane_offsets: cos2=%g outside [0, 1]", cos2);
  GS_REQUIRE(bin > 0.0f && bin < INFINITY, "tsdf_plane_offsets: bin=%g", bin);
  GS_REQUIRE(tsdf && weight && normals && o0 && hist, "tsdf_plane_offsets: null pointer");
  if (n_planes == 0) return GS_OK;
  OffsetsArgs a;
  a.d = plane_field(tsdf, weight, nx, ny, nz, lo_x, lo_y, lo_z, voxel, min_weight);
  a.n = normals; a.o0 = o0; a.hist = hist;
  a.n_bins = n_bins; a.cos2 = cos2; a.bin = bin;
  const int per_launch = PL_OFFSET_BINS / n_bins;             // >= 7
  GS_TIMING_PRE();
  for (int lo = 0; lo < n_planes; lo += per_launch) {
    a.j_lo = lo; a.count = plane_min(per_launch, n_planes - lo);
    tsdf_plane_offsets_kernel<<<plane_hist_grid(a.d.n_cells), PL_HIST_THREADS, 0, (hipStream_t)stream>>>(a);
    GS_CHECK_LAUNCH("tsdf_plane_offsets");
  }
  return GS_OK;
}

extern "C" size_t gs_tsdf_plane_workspace_bytes(int n_planes, int nx, int ny, int nz) {
  if (n_planes < 0 || n_planes > PL_MAX_PLANES || !tsdf_dims_ok(nx, ny, nz)) return 0;
  const size_t chunks = (size_t)gs_cdiv(plane_cells(nx, ny, nz), gs_tsdf_align_chunk());
  return (size_t)n_planes * chunks * PL_ROW * sizeof(double);
}

extern "C" int gs_tsdf_plane_moments(const float* tsdf, const float* weight, int nx, int ny, int nz, float lo_x, float lo_y,
                                     float lo_z, float voxel, float min_weight, const double* planes, int n_planes,
                                     float cos2, float band, float ref_x, float ref_y, float ref_z, void* workspace,
                                     double* out, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_plane_moments: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(n_planes >= 0 && n_planes <= PL_MAX_PLANES, "tsdf_plane_moments: n_planes=%d outside [0, %d]", n_planes,
             PL_MAX_PLANES);
  GS_REQUIRE(voxel > 0.0f && voxel < INFINITY, "tsdf_plane_moments: voxel=%g", voxel);
  GS_REQUIRE(plane_finite(lo_x) && plane_finite(lo_y) && plane_finite(lo_z), "tsdf_plane_moments: lo=(%g, %g, %g)", lo_x, lo_y,
             lo_z);
  GS_REQUIRE(plane_finite(ref_x) && plane_finite(ref_y) && plane_finite(ref_z), "tsdf_plane_moments: ref=(%g, %g, %g)", ref_x,
             ref_y, ref_z);
  GS_REQUIRE(plane_finite(min_weight), "tsdf_plane_moments: min_weight=%g", min_weight);
  GS_REQUIRE(cos2 >= 0.0f && cos2 <= 1.0f, "tsdf_plane_moments: cos2=%g outside [0, 1]", cos2);
  GS_REQUIRE(band >= 0.0f && band < INFINITY, "tsdf_plane_moments: band=%g", band);
  GS_REQUIRE(tsdf && weight && planes && workspace && out, "tsdf_plane_moments: null pointer");
  if (n_planes == 0) return GS_OK;
  MomentsArgs a;
  a.d = plane_field(tsdf, weight, nx, ny, nz, lo_x, lo_y, lo_z, voxel, min_weight);
  a.planes = planes; a.partial = (double*)workspace;
  a.n_planes = n_planes; a.chunk = gs_tsdf_align_chunk(); a.n_chunks = gs_cdiv(a.d.n_cells, a.chunk);
  a.cos2 = cos2; a.band = band;
  a.rx = ref_x; a.ry = ref_y; a.rz = ref_z;
  GS_TIMING_PRE();
  tsdf_plane_moments_kernel<<<(unsigned)(gs_cdiv(n_planes, PL_GROUP) * a.n_chunks), PL_THREADS, 0, (hipStream_t)stream>>>(a);
  GS_CHECK_LAUNCH("tsdf_plane_moments");
  tsdf_plane_sum_kernel<<<(unsigned)n_planes, GS_WAVE, 0, (hipStream_t)stream>>>(a.partial, a.n_chunks, out);
  GS_CHECK_LAUNCH("tsdf_plane_sum");
  return GS_OK;
}
