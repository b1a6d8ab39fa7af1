// Mesh culling (Mesher.cull_mesh, reference src/mesher.py:155-240): depth maps of a mesh at many poses, per-vertex
// visibility against them, face-adjacency connected components with deterministic fp64 areas, and an exact interior-discard
// filter in front of the convex hull behind the oriented bounding boxes.  Contracts: include/goslam_neus.h (gs_mesh_*,
// gs_face_*, gs_hull_*).
#include "mesh_raster.h"

namespace {

// ---------------------------------------------------------------------------------------
// depth maps
// ---------------------------------------------------------------------------------------
constexpr unsigned MD_EMPTY = 0xffffffffu;

// a fragment of the depth maps: the min of the fp32 bit patterns
struct DepthFrag {
  unsigned* zbuf;
  size_t hw;
  __device__ __forceinline__ void operator()(int k, size_t px, double z, int) const {
    atomicMin(zbuf + (size_t)k * hw + px, __float_as_uint((float)z));
  }
};

__global__ __launch_bounds__(MD_BLOCK) void mesh_depth_kernel(const float* __restrict__ V, const int* __restrict__ Fc,
                                                              int nf, int nv, const float* __restrict__ w2c, int K,
                                                              double fx, double fy, double cx, double cy, int H, int W,
                                                              double znear, double zfar, unsigned* __restrict__ zbuf,
                                                              int2* __restrict__ large, int large_cap,
                                                              int* __restrict__ large_count) {
  raster_faces(V, Fc, nf, nv, w2c, K, fx, fy, cx, cy, H, W, znear, zfar, large, large_cap, large_count,
               DepthFrag{zbuf, (size_t)H * W});
}

__global__ __launch_bounds__(MD_BLOCK) void mesh_depth_large_kernel(const float* __restrict__ V,
                                                                    const int* __restrict__ Fc, const float* __restrict__ w2c,
                                                                    double fx, double fy, double cx, double cy, int H,
                                                                    int W, double znear, double zfar,
                                                                    unsigned* __restrict__ zbuf,
                                                                    const int2* __restrict__ large, int large_cap,
                                                                    const int* __restrict__ large_count) {
  raster_large_faces(V, Fc, w2c, fx, fy, cx, cy, H, W, znear, zfar, large, large_cap, large_count,
                     DepthFrag{zbuf, (size_t)H * W});
}

__global__ void mesh_depth_finalize_kernel(unsigned* __restrict__ zbuf, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && zbuf[i] == MD_EMPTY) zbuf[i] = 0u;   // 0.0f
}

// ---------------------------------------------------------------------------------------
// visibility masks
// ---------------------------------------------------------------------------------------
// F.grid_sample(depth[1,1,H,W], grid, padding_mode='border', align_corners=True) at one point, torch's CPU kernel op by op.
__device__ __forceinline__ float sample_border(const float* __restrict__ d, int H, int W, float u, float v) {
  float gx = u / (float)(W - 1);
  gx = gx * 2.0f;
  gx = gx - 1.0f;
  float gy = v / (float)(H - 1);
  gy = gy * 2.0f;
  gy = gy - 1.0f;
  float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1);
  float iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
  ix = fminf((float)(W - 1), fmaxf(ix, 0.0f));
  iy = fminf((float)(H - 1), fmaxf(iy, 0.0f));
  const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.0f, y1 = y0 + 1.0f;
  const float nw = (x1 - ix) * (y1 - iy), ne = (ix - x0) * (y1 - iy);
  const float sw = (x1 - ix) * (iy - y0), se = (ix - x0) * (iy - y0);
  const int xi = (int)x0, yi = (int)y0;
  float out = 0.0f;
  const bool xin0 = xi >= 0 && xi < W, xin1 = xi + 1 >= 0 && xi + 1 < W;
  const bool yin0 = yi >= 0 && yi < H, yin1 = yi + 1 >= 0 && yi + 1 < H;
  if (yin0 && xin0) out += d[(size_t)yi * W + xi] * nw;
  if (yin0 && xin1) out += d[(size_t)yi * W + xi + 1] * ne;
  if (yin1 && xin0) out += d[(size_t)(yi + 1) * W + xi] * sw;
  if (yin1 && xin1) out += d[(size_t)(yi + 1) * W + xi + 1] * se;
  return out;
}

__global__ __launch_bounds__(256) void mesh_visibility_kernel(const float* __restrict__ P, int n,
                                                              const float* __restrict__ w2c, const float* __restrict__ depth,
                                                              int K, float fx, float fy, float cx, float cy, int H, int W,
                                                              float radius, uint8_t* __restrict__ seen,
                                                              uint8_t* __restrict__ forecast) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = P[3 * (size_t)i], y = P[3 * (size_t)i + 1], zw = P[3 * (size_t)i + 2];
  bool s = seen[i] != 0, fc = forecast[i] != 0;
  const float umax = (float)(W - 1), vmax = (float)(H - 1);
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const float* M = w2c + 16 * (size_t)k;
    const float X = fmaf(M[2], zw, fmaf(M[1], y, M[0] * x)) + M[3];
    const float Y = fmaf(M[6], zw, fmaf(M[5], y, M[4] * x)) + M[7];
    const float Z = fmaf(M[10], zw, fmaf(M[9], y, M[8] * x)) + M[11];
    const float z = Z + 1e-8f;
    const float u = fmaf(cx, Z, fx * X) / z, v = fmaf(cy, Z, fy * Y) / z;
    const bool inf = (u >= 0.0f) && (u <= umax) && (v >= 0.0f) && (v <= vmax) && (z > 0.0f);
    const bool ff = (u >= -radius) && (u <= umax + radius) && (v >= -radius) && (v <= vmax + radius) && (z > 0.0f);
    if (!inf && !ff) continue;
    const float d = sample_border(depth + (size_t)k * H * W, H, W, u, v);
    const bool front = d > 0.0f ? (z < d + 0.05f) : true;
    s = s || (inf && front);
    fc = fc || (inf && front) || (ff && front);
  }
  seen[i] = s;
  forecast[i] = fc;
}

// ---------------------------------------------------------------------------------------
// connected components
// ---------------------------------------------------------------------------------------
constexpr unsigned long long CC_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {   // splitmix64 finaliser
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ bool edge_key(const int* __restrict__ Fc, int f, int e, unsigned long long& key) {
  const int a = Fc[3 * (size_t)f + e], b = Fc[3 * (size_t)f + (e + 1) % 3];
  if (a == b) return false;                       // an edge with equal endpoints connects nothing
  const unsigned lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
  key = ((unsigned long long)lo << 32) | hi;
  return true;
}

__global__ void cc_init_kernel(unsigned long long* __restrict__ keys, int* __restrict__ first, size_t cap,
                               int* __restrict__ parent, int nf) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < cap) { keys[i] = CC_EMPTY; first[i] = 0x7fffffff; }
  if (i < (size_t)nf) parent[i] = (int)i;
}

// Edge -> smallest face using it: open addressing, linear probing, capacity a power of two above the edge count.
__global__ void cc_insert_kernel(const int* __restrict__ Fc, int nf, unsigned long long* __restrict__ keys,
                                 int* __restrict__ first, size_t cap) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 3LL * nf) return;
  const int f = (int)(t / 3), e = (int)(t % 3);
  unsigned long long key;
  if (!edge_key(Fc, f, e, key)) return;
  size_t h = mix64(key) & (cap - 1);
  for (size_t probe = 0; probe < cap; ++probe, h = (h + 1) & (cap - 1)) {
    const unsigned long long old = atomicCAS(&keys[h], CC_EMPTY, key);
    if (old == CC_EMPTY || old == key) {
      atomicMin(&first[h], f);
      return;
    }
  }
}

__device__ __forceinline__ int cc_parent(const int* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int cc_find(int* parent, int x) {
  int p = cc_parent(parent, x);
  while (p != x) {
    x = p;
    p = cc_parent(parent, x);
  }
  return x;
}

// Union of every face with the first face of each of its edges.  Hooking always puts the larger root under the smaller
// one (a compare-and-swap that only succeeds on a root), so every root is the smallest face index of its component.
__global__ void cc_union_kernel(const int* __restrict__ Fc, int nf, const unsigned long long* __restrict__ keys,
                                const int* __restrict__ first, size_t cap, int* __restrict__ parent) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 3LL * nf) return;
  const int f = (int)(t / 3), e = (int)(t % 3);
  unsigned long long key;
  if (!edge_key(Fc, f, e, key)) return;
  size_t h = mix64(key) & (cap - 1);
  int g = -1;
  for (size_t probe = 0; probe < cap; ++probe, h = (h + 1) & (cap - 1)) {
    if (keys[h] == key) { g = first[h]; break; }
  }
  if (g < 0 || g == f) return;
  int a = f, b = g;
  while (true) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) { const int tmp = a; a = b; b = tmp; }   // hook a (larger root) under b
    const int old = atomicCAS(&parent[a], a, b);
    if (old == a) return;
    a = old;                                           // a was hooked meanwhile: retry from its new parent
  }
}

__global__ void cc_compress_kernel(const int* __restrict__ parent, int nf, int* __restrict__ labels) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  int x = f, p = parent[x];
  while (p != x) { x = p; p = parent[x]; }
  labels[f] = x;
}

// fp64 face areas, 0.5 |(v1 - v0) x (v2 - v0)|
__global__ void cc_area_kernel(const double* __restrict__ V, const int* __restrict__ Fc, int nf,
                               double* __restrict__ area) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const double* a = V + 3 * (size_t)Fc[3 * (size_t)f];
  const double* b = V + 3 * (size_t)Fc[3 * (size_t)f + 1];
  const double* c = V + 3 * (size_t)Fc[3 * (size_t)f + 2];
  const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  double x[3];
  cross3(u, w, x);
  area[f] = 0.5 * sqrt(__dadd_rn(__dadd_rn(__dmul_rn(x[0], x[0]), __dmul_rn(x[1], x[1])), __dmul_rn(x[2], x[2])));
}

constexpr int CC_TILE = 1024;

// Per tile of the label-sorted faces, each run of one label (a piece) summed serially in ascending position; the sum is
// stored at the piece's last position.
__global__ void cc_piece_kernel(const double* __restrict__ area, const int* __restrict__ perm,
                                const int* __restrict__ slab, int nf, double* __restrict__ piece) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nf) return;
  const bool end = i == nf - 1 || slab[i + 1] != slab[i] || (i % CC_TILE) == CC_TILE - 1;
  if (!end) return;
  const int t0 = i - i % CC_TILE;
  int j = i;
  while (j > t0 && slab[j - 1] == slab[i]) --j;
  double s = 0.0;
  for (; j <= i; ++j) s += area[perm[j]];
  piece[i] = s;
}

// Per label (at its first sorted position): the pieces in tile order.  comp_area[label] = the sum; 0 for non-roots.
__global__ void cc_segment_kernel(const double* __restrict__ piece, const int* __restrict__ slab, int nf,
                                  double* __restrict__ comp_area) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nf || (s > 0 && slab[s - 1] == slab[s])) return;
  const int lab = slab[s];
  int lo = s, hi = nf;               // first position with a larger label
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (slab[mid] <= lab) lo = mid + 1; else hi = mid;
  }
  const int e = lo - 1;
  double acc = 0.0;
  for (int t = s / CC_TILE; t <= e / CC_TILE; ++t) acc += piece[min(e, t * CC_TILE + CC_TILE - 1)];
  comp_area[lab] = acc;
}

// total = sum of comp_area in a fixed order: per thread a strided serial sum, then a fixed LDS tree.
__global__ __launch_bounds__(1024) void cc_total_kernel(const double* __restrict__ comp_area, int nf,
                                                        double* __restrict__ total) {
  __shared__ double red[1024];
  double s = 0.0;
  for (int i = threadIdx.x; i < nf; i += 1024) s += comp_area[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = red[0];
}

// ---------------------------------------------------------------------------------------
// convex-hull pre-filter
// ---------------------------------------------------------------------------------------
constexpr int HULL_DIRS = 13;
constexpr int HULL_BLOCK = 256;
__constant__ double kHullDir[HULL_DIRS][3] = {
    {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, -1, 0}, {1, 0, 1}, {1, 0, -1},
    {0, 1, 1}, {0, 1, -1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {-1, 1, 1},
};

struct Ext { double val; int idx; };

// a beats b: larger value, ties to the lower index; NaN never wins
__device__ __forceinline__ bool ext_better(double va, int ia, double vb, int ib) {
  return va > vb || (va == vb && ia < ib);
}

// Per workgroup, for each of the 26 functionals +-dir . p (fp64), the best (value, index); ext[block][26].
__global__ __launch_bounds__(HULL_BLOCK) void hull_extreme_kernel(const float* __restrict__ P, int n,
                                                                  Ext* __restrict__ ext) {
  __shared__ double sv[HULL_BLOCK];
  __shared__ int si[HULL_BLOCK];
  const int i = blockIdx.x * HULL_BLOCK + threadIdx.x;
  double p[3] = {0, 0, 0};
  const bool ok = i < n;
  if (ok) { p[0] = P[3 * (size_t)i]; p[1] = P[3 * (size_t)i + 1]; p[2] = P[3 * (size_t)i + 2]; }
  for (int q = 0; q < 2 * HULL_DIRS; ++q) {
    const double sg = q < HULL_DIRS ? 1.0 : -1.0;
    const double* d = kHullDir[q % HULL_DIRS];
    const double v = sg * (d[0] * p[0] + d[1] * p[1] + d[2] * p[2]);
    sv[threadIdx.x] = (ok && v == v) ? v : -INFINITY;
    si[threadIdx.x] = (ok && v == v) ? i : 0x7fffffff;
    __syncthreads();
    for (int w = HULL_BLOCK / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w && ext_better(sv[threadIdx.x + w], si[threadIdx.x + w], sv[threadIdx.x], si[threadIdx.x])) {
        sv[threadIdx.x] = sv[threadIdx.x + w];
        si[threadIdx.x] = si[threadIdx.x + w];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) ext[(size_t)blockIdx.x * 2 * HULL_DIRS + q] = Ext{sv[0], si[0]};
    __syncthreads();
  }
}

// One workgroup per functional: the best over all blocks -> idx[26] (-1 when there is no finite point).
__global__ __launch_bounds__(HULL_BLOCK) void hull_extreme_final_kernel(const Ext* __restrict__ ext, int nblk,
                                                                        int* __restrict__ idx) {
  __shared__ double sv[HULL_BLOCK];
  __shared__ int si[HULL_BLOCK];
  const int q = blockIdx.x;
  double bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int b = threadIdx.x; b < nblk; b += HULL_BLOCK) {
    const Ext e = ext[(size_t)b * 2 * HULL_DIRS + q];
    if (ext_better(e.val, e.idx, bv, bi)) { bv = e.val; bi = e.idx; }
  }
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int w = HULL_BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w && ext_better(sv[threadIdx.x + w], si[threadIdx.x + w], sv[threadIdx.x], si[threadIdx.x])) {
      sv[threadIdx.x] = sv[threadIdx.x + w];
      si[threadIdx.x] = si[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) idx[q] = si[0] == 0x7fffffff ? -1 : si[0];
}

// keep[i] = 0 iff point i is strictly inside every plane n.p + c <= 0 by more than margin, in fp64.
__global__ __launch_bounds__(256) void hull_filter_kernel(const float* __restrict__ P, int n,
                                                          const double* __restrict__ planes, int nplanes, double margin,
                                                          uint8_t* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = P[3 * (size_t)i], y = P[3 * (size_t)i + 1], z = P[3 * (size_t)i + 2];
  bool inside = true;
  for (int k = 0; k < nplanes && inside; ++k) {
    const double* pl = planes + 4 * k;
    inside = pl[0] * x + pl[1] * y + pl[2] * z + pl[3] < -margin;
  }
  keep[i] = !inside;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------
extern "C" size_t gs_mesh_depth_workspace_bytes(void) {
  return 256 + (size_t)GS_MESH_DEPTH_LARGE_CAP * sizeof(int2);
}

extern "C" int gs_mesh_depth(const float* vertices, int n_vertices, const int* faces, int n_faces, const float* w2c,
                             int n_poses, float fx, float fy, float cx, float cy, int height, int width, float znear,
                             float zfar, float* depth, void* workspace, size_t workspace_bytes, gs_stream_t stream) {
  GS_REQUIRE(depth && w2c && workspace, "mesh_depth: null pointer");
  GS_REQUIRE(n_vertices >= 0 && n_faces >= 0 && n_poses >= 0, "mesh_depth: negative size");
  GS_REQUIRE(n_faces == 0 || (vertices && faces), "mesh_depth: null mesh");
  GS_REQUIRE(height >= 1 && width >= 1 && (long long)height * width <= (1LL << 24),
             "mesh_depth: image %d x %d unsupported", height, width);
  GS_REQUIRE(fx != 0.0f && fy != 0.0f && znear > 0.0f && zfar > znear, "mesh_depth: bad camera");
  if (workspace_bytes < gs_mesh_depth_workspace_bytes()) {
    gs_set_error("mesh_depth: workspace %zu < %zu bytes", workspace_bytes, gs_mesh_depth_workspace_bytes());
    return GS_ERR_WORKSPACE;
  }
  if (n_poses == 0) return GS_OK;
  int* count = (int*)workspace;
  int2* large = (int2*)((char*)workspace + 256);
  const size_t npix = (size_t)n_poses * height * width;
  hipStream_t st = (hipStream_t)stream;
  GS_TIMING_PRE();
  if (hipMemsetAsync(depth, 0xff, npix * sizeof(float), st) != hipSuccess ||
      hipMemsetAsync(count, 0, sizeof(int), st) != hipSuccess) {
    gs_set_error("mesh_depth: memset failed");
    return GS_ERR_LAUNCH;
  }
  if (n_faces > 0) {
    mesh_depth_kernel<<<gs_cdiv(n_faces, MD_BLOCK), MD_BLOCK, 0, st>>>(
        vertices, faces, n_faces, n_vertices, w2c, n_poses, fx, fy, cx, cy, height, width, znear, zfar,
        (unsigned*)depth, large, GS_MESH_DEPTH_LARGE_CAP, count);
    GS_CHECK_LAUNCH("mesh_depth");
    mesh_depth_large_kernel<<<1024, MD_BLOCK, 0, st>>>(vertices, faces, w2c, fx, fy, cx, cy, height, width, znear, zfar,
                                                       (unsigned*)depth, large, GS_MESH_DEPTH_LARGE_CAP, count);
    GS_CHECK_LAUNCH("mesh_depth_large");
  }
  mesh_depth_finalize_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, st>>>((unsigned*)depth, npix);
  GS_CHECK_LAUNCH("mesh_depth_finalize");
  return GS_OK;
}

extern "C" int gs_mesh_visibility(const float* points, int n_points, const float* w2c, const float* depth, int n_poses,
                                  float fx, float fy, float cx, float cy, int height, int width, float forecast_radius,
                                  uint8_t* seen, uint8_t* forecast, gs_stream_t stream) {
  GS_REQUIRE(n_points >= 0 && n_poses >= 0, "mesh_visibility: negative size");
  GS_REQUIRE(height >= 2 && width >= 2, "mesh_visibility: image %d x %d unsupported", height, width);
  if (n_points == 0 || n_poses == 0) return GS_OK;
  GS_REQUIRE(points && w2c && depth && seen && forecast, "mesh_visibility: null pointer");
  GS_TIMING_PRE();
  mesh_visibility_kernel<<<gs_cdiv(n_points, 256), 256, 0, (hipStream_t)stream>>>(
      points, n_points, w2c, depth, n_poses, fx, fy, cx, cy, height, width, forecast_radius, seen, forecast);
  GS_CHECK_LAUNCH("mesh_visibility");
  return GS_OK;
}

static size_t cc_capacity(int n_faces) {
  size_t cap = 1024;
  while (cap < 2 * 3 * (size_t)n_faces) cap <<= 1;
  return cap;
}

extern "C" size_t gs_face_components_workspace_bytes(int n_faces) {
  if (n_faces < 0) return 0;
  const size_t cap = cc_capacity(n_faces);
  return cap * sizeof(unsigned long long) + cap * sizeof(int) + (size_t)n_faces * sizeof(int) + 256;
}

extern "C" int gs_face_components(const int* faces, int n_faces, int* labels, void* workspace, size_t workspace_bytes,
                                  gs_stream_t stream) {
  GS_REQUIRE(n_faces >= 0 && n_faces <= (1 << 28), "face_components: %d faces unsupported", n_faces);
  if (n_faces == 0) return GS_OK;
  GS_REQUIRE(faces && labels && workspace, "face_components: null pointer");
  if (workspace_bytes < gs_face_components_workspace_bytes(n_faces)) {
    gs_set_error("face_components: workspace %zu < %zu bytes", workspace_bytes,
                 gs_face_components_workspace_bytes(n_faces));
    return GS_ERR_WORKSPACE;
  }
  const size_t cap = cc_capacity(n_faces);
  unsigned long long* keys = (unsigned long long*)workspace;
  int* first = (int*)(keys + cap);
  int* parent = first + cap;
  hipStream_t st = (hipStream_t)stream;
  const int edge_blocks = (int)((3LL * n_faces + 255) / 256);
  GS_TIMING_PRE();
  cc_init_kernel<<<(unsigned)((cap + 255) / 256), 256, 0, st>>>(keys, first, cap, parent, n_faces);
  GS_CHECK_LAUNCH("face_components_init");
  cc_insert_kernel<<<edge_blocks, 256, 0, st>>>(faces, n_faces, keys, first, cap);
  GS_CHECK_LAUNCH("face_components_insert");
  cc_union_kernel<<<edge_blocks, 256, 0, st>>>(faces, n_faces, keys, first, cap, parent);
  GS_CHECK_LAUNCH("face_components_union");
  cc_compress_kernel<<<gs_cdiv(n_faces, 256), 256, 0, st>>>(parent, n_faces, labels);
  GS_CHECK_LAUNCH("face_components_compress");
  return GS_OK;
}

extern "C" int gs_face_component_areas(const double* vertices, const int* faces, int n_faces, const int* perm,
                                       const int* sorted_labels, double* comp_area, double* total, void* workspace,
                                       size_t workspace_bytes, gs_stream_t stream) {
  GS_REQUIRE(n_faces >= 0 && n_faces <= (1 << 28), "face_component_areas: %d faces unsupported", n_faces);
  GS_REQUIRE(total && (n_faces == 0 || (vertices && faces && perm && sorted_labels && comp_area && workspace)),
             "face_component_areas: null pointer");
  if (workspace_bytes < 2 * (size_t)n_faces * sizeof(double)) {
    gs_set_error("face_component_areas: workspace %zu < %zu bytes", workspace_bytes, 2 * (size_t)n_faces * sizeof(double));
    return GS_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* area = (double*)workspace;
  double* piece = area + n_faces;
  GS_TIMING_PRE();
  if (n_faces > 0) {
    if (hipMemsetAsync(comp_area, 0, (size_t)n_faces * sizeof(double), st) != hipSuccess) {
      gs_set_error("face_component_areas: memset failed");
      return GS_ERR_LAUNCH;
    }
    const int nb = gs_cdiv(n_faces, 256);
    cc_area_kernel<<<nb, 256, 0, st>>>(vertices, faces, n_faces, area);
    GS_CHECK_LAUNCH("face_areas");
    cc_piece_kernel<<<nb, 256, 0, st>>>(area, perm, sorted_labels, n_faces, piece);
    GS_CHECK_LAUNCH("face_area_pieces");
    cc_segment_kernel<<<nb, 256, 0, st>>>(piece, sorted_labels, n_faces, comp_area);
    GS_CHECK_LAUNCH("face_area_segments");
  }
  cc_total_kernel<<<1, 1024, 0, st>>>(comp_area, n_faces, total);
  GS_CHECK_LAUNCH("face_area_total");
  return GS_OK;
}

extern "C" size_t gs_hull_extremes_workspace_bytes(int n_points) {
  if (n_points < 0) return 0;
  return (size_t)gs_cdiv(n_points > 0 ? n_points : 1, HULL_BLOCK) * 2 * HULL_DIRS * sizeof(Ext);
}

extern "C" int gs_hull_extremes(const float* points, int n_points, int* idx, void* workspace, size_t workspace_bytes,
                                gs_stream_t stream) {
  GS_REQUIRE(n_points >= 1, "hull_extremes: need at least one point");
  GS_REQUIRE(points && idx && workspace, "hull_extremes: null pointer");
  if (workspace_bytes < gs_hull_extremes_workspace_bytes(n_points)) {
    gs_set_error("hull_extremes: workspace %zu < %zu bytes", workspace_bytes, gs_hull_extremes_workspace_bytes(n_points));
    return GS_ERR_WORKSPACE;
  }
  const int nblk = gs_cdiv(n_points, HULL_BLOCK);
  GS_TIMING_PRE();
  hull_extreme_kernel<<<nblk, HULL_BLOCK, 0, (hipStream_t)stream>>>(points, n_points, (Ext*)workspace);
  GS_CHECK_LAUNCH("hull_extremes");
  hull_extreme_final_kernel<<<2 * HULL_DIRS, HULL_BLOCK, 0, (hipStream_t)stream>>>((const Ext*)workspace, nblk, idx);
  GS_CHECK_LAUNCH("hull_extremes_final");
  return GS_OK;
}

extern "C" int gs_hull_prefilter(const float* points, int n_points, const double* planes, int n_planes, double margin,
                                 uint8_t* keep, gs_stream_t stream) {
  GS_REQUIRE(n_points >= 0 && n_planes >= 0 && margin >= 0.0, "hull_prefilter: bad arguments");
  if (n_points == 0) return GS_OK;
  GS_REQUIRE(points && keep && (n_planes == 0 || planes), "hull_prefilter: null pointer");
  GS_TIMING_PRE();
  hull_filter_kernel<<<gs_cdiv(n_points, 256), 256, 0, (hipStream_t)stream>>>(points, n_points, planes, n_planes, margin,
                                                                              keep);
  GS_CHECK_LAUNCH("hull_prefilter");
  return GS_OK;
}
