// The reconstruction video (MeshVideo, reference src/tools/meshvideo.py) without a window: a visibility buffer of the mesh
// and of depth-tested line overlays, area-weighted vertex normals in fixed point, and the resolve pass that shades what
// won each pixel.  Every result is independent of arrival order.  Contracts: include/goslam_neus.h (gs_mesh_visbuf,
// gs_line_visbuf, gs_vertex_normals, gs_visbuf_resolve); the rasteriser is cull.hip's (mesh_raster.h).
#include "mesh_raster.h"

namespace {

constexpr unsigned long long VB_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long vb_key(double z, unsigned id) {
  return ((unsigned long long)__float_as_uint((float)z) << 32) | id;
}

// a fragment of the visibility buffer: the min of (fp32 depth bits, face), so equal depths go to the lower face
struct VisFrag {
  unsigned long long* vb;
  size_t hw;
  __device__ __forceinline__ void operator()(int k, size_t px, double z, int f) const {
    atomicMin(vb + (size_t)k * hw + px, vb_key(z, (unsigned)f));
  }
};

__global__ __launch_bounds__(MD_BLOCK) void mesh_visbuf_kernel(const float* __restrict__ V, const int* __restrict__ Fc,
                                                               int nf, int nv, const float* __restrict__ w2c, int K,
                                                               double fx, double fy, double cx, double cy, int H, int W,
                                                               double znear, double zfar,
                                                               unsigned long long* __restrict__ vb,
                                                               int2* __restrict__ large, int large_cap,
                                                               int* __restrict__ large_count) {
  raster_faces(V, Fc, nf, nv, w2c, K, fx, fy, cx, cy, H, W, znear, zfar, large, large_cap, large_count,
               VisFrag{vb, (size_t)H * W});
}

__global__ __launch_bounds__(MD_BLOCK) void mesh_visbuf_large_kernel(const float* __restrict__ V,
                                                                     const int* __restrict__ Fc,
                                                                     const float* __restrict__ w2c, double fx, double fy,
                                                                     double cx, double cy, int H, int W, double znear,
                                                                     double zfar, unsigned long long* __restrict__ vb,
                                                                     const int2* __restrict__ large, int large_cap,
                                                                     const int* __restrict__ large_count) {
  raster_large_faces(V, Fc, w2c, fx, fy, cx, cy, H, W, znear, zfar, large, large_cap, large_count,
                     VisFrag{vb, (size_t)H * W});
}

// ---------------------------------------------------------------------------------------
// lines
// ---------------------------------------------------------------------------------------
// Narrow [ta, tb] to the part of t in which p0 + t dp lies in [0, hi): a conservative range for the walk, the exact test
// is made per step.
__device__ __forceinline__ void clip_range(double p0, double dp, double hi, double& ta, double& tb) {
  if (dp == 0.0) {
    if (!(p0 >= 0.0 && p0 < hi)) tb = -1.0;
    return;
  }
  const double t0 = (0.0 - p0) / dp, t1 = (hi - p0) / dp;
  ta = fmax(ta, fmin(t0, t1));
  tb = fmin(tb, fmax(t0, t1));
}

// One wave per (segment, pose).
__global__ __launch_bounds__(64) void line_visbuf_kernel(const float* __restrict__ S, int ns, unsigned id_base,
                                                         const float* __restrict__ w2c, int K, double fx, double fy,
                                                         double cx, double cy, int H, int W, double znear, double zfar,
                                                         unsigned long long* __restrict__ vb) {
  const long long job = blockIdx.x;
  const int s = (int)(job / K), k = (int)(job % K);
  if (s >= ns) return;
  double M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = (double)w2c[12 * (size_t)k + i];
  double P[2][3];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float* q = S + 6 * (size_t)s + 3 * j;
    const double x = q[0], y = q[1], z = q[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) P[j][r] = ((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3];
  }
  bool finite = true;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 3; ++r) finite = finite && isfinite(P[j][r]);
  if (!finite || (P[0][2] < znear && P[1][2] < znear)) return;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (P[j][2] < znear) {                     // the other end is in front of the plane
      const double* A = P[1 - j];
      const double a = (znear - A[2]) / (P[j][2] - A[2]);
      P[j][0] = A[0] + a * (P[j][0] - A[0]);
      P[j][1] = A[1] + a * (P[j][1] - A[1]);
      P[j][2] = znear;
    }
  }
  const double u0 = fx * P[0][0] / P[0][2] + cx, v0 = fy * P[0][1] / P[0][2] + cy;
  const double u1 = fx * P[1][0] / P[1][2] + cx, v1 = fy * P[1][1] / P[1][2] + cy;
  const double nd = fmax(fabs(floor(u1) - floor(u0)), fabs(floor(v1) - floor(v0)));
  if (!(nd < 4503599627370496.0)) return;      // non-finite projection
  const double du = u1 - u0, dv = v1 - v0;
  double ta = 0.0, tb = 1.0;
  clip_range(u0, du, (double)W, ta, tb);
  clip_range(v0, dv, (double)H, ta, tb);
  if (!(ta <= tb)) return;
  const long long n = (long long)nd;
  const long long i0 = max(0LL, (long long)floor(ta * nd) - 2), i1 = min(n, (long long)ceil(tb * nd) + 2);
  const double iz0 = 1.0 / P[0][2], diz = 1.0 / P[1][2] - iz0;
  unsigned long long* vk = vb + (size_t)k * H * W;
  for (long long i = i0 + threadIdx.x; i <= i1; i += 64) {
    const double t = n > 0 ? (double)i / nd : 0.0;
    const double u = u0 + t * du, v = v0 + t * dv;
    const double c = floor(u), r = floor(v);
    if (!(c >= 0.0 && c < (double)W && r >= 0.0 && r < (double)H)) continue;
    const double z = 1.0 / (iz0 + t * diz);
    if (!(z >= znear && z <= zfar)) continue;
    atomicMin(vk + (size_t)r * W + (size_t)c, vb_key(z, id_base + (unsigned)s));
  }
}

// ---------------------------------------------------------------------------------------
// vertex normals
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void normal_accumulate_kernel(const float* __restrict__ V, int nv,
                                                                const int* __restrict__ Fc, int nf, double scale,
                                                                unsigned long long* __restrict__ sums) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int vid[3] = {Fc[3 * (size_t)f], Fc[3 * (size_t)f + 1], Fc[3 * (size_t)f + 2]};
  if (vid[0] < 0 || vid[1] < 0 || vid[2] < 0 || vid[0] >= nv || vid[1] >= nv || vid[2] >= nv) return;
  double p[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int r = 0; r < 3; ++r) p[j][r] = V[3 * (size_t)vid[j] + r];
  const double a[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
  const double b[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
  double x[3];
  cross3(a, b, x);
  long long q[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double y = rint(x[r] * scale);
    if (!(fabs(y) < 4611686018427387904.0)) return;   // 2^62; also NaN
    q[r] = (long long)y;
  }
  if (q[0] == 0 && q[1] == 0 && q[2] == 0) return;
  // two's-complement wrap-around makes the unsigned add the signed one
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (q[r] != 0) atomicAdd(sums + 3 * (size_t)vid[j] + r, (unsigned long long)q[r]);
}

__global__ __launch_bounds__(256) void normal_normalize_kernel(const long long* __restrict__ sums, int nv,
                                                               float* __restrict__ N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const double x = (double)sums[3 * (size_t)i], y = (double)sums[3 * (size_t)i + 1], z = (double)sums[3 * (size_t)i + 2];
  const double len = sqrt((x * x + y * y) + z * z);
  const bool ok = len > 0.0;
  N[3 * (size_t)i] = ok ? (float)(x / len) : 0.0f;
  N[3 * (size_t)i + 1] = ok ? (float)(y / len) : 0.0f;
  N[3 * (size_t)i + 2] = ok ? (float)(z / len) : 0.0f;
}

// ---------------------------------------------------------------------------------------
// resolve
// ---------------------------------------------------------------------------------------
constexpr int RS_BLOCK = 256;

struct ShadeArgs {
  const float* V; const int* Fc; const float* w2c;
  const uint8_t* vcol; const float* vnrm; const uint8_t* lcol;
  int nv, nf, ns, flat, H, W;
  double fx, fy, cx, cy, ambient, diffuse;
  unsigned background;
};

__device__ __forceinline__ unsigned shade_pixel(const ShadeArgs& A, unsigned long long key, int k, int r, int c) {
  if (key == VB_EMPTY) return A.background;
  const unsigned id = (unsigned)key;
  if (id >= (unsigned)A.nf) {
    const unsigned s = id - (unsigned)A.nf;
    if (s >= (unsigned)A.ns) return A.background;
    const uint8_t* q = A.lcol + 3 * (size_t)s;
    return ((unsigned)q[0] << 16) | ((unsigned)q[1] << 8) | q[2];
  }
  const int vid[3] = {A.Fc[3 * (size_t)id], A.Fc[3 * (size_t)id + 1], A.Fc[3 * (size_t)id + 2]};
  if (vid[0] < 0 || vid[1] < 0 || vid[2] < 0 || vid[0] >= A.nv || vid[1] >= A.nv || vid[2] >= A.nv)
    return A.background;
  const float* M = A.w2c + 12 * (size_t)k;
  Tri t;
  double zmin, zmax, n[3], e[3], dx, dy;
  tri_camera(A.V, vid, M, t, zmin, zmax);
  tri_edges(vid, t, n);
  tri_edge_functions(t, r, c, A.fx, A.fy, A.cx, A.cy, e, dx, dy);
  const double den = e[0] + e[1] + e[2];
  if (!(den != 0.0) || !isfinite(den)) return A.background;
  const double w[3] = {e[1] / den, e[2] / den, e[0] / den};
  if (!A.flat) {
    double nw[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) nw[q] = nw[q] + w[j] * (double)A.vnrm[3 * (size_t)vid[j] + q];
#pragma unroll
    for (int q = 0; q < 3; ++q)
      n[q] = ((double)M[4 * q] * nw[0] + (double)M[4 * q + 1] * nw[1]) + (double)M[4 * q + 2] * nw[2];
  }
  const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2], dd = (dx * dx + dy * dy) + 1.0;
  const double nd = (n[0] * dx + n[1] * dy) + n[2];
  const double cosine = nn > 0.0 && isfinite(nn) ? fabs(nd) / sqrt(nn * dd) : 0.0;
  const double shade = A.ambient + A.diffuse * cosine;
  unsigned out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    double albedo = 255.0 * GS_SHADE_GREY;
    if (A.vcol) {
      albedo = 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) albedo = albedo + w[j] * (double)A.vcol[3 * (size_t)vid[j] + ch];
    }
    const double v = rint(fmin(fmax(albedo * shade, 0.0), 255.0));
    out = (out << 8) | (unsigned)(v == v ? (int)v : 0);
  }
  return out;
}

// One thread per pixel; the workgroup's 768 output bytes are staged in LDS and leave as 192 dwords (a thread's own three
// bytes would be three byte stores at a stride of 3).
__global__ __launch_bounds__(RS_BLOCK) void visbuf_resolve_kernel(const unsigned long long* __restrict__ vb, size_t npix,
                                                                  ShadeArgs A, uint8_t* __restrict__ img) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[3 * RS_BLOCK];
  const size_t base = (size_t)blockIdx.x * RS_BLOCK, i = base + threadIdx.x;
  if (i < npix) {
    const size_t hw = (size_t)A.H * A.W;
    const int k = (int)(i / hw), p = (int)(i % hw);
    const unsigned rgb = shade_pixel(A, vb[i], k, p / A.W, p % A.W);
    stage[3 * threadIdx.x] = (uint8_t)(rgb >> 16);
    stage[3 * threadIdx.x + 1] = (uint8_t)(rgb >> 8);
    stage[3 * threadIdx.x + 2] = (uint8_t)rgb;
  }
  __syncthreads();
  uint8_t* out = img + 3 * base;
  if (base + RS_BLOCK <= npix && ((uintptr_t)img & 3) == 0) {
    if (threadIdx.x < 3 * RS_BLOCK / 4) ((unsigned*)out)[threadIdx.x] = ((const unsigned*)stage)[threadIdx.x];
  } else {
    const size_t nb = 3 * (npix - base < (size_t)RS_BLOCK ? npix - base : (size_t)RS_BLOCK);
    for (size_t b = threadIdx.x; b < nb; b += RS_BLOCK) out[b] = stage[b];
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------
extern "C" size_t gs_mesh_visbuf_workspace_bytes(void) { return 256 + (size_t)GS_MESH_DEPTH_LARGE_CAP * sizeof(int2); }

extern "C" int gs_mesh_visbuf(const float* vertices, int n_vertices, const int* faces, int n_faces, const float* w2c,
                              int n_poses, float fx, float fy, float cx, float cy, int height, int width, float znear,
                              float zfar, unsigned long long* visbuf, void* workspace, size_t workspace_bytes,
                              gs_stream_t stream) {
  GS_REQUIRE(visbuf && w2c && workspace, "mesh_visbuf: null pointer");
  GS_REQUIRE(n_vertices >= 0 && n_faces >= 0 && n_poses >= 0, "mesh_visbuf: negative size");
  GS_REQUIRE(n_faces == 0 || (vertices && faces), "mesh_visbuf: null mesh");
  GS_REQUIRE(height >= 1 && width >= 1 && (long long)height * width <= (1LL << 24),
             "mesh_visbuf: image %d x %d unsupported", height, width);
  GS_REQUIRE(fx != 0.0f && fy != 0.0f && znear > 0.0f && zfar > znear, "mesh_visbuf: bad camera");
  if (workspace_bytes < gs_mesh_visbuf_workspace_bytes()) {
    gs_set_error("mesh_visbuf: workspace %zu < %zu bytes", workspace_bytes, gs_mesh_visbuf_workspace_bytes());
    return GS_ERR_WORKSPACE;
  }
  if (n_poses == 0) return GS_OK;
  int* count = (int*)workspace;
  int2* large = (int2*)((char*)workspace + 256);
  const size_t npix = (size_t)n_poses * height * width;
  hipStream_t st = (hipStream_t)stream;
  GS_TIMING_PRE();
  if (hipMemsetAsync(visbuf, 0xff, npix * sizeof(unsigned long long), st) != hipSuccess ||
      hipMemsetAsync(count, 0, sizeof(int), st) != hipSuccess) {
    gs_set_error("mesh_visbuf: memset failed");
    return GS_ERR_LAUNCH;
  }
  if (n_faces > 0) {
    mesh_visbuf_kernel<<<gs_cdiv(n_faces, MD_BLOCK), MD_BLOCK, 0, st>>>(
        vertices, faces, n_faces, n_vertices, w2c, n_poses, fx, fy, cx, cy, height, width, znear, zfar, visbuf, large,
        GS_MESH_DEPTH_LARGE_CAP, count);
    GS_CHECK_LAUNCH("mesh_visbuf");
    mesh_visbuf_large_kernel<<<1024, MD_BLOCK, 0, st>>>(vertices, faces, w2c, fx, fy, cx, cy, height, width, znear, zfar,
                                                        visbuf, large, GS_MESH_DEPTH_LARGE_CAP, count);
    GS_CHECK_LAUNCH("mesh_visbuf_large");
  }
  return GS_OK;
}

extern "C" int gs_line_visbuf(const float* segments, int n_segments, unsigned id_base, const float* w2c, int n_poses,
                              float fx, float fy, float cx, float cy, int height, int width, float znear, float zfar,
                              unsigned long long* visbuf, gs_stream_t stream) {
  GS_REQUIRE(n_segments >= 0 && n_poses >= 0, "line_visbuf: negative size");
  GS_REQUIRE((unsigned long long)id_base + (unsigned long long)n_segments <= 0xffffffffull, "line_visbuf: ids overflow");
  GS_REQUIRE(height >= 1 && width >= 1 && (long long)height * width <= (1LL << 24),
             "line_visbuf: image %d x %d unsupported", height, width);
  GS_REQUIRE(fx != 0.0f && fy != 0.0f && znear > 0.0f && zfar > znear, "line_visbuf: bad camera");
  if (n_segments == 0 || n_poses == 0) return GS_OK;
  GS_REQUIRE(segments && w2c && visbuf, "line_visbuf: null pointer");
  GS_REQUIRE((long long)n_segments * n_poses <= 0x7fffffffLL, "line_visbuf: %d segments x %d poses unsupported",
             n_segments, n_poses);
  GS_TIMING_PRE();
  line_visbuf_kernel<<<(unsigned)((long long)n_segments * n_poses), 64, 0, (hipStream_t)stream>>>(
      segments, n_segments, id_base, w2c, n_poses, fx, fy, cx, cy, height, width, znear, zfar, visbuf);
  GS_CHECK_LAUNCH("line_visbuf");
  return GS_OK;
}

extern "C" int gs_vertex_normals(const float* vertices, int n_vertices, const int* faces, int n_faces, double scale,
                                 long long* sums, float* normals, gs_stream_t stream) {
  GS_REQUIRE(n_vertices >= 0 && n_faces >= 0, "vertex_normals: negative size");
  GS_REQUIRE(scale > 0.0 && scale < 1e300, "vertex_normals: bad scale");
  if (n_vertices == 0) return GS_OK;
  GS_REQUIRE(vertices && sums && normals && (n_faces == 0 || faces), "vertex_normals: null pointer");
  hipStream_t st = (hipStream_t)stream;
  GS_TIMING_PRE();
  if (hipMemsetAsync(sums, 0, 3 * (size_t)n_vertices * sizeof(long long), st) != hipSuccess) {
    gs_set_error("vertex_normals: memset failed");
    return GS_ERR_LAUNCH;
  }
  if (n_faces > 0) {
    normal_accumulate_kernel<<<gs_cdiv(n_faces, 256), 256, 0, st>>>(vertices, n_vertices, faces, n_faces, scale,
                                                                    (unsigned long long*)sums);
    GS_CHECK_LAUNCH("vertex_normals_accumulate");
  }
  normal_normalize_kernel<<<gs_cdiv(n_vertices, 256), 256, 0, st>>>(sums, n_vertices, normals);
  GS_CHECK_LAUNCH("vertex_normals_normalize");
  return GS_OK;
}

extern "C" int gs_visbuf_resolve(const unsigned long long* visbuf, int n_poses, int height, int width,
                                 const float* vertices, int n_vertices, const int* faces, int n_faces, const float* w2c,
                                 float fx, float fy, float cx, float cy, const uint8_t* vertex_colors,
                                 const float* vertex_normals, int flat, const uint8_t* line_colors, int n_segments,
                                 float ambient, float diffuse, unsigned background, uint8_t* image, gs_stream_t stream) {
  GS_REQUIRE(n_poses >= 0 && n_vertices >= 0 && n_faces >= 0 && n_segments >= 0, "visbuf_resolve: negative size");
  GS_REQUIRE(height >= 1 && width >= 1 && (long long)height * width <= (1LL << 24),
             "visbuf_resolve: image %d x %d unsupported", height, width);
  GS_REQUIRE(fx != 0.0f && fy != 0.0f, "visbuf_resolve: bad camera");
  if (n_poses == 0) return GS_OK;
  GS_REQUIRE(visbuf && image && w2c, "visbuf_resolve: null pointer");
  GS_REQUIRE(n_faces == 0 || (vertices && faces), "visbuf_resolve: null mesh");
  GS_REQUIRE(n_segments == 0 || line_colors, "visbuf_resolve: null line colours");
  ShadeArgs A;
  A.V = vertices; A.Fc = faces; A.w2c = w2c;
  A.vcol = vertex_colors; A.vnrm = vertex_normals; A.lcol = line_colors;
  A.nv = n_vertices; A.nf = n_faces; A.ns = n_segments; A.flat = (flat != 0 || !vertex_normals) ? 1 : 0;
  A.H = height; A.W = width;
  A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.ambient = ambient; A.diffuse = diffuse;
  A.background = background & 0xffffffu;
  const size_t npix = (size_t)n_poses * height * width;
  GS_TIMING_PRE();
  visbuf_resolve_kernel<<<(unsigned)((npix + RS_BLOCK - 1) / RS_BLOCK), RS_BLOCK, 0, (hipStream_t)stream>>>(visbuf, npix,
                                                                                                          A, image);
  GS_CHECK_LAUNCH("visbuf_resolve");
  return GS_OK;
}
