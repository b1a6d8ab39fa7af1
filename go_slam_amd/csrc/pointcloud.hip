// Keyframe point cloud (droid_visualization's data path, src/visualization.py:104-150): depth_filter's multi-view
// count, the keep mask, iproj and the colour gather fused into three launches that write only the surviving points --
// count, scan, emit, as mesh.hip does for marching cubes.  Contract and ordering: include/goslam_hip.h.
//
// A workgroup owns a tile of PC_TILE consecutive pixels of one listed keyframe (grid = (tiles, keyframes)), so the
// workgroups in linear order (list position, tile) are the output order.  The count pass leaves one 64-bit keep word
// per wave and iteration (a ballot) and the tile's survivor count; the scan turns the counts into each tile's first
// output slot; the emit pass finds a pixel's slot from the tile's base, the popcounts of the tile's earlier words and
// the lanes below it in its own word.  No atomics, so the order is fixed.  Compiled with -ffp-contract=off: the count
// and the back-projection are geom_common.h's, the same code gs_depth_filter and gs_iproj run.
#include "geom_common.h"

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_ITERS = 4;                              // pixels per lane
constexpr int PC_TILE = PC_THREADS * PC_ITERS;           // pixels per workgroup
constexpr int PC_WORDS = PC_TILE / 64;                   // keep words per workgroup
constexpr int PC_SCAN_THREADS = 1024;

struct PcLayout {                    // workspace carve-up (gs_pointcloud_workspace_bytes)
  unsigned long long* words;         // per workgroup PC_WORDS keep words; bit l of word i*4+w = pixel i*256 + w*64 + l
  unsigned* count;                   // per workgroup: survivors
  long long* base;                   // per workgroup: its first output slot (scan)
  size_t bytes;
};

PcLayout pc_layout(void* ws, size_t nblk) {
  char* b = (char*)ws;
  PcLayout L;
  size_t o = 0;
  L.words = (unsigned long long*)(b + o); o += gs_align(nblk * PC_WORDS * 8);
  L.count = (unsigned*)(b + o);           o += gs_align(nblk * 4);
  L.base = (long long*)(b + o);           o += gs_align(nblk * 8);
  L.bytes = o;
  return L;
}

bool pc_shape_ok(int k, int h, int w) {
  if (k < 0 || k > 65535 || h <= 0 || w <= 0) return false;
  const long long hw = (long long)h * w;
  if (hw > (1LL << 30)) return false;
  return (long long)k * ((hw + PC_TILE - 1) / PC_TILE) <= (1LL << 30);
}

// The ballot words of one iteration and the workgroup's survivor count (thread 0 writes it).
__device__ __forceinline__ void pc_store_word(bool keep, int i, unsigned long long* words, unsigned& n) {
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) words[i * 4 + (threadIdx.x >> 6)] = m;
  n += (unsigned)__popcll(m);
}

__device__ __forceinline__ void pc_store_count(unsigned n, unsigned* count, size_t blk) {
  __shared__ unsigned lds[PC_THREADS / 64];
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) count[blk] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// keep = (depth_filter count >= visible_num) & (disparity > disp_floor[b]); the count is only evaluated where the
// disparity test passes (the conjunction is the same).
__global__ __launch_bounds__(PC_THREADS) void pc_count_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intr,
    const int64_t* __restrict__ index, const float* __restrict__ disp_floor, float thresh, float visible_num, int num,
    int hw, int ht, int wd, unsigned long long* __restrict__ words, unsigned* __restrict__ count) {
  const int b = blockIdx.y;
  const size_t blk = (size_t)b * gridDim.x + blockIdx.x;
  const long long ix = index[b];
  const bool ok = ix >= 0 && ix < num;
  const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
  const float floor_b = disp_floor[b];
  unsigned n = 0;
#pragma unroll
  for (int i = 0; i < PC_ITERS; ++i) {
    const int p = blockIdx.x * PC_TILE + i * PC_THREADS + threadIdx.x;
    bool keep = false;
    if (ok && p < hw && disps[(size_t)ix * hw + p] > floor_b)
      keep = gs_depth_filter_count(poses, disps, (int)ix, p, fx, fy, cx, cy, thresh, num, hw, ht, wd) >= visible_num;
    pc_store_word(keep, i, words + blk * PC_WORDS, n);
  }
  pc_store_count(n, count, blk);
}

// keep = mask != 0 (the mask's bool(): NaN keeps).
__global__ __launch_bounds__(PC_THREADS) void pc_mask_kernel(
    const float* __restrict__ mask, const int64_t* __restrict__ index, int num, int hw,
    unsigned long long* __restrict__ words, unsigned* __restrict__ count) {
  const int b = blockIdx.y;
  const size_t blk = (size_t)b * gridDim.x + blockIdx.x;
  const long long ix = index[b];
  const bool ok = ix >= 0 && ix < num;
  unsigned n = 0;
#pragma unroll
  for (int i = 0; i < PC_ITERS; ++i) {
    const int p = blockIdx.x * PC_TILE + i * PC_THREADS + threadIdx.x;
    const bool keep = ok && p < hw && mask[(size_t)ix * hw + p] != 0.0f;
    pc_store_word(keep, i, words + blk * PC_WORDS, n);
  }
  pc_store_count(n, count, blk);
}

// One workgroup: every thread sums a contiguous run of the workgroup counts, the runs' exclusive prefix, then each run
// is walked again writing the bases.  offsets[b] = base of keyframe b's first tile, offsets[k] = the grand total.
__global__ __launch_bounds__(PC_SCAN_THREADS) void pc_scan_kernel(const unsigned* __restrict__ count,
                                                                 long long* __restrict__ base, int nblk, int tiles,
                                                                 int k, long long* __restrict__ offsets) {
  __shared__ unsigned long long lds[PC_SCAN_THREADS / 64];
  const int per = (nblk + PC_SCAN_THREADS - 1) / PC_SCAN_THREADS;
  const int lo = min(nblk, (int)threadIdx.x * per), hi = min(nblk, lo + per);
  unsigned long long s = 0;
  for (int i = lo; i < hi; ++i) s += count[i];
  // exclusive prefix of s over the workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long inc = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  unsigned long long run = inc - s, total = 0;
#pragma unroll
  for (int w = 0; w < PC_SCAN_THREADS / 64; ++w) {
    run += (w < wave) ? lds[w] : 0ull;
    total += lds[w];
  }
  for (int i = lo; i < hi; ++i) {
    base[i] = (long long)run;
    if (i % tiles == 0) offsets[i / tiles] = (long long)run;
    run += count[i];
  }
  if (threadIdx.x == 0) offsets[k] = (long long)total;
}

// Surviving pixel -> points[o] = iproj of its disparity through poses_inv[b], colors[o] = images[ix][:, p].
__global__ __launch_bounds__(PC_THREADS) void pc_emit_kernel(
    const float* __restrict__ poses_inv, const float* __restrict__ disps, const float* __restrict__ intr,
    const float* __restrict__ images, const int64_t* __restrict__ index, int num, int hw, int wd,
    const unsigned long long* __restrict__ words, const long long* __restrict__ base, long long n_points,
    float* __restrict__ points, float* __restrict__ colors) {
  __shared__ unsigned long long w[PC_WORDS];
  const int b = blockIdx.y;
  const size_t blk = (size_t)b * gridDim.x + blockIdx.x;
  if (threadIdx.x < PC_WORDS) w[threadIdx.x] = words[blk * PC_WORDS + threadIdx.x];
  __syncthreads();
  const long long ix = index[b];
  if (ix < 0 || ix >= num) return;   // the count pass kept nothing there
  float t[3], q[4];
  gs_load_pose(poses_inv, b, t, q);
  const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long o0 = base[blk];
  const float* img = images + (size_t)ix * 3 * hw;
#pragma unroll
  for (int i = 0; i < PC_ITERS; ++i) {
    const int wi = i * 4 + wave;
    const unsigned long long word = w[wi];
    if (!((word >> lane) & 1ull)) continue;
    unsigned before = 0;
    for (int j = 0; j < wi; ++j) before += (unsigned)__popcll(w[j]);
    const long long o = o0 + before + __popcll(word & ((1ull << lane) - 1ull));
    if (o >= n_points) continue;
    const int p = blockIdx.x * PC_TILE + i * PC_THREADS + threadIdx.x;
    float* pt = points + (size_t)o * 3;
    gs_iproj_point(t, q, fx, fy, cx, cy, (float)(p % wd), (float)(p / wd), disps[(size_t)ix * hw + p], pt);
    float* cl = colors + (size_t)o * 3;
    cl[0] = img[p];
    cl[1] = img[(size_t)hw + p];
    cl[2] = img[(size_t)2 * hw + p];
  }
}

int pc_tiles(int h, int w) { return gs_cdiv(h * w, PC_TILE); }

}  // namespace

#define GS_PC_LAYOUT(name)                                                                                   \
  GS_REQUIRE(pc_shape_ok(k, h, w), name ": bad shape k=%d h=%d w=%d", k, h, w);                              \
  const int tiles = pc_tiles(h, w);                                                                          \
  const int nblk = k * tiles;                                                                                \
  const PcLayout L = pc_layout(const_cast<void*>((const void*)workspace), (size_t)nblk);                     \
  if (workspace_bytes < L.bytes) {                                                                           \
    gs_set_error(name ": workspace %zu < %zu bytes", workspace_bytes, L.bytes);                             \
    return GS_ERR_WORKSPACE;                                                                                 \
  }

extern "C" size_t gs_pointcloud_workspace_bytes(int k, int h, int w) {
  if (!pc_shape_ok(k, h, w)) return 0;
  return pc_layout(nullptr, (size_t)k * pc_tiles(h, w)).bytes;
}

extern "C" int gs_pointcloud_count(const float* poses, const float* disps, const float* intrinsics,
                                   const int64_t* index, const float* disp_floor, float thresh, float visible_num,
                                   int k, int num, int h, int w, void* workspace, size_t workspace_bytes,
                                   gs_stream_t stream) {
  GS_REQUIRE(poses && disps && intrinsics && index && disp_floor && workspace, "pointcloud_count: null pointer");
  GS_REQUIRE(num > 0, "pointcloud_count: num=%d", num);
  GS_PC_LAYOUT("pointcloud_count");
  if (k == 0) return GS_OK;
  GS_TIMING_PRE();
  pc_count_kernel<<<dim3(tiles, k), PC_THREADS, 0, (hipStream_t)stream>>>(
      poses, disps, intrinsics, index, disp_floor, thresh, visible_num, num, h * w, h, w, L.words, L.count);
  GS_CHECK_LAUNCH("pointcloud_count");
  return GS_OK;
}

extern "C" int gs_pointcloud_mask(const float* mask, const int64_t* index, int k, int num, int h, int w,
                                  void* workspace, size_t workspace_bytes, gs_stream_t stream) {
  GS_REQUIRE(mask && index && workspace, "pointcloud_mask: null pointer");
  GS_REQUIRE(num > 0, "pointcloud_mask: num=%d", num);
  GS_PC_LAYOUT("pointcloud_mask");
  if (k == 0) return GS_OK;
  GS_TIMING_PRE();
  pc_mask_kernel<<<dim3(tiles, k), PC_THREADS, 0, (hipStream_t)stream>>>(mask, index, num, h * w, L.words, L.count);
  GS_CHECK_LAUNCH("pointcloud_mask");
  return GS_OK;
}

extern "C" int gs_pointcloud_scan(int k, int h, int w, void* workspace, size_t workspace_bytes, long long* offsets,
                                  gs_stream_t stream) {
  GS_REQUIRE(workspace && offsets, "pointcloud_scan: null pointer");
  GS_PC_LAYOUT("pointcloud_scan");
  GS_TIMING_PRE();
  pc_scan_kernel<<<1, PC_SCAN_THREADS, 0, (hipStream_t)stream>>>(L.count, L.base, nblk, tiles, k, offsets);
  GS_CHECK_LAUNCH("pointcloud_scan");
  return GS_OK;
}

extern "C" int gs_pointcloud_emit(const float* poses_inv, const float* disps, const float* intrinsics,
                                  const float* images, const int64_t* index, int k, int num, int h, int w,
                                  const void* workspace, size_t workspace_bytes, long long n_points, float* points,
                                  float* colors, gs_stream_t stream) {
  GS_REQUIRE(poses_inv && disps && intrinsics && images && index && workspace, "pointcloud_emit: null pointer");
  GS_REQUIRE(num > 0 && n_points >= 0, "pointcloud_emit: num=%d n_points=%lld", num, n_points);
  GS_REQUIRE(n_points == 0 || (points && colors), "pointcloud_emit: null output");
  GS_PC_LAYOUT("pointcloud_emit");
  if (k == 0 || n_points == 0) return GS_OK;
  GS_TIMING_PRE();
  pc_emit_kernel<<<dim3(tiles, k), PC_THREADS, 0, (hipStream_t)stream>>>(
      poses_inv, disps, intrinsics, images, index, num, h * w, w, L.words, L.base, n_points, points, colors);
  GS_CHECK_LAUNCH("pointcloud_emit");
  return GS_OK;
}
