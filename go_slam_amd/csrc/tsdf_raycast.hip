// Raycast of the TSDF lattice of tsdf.hip: depth, normal and colour images from given camera poses (no counterpart in
// the reference).  Contract: include/goslam_hip.h (gs_tsdf_raycast, gs_tsdf_brick_flags);
// tests/tsdf_raycast_restatement.py restates it serially.  Compiled with -ffp-contract=off.
//
// tsdf_raycast_kernel: one lane per pixel, one wave per 8 x 8 pixel tile (a wave's rays stay in neighbouring cells, so
// its eight corner loads per sample fall into a few cache lines), one workgroup per tile and frame.  The frame's matrix
// sits at a wave-uniform address and is read by scalar loads; intrinsics and lattice constants are kernel arguments.
// No LDS, no atomics; every pixel is owned by one lane and every output is written by plain vector stores.  The march
// is a `for` over i up to the header's GS_TSDF_RAY_STEPS (an argument computed on the host): it ends whatever the pose
// holds.  With brick flags a sample in an unflagged brick is stepped over without touching tsdf or weight; the sample
// before a candidate far end is evaluated on demand (see the header for why this cannot change a result).
//
// tsdf_brick_flags_kernel: one wave per brick; lanes stride over the brick's up to 9^3 corner points, the wave votes.
#include "tsdf_cell.h"

namespace {

constexpr int RAY_TILE = 8;                 // pixels per side of a wave's tile
constexpr int RAY_THREADS = RAY_TILE * RAY_TILE;
constexpr int BRICK = 8;                    // cells per side of a brick

struct RayVol {            // by-value kernel arguments (SGPRs)
  TsdfLattice l;
  int nx;
  int by, bz;              // bricks along y and z
  float min_weight;
};

struct RayCell {
  size_t at;               // offset of corner (0,0,0)
  float sx, sy, sz;        // fractions
  int ax, ay, az;
};

// the cell of g: false unless g has one (tsdf_cell_inside)
__device__ __forceinline__ bool ray_cell(const RayVol v, float gx, float gy, float gz, RayCell& c) {
  const float ax = floorf(gx), ay = floorf(gy), az = floorf(gz);
  if (!tsdf_cell_inside(v.l, ax, ay, az)) return false;
  c.ax = (int)ax; c.ay = (int)ay; c.az = (int)az;
  c.at = tsdf_cell_at<size_t>(v.l, c.ax, c.ay, c.az);
  c.sx = gx - ax; c.sy = gy - ay; c.sz = gz - az;
  return true;
}

// sample(t) of the header: valid?, and the value
__device__ __forceinline__ bool ray_sample(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                           const RayVol v, const RayCell c, float& f) {
  if (!tsdf_corners_at_least(tsdf_corners_load(weight, c.at, v.l.ny, v.l.nz), v.min_weight)) return false;
  f = tsdf_corners_value(tsdf_corners_load(tsdf, c.at, v.l.ny, v.l.nz), c.sx, c.sy, c.sz);
  return true;
}

__device__ __forceinline__ bool ray_finite(float x) { return fabsf(x) < INFINITY; }

template <bool COLOR>
__global__ __launch_bounds__(RAY_THREADS) void tsdf_raycast_kernel(
    const float* __restrict__ tsdf, const float* __restrict__ weight, const float* __restrict__ colors,
    const unsigned char* __restrict__ flags, const float* __restrict__ c2w, RayVol v, int h, int w, int tiles_x,
    int tiles, float fx, float fy, float cx, float cy, float near, float far, float step, int max_steps,
    float* __restrict__ depth, float* __restrict__ normal, float* __restrict__ color) {
  const int frame = blockIdx.x / tiles;
  const int tile = blockIdx.x - frame * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int iu = tx * RAY_TILE + (threadIdx.x & (RAY_TILE - 1));
  const int iv = ty * RAY_TILE + (threadIdx.x >> 3);
  if (iu >= w || iv >= h) return;
  const float* __restrict__ m = c2w + (size_t)frame * 12;
  const size_t pix = ((size_t)frame * h + iv) * w + iu;

  float out_d = 0.0f, out_n[3] = {0.0f, 0.0f, 0.0f}, out_c[3] = {0.0f, 0.0f, 0.0f};
  do {                                                       // left by `break` on a miss
    const float dx = ((float)iu - cx) / fx, dy = ((float)iv - cy) / fy;
    const float dwx = (m[0] * dx + m[1] * dy) + m[2];
    const float dwy = (m[4] * dx + m[5] * dy) + m[6];
    const float dwz = (m[8] * dx + m[9] * dy) + m[10];
    const float ogx = (m[3] - v.l.lox) / v.l.voxel, ogy = (m[7] - v.l.loy) / v.l.voxel, ogz = (m[11] - v.l.loz) / v.l.voxel;
    const float dgx = dwx / v.l.voxel, dgy = dwy / v.l.voxel, dgz = dwz / v.l.voxel;
    if (!(ray_finite(ogx) && ray_finite(ogy) && ray_finite(ogz) && ray_finite(dgx) && ray_finite(dgy) &&
          ray_finite(dgz)))
      break;
    const float dt = (step * v.l.voxel) / sqrtf((dwx * dwx + dwy * dwy) + dwz * dwz);
    if (!(dt > 0.0f && dt < INFINITY)) break;
    float t0 = near, t1 = far;
    bool inside = true;
    {
      const float og[3] = {ogx, ogy, ogz}, dg[3] = {dgx, dgy, dgz}, top[3] = {v.l.topx, v.l.topy, v.l.topz};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (dg[a] == 0.0f) {
          inside = inside && (og[a] >= 0.0f && og[a] <= top[a]);
        } else {
          const float ta = (0.0f - og[a]) / dg[a], tb = (top[a] - og[a]) / dg[a];
          const float lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
          t0 = lo > t0 ? lo : t0;
          t1 = hi < t1 ? hi : t1;
        }
      }
    }
    if (!inside) break;

    bool hit = false, prev_known = false, prev_valid = false;
    float f_prev = 0.0f, t_star = 0.0f;
    for (int i = 0; i <= max_steps; ++i) {
      const float t = t0 + (float)i * dt;
      if (!(t < t1)) break;
      RayCell c;
      bool valid = ray_cell(v, ogx + t * dgx, ogy + t * dgy, ogz + t * dgz, c);
      if (valid && flags) {
        const size_t brick = ((size_t)(c.ax >> 3) * v.by + (c.ay >> 3)) * v.bz + (c.az >> 3);
        if (flags[brick] == 0) {             // every corner >= 0: f_i >= 0 or invalid, never the far end of a hit
          prev_known = false;
          continue;
        }
      }
      float f = 0.0f;
      if (valid) valid = ray_sample(tsdf, weight, v, c, f);
      if (valid && f < 0.0f && i >= 1) {
        const float tp = t0 + (float)(i - 1) * dt;
        if (!prev_known) {
          RayCell cp;
          prev_valid = ray_cell(v, ogx + tp * dgx, ogy + tp * dgy, ogz + tp * dgz, cp);
          if (prev_valid) prev_valid = ray_sample(tsdf, weight, v, cp, f_prev);
        }
        if (prev_valid && f_prev >= 0.0f) {
          t_star = tp + dt * (f_prev / (f_prev - f));
          hit = true;
          break;
        }
      }
      prev_known = true;
      prev_valid = valid;
      f_prev = f;
    }
    if (!hit) break;

    RayCell c;
    if (!ray_cell(v, ogx + t_star * dgx, ogy + t_star * dgy, ogz + t_star * dgz, c)) break;
    if (!tsdf_corners_at_least(tsdf_corners_load(weight, c.at, v.l.ny, v.l.nz), v.min_weight)) break;
    float n[3];
    tsdf_corners_gradient(tsdf_corners_load(tsdf, c.at, v.l.ny, v.l.nz), c.sx, c.sy, c.sz, n);
    const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    out_d = t_star;
    if (len > 0.0f) {
      out_n[0] = n[0] / len; out_n[1] = n[1] / len; out_n[2] = n[2] / len;
    }
    if (COLOR) {
      const size_t np = (size_t)v.nx * v.l.ny * v.l.nz;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        out_c[ch] = tsdf_corners_value(tsdf_corners_load(colors + ch * np, c.at, v.l.ny, v.l.nz), c.sx, c.sy, c.sz);
    }
  } while (false);

  depth[pix] = out_d;
  normal[pix * 3 + 0] = out_n[0];
  normal[pix * 3 + 1] = out_n[1];
  normal[pix * 3 + 2] = out_n[2];
  if (COLOR) {
    color[pix * 3 + 0] = out_c[0];
    color[pix * 3 + 1] = out_c[1];
    color[pix * 3 + 2] = out_c[2];
  }
}

__global__ __launch_bounds__(64) void tsdf_brick_flags_kernel(const float* __restrict__ tsdf, int nx, int ny, int nz,
                                                              int by, int bz, unsigned char* __restrict__ flags) {
  const int brick = blockIdx.x;
  const int bi = brick / (by * bz), rem = brick - bi * (by * bz);
  const int bj = rem / bz, bk = rem - bj * bz;
  const int x0 = bi * BRICK, y0 = bj * BRICK, z0 = bk * BRICK;
  const int ex = min(BRICK + 1, nx - x0), ey = min(BRICK + 1, ny - y0), ez = min(BRICK + 1, nz - z0);   // points per axis
  const int count = ex * ey * ez;
  bool neg = false;
  for (int p = threadIdx.x; p < count; p += 64) {
    const int i = p / (ey * ez), r = p - i * (ey * ez);
    const int j = r / ez, k = r - j * ez;
    neg = neg || tsdf[((size_t)(x0 + i) * ny + (y0 + j)) * nz + (z0 + k)] < 0.0f;
  }
  const bool any = __any(neg);
  if (threadIdx.x == 0) flags[brick] = any ? 1 : 0;
}

}  // namespace

extern "C" size_t gs_tsdf_brick_flags_bytes(int nx, int ny, int nz) {
  if (!tsdf_dims_ok(nx, ny, nz)) return 0;
  return (size_t)gs_cdiv(nx - 1, BRICK) * gs_cdiv(ny - 1, BRICK) * gs_cdiv(nz - 1, BRICK);
}

extern "C" int gs_tsdf_brick_flags(const float* tsdf, int nx, int ny, int nz, unsigned char* flags,
                                   gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_brick_flags: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(tsdf && flags, "tsdf_brick_flags: null pointer");
  const int by = gs_cdiv(ny - 1, BRICK), bz = gs_cdiv(nz - 1, BRICK);
  const unsigned bricks = (unsigned)gs_tsdf_brick_flags_bytes(nx, ny, nz);      // at most 128^3
  GS_TIMING_PRE();
  tsdf_brick_flags_kernel<<<bricks, 64, 0, (hipStream_t)stream>>>(tsdf, nx, ny, nz, by, bz, flags);
  GS_CHECK_LAUNCH("tsdf_brick_flags");
  return GS_OK;
}

extern "C" int gs_tsdf_raycast(const float* tsdf, const float* weight, const float* colors, int nx, int ny, int nz,
                               const unsigned char* flags, const float* c2w, int k, int h, int w, float fx, float fy,
                               float cx, float cy, float lo_x, float lo_y, float lo_z, float voxel, float near,
                               float far, float step_voxels, float min_weight, float* depth, float* normal,
                               float* color, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), "tsdf_raycast: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
  GS_REQUIRE(k >= 0 && h >= 1 && w >= 1, "tsdf_raycast: k=%d h=%d w=%d", k, h, w);
  GS_REQUIRE(step_voxels > 0.0f && step_voxels <= 1.0f, "tsdf_raycast: step_voxels=%g outside (0, 1]", step_voxels);
  GS_REQUIRE(voxel > 0.0f && voxel < INFINITY, "tsdf_raycast: voxel=%g", voxel);
  GS_REQUIRE(near >= 0.0f && far > near, "tsdf_raycast: near=%g far=%g (need 0 <= near < far)", near, far);
  GS_REQUIRE(fx != 0.0f && fy != 0.0f, "tsdf_raycast: fx=%g fy=%g", fx, fy);
  const double steps = ceil((double)(nx + ny + nz) / (double)step_voxels) + 2.0;
  GS_REQUIRE(steps <= 16777216.0, "tsdf_raycast: step_voxels=%g needs %.0f steps (at most 2^24)", step_voxels, steps);
  GS_REQUIRE(!color || colors, "tsdf_raycast: a colour image without a colour lattice");
  if (k == 0) return GS_OK;
  GS_REQUIRE(tsdf && weight && c2w && depth && normal, "tsdf_raycast: null pointer");
  const int tiles_x = gs_cdiv(w, RAY_TILE), tiles_y = gs_cdiv(h, RAY_TILE);
  const long long tiles = (long long)tiles_x * tiles_y, blocks = tiles * k;
  GS_REQUIRE(blocks <= 0x7fffffffLL, "tsdf_raycast: %d frames of %d x %d pixels are too many for one launch", k, h, w);
  RayVol v;
  v.l = tsdf_lattice(nx, ny, nz, lo_x, lo_y, lo_z, voxel);
  v.nx = nx;
  v.by = gs_cdiv(ny - 1, BRICK); v.bz = gs_cdiv(nz - 1, BRICK);
  v.min_weight = min_weight;
  GS_TIMING_PRE();
  if (color)
    tsdf_raycast_kernel<true><<<(unsigned)blocks, RAY_THREADS, 0, (hipStream_t)stream>>>(
        tsdf, weight, colors, flags, c2w, v, h, w, tiles_x, (int)tiles, fx, fy, cx, cy, near, far, step_voxels,
        (int)steps, depth, normal, color);
  else
    tsdf_raycast_kernel<false><<<(unsigned)blocks, RAY_THREADS, 0, (hipStream_t)stream>>>(
        tsdf, weight, nullptr, flags, c2w, v, h, w, tiles_x, (int)tiles, fx, fy, cx, cy, near, far, step_voxels,
        (int)steps, depth, normal, nullptr);
  GS_CHECK_LAUNCH("tsdf_raycast");
  return GS_OK;
}
