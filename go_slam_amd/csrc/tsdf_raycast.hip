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
#include "common.h"

namespace {

constexpr int RAY_TILE = 8;                 // pixels per side of a wave's tile
constexpr int RAY_THREADS = RAY_TILE * RAY_TILE;
constexpr int BRICK = 8;                    // cells per side of a brick

struct RayVol {            // by-value kernel arguments (SGPRs)
  int nx, ny, nz;
  int by, bz;              // bricks along y and z
  float topx, topy, topz;  // float(n - 1)
  float lox, loy, loz, voxel;
  float min_weight;
};

struct RayCell {
  size_t at;               // offset of corner (0,0,0)
  float sx, sy, sz;        // fractions
  int ax, ay, az;
};

// the cell of g: false unless 0 <= floorf(g) < n - 1 on every axis (NaN fails), compared before the casts
__device__ __forceinline__ bool ray_cell(const RayVol v, float gx, float gy, float gz, RayCell& c) {
  const float ax = floorf(gx), ay = floorf(gy), az = floorf(gz);
  if (!(ax >= 0.0f && ax < v.topx && ay >= 0.0f && ay < v.topy && az >= 0.0f && az < v.topz)) return false;
  c.ax = (int)ax; c.ay = (int)ay; c.az = (int)az;
  c.at = ((size_t)c.ax * v.ny + c.ay) * v.nz + c.az;
  c.sx = gx - ax; c.sy = gy - ay; c.sz = gz - az;
  return true;
}

__device__ __forceinline__ float ray_lerp(float p, float q, float s) { return p + s * (q - p); }

struct RayCorners { float v000, v001, v010, v011, v100, v101, v110, v111; };   // v[x][y][z]

__device__ __forceinline__ RayCorners ray_load(const float* __restrict__ p, size_t at, int ny, int nz) {
  const size_t sy = (size_t)nz, sx = (size_t)ny * nz;
  RayCorners c;
  c.v000 = p[at];           c.v001 = p[at + 1];
  c.v010 = p[at + sy];      c.v011 = p[at + sy + 1];
  c.v100 = p[at + sx];      c.v101 = p[at + sx + 1];
  c.v110 = p[at + sx + sy]; c.v111 = p[at + sx + sy + 1];
  return c;
}

__device__ __forceinline__ bool ray_seen(const RayCorners w, float m) {
  return w.v000 >= m && w.v001 >= m && w.v010 >= m && w.v011 >= m && w.v100 >= m && w.v101 >= m && w.v110 >= m &&
         w.v111 >= m;
}

// lerps along z (four), then y (two), then x (one)
__device__ __forceinline__ float ray_trilinear(const RayCorners c, float sx, float sy, float sz) {
  const float c00 = ray_lerp(c.v000, c.v001, sz), c01 = ray_lerp(c.v010, c.v011, sz);
  const float c10 = ray_lerp(c.v100, c.v101, sz), c11 = ray_lerp(c.v110, c.v111, sz);
  return ray_lerp(ray_lerp(c00, c01, sy), ray_lerp(c10, c11, sy), sx);
}

// sample(t) of the header: valid?, and the value
__device__ __forceinline__ bool ray_sample(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                           const RayVol v, const RayCell c, float& f) {
  if (!ray_seen(ray_load(weight, c.at, v.ny, v.nz), v.min_weight)) return false;
  f = ray_trilinear(ray_load(tsdf, c.at, v.ny, v.nz), c.sx, c.sy, c.sz);
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
    const float ogx = (m[3] - v.lox) / v.voxel, ogy = (m[7] - v.loy) / v.voxel, ogz = (m[11] - v.loz) / v.voxel;
    const float dgx = dwx / v.voxel, dgy = dwy / v.voxel, dgz = dwz / v.voxel;
    if (!(ray_finite(ogx) && ray_finite(ogy) && ray_finite(ogz) && ray_finite(dgx) && ray_finite(dgy) &&
          ray_finite(dgz)))
      break;
    const float dt = (step * v.voxel) / sqrtf((dwx * dwx + dwy * dwy) + dwz * dwz);
    if (!(dt > 0.0f && dt < INFINITY)) break;
    float t0 = near, t1 = far;
    bool inside = true;
    {
      const float og[3] = {ogx, ogy, ogz}, dg[3] = {dgx, dgy, dgz}, top[3] = {v.topx, v.topy, v.topz};
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
    if (!ray_seen(ray_load(weight, c.at, v.ny, v.nz), v.min_weight)) break;
    const RayCorners s = ray_load(tsdf, c.at, v.ny, v.nz);
    // z-lerps of the four z-edges, y-lerps of the four y-edges
    const float z00 = ray_lerp(s.v000, s.v001, c.sz), z01 = ray_lerp(s.v010, s.v011, c.sz);
    const float z10 = ray_lerp(s.v100, s.v101, c.sz), z11 = ray_lerp(s.v110, s.v111, c.sz);
    const float y00 = ray_lerp(s.v000, s.v010, c.sy), y01 = ray_lerp(s.v001, s.v011, c.sy);
    const float y10 = ray_lerp(s.v100, s.v110, c.sy), y11 = ray_lerp(s.v101, s.v111, c.sy);
    const float nx = ray_lerp(z10, z11, c.sy) - ray_lerp(z00, z01, c.sy);
    const float ny = ray_lerp(z01, z11, c.sx) - ray_lerp(z00, z10, c.sx);
    const float nz = ray_lerp(y01, y11, c.sx) - ray_lerp(y00, y10, c.sx);
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    out_d = t_star;
    if (len > 0.0f) {
      out_n[0] = nx / len; out_n[1] = ny / len; out_n[2] = nz / len;
    }
    if (COLOR) {
      const size_t np = (size_t)v.nx * v.ny * v.nz;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        out_c[ch] = ray_trilinear(ray_load(colors + ch * np, c.at, v.ny, v.nz), c.sx, c.sy, c.sz);
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

bool ray_dims_ok(int nx, int ny, int nz) {
  return nx >= 2 && nx <= 1024 && ny >= 2 && ny <= 1024 && nz >= 2 && nz <= 1024;
}

}  // namespace

extern "C" size_t gs_tsdf_brick_flags_bytes(int nx, int ny, int nz) {
  if (!ray_dims_ok(nx, ny, nz)) return 0;
  return (size_t)gs_cdiv(nx - 1, BRICK) * gs_cdiv(ny - 1, BRICK) * gs_cdiv(nz - 1, BRICK);
}

extern "C" int gs_tsdf_brick_flags(const float* tsdf, int nx, int ny, int nz, unsigned char* flags,
                                   gs_stream_t stream) {
  GS_REQUIRE(ray_dims_ok(nx, ny, nz), "tsdf_brick_flags: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
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
  GS_REQUIRE(ray_dims_ok(nx, ny, nz), "tsdf_raycast: lattice %d x %d x %d outside [2, 1024]", nx, ny, nz);
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
  v.nx = nx; v.ny = ny; v.nz = nz;
  v.by = gs_cdiv(ny - 1, BRICK); v.bz = gs_cdiv(nz - 1, BRICK);
  v.topx = (float)(nx - 1); v.topy = (float)(ny - 1); v.topz = (float)(nz - 1);
  v.lox = lo_x; v.loy = lo_y; v.loz = lo_z; v.voxel = voxel;
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
