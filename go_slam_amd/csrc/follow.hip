// Sampled-rollout (MPPI) controller over the distance field and a cost-to-go field (no counterpart in the reference).
// Contract: include/goslam_hip.h (gs_follow_*); tests/follow_restatement.py restates it serially.  The rollout is fp32,
// one rounding per operation (-ffp-contract=off) and uses only + - * / floorf and comparisons, so its outputs equal the
// restatement's bit for bit; the weights and the update are fixed-order fp64 sums.
//
// follow_rollouts_kernel: one lane per rollout, one wave per workgroup (K = 4096 is 64 waves on 256 CUs: the kernel is a
//   chain of T dependent rounds of gathers and bound by their latency, measured 35 us at T = 32 for K = 256 as for
//   K = 16384; the lattice is not staged in LDS).  Step
//   t + 1's noise is loaded before step t's gathers are consumed; U and the parameters are wave-uniform (SGPRs).
// follow_weights_kernel: one workgroup; the minimum of (S, k) as one ordered 64-bit key, then omega, eta and ess.
// follow_update_kernel: one workgroup per step t; recomputes the applied perturbation with follow_control, the rollout's
//   own function, so nothing of size [T,K,2] is stored.
// Sums over k: a thread adds its strided elements in increasing k, a wave adds by the xor butterfly (both partners form
// the same sum), thread 0 adds the waves in increasing order: no atomics, the same bits every run.
// No inline assembly, no scratch, no dynamic LDS.
#include "common.h"
#include "tsdf_cell.h"

namespace {

constexpr int FOLLOW_ROLL_THREADS = GS_WAVE;
constexpr int FOLLOW_WEIGHT_THREADS = 1024;
constexpr int FOLLOW_UPDATE_THREADS = 256;
constexpr int FOLLOW_INF = 0x3fffffff;                      // GS_GEO_INF

struct FollowModel {                                        // by-value kernel argument (SGPRs)
  int up_axis;
  float height, dt, half_dt, v_max, w_max, reach, margin;  // reach = robot_radius + margin
  float w_togo, w_clear, w_turn, w_end, collision_cost, metres_per_milli;
};

// the control a rollout applies at a step: U + noise, a non-finite sum replaced by U, clamped by comparisons
__device__ __forceinline__ float2 follow_control(float2 u, float2 nz, float v_max, float w_max) {
  float v = u.x + nz.x, w = u.y + nz.y;
  if (!(fabsf(v) < INFINITY)) v = u.x;
  if (!(fabsf(w) < INFINITY)) w = u.y;
  v = v < 0.0f ? 0.0f : (v > v_max ? v_max : v);
  w = w < -w_max ? -w_max : (w > w_max ? w_max : w);
  return make_float2(v, w);
}

struct FollowSample { bool live; float togo_term, cost, d; };

// The point (x, y) of the plane of motion: has it a cell, may the robot's centre be at its nearest lattice point, and if
// so its to-go term, its step cost without the turn term and the trilinear distance.
__device__ __forceinline__ FollowSample follow_sample(const float* __restrict__ dist, const int* __restrict__ togo,
                                                      const TsdfLattice& lat, const FollowModel& m, float x, float y) {
  const float px = m.up_axis == 0 ? m.height : x;
  const float py = m.up_axis == 1 ? m.height : (m.up_axis == 0 ? x : y);
  const float pz = m.up_axis == 2 ? m.height : y;
  const float gx = (px - lat.lox) / lat.voxel, gy = (py - lat.loy) / lat.voxel, gz = (pz - lat.loz) / lat.voxel;
  const float ax = floorf(gx), ay = floorf(gy), az = floorf(gz);
  FollowSample r;
  r.live = false; r.togo_term = 0.0f; r.cost = 0.0f; r.d = 0.0f;
  if (!tsdf_cell_inside(lat, ax, ay, az)) return r;
  // 0 <= a <= n - 2 and g < n - 1, so floorf(g + 0.5) lies in [0, n - 1]
  const int ix = (int)floorf(gx + 0.5f), iy = (int)floorf(gy + 0.5f), iz = (int)floorf(gz + 0.5f);
  const int tv = togo[tsdf_cell_at<unsigned>(lat, ix, iy, iz)];
  const TsdfCorners c = tsdf_corners_load(dist, tsdf_cell_at<unsigned>(lat, (int)ax, (int)ay, (int)az), lat.ny, lat.nz);
  if (tv >= FOLLOW_INF) return r;
  r.live = true;
  r.d = tsdf_corners_value(c, gx - ax, gy - ay, gz - az);
  r.togo_term = m.w_togo * ((float)tv * m.metres_per_milli);
  r.cost = r.togo_term;
  if (r.d < m.reach) r.cost = r.cost + (m.w_clear * (m.reach - r.d)) / m.margin;
  return r;
}

__global__ __launch_bounds__(FOLLOW_ROLL_THREADS) void follow_rollouts_kernel(
    const float* __restrict__ dist, const int* __restrict__ togo, TsdfLattice lat, FollowModel m, float x0, float y0,
    float c0, float s0, const float2* __restrict__ U, const float2* __restrict__ noise, int K, int T,
    float* __restrict__ S, float* __restrict__ end, int* __restrict__ hit_step, float* __restrict__ min_dist) {
  const int k = blockIdx.x * FOLLOW_ROLL_THREADS + threadIdx.x;
  if (k >= K) return;
  float x = x0, y = y0, c = c0, s = s0;
  const FollowSample first = follow_sample(dist, togo, lat, m, x, y);
  float frozen = first.live ? first.cost : 0.0f;            // what a rollout stuck at its last good state pays per step
  float last_togo = first.togo_term;
  float sum = 0.0f, closest = INFINITY;
  int hit = T;
  float2 nz = noise[k];
  for (int t = 0; t < T; ++t) {
    const float2 nz_next = t + 1 < T ? noise[(t + 1) * K + k] : make_float2(0.0f, 0.0f);
    if (hit == T) {
      const float2 u = follow_control(U[t], nz, m.v_max, m.w_max);
      const float h = m.half_dt * u.y, hh = h * h, den = 1.0f + hh;
      const float cr = (1.0f - hh) / den, sr = (2.0f * h) / den;
      const float c1 = c * cr - s * sr, s1 = s * cr + c * sr;
      const float dv = m.dt * u.x;
      const float x1 = x + dv * c1, y1 = y + dv * s1;
      const FollowSample at = follow_sample(dist, togo, lat, m, x1, y1);
      if (at.live) {
        x = x1; y = y1; c = c1; s = s1;
        frozen = at.cost + m.w_turn * (u.y * u.y);
        last_togo = at.togo_term;
        closest = at.d < closest ? at.d : closest;
        sum = sum + frozen;
      } else {
        hit = t;
        sum = sum + m.collision_cost;
        sum = sum + frozen;
      }
    } else {
      sum = sum + frozen;
    }
    nz = nz_next;
  }
  if (hit == T) sum = sum + m.w_end * last_togo;
  S[k] = sum;
  end[(size_t)k * 4 + 0] = x; end[(size_t)k * 4 + 1] = y; end[(size_t)k * 4 + 2] = c; end[(size_t)k * 4 + 3] = s;
  hit_step[k] = hit;
  min_dist[k] = closest;
}

// a float's bits as an unsigned that orders as the float does (-0 below +0)
__device__ __forceinline__ unsigned follow_ordered(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float follow_unordered(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__global__ __launch_bounds__(FOLLOW_WEIGHT_THREADS) void follow_weights_kernel(const float* __restrict__ S, int K,
                                                                               double lambda, float* __restrict__ s_min,
                                                                               int* __restrict__ best,
                                                                               double* __restrict__ omega,
                                                                               double* __restrict__ stats) {
  constexpr int WAVES = FOLLOW_WEIGHT_THREADS / GS_WAVE;
  __shared__ unsigned long long keys[WAVES];
  __shared__ double sums[2][WAVES];
  const int tid = threadIdx.x, lane = tid & (GS_WAVE - 1), wave = tid / GS_WAVE;
  unsigned long long key = ~0ull;
  for (int k = tid; k < K; k += FOLLOW_WEIGHT_THREADS) {
    const unsigned long long cand = (unsigned long long)follow_ordered(S[k]) << 32 | (unsigned)k;
    key = cand < key ? cand : key;
  }
  key = gs_wave_min_u64(key);
  if (lane == 0) keys[wave] = key;
  __syncthreads();
  key = keys[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) key = keys[w] < key ? keys[w] : key;
  const float low = follow_unordered((unsigned)(key >> 32));
  double e1 = 0.0, e2 = 0.0;
  for (int k = tid; k < K; k += FOLLOW_WEIGHT_THREADS) {
    const double o = exp(-((double)S[k] - (double)low) / lambda);
    omega[k] = o;
    e1 += o;
    e2 += o * o;
  }
  e1 = gs_wave_sum_f64(e1);
  e2 = gs_wave_sum_f64(e2);
  if (lane == 0) {
    sums[0][wave] = e1;
    sums[1][wave] = e2;
  }
  __syncthreads();
  if (tid != 0) return;
  double eta = sums[0][0], sq = sums[1][0];
  for (int w = 1; w < WAVES; ++w) {
    eta += sums[0][w];
    sq += sums[1][w];
  }
  s_min[0] = low;
  best[0] = (int)(key & 0xffffffffu);
  stats[0] = eta;
  stats[1] = eta * eta / sq;
}

__global__ __launch_bounds__(FOLLOW_UPDATE_THREADS) void follow_update_kernel(
    const float2* __restrict__ U, const float2* __restrict__ noise, const double* __restrict__ omega,
    const double* __restrict__ stats, int K, int T, float v_max, float w_max, int shift, float2* __restrict__ U_new,
    float2* __restrict__ u_exec) {
  constexpr int WAVES = FOLLOW_UPDATE_THREADS / GS_WAVE;
  __shared__ double sums[2][WAVES];
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & (GS_WAVE - 1), wave = tid / GS_WAVE;
  const float2 u = U[t];
  double av = 0.0, aw = 0.0;
  for (int k = tid; k < K; k += FOLLOW_UPDATE_THREADS) {
    const float2 applied = follow_control(u, noise[t * K + k], v_max, w_max);
    const double o = omega[k];
    av += o * (double)(applied.x - u.x);
    aw += o * (double)(applied.y - u.y);
  }
  av = gs_wave_sum_f64(av);
  aw = gs_wave_sum_f64(aw);
  if (lane == 0) {
    sums[0][wave] = av;
    sums[1][wave] = aw;
  }
  __syncthreads();
  if (tid != 0) return;
  av = sums[0][0];
  aw = sums[1][0];
  for (int w = 1; w < WAVES; ++w) {
    av += sums[0][w];
    aw += sums[1][w];
  }
  const double eta = stats[0];
  float v = u.x + (float)(av / eta), w = u.y + (float)(aw / eta);
  v = v < 0.0f ? 0.0f : (v > v_max ? v_max : v);
  w = w < -w_max ? -w_max : (w > w_max ? w_max : w);
  const float2 row = make_float2(v, w);
  if (shift == 0) {
    U_new[t] = row;
  } else {
    if (t > 0) U_new[t - 1] = row;
    if (t == T - 1) U_new[t] = row;
  }
  if (t == 0 && u_exec) u_exec[0] = row;
}

bool follow_sizes_ok(int K, int T) { return K >= 1 && K <= GS_FOLLOW_MAX_ROLLOUTS && T >= 1 && T <= GS_FOLLOW_MAX_STEPS; }
bool follow_finite(float v) { return v > -INFINITY && v < INFINITY; }
bool follow_positive(float v) { return v > 0.0f && v < INFINITY; }
bool follow_weight(float v) { return v >= 0.0f && v < INFINITY; }

}  // namespace

extern "C" int gs_follow_rollouts(const float* dist, const int* togo, int n0, int n1, int n2, float lo_x, float lo_y,
                                  float lo_z, float voxel, int up_axis, float height, float x, float y, float c, float s,
                                  const float* U, const float* noise, int K, int T, float dt, float v_max, float w_max,
                                  float robot_radius, float margin, float w_togo, float w_clear, float w_turn,
                                  float w_end, float collision_cost, float* S, float* end, int* hit_step,
                                  float* min_dist, gs_stream_t stream) {
  GS_REQUIRE(tsdf_dims_ok(n0, n1, n2), "follow_rollouts: lattice %d x %d x %d outside [2, 1024]", n0, n1, n2);
  GS_REQUIRE(follow_sizes_ok(K, T), "follow_rollouts: K=%d (1 .. %d), T=%d (1 .. %d)", K, GS_FOLLOW_MAX_ROLLOUTS, T,
             GS_FOLLOW_MAX_STEPS);
  GS_REQUIRE(follow_positive(voxel) && follow_finite(lo_x) && follow_finite(lo_y) && follow_finite(lo_z),
             "follow_rollouts: voxel=%g lo=(%g, %g, %g)", voxel, lo_x, lo_y, lo_z);
  GS_REQUIRE(up_axis >= 0 && up_axis <= 2 && follow_finite(height), "follow_rollouts: up_axis=%d height=%g", up_axis,
             height);
  GS_REQUIRE(follow_finite(x) && follow_finite(y) && follow_finite(c) && follow_finite(s),
             "follow_rollouts: state (%g, %g, %g, %g) is not finite", x, y, c, s);
  GS_REQUIRE(follow_positive(dt) && follow_positive(v_max) && follow_positive(w_max) && follow_positive(margin) &&
                 follow_weight(robot_radius),
             "follow_rollouts: dt=%g v_max=%g w_max=%g margin=%g must be positive and finite, robot_radius=%g >= 0", dt,
             v_max, w_max, margin, robot_radius);
  GS_REQUIRE(follow_weight(w_togo) && follow_weight(w_clear) && follow_weight(w_turn) && follow_weight(w_end) &&
                 follow_weight(collision_cost),
             "follow_rollouts: weights (%g, %g, %g, %g) and collision_cost=%g must be finite and >= 0", w_togo, w_clear,
             w_turn, w_end, collision_cost);
  GS_REQUIRE(dist && togo && U && noise && S && end && hit_step && min_dist, "follow_rollouts: null pointer");
  GS_REQUIRE((uintptr_t)U % 8 == 0 && (uintptr_t)noise % 8 == 0, "follow_rollouts: U or noise is not 8-byte aligned");
  FollowModel m;
  m.up_axis = up_axis; m.height = height; m.dt = dt; m.half_dt = 0.5f * dt; m.v_max = v_max; m.w_max = w_max;
  m.reach = robot_radius + margin; m.margin = margin;
  m.w_togo = w_togo; m.w_clear = w_clear; m.w_turn = w_turn; m.w_end = w_end; m.collision_cost = collision_cost;
  m.metres_per_milli = voxel / 1000.0f;
  GS_TIMING_PRE();
  follow_rollouts_kernel<<<gs_cdiv(K, FOLLOW_ROLL_THREADS), FOLLOW_ROLL_THREADS, 0, (hipStream_t)stream>>>(
      dist, togo, tsdf_lattice(n0, n1, n2, lo_x, lo_y, lo_z, voxel), m, x, y, c, s, (const float2*)U,
      (const float2*)noise, K, T, S, end, hit_step, min_dist);
  GS_CHECK_LAUNCH("follow_rollouts");
  return GS_OK;
}

extern "C" int gs_follow_weights(const float* S, int K, float lambda, float* s_min, int* best, double* omega,
                                 double* stats, gs_stream_t stream) {
  GS_REQUIRE(K >= 1 && K <= GS_FOLLOW_MAX_ROLLOUTS, "follow_weights: K=%d (1 .. %d)", K, GS_FOLLOW_MAX_ROLLOUTS);
  GS_REQUIRE(follow_positive(lambda), "follow_weights: lambda=%g must be positive and finite", lambda);
  GS_REQUIRE(S && s_min && best && omega && stats, "follow_weights: null pointer");
  GS_REQUIRE((uintptr_t)omega % 8 == 0 && (uintptr_t)stats % 8 == 0, "follow_weights: omega or stats is not 8-byte aligned");
  GS_TIMING_PRE();
  follow_weights_kernel<<<1, FOLLOW_WEIGHT_THREADS, 0, (hipStream_t)stream>>>(S, K, (double)lambda, s_min, best, omega,
                                                                             stats);
  GS_CHECK_LAUNCH("follow_weights");
  return GS_OK;
}

extern "C" int gs_follow_update(const float* U, const float* noise, const double* omega, const double* stats, int K,
                                int T, float v_max, float w_max, int shift, float* U_new, float* u_exec,
                                gs_stream_t stream) {
  GS_REQUIRE(follow_sizes_ok(K, T), "follow_update: K=%d (1 .. %d), T=%d (1 .. %d)", K, GS_FOLLOW_MAX_ROLLOUTS, T,
             GS_FOLLOW_MAX_STEPS);
  GS_REQUIRE(follow_positive(v_max) && follow_positive(w_max), "follow_update: v_max=%g w_max=%g must be positive and finite",
             v_max, w_max);
  GS_REQUIRE(shift == 0 || shift == 1, "follow_update: shift=%d is not 0 or 1", shift);
  GS_REQUIRE(U && noise && omega && stats && U_new && (u_exec || shift == 0), "follow_update: null pointer");
  GS_REQUIRE(U_new != U, "follow_update: U_new must not be U (a shifted row lands in a row another workgroup reads)");
  GS_REQUIRE((uintptr_t)U % 8 == 0 && (uintptr_t)noise % 8 == 0 && (uintptr_t)U_new % 8 == 0 && (uintptr_t)u_exec % 8 == 0 &&
                 (uintptr_t)omega % 8 == 0 && (uintptr_t)stats % 8 == 0,
             "follow_update: a buffer is not 8-byte aligned");
  GS_TIMING_PRE();
  follow_update_kernel<<<T, FOLLOW_UPDATE_THREADS, 0, (hipStream_t)stream>>>(
      (const float2*)U, (const float2*)noise, omega, stats, K, T, v_max, w_max, shift, (float2*)U_new, (float2*)u_exec);
  GS_CHECK_LAUNCH("follow_update");
  return GS_OK;
}
