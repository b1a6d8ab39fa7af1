// Helpers shared by the NeuS kernels (neus.hip, neus_bwd.hip, grid_autograd.hip, render_img.hip): the wave-merged table-gradient scatter, the per-ray sample placement and the piece layout of a segmented call.
#pragma once
#include "common.h"
#include "grid_cell.h"
#include "../../include/goslam_neus.h"

namespace {

// sin / cos of a Fourier-feature argument (InstantNeuS.py:64,72,177,196: `torch.sin(x @ _B)`, _B = 25 * randn -- arguments
// of a few hundred radians).  The forward rounds the value to fp16 at once (it is a colour-MLP input) and the backward's
// d arg row is fp16 as well, so libm's sinf / cosf -- ~40 VALU instructions each on its small-argument path, 33 per point:
// a quarter of the forward point stage's arithmetic -- buy nothing: two-term Cody-Waite reduction to [-pi, pi]
// (k * 6.28125 is exact for |k| < 2^16, the remainder of 2 pi follows in a second fma: reduction error < 3e-7 rad for
// |x| < 1e4) and the hardware's v_sin_f32 / v_cos_f32 (argument in revolutions): 6 instructions, |error| < 2e-6 against
// libm on [-1e3, 1e3] (tests/test_neus_gpu.py::test_embedding_sine_*), i.e. below 1 / 100 of an fp16 ulp at 1.
__device__ __forceinline__ float emb_reduce(float x) {
  const float k = __builtin_rintf(x * 0.15915494309189535f);
  float r = fmaf(-k, 6.28125f, x);
  r = fmaf(-k, 1.9353071795864769e-3f, r);
  return r * 0.15915494309189535f;                  // revolutions, |.| <= 1/2 (+ rounding)
}
__device__ __forceinline__ float emb_sin(float x) { return __builtin_amdgcn_sinf(emb_reduce(x)); }
__device__ __forceinline__ float emb_cos(float x) { return __builtin_amdgcn_cosf(emb_reduce(x)); }

// normalized_3d_coordinate (InstantNeuS.py:12-32) with the STATIC bound, clamped to [-1,1]; `view` = the grid's [0,1] input.
// `inside` (the clamp passes the gradient on [-1, 1]) and `span` make up the Jacobian d p / d x = inside * 2 / span, which
// every caller applies in its own operation order.
__device__ __forceinline__ void normalise_point(const float bound[6], const float pt[3], float p[3], float view[3],
                                                float inside[3], float span[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    span[d] = bound[2 * d + 1] - bound[2 * d];
    float q = (pt[d] - bound[2 * d]) / span[d] * 2.0f - 1.0f;
    inside[d] = (q >= -1.0f && q <= 1.0f) ? 1.0f : 0.0f;
    q = fminf(fmaxf(q, -1.0f), 1.0f);
    p[d] = q;
    view[d] = (q + 1.0f) / 2.0f;
  }
}

// NeuS (InstantNeuS.py:276-293): the SDF estimates half a step before / behind the sample and their sigmoid CDFs
__device__ __forceinline__ void neus_cdf_pair(float sdf, float iter_cos, float dist, float inv_s, float& est_prev,
                                              float& est_next, float& prev_cdf, float& next_cdf) {
  est_next = sdf + iter_cos * dist / 2.0f;
  est_prev = sdf - iter_cos * dist / 2.0f;
  prev_cdf = 1.0f / (1.0f + expf(-(est_prev * inv_s)));
  next_cdf = 1.0f / (1.0f + expf(-(est_next * inv_s)));
}

// Scatter one level's 8 corners x 2 features.  Lanes are consecutive samples of a ray, so
// neighbours often sit in the SAME cell (always at the coarse levels): runs of equal cells are
// pre-reduced inside the wave with a segmented scan and only the run's last lane issues atomics --
// at the coarse levels this removes ~10x of the (memory-side, heavily contended) atomic traffic.
// `tab16` != nullptr: tiny-cuda-nn's own accumulation mode -- the table gradient is fp16, both features
// of an entry go out as ONE packed atomic (global_atomic_pk_add_f16), pre-multiplied by the loss scale
// (tcnn: 128) so that small contributions stay above fp16's subnormal range; half the atomic count.
typedef _Float16 half2a __attribute__((ext_vector_type(2)));
// Runs of consecutive lanes in the same cell: inclusive segmented sum of the 8 x 2 corner contributions; returns
// whether this lane is the LAST of its run (the one that holds the run's total and emits it).
// value of the lane below (lane 0: its own) -- DPP wave_shr:1, one full-rate VALU move instead of the address arithmetic +
// ds_bpermute + LDS-return wait of __shfl_up(v, 1): the neighbour test and the scan's first (and at the fine levels only)
// step use 20 of them per level
__device__ __forceinline__ int wave_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float wave_shr1(float v) {
  return __builtin_bit_cast(float, wave_shr1(__builtin_bit_cast(int, v)));
}

__device__ __forceinline__ bool lvl_prereduce(float (&gacc)[8][2], const uint32_t (&gi)[3], bool on, int lane) {
  const uint32_t p0 = (uint32_t)wave_shr1((int)gi[0]), p1 = (uint32_t)wave_shr1((int)gi[1]), p2 = (uint32_t)wave_shr1((int)gi[2]);
  const int on_prev = wave_shr1((int)on);
  const bool same = (lane > 0) && on && on_prev && p0 == gi[0] && p1 == gi[1] && p2 == gi[2];
  const unsigned long long same_mask = __ballot(same);
  bool tail = true;
  if (same_mask != 0ull) {                            // wave-uniform
    const unsigned long long starts = ~same_mask;     // bit set where a run begins
    const unsigned long long below = starts & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
    const int run_start = 63 - __builtin_clzll(below);
    // (the scan stops as soon as no lane reaches back `off` lanes inside its run -- i.e. after ceil(log2(longest run)) of
    // the 6 doubling steps: skipping a step in which no lane takes anything changes nothing, and at the fine levels, where
    // runs are 2-3 lanes long, it saves 64-80 of the 96 cross-lane moves the backward's ISA count shows per level)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const bool take = (lane - off) >= run_start;
      if (__ballot(take) == 0ull) break;            // wave-uniform
      // all sixteen lane exchanges first, then ONE predicated block of adds (round 6: exchange + select + add per value
      // was 243 v_cndmask per level in the ISA -- half of this function's vector instructions)
      float u[8][2];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        u[c][0] = off == 1 ? wave_shr1(gacc[c][0]) : __shfl_up(gacc[c][0], off, 64);
        u[c][1] = off == 1 ? wave_shr1(gacc[c][1]) : __shfl_up(gacc[c][1], off, 64);
      }
      if (take) {
#pragma unroll
        for (int c = 0; c < 8; ++c) { gacc[c][0] += u[c][0]; gacc[c][1] += u[c][1]; }
      }
    }
    tail = (lane == 63) || (((starts >> (lane + 1)) & 1ull) != 0ull);
  }
  return tail;
}

__device__ __forceinline__ void lvl_scatter(float* __restrict__ tab, _Float16* __restrict__ tab16, float scale16,
                                            const uint32_t (&cidx)[8], float (&gacc)[8][2],
                                            const uint32_t (&gi)[3], bool on, int lane) {
  const bool tail = lvl_prereduce(gacc, gi, on, lane);
  if (tab16) {
    // The atomics are executed memory-side: every (lane, address) pair that is not merged in the TA costs a
    // fabric transaction, and 128 of them per point are what bound this kernel.  The two x-neighbours of a
    // cell (corners c, c^1) are ADJACENT table entries whenever the level is dense or x is even (the hash
    // multiplies x by 1), so lanes 2i / 2i+1 issue them in the SAME instruction -- first for point 2i, then
    // for point 2i+1 -- which lets the hardware merge the pair into one 64-byte request.
    const bool act = on && tail;
#pragma unroll
    for (int cp = 0; cp < 4; ++cp) {
      const int c0 = 2 * cp, c1 = 2 * cp + 1;
      const half2a v0 = {(_Float16)(gacc[c0][0] * scale16), (_Float16)(gacc[c0][1] * scale16)};
      const half2a v1 = {(_Float16)(gacc[c1][0] * scale16), (_Float16)(gacc[c1][1] * scale16)};
      const int u0 = __builtin_bit_cast(int, v0), u1 = __builtin_bit_cast(int, v1);
      const int a0 = (act && (gacc[c0][0] != 0.0f || gacc[c0][1] != 0.0f)) ? 1 : 0;
      const int a1 = (act && (gacc[c1][0] != 0.0f || gacc[c1][1] != 0.0f)) ? 1 : 0;
      const int i0 = (int)cidx[c0], i1 = (int)cidx[c1];
      const bool odd = lane & 1;
      // round A: point 2i -- even lane its own c0, odd lane the even neighbour's c1
      {
        const int ni = __builtin_amdgcn_mov_dpp(i1, 0xA0, 0xf, 0xf, true);     // quad_perm [0,0,2,2]
        const int nu = __builtin_amdgcn_mov_dpp(u1, 0xA0, 0xf, 0xf, true);
        const int na = __builtin_amdgcn_mov_dpp(a1, 0xA0, 0xf, 0xf, true);
        const int idx = odd ? ni : i0, uu = odd ? nu : u0, aa = odd ? na : a0;
        if (aa)
          __builtin_amdgcn_global_atomic_fadd_v2f16(
              (__attribute__((address_space(1))) half2a*)(tab16 + (size_t)(uint32_t)idx * 2), __builtin_bit_cast(half2a, uu));
      }
      // round B: point 2i+1 -- odd lane its own c1, even lane the odd neighbour's c0
      {
        const int ni = __builtin_amdgcn_mov_dpp(i0, 0xF5, 0xf, 0xf, true);     // quad_perm [1,1,3,3]
        const int nu = __builtin_amdgcn_mov_dpp(u0, 0xF5, 0xf, 0xf, true);
        const int na = __builtin_amdgcn_mov_dpp(a0, 0xF5, 0xf, 0xf, true);
        const int idx = odd ? i1 : ni, uu = odd ? u1 : nu, aa = odd ? a1 : na;
        if (aa)
          __builtin_amdgcn_global_atomic_fadd_v2f16(
              (__attribute__((address_space(1))) half2a*)(tab16 + (size_t)(uint32_t)idx * 2), __builtin_bit_cast(half2a, uu));
      }
    }
  } else if (on && tail) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float* gp = tab + (size_t)cidx[c] * 2;
      if (gacc[c][0] != 0.0f) atomicAdd(gp, gacc[c][0]);
      if (gacc[c][1] != 0.0f) atomicAdd(gp + 1, gacc[c][1]);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Sample placement of ONE ray by one wave (Renderer.render_batch_ray, src/render.py:99-171): ray/AABB far bound,
// stratified + near-surface samples, the merge of the two sorted runs (= the reference's torch.sort), dists.  Shared by
// gs_render_sample's wave kernel (one batch) and the whole-image sampler of render_img.hip (many batches), so that both
// place bit-identical samples from the same ray, batch maximum and perturbation row.  n_samples, n_surface <= 64: lane j
// owns stratified sample j and near-surface sample j; the merge position of each is its index plus its rank in the other
// run (ties resolved like the sequential merge: stratified first).  `sa`, `sb`, `sz`: the wave's own LDS rows (64, 64,
// 128 floats).  Every wave of the workgroup that has a ray must call this (it holds two workgroup barriers).
__device__ __forceinline__ void gs_place_ray_wave(const float o[3], const float d[3], const float* __restrict__ bound,
                                                  bool has_depth, float gd, float gt_max,
                                                  const float* __restrict__ t_samples, const float* __restrict__ t_surface,
                                                  const float* __restrict__ perturb, int ns, int nsurf,
                                                  float* sa, float* sb, float* sz,
                                                  float* __restrict__ zo, float* __restrict__ dd, int lane) {
  // far_bb = min_dim max((b0-o)/d, (b1-o)/d) + 0.01        (render.py:112-118; torch.max / torch.min propagate NaN)
  float far_bb = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float t0 = (bound[2 * k + 0] - o[k]) / d[k];
    const float t1 = (bound[2 * k + 1] - o[k]) / d[k];
    const float tm = (t0 != t0 || t1 != t1) ? NAN : fmaxf(t0, t1);
    far_bb = (tm != tm || far_bb != far_bb) ? NAN : fminf(far_bb, tm);
  }
  far_bb = far_bb + 0.01f;
  float nearv, farv;
  if (has_depth) {
    nearv = gd * 0.01f;
    farv = fminf(fmaxf(far_bb, 0.0f), gt_max * 1.2f);     // torch.clamp(far_bb, 0, max)
    if (far_bb != far_bb) farv = far_bb;
  } else {
    nearv = 0.01f;
    farv = far_bb;
    nsurf = 0;
  }
  const int total = ns + nsurf;
  const float span = farv - nearv;
  auto zu = [&](int j) { return nearv + span * t_samples[j]; };
  // (descending runs -- far < near, or no-depth rays under a batch maximum below 0.001 -- are walked backwards: the
  // merge below then equals the reference's sort in those degenerate cases too; without near-surface samples the
  // reference does not sort, render.py:162, and the run is left as it is)
  const bool rev_a = span < 0.0f && nsurf > 0, rev_b = !(gd > 0.0f) && gt_max < 0.001f;
  float za = INFINITY, zb = INFINITY;
  if (lane < ns) {
    const int j = rev_a ? ns - 1 - lane : lane;
    float z = zu(j);
    if (perturb) {
      const float lo = (j == 0) ? z : 0.5f * (zu(j - 1) + z);
      const float hi = (j == ns - 1) ? z : 0.5f * (z + zu(j + 1));
      z = lo + (hi - lo) * perturb[j];
    }
    za = z;
  }
  if (lane < nsurf) {
    const float t = t_surface[rev_b ? nsurf - 1 - lane : lane];
    if (gd > 0.0f) {
      const float snr = (1.0f - 0.1f) * gd, sfar = (1.0f + 0.1f) * gd;
      zb = (snr + (sfar - snr) * t) * 1.0f + (0.001f + (gt_max - 0.001f) * t) * (1.0f - 1.0f);
    } else {
      const float vd = gd * 0.0f;
      const float snr = (1.0f - 0.1f) * vd, sfar = (1.0f + 0.1f) * vd;
      zb = (snr + (sfar - snr) * t) * 0.0f + (0.001f + (gt_max - 0.001f) * t) * (1.0f - 0.0f);
    }
  }
  sa[lane] = za;
  sb[lane] = zb;
  __syncthreads();
  int ra = 0, rb = 0;      // #surface < za ; #stratified <= zb
  for (int k = 0; k < nsurf; ++k) ra += (sb[k] < za) ? 1 : 0;
  for (int k = 0; k < ns; ++k) rb += (sa[k] <= zb) ? 1 : 0;
  if (lane < ns) sz[lane + ra] = za;
  if (lane < nsurf) sz[lane + rb] = zb;
  __syncthreads();
  for (int k = lane; k < total; k += 64) {
    const float z = sz[k];
    zo[k] = z;
    dd[k] = (k + 1 < total) ? sz[k + 1] - z : span / (float)ns;    // last: mean of (far-near)/N_samples (:149)
  }
}

// Piece k of a call that covers n rays in ray batches of `batch` rays, each cut into runs of `piece` rays (the last
// batch and the last piece of a batch ragged): rays [r0, r1).  Batches hold ceil(batch / piece) pieces each, in order.
__device__ __host__ __forceinline__ void gs_piece_range(int k, int n, int batch, int piece, int& r0, int& r1) {
  const int ppb = (batch + piece - 1) / piece;
  const int b = k / ppb, j = k - b * ppb;
  const int bend = b * batch + batch < n ? b * batch + batch : n;
  r0 = b * batch + j * piece;
  r1 = r0 + piece < bend ? r0 + piece : bend;
}
__device__ __host__ __forceinline__ int gs_piece_count(int n, int batch, int piece) {
  if (n <= 0) return 0;
  const int nb = (n + batch - 1) / batch, ppb = (batch + piece - 1) / piece;
  const int last = n - (nb - 1) * batch;
  return (nb - 1) * ppb + (last + piece - 1) / piece;
}

}  // namespace
