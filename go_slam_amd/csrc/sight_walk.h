// The supercover walk between two cells of a lattice and the length of a leg, shared by every kernel of sight.hip: the
// contract is include/goslam_hip.h (gs_segment_* / gs_path_*), tests/sight_restatement.py restates it serially.
// Integer only; the cell under the walk is carried as its linear index, so a visitor is one load.
#pragma once

namespace {

// Visits the linear index of every cell of the supercover of a and b, a first; `visit` returns false to stop the walk,
// which then returns false.  Both ends must lie inside the lattice [*, n1, n2] (the caller's one bounds check: every
// visited cell lies in the box the ends span).  Registers only: no arrays, every axis written out.
template <class Visit>
__device__ __forceinline__ bool sight_walk(int a0, int a1, int a2, int b0, int b1, int b2, int n1, int n2,
                                           Visit&& visit) {
  const int d0 = b0 - a0, d1 = b1 - a1, d2 = b2 - a2;
  const int w0 = d0 < 0 ? -d0 : d0, w1 = d1 < 0 ? -d1 : d1, w2 = d2 < 0 ? -d2 : d2;
  // one step along an axis as a step of the linear index
  const int s0 = d0 > 0 ? n1 * n2 : (d0 < 0 ? -(n1 * n2) : 0);
  const int s1 = d1 > 0 ? n2 : (d1 < 0 ? -n2 : 0);
  const int s2 = d2 > 0 ? 1 : (d2 < 0 ? -1 : 0);
  int at = (a0 * n1 + a1) * n2 + a2;
  if (!visit(at)) return false;
  int k0 = 0, k1 = 0, k2 = 0;
  for (int step = w0 + w1 + w2; step > 0 && (k0 < w0 || k1 < w1 || k2 < w2); --step) {
    // axis k crosses at c_k / (2 v_k); a finished axis never does: 1 / 0
    const int c0 = k0 < w0 ? 2 * k0 + 1 : 1, v0 = k0 < w0 ? w0 : 0;
    const int c1 = k1 < w1 ? 2 * k1 + 1 : 1, v1 = k1 < w1 ? w1 : 0;
    const int c2 = k2 < w2 ? 2 * k2 + 1 : 1, v2 = k2 < w2 ? w2 : 0;
    const int p01 = c0 * v1, p10 = c1 * v0, p02 = c0 * v2, p20 = c2 * v0, p12 = c1 * v2, p21 = c2 * v1;
    // t_a <= t_b  <=>  c_a v_b <= c_b v_a; at least one axis is unfinished, and a finished one loses against it
    const bool in0 = p01 <= p10 && p02 <= p20;
    const bool in1 = p10 <= p01 && p12 <= p21;
    const bool in2 = p20 <= p02 && p21 <= p12;
    const int o0 = in0 ? s0 : 0, o1 = in1 ? s1 : 0, o2 = in2 ? s2 : 0;
    const int ties = (int)in0 + (int)in1 + (int)in2;
    if (ties > 1) {                                         // through an edge or a corner: the whole box around it
      if (in0 && !visit(at + o0)) return false;
      if (in1 && !visit(at + o1)) return false;
      if (in2 && !visit(at + o2)) return false;
      if (ties == 3) {
        if (!visit(at + o0 + o1)) return false;
        if (!visit(at + o0 + o2)) return false;
        if (!visit(at + o1 + o2)) return false;
      }
    }
    at += o0 + o1 + o2;
    if (!visit(at)) return false;
    k0 += (int)in0;
    k1 += (int)in1;
    k2 += (int)in2;
  }
  return true;
}

// floor(sqrt(1000000 * |d|^2)), a leg's length in milli-voxels: an fp64 sqrt (correctly rounded, so at most one off the
// floor) and the integer correction.  Unsigned 64-bit throughout: no component is trusted to be a lattice difference.
__host__ __device__ __forceinline__ int sight_leg_length(int d0, int d1, int d2) {
  const unsigned long long e0 = (unsigned long long)(d0 < 0 ? -(long long)d0 : (long long)d0);
  const unsigned long long e1 = (unsigned long long)(d1 < 0 ? -(long long)d1 : (long long)d1);
  const unsigned long long e2 = (unsigned long long)(d2 < 0 ? -(long long)d2 : (long long)d2);
  if (e0 > 1023ull || e1 > 1023ull || e2 > 1023ull) return 0x7fffffff;      // no leg of a lattice
  const unsigned long long s = 1000000ull * (e0 * e0 + e1 * e1 + e2 * e2);
  unsigned long long r = (unsigned long long)sqrt((double)s);
  if (r * r > s) --r;
  else if ((r + 1) * (r + 1) <= s) ++r;
  return (int)r;
}

}  // namespace
