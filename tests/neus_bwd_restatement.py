"""fp64 restatement of the NeuS training backward's ray and point kernels (go_slam_amd/csrc/neus_bwd.hip), host only.

  ray_bwd     neus_ray_bwd_kernel (gs_neus_backward_rays): compositing backward -> d_alpha, d_rgb, d_grad
  point_bwd   neus_point_bwd_kernel<BINNED, AUX> (gs_neus_backward_points[_binned]): NeuS alpha chain, SDF linear layer,
              hash-grid value and second-order paths -> the per-point rows, the table gradient and d_inv_s

Every function evaluates the kernel's contract in float64 from the kernel's own fp32 / fp16 operands, following the
kernel's operation order, and carries a running error bound beside every value (class `E`): an operation that the kernel
does in fp32 adds u (|result| + bound) to the propagated bound of its operands, plus 2^-149 when the result may be
subnormal (u = 2^-24; fp16 roundings add u16 = 2^-11 relative and 2^-25 absolute).  So the bound of an output is the
first-order forward error of exactly the kernel's chain -- the suffix sums, the scans and the division by
(1 - a + 1e-7) included -- per element, never a norm.  Sums over lanes (scans, wave sums) are evaluated as the kernel's
trees; where the order is not fixed (atomics) a sum of m terms gets m u sum |terms|.

Stated bounds and exceptions:
  * expf is not correctly rounded (ocml): the sigmoids are bounded as 1 / (1 + e^-x) with 8 u relative on e^-x's
    evaluation plus the propagation of x's bound through the sigmoid (monotone: the larger side), plus 2^-126 absolute
    where e^-x may overflow fp32 (p then 0, the true p < 2^-127).
  * emb_cos (hardware v_cos_f32 after a Cody-Waite reduction, csrc/neus_common.h): 4e-6 absolute for |arg| < 1e3,
    plus the argument's own bound (|d cos| <= |d arg|).
  * The sample position, the bound normalisation (qn, the `inside` gate at qn = +-1, the clamp) and the cell coordinates
    (floor, fraction f) are not gradients: they are restated in fp32 operation by operation (the library is built with
    -ffp-contract=off; fmaf(scale, view, 0.5) is one rounding) and the test compares the pts rows bit for bit, so the
    gate at qn = +-1 and the cell at a cell face (f = 0) are decided exactly as the kernel decides them.
  * Gate decisions on computed values -- cosv < 0, the clip gate raw in [0, 1], |g| > 0 -- are taken from the fp64
    value; where the value lies within its own bound of the threshold the fp32 kernel may decide otherwise, so the point
    is a gate exception: every combination of its doubtful gates is evaluated, its rows may match any of them, and the
    table / d_inv_s bounds grow by the largest change of its records.  The number of exceptions per gate is reported.
  * Table gradient, per entry, from the records of pass 1 (one record per run of consecutive live lanes of a wave in
    the same cell: the run's fp32 pre-reduction, <= 6 doubling steps, adds 6 u sum |records|):
      fp32 atomics   sum of the k run records in any order: k u sum |run records| on top of the records' bounds;
      fp16 atomics   each run record x loss scale rounded to fp16 (u16 relative + 2^-25), then k fp16 read-modify-writes,
                     each rounding the running sum: k (u16 sum |records| + 2^-25) -- subnormals floored at 2^-25;
      binned         (hashed levels) each run record rounded once to fp16, summed exactly in 64-bit fixed point, the sum
                     rounded double -> float (u), added in fp32 to what the overflow atomics left (u) and rounded to fp16
                     (u16 + 2^-25).  Records of a (workgroup, level, bin) with more than ST_SLOTS = 48 records may go out
                     as fp16 atomics instead: those entries get the fp16-atomic term for them on top.
    Entries that no record touches are exactly 0.
  * d_inv_s: one wave tree (6), a 4-wave sum (2), one atomic per workgroup (any order): (8 + workgroups) u sum |terms|.
"""
import itertools
import math

import numpy as np

from oracle import neus_oracle as NO

U = 2.0 ** -24              # fp32 unit roundoff
U16 = 2.0 ** -11            # fp16 unit roundoff
ETA = 2.0 ** -149           # fp32: absolute rounding error below the normal range
ETA16 = 2.0 ** -25          # fp16: half the subnormal spacing
TINY = 2.0 ** -126          # smallest normal fp32
EXP_ULP = 8 * U             # expf (ocml) relative error allowance
COS_ABS = 4e-6              # emb_cos absolute error allowance
C7 = float(np.float32(1e-7))
C5 = float(np.float32(1e-5))
ST_SLOTS = 48
BIN_SHIFT = 13
LEVELS = NO.N_LEVELS


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def h16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


# ------------------------------------------------------------------------------------------ error-carrying numbers ----
class E:
    """value (float64, the exact result of the kernel's chain on its own operands) and bound on |fp32 result - value|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    def __getitem__(self, k):
        return E(self.v[k], self.e[k])


def _rnd(v, e):
    """one fp32 rounding of a result whose exact value is v and whose operands' error propagates to e"""
    m = np.abs(v) + e
    return e + U * m + np.where((m > 0) & (m < TINY), ETA, 0.0)


def _c(x):
    return x if isinstance(x, E) else E(x)


def add(a, b):
    a, b = _c(a), _c(b)
    v = a.v + b.v
    return E(v, _rnd(v, a.e + b.e))


def sub(a, b):
    a, b = _c(a), _c(b)
    v = a.v - b.v
    return E(v, _rnd(v, a.e + b.e))


def mul(a, b):
    a, b = _c(a), _c(b)
    v = a.v * b.v
    return E(v, _rnd(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e))


def fma(a, b, c):
    a, b, c = _c(a), _c(b), _c(c)
    v = a.v * b.v + c.v
    return E(v, _rnd(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + c.e))


def div(a, b):
    a, b = _c(a), _c(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = a.v / b.v
        den = np.abs(b.v) - b.e
        e = np.where(den > 0, (a.e + np.abs(v) * b.e) / np.where(den > 0, den, 1.0), np.inf)
    return E(v, _rnd(v, e))


def sqrt(a):
    v = np.sqrt(a.v)
    e = np.maximum(np.sqrt(a.v + a.e) - v, v - np.sqrt(np.maximum(a.v - a.e, 0.0)))
    return E(v, _rnd(v, e))


def sel(c, a, b):
    a, b = _c(a), _c(b)
    return E(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def live(a, on):
    """x * live with live exactly 0 or 1 (no rounding)"""
    return E(np.where(on, a.v, 0.0), np.where(on, a.e, 0.0))


def round16(a):
    """(_Float16) of an fp32 value: bound of |fp16(fp32 result) - value|"""
    m = np.abs(a.v) + a.e
    return E(a.v, a.e + U16 * m + np.where(m > 0, ETA16, 0.0))


def sigmoid(x):
    """1 / (1 + expf(-x)) in the kernel's three operations, bounded as a whole (see the module docstring)"""
    def s(t):
        with np.errstate(over="ignore"):
            return np.where(t >= 0, 1.0 / (1.0 + np.exp(-np.abs(t))), np.exp(-np.abs(t)) / (1.0 + np.exp(-np.abs(t))))
    v = s(x.v)
    prop = np.maximum(s(x.v + x.e) - v, v - s(x.v - x.e))
    e = prop + (EXP_ULP + 3 * U) * v + np.where(v < 2.0 ** -100, TINY, 0.0)
    return E(v, e)


# ------------------------------------------------------------------------------------------------- ray backward ----
def _wave_tree_sum(x):
    """gs_wave_sum over the last axis (64 lanes): a depth-6 pairwise tree"""
    while x.v.shape[-1] > 1:
        x = add(x[..., 0::2], x[..., 1::2])
    return x[..., 0]


def _shift(x, off, up, fill):
    """__shfl_up / __shfl_down by `off` over the last axis (lanes that would read outside keep `fill`)"""
    v = np.full_like(x.v, fill)
    e = np.zeros_like(x.e)
    if up:
        v[..., off:], e[..., off:] = x.v[..., :-off], x.e[..., :-off]
    else:
        v[..., :-off], e[..., :-off] = x.v[..., off:], x.e[..., off:]
    return E(v, e)


def _scan(x, op, up):
    """Hillis-Steele inclusive scan over 64 lanes (the kernel's wave_incl_prod / wave_incl_suffix_sum)"""
    lane = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        u = _shift(x, off, up, 0.0)
        take = (lane >= off) if up else (lane + off < 64)
        x = sel(take, op(x, u), x)
    return x


def ray_bwd(alpha, rgb, z_mid, grad, mask, d_color, d_depth, d_dvar, d_normal, d_wsum):
    """alpha f32 [n,s] (stored, masked), rgb f16 [n,s,3], z_mid f32 [n,s], grad f32 [n,s,3], mask bool [n,s]; upstream
    d_color [n,3], d_depth [n], d_dvar [n], d_normal [n,3], d_wsum [n].  Returns {name: E} for d_alpha [n,s],
    d_rgb [n,s,3], d_grad [n,s,3]."""
    n, s = alpha.shape
    assert 1 <= s <= 128
    pad = lambda x, fill=0.0: np.concatenate(
        [np.asarray(x, np.float64), np.full((n, 128 - s) + x.shape[2:], fill)], 1).reshape((n, 2, 64) + x.shape[2:])
    on = pad(np.ones((n, s)), 0.0) > 0
    a = E(pad(alpha))
    z = E(pad(z_mid))
    mk = pad(np.asarray(mask, np.float64))
    g = pad(grad)
    c = pad(np.asarray(rgb, np.float64))
    # transmittance: prefix product of t = 1 - a + 1e-7 per half, the second half times the first half's total
    t = sel(on, add(sub(1.0, a), C7), 1.0)
    T = [None, None]
    Trun = E(np.ones(n))
    for h in range(2):
        incl = _scan(t[:, h], mul, True)
        excl = _shift(incl, 1, True, 1.0)
        T[h] = mul(E(Trun.v[:, None], Trun.e[:, None]), excl)
        Trun = mul(Trun, incl[:, 63])
    T = E(np.stack([T[0].v, T[1].v], 1), np.stack([T[0].e, T[1].e], 1))
    w = mul(a, T)
    wsum = _wave_tree_sum(add(w[:, 0], w[:, 1]))
    dep = _wave_tree_sum(add(mul(z[:, 0], w[:, 0]), mul(z[:, 1], w[:, 1])))
    col = lambda x: np.asarray(x, np.float64).reshape(n)[:, None, None]
    dc = [col(np.asarray(d_color)[:, k]) for k in range(3)]
    dn = [col(np.asarray(d_normal)[:, k]) for k in range(3)]
    ddv, dws, dd = col(d_dvar), col(d_wsum), col(d_depth)
    ex = lambda x: E(x.v[:, None, None], x.e[:, None, None])
    dep3, wsum3 = ex(dep), ex(wsum)
    dd_tot = sub(dd, mul(mul(2.0, ddv), sub(dep3, mul(dep3, wsum3))))
    dz = sub(z, dep3)
    v = add(mul(dc[0], c[..., 0]), mul(dc[1], c[..., 1]))
    v = add(v, mul(dc[2], c[..., 2]))
    v = add(add(add(v, mul(dd_tot, z)), dws), mul(mul(ddv, dz), dz))
    nrm = add(add(mul(dn[0], g[..., 0]), mul(dn[1], g[..., 1])), mul(dn[2], g[..., 2]))
    v = add(v, mul(nrm, mk))
    dLdw = sel(on, v, 0.0)
    u = mul(dLdw, w)
    inc1 = _scan(u[:, 1], add, False)
    R1 = _shift(inc1, 1, False, 0.0)                        # the next lane's inclusive suffix sum
    R0 = add(_shift(_scan(u[:, 0], add, False), 1, False, 0.0), E(inc1.v[:, :1], inc1.e[:, :1]))
    R = E(np.stack([R0.v, R1.v], 1), np.stack([R0.e, R1.e], 1))
    da = sub(mul(dLdw, T), div(R, add(sub(1.0, a), C7)))
    flat = lambda x: E(x.v.reshape((n, 128) + x.v.shape[3:])[:, :s], x.e.reshape((n, 128) + x.v.shape[3:])[:, :s])
    d_alpha = flat(mul(da, mk))
    wm = [mul(mul(dc[k], w), mk) for k in range(3)]
    gm = [mul(mul(dn[k], w), mk) for k in range(3)]
    st = lambda xs: flat(E(np.stack([x.v for x in xs], -1), np.stack([x.e for x in xs], -1)))
    return {"d_alpha": d_alpha, "d_rgb": st(wm), "d_grad": st(gm)}


# ----------------------------------------------------------------------------------------------- point backward ----
def grid_corners(meta, l, gi):
    """csrc/grid_cell.h grid_corners: the 8 corner entries (within level l) of the cells gi uint32 [N,3] -> int64 [N,8]
    (uint32 arithmetic: dense base + strides, or the xor hash; then `% size`)"""
    M = 0xFFFFFFFF
    g = gi.astype(np.uint64)
    size = int(meta["size"][l])
    out = np.zeros((gi.shape[0], 8), np.uint64)
    for c in range(8):
        b = [(c >> d) & 1 for d in range(3)]
        x, y, zz = (g[:, 0] + b[0]) & M, (g[:, 1] + b[1]) & M, (g[:, 2] + b[2]) & M
        if int(meta["hashed"][l]):
            idx = (x ^ ((y * 2654435761) & M) ^ ((zz * 805459861) & M)) & M
        else:
            r = int(meta["resolution"][l])
            idx = (x + y * r + zz * ((r * r) & M)) & M
        out[:, c] = idx % size
    return out.astype(np.int64)


def positions(rays_o, rays_d, z_vals, dists, s, bound):
    """the fp32 front of the point kernel, op by op: pts [N,3], p_ (clamped qn) [N,3], inside [N,3], view [N,3]"""
    F = np.float32
    ray = np.arange(z_vals.size) // s
    zm = (z_vals.astype(F) + dists.astype(F) / F(2)).astype(F)
    pt = (rays_o.astype(F)[ray] + (rays_d.astype(F)[ray] * zm[:, None]).astype(F)).astype(F)
    b = np.asarray(bound, F).reshape(3, 2)
    span = (b[:, 1] - b[:, 0]).astype(F)
    qn = ((((pt - b[:, 0]).astype(F) / span).astype(F) * F(2)).astype(F) - F(1)).astype(F)
    inside = (qn >= -1) & (qn <= 1)
    qn = np.minimum(np.maximum(qn, F(-1)), F(1))
    view = (((qn + F(1)).astype(F)) / F(2)).astype(F)
    return pt, qn, inside, view, span


def cells(view, scale):
    """pos = fmaf(scale, view, 0.5) (one rounding), floor, fraction"""
    pos = (view.astype(np.float64) * np.float64(np.float32(scale)) + 0.5).astype(np.float32)
    fl = np.floor(pos)
    return fl.astype(np.int64).astype(np.uint32), (pos - fl).astype(np.float64)


def _chain(P, idx, dec, level_cb):
    """the per-point chain of neus_point_bwd_kernel for the points `idx` (int array) with gate decisions `dec` (dict of
    bool arrays over idx, or None: the fp64 decisions).  level_cb(l, gi, cidx, gacc) receives every level's records
    (gacc: E [n,8,2]).  Returns (rows dict of E, d_invs E [n], gates dict of (decision, doubtful))."""
    on = P["on"][idx]
    g = [E(P["grad"][idx, d]) for d in range(3)]
    dg_in = [P["d_grad"][idx, d] for d in range(3)]
    dirv = [P["dir"][idx, d] for d in range(3)]
    dist, sdf, inv_s = P["dists"][idx], P["sdf"][idx], P["inv_s"]
    dx = P["dx"][idx]                     # E [n,80]: dX as the kernel reads it (f16 * 1/scale: one rounding)
    dxh = lambda k: E(dx.v[:, 32 + k], dx.e[:, 32 + k])
    gates = {}
    d_sdf = live(E(P["d_sdf"][idx]), on)
    gn = sqrt(add(add(mul(g[0], g[0]), mul(g[1], g[1])), mul(g[2], g[2])))
    gates["gn"] = (gn.v > 0, (gn.v <= gn.e) & (gn.e > 0))
    d_gn = gates["gn"][0] if dec is None else dec["gn"]
    eik = div(mul(mul(P["gerr"][idx], 2.0), sub(gn, 1.0)), sel(d_gn, gn, 1.0))
    eik = sel(d_gn, eik, 0.0)
    dg = [live(add(add(dg_in[d], mul(eik, g[d])), dxh(1 + d)), on) for d in range(3)]
    da = live(E(P["d_alpha"][idx]), on)
    cosv = add(add(mul(dirv[0], g[0]), mul(dirv[1], g[1])), mul(dirv[2], g[2]))
    gates["cos"] = (cosv.v < 0, (np.abs(cosv.v) <= cosv.e) & (cosv.e > 0))
    d_cos = gates["cos"][0] if dec is None else dec["cos"]
    c = sel(d_cos, cosv, 0.0)
    half = div(mul(c, dist), 2.0)
    est_next, est_prev = add(sdf, half), sub(sdf, half)
    p = sigmoid(mul(est_prev, inv_s))
    q = sigmoid(mul(est_next, inv_s))
    pe = add(p, C5)
    raw = div(add(sub(p, q), C5), pe)
    amb = (np.abs(raw.v) <= raw.e) | (np.abs(raw.v - 1.0) <= raw.e)
    gates["raw"] = ((raw.v >= 0) & (raw.v <= 1), amb & (da.v != 0))
    d_raw = (gates["raw"][0] if dec is None else dec["raw"]) & (da.v != 0)
    dp = div(mul(da, q), mul(pe, pe))
    dq = div(E(-da.v, da.e), pe)
    dprev = mul(mul(dp, p), sub(1.0, p))
    dnext = mul(mul(dq, q), sub(1.0, q))
    d_invs = sel(d_raw, add(mul(dprev, est_prev), mul(dnext, est_next)), 0.0)
    d_sdf = sel(d_raw, add(d_sdf, mul(add(dprev, dnext), inv_s)), d_sdf)
    dcv = div(mul(mul(sub(dnext, dprev), inv_s), dist), 2.0)
    for d in range(3):
        dg[d] = sel(d_raw & d_cos, add(dg[d], mul(dcv, dirv[d])), dg[d])
    # bound normalisation (inside / clamp / view exact: fp32 restated)
    inside = P["inside"][idx]
    span = P["span"]
    dG = [div(mul(mul(dg[d], inside[:, d].astype(np.float64)), 2.0), float(span[d])) for d in range(3)]
    rs = P["row_scale"]
    n = len(idx)
    rows = {"d_out": [mul(d_sdf, rs)] + [mul(live(dxh(4 + o - 1), on), rs) for o in range(1, 32)],
            "lin_in": [live(E(P["qn"][idx, d]), on) for d in range(3)],
            "dw0": [mul(dG[d], rs) for d in range(3)]}
    dov = [d_sdf] + [live(dxh(4 + o - 1), on) for o in range(1, 32)]
    W = P["sdf_w"]
    meta = P["meta"]
    view = P["view"][idx]
    for l in range(LEVELS):
        scale = float(np.float32(meta["scale"][l]))
        gi, f = cells(view, scale)
        cidx = grid_corners(meta, l, gi) + int(meta["offset"][l])
        fr = [E(f[:, d]) for d in range(3)]
        om = [sub(1.0, fr[d]) for d in range(3)]
        wc = []
        for cc in range(8):
            w = E(np.ones(n))
            for d in range(3):
                w = mul(w, fr[d] if (cc >> d) & 1 else om[d])
            wc.append(w)
        if P["aux"] is not None:
            rec = P["aux"][l][idx]                                  # [n,8] f16 values
            e = [live(E(rec[:, 0]), on), live(E(rec[:, 1]), on)]
            dy = [[live(E(rec[:, 2 + gd]), on) for gd in range(3)], [live(E(rec[:, 5 + gd]), on) for gd in range(3)]]
        else:
            vals = P["grid16"].reshape(-1, 2)[cidx]                 # [n,8,2]
            e = [E(np.zeros(n)), E(np.zeros(n))]
            for cc in range(8):
                e = [fma(wc[cc], vals[:, cc, ft], e[ft]) for ft in range(2)]
            dy = [[None] * 3, [None] * 3]
        de = []
        for ft in range(2):
            acc = [E(np.zeros(n)), E(np.zeros(n))]
            for o in range(32):
                acc[o & 1] = fma(dov[o], float(W[o, 3 + 2 * l + ft]), acc[o & 1])
            de.append(add(acc[0], acc[1]))
        gw = [float(h16(W[0, 3 + 2 * l])), float(h16(W[0, 4 + 2 * l]))]
        gacc = [[mul(de[ft], wc[cc]) for ft in range(2)] for cc in range(8)]
        for gd in range(3):
            o0, o1 = (1 if gd == 0 else 0), (1 if gd == 2 else 2)
            a = [E(np.zeros(n)), E(np.zeros(n))]
            for k in range(4):
                w = mul(mul(scale, fr[o0] if k & 1 else om[o0]), fr[o1] if k & 2 else om[o1])
                cl = ((k & 1) << o0) | (((k >> 1) & 1) << o1)
                cr = cl | (1 << gd)
                if P["aux"] is None:
                    a = [fma(w, sub(vals[:, cr, ft], vals[:, cl, ft]), a[ft]) for ft in range(2)]
                for ft in range(2):
                    sv = mul(mul(mul(0.5, dG[gd]), gw[ft]), w)
                    gacc[cr][ft] = add(gacc[cr][ft], sv)
                    gacc[cl][ft] = sub(gacc[cl][ft], sv)
            if P["aux"] is None:
                dy[0][gd], dy[1][gd] = a
        for ft in range(2):
            rows["lin_in"].append(live(round16(e[ft]), on))
            t = add(add(mul(dG[0], dy[ft][0]), mul(dG[1], dy[ft][1])), mul(dG[2], dy[ft][2]))
            rows["dw0"].append(mul(mul(rs, 0.5), t))
        G = E(np.stack([np.stack([gacc[cc][ft].v for ft in range(2)], -1) for cc in range(8)], 1),
              np.stack([np.stack([gacc[cc][ft].e for ft in range(2)], -1) for cc in range(8)], 1))
        level_cb(l, gi, cidx, G)
    pts = P["pts"][idx]
    B = P["color_B"]
    dxe = lambda k: E(dx.v[:, k], dx.e[:, k])
    rows["d_arg"] = []
    for cc in range(33):
        arg = add(add(mul(pts[:, 0], float(B[0, cc])), mul(pts[:, 1], float(B[1, cc]))), mul(pts[:, 2], float(B[2, cc])))
        cs = E(np.cos(arg.v), arg.e + COS_ABS)
        rows["d_arg"].append(mul(live(mul(dxe(cc), cs), on), rs))
    out = {k: E(np.stack([x.v for x in xs], 1), np.stack([x.e for x in xs], 1)) for k, xs in rows.items()}
    return out, d_invs, gates


def prepare(rays_o, rays_d, z_vals, dists, s, grid16, sdf_w, color_B, inv_s, bound, sdf, grad, mask, d_alpha, d_sdf,
            d_grad, dX, dx_scale, d_gerr_ray, row_scale, enc_aux=None, meta=None):
    """the point kernel's inputs as numpy (dX: f32, or f16 holding dx_scale * gradient), flattened per point"""
    meta = meta or NO.grid_meta()
    npt = z_vals.size
    ray = np.arange(npt) // s
    pt, qn, inside, view, span = positions(rays_o, rays_d, z_vals.reshape(-1), dists.reshape(-1), s, bound)
    dX = np.asarray(dX)
    if dX.dtype == np.float16:
        inv = float(np.float32(1.0) / np.float32(dx_scale))
        xv = dX.astype(np.float64) * inv
        dx = E(xv, U * np.abs(xv) + np.where(xv != 0, ETA, 0.0))
    else:
        dx = E(dX.astype(np.float64))
    return dict(
        on=np.asarray(mask).reshape(-1) != 0, grad=np.asarray(grad, np.float64).reshape(-1, 3),
        d_grad=np.asarray(d_grad, np.float64).reshape(-1, 3), dir=np.asarray(rays_d, np.float64)[ray],
        dists=np.asarray(dists, np.float64).reshape(-1), sdf=np.asarray(sdf, np.float64).reshape(-1),
        inv_s=float(np.float32(inv_s)), dx=dx, d_sdf=np.asarray(d_sdf, np.float64).reshape(-1),
        d_alpha=np.asarray(d_alpha, np.float64).reshape(-1), gerr=np.asarray(d_gerr_ray, np.float64).reshape(-1)[ray],
        inside=inside, span=span.astype(np.float64), qn=qn.astype(np.float64), view=view, pts=pt.astype(np.float64),
        row_scale=float(np.float32(row_scale)), sdf_w=np.asarray(sdf_w, np.float32).astype(np.float64),
        color_B=np.asarray(color_B, np.float32).astype(np.float64), meta=meta,
        grid16=np.asarray(grid16, np.float16).astype(np.float64).reshape(-1),
        aux=None if enc_aux is None else np.asarray(enc_aux, np.float16).astype(np.float64), npt=npt)


class _Table:
    """per-entry exact sum and bound of the table gradient for one accumulation mode ("f32", "f16", "binned")"""

    def __init__(self, mode, meta, on, scale16):
        self.mode, self.meta, self.on = mode, meta, on
        self.sc = 1.0 if mode == "f32" else float(np.float32(scale16))
        tot = int(meta["total"]) * 2
        self.S = np.zeros(tot)           # exact sum (kernel units: x scale16 for fp16 modes)
        self.Eb = np.zeros(tot)          # sum of the records' own bounds (+ fp16 record rounding)
        self.A = np.zeros(tot)           # sum |record| (in the mode's units)
        self.K = np.zeros(tot)           # run records per entry (atomics, or maybe-atomics in binned mode)
        self.A_at = np.zeros(tot)        # binned: sum |record| of the maybe-atomic records
        self.hashed = np.zeros(tot, bool)
        self.touched = np.zeros(tot, bool)
        npt = on.size
        self.wave = np.arange(npt) // 64
        self.wg = np.arange(npt) // 256

    def runs(self, gi):
        on = self.on
        same = np.zeros(on.size, bool)
        same[1:] = on[1:] & on[:-1] & (self.wave[1:] == self.wave[:-1]) & (gi[1:] == gi[:-1]).all(1)
        return np.cumsum(~same) - 1

    def add_level(self, l, gi, cidx, G, extra=None):
        run = self.runs(gi)
        nr = run[-1] + 1 if run.size else 0
        sel_on = self.on
        # run sums of the live lanes (fp32 pre-reduction: <= 6 doubling steps)
        rv = np.zeros((nr, 8, 2))
        ra = np.zeros((nr, 8, 2))
        re = np.zeros((nr, 8, 2))
        np.add.at(rv, run[sel_on], G.v[sel_on])
        np.add.at(ra, run[sel_on], np.abs(G.v[sel_on]) + G.e[sel_on])
        np.add.at(re, run[sel_on], G.e[sel_on])
        re = re + 6 * U * ra * 1.0001
        first = np.zeros(nr, np.int64)
        first[run[::-1]] = np.arange(run.size)[::-1]
        live_run = sel_on[first]
        ent = cidx[first]                                    # [nr,8] entries of each run
        nz = ((np.abs(rv) + re) > 0).any(-1) & live_run[:, None]   # a record goes out (fp32 gacc != 0 may hold)
        hashed = bool(self.meta["hashed"][l])
        e2 = (ent[..., None] * 2 + np.arange(2)).reshape(nr, 16)
        nz2 = np.repeat(nz[..., None], 2, -1).reshape(nr, 16)
        val = (rv * self.sc).reshape(nr, 16)
        err = (re * self.sc).reshape(nr, 16)
        if self.mode != "f32":                               # each record rounded to fp16
            m = np.abs(val) + err
            err = err + U * m + U16 * (m + U * m) + np.where(m > 0, ETA16, 0.0)
        idx, val, err = e2[nz2], val[nz2], err[nz2]
        np.add.at(self.S, idx, val)
        np.add.at(self.Eb, idx, err)
        np.add.at(self.A, idx, np.abs(val) + err)
        self.touched[idx] = True
        if self.mode == "binned" and hashed:
            self.hashed[idx] = True
            # records per (workgroup, bin) beyond the staging slots may go out as fp16 atomics
            wg = self.wg[first]
            binr = (ent - int(self.meta["offset"][l])) >> BIN_SHIFT  # (bins are counted within the level)
            key = (wg[:, None] * 64 + binr)[nz]
            cnt = np.bincount(key, minlength=int(key.max()) + 1 if key.size else 1)
            over = np.zeros((nr, 8), bool)
            over[nz] = cnt[key] > ST_SLOTS
            o2 = np.repeat(over[..., None], 2, -1).reshape(nr, 16)[nz2]
            np.add.at(self.K, idx[o2], 1.0)
            np.add.at(self.A_at, idx[o2], np.abs(val[o2]) + err[o2])
        else:
            np.add.at(self.K, idx, 1.0)

    def widen(self, idx, d):
        np.add.at(self.Eb, idx, d)
        np.add.at(self.A, idx, d)

    def result(self):
        """(exact value, bound) per entry in the kernel's units"""
        S, A, K = self.S, self.A, self.K
        if self.mode == "f32":
            b = self.Eb + K * U * A * 1.0001
        else:
            b = self.Eb + K * (U16 * A * 1.0001 + ETA16)
            if self.mode == "binned":
                h = self.hashed
                m = np.abs(S) + self.Eb + self.K * (U16 * self.A_at * 1.0001 + ETA16)
                bh = (self.Eb + self.K * (U16 * self.A_at * 1.0001 + ETA16) + 2 * U * m
                      + U16 * (m + 2 * U * m) + ETA16)
                b = np.where(h, bh, b)
        return S, np.where(self.touched, b, 0.0)


def point_bwd(P, table_mode="f32", scale16=128.0):
    """the whole point backward for prepared inputs P (prepare()).  Returns a dict: rows {name: E [N, cols]} (f32
    layout: d_out 32, lin_in 35, dw0 35, d_arg 33), pts [N,3] (exact fp32), table (value, bound) per entry in the mode's
    units, touched bool, d_inv_s (value, bound), exceptions {gate: count}, alt [(point index, rows dict)] for
    gate-exception points (the rows of every other admissible combination of their gate decisions)."""
    npt = P["npt"]
    tab = _Table(table_mode, P["meta"], P["on"], scale16)
    allidx = np.arange(npt)
    rows, dinv, gates = _chain(P, allidx, None, tab.add_level)
    doubt = {k: gates[k][1] & P["on"] for k in gates}
    amb = np.zeros(npt, bool)
    for k in doubt:
        amb |= doubt[k]
    alt = []
    dinv_w = 0.0
    aidx = np.nonzero(amb)[0]
    if aidx.size:
        main = {}
        _, _, _ = _chain(P, aidx, {k: gates[k][0][aidx] for k in gates},
                         lambda l, gi, cidx, G: main.__setitem__(l, (cidx, G)))
        keys = [k for k in ("gn", "cos", "raw")]
        dmax = {}
        for combo in itertools.product((False, True), repeat=3):
            if not any(combo):
                continue
            flip = dict(zip(keys, combo))
            okp = np.ones(aidx.size, bool)
            for k in keys:
                if flip[k]:
                    okp &= doubt[k][aidx]
            if not okp.any():
                continue
            sub_idx = aidx[okp]
            dec = {k: (gates[k][0][sub_idx] ^ flip[k]) for k in keys}
            recs = {}
            r2, d2, _ = _chain(P, sub_idx, dec, lambda l, gi, cidx, G: recs.__setitem__(l, (cidx, G)))
            for j, p in enumerate(sub_idx):
                alt.append((int(p), {k: v[j] for k, v in r2.items()}))
            pos = np.nonzero(okp)[0]
            for l in range(LEVELS):
                cidx, G = recs[l]
                cm, Gm = main[l][0][pos], main[l][1][pos]
                d = np.abs(G.v - Gm.v) + G.e + Gm.e
                key = (l, tuple(sub_idx))
                dmax[key] = (cidx, d)
            dinv_w += float(np.sum(np.abs(d2.v - dinv.v[sub_idx]) + d2.e))
        sc = tab.sc
        for (l, _), (cidx, d) in dmax.items():
            e2 = (cidx[..., None] * 2 + np.arange(2)).reshape(-1)
            tab.widen(e2, (d * sc * (1 + U16 * 4)).reshape(-1) + np.where(d.reshape(-1) > 0, ETA16, 0.0))
            tab.touched[e2[(d.reshape(-1) > 0)]] = True
    S, Bt = tab.result()
    nblk = -(-npt // 256)
    on = P["on"]
    dv = float(np.sum(dinv.v[on]))
    db = float(np.sum(dinv.e[on]) + (8 + nblk) * U * np.sum(np.abs(dinv.v[on]) + dinv.e[on]) * 1.0001) + dinv_w
    return dict(rows=rows, pts=P["pts"], table=(S, Bt), touched=tab.touched, table_k=tab.K, d_inv_s=(dv, db + (ETA if db > 0 else 0)),
                exceptions={k: int(doubt[k].sum()) for k in doubt}, alt=alt)


# ------------------------------------------------------------------------------------------------------ scenes ----
BOUND = np.array([-2.5, 2.5, -2.5, 2.5, -2.5, 2.5], np.float32)


def params(seed=0, meta=None):
    """trained-like parameters (oracle make_params' shapes and scales, grid_init 0.3): sdf_w f32 [32,35], color_B f32
    [3,33], grid f16 [total*2]"""
    meta = meta or NO.grid_meta()
    rng = np.random.default_rng(seed)
    sdf_w = np.zeros((32, 35), np.float32)
    sdf_w[:, :3] = rng.standard_normal((32, 3)) * 0.25
    sdf_w[:, 3:] = rng.standard_normal((32, 32)) * 0.1
    color_B = (rng.standard_normal((3, 33)) * 25.0).astype(np.float32)
    grid = np.empty(int(meta["total"]) * 2, np.float16)
    for l in range(LEVELS):
        a, b = 2 * int(meta["offset"][l]), 2 * (int(meta["offset"][l]) + int(meta["size"][l]))
        grid[a:b] = (rng.random(b - a, np.float32) * 2 - 1) * (0.3 * 15.0 / float(meta["scale"][l]))
    return dict(sdf_w=sdf_w, color_B=color_B, grid=grid)


def _face_value(l, meta, target):
    """a world x near `target` whose fp32 normalisation puts it exactly on a cell face of level l (f == 0)"""
    sc = float(np.float32(meta["scale"][l]))
    k0 = math.floor((float(target) + 2.5) / 5.0 * sc + 0.5)
    for k in sorted(range(max(1, k0 - 40), k0 + 40), key=lambda k: abs(k - k0)):
        x0 = np.float32(-2.5 + (k - 0.5) / sc * 5.0)
        cand = [x0]
        lo = hi = x0
        for _ in range(64):
            lo, hi = np.nextafter(lo, np.float32(-9)), np.nextafter(hi, np.float32(9))
            cand += [lo, hi]
        xs = np.array(cand, np.float32)
        z = np.zeros(len(xs), np.float32)
        _, _, _, view, _ = positions(np.stack([xs, z, z], 1), np.zeros((len(xs), 3), np.float32), z, z, 1, BOUND)
        _, f = cells(view, sc)
        hit = np.nonzero(f[:, 0] == 0.0)[0]
        if hit.size and abs(xs[hit[0]]) < 2.5:
            return xs[hit[0]]
    raise AssertionError("no face point found")


def scene(name, seed=1, meta=None):
    """inputs of the point backward (numpy): rays_o/rays_d f32 [n,3], z_vals/dists f32 [n,s], sdf, grad, mask, d_alpha,
    d_sdf, d_grad, dX f32 [n*s,80], d_gerr_ray [n], inv_s, enc_aux f16 [16,n*s,8].

      soft     257 points, rays of 1 sample, inv_s ~ 7.4 (variance 0.2), random everything
      big      4099 rays x 72 samples along sorted depths (production-sized, ragged: runs of equal cells)
      hard3    inv_s = 1e3 / hard5: inv_s = 1e5 -- saturating sdf values, cos > 0 / < 0 / == 0 exactly, |g| = 0,
               masked points, points on and just outside the bound faces, points on cell faces and the far corner
      lanes    scatter layouts: one cell for a whole wave, two alternating cells, random run lengths, masked lanes in
               runs, odd/even neighbours in and out of a cell; plus a ragged tail
      line     a workgroup of points one finest cell apart along x: > 48 records of one (level, bin) -> overflow atomics
      one      a single point"""
    meta = meta or NO.grid_meta()
    rng = np.random.default_rng(seed)
    F = np.float32
    inv_s = float(np.exp(np.float64(0.2) * 10.0))
    s = 1
    if name == "big":
        n, s = 4099, 72
        o = rng.uniform(-1.5, 1.5, (n, 3))
        d = rng.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        z = np.sort(rng.uniform(0.05, 2.5, (n, s)), 1)
        dist = np.concatenate([np.diff(z, axis=1), np.full((n, 1), 0.02)], 1)
        pos = None
    else:
        if name == "soft":
            pos = rng.uniform(-2.4, 2.4, (257, 3))
        elif name == "one":
            pos = rng.uniform(-2.4, 2.4, (1, 3))
        elif name in ("hard3", "hard5"):
            npt = 63 if name == "hard5" else 65
            pos = rng.uniform(-2.4, 2.4, (npt, 3))
            pos[0, 0], pos[1, 1], pos[2, 2] = -2.5, 2.5, 2.5                   # on bound faces
            pos[3, 0] = np.nextafter(F(2.5), F(9))                              # just outside
            pos[4, 1] = np.nextafter(F(-2.5), F(-9))
            pos[5] = (2.5, 2.5, 2.5)                                            # far corner of every level
            for k, l in enumerate((0, 1, 4, 7, 15)):                            # on a cell face of level l (f = 0)
                pos[6 + k, 0] = _face_value(l, meta, pos[6 + k, 0])
            inv_s = 1e3 if name == "hard3" else 1e5
        elif name == "lanes":
            base = rng.uniform(-2.0, 2.0, (6, 3))
            pts = [np.repeat(base[:1], 64, 0)]                                  # wave 0: one cell
            pts.append(np.where((np.arange(64) % 2)[:, None] == 0, base[1], base[2]))        # wave 1: alternating
            runs = np.repeat(np.arange(64), rng.integers(1, 9, 64))[:64]
            pts.append(base[3] + runs[:, None] * 0.01)                          # wave 2: random run lengths
            pts.append(base[4] + runs[::-1, None] * 0.013)                      # wave 3: same, masked lanes inside
            pair = (np.arange(64) // 2) * 0.011 + np.where(np.arange(64) % 4 == 3, 0.0031, 0.0)
            pts.append(base[5] + pair[:, None])                                 # wave 4: pairs in / out of one cell
            pts.append(rng.uniform(-2.0, 2.0, (5, 3)))                          # ragged tail
            pos = np.concatenate(pts, 0)
        elif name == "line":
            cell = 5.0 / float(meta["scale"][LEVELS - 1])
            pos = np.zeros((259, 3))
            pos[:, 0] = -2.4 + (np.arange(259) + 0.5) * cell
            pos[:, 1], pos[:, 2] = 0.3, -0.7
        else:
            raise KeyError(name)
        n = pos.shape[0]
        o = pos
        d = rng.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        z = np.zeros((n, 1))
        dist = np.zeros((n, 1))
        if name in ("soft", "one", "hard3", "hard5"):     # (dists > 0: the cos term of the alpha reaches d grad)
            dist[:, 0] = rng.uniform(0.005, 0.05, n)
            dist[:11] = 0.0                               # (bound / face / corner points sit exactly at their origin)
    npt = n * s
    sdf = rng.standard_normal(npt) * 0.3
    grad = rng.standard_normal((npt, 3))
    mask = rng.random(npt) < 0.9
    if name in ("hard3", "hard5"):
        m = npt
        sdf[:m // 3] = rng.choice([-1.0, 1.0, -0.05, 0.05, -1e-3, 1e-3, 0.0], m // 3)
        # cos == 0 exactly: axis-aligned direction, gradient perpendicular to it
        d[20:24] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]]
        grad[20:24] = [[0, 0.7, -0.3], [1.1, 0, 0.2], [0.3, -0.9, 0], [0, 0, 0]]       # (the last: |g| = 0)
        grad[24] = 0.0
        grad[25:35] = d[25:35] * rng.choice([-1.0, 1.0], (10, 1)) * 0.9                  # cos of either sign, saturating
        sdf[25:35] = rng.choice([-2.0, 2.0, 0.5, -0.5], 10)
        mask[:] = True
        mask[36:40] = False
        mask[0] = True
    if name == "lanes":
        mask[:] = True
        mask[192 + np.array([3, 4, 10, 11, 12, 30, 31])] = False
    if name == "line":
        mask[:] = True
    d_alpha = rng.standard_normal(npt) * 0.1
    d_alpha[rng.random(npt) < 0.05] = 0.0
    d_sdf = rng.standard_normal(npt) * 0.1 * (rng.random(npt) < 0.3)
    d_grad = rng.standard_normal((npt, 3)) * 0.01
    dX = rng.standard_normal((npt, 80)) * 0.01
    dX[:, 67:] = 0.0
    d_gerr = rng.standard_normal(n) * 0.01
    aux = np.empty((LEVELS, npt, 8), np.float16)
    aux[..., :2] = rng.standard_normal((LEVELS, npt, 2)) * 0.1
    aux[..., 2:] = rng.standard_normal((LEVELS, npt, 6)) * 5.0
    return dict(rays_o=o.astype(F), rays_d=d.astype(F), z_vals=z.astype(F), dists=dist.astype(F), s=s,
                sdf=sdf.astype(F), grad=grad.astype(F), mask=mask.astype(np.uint8), d_alpha=d_alpha.astype(F),
                d_sdf=d_sdf.astype(F), d_grad=d_grad.astype(F), dX=dX.astype(F), d_gerr_ray=d_gerr.astype(F),
                inv_s=F(inv_s), enc_aux=aux)


def prepare_scene(sc, prm, dx16=False, dx_scale=128.0, aux=False, row_scale=1.0, meta=None):
    """prepare() for scene() / params() dictionaries; dx16: dX as f16 holding dx_scale * gradient"""
    dX = (sc["dX"] * np.float32(dx_scale)).astype(np.float16) if dx16 else sc["dX"]
    return prepare(sc["rays_o"], sc["rays_d"], sc["z_vals"], sc["dists"], sc["s"], prm["grid"], prm["sdf_w"],
                   prm["color_B"], sc["inv_s"], BOUND, sc["sdf"], sc["grad"], sc["mask"], sc["d_alpha"], sc["d_sdf"],
                   sc["d_grad"], dX, dx_scale if dx16 else 1.0, sc["d_gerr_ray"], row_scale,
                   sc["enc_aux"] if aux else None, meta)


def ray_scene(n, s, regime, seed=0):
    """inputs of the ray backward: alpha (stored = alpha * mask), rgb f16, z_mid, grad, mask and the five upstream
    gradients for a regime: soft | one_opaque | opaque_several | near_one | opaque_run | zero | mixed_mask | far_z"""
    rng = np.random.default_rng(seed)
    F = np.float32
    a = rng.uniform(0.0, 0.3, (n, s))
    mask = np.ones((n, s), bool)
    z = np.sort(rng.uniform(0.1, 4.0, (n, s)), 1)
    if regime == "one_opaque":
        a[:, s // 2] = 1.0
    elif regime == "opaque_several":
        a[:, rng.integers(0, s, 3)] = 1.0
    elif regime == "near_one":
        a[:, ::3] = 1.0 - 2.0 ** -24
    elif regime == "opaque_run":
        a = rng.uniform(0.9, 1.0, (n, s))
        a[:, s // 3: s // 3 + 9] = 1.0                     # runs of >= 7 opaque samples: T through subnormals to 0
    elif regime == "zero":
        a[:] = 0.0
    elif regime == "mixed_mask":
        mask = rng.random((n, s)) < 0.6
    elif regime == "far_z":
        z = 1e3 + np.sort(rng.uniform(0.0, 2.0, (n, s)), 1)
        a = rng.uniform(0.2, 0.9, (n, s))
    a = (a.astype(F) * mask).astype(F)
    rgb = rng.uniform(0, 1, (n, s, 3)).astype(np.float16) * mask[..., None]
    grad = rng.standard_normal((n, s, 3)).astype(F)
    up = dict(d_color=rng.standard_normal((n, 3)), d_depth=rng.standard_normal(n), d_dvar=rng.standard_normal(n),
              d_normal=rng.standard_normal((n, 3)), d_wsum=rng.standard_normal(n))
    return dict(alpha=a, rgb=rgb.astype(np.float16), z_mid=z.astype(F), grad=grad, mask=mask,
                **{k: v.astype(F) for k, v in up.items()})


UPSTREAM = ("d_color", "d_depth", "d_dvar", "d_normal", "d_wsum")


def only(sc, which):
    """the scene with every upstream term but `which` zeroed (which = 'all': unchanged)"""
    out = dict(sc)
    if which != "all":
        for k in UPSTREAM:
            if k != which:
                out[k] = np.zeros_like(sc[k])
    return out
