"""fp64 restatement of the NeuS forward (go_slam_amd/csrc/neus.hip) and of the colour MLP's forward and backward
(neus.hip wave_mlp64 / neus_mlp_kernel / mlp_pad_kernel, neus_mlp_bwd.hip), host only.

  point_fwd   neus_encode_levels_kernel + neus_point_kernel (both gather orders, main and force pass): z_mid, mask, the
              hash-grid levels, the SDF layer, d sdf / d x, the NeuS alpha, the 80-column colour-MLP input row, enc_aux
  mlp_fwd     H1 = fp16(relu(W1 X)), H2 = fp16(relu(W2 H1)), out = fp16(W3 H2), rgb = fp16(sigmoid(out))
  mlp_bwd     gs_mlp_backward's contract (include/goslam_neus.h): dpre, dH2, dH1, dX and the three weight gradients
  ray_fwd     neus_ray_kernel: the transmittance scan, colour, depth, depth variance, normal, weight sum, eikonal term
  piece_sum   neus_piece_sum_kernel

The conventions are those of tests/neus_bwd_restatement.py, whose value class `E` and operations this module imports: a
value is the exact float64 result of the kernel's chain on the kernel's own fp32 / fp16 operands, in the kernel's
operation order, and its bound is the first-order forward error of that chain -- every fp32 operation adds
u (|result| + bound) (u = 2^-24) plus 2^-149 where the result may be subnormal, every fp16 rounding u16 = 2^-11
relative plus 2^-25 absolute.  Wave sums are the kernel's depth-6 trees, scans its Hillis-Steele steps.

Stated bounds and exceptions:
  * MFMA (v_mfma_f32_32x32x16_f16, chained over K): an output is an fp32 sum of K exact fp16 x fp16 products in an
    order the hardware does not document, bounded by K u sum |terms| (+ K 2^-149) on top of the propagated bounds of
    its operands.  Weight gradients (gs_mlp_backward's `partial`): one accumulator chain per wave over its blocks (2 NSUB
    MFMAs per block), the four waves' chains added in pairs, 16 products per MFMA: m = 2 NSUB blocks_per_wave + 18
    roundings, m u sum |terms| per entry; the host's fp64 sum of the partial rows is exact to 2^-50 relative.
  * fp16 subnormal MFMA operands are NOT flushed on gfx950 (measured: tests/test_neus_fwd_numerics_gpu.py
    ::test_mfma_keeps_fp16_subnormal_operands -- an fp16 subnormal input, hidden activation and weight each reach the
    output exactly), so the bounds above need no flush term.
  * expf (ocml) in the sigmoids: neus_bwd_restatement.sigmoid (8 u relative, 2^-126 absolute where expf may overflow).
  * emb_sin (Cody-Waite reduction + v_sin_f32): 4e-6 absolute for |arg| < 1e3 plus the argument's bound.
  * The sample position, the realtime-bound mask (strict inequalities), qn, `inside`, view and the cell coordinates are
    restated in fp32 operation by operation (neus_bwd_restatement.positions / cells; the library is built with
    -ffp-contract=off) and compared bit for bit.
  * Gates decided on computed values: the cos gate (iter_cos = min(cos, 0)), the alpha clip to [0, 1] and the ReLUs of
    the forward are 1-Lipschitz functions of their argument, so the argument's bound carries through whatever the fp32
    kernel decides; points within their bound of a threshold are only counted (`gates`).  The backward's [H > 0] mask
    is not continuous: where the kernel's fp16 H may be 0 or not (the fp32 pre-activation within its bound of 2^-25, the
    point below which fp16 rounds to 0) the entry is a gate exception -- its dH entry's bound grows by |dH|, i.e. dX may
    match either decision, and the dW entries it feeds grow through the same propagation.  Counted per GEMM.
  * The two gather orders of neus_point_kernel do the same operations in the same order (the level-major record holds
    fmaf(g1, dv1, g0 * dv0) of one level, added to the running sum exactly as the point-major loop adds it), so this one
    restatement serves both and the kernel's per-point outputs must agree bit for bit.
"""
import numpy as np

import neus_bwd_restatement as R
from neus_bwd_restatement import (E, U, ETA, C7, C5, COS_ABS, LEVELS, add, sub, mul, fma, div, sqrt, live, round16,
                                  sigmoid, _wave_tree_sum, _scan, _shift, positions, cells, grid_corners)

SUB16 = 2.0 ** -24           # smallest fp16 subnormal


def _relu(x):
    return E(np.maximum(x.v, 0.0), x.e)


def _stack(xs, axis=-1):
    return E(np.stack([x.v for x in xs], axis), np.stack([x.e for x in xs], axis))


def mfma(W, X, K=None):
    """Y = X W^T on the matrix cores: W exact fp16 values [m, k] (float64), X E [n, k] (fp16 operands).  fp32 sums of K
    exact products in any order."""
    W = np.asarray(W, np.float64)
    K = W.shape[1] if K is None else K
    aw = np.abs(W)
    v = X.v @ W.T
    a = np.abs(X.v) @ aw.T
    prop = X.e @ aw.T
    m = a + prop
    return E(v, prop + K * U * m + 2.0 ** -50 * a + np.where(m > 0, K * ETA, 0.0))


def _outer_sum(a, b, m):
    """sum over points (axis 0) of a[:, i] b[:, j] in fp32 accumulator chains of m roundings: E [i, j]"""
    v = a.v.T @ b.v
    A = np.abs(a.v).T @ np.abs(b.v)
    prop = np.abs(a.v).T @ b.e + a.e.T @ np.abs(b.v) + a.e.T @ b.e
    mm = A + prop
    return E(v, prop + m * U * mm + a.v.shape[0] * 2.0 ** -52 * A + np.where(mm > 0, m * ETA, 0.0))


def split_mlp(W):
    W = np.asarray(W, np.float16).astype(np.float64).reshape(-1)
    return W[:5120].reshape(64, 80), W[5120:9216].reshape(64, 64), W[9216:].reshape(16, 64)


def pad_rows(x, n_in):
    """mlp_pad_kernel: [n, n_in] fp16 rows -> [n, 80], the missing columns exactly 1"""
    x = np.asarray(x, np.float16).astype(np.float64).reshape(-1, n_in)
    return np.concatenate([x, np.ones((x.shape[0], 80 - n_in))], 1)


def mlp_fwd(X, W, n_out=3, _wrong=None):
    """X fp16 values [n, 80] (already padded), W the tcnn parameter vector [10240] fp16.  Returns dict of E: h1, h2
    (fp16, post-ReLU), out [n, n_out] (fp16 network output), rgb (fp16 sigmoid of the fp16 output).
    _wrong (tests only): 'swap_w2_k' -- W2's K fragments 1 and 2 exchanged."""
    W1, W2, W3 = split_mlp(W)
    if _wrong == "swap_w2_k":
        W2 = W2[:, np.r_[0:16, 32:48, 16:32, 48:64]]
    x = E(np.asarray(X, np.float64))
    h1 = round16(_relu(mfma(W1, x)))
    h2 = round16(_relu(mfma(W2, h1)))
    out = round16(mfma(W3[:n_out], h2))
    rgb = round16(sigmoid(out))
    return {"h1": h1, "h2": h2, "out": out, "rgb": rgb}


def _gate(dpre, pre):
    """dH = fp16(dpre) * [H > 0], H = fp16(relu(pre)) the kernel's fp16 activation: H > 0 iff the fp32 pre-activation
    exceeds 2^-25 (half the smallest fp16 subnormal rounds to 0).  (E, number of gate exceptions)"""
    d = round16(dpre)
    on = pre.v - pre.e > SUB16 / 2
    off = pre.v + pre.e <= SUB16 / 2
    doubt = ~on & ~off
    keep = on | (doubt & (pre.v > SUB16 / 2))
    v = np.where(keep, d.v, 0.0)
    e = np.where(keep & ~doubt, d.e, 0.0) + np.where(doubt, d.e + np.abs(d.v), 0.0)
    return E(v, e), int(doubt.sum())


def mlp_bwd_chain(n):
    """roundings on a weight-gradient accumulator chain of gs_mlp_backward for n points (neus_mlp_bwd.hip's grid)"""
    nsub = 2 if n >= 2 * 64 * 1024 else 1
    nblk = -(-n // (32 * nsub))
    grid = -(-nblk // 4) if nblk < 1024 else 256
    return 2 * nsub * -(-nblk // (4 * grid)) + 18


def mlp_bwd(X, W, d_rgb, rgb, ls, _wrong=None):
    """gs_mlp_backward for X fp16 [n, 80], W [10240] fp16, d_rgb f32 [n, 3], rgb fp16 [n, 3] or None, loss scale ls.
    Returns dict of E in the kernel's (loss-scaled) units: dX [n, 80], dW1 [64, 80], dW2 [64, 64], dW3 [16, 64];
    gates {'h2': count, 'h1': count}.  _wrong (tests only): 'mask_ge' -- [H >= 0] instead of [H > 0]."""
    W1, W2, W3 = split_mlp(W)
    x = E(np.asarray(X, np.float64))
    n = x.v.shape[0]
    p1 = mfma(W1, x)
    h1 = round16(_relu(p1))
    p2 = mfma(W2, h1)
    h2 = round16(_relu(p2))
    dr = E(np.asarray(d_rgb, np.float32).astype(np.float64))
    if rgb is not None:
        y = np.asarray(rgb, np.float16).astype(np.float64)
        dr = mul(dr, mul(y, 1.0 - y))                     # (1 - y is exact in fp32 for an fp16 y in [0, 1])
    dpre = round16(mul(dr, float(np.float32(ls))))
    gates = {}
    if _wrong == "mask_ge":
        gate = lambda d, pre: (round16(d), 0)
    else:
        gate = _gate
    dh2, gates["h2"] = gate(mfma(W3[:3].T, dpre, 16), p2)
    dh1, gates["h1"] = gate(mfma(W2.T, dh2), p1)
    dx = round16(mfma(W1.T, dh1))
    m = mlp_bwd_chain(n)
    dw3 = _outer_sum(dpre, h2, m)
    dw3 = E(np.concatenate([dw3.v, np.zeros((13, 64))]), np.concatenate([dw3.e, np.zeros((13, 64))]))
    return {"dX": dx, "dW1": _outer_sum(dh1, x, m), "dW2": _outer_sum(dh2, h1, m), "dW3": dw3, "gates": gates}


# ---------------------------------------------------------------------------------------------------- ray stage ----
def ray_fwd(alpha, rgb, z_mid, grad, mask, gerr_scale, _wrong=None):
    """neus_ray_kernel from the point kernel's own outputs: alpha f32 [n, s] (as stored), rgb f16 [n, s, 3], z_mid f32
    [n, s], grad f32 [n, s, 3], mask [n, s]; gerr_scale f32 scalar or per ray [n].  Returns dict of E: color [n, 3],
    depth, depth_var, weight_sum, grad_err [n], normal [n, 3].
    _wrong (tests only): 'no_c7' (t = 1 - a), 'excl_shift' (the exclusive product one lane late), 'var_depth' (the
    variance about depth / weight_sum)."""
    alpha = np.asarray(alpha, np.float32)
    n, s = alpha.shape
    nc = -(-s // 64)
    S = nc * 64
    pad = lambda x: np.concatenate([np.asarray(x, np.float64), np.zeros((n, S - s) + np.shape(x)[2:])], 1).reshape(
        (n, nc, 64) + np.shape(x)[2:])
    on = pad(np.ones((n, s))) > 0
    a = E(pad(alpha))
    z = E(pad(z_mid))
    mk = pad(np.asarray(mask, np.float64)) != 0
    g = [E(pad(np.asarray(grad, np.float32)[..., d])) for d in range(3)]
    c = [E(pad(np.asarray(rgb, np.float16)[..., d].astype(np.float64))) for d in range(3)]
    t = R.sel(on, sub(sub(1.0, a), 0.0) if _wrong == "no_c7" else add(sub(1.0, a), C7), 1.0)
    ws = []
    Trun = E(np.ones(n))
    for k in range(nc):
        incl = _scan(t[:, k], mul, True)
        excl = _shift(incl, 2 if _wrong == "excl_shift" else 1, True, 1.0)
        ws.append(mul(a[:, k], mul(E(Trun.v[:, None], Trun.e[:, None]), excl)))
        Trun = mul(Trun, incl[:, 63])
    w = _stack(ws, 1)
    zero = E(np.zeros((n, 64)))
    acc = {"wsum": zero, "dep": zero, "ge": zero}
    for d in range(3):
        acc[f"col{d}"] = zero
        acc[f"nrm{d}"] = zero
    nr = sub(sqrt(add(add(mul(g[0], g[0]), mul(g[1], g[1])), mul(g[2], g[2]))), 1.0)
    for k in range(nc):
        o = on[:, k]
        wk = w[:, k]
        step = lambda name, x: acc.__setitem__(name, R.sel(o, add(acc[name], x), acc[name]))
        step("wsum", wk)
        step("dep", mul(z[:, k], wk))
        for d in range(3):
            step(f"col{d}", mul(c[d][:, k], wk))
            step(f"nrm{d}", live(mul(g[d][:, k], wk), mk[:, k]))
        step("ge", live(mul(nr[:, k], nr[:, k]), mk[:, k]))
    tot = {k: _wave_tree_sum(v) for k, v in acc.items()}
    dep = acc["dep"] if _wrong == "var_depth" else E(tot["dep"].v[:, None], tot["dep"].e[:, None])
    var = zero
    for k in range(nc):
        dz = sub(z[:, k], dep)
        var = R.sel(on[:, k], add(var, mul(mul(dz, dz), w[:, k])), var)
    gs = np.broadcast_to(np.asarray(gerr_scale, np.float32).astype(np.float64), (n,))
    return {"color": _stack([tot[f"col{d}"] for d in range(3)]), "depth": tot["dep"], "depth_var": _wave_tree_sum(var),
            "normal": _stack([tot[f"nrm{d}"] for d in range(3)]), "weight_sum": tot["wsum"],
            "grad_err": mul(tot["ge"], gs)}


def piece_mean_scale(n, s, batch, piece):
    """per ray: f32(1 / (n_piece s)) of its piece (neus_ray_kernel's piece_mean)"""
    out = np.empty(n)
    for k, (r0, r1) in enumerate(pieces(n, batch, piece)):
        out[r0:r1] = np.float32(1.0 / ((r1 - r0) * s))
    return out


def pieces(n, batch, piece):
    """gs_piece_range for every piece: [(r0, r1)]"""
    out = []
    for b0 in range(0, n, batch):
        b1 = min(b0 + batch, n)
        out += [(r0, min(r0 + piece, b1)) for r0 in range(b0, b1, piece)]
    return out


def piece_sum(gerr_ray, n, batch, piece):
    """neus_piece_sum_kernel: fp64 sums of the f32 per-ray values, rounded once to f32: (value, bound) per piece"""
    g = np.asarray(gerr_ray, np.float32).astype(np.float64)
    out = []
    for r0, r1 in pieces(n, batch, piece):
        v = float(np.sum(g[r0:r1]))
        a = float(np.sum(np.abs(g[r0:r1])))
        out.append((v, U * abs(v) + 2.0 ** -45 * a + (ETA if a > 0 else 0.0)))
    return np.array(out)


# -------------------------------------------------------------------------------------------------- point stage ----
def z_mid_mask(rays_o, rays_d, z_vals, dists, s, rt_bound):
    """point_of: z_mid f32 [N] and the realtime-bound mask (strict inequalities) of every point, in fp32"""
    F = np.float32
    zv, dv = np.asarray(z_vals, F).reshape(-1), np.asarray(dists, F).reshape(-1)
    zm = (zv + (dv / F(2)).astype(F)).astype(F)
    pt = positions(rays_o, rays_d, zv, dv, s, R.BOUND)[0]
    rb = np.asarray(rt_bound, F).reshape(6)
    m = np.ones(zm.shape, bool)
    for d in range(3):
        m &= (pt[:, d] < rb[2 * d + 1]) & (pt[:, d] > rb[2 * d])
    return zm, m


def forced_mask(mask, s, n, batch, piece):
    """the force pass: per piece with no point in bound, its first min(100, n_piece s) points are live"""
    m = np.array(mask, bool).reshape(-1)
    for r0, r1 in pieces(n, batch, piece):
        p0, p1 = r0 * s, r1 * s
        if not m[p0:p1].any():
            m[p0:min(p0 + 100, p1)] = True
    return m


def point_fwd(rays_o, rays_d, z_vals, dists, s, grid16, sdf_w, sdf_b, color_B, inv_s, bound, live_mask, meta):
    """neus_point_kernel's per-point outputs for the live points `live_mask` [N] (the realtime mask, after the force
    pass).  Returns dict: idx (live point indices), pts f32 [N, 3]; E over the live points: sdf, grad [., 3], alpha,
    mlp_in [., 80] (fp16), enc_aux [16, ., 8] (fp16); gates {'cos': count, 'clip': count}."""
    F = np.float32
    zv, dv = np.asarray(z_vals, F).reshape(-1), np.asarray(dists, F).reshape(-1)
    pt, qn, inside, view, span = positions(rays_o, rays_d, zv, dv, s, bound)
    idx = np.nonzero(np.asarray(live_mask, bool).reshape(-1))[0]
    n = idx.size
    ray = idx // s
    W = np.asarray(sdf_w, F).astype(np.float64)
    b = np.asarray(sdf_b, F).astype(np.float64)
    B = np.asarray(color_B, F).astype(np.float64).reshape(3, 33)
    g16 = np.asarray(grid16, np.float16).astype(np.float64).reshape(-1, 2)
    p = qn[idx].astype(np.float64)
    vw = view[idx]
    out = E(np.zeros((n, 32)))
    for d in range(3):
        out = fma(W[:, d][None], p[:, d:d + 1], out) if d else mul(W[:, d][None], p[:, d:d + 1])
    gview = [E(np.zeros(n)) for _ in range(3)]
    aux = []
    for l in range(LEVELS):
        scale = float(np.float32(meta["scale"][l]))
        gi, f = cells(vw, scale)
        vals = g16[grid_corners(meta, l, gi) + int(meta["offset"][l])]          # [n, 8, 2]
        fr = [E(f[:, d]) for d in range(3)]
        om = [sub(1.0, fr[d]) for d in range(3)]
        val = [E(np.zeros(n)), E(np.zeros(n))]
        for c in range(8):
            w = E(np.ones(n))
            for d in range(3):
                w = mul(w, fr[d] if (c >> d) & 1 else om[d])
            val = [fma(w, vals[:, c, ft], val[ft]) for ft in range(2)]
        dv_ = []
        for gd in range(3):
            o0, o1 = (1 if gd == 0 else 0), (1 if gd == 2 else 2)
            a = [E(np.zeros(n)), E(np.zeros(n))]
            for k in range(4):
                w = mul(mul(scale, fr[o0] if k & 1 else om[o0]), fr[o1] if k & 2 else om[o1])
                cl = ((k & 1) << o0) | (((k >> 1) & 1) << o1)
                cr = cl | (1 << gd)
                a = [fma(w, sub(vals[:, cr, ft], vals[:, cl, ft]), a[ft]) for ft in range(2)]
            dv_.append(a)
        e0, e1 = round16(val[0]), round16(val[1])
        aux.append(_stack([e0, e1] + [round16(dv_[gd][0]) for gd in range(3)] + [round16(dv_[gd][1]) for gd in range(3)]))
        g0, g1 = float(R.h16(W[0, 3 + 2 * l])), float(R.h16(W[0, 4 + 2 * l]))
        for d in range(3):
            gview[d] = add(gview[d], fma(g1, dv_[d][1], mul(g0, dv_[d][0])))
        out = fma(W[:, 4 + 2 * l][None], E(e1.v[:, None], e1.e[:, None]),
                  fma(W[:, 3 + 2 * l][None], E(e0.v[:, None], e0.e[:, None]), out))
    out = add(out, b[None])
    sdf = out[:, 0]
    grad = [div(mul(live(add(W[0, d], div(gview[d], 2.0)), inside[idx, d]), 2.0), float(span[d])) for d in range(3)]
    dirs = np.asarray(rays_d, F).astype(np.float64)[ray]
    cosv = add(add(mul(dirs[:, 0], grad[0]), mul(dirs[:, 1], grad[1])), mul(dirs[:, 2], grad[2]))
    gates = {"cos": int(((np.abs(cosv.v) <= cosv.e) & (cosv.e > 0)).sum())}
    ic = E(np.minimum(cosv.v, 0.0), cosv.e)                 # -max(-cos, 0): 1-Lipschitz
    half = div(mul(ic, dv[idx].astype(np.float64)), 2.0)
    inv = float(np.float32(inv_s))
    pc = sigmoid(mul(sub(sdf, half), inv))
    nc = sigmoid(mul(add(sdf, half), inv))
    raw = div(add(sub(pc, nc), C5), add(pc, C5))
    gates["clip"] = int(((np.abs(raw.v) <= raw.e) | (np.abs(raw.v - 1.0) <= raw.e)).sum())
    alpha = E(np.clip(raw.v, 0.0, 1.0), np.minimum(raw.e, 1.0))
    P = pt[idx].astype(np.float64)
    row = []
    for c in range(33):
        arg = add(add(mul(P[:, 0], B[0, c]), mul(P[:, 1], B[1, c])), mul(P[:, 2], B[2, c]))
        row.append(round16(E(np.sin(arg.v), arg.e + COS_ABS)))
    row += [round16(grad[d]) for d in range(3)]
    row += [round16(out[:, 1 + k]) for k in range(31)]
    row += [E(np.ones(n))] * 13
    return {"idx": idx, "pts": pt, "sdf": sdf, "grad": _stack(grad), "alpha": alpha, "mlp_in": _stack(row),
            "enc_aux": _stack(aux, 0), "gates": gates}
