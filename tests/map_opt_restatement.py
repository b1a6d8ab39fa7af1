"""fp64 restatement of the mapper step's small kernels (go_slam_amd/csrc/map_opt.hip), host only.

The contracts are the ones include/goslam_neus.h states for gs_map_grad_sqnorm, gs_map_adamw(_seg), gs_map_step_prep,
gs_map_gram and gs_map_step_post; the optimiser's is the reference's own (src/mapping.py:55-58,135-137):
clip_grad_norm_(35, error_if_nonfinite=False) over every trained parameter, then torch.optim.AdamW with two groups.
Every function here evaluates its contract in float64 from the kernels' own fp16 / fp32 inputs (scalars that reach a
kernel as `float` are rounded to float32 first by the caller, `f32()`), so the difference to a kernel is the kernel's
rounding alone.  The Gram functions take torch tensors (the large shapes are evaluated in fp64 on the device); the
rest take numpy arrays.

Besides the restatement this module holds the error bounds the GPU tests apply (u = 2^-24, fp32's unit roundoff;
a chain of m fp32 additions of terms t_i is within m u sum |t_i| of the exact sum)."""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32

# the dense-gradient buffer gs_map_step_post writes: [mlp 10240 | sdf_w 32x35 | sdf_b 32 | color_B 3x33 | variance | loss]
N_MLP, N_W, N_B, N_CB = 10240, 32 * 35, 32, 3 * 33
OFF_W, OFF_B, OFF_CB = N_MLP, N_MLP + N_W, N_MLP + N_W + N_B
OFF_VAR = N_MLP + N_W + N_B + N_CB                      # 11491
OFF_LOSS = OFF_VAR + 1
ND = OFF_VAR + 1                                        # 11492 trained dense parameters (FlatAdamW.nd)


def f32(x):
    """a host scalar as the kernel receives it (ctypes c_float), back in float64"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------- Gram ----
def gram_blocks(n_rows):
    """gs_map_gram_blocks: one workgroup per >= 64 groups of 16 rows, at least 1, at most 256"""
    nb = (n_rows // 16) // 64
    return min(256, max(1, nb))


def gram_split(n_rows):
    """[(row_lo, row_hi)] of every workgroup of gs_map_gram: per = ceil(groups / blocks) groups each, contiguous; the
    trailing workgroups may be empty (lo == hi) when blocks * per overshoots the group count"""
    ng = n_rows // 16
    nb = gram_blocks(n_rows)
    per = -(-ng // nb)
    out = []
    for b in range(nb):
        lo = min(ng, b * per)
        hi = min(ng, lo + per) if b * per < ng else lo
        out.append((16 * lo, 16 * hi))
    return out


def gram_written():
    """bool [40,160]: the entries gs_map_gram forms -- rows 0..31 x columns 32..95 (d_out^T [pts | lin_in | dw0 head]),
    rows 32..39 x columns 0..31 and 64..159 ([pts, 1]^T [d_out | lin_in.. | dw0 | d_arg]); rows 32..39 x columns 32..63
    are not formed"""
    w = torch.zeros(40, 160, dtype=torch.bool)
    w[0:32, 32:96] = True
    w[32:40, 0:32] = True
    w[32:40, 64:160] = True
    return w


def gram(rows):
    """(rows[:, :40]^T rows, |rows[:, :40]|^T |rows|) in float64: the product and the sum of |a_i b_i| per entry"""
    r = rows.double()
    a = r.abs()
    return r[:, :40].T @ r, a[:, :40].T @ a


def gram_partials(rows):
    """per workgroup of gram_split: (partial [nb,40,160], sum |a_i b_i| [nb,40,160]) in float64; empty workgroups 0"""
    n_rows = rows.shape[0]
    split = gram_split(n_rows)
    G = torch.zeros(len(split), 40, 160, dtype=torch.float64, device=rows.device)
    A = torch.zeros_like(G)
    for b, (lo, hi) in enumerate(split):
        if hi > lo:
            G[b], A[b] = gram(rows[lo:hi])
    return G, A


def gram_depth(n_rows):
    """D = 16 ceil(per / 8) + 8: the longest fp32 addition chain behind one partial entry -- a wave takes every 8th of
    the workgroup's `per` groups, one 16-deep MFMA per group, then the fixed 8-wave merge"""
    ng = n_rows // 16
    per = -(-ng // gram_blocks(n_rows))
    return 16 * (-(-per // 8)) + 8


def gram_bound(n_rows, absprod):
    """|G - G64| <= 2 (D + 2) u sum |a_i b_i| (fp16 x fp16 products are exact in fp32; 2x covers gamma vs m u)"""
    return 2 * (gram_depth(n_rows) + 2) * U * absprod


# ------------------------------------------------------------------------------------------------------- post ----
def _post_entries():
    """for every dense output slot e < N_W + N_B + N_CB: the Gram entries (r, c) summed into it"""
    ent = []
    for o in range(32):                                 # d sdf_layer.weight = d_out^T lin_in; row 0 += colsum(dw0)
        for c in range(35):
            ent.append([(o, 40 + c)] + ([(35, 80 + c)] if o == 0 else []))
    for c in range(32):                                 # d bias = colsum(d_out) (row 35 = the ones column)
        ent.append([(35, c)])
    for d in range(3):                                  # d color_B = pts^T d_arg
        for c in range(33):
            ent.append([(32 + d, 120 + c)])
    return ent


POST_ENTRIES = _post_entries()


def post_dense(G):
    """d sdf_w (flat 1120) | d sdf_b (32) | d color_B (flat 99) from one summed, unscaled Gram matrix [40,160] (any
    dtype, numpy or torch): the index map of gs_map_step_post"""
    G = np.asarray(G, np.float64)
    return np.array([sum(G[r, c] for r, c in e) for e in POST_ENTRIES])


def variance_gate(variance, scale_factor):
    """d variance flows only where inv_s = clamp(exp(variance * scale), 1e-6, 1e6) is not clamped"""
    raw = math.exp(variance * scale_factor)
    return 1e-6 <= raw <= 1e6


def post(gram_chunks, inv_ls, mlp_partial, d_invs, variance, inv_s, scale_factor, loss_rays, gerr, w_eik, s, counts):
    """(g32 [ND + 1] float64: mlp | sdf_w | sdf_b | cB | d variance | loss, bound [ND + 1]).  gram_chunks [nchunk,40,160]
    and mlp_partial [nb,10240] are summed over their first axis and scaled by inv_ls; the bound per slot is
    (2 ceil(m / 8) + 10) u sum |terms| with m the number of partials (nchunk or nb), the 2 for sdf_w row 0 which adds
    two Gram entries per chunk in one chain; for the loss (2 ceil(n / 256) + 12) u sum |terms| (256 lanes over n rays,
    the wave and workgroup sums, and the eikonal term's three roundings); 3 u for d variance (two products)"""
    gram_chunks = np.asarray(gram_chunks, np.float64)
    mlp_partial = np.asarray(mlp_partial, np.float64)
    nchunk, nb = gram_chunks.shape[0], mlp_partial.shape[0]
    out = np.zeros(ND + 1)
    bnd = np.zeros(ND + 1)
    k_chunk = 2 * (-(-nchunk // 8)) + 10
    out[:N_MLP] = mlp_partial.sum(0) * inv_ls
    bnd[:N_MLP] = (2 * (-(-nb // 8)) + 10) * U * np.abs(mlp_partial).sum(0) * abs(inv_ls)
    with np.errstate(invalid="ignore"):
        out[OFF_W:OFF_VAR] = post_dense(gram_chunks.sum(0)) * inv_ls
    bnd[OFF_W:OFF_VAR] = k_chunk * U * post_dense(np.abs(gram_chunks).sum(0)) * abs(inv_ls)
    dv = d_invs * scale_factor * inv_s if variance_gate(variance, scale_factor) else 0.0
    out[OFF_VAR] = dv
    bnd[OFF_VAR] = 3 * U * abs(dv)
    loss_rays = np.asarray(loss_rays, np.float64)
    gerr = np.asarray(gerr, np.float64)
    n = loss_rays.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        out[OFF_LOSS] = loss_rays.sum() + w_eik * gerr.sum() / (counts[1] * s)
        absum = np.abs(loss_rays).sum() + abs(w_eik) * np.abs(gerr).sum() / (counts[1] * s)
    bnd[OFF_LOSS] = (2 * (-(-n // 256)) + 12) * U * absum
    return out, bnd


# ------------------------------------------------------------------------------------------------------- prep ----
def counts(rays_depth):
    """[valid rays, rays, max depth] with torch's rules: depth > 0 counts (NaN does not), the maximum is NaN if any depth
    is NaN (torch.max), and 0 for an empty batch"""
    d = np.asarray(rays_depth, np.float32).astype(np.float64)
    n = d.shape[0]
    if n == 0:
        mx = 0.0
    elif np.isnan(d).any():
        mx = float("nan")
    else:
        mx = float(d.max())
    return np.array([float((d > 0).sum()), float(n), mx])


def inv_s(variance, scale_factor):
    """clamp(exp(variance * scale), 1e-6, 1e6) with the product rounded to fp32 as the kernel forms it (the exponent's
    relative error would otherwise be |variance * scale| u, not the exponential's own)"""
    x = float(np.float32(np.float32(variance) * np.float32(scale_factor)))
    return min(max(math.exp(x), 1e-6), 1e6)


def prep(rays_depth, variance, scale_factor, w_eik, s, counts_in=None, sdf_w=None, mlp16=None, frag_index=None):
    """dict of gs_map_step_prep's outputs: counts, inv_s, d_gerr [n] (float64), sdf_wt (float32 [1024], the transpose of
    sdf_w [32,35] columns 3..34: sdf_wt[lf * 32 + o] = sdf_w[o][3 + lf]), mlp_wpack (fp16 [20480], the gather
    mlp16[frag_index], 0 where frag_index == 10240)"""
    c = np.asarray(counts_in, np.float32).astype(np.float64) if counts_in is not None else counts(rays_depth)
    n = np.asarray(rays_depth).shape[0] if rays_depth is not None else 0
    with np.errstate(divide="ignore", invalid="ignore"):
        dg = np.float64(w_eik) / np.float64(np.float32(c[1] * s))
    out = {"counts": c, "inv_s": inv_s(variance, scale_factor), "d_gerr": np.full(n, dg)}
    if sdf_w is not None:
        out["sdf_wt"] = np.ascontiguousarray(np.asarray(sdf_w, np.float32).reshape(32, 35)[:, 3:].T).reshape(-1)
    if mlp16 is not None:
        ext = np.concatenate([np.asarray(mlp16, np.float16).reshape(-1), np.zeros(1, np.float16)])
        out["mlp_wpack"] = ext[np.asarray(frag_index)]
    return out


# ---------------------------------------------------------------------------------------------------- sqnorm ----
def sqnorm(g16, inv_scale16, g32):
    """sum (g16 * inv_scale16)^2 + sum g32^2 in float64 (NaN if any term is NaN, +inf if any is infinite)"""
    a = np.asarray(g16, np.float16).astype(np.float64) * inv_scale16
    b = np.asarray(g32, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return float((a * a).sum() + (b * b).sum())


def sqnorm_blocks(n16, n32):
    """gs_map_grad_sqnorm's workgroup count: one per 256 work items (8 fp16 or 1 fp32 each), 1 .. 256"""
    return min(256, max(1, -(-(n16 // 8 + n32) // 256)))


def sqnorm_rel_bound(n16, n32):
    """relative error bound (all terms are positive): (8 ceil(n8 / stride) + 8 + n32 / stride + 300) u with stride =
    256 blocks -- a lane's chain through the 8-deep unrolled loop, its remainder and tails, the wave and workgroup sums
    and up to 256 workgroup atomics"""
    stride = 256 * sqnorm_blocks(n16, n32)
    n8 = n16 // 8
    return (8 * (-(-n8 // stride)) + 8 + n32 / stride + 300) * U


# ----------------------------------------------------------------------------------------------- clip + AdamW ----
def clip_coef(total_sq, max_norm):
    """torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): coef = max_norm / (norm + 1e-6) clamped to 1 by
    torch.clamp -- which keeps a NaN (a NaN norm turns every gradient into NaN) -- and 0 for an infinite norm"""
    c = max_norm / (math.sqrt(total_sq) + 1e-6) if not math.isnan(total_sq) else float("nan")
    return c if (c < 1.0 or math.isnan(c)) else 1.0


def clip_adamw(params, grads, lrs, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=35.0, m=None,
               v=None, step0=1, clip=True):
    """clip_grad_norm_ over all groups, then torch.optim.AdamW's update, for len(grads) steps, in float64.

    params: list of float64 arrays (one per group), grads: per step, a list of gradient arrays (one per group), lrs: per
    group.  m / v: initial moments (zeros by default); step0: the step count of the first step (>= 1).  clip=False: no
    clipping (gs_map_adamw_seg with sqnorm == NULL).  Returns (p, m, v, bounds) where bounds[g] = (bp, bm, bv) are the
    per-element error allowances of an fp32 evaluation accumulated over the steps:
        p: 2 ulp32(p_t) + 2^-16 lr |m_hat_t / denom_t|     m: 2 ulp32(m_t) + 2^-16 (b1 |m_{t-1}| + (1 - b1) |g'_t|)
        v: 2 ulp32(v_t) + 2^-16 v_t
    (the clip coefficient, the bias corrections from fp32 powf and the fp32 arithmetic each contribute a few u to the
    relative error of a step's update; 2^-16 = 256 u leaves them room without admitting a wrong formula)."""
    b1, b2 = betas
    ng = len(params)
    p = [np.array(x, np.float64) for x in params]
    m = [np.zeros_like(x) for x in p] if m is None else [np.array(x, np.float64) for x in m]
    v = [np.zeros_like(x) for x in p] if v is None else [np.array(x, np.float64) for x in v]
    bp = [np.zeros_like(x) for x in p]
    bm = [np.zeros_like(x) for x in p]
    bv = [np.zeros_like(x) for x in p]
    with np.errstate(invalid="ignore", over="ignore"):
        for k, gs in enumerate(grads):
            t = step0 + k
            gs = [np.asarray(g, np.float64) for g in gs]
            coef = clip_coef(sum(float((g * g).sum()) for g in gs), max_norm) if clip else 1.0
            bc1 = 1.0 - b1 ** t
            bc2s = math.sqrt(1.0 - b2 ** t)
            for i in range(ng):
                g = gs[i] * coef
                lr = lrs[i]
                m_prev = np.abs(m[i])
                p[i] = p[i] * (1.0 - lr * weight_decay)
                m[i] = b1 * m[i] + (1.0 - b1) * g
                v[i] = b2 * v[i] + (1.0 - b2) * g * g
                denom = np.sqrt(v[i]) / bc2s + eps
                upd = (lr / bc1) * (m[i] / denom)
                p[i] = p[i] - upd
                bp[i] += 2 * ulp32(p[i]) + 2.0 ** -16 * np.abs(upd)
                bm[i] += 2 * ulp32(m[i]) + 2.0 ** -16 * (b1 * m_prev + (1.0 - b1) * np.abs(g))
                bv[i] += 2 * ulp32(v[i]) + 2.0 ** -16 * np.abs(v[i])
    return p, m, v, list(zip(bp, bm, bv))


# ------------------------------------------------------------------------------------------------------ helpers ----
def ulp32(x):
    """spacing of float32 at |x| (NaN / inf propagate)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def ulps32(a, b):
    """integer float32 ulp distance (monotone integer order of the bit patterns)"""
    ai = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    bi = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -2147483648 - ai, ai)
    bi = np.where(bi < 0, -2147483648 - bi, bi)
    return np.abs(ai - bi)


def same_nonfinite(a, b):
    """a and b (float arrays) are NaN at the same places and +-inf at the same places with the same sign"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return bool((np.isnan(a) == np.isnan(b)).all() and (np.isposinf(a) == np.isposinf(b)).all()
                and (np.isneginf(a) == np.isneginf(b)).all())
