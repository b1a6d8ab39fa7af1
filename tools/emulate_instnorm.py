"""The statistics scheme of go_slam_amd/csrc/instnorm.hip restated in NumPy fp32 (developer / CPU-test tool): per
256-pixel chunk the sums of d = x - k and d^2 with k = the chunk's first pixel, accumulated per thread (4 samples in
flight, `lanes` threads per channel group) and added through LDS; chunk moments (n, mean, M2); Chan merges of the chunks
in the order instnorm_final_kernel uses (per channel `per` threads take every per-th chunk, 8 at a time, then the
threads' results are merged in thread order); and the apply kernel's rounding chain."""
import numpy as np

IN_CHUNK = 256
f32 = np.float32


def merge(a, b):
    """Chan et al. on (n, mean, M2) triples, fp32, as `merge` in instnorm.hip"""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    n = f32(a[0] + b[0])
    d = f32(b[1] - a[1])
    f = f32(b[0] / n)
    return (n, f32(a[1] + d * f), f32(f32(a[2] + b[2]) + f32(f32(d * d) * a[0]) * f))


def chunk_moments(x, c):
    """x [pixels, c] fp16 (bias already added): (n, mean, M2) per channel of one chunk, thread by thread"""
    c8n = c // 8
    lanes = 256 // c8n
    k = x[0].astype(f32)
    s1 = np.zeros((lanes, c), f32)
    s2 = np.zeros((lanes, c), f32)
    for pl in range(lanes):
        for p in range(pl, x.shape[0], lanes):
            d = x[p].astype(f32) - k
            s1[pl] = s1[pl] + d
            s2[pl] = (d * d + s2[pl]).astype(f32)           # fmaf: one rounding
    a1 = np.zeros(c, f32)
    a2 = np.zeros(c, f32)
    for pl in range(lanes):                                  # the LDS column sums, lane after lane
        a1 = a1 + s1[pl]
        a2 = a2 + s2[pl]
    n = f32(x.shape[0])
    mean = k + a1 / n
    m2 = np.maximum(a2 - a1 * a1 / n, f32(0))
    return n, mean.astype(f32), m2.astype(f32)


def image_stats(x, eps=1e-5):
    """x [hw, c] fp16 -> (mean, invstd) fp32 per channel, as instnorm_stats_kernel + instnorm_final_kernel"""
    hw, c = x.shape
    chunks = [chunk_moments(x[p0:p0 + IN_CHUNK], c) for p0 in range(0, hw, IN_CHUNK)]
    nblk = len(chunks)
    per = 256 // min(c, 256)
    mean = np.zeros(c, f32)
    invstd = np.zeros(c, f32)
    for ch in range(c):
        parts = []
        for part in range(per):
            acc = (f32(0), f32(0), f32(0))
            for b in range(part, nblk, per):
                n, m, m2 = chunks[b]
                acc = merge(acc, (n, m[ch], m2[ch]))
            parts.append(acc)
        r = parts[0]
        for q in range(1, per):
            r = merge(r, parts[q])
        var = f32(r[2] / r[0]) if r[0] > 0 else f32(0)
        mean[ch] = r[1]
        invstd[ch] = f32(1.0) / np.sqrt(f32(var + f32(eps)), dtype=f32)
    return mean, invstd


def norm_act(x, bias, skip, instance, relu_in, relu_out, eps=1e-5):
    """the whole gs_norm_act on one image: x, skip [hw, c] fp16, bias [c] fp16 or None"""
    v = x
    if bias is not None:
        v = (x.astype(f32) + bias.astype(f32)).astype(np.float16)
    if instance:
        mean, invstd = image_stats(v, eps)
        v = ((v.astype(f32) - mean) * invstd).astype(np.float16)
    if relu_in:
        v = np.maximum(v, np.float16(0))
    if skip is not None:
        v = (skip.astype(f32) + v.astype(f32)).astype(np.float16)
    if relu_out:
        v = np.maximum(v, np.float16(0))
    return v


# ---- the statistics gs_enc_conv leaves in its epilogue (stats_ws) and instnorm_final_sums_kernel merges -------------------

def enc_waves(ho, wo, c):
    """The epilogue's geometry (enc_conv.hip, 1 <= c / 32 m-tiles): per workgroup, the list of its waves as
    (m-tile, output row, first column); a wave covers 32 channels x up to 32 pixels of one row."""
    mtiles = c // 32
    groups_x = (wo + 31) // 32
    waves = ho * groups_x * mtiles
    nblk = (waves + 3) // 4
    out = []
    for blk in range(nblk):
        ws = []
        for wv in range(4):
            wid = blk * 4 + wv
            if wid >= waves:
                continue
            pg = wid // mtiles
            ws.append((wid % mtiles, pg // groups_x, 32 * (pg % groups_x)))
        out.append(ws)
    return out


def _tree32(x):
    """the half-wave reduce-scatter (gs_rs_step with masks 16, 8, 4, 2, 1) over 32 pixel rows: pairs (r, r + m)"""
    for m in (16, 8, 4, 2, 1):
        x = x[:m] + x[m:2 * m]
    return x[0]


def _wave_tile(v, oy, ox0, c0):
    """the 32 x 32 block of one wave as float32 (pixels past the row end read as 0 with a count of valid pixels)"""
    wo = v.shape[1]
    nvalid = min(32, wo - ox0)
    t = np.zeros((32, 32), f32)
    t[:nvalid] = v[oy, ox0:ox0 + nvalid, c0:c0 + 32].astype(f32)
    return t, nvalid


def fused_sums_stats(v, stat_bias=None, eps=1e-5):
    """The epilogue statistics as they were: per workgroup the fp32 sums of d = v - stat_bias and d^2 (per wave a
    32-pixel tree, then the four wave slabs added in wave order), then instnorm_final_sums_kernel: per channel
    `per` = 1024 / c threads add every per-th slab in ascending order, thread 0 adds the parts, then
    mean = bias + S1 / N and var = S2 / N - (S1 / N)^2 in fp64 from the fp32 totals.
    v [ho, wo, c] fp16 = half(half(conv) + stat_bias), the tensor the norm sees."""
    ho, wo, c = v.shape
    b = np.zeros(c, f32) if stat_bias is None else stat_bias.astype(f32)
    slabs = []
    for ws in enc_waves(ho, wo, c):
        red = np.zeros((4, c, 2), f32)
        for wv, (mt, oy, ox0) in enumerate(ws):
            t, nvalid = _wave_tile(v, oy, ox0, 32 * mt)
            d = t - b[32 * mt:32 * mt + 32]
            d[nvalid:] = 0
            red[wv, 32 * mt:32 * mt + 32, 0] = _tree32(d)
            red[wv, 32 * mt:32 * mt + 32, 1] = _tree32((d * d).astype(f32))
        slabs.append(((red[0] + red[1]) + red[2]) + red[3])
    slabs = np.stack(slabs)                                  # [nblk, c, 2]
    per = 1024 // c
    parts = np.zeros((per, c, 2), f32)
    for part in range(per):
        for blk in range(part, len(slabs), per):
            parts[part] = parts[part] + slabs[blk]
    tot = parts[0].copy()
    for q in range(1, per):
        tot = tot + parts[q]
    n = float(ho * wo)
    mean_d = tot[:, 0].astype(np.float64) / n
    var = np.maximum(tot[:, 1].astype(np.float64) / n - mean_d * mean_d, 0.0)
    return (b + mean_d.astype(f32)).astype(f32), (1.0 / np.sqrt(var + eps)).astype(f32)


def fused_moments_stats(v, stat_bias=None, eps=1e-5):
    """The epilogue statistics as they are: every wave shifts its sums by its own first pixel k (per channel),
    d = v - k, 32-pixel trees of d and d^2 -> (n, mean = k + S1 / n, M2 = S2 - S1 * (S1 / n)); the workgroup merges
    its waves' moments (shifted by the first covering wave's mean, one division) and publishes (n, mean, M2);
    instnorm_final_sums_kernel then
    adds, per channel in fp64, n (mean - K) and M2 + n (mean - K)^2 with K = slab 0's mean (slab 1's where slab 0
    does not cover the channel: 256 channels), per thread in ascending slab order, then the threads' parts as a tree.
    (stat_bias only forms v: the statistics no longer depend on it.)"""
    ho, wo, c = v.shape
    slabs = []
    for ws in enc_waves(ho, wo, c):
        red = [[(f32(0), f32(0), f32(0))] * c for _ in range(4)]
        for wv, (mt, oy, ox0) in enumerate(ws):
            t, nvalid = _wave_tile(v, oy, ox0, 32 * mt)
            k = t[0].copy()
            d = (t - k).astype(f32)
            d[nvalid:] = 0
            s1 = _tree32(d)
            s2 = _tree32((d * d).astype(f32))
            nf = f32(nvalid)
            m = (s1 / nf).astype(f32)
            mean = (k + m).astype(f32)
            m2 = np.maximum((s2 - (s1 * m).astype(f32)).astype(f32), f32(0))
            for j in range(32):
                red[wv][32 * mt + j] = (nf, mean[j], m2[j])
        slab = []
        for ch in range(c):                                  # red_publish: one division
            n_ = [red[wv][ch][0] for wv in range(4)]
            m_ = [red[wv][ch][1] for wv in range(4)]
            q_ = [red[wv][ch][2] for wv in range(4)]
            mr = next((m_[wv] for wv in range(3) if n_[wv] > 0), m_[3])
            N = S = Q = f32(0)
            for wv in range(4):
                dm = f32(m_[wv] - mr)
                N = f32(N + n_[wv])
                S = f32(S + f32(n_[wv] * dm))
                Q = f32(Q + f32(q_[wv] + f32(f32(n_[wv] * dm) * dm)))
            ds = f32(S / N) if N > 0 else f32(0)
            slab.append((N, f32(mr + ds), max(f32(Q - f32(S * ds)), f32(0))))
        slabs.append(slab)
    nblk = len(slabs)
    per = 1024 // c
    mean = np.zeros(c, f32)
    invstd = np.zeros(c, f32)
    for ch in range(c):
        K = float(slabs[0][ch][1] if slabs[0][ch][0] > 0 else slabs[min(1, nblk - 1)][ch][1])
        N = A = B = 0.0
        parts = []
        for part in range(per):
            N = A = B = 0.0
            for blk in range(part, nblk, per):
                n_, m_, m2_ = (float(x) for x in slabs[blk][ch])
                dm = m_ - K
                N += n_
                A += n_ * dm
                B += m2_ + n_ * dm * dm
            parts.append([N, A, B])
        half = per // 2
        while half >= 1:                                     # the parts added as a binary tree
            for p in range(half):
                parts[p] = [parts[p][i] + parts[p + half][i] for i in range(3)]
            half //= 2
        tot = parts[0]
        md = tot[1] / tot[0]
        var = max(tot[2] / tot[0] - md * md, 0.0)
        mean[ch] = f32(K + md)
        invstd[ch] = f32(1.0 / np.sqrt(var + eps))
    return mean, invstd
