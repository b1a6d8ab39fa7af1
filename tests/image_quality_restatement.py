"""NumPy fp64 restatement of gs_image_quality (include/goslam_neus.h; kernel in go_slam_amd/csrc/image_quality.hip), with
a running forward-error bound beside every output.

Independent order of summation.  The kernel filters separably (11 horizontal taps, then 11 vertical taps of the row
results) and reduces per thread, per wave, per workgroup and over workgroups.  Here every window moment is the direct
sum of its 121 taps, weight w[r][c] = g[r] g[c], in row-major tap order, and every image-wide sum is math.fsum (exactly
rounded).  Nothing of the kernel's order is repeated, so agreement is not an artefact of sharing one.

The bound.  u = 2^-53.  A sum of terms a_k evaluated in ANY order with a chain of at most L rounded operations from a
term's inputs to the result differs from the exact sum by at most L u sum|a_k| to first order (Higham, Accuracy and
Stability of Numerical Algorithms, 4.2); an error d_k already in a term adds sum|d_k|.  Each stage below counts L for
the LONGER of the two chains (this file's and the kernel's) and carries sum|a_k| and sum|d_k| along; products and
quotients follow the product rule with the second-order terms kept.  Both the kernel and this restatement obey the bound
against the exact value, so the two differ by at most TWICE the bound: that is the tolerance of
tests/test_image_quality_gpu.py, no constant is chosen.

Two constants are counted rather than chosen:
  WEIGHT_REL   the weights.  g_k = exp(.) / sum: exp within 1 ulp (2 u) in glibc, the device library and NumPy alike, the
               sum of 11 positive terms 11 u, the division u: 14 u per g_k.  A tap's weight is g_r g_c (formed here,
               applied one factor at a time in the kernel): 2 x 14 u + u = 29 u relative, whichever library made it.
  LOG10_ULPS   log10 in fp64: 2 ulp in glibc's table for x86-64, 1 ulp in the device library's; 2 is taken, and an ulp
               is at most 2 u relative.
"""
import math

import numpy as np

U = 2.0 ** -53
TAPS = 11
APRON = TAPS - 1
C1 = 0.01 * 0.01            # the same two roundings as the kernel's constants
C2 = 0.03 * 0.03
WEIGHT_REL = 29 * U
LOG10_ULPS = 2
TILE = (16, 32)             # GS_IQ_TILE_H, GS_IQ_TILE_W: only the chain lengths of the image-wide sums depend on it
THREADS = 256

KEYS = ("mse", "psnr", "ssim", "depth_l1", "n_depth", "n_windows", "reserved0", "reserved1")


def gaussian_window():
    """g_k = exp(-(k-5)^2 / 4.5) / sum, fp64 [11]"""
    k = np.arange(TAPS, dtype=np.float64) - APRON // 2
    e = np.exp(-(k * k) / 4.5)
    return e / e.sum()


# chain of one window moment: the weight product, the square or product of the two values, the tap's multiplication and
# 121 additions here (124); in the kernel the value product, two multiplications and two runs of 11 additions (25)
L_MOMENT = 1 + 1 + 1 + TAPS * TAPS


def reduction_chain(n_blocks, per_thread):
    """additions between a term and the kernel's image-wide sum: a thread's own terms in a row, the wave butterfly (6),
    the four waves (3); then in the last workgroup the serial adds over workgroups, the butterfly and the waves again.
    (math.fsum here rounds once.)"""
    return per_thread + 6 + 3 + (n_blocks + THREADS - 1) // THREADS + 6 + 3


def tiles(H, W, tile=TILE):
    th, tw = tile
    return (H - APRON + th - 1) // th, (W - APRON + tw - 1) // tw


def window_moments(x, y, accumulate=np.float64):
    """x, y fp32 [H,W,3] -> dict of fp64 [H-10, W-10, 3] arrays: the moments `x`, `y`, `xx`, `yy`, `xy` and, per moment,
    `b_*`: its error bound.  accumulate=np.float32 forms the products and runs the 121-tap sums in fp32 instead (what a
    kernel without fp64 moments would do); the bounds stay those of fp64."""
    x = np.asarray(x, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    assert x.shape == y.shape and x.ndim == 3 and x.shape[2] == 3
    H, W = x.shape[:2]
    assert H >= TAPS and W >= TAPS
    hv, wv = H - APRON, W - APRON
    g = gaussian_window()
    w2 = g[:, None] * g[None, :]
    xa, ya = x.astype(accumulate), y.astype(accumulate)
    terms = {"x": xa, "y": ya, "xx": xa * xa, "yy": ya * ya, "xy": xa * ya}
    x64, y64 = np.abs(x.astype(np.float64)), np.abs(y.astype(np.float64))
    mags = {"x": x64, "y": y64, "xx": x64 * x64, "yy": y64 * y64, "xy": x64 * y64}
    out = {k: np.zeros((hv, wv, 3), dtype=accumulate) for k in terms}
    mag = {k: np.zeros((hv, wv, 3), dtype=np.float64) for k in terms}
    for r in range(TAPS):
        for c in range(TAPS):
            w = accumulate(w2[r, c])
            for k in terms:
                out[k] = out[k] + w * terms[k][r:r + hv, c:c + wv]
                mag[k] = mag[k] + w2[r, c] * mags[k][r:r + hv, c:c + wv]
    res = {k: v.astype(np.float64) for k, v in out.items()}
    for k in terms:
        res["b_" + k] = (L_MOMENT * U + WEIGHT_REL) * mag[k] * (1 + 2 * L_MOMENT * U)
    return res


def ssim_map(m):
    """moments -> (s, d_s, parts): the index of every window, its bound, and the intermediate values by name"""
    mx, my = m["x"], m["y"]
    bx, by = m["b_x"], m["b_y"]
    mxx, myy, mxy = mx * mx, my * my, mx * my
    d_mxx = 2 * np.abs(mx) * bx + bx * bx + U * np.abs(mxx)
    d_myy = 2 * np.abs(my) * by + by * by + U * np.abs(myy)
    d_mxy = np.abs(mx) * by + np.abs(my) * bx + bx * by + U * np.abs(mxy)
    vx, vy, cov = m["xx"] - mxx, m["yy"] - myy, m["xy"] - mxy
    d_vx = m["b_xx"] + d_mxx + U * np.abs(vx)
    d_vy = m["b_yy"] + d_myy + U * np.abs(vy)
    d_cov = m["b_xy"] + d_mxy + U * np.abs(cov)
    A = (mxy + mxy) + C1
    B = (cov + cov) + C2
    C = (mxx + myy) + C1
    D = (vx + vy) + C2
    d_A = 2 * d_mxy + U * np.abs(A)
    d_B = 2 * d_cov + U * np.abs(B)
    d_C = d_mxx + d_myy + 2 * U * np.abs(C)
    d_D = d_vx + d_vy + 2 * U * np.abs(D)
    num, den = A * B, C * D
    d_num = np.abs(A) * d_B + np.abs(B) * d_A + d_A * d_B + U * np.abs(num)
    d_den = np.abs(C) * d_D + np.abs(D) * d_C + d_C * d_D + U * np.abs(den)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = num / den
        room = np.abs(den) - d_den
        d_s = np.where(room > 0, (d_num + np.abs(s) * d_den) / room + U * np.abs(s), np.inf)
    d_s = np.where(np.isnan(s), np.nan, d_s)
    return s, d_s, {"vx": vx, "vy": vy, "cov": cov, "d_vx": d_vx, "d_vy": d_vy, "d_cov": d_cov}


def _fsum(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    if np.isnan(a).any():
        return float("nan")
    if np.isinf(a).any():
        return float(a.sum())
    return math.fsum(a.tolist())


def image_quality(pred_rgb, gt_rgb, pred_depth=None, gt_depth=None, accumulate=np.float64, tile=TILE):
    """pred_rgb, gt_rgb fp32 [H,W,3]; pred_depth, gt_depth fp32 [H,W] or both None -> (out fp64 [8], bound fp64 [8]) in
    the kernel's layout: mse, psnr, ssim, depth_l1, n_depth, n_windows, 0, 0.  The counts are exact (bound 0)."""
    x = np.asarray(pred_rgb, dtype=np.float32)
    y = np.asarray(gt_rgb, dtype=np.float32)
    if x.shape != y.shape or x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("image_quality: pred_rgb and gt_rgb must both be [H,W,3]")
    H, W = x.shape[:2]
    if H < TAPS or W < TAPS:
        raise ValueError(f"image_quality: a {H} x {W} image is smaller than the {TAPS} x {TAPS} window")
    if (pred_depth is None) != (gt_depth is None):
        raise ValueError("image_quality: pred_depth and gt_depth are given both or neither")
    th, tw = tile
    ty, tx = tiles(H, W, tile)
    nblk = tx * ty
    out, bound = np.zeros(8), np.zeros(8)

    # colour error: d = x - y (1 rounding, relative u), d^2 (1), the sum, the division
    d = x.astype(np.float64) - y.astype(np.float64)
    sq = d * d
    n_values = 3.0 * H * W
    s_sq = _fsum(sq)
    L = reduction_chain(nblk, -(-(th + APRON) * (tw + APRON) * 3 // THREADS))
    mse = s_sq / n_values
    b_mse = (3 + L + 1) * U * s_sq / n_values if not math.isnan(s_sq) else float("nan")
    out[0], bound[0] = mse, b_mse
    if math.isnan(mse):
        out[1], bound[1] = float("nan"), float("nan")
    elif mse == 0.0:
        out[1], bound[1] = float("inf"), 0.0
    else:
        lg = math.log10(mse)
        out[1] = -10.0 * lg
        room = mse - b_mse
        bound[1] = (10.0 / math.log(10.0)) * b_mse / room + 10.0 * LOG10_ULPS * 2 * U * abs(lg) + U * abs(out[1]) \
            if room > 0 else float("inf")

    # structural similarity
    m = window_moments(x, y, accumulate)
    s, d_s, _ = ssim_map(m)
    n_windows = 3.0 * (H - APRON) * (W - APRON)
    s_s = _fsum(s)
    L = reduction_chain(nblk, 3 * -(-th * tw // THREADS))
    out[2] = s_s / n_windows
    bound[2] = (_fsum(d_s) + L * U * _fsum(np.abs(s))) / n_windows + U * abs(out[2])
    out[5] = n_windows

    # depth error over the pixels with a measurement
    out[3], bound[3] = float("nan"), float("nan")
    if gt_depth is not None:
        p = np.asarray(pred_depth, dtype=np.float32).astype(np.float64).reshape(H, W)
        g32 = np.asarray(gt_depth, dtype=np.float32).reshape(H, W)
        valid = g32 > 0
        n = int(valid.sum())
        out[4] = float(n)
        if n:
            t = np.abs(p[valid] - g32.astype(np.float64)[valid])
            s_t = _fsum(t)
            L = reduction_chain(nblk, -(-(th + APRON) * (tw + APRON) // THREADS))
            out[3] = s_t / n
            bound[3] = (1 + L + 1) * U * s_t / n if not math.isnan(s_t) else float("nan")
    return out, bound


# ---------------------------------------------------------------------------------------------- a test input ------
CANCEL_AMPLITUDE = 1e-3      # separates fp32 from fp64 moments by a factor of ~1e6 (test_image_quality_cpu prints it)


def cancelling_pair(H=11, W=12, amplitude=CANCEL_AMPLITUDE, seed=6):
    """Two images of 0.9 plus independent uniform noise of the given amplitude: window variances of amplitude^2 / 3
    under E[x^2] of 0.81."""
    r = np.random.default_rng(seed)
    x = (0.9 + amplitude * (2 * r.random((H, W, 3)) - 1)).astype(np.float32)
    y = (0.9 + amplitude * (2 * r.random((H, W, 3)) - 1)).astype(np.float32)
    return x, y
