"""A float64 referee for the correlation-volume window lookups of csrc/corr_lookup.hip (CPU only: numpy + torch float64).

The model is zero-padded bilinear sampling, not the kernel's loop: tap (i, j) of level l is the bilinear sample of plane l at
(x / 2^l + i - r, y / 2^l + j - r), 0 outside the plane, channel (2r+1)^2 l + (2r+1) i + j.  With fx = floorf(x / 2^l),
dx = x / 2^l - fx (fp32, as the contract says; likewise y) the four corners and their fp32 weights are

    s00 = P[fy + j - r    ][fx + i - r    ]   w_se = (1 - dx) (1 - dy)
    s01 = P[fy + j - r + 1][fx + i - r    ]   w_sw = (1 - dx) dy
    s10 = P[fy + j - r    ][fx + i - r + 1]   w_ne = dx (1 - dy)
    s11 = P[fy + j - r + 1][fx + i - r + 1]   w_nw = dx dy

  lookup_ref    ref = sum s_k w_k, mag = sum |s_k| w_k, ssum = sum |s_k|, all in float64 from the fp32 weights
  lookup_chain  the contract's rounding sequence in the volume's dtype: the weight cast to dtype, then
                ((s00 w_se + s01 w_sw) + s10 w_ne) + s11 w_nw with one rounding per operation
  hard_bound    what any correct execution of that sequence can be off by (derived below)

A non-finite coordinate makes dx or dy NaN, so all four weights and with them every tap of every level of that pixel are
NaN: that is the documented behaviour of every forward entry (include/goslam_hip.h), and both models give it without a
special case.  A non-finite CELL reaches exactly the taps whose four corners include it (inf x 0 = NaN included).

Equality "bit for bit" (`same_bits`) means: the same value, or NaN in both.  The sign of a ZERO result is not pinned --
the reference accumulates into a +0 accumulator, the radius-3 kernels start from the first product, so a sum of -0 terms
is -0 in one and +0 in the other -- and neither is a NaN's payload.

hard_bound, fp16 (u = 2^-11, subnormal spacing 2^-24, so a rounding below 2^-14 is off by at most 2^-25):
  weight    w^ = w (1 + d) + e                  |d| <= u, |e| <= 2^-25      error in the sum: |s| (w u + 2^-25)
  product   p^ = s w^ (1 + d) + e                                           |s| w^ u + 2^-25
  3 sums    each (a + b)(1 + d); a sum of two fp16 numbers that lands in the subnormal range is exact, the +3 below is
            slack.  A term passes at most 5 roundings (its weight, its product, three sums): (1 + u)^5 - 1 <= 5 u (1 + 2^-9)
  total     |y - ref| <= (5 u mag + 2^-25 (ssum + 7)) (1 + 2^-9)
  The issue's form multiplies only the first term by (1 + 2^-9); the absolute floors pass through the later roundings as
  well, which matters once ssum reaches 4 x 65504, so the factor is applied to both.  Only finite results are bounded: an
  fp16 partial sum of 65504-sized terms may overflow, which the bit equality with lookup_chain pins instead.
fp32 / fp64 (u = 2^-24 / 2^-53): the weight cast is exact, four roundings: (4 u mag + 4 tiny) (1 + 2^-9), tiny = the
  smallest subnormal (2^-149 / 2^-1074) for a product that underflows."""
import numpy as np
import torch
import torch.nn.functional as F

NP_DT = {"f16": np.float16, "f32": np.float32, "f64": np.float64}
FAULTS = ("swap_xy", "chan_ji", "trunc", "off_by_one", "clamp_edge", "half_pixel", "tile8_row_below", "fp32_accum")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid="ignore"):
        return (a == b) | (np.isnan(a) & np.isnan(b))


def _corners(plane, cx, cy, radius, fault=None):
    """plane float64 [n,P,hl,wl]; cx, cy fp32 [n,P] (level coordinates) -> (s00, s01, s10, s11) float64 [n,P,rd(j),rd(i)]
    and the four fp32 weights (w_se, w_sw, w_ne, w_nw) [n,P]"""
    assert cx.dtype == np.float32 and cy.dtype == np.float32
    n, P, hl, wl = plane.shape
    rd = 2 * radius + 1
    M = rd + 4
    with np.errstate(invalid="ignore"):
        fl = np.trunc if fault == "trunc" else np.floor
        fx, fy = fl(cx), fl(cy)
        dx, dy = cx - fx, cy - fy                                                   # fp32; NaN for a non-finite coordinate
        one = np.float32(1.0)
        wts = ((one - dx) * (one - dy), (one - dx) * dy, dx * (one - dy), dx * dy)
    assert all(t.dtype == np.float32 for t in wts)
    big = float(max(hl, wl) + 4 * M)
    ix = np.nan_to_num(np.clip(fx.astype(np.float64), -big, big), nan=-big).astype(np.int64)
    iy = np.nan_to_num(np.clip(fy.astype(np.float64), -big, big), nan=-big).astype(np.int64)
    off = np.arange(rd + 1) - radius + (1 if fault == "off_by_one" else 0)
    X = ix[..., None] + off                                                         # [n,P,rd+1]
    Y = iy[..., None] + off
    Y2 = np.broadcast_to(Y[..., :, None], (n, P, rd + 1, rd + 1))
    if fault == "tile8_row_below":                                                  # the second 8-wide tile read one row down
        Y2 = Y2 + ((X >> 3) != (X[..., :1] >> 3))[..., None, :]
    pad = np.pad(plane, ((0, 0), (0, 0), (M, M), (M, M)), mode="edge" if fault == "clamp_edge" else "constant")
    Xp = np.clip(X + M, 0, wl + 2 * M - 1)[..., None, :]
    Yp = np.clip(Y2 + M, 0, hl + 2 * M - 1)
    win = pad[np.arange(n)[:, None, None, None], np.arange(P)[None, :, None, None], Yp, Xp]       # [n,P,y,x]
    return (win[:, :, :rd, :rd], win[:, :, 1:, :rd], win[:, :, :rd, 1:], win[:, :, 1:, 1:]), wts


def _level_coords(coords, l, fault=None):
    c = np.asarray(coords, dtype=np.float32)
    if fault == "swap_xy":
        c = c[..., ::-1]
    inv = np.float32(1.0 / (1 << l))
    if fault == "half_pixel":
        return (c[..., 0] + np.float32(0.5)) * inv - np.float32(0.5), (c[..., 1] + np.float32(0.5)) * inv - np.float32(0.5)
    return c[..., 0] * inv, c[..., 1] * inv                                        # exact (a power of two), fp32


def _channels(t, fault=None):
    """[n,P,j,i] -> [n,P,rd*rd], channel rd i + j"""
    n, P, rd, _ = t.shape
    return (t if fault == "chan_ji" else t.transpose(0, 1, 3, 2)).reshape(n, P, rd * rd)


def _f64(level):
    a = level.numpy() if isinstance(level, torch.Tensor) else np.asarray(level)
    return a.astype(np.float64)


def lookup_ref(levels, coords, radius):
    """levels: planes [n,P,h_l,w_l] (any float dtype), coords fp32 [n,P,2] (x, y) -> (ref, mag, ssum) float64
    [n,P,len(levels) (2r+1)^2]"""
    ref, mag, ssum = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for l, lv in enumerate(levels):
            s, w = _corners(_f64(lv), *_level_coords(coords, l), radius)
            w = [t.astype(np.float64)[..., None, None] for t in w]
            ref.append(_channels(sum(a * b for a, b in zip(s, w))))
            mag.append(_channels(sum(np.abs(a) * b for a, b in zip(s, w))))
            ssum.append(_channels(sum(np.abs(a) for a in s)))
    return np.concatenate(ref, -1), np.concatenate(mag, -1), np.concatenate(ssum, -1)


def lookup_chain(levels, coords, radius, dtype, fault=None):
    """the contract's rounding sequence in `dtype` ("f16" / "f32" / "f64") -> numpy array of that dtype [n,P,L (2r+1)^2].
    `fault` builds one of the wrong lookups of FAULTS (tests/test_lookup_referee_cpu.py)."""
    dt = NP_DT[dtype]
    out = []
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for l, lv in enumerate(levels):
            tile_fault = fault if not (fault == "tile8_row_below" and l >= 2) else None
            s, w = _corners(_f64(lv), *_level_coords(coords, l, fault), radius, tile_fault)
            s = [a.astype(dt) for a in s]                                           # (exact: the planes hold dtype values)
            w = [t.astype(dt)[..., None, None] for t in w]
            if fault == "fp32_accum":
                acc = sum(a.astype(np.float32) * b.astype(np.float32) for a, b in zip(s, w)).astype(dt)
            else:
                acc = s[0] * w[0]
                for k in (1, 2, 3):
                    acc = acc + s[k] * w[k]
            assert acc.dtype == dt
            out.append(_channels(acc, fault))
    return np.concatenate(out, -1)


def hard_bound(ref, mag, ssum, dtype):
    if dtype == "f16":
        return (5.0 * 2.0 ** -11 * mag + 2.0 ** -25 * (ssum + 7.0)) * (1.0 + 2.0 ** -9)
    u, tiny = (2.0 ** -24, 2.0 ** -149) if dtype == "f32" else (2.0 ** -53, 2.0 ** -1074)
    return (4.0 * u * mag + 4.0 * tiny) * (1.0 + 2.0 ** -9)


def ratio(y, ref, mag, ssum, dtype):
    """|y - ref| / hard_bound where ref is finite (inf where y is not finite there; 0 where err = bound = 0); elsewhere
    NaN -- those elements are the bit equality's"""
    y = np.asarray(y).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(y - ref)
        b = hard_bound(ref, mag, ssum, dtype)
        q = np.where(err == 0.0, 0.0, err / b)
    q = np.where(np.isfinite(y), q, np.inf)
    return np.where(np.isfinite(ref) & np.isfinite(mag), q, np.nan)


def backward_ref(coords, grad, radius, h2, w2):
    """the adjoint of one level's lookup in float64: coords fp32 [n,P,2], grad [n,P,rd*rd] (channel rd i + j) ->
    (vol_grad, vol_grad of |grad|) [n,P,h2,w2]; a pixel with a non-finite coordinate contributes nothing"""
    n, P, _ = grad.shape
    rd = 2 * radius + 1
    M = rd + 4
    cx, cy = _level_coords(coords, 0)
    ok = np.isfinite(cx) & np.isfinite(cy)
    ones = np.ones((n, P, 1, 1))
    _, w = _corners(ones, np.where(ok, cx, np.float32(0)), np.where(ok, cy, np.float32(0)), radius)
    big = float(max(h2, w2) + 4 * M)
    ix = np.clip(np.floor(np.where(ok, cx, 0)).astype(np.float64), -big, big).astype(np.int64)
    iy = np.clip(np.floor(np.where(ok, cy, 0)).astype(np.float64), -big, big).astype(np.int64)
    g = np.asarray(grad, dtype=np.float64).reshape(n, P, rd, rd) * ok[..., None, None]              # [n,P,i,j]
    out = np.zeros((2, n, P, h2 + 2 * M, w2 + 2 * M))
    nn, pp = np.arange(n)[:, None, None, None], np.arange(P)[None, :, None, None]
    ii, jj = np.arange(rd)[None, None, :, None], np.arange(rd)[None, None, None, :]
    for (ox, oy), wk in zip(((0, 0), (0, 1), (1, 0), (1, 1)), w):
        X = np.clip(ix[..., None, None] + ii - radius + ox + M, 0, w2 + 2 * M - 1)
        Y = np.clip(iy[..., None, None] + jj - radius + oy + M, 0, h2 + 2 * M - 1)
        X, Y = np.broadcast_to(X, g.shape), np.broadcast_to(Y, g.shape)
        t = g * wk.astype(np.float64)[..., None, None]
        np.add.at(out[0], (nn, pp, Y, X), t)
        np.add.at(out[1], (nn, pp, Y, X), np.abs(t))
    return out[0][..., M:M + h2, M:M + w2], out[1][..., M:M + h2, M:M + w2]


def grid_sample_ref(levels, coords, radius):
    """the same taps by torch's own bilinear sampler in float64 (zeros padding, align_corners): a fully foreign check for
    cases with moderate coordinates"""
    rd = 2 * radius + 1
    out = []
    for l, lv in enumerate(levels):
        p = F.pad(torch.from_numpy(_f64(lv)), (0, 1, 0, 1))      # one more zero row and column: the same zero-padded
        n, P, hl, wl = p.shape                                   # plane, and no level is 1 wide (align_corners divides by w - 1)
        cx, cy = _level_coords(coords, l)
        ii, jj = torch.meshgrid(torch.arange(rd, dtype=torch.float64), torch.arange(rd, dtype=torch.float64), indexing="ij")
        # the position is rebuilt from the fp32 fraction the contract computes, floor(c) + (c - floor(c))_fp32: it differs
        # from c by at most 2^-25, and the sampler's float64 weights then differ from the fp32 products by roundings
        # that are RELATIVE to each weight (1 - dy computed from c itself is not, when dy is within 2^-10 of 1)
        px = np.floor(cx).astype(np.float64) + (cx - np.floor(cx)).astype(np.float64)
        py = np.floor(cy).astype(np.float64) + (cy - np.floor(cy)).astype(np.float64)
        gx = torch.from_numpy(px)[..., None, None] + ii - radius                             # [n,P,i,j]
        gy = torch.from_numpy(py)[..., None, None] + jj - radius
        grid = torch.stack([2.0 * gx / (wl - 1) - 1.0, 2.0 * gy / (hl - 1) - 1.0], -1)
        s = F.grid_sample(p.reshape(n * P, 1, hl, wl), grid.reshape(n * P, rd, rd, 2), mode="bilinear",
                          padding_mode="zeros", align_corners=True)
        out.append(s.reshape(n, P, rd * rd).numpy())
    return np.concatenate(out, -1)


# ------------------------------------------------------------------------------------------------------ tile8 layout

def tile8_pack(plane_batch, pad=0.0):
    """[..., hl, wl] -> [..., plane]: the inverse of droid_backends.corr_untile8 -- 8 x 8 tiles, element (y, x) at
    ((y >> 3) ntx + (x >> 3)) 64 + 8 (y & 7) + (x & 7); cells of partial tiles beyond the plane hold `pad`"""
    t = plane_batch if isinstance(plane_batch, torch.Tensor) else torch.from_numpy(np.asarray(plane_batch))
    hl, wl = t.shape[-2:]
    nty, ntx = (hl + 7) // 8, (wl + 7) // 8
    full = torch.full(tuple(t.shape[:-2]) + (nty * 8, ntx * 8), pad, dtype=t.dtype)
    full[..., :hl, :wl] = t
    lead = tuple(t.shape[:-2])
    k = len(lead)
    full = full.reshape(lead + (nty, 8, ntx, 8)).permute(*range(k), k, k + 2, k + 1, k + 3)
    return full.reshape(lead + (nty * ntx * 64,)).contiguous()


# ------------------------------------------------------------------------------------------------------ seeded cases

TARGETS = [(16, 32), (24, 48), (12, 16), (15, 20), (8, 12)]
SOURCES = [(5, 7), (9, 8)]
REGIMES = ["plain", "cancelling", "extreme"]
NOISE = (0.5, 4.0, 40.0)                         # one per edge
SLOTS, CAPACITY = [4, 0, 2], 5
CASES = [f"{h}x{w}-{r}" for h, w in TARGETS for r in REGIMES]
INF_PIXEL, NAN_PIXEL = (0, 5), (0, 6)            # (edge, pixel) whose planes hold the one inf / NaN cell per level
SPECIAL_EDGE = 1


def special_coords(h2, w2):
    """the fixed pixels of edge 1: (x, y) pairs"""
    mx, my = 0.5 * w2 + 0.3, 0.5 * h2 - 0.2
    out = [(3.0, 2.0), (float(w2 - 1), float(h2 - 1)), (2.5, 4.0), (5.0, 1.5), (3.5, 2.5)]
    for vx, vy in zip((-0.25, w2 - 1.5, -3.0, -4.0, w2 + 3.0, w2 + 4.0), (-0.25, h2 - 1.5, -3.0, -4.0, h2 + 3.0, h2 + 4.0)):
        out += [(vx, my), (mx, vy)]                                    # windows that just touch / just leave each border
    for k, v in enumerate((1e6, -1e6, 1e6 + 0.5, -(1e6 + 0.5), 1e9, -3e38)):
        out.append((v, my) if k % 2 == 0 else (mx, v))
        out.append((mx, v) if k % 2 == 0 else (v, my))
    out += [(1e-40, my), (mx, -1e-40), (-1e-40, 1e-40)]
    return out


_CACHE = {}


def case(name):
    """-> dict: h2, w2, h1, w1, n = 3, levels: four np.float16 arrays [3,P,h2 >> l,w2 >> l] (fp16 values: the fp32 and
    fp64 runs read the same numbers), coords np.float32 [3,P,2].  Edge e carries the identity grid scaled to the target
    map plus NOISE[e] pixels of noise; edge 1's first pixels carry special_coords; in the cancelling regime edge 0's x is
    moved to a half-integer + 1e-3 randn, where a +-c checkerboard blends to ~2e-3 of its magnitude."""
    if name in _CACHE:
        return _CACHE[name]
    size, regime = name.split("-")
    h2, w2 = map(int, size.split("x"))
    k = CASES.index(name)
    h1, w1 = SOURCES[(k // 3 + k % 3) % 2]
    n, P = 3, h1 * w1
    rng = np.random.default_rng(4200 + k)
    ys, xs = np.meshgrid(np.arange(h1), np.arange(w1), indexing="ij")
    base = np.stack([xs.reshape(-1) * (w2 - 1) / (w1 - 1), ys.reshape(-1) * (h2 - 1) / (h1 - 1)], -1)      # [P,2]
    coords = np.stack([base + NOISE[e] * rng.standard_normal((P, 2)) for e in range(n)])
    if regime == "cancelling":
        coords[0, :, 0] = np.floor(coords[0, :, 0]) + 0.5 + 1e-3 * rng.standard_normal(P)
    sp = special_coords(h2, w2)
    assert len(sp) <= P
    coords[SPECIAL_EDGE, :len(sp)] = np.array(sp)
    with np.errstate(over="ignore"):
        coords = coords.astype(np.float32)
    assert np.isfinite(coords).all()
    levels = []
    for l in range(4):
        hl, wl = h2 >> l, w2 >> l
        if regime == "plain":
            v = rng.standard_normal((n, P, hl, wl))
        elif regime == "cancelling":
            yy, xx = np.meshgrid(np.arange(hl), np.arange(wl), indexing="ij")
            v = np.where((xx + yy) % 2 == 0, 1.0, -1.0) * 100.0 * (1.0 + 2.0 ** -10 * rng.standard_normal((n, P, hl, wl)))
        else:
            kind = rng.integers(0, 4, (n, P, hl, wl))
            v = rng.standard_normal((n, P, hl, wl))
            v = np.where(kind == 1, np.where(v < 0, -65504.0, 65504.0), v)
            v = np.where(kind == 2, np.sign(v) * rng.integers(1, 1024, v.shape) * 2.0 ** -24, v)
            for (e, p), bad in ((INF_PIXEL, np.inf), (NAN_PIXEL, np.nan)):
                cx, cy = coords[e, p] / np.float32(1 << l)
                v[e, p, int(np.clip(np.floor(cy), 0, hl - 1)), int(np.clip(np.floor(cx), 0, wl - 1))] = bad
        levels.append(v.astype(np.float16))
    _CACHE[name] = {"name": name, "regime": regime, "h2": h2, "w2": w2, "h1": h1, "w1": w1, "n": n, "levels": levels,
                    "coords": coords}
    return _CACHE[name]


def moderate(c):
    """the pixels inside the grid_sample check's domain [n,P]: coordinates within 1e3 of the map and not the +-1e-40 ones,
    whose weights the grid normalisation (an absolute 2^-53 of the plane's width) swallows"""
    a = np.abs(c["coords"])
    return ((a < 1e3) & ((a == 0) | (a > 1e-30))).all(-1)
