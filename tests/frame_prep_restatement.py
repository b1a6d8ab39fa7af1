"""The frame preprocessing of the reference's datasets (src/datasets.py) restated in numpy: the specification that
csrc/frame_prep.hip is tested against bit for bit.

The reference calls OpenCV for it:
  * `cv2.initUndistortRectifyMap(K, D, R, P, size, CV_32F)` (EuRoC's rectification) and `cv2.undistort(img, K, D)` (the
    `cfg['cam']['distortion']` path, the same map with R = I and P = K);
  * `cv2.remap(img, map_x, map_y, INTER_LINEAR)`: BORDER_CONSTANT with value 0, float maps rounded to 1/32 pixel, the
    32 x 32 table of 15-bit bilinear weights, (sum + 2^14) >> 15;
  * `cv2.resize(img, (W, H))`, INTER_LINEAR on 8-bit data: source coordinate (d + 0.5) * src/dst - 0.5 in double,
    rounded to float, clamped to the frame; 11-bit weights rounded per tap from the float fraction; the horizontal pass
    in integers; the vertical pass with the vector path's 8-bit rounding (each row >> 4, times the weight, the high
    16 bits kept, the two summed, (s + 2) >> 2).  An exact 2x downscale in both directions is INTER_AREA:
    (a + b + c + d + 2) >> 2.
Depth follows numpy and torch: `uint16.astype(float32) / float32(scale)`, then F.interpolate(mode='nearest'),
src = min(floor(dst * float32(in / out)), in - 1).

cv2 is not installed where this project is built and tested, so byte equality of this restatement with a real cv2
build has never been measured.  Known places where a real build may differ by one level: the scalar tail of OpenCV's
vertical pass (the last few bytes of a row, how many depends on the CPU's vector width) rounds exactly,
(S0 * b0 + S1 * b1 + 2^21) >> 22, where this restatement applies the vector rounding to every byte; OpenCV's
vectorised map computation (AVX2) and its LU inverse may round the float64 map differently from the scalar formula
restated here; `cv2.undistort` rounds its float64 coordinates to fixed point directly where this restatement goes
through float32 maps.  The tests pin this restatement, not cv2.
"""
import numpy as np

RESIZE_BITS = 11
RESIZE_ONE = 1 << RESIZE_BITS          # INTER_RESIZE_COEF_SCALE
REMAP_BITS = 15                        # INTER_REMAP_COEF_BITS
TAB = 32                               # INTER_TAB_SIZE


def _round_even(x):
    """cvRound: round half to even (lrint in the default mode)."""
    return np.rint(x)


def _linear_taps(n_src, n_dst):
    """Per destination index of one axis: (first source index, weight 0, weight 1, the unclamped source index) as
    cv::resize's table setup makes them.  The horizontal clamp (first index 0 / last index, fraction 0) is applied by
    the caller; the vertical table is not clamped (its rows are clipped when they are read)."""
    scale = 1.0 / (float(n_dst) / float(n_src))                 # scale_x = 1 / inv_scale_x, in double
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)             # (float)((dx + 0.5) * scale_x - 0.5)
    s = np.floor(f).astype(np.int64)                             # cvFloor
    f = (f - s.astype(np.float32)).astype(np.float32)            # fx -= sx (float)
    return s, f


def _weights(f):
    one = np.float32(1.0)
    w0 = _round_even((one - f).astype(np.float32) * np.float32(RESIZE_ONE)).astype(np.int64)
    w1 = _round_even(f * np.float32(RESIZE_ONE)).astype(np.int64)
    return w0, w1


def is_area_2x(h, w, h_dst, w_dst):
    """cv::resize switches INTER_LINEAR to INTER_AREA when both scales are exactly 2."""
    return h == 2 * h_dst and w == 2 * w_dst


def resize_u8(img, h_dst, w_dst):
    """cv2.resize(img, (w_dst, h_dst)) with INTER_LINEAR on uint8 [h, w] or [h, w, c]."""
    img = np.asarray(img, dtype=np.uint8)
    squeeze = img.ndim == 2
    src = img[:, :, None] if squeeze else img
    h, w, _ = src.shape
    if (h, w) == (h_dst, w_dst):
        out = src.copy()
    elif is_area_2x(h, w, h_dst, w_dst):
        s = src.astype(np.int64)
        out = ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    else:
        sx, fx = _linear_taps(w, w_dst)
        lo = sx < 0
        fx = np.where(lo, np.float32(0.0), fx)
        sx = np.where(lo, 0, sx)
        hi = sx >= w - 1
        fx = np.where(hi, np.float32(0.0), fx)
        sx = np.where(hi, w - 1, sx)
        a0, a1 = _weights(fx)
        sx1 = np.minimum(sx + 1, w - 1)                          # read only where a1 == 0 at the clamp
        s = src.astype(np.int64)
        hrow = s[:, sx] * a0[None, :, None] + s[:, sx1] * a1[None, :, None]    # [h, w_dst, c], int

        sy, fy = _linear_taps(h, h_dst)
        b0, b1 = _weights(fy)
        r0 = np.clip(sy, 0, h - 1)
        r1 = np.clip(sy + 1, 0, h - 1)
        out = vresize_u8(hrow[r0], hrow[r1], b0[:, None, None], b1[:, None, None])
    return out[:, :, 0] if squeeze else out


def vresize_u8(S0, S1, b0, b1):
    """VResizeLinearVec_32s8u: pack(S >> 4) to int16 (saturating), mul_hi by the int16 weight, saturating int16 add,
    (s + 2) >> 2 packed to uint8 (saturating)."""
    def mul_hi(S, b):
        v = np.clip(S >> 4, -32768, 32767)
        return (v * b) >> 16
    s = np.clip(mul_hi(S0, b0) + mul_hi(S1, b1), -32768, 32767)
    return np.clip((s + 2) >> 2, 0, 255).astype(np.uint8)


def remap_u8(img, map_x, map_y):
    """cv2.remap(img, map_x, map_y, INTER_LINEAR) with float32 maps [mh, mw], BORDER_CONSTANT 0."""
    img = np.asarray(img, dtype=np.uint8)
    squeeze = img.ndim == 2
    src = (img[:, :, None] if squeeze else img).astype(np.int64)
    h, w, c = src.shape
    mx = np.asarray(map_x, dtype=np.float32)
    my = np.asarray(map_y, dtype=np.float32)
    # cvRound(v * INTER_TAB_SIZE): the product is exact in float32; out-of-int range is clipped (far outside anyway)
    ix = np.clip(_round_even(mx.astype(np.float64) * TAB), -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    iy = np.clip(_round_even(my.astype(np.float64) * TAB), -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    tx, ty = ix & (TAB - 1), iy & (TAB - 1)
    sx = np.clip(ix >> 5, -32768, 32767)                         # saturate_cast<short>(sx >> INTER_BITS)
    sy = np.clip(iy >> 5, -32768, 32767)
    # BilinearTab_i: the float products are exact multiples of 2^-10 and already sum to 2^15
    w00 = (TAB - ty) * (TAB - tx) * 32
    w01 = (TAB - ty) * tx * 32
    w10 = ty * (TAB - tx) * 32
    w11 = ty * tx * 32

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        v = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(ok[..., None], v, 0)
    acc = (tap(sy, sx) * w00[..., None] + tap(sy, sx + 1) * w01[..., None]
           + tap(sy + 1, sx) * w10[..., None] + tap(sy + 1, sx + 1) * w11[..., None])
    out = np.clip((acc + (1 << (REMAP_BITS - 1))) >> REMAP_BITS, 0, 255).astype(np.uint8)
    return out[:, :, 0] if squeeze else out


def nearest_index(n_in, n_out):
    """torch's nearest source index (UpSample.h nearest_idx): min(floor(d * float(in / out)), in - 1), float32."""
    scale = np.float32(np.float32(n_in) / np.float32(n_out))
    d = np.arange(n_out, dtype=np.float32)
    return np.minimum(np.floor(d * scale).astype(np.int64), n_in - 1)


def depth_resize(depth_u16, scale, h_dst, w_dst):
    """F.interpolate(torch.from_numpy(d.astype(float32) / scale)[None, None], (h_dst, w_dst), mode='nearest')[0, 0]."""
    d = np.asarray(depth_u16).astype(np.float32) / np.float32(scale)
    return d[nearest_index(d.shape[0], h_dst)][:, nearest_index(d.shape[1], w_dst)]


def init_undistort_rectify_map(K, D, R, P, size):
    """cv2.initUndistortRectifyMap(K, D, R, P, (w, h), CV_32F) -> (map_x, map_y) float32 [h, w]: the scalar loop of
    OpenCV's computer in float64 (the running sums _x += ir[0] along a row included), D = k1 k2 p1 p2 [k3]."""
    w, h = size
    K = np.asarray(K, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)[:3, :3]
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    D = np.zeros(5) if D is None else np.asarray(D, dtype=np.float64).reshape(-1)
    k1, k2, p1, p2 = D[:4]
    k3 = D[4] if D.size >= 5 else 0.0
    ir = np.linalg.inv(P @ R).reshape(-1)
    u0, v0, fx, fy = K[0, 2], K[1, 2], K[0, 0], K[1, 1]
    i = np.arange(h, dtype=np.float64)
    _x = i * ir[1] + ir[2]
    _y = i * ir[4] + ir[5]
    _w = i * ir[7] + ir[8]
    map_x = np.empty((h, w), dtype=np.float32)
    map_y = np.empty((h, w), dtype=np.float32)
    for j in range(w):
        ww = 1.0 / _w
        x = _x * ww
        y = _y * ww
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        _2xy = 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((0.0 * r2 + 0.0) * r2 + 0.0) * r2)
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + 0.0 * r2 + 0.0 * r2 * r2
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + 0.0 * r2 + 0.0 * r2 * r2
        map_x[:, j] = (fx * xd + u0).astype(np.float32)
        map_y[:, j] = (fy * yd + v0).astype(np.float32)
        _x = _x + ir[0]
        _y = _y + ir[3]
        _w = _w + ir[6]
    return map_x, map_y


def undistort_maps(K, D, size):
    """The maps of cv2.undistort(img, K, D): R = I, P = K."""
    return init_undistort_rectify_map(K, D, np.eye(3), K, size)


def color_item(bgr, H_out, W_out, H_edge, W_edge, maps=None):
    """The colour half of BaseDataset.__getitem__ / EuRoC.__getitem__ for one view: uint8 [h, w, 3] (BGR, cv2.imread's
    order) or [h, w] grey -> float32 [3, H_out, W_out] RGB in [0, 1]."""
    img = np.asarray(bgr, dtype=np.uint8)
    if maps is not None:
        img = remap_u8(img, maps[0], maps[1])
    img = resize_u8(img, H_out + 2 * H_edge, W_out + 2 * W_edge)
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    rgb = img[:, :, ::-1].transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(rgb[:, H_edge:H_edge + H_out, W_edge:W_edge + W_out])


def depth_item(depth_u16, scale, H_out, W_out, H_edge, W_edge):
    d = depth_resize(depth_u16, scale, H_out + 2 * H_edge, W_out + 2 * W_edge)
    return np.ascontiguousarray(d[H_edge:H_edge + H_out, W_edge:W_edge + W_out])
