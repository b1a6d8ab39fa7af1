"""Track the robot on the map as it drives: Monte Carlo localisation on a 2-D occupancy map
(csrc/mcl.hip; include/goslam_hip.h, gs_mcl_*; tests/mcl_restatement.py).

The map is the dict `scan.py` takes, read the same way (254 free, 205 unknown, anything else occupied).  A particle is a
row (x, y, h) of an int32 [N,3] tensor: x, y in milli-cells with 0 <= x < 1000 n_u, 0 <= y < 1000 n_v (the cell is
x // 1000, a cell's centre is at 500), h a heading index in [0, H) for the yaw 2 pi h / H -- yaw 0 along +u, positive
toward +v, as in `scan.py`.  A metric position is origin + x / 1000 * resolution.

`move` (gs_mcl_move) applies an odometry step and per-particle noise, `weigh` (gs_mcl_weigh) sums the likelihood field of
`scan.field` at the end points of a scan's beams, `estimate` (gs_mcl_estimate) turns the sums into weights, their prefix
sums and sixteen words of statistics, `resample` (gs_mcl_resample) draws the next generation systematically.  The kernels
are integer and equal the serial restatement bit for bit; the tables (`heading_table`, `beam_ends`, `weight_table`) are
made on the host in float64 by functions the restatement's callers use too.  `ParticleFilter` keeps the field, the tables
and two particle buffers on the device and reads sixteen words per tick; `track_on_map` drives it along a list of poses
with simulated scans and drifting odometry; `mcl_text` / `parse_mcl` are a run's map/mcl.txt (`mcl_config`).
"""
import math
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from . import plan as _plan
from . import scan as _scan

MAX_PARTICLES = 65536                  # GS_MCL_MAX_PARTICLES
MAX_HEADINGS = 1024
MAX_BEAMS = _scan.MAX_BEAMS
MAX_LUT = 65536
MAX_STEP = 1 << 20                     # |df|, |dl|, |dh|, |noise|
MAX_END = 4000000                      # an end point further than this from the robot (milli-cells) counts as outside
MAX_W = 1 << 36
ROT_ONE = 1 << 14
WEIGHT_ONE = 1 << 20
N_STATS = 16                           # GS_MCL_STATS
NO_SCORE = -1                          # the u32 word 0xffffffff read as int32
NO_BEST = 0xffffffffffffffff
_MASK64 = (1 << 64) - 1

_int, _flag, _number = _scan._int, _scan._flag, _scan._number


# ---- the tables (host, float64) ------------------------------------------------------------------------------------------
def heading_table(n_headings):
    """int32 [H,2] (numpy): rint(2^14 (cos, sin)(2 pi k / H)), k = 0 .. H - 1, 1 <= H <= 1024."""
    H = _int(n_headings, 1, MAX_HEADINGS, "n_headings", "heading_table")
    t = 2.0 * math.pi * np.arange(H, dtype=np.float64) / H
    return np.rint(ROT_ONE * np.stack([np.cos(t), np.sin(t)], axis=-1)).astype(np.int32)


def beam_ends(ranges_m, angles, n_headings, resolution, min_range=0.0, max_range=math.inf):
    """int32 [H,B',2] (numpy): per heading k the end point of every valid beam (`scan.valid_beams`) in milli-cells from the
    robot, rint(1000 * r / resolution * cos(angle + 2 pi k / H)) and likewise with sin, in numpy float64:
    `scan.beam_offsets` at a thousand times the resolution.  B' may be 0.  A component beyond 32 bits is clamped there
    (the kernel counts anything beyond 4 000 000 as outside the map)."""
    what = "beam_ends"
    a = _scan._angles(angles, what)
    r = _scan._ranges(ranges_m, a.shape[0], what)
    H = _int(n_headings, 1, MAX_HEADINGS, "n_headings", what)
    res = _number(resolution, "resolution", what, positive=True)
    lo, hi = _scan._range_limits(min_range, max_range, what)
    keep = _scan.valid_beams(r, lo, hi)
    r, a = r[keep], a[keep]
    t = (2.0 * math.pi * np.arange(H, dtype=np.float64) / H)[:, None] + a[None, :]
    reach = 1000.0 * r[None, :] / res
    ends = np.stack([np.rint(reach * np.cos(t)), np.rint(reach * np.sin(t))], axis=-1)
    return np.clip(ends, -0x7fffffff, 0x7fffffff).astype(np.int32)


def weight_table(n_beams, sigma_cells=2.0, squash=None):
    """uint32 [L] (numpy): lut[d] = floor(2^20 exp(-d * squash / (2 sigma_cells^2))) for d a difference of two sums of the
    likelihood field (squared cells), cut before its first zero and at L <= 65536.  squash defaults to min(1, 30 /
    n_beams): at most thirty beams count as independent measurements.  Built once per filter from the scanner's beam
    count."""
    what = "weight_table"
    n = _int(n_beams, 1, MAX_BEAMS, "n_beams", what)
    sigma = _number(sigma_cells, "sigma_cells", what, positive=True)
    squash = min(1.0, 30.0 / n) if squash is None else _number(squash, "squash", what, positive=True)
    if not (math.isfinite(sigma) and math.isfinite(squash)):
        raise ValueError(f"{what}: sigma_cells and squash must be finite (got {sigma}, {squash})")
    lut = np.floor(WEIGHT_ONE * np.exp(-np.arange(MAX_LUT, dtype=np.float64) * squash / (2.0 * sigma * sigma)))
    zero = np.nonzero(lut == 0)[0]
    return lut[:int(zero[0]) if zero.size else MAX_LUT].astype(np.uint32)


# ---- the four kernels ---------------------------------------------------------------------------------------------------
def _flat(a, name, what, dev, size=None, wide=False):
    """`a` (a tensor or an array of integers [n]) as a contiguous int32 (wide: int64) tensor on `dev`."""
    dtype = torch.int64 if wide else torch.int32
    if not isinstance(a, torch.Tensor):
        arr = np.asarray(a)
        if arr.dtype.kind not in "ui":
            raise ValueError(f"{what}: {name} must be integers (got {arr.dtype})")
        if arr.dtype == np.uint32 and not wide:
            arr = arr.view(np.int32)                                    # the u32 words as the kernel sees them
        elif arr.dtype == np.uint64:
            arr = arr.view(np.int64)
        a = torch.from_numpy(np.array(arr, order="C"))
    if a.is_floating_point() or a.dtype == torch.bool or a.dim() != 1 or (size is not None and a.shape[0] != size):
        raise ValueError(f"{what}: {name} must be integers [{'n' if size is None else size}] "
                         f"(got {a.dtype} {list(a.shape)})")
    return a.to(device=dev, dtype=dtype).contiguous()


def _particles(particles, what, name="particles"):
    if not isinstance(particles, torch.Tensor) or particles.dtype != torch.int32 or particles.dim() != 2 \
            or particles.shape[1] != 3 or particles.shape[0] > MAX_PARTICLES or not particles.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous int32 tensor [N,3] with N <= {MAX_PARTICLES} "
                         f"(got {getattr(particles, 'dtype', type(particles).__name__)} "
                         f"{list(getattr(particles, 'shape', []))})")
    return particles


def _table(rot, what, dev):
    rot = _scan._rows(rot, "rot", "[H,2]", 2, what, dev)
    if rot.dim() != 2 or not 1 <= rot.shape[0] <= MAX_HEADINGS:
        raise ValueError(f"{what}: rot must be [H,2] with 1 <= H <= {MAX_HEADINGS} (got {list(rot.shape)})")
    return rot


def _dims(a, name, what, ok, want):
    """The shape of a tensor or an array, checked by `ok` before anything moves to a device."""
    shape = tuple(int(n) for n in (a.shape if isinstance(a, torch.Tensor) else np.asarray(a).shape))
    if not ok(shape):
        raise ValueError(f"{what}: {name} must be {want} (got {list(shape)})")
    return shape


def _shares_memory(a, b):
    lo_a, lo_b = a.data_ptr(), b.data_ptr()
    return lo_a < lo_b + b.numel() * b.element_size() and lo_b < lo_a + a.numel() * a.element_size()


@torch.no_grad()
def move(particles, rot, noise, odometry, shape, out=None):
    """gs_mcl_move: particles int32 [N,3] on a GPU, rot integers [H,2] (`heading_table`), noise integers [N,3], odometry
    (df, dl, dh) -- forward and left in milli-cells and heading steps, each within 2^20 in size, as the noise must be --,
    shape (n_u, n_v) of the map.  -> int32 [N,3]: x' = clamp(x + ((f c - l s + 8192) >> 14), 0, 1000 n_u - 1) with f = df +
    noise 0, l = dl + noise 1, (c, s) = rot[h], y' likewise with f s + l c, h' = (h + dh + noise 2) mod H.  `out` may be
    `particles` itself (in place); any other overlap is refused.  Enqueues on the current stream and reads nothing back.
    ValueError before the device is touched."""
    what = "mcl.move"
    _particles(particles, what)
    try:
        df, dl, dh = odometry
        n_u, n_v = shape
    except (TypeError, ValueError):
        raise ValueError(f"{what}: odometry is (df, dl, dh) and shape (n_u, n_v) (got {odometry!r}, {shape!r})") from None
    df, dl, dh = (_int(v, -MAX_STEP, MAX_STEP, f"odometry {k}", what) for v, k in zip((df, dl, dh), ("df", "dl", "dh")))
    n_u, n_v = _int(n_u, 1, _scan.MAX_CELLS, "n_u", what), _int(n_v, 1, _scan.MAX_CELLS, "n_v", what)
    N = int(particles.shape[0])
    _dims(rot, "rot", what, lambda d: len(d) == 2 and d[1] == 2 and 1 <= d[0] <= MAX_HEADINGS, f"[H,2] with 1 <= H <= {MAX_HEADINGS}")
    _dims(noise, "noise", what, lambda d: d == (N, 3), f"[{N},3]")
    _scan._on_gpu(particles, "particles", what)
    dev = particles.device
    rot = _table(rot, what, dev)
    noise = _scan._rows(noise, "noise", "[N,3]", 3, what, dev)
    if tuple(noise.shape) != (N, 3):
        raise ValueError(f"{what}: noise must be [{N},3] (got {list(noise.shape)})")
    if out is None:
        out = torch.empty_like(particles)
    elif out is not particles:
        _particles(out, what, "out")
        if tuple(out.shape) != (N, 3) or out.device != dev or (out.data_ptr() != particles.data_ptr() and _shares_memory(out, particles)):
            raise ValueError(f"{what}: out must be [{N},3] on {dev}, the particles themselves or apart from them")
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_mcl_move(_lib.ptr(particles), N, _lib.ptr(rot), int(rot.shape[0]), _lib.ptr(noise), df, dl, dh,
                                    n_u, n_v, _lib.ptr(out), _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return out


@torch.no_grad()
def weigh(cost, cells, particles, ends, cap, allow_unknown=False, out=None):
    """gs_mcl_weigh: cost (of `scan.field`) and cells uint8 [n_u,n_v], particles int32 [N,3], ends integers [H,B,2]
    (`beam_ends`), cap the cost of an end point outside the map.  -> (S int32 [N], the kernel's u32 words: -1 (0xffffffff)
    where the particle's cell is not free -- with `allow_unknown` an unknown cell counts as free --, else the sum over the
    beams of the field at floor((x + ex) / 1000), floor((y + ey) / 1000); best int64 [1], the kernel's u64 word: the
    smallest (S << 32) | p over the standing particles, -1 (all ones) without one) on the map's device; `out` = (S, best).
    Enqueues on the current stream and reads nothing back.  ValueError before the device is touched."""
    what = "mcl.weigh"
    _scan._map_tensor(cost, "cost", what)
    _scan._map_tensor(cells, "cells", what, tuple(cost.shape))
    _particles(particles, what)
    cap = _int(cap, 1, _scan.R_MAX * _scan.R_MAX + 1, "cap", what)
    allow_unknown = _flag(allow_unknown, "allow_unknown", what)
    _dims(ends, "ends", what, lambda d: len(d) == 3 and d[2] == 2 and 1 <= d[0] <= MAX_HEADINGS and 1 <= d[1] <= MAX_BEAMS,
          f"[H,B,2] with 1 <= H <= {MAX_HEADINGS} and 1 <= B <= {MAX_BEAMS}")
    _scan._on_gpu(cost, "cost", what)
    dev = cost.device
    if cells.device != dev or particles.device != dev:
        raise ValueError(f"{what}: cells and particles must be on {dev} like cost")
    ends = _scan._rows(ends, "ends", "[H,B,2]", 2, what, dev)
    if ends.dim() != 3 or not (1 <= ends.shape[0] <= MAX_HEADINGS and 1 <= ends.shape[1] <= MAX_BEAMS):
        raise ValueError(f"{what}: ends must be [H,B,2] with 1 <= H <= {MAX_HEADINGS} and 1 <= B <= {MAX_BEAMS} "
                         f"(got {list(ends.shape)})")
    N = int(particles.shape[0])
    S, best = _scan._out(out, (("S", torch.int32, (N,)), ("best", torch.int64, (1,))), dev, what)
    cost, cells = cost.contiguous(), cells.contiguous()
    n_u, n_v = (int(n) for n in cost.shape)
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_mcl_weigh(_lib.ptr(cost), _lib.ptr(cells), n_u, n_v, _lib.ptr(particles), N, _lib.ptr(ends),
                                     int(ends.shape[0]), int(ends.shape[1]), cap, int(allow_unknown), _lib.ptr(S),
                                     _lib.ptr(best), _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return S, best


@torch.no_grad()
def estimate(S, particles, rot, lut, out=None):
    """gs_mcl_estimate: S int32 [N] (of `weigh`), particles int32 [N,3] with N >= 1, rot integers [H,2], lut integers [L]
    (`weight_table`).  -> (w int32 [N] = lut[S - S_min] where the particle stands and S - S_min < L, else 0; cum int64 [N],
    the inclusive prefix sums of w; stats int64 [16], the kernel's u64 words (`moments` reads them): W, sum w^2, the
    particles standing, those with w > 0, best, sum w x, sum w y, sum w c, sum w s, then sum w (v >> 20) and sum w (v &
    0xfffff) for v = x^2, y^2 and x y, and a zero) on the particles' device; `out` = (w, cum, stats).  Enqueues on the
    current stream and reads nothing back.  ValueError before the device is touched."""
    what = "mcl.estimate"
    _particles(particles, what)
    N = int(particles.shape[0])
    if N < 1:
        raise ValueError(f"{what}: no particle")
    _dims(S, "S", what, lambda d: d == (N,), f"[{N}]")
    _dims(lut, "lut", what, lambda d: len(d) == 1 and 1 <= d[0] <= MAX_LUT, f"[L] with 1 <= L <= {MAX_LUT}")
    _dims(rot, "rot", what, lambda d: len(d) == 2 and d[1] == 2 and 1 <= d[0] <= MAX_HEADINGS, f"[H,2] with 1 <= H <= {MAX_HEADINGS}")
    _scan._on_gpu(particles, "particles", what)
    dev = particles.device
    S = _flat(S, "S", what, dev, N)
    lut = _flat(lut, "lut", what, dev)
    if not 1 <= lut.shape[0] <= MAX_LUT:
        raise ValueError(f"{what}: lut must have 1 to {MAX_LUT} entries (got {lut.shape[0]})")
    rot = _table(rot, what, dev)
    w, cum, stats = _scan._out(out, (("w", torch.int32, (N,)), ("cum", torch.int64, (N,)),
                                     ("stats", torch.int64, (N_STATS,))), dev, what)
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_mcl_estimate(_lib.ptr(S), _lib.ptr(particles), N, _lib.ptr(rot), int(rot.shape[0]),
                                        _lib.ptr(lut), int(lut.shape[0]), _lib.ptr(w), _lib.ptr(cum), _lib.ptr(stats),
                                        _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return w, cum, stats


@torch.no_grad()
def resample(cum, particles, W, q, out=None):
    """gs_mcl_resample: cum int64 [N] (of `estimate`) with W = cum[-1] in [1, 2^36] and 0 <= q < W, Python integers the host
    has read; particles int32 [N,3].  -> int32 [N,3], new particle j the old particle i with the smallest i such that
    cum[i] * N > j * W + q (systematic resampling).  `out` must share no memory with `particles`.  Enqueues on the current
    stream and reads nothing back.  ValueError before the device is touched."""
    what = "mcl.resample"
    _particles(particles, what)
    W = _int(W, 1, MAX_W, "W", what)
    q = _int(q, 0, W - 1, "q", what)
    N = int(particles.shape[0])
    _dims(cum, "cum", what, lambda d: d == (N,), f"[{N}]")
    _scan._on_gpu(particles, "particles", what)
    dev = particles.device
    cum = _flat(cum, "cum", what, dev, N, wide=True)
    if out is None:
        out = torch.empty_like(particles)
    else:
        _particles(out, what, "out")
        if tuple(out.shape) != (N, 3) or out.device != dev or _shares_memory(out, particles):
            raise ValueError(f"{what}: out must be [{N},3] on {dev} and share no memory with particles")
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_mcl_resample(_lib.ptr(cum), _lib.ptr(particles), N, W, q, _lib.ptr(out), _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return out


# ---- the host side of a tick --------------------------------------------------------------------------------------------
def motion_noise(n_particles, sigmas, generator=None, device=None):
    """int32 [N,3]: per particle the noise of one `move`, normal with standard deviations `sigmas` = (forward, left in
    milli-cells, heading in steps), drawn in float32 by `generator` on its device, scaled, rounded to nearest, clamped to
    +-2^20 and moved to `device` (default: the generator's, the CPU without one)."""
    what = "mcl.motion_noise"
    N = _int(n_particles, 0, MAX_PARTICLES, "n_particles", what)
    try:
        sig = [_number(s, f"sigmas[{i}]", what) for i, s in enumerate(sigmas)]
    except TypeError:
        raise ValueError(f"{what}: sigmas is (forward, left, heading) (got {sigmas!r})") from None
    if len(sig) != 3 or not all(math.isfinite(s) for s in sig):
        raise ValueError(f"{what}: sigmas is three finite numbers (forward, left, heading) (got {sigmas!r})")
    src = generator.device if generator is not None else torch.device("cpu")
    nz = torch.randn((N, 3), dtype=torch.float32, device=src, generator=generator)
    nz = torch.round(nz * torch.tensor(sig, dtype=torch.float32, device=src)).clamp_(-MAX_STEP, MAX_STEP).to(torch.int32)
    return nz if device is None else nz.to(device)


def odometry_steps(d_forward_m, d_left_m, d_yaw, resolution, n_headings):
    """(df, dl, dh): an odometry increment in the robot's frame -- metres forward and to the left, radians of yaw -- as the
    integers of `move`: milli-cells rint(1000 d / resolution) and heading steps rint(d_yaw * H / 2 pi).  ValueError for a
    step beyond 2^20."""
    what = "odometry_steps"
    res = _number(resolution, "resolution", what, positive=True)
    H = _int(n_headings, 1, MAX_HEADINGS, "n_headings", what)
    vals = []
    for name, v in (("d_forward_m", d_forward_m), ("d_left_m", d_left_m), ("d_yaw", d_yaw)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError(f"{what}: {name} must be a finite number (got {v!r})")
        vals.append(float(v))
    steps = (round(1000.0 * vals[0] / res), round(1000.0 * vals[1] / res), round(vals[2] * H / (2.0 * math.pi)))
    if any(abs(s) > MAX_STEP for s in steps):
        raise ValueError(f"{what}: the step {steps} exceeds 2^20 milli-cells or heading steps")
    return steps


def moments(stats):
    """The exact sums behind the sixteen words of `estimate` (a sequence of integers, signed or not): {"W", "W2",
    "standing", "positive", "best", "x", "y", "c", "s", "xx", "yy", "xy"} in Python integers."""
    u = [int(v) & _MASK64 for v in stats]
    if len(u) != N_STATS:
        raise ValueError(f"mcl.moments: stats has {N_STATS} words (got {len(u)})")
    sign = lambda v: v - (1 << 64) if v >> 63 else v            # noqa: E731
    return {"W": u[0], "W2": u[1], "standing": u[2], "positive": u[3], "best": u[4], "x": u[5], "y": u[6],
            "c": sign(u[7]), "s": sign(u[8]), "xx": (u[9] << 20) + u[10], "yy": (u[11] << 20) + u[12],
            "xy": (u[13] << 20) + u[14]}


def pose_from_moments(m, origin, resolution, n_headings):
    """The weighted mean pose of `moments`' dict on a map: {"xy" metres, "milli": the mean (x, y) in milli-cells, "cell",
    "yaw" = atan2(sum w s, sum w c), "heading": the yaw in steps in [0, H), "cov": the 2 x 2 covariance in m^2 from the
    exact second moments, "yaw_concentration": |sum w (c, s)| / (2^14 W) in [0, 1], "ess": W^2 / sum w^2}; None when
    W == 0."""
    W = m["W"]
    if W == 0:
        return None
    mx, my = Fraction(m["x"], W), Fraction(m["y"], W)
    scale = (float(resolution) / 1000.0) ** 2
    cxx, cyy = Fraction(m["xx"], W) - mx * mx, Fraction(m["yy"], W) - my * my
    cxy = Fraction(m["xy"], W) - mx * my
    yaw = math.atan2(m["s"], m["c"])
    return {"xy": (origin[0] + float(mx) / 1000.0 * resolution, origin[1] + float(my) / 1000.0 * resolution),
            "milli": (float(mx), float(my)), "cell": (int(mx) // 1000, int(my) // 1000), "yaw": yaw,
            "heading": (yaw / (2.0 * math.pi) * n_headings) % n_headings,
            "cov": ((float(cxx) * scale, float(cxy) * scale), (float(cxy) * scale, float(cyy) * scale)),
            "yaw_concentration": math.hypot(m["c"], m["s"]) / (ROT_ONE * W), "ess": W * W / m["W2"]}


class ParticleFilter:
    """Monte Carlo localisation of a planar robot with a range scanner on the map `grid`.

    n_particles in [1, 65536]; headings H in [1, 1024]; n_beams the scanner's beam count (the weight table's squash);
    radius_cells the likelihood field's radius (`scan.field`); sigma_cells the scan model's standard deviation in cells;
    noise = (forward m, left m, yaw rad) the motion noise's standard deviations per tick and noise_rate their growth per
    metre moved (forward and left) and per radian turned (yaw): sigmas = noise + noise_rate * |motion|.  The defaults of
    noise, noise_rate, sigma_cells and lost_ticks are starting values that no measurement has tuned.  min_range /
    max_range drop beams as `scan.valid_beams` does.  The motion noise and the seeding come from a torch generator on the
    device seeded with `seed`; the resampling offset from Python's generator with the same seed.

    `seed_around` or `seed_free` places the particles; `step` (metres and radians) or `tick` (the integers of `move`) runs
    move, weigh and estimate, reads sixteen words, and resamples when the effective sample size falls below N / 2.
    `lost` turns true when no particle stands, or when the best particle's mean cost per beam has exceeded sigma_cells^2
    for `lost_ticks` ticks running; `recover` answers it with `scan.localize_on_map`."""

    def __init__(self, grid, n_particles=2048, headings=360, *, n_beams, radius_cells=6, sigma_cells=2.0,
                 noise=(0.01, 0.005, 0.01), noise_rate=(0.1, 0.05, 0.1), allow_unknown=False, seed=0, lost_ticks=3,
                 min_range=0.0, max_range=math.inf, device=None):
        what = "ParticleFilter"
        cells, self.origin, self.resolution, dev = _scan._grid(grid, what, device)
        self.N = _int(n_particles, 1, MAX_PARTICLES, "n_particles", what)
        self.H = _int(headings, 1, MAX_HEADINGS, "headings", what)
        self.R = _int(radius_cells, _scan.R_MIN, _scan.R_MAX, "radius_cells", what)
        self.sigma_cells = _number(sigma_cells, "sigma_cells", what, positive=True)
        lut = weight_table(n_beams, self.sigma_cells)
        self.noise = self._three(noise, "noise", what)
        self.noise_rate = self._three(noise_rate, "noise_rate", what)
        self.allow_unknown = _flag(allow_unknown, "allow_unknown", what)
        self.seed = _int(seed, 0, (1 << 63) - 1, "seed", what)
        self.lost_ticks = _int(lost_ticks, 1, 1 << 20, "lost_ticks", what)
        self.min_range, self.max_range = _scan._range_limits(min_range, max_range, what)
        if dev.type == "cuda" and dev.index is None:            # the generator and its tensors must name the same device
            dev = torch.device("cuda", torch.cuda.current_device())
        self.grid, self.device, self.shape = grid, dev, tuple(int(n) for n in cells.shape)
        self.cells = cells.to(dev).contiguous()
        self.cost = _scan.field(self.cells, self.R)
        self.rot = torch.from_numpy(heading_table(self.H)).to(dev)
        self.lut = torch.from_numpy(lut.view(np.int32).copy()).to(dev)
        self.particles = torch.zeros((self.N, 3), dtype=torch.int32, device=dev)
        self._spare = torch.empty_like(self.particles)
        self._out = (torch.empty(self.N, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int64, device=dev),
                     torch.empty(self.N, dtype=torch.int32, device=dev), torch.empty(self.N, dtype=torch.int64, device=dev),
                     torch.empty(N_STATS, dtype=torch.int64, device=dev))
        self.generator = torch.Generator(device=dev)
        self.generator.manual_seed(self.seed)
        import random
        self._draw = random.Random(self.seed)
        self.lost, self._bad_ticks, self.seeded = False, 0, False

    @staticmethod
    def _three(v, name, what):
        try:
            out = tuple(_number(a, f"{name}[{i}]", what) for i, a in enumerate(v))
        except TypeError:
            out = ()
        if len(out) != 3 or not all(math.isfinite(a) for a in out):
            raise ValueError(f"{what}: {name} is three finite numbers >= 0 (forward m, left m, yaw rad) (got {v!r})")
        return out

    def _milli(self, xy, what):
        try:
            x, y = (float(v) for v in xy)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: xy must be (x, y) in metres (got {xy!r})") from None
        if not (math.isfinite(x) and math.isfinite(y)):
            raise ValueError(f"{what}: xy must be finite (got {xy!r})")
        return ((x - self.origin[0]) / self.resolution * 1000.0, (y - self.origin[1]) / self.resolution * 1000.0)

    @torch.no_grad()
    def seed_around(self, xy, yaw, sigma_xy_m, sigma_yaw):
        """Every particle normal around the pose (xy metres, yaw radians) with standard deviations sigma_xy_m and sigma_yaw,
        rounded to milli-cells and heading steps, clamped to the map and wrapped.  Clears `lost`."""
        what = "ParticleFilter.seed_around"
        mx, my = self._milli(xy, what)
        yaw = float(_scan._yaws(yaw, what, "yaw").reshape(()))
        sx = _number(sigma_xy_m, "sigma_xy_m", what) / self.resolution * 1000.0
        sh = _number(sigma_yaw, "sigma_yaw", what) * self.H / (2.0 * math.pi)
        centre = torch.tensor([mx, my, yaw * self.H / (2.0 * math.pi)], dtype=torch.float64, device=self.device)
        spread = torch.tensor([sx, sx, sh], dtype=torch.float64, device=self.device)
        nz = torch.randn((self.N, 3), dtype=torch.float32, device=self.device, generator=self.generator).double()
        p = torch.round(centre + nz * spread)
        hi = torch.tensor([1000.0 * self.shape[0] - 1, 1000.0 * self.shape[1] - 1], dtype=torch.float64, device=self.device)
        p[:, :2] = torch.minimum(torch.clamp(p[:, :2], min=0.0), hi)
        p[:, 2] = torch.remainder(p[:, 2], float(self.H))
        self.particles.copy_(p.to(torch.int32))
        self.lost, self._bad_ticks, self.seeded = False, 0, True

    @torch.no_grad()
    def seed_free(self):
        """Every particle uniform over the cells a robot may stand on (free; with allow_unknown also unknown), within the
        cell, and over all headings.  ValueError when the map has no such cell.  Clears `lost`."""
        ok = self.cells == _scan.MAP_FREE
        if self.allow_unknown:
            ok = ok | (self.cells == _scan.MAP_UNKNOWN)
        at = torch.nonzero(ok)
        if at.shape[0] == 0:
            raise ValueError("ParticleFilter.seed_free: the map has no cell a robot may stand on")

        def draw(high):
            return torch.randint(0, high, (self.N,), device=self.device, generator=self.generator)
        cell = at[draw(int(at.shape[0]))]
        p = torch.stack([cell[:, 0] * 1000 + draw(1000), cell[:, 1] * 1000 + draw(1000), draw(self.H)], dim=1)
        self.particles.copy_(p.to(torch.int32))
        self.lost, self._bad_ticks, self.seeded = False, 0, True

    def step(self, odometry, ranges_m, angles):
        """One tick from an odometry increment (d_forward_m, d_left_m, d_yaw) in the robot's frame and the scan taken after
        it (ranges_m [B] metres at `angles` [B] radians): `tick` with `odometry_steps` and the sigmas noise + noise_rate *
        |motion| in the units of `move`."""
        what = "ParticleFilter.step"
        try:
            d_f, d_l, d_yaw = odometry
        except (TypeError, ValueError):
            raise ValueError(f"{what}: odometry is (d_forward_m, d_left_m, d_yaw) (got {odometry!r})") from None
        steps = odometry_steps(d_f, d_l, d_yaw, self.resolution, self.H)
        moved, turned = abs(float(d_f)) + abs(float(d_l)), abs(float(d_yaw))
        to_milli, to_steps = 1000.0 / self.resolution, self.H / (2.0 * math.pi)
        sigmas = ((self.noise[0] + self.noise_rate[0] * moved) * to_milli, (self.noise[1] + self.noise_rate[1] * moved) * to_milli,
                  (self.noise[2] + self.noise_rate[2] * turned) * to_steps)
        return self.tick(steps, ranges_m, angles, sigmas)

    @torch.no_grad()
    def tick(self, steps, ranges_m, angles, sigmas):
        """One tick in the integers of `move`: steps (df, dl, dh), the scan, and the noise's standard deviations `sigmas`
        (milli-cells, milli-cells, heading steps).  Computes `beam_ends`, launches move, weigh and estimate, reads the
        sixteen words once, and launches resample when 2 W^2 < N sum w^2.  -> {"found": a particle has weight, "xy"
        metres, "yaw", "cell", "cov" (2 x 2, m^2), "yaw_concentration", "ess", "milli", "heading" (`pose_from_moments`;
        None / 0 when nothing stands), "best_mean_cost": S_min / B', "n_standing", "n_beams": B', "resampled", "lost"}."""
        what = "ParticleFilter.tick"
        if not self.seeded:
            raise ValueError(f"{what}: seed the particles first (seed_around, seed_free or recover)")
        ends = beam_ends(ranges_m, angles, self.H, self.resolution, self.min_range, self.max_range)
        noise = motion_noise(self.N, sigmas, self.generator)
        move(self.particles, self.rot, noise, steps, self.shape, out=self.particles)
        B = int(ends.shape[1])
        res = {"found": False, "xy": None, "yaw": None, "cell": None, "cov": None, "yaw_concentration": 0.0, "ess": 0.0,
               "milli": None, "heading": None, "best_mean_cost": math.inf, "n_standing": 0, "n_beams": B, "resampled": False}
        if B > 0:
            S, best, w, cum, stats = self._out
            weigh(self.cost, self.cells, self.particles, torch.from_numpy(ends).to(self.device), self.R * self.R + 1,
                  self.allow_unknown, out=(S, best))
            estimate(S, self.particles, self.rot, self.lut, out=(w, cum, stats))
            m = moments(stats.cpu().tolist())                   # the one read
            res["n_standing"] = m["standing"]
            if m["W"] > 0:
                res.update(pose_from_moments(m, self.origin, self.resolution, self.H), found=True,
                           best_mean_cost=(m["best"] >> 32) / B)
                if 2 * m["W"] * m["W"] < self.N * m["W2"]:
                    q = (self._draw.getrandbits(32) * m["W"]) >> 32
                    resample(cum, self.particles, m["W"], q, out=self._spare)
                    self.particles, self._spare = self._spare, self.particles
                    res["resampled"] = True
        bad = not res["found"] or res["best_mean_cost"] > self.sigma_cells ** 2
        self._bad_ticks = self._bad_ticks + 1 if bad else 0
        self.lost = res["n_standing"] == 0 or self._bad_ticks >= self.lost_ticks
        res["lost"] = self.lost
        return res

    def recover(self, ranges_m, angles, around=None, sigma_xy_m=None, sigma_yaw=None):
        """The answer to `lost`: the exhaustive match `scan.localize_on_map` of the scan over the filter's headings
        (`around` as there) and, when it finds a pose, `seed_around` it with sigma_xy_m (default one cell) and sigma_yaw
        (default one heading step).  -> localize_on_map's dict."""
        res = _scan.localize_on_map(self.grid, ranges_m, angles, n_yaw=self.H, around=around, radius_cells=self.R,
                                    allow_unknown=self.allow_unknown, min_range=self.min_range, max_range=self.max_range,
                                    device=self.device)
        if res["found"]:
            self.seed_around(res["xy"], res["yaw"], self.resolution if sigma_xy_m is None else sigma_xy_m,
                             2.0 * math.pi / self.H if sigma_yaw is None else sigma_yaw)
        return res


# ---- the simulation loop and a run's map/mcl.txt ------------------------------------------------------------------------
MCL_ROW_ORDER = ("true_x", "true_y", "true_yaw", "est_x", "est_y", "est_yaw", "error_m", "yaw_error", "ess",
                 "best_mean_cost", "n_standing", "resampled", "lost", "relocalized")
_MCL_ROW_INTS = ("n_standing", "resampled", "lost", "relocalized")
MCL_SUMMARY_ORDER = ("particles", "headings", "ticks", "poses_skipped", "relocalized", "max_error_m")
_MCL_SUMMARY_FLOATS = ("max_error_m",)
_MCL_HEAD = "Monte Carlo localisation on the occupancy map"


def _wrap_angle(a):
    return (a + math.pi) % (2.0 * math.pi) - math.pi


@torch.no_grad()
def track_on_map(grid, poses, scanner, n_particles=2048, headings=360, drift=None, seed=0, sigma_xy_m=None,
                 sigma_yaw=None, **filter_args):
    """Drive a `ParticleFilter` along `poses` ([(xy, yaw) or None], `scan.planar_poses`) on the map `grid`: the poses that
    are None, outside the map or on a cell that is not free are skipped; the filter is seeded around the first of the
    others (sigma_xy_m, default two cells; sigma_yaw, default three heading steps); at each later one a scan is cast from
    the true pose (`scan.scan_on_map` with scanner = {"beams", "fov_deg", "max_range"}), the odometry is the motion from
    the previous pose in its frame, with drift = {"scale": factor on the distances, "yaw_deg_per_m": added turn per metre
    moved}, the filter steps, and when it reports `lost` it recovers by `ParticleFilter.recover` (counted).  -> {"rows":
    per tick the true and the estimated pose, error_m, yaw_error (radians), ess, best_mean_cost, n_standing, resampled,
    lost, relocalized; "particles", "headings", "ticks", "poses_skipped", "relocalized", "max_error_m": the largest
    error_m (0.0 without a tick)}.  A tick without an estimate (nothing stands) has NaN estimates and an infinite error."""
    what = "track_on_map"
    cells, origin, res, dev = _scan._grid(grid, what, filter_args.get("device"))
    if not isinstance(scanner, dict) or set(scanner) - {"beams", "fov_deg", "max_range"}:
        raise ValueError(f"{what}: scanner must be a dict with keys among beams, fov_deg, max_range (got {scanner!r})")
    beams, fov, reach = scanner.get("beams", 360), scanner.get("fov_deg", 360.0), scanner.get("max_range")
    _scan.beam_angles(beams, fov)
    drift = {} if drift is None else drift
    if not isinstance(drift, dict) or set(drift) - {"scale", "yaw_deg_per_m"}:
        raise ValueError(f"{what}: drift must be a dict with keys among scale, yaw_deg_per_m (got {drift!r})")
    scale = _number(drift.get("scale", 1.0), "drift scale", what, positive=True)
    turn = drift.get("yaw_deg_per_m", 0.0)
    if isinstance(turn, bool) or not isinstance(turn, (int, float)) or not math.isfinite(float(turn)):
        raise ValueError(f"{what}: drift yaw_deg_per_m must be a finite number (got {turn!r})")
    turn = math.radians(float(turn))
    pf = ParticleFilter(grid, n_particles, headings, n_beams=beams, seed=seed,
                        max_range=math.inf if reach is None else reach, **filter_args)
    host = cells.cpu().numpy()
    rows, skipped, relocalized, last = [], 0, 0, None
    for pose in poses:
        cell = None
        if pose is not None:
            try:
                cell = _plan.map_cell(cells.shape, origin, res, pose[0], "pose", what)
            except ValueError:
                cell = None
        if cell is None or host[cell] != _scan.MAP_FREE:
            skipped += 1
            continue
        xy, yaw = (float(pose[0][0]), float(pose[0][1])), float(pose[1])
        if last is None:
            pf.seed_around(xy, yaw, 2.0 * res if sigma_xy_m is None else sigma_xy_m,
                           3.0 * 2.0 * math.pi / pf.H if sigma_yaw is None else sigma_yaw)
            last = (xy, yaw)
            continue
        dx, dy = xy[0] - last[0][0], xy[1] - last[0][1]
        c, s = math.cos(last[1]), math.sin(last[1])
        d_f, d_l = (dx * c + dy * s) * scale, (-dx * s + dy * c) * scale
        d_yaw = _wrap_angle(yaw - last[1]) + turn * math.hypot(dx, dy)
        scan = _scan.scan_on_map(grid, xy, yaw, beams, fov, reach, True, device=dev)
        ranges = scan["ranges_m"].cpu().numpy()
        est = pf.step((d_f, d_l, d_yaw), ranges, scan["angles"])
        row = {"true_x": xy[0], "true_y": xy[1], "true_yaw": yaw, "est_x": math.nan, "est_y": math.nan, "est_yaw": math.nan,
               "error_m": math.inf, "yaw_error": math.inf, "ess": float(est["ess"]),
               "best_mean_cost": float(est["best_mean_cost"]), "n_standing": est["n_standing"],
               "resampled": int(est["resampled"]), "lost": int(est["lost"]), "relocalized": 0}
        if est["found"]:
            row.update(est_x=est["xy"][0], est_y=est["xy"][1], est_yaw=est["yaw"],
                       error_m=math.hypot(est["xy"][0] - xy[0], est["xy"][1] - xy[1]),
                       yaw_error=abs(_wrap_angle(est["yaw"] - yaw)))
        if est["lost"]:
            found = pf.recover(ranges, scan["angles"])
            row["relocalized"] = int(found["found"])
            relocalized += row["relocalized"]
        rows.append(row)
        last = (xy, yaw)
    return {"rows": rows, "particles": pf.N, "headings": pf.H, "ticks": len(rows), "poses_skipped": skipped,
            "relocalized": relocalized, "max_error_m": max((r["error_m"] for r in rows), default=0.0)}


def mcl_config(value, what="fuse_from_config: tsdf.esdf.mcl"):
    """None when the config value is absent (or has enable false), else the checked {"up_axis", "height", "beams",
    "fov_deg", "max_range", "every", "particles", "headings", "drift": {"scale", "yaw_deg_per_m"}, "seed"}: up_axis and
    height (h0, h1) as in tsdf.esdf.slice, beams 360, fov_deg 360 and max_range (metres; None: the whole map) of the
    scanner, every >= 1 (5), particles in [1, 65536] (2048), headings in [1, 1024] (360), drift's scale > 0 (1) and
    yaw_deg_per_m (0), seed >= 0 (0).  ValueError for an unknown key or a bad value.  Touches no device."""
    if value is None:
        return None
    keys = {"enable", "up_axis", "height", "beams", "fov_deg", "max_range", "every", "particles", "headings", "drift", "seed"}
    if not isinstance(value, dict) or set(value) - keys:
        raise ValueError(f"{what} must be a dict with keys among {sorted(keys)} (got {value!r})")
    if not isinstance(value.get("enable", True), bool):
        raise ValueError(f"{what}.enable must be a bool (got {value['enable']!r})")
    if not value.get("enable", True):
        return None
    base = _scan.scan_config({k: value[k] for k in ("up_axis", "height", "beams", "fov_deg", "max_range", "every")
                              if k in value}, what)
    drift = value.get("drift", {})
    if not isinstance(drift, dict) or set(drift) - {"scale", "yaw_deg_per_m"}:
        raise ValueError(f"{what}.drift must be a dict with keys among ['scale', 'yaw_deg_per_m'] (got {drift!r})")
    scale = _number(drift.get("scale", 1.0), "drift.scale", what, positive=True)
    turn = drift.get("yaw_deg_per_m", 0.0)
    if isinstance(turn, bool) or not isinstance(turn, (int, float)) or not math.isfinite(float(turn)) \
            or not math.isfinite(scale):
        raise ValueError(f"{what}.drift: scale and yaw_deg_per_m must be finite numbers (got {drift!r})")
    return {"up_axis": base["up_axis"], "height": base["height"], "beams": base["beams"], "fov_deg": base["fov_deg"],
            "max_range": base["max_range"], "every": base["every"],
            "particles": _int(value.get("particles", 2048), 1, MAX_PARTICLES, "particles", what),
            "headings": _int(value.get("headings", 360), 1, MAX_HEADINGS, "headings", what),
            "drift": {"scale": scale, "yaw_deg_per_m": float(turn)},
            "seed": _int(value.get("seed", 0), 0, (1 << 63) - 1, "seed", what)}


def track_poses(grid, poses, cfg):
    """The dict `mcl_text` writes: `track_on_map` over every cfg["every"]-th pose with cfg's scanner, particles, headings,
    drift and seed (`mcl_config`)."""
    return track_on_map(grid, poses[::cfg["every"]],
                        {"beams": cfg["beams"], "fov_deg": cfg["fov_deg"], "max_range": cfg["max_range"]},
                        n_particles=cfg["particles"], headings=cfg["headings"], drift=cfg["drift"], seed=cfg["seed"])


def mcl_text(result):
    """The text of map/mcl.txt: two header lines, one tab-separated row per tick in MCL_ROW_ORDER, then `name<TAB>value`
    per summary value.  Numbers are written with repr(): reading the file gives them back bit for bit."""
    lines = [_MCL_HEAD + ": a particle filter driven along the run's poses with a range scan cast at each and odometry "
             "from consecutive poses (metres and radians; error_m and yaw_error against the true pose; lost: the filter "
             "asked for the exhaustive match, relocalized: the match found a pose)", "\t".join(MCL_ROW_ORDER)]
    for row in result["rows"]:
        lines.append("\t".join(repr(int(row[k]) if k in _MCL_ROW_INTS else float(row[k])) for k in MCL_ROW_ORDER))
    lines += [f"{k}\t{(float(result[k]) if k in _MCL_SUMMARY_FLOATS else int(result[k]))!r}" for k in MCL_SUMMARY_ORDER]
    return "\n".join(lines) + "\n"


def parse_mcl(text):
    """mcl_text's inverse: the dict it was given."""
    lines = text.splitlines()
    n = len(lines) - 2 - len(MCL_SUMMARY_ORDER)
    if n < 0 or not lines[0].startswith(_MCL_HEAD) or lines[1].split("\t") != list(MCL_ROW_ORDER):
        raise ValueError("not a map/mcl.txt")
    result = {"rows": []}
    for line in lines[2:2 + n]:
        values = line.split("\t")
        if len(values) != len(MCL_ROW_ORDER):
            raise ValueError(f"mcl.txt: a row of {len(values)} values, {len(MCL_ROW_ORDER)} are expected")
        result["rows"].append({k: int(s) if k in _MCL_ROW_INTS else float(s) for k, s in zip(MCL_ROW_ORDER, values)})
    for key, line in zip(MCL_SUMMARY_ORDER, lines[2 + n:]):
        name, _, value = line.partition("\t")
        if name != key:
            raise ValueError(f"mcl.txt: expected {key}, found {name}")
        result[key] = float(value) if key in _MCL_SUMMARY_FLOATS else int(value)
    return result
