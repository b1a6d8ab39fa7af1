"""Following a planned route: a sampled-rollout (model-predictive path-integral) controller of a differential-drive base
over a fused volume's distance field (csrc/follow.hip; include/goslam_hip.h, gs_follow_*; tests/follow_restatement.py;
DESIGN.md section 34).

Every tick `rollouts` runs K perturbed control sequences of T steps from the robot's state through `ESDF.dist` and the
cost-to-go field of the goal (`plan.geodesic_field` over `ESDF.passable`), `weights` turns their costs into fp64 weights
and `update` moves the nominal sequence to the weighted mean of the applied controls and shifts it by one step.  The
model is a unicycle stepped by Cayley's rotation, fp32 with + - * / alone, so the rollouts equal their numpy restatement
bit for bit.  `Controller` keeps the fields and the nominal sequence on the device (`step`: three launches and one small
read) and `drive` closes the loop on the host with the same step; `ESDF.follow` (tsdf.py) is the one call from a start
and a goal, and `follow_text` / `parse_follow` are the run's map/follow.txt.
"""
import math

import numpy as np
import torch

from . import _lib
from . import plan as _plan

MAX_ROLLOUTS = 65536                   # GS_FOLLOW_MAX_ROLLOUTS
MAX_STEPS = 256                        # GS_FOLLOW_MAX_STEPS
INF = _plan.INF
# per step: togo [1 / m of route left], clear [at the surface of the robot], turn [1 / (rad/s)^2]; end: the weight of the
# last step's to-go term again; collision: once per rollout; margin [m]: the band beyond the radius that costs
DEFAULT_WEIGHTS = {"togo": 1.0, "clear": 1.0, "turn": 0.02, "end": 8.0, "collision": 100.0, "margin": 0.1}
DEFAULT_TOLERANCE = 2000               # milli-voxels of route left at which the goal counts as reached


def _number(value, name, what, positive=False):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}: {name} must be a number (got {value!r})")
    value = float(value)
    if not math.isfinite(value) or not math.isfinite(float(np.float32(value))) or value < 0 or (positive and value <= 0):
        raise ValueError(f"{what}: {name} must be finite and {'positive' if positive else '>= 0'} (got {value})")
    return value


def _count(value, name, top, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= top:
        raise ValueError(f"{what}: {name} must be an integer in [1, {top}] (got {value!r})")
    return int(value)


def cost_weights(weights, what="follow"):
    """DEFAULT_WEIGHTS with the dict `weights` (None: nothing) laid over it, every value checked; ValueError for an
    unknown key, a value that is no finite number >= 0, or a margin that is not positive."""
    if weights is None:
        weights = {}
    if not isinstance(weights, dict) or set(weights) - set(DEFAULT_WEIGHTS):
        raise ValueError(f"{what}: weights is a dict with keys among {sorted(DEFAULT_WEIGHTS)} (got {weights!r})")
    out = dict(DEFAULT_WEIGHTS)
    out.update(weights)
    return {k: _number(v, f"weights[{k!r}]", what, positive=(k == "margin")) for k, v in out.items()}


def model_arguments(up_axis, height, dt, v_max, w_max, robot_radius, weights, what="follow"):
    """The checked model parameters as a dict, or ValueError.  Touches no device."""
    if isinstance(up_axis, bool) or not isinstance(up_axis, (int, np.integer)) or not 0 <= int(up_axis) <= 2:
        raise ValueError(f"{what}: up_axis must be 0, 1 or 2 (got {up_axis!r})")
    if isinstance(height, bool) or not isinstance(height, (int, float, np.integer, np.floating)) \
            or not math.isfinite(float(height)):
        raise ValueError(f"{what}: height must be a finite world coordinate (got {height!r})")
    return {"up_axis": int(up_axis), "height": float(height), "dt": _number(dt, "dt", what, True),
            "v_max": _number(v_max, "v_max", what, True), "w_max": _number(w_max, "w_max", what, True),
            "robot_radius": _number(robot_radius, "robot_radius", what), "weights": cost_weights(weights, what)}


def state_arguments(state, what="follow"):
    """(x, y, c, s) as four finite floats, or ValueError."""
    try:
        s = [float(v) for v in (state.tolist() if hasattr(state, "tolist") else state)]
    except (TypeError, ValueError):
        s = []
    if len(s) != 4 or not all(math.isfinite(v) for v in s):
        raise ValueError(f"{what}: a state is four finite numbers (x, y, c, s) (got {state!r})")
    return s


def noise(K, T, sigma_v, sigma_w, generator=None, device=None):
    """The perturbations of one tick, float32 [T,K,2]: normal with standard deviations (sigma_v, sigma_w), drawn by
    `generator` on its device and moved to `device` (default: the generator's, the CPU without one).  Rollout 0 is all
    zeros, so the nominal sequence is always a candidate."""
    what = "follow.noise"
    K, T = _count(K, "K", MAX_ROLLOUTS, what), _count(T, "T", MAX_STEPS, what)
    sigma_v, sigma_w = _number(sigma_v, "sigma_v", what), _number(sigma_w, "sigma_w", what)
    src = generator.device if generator is not None else torch.device("cpu")
    nz = torch.randn((T, K, 2), dtype=torch.float32, device=src, generator=generator)
    nz = nz * torch.tensor([sigma_v, sigma_w], dtype=torch.float32, device=src)
    nz[:, 0, :] = 0
    return nz if device is None else nz.to(device)


def _checked(t, name, dtype, shape, what):
    """`t`, a tensor of exactly this dtype and shape, or ValueError; touches no device."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be a {dtype} tensor {list(shape)} "
                         f"(got {getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))})")
    return t


def _sizes(noise_, what):
    if not isinstance(noise_, torch.Tensor) or noise_.dim() != 3 or noise_.shape[2] != 2:
        raise ValueError(f"{what}: noise must be a float32 tensor [T,K,2] (got {list(getattr(noise_, 'shape', []))})")
    T, K = int(noise_.shape[0]), int(noise_.shape[1])
    return _count(K, "K", MAX_ROLLOUTS, what), _count(T, "T", MAX_STEPS, what)


@torch.no_grad()
def rollouts(dist, togo, lo, voxel, state, U, noise, up_axis, height, dt, v_max, w_max, robot_radius, weights=None):
    """gs_follow_rollouts: K rollouts of T steps from `state` (x, y, c, s) under the nominal controls U [T,2] plus noise
    [T,K,2] through dist float32 and togo int32, both [n0,n1,n2] on the lattice (lo, voxel).  -> {"S": float32 [K] the
    costs, "end": float32 [K,4] the last states, "hit_step": int32 [K] (T: never collided), "min_dist": float32 [K] the
    smallest distance over a rollout's live steps (inf without one)}, on the fields' device.  ValueError before the
    device is touched; nothing is read back."""
    what = "follow.rollouts"
    K, T = _sizes(noise, what)
    if not isinstance(dist, torch.Tensor) or dist.dim() != 3 or not all(2 <= int(n) <= 1024 for n in dist.shape):
        raise ValueError(f"{what}: dist must be [n0,n1,n2] with every size in [2, 1024] "
                         f"(got {list(getattr(dist, 'shape', []))})")
    dims = tuple(int(n) for n in dist.shape)
    m = model_arguments(up_axis, height, dt, v_max, w_max, robot_radius, weights, what)
    state = state_arguments(state, what)
    voxel = _number(voxel, "voxel", what, True)
    lo = [float(v) for v in lo]
    if len(lo) != 3 or not all(math.isfinite(v) for v in lo):
        raise ValueError(f"{what}: lo is three finite world coordinates (got {lo!r})")
    fields = (_checked(dist, "dist", torch.float32, dims, what), _checked(togo, "togo", torch.int32, dims, what),
              _checked(U, "U", torch.float32, (T, 2), what), _checked(noise, "noise", torch.float32, (T, K, 2), what))
    dev = dist.device if dist.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dist, togo, U, noise = (t.to(dev).contiguous() for t in fields)
    out = {"S": torch.empty(K, dtype=torch.float32, device=dev), "end": torch.empty((K, 4), dtype=torch.float32, device=dev),
           "hit_step": torch.empty(K, dtype=torch.int32, device=dev),
           "min_dist": torch.empty(K, dtype=torch.float32, device=dev)}
    w = m["weights"]
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_follow_rollouts(
            _lib.ptr(dist), _lib.ptr(togo), *dims, lo[0], lo[1], lo[2], voxel, m["up_axis"], m["height"], *state,
            _lib.ptr(U), _lib.ptr(noise), K, T, m["dt"], m["v_max"], m["w_max"], m["robot_radius"], w["margin"], w["togo"],
            w["clear"], w["turn"], w["end"], w["collision"], _lib.ptr(out["S"]), _lib.ptr(out["end"]),
            _lib.ptr(out["hit_step"]), _lib.ptr(out["min_dist"]), _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return out


@torch.no_grad()
def weights(S, lam):
    """gs_follow_weights: the costs S float32 [K] (on the GPU) -> {"s_min": float32 [1], "best": int32 [1] the lowest k
    with the smallest cost, "omega": float64 [K] = exp(-(S - s_min) / lam), "stats": float64 [2] = (eta, ess), the sum of
    the weights and the effective sample size}.  ValueError before the device is touched; nothing is read back."""
    what = "follow.weights"
    if not isinstance(S, torch.Tensor) or S.dtype != torch.float32 or S.dim() != 1 or not S.is_cuda:
        raise ValueError(f"{what}: S must be a float32 tensor [K] on the GPU")
    K = _count(int(S.shape[0]), "K", MAX_ROLLOUTS, what)
    lam = _number(lam, "lam", what, True)
    dev = S.device
    S = S.contiguous()
    out = {"s_min": torch.empty(1, dtype=torch.float32, device=dev), "best": torch.empty(1, dtype=torch.int32, device=dev),
           "omega": torch.empty(K, dtype=torch.float64, device=dev), "stats": torch.empty(2, dtype=torch.float64, device=dev)}
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_follow_weights(_lib.ptr(S), K, lam, _lib.ptr(out["s_min"]), _lib.ptr(out["best"]),
                                          _lib.ptr(out["omega"]), _lib.ptr(out["stats"]), _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return out


@torch.no_grad()
def update(U, noise, omega, stats, v_max, w_max, shift=True, out=None):
    """gs_follow_update: the nominal controls U float32 [T,2] moved to the weighted mean of the controls the rollouts
    applied under noise [T,K,2] and the weights (omega float64 [K], stats float64 [2]) of `weights`, clamped to the
    limits.  With `shift` row t goes to row t - 1 and the last row is repeated: the sequence of the next tick.  ->
    (U_new float32 [T,2], written into `out` when given (another tensor than U), u_exec float32 [2], the unshifted row
    0: the control to execute now).  ValueError before the device is touched; nothing is read back."""
    what = "follow.update"
    K, T = _sizes(noise, what)
    if not isinstance(U, torch.Tensor) or not U.is_cuda:
        raise ValueError(f"{what}: U must be a float32 tensor [T,2] on the GPU")
    dev = U.device
    v_max, w_max = _number(v_max, "v_max", what, True), _number(w_max, "w_max", what, True)
    fields = (_checked(U, "U", torch.float32, (T, 2), what), _checked(noise, "noise", torch.float32, (T, K, 2), what),
              _checked(omega, "omega", torch.float64, (K,), what), _checked(stats, "stats", torch.float64, (2,), what))
    U, noise, omega, stats = (t.to(dev).contiguous() for t in fields)
    if out is None:
        out = torch.empty((T, 2), dtype=torch.float32, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (T, 2) \
            or out.device != dev or not out.is_contiguous() or out.data_ptr() == U.data_ptr():
        raise ValueError(f"{what}: out must be a contiguous float32 tensor [{T},2] on {dev}, another one than U")
    u_exec = torch.empty(2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_follow_update(_lib.ptr(U), _lib.ptr(noise), _lib.ptr(omega), _lib.ptr(stats), K, T, v_max,
                                         w_max, 1 if shift else 0, _lib.ptr(out), _lib.ptr(u_exec), _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return out, u_exec


def no_drive():
    """`Controller.drive`'s dict before the first tick: what a start without a route to the goal gets."""
    return {"reached": False, "ticks": 0, "trace": np.zeros((0, 4), np.float32), "controls": np.zeros((0, 2), np.float32),
            "length_m": 0.0, "min_clearance_m": math.inf, "stops": 0, "ess_min": math.inf}


class _HostModel:
    """The rollout's step and sample for one state on the host, numpy float32 with one operation per line: what `drive`
    applies the commanded control with.  `dist` and `togo` are host copies of the fields."""

    def __init__(self, dist, togo, lo, voxel, m):
        f = np.float32
        self.dist, self.togo, self.dims = dist, togo, dist.shape
        self.lo, self.voxel = [f(v) for v in lo], f(voxel)
        self.up_axis, self.height, self.dt, self.half_dt = m["up_axis"], f(m["height"]), f(m["dt"]), f(0.5) * f(m["dt"])

    def step(self, state, v, w):
        f = np.float32
        x, y, c, s = (f(a) for a in state)
        v, w = f(v), f(w)
        h = self.half_dt * w
        hh = h * h
        den = f(1.0) + hh
        cr = (f(1.0) - hh) / den
        sr = (f(2.0) * h) / den
        c1 = c * cr - s * sr
        s1 = s * cr + c * sr
        dv = self.dt * v
        return [x + dv * c1, y + dv * s1, c1, s1]

    def cell(self, x, y):
        """(the nearest lattice point, the trilinear distance) of a position, or None where the rollout collides for
        want of a cell."""
        f = np.float32
        planar = iter((f(x), f(y)))
        p = [self.height if a == self.up_axis else next(planar) for a in range(3)]
        g = [(p[a] - self.lo[a]) / self.voxel for a in range(3)]
        a = [np.floor(v) for v in g]
        if not all(a[i] >= 0 and a[i] < f(self.dims[i] - 1) for i in range(3)):
            return None
        near = [int(np.floor(g[i] + f(0.5))) for i in range(3)]
        i0, i1, i2 = (int(v) for v in a)
        sx, sy, sz = (g[i] - a[i] for i in range(3))
        v = self.dist[i0:i0 + 2, i1:i1 + 2, i2:i2 + 2]
        lerp = lambda p_, q_, s_: p_ + s_ * (q_ - p_)   # noqa: E731
        z00, z01 = lerp(v[0, 0, 0], v[0, 0, 1], sz), lerp(v[0, 1, 0], v[0, 1, 1], sz)
        z10, z11 = lerp(v[1, 0, 0], v[1, 0, 1], sz), lerp(v[1, 1, 0], v[1, 1, 1], sz)
        return near, float(lerp(lerp(z00, z01, sy), lerp(z10, z11, sy), sx))


class Controller:
    """The controller of one goal on one `ESDF`.  Built once: `passable(robot_radius, allow_unknown)`, the goal's
    cost-to-go field (`.field`; the goal moved by `snap` metres to a passable cell as `ESDF.plan` does, `.goal_cell`, None
    when there is none) and the nominal controls `.U` float32 [T,2], zeros, on the device.  `weights` lays over
    DEFAULT_WEIGHTS; `sigma` = (sigma_v, sigma_w) of the noise, `lam` the temperature; `generator` (default: one on the
    field's device seeded with `seed`) draws the noise.  ValueError for a bad argument before the device is touched."""

    def __init__(self, esdf, goal, up_axis, height, robot_radius, allow_unknown=False, snap=0.0, K=2048, T=32, dt=0.1,
                 v_max=0.5, w_max=1.5, sigma=(0.15, 0.6), lam=0.3, weights=None, seed=0, generator=None):
        what = "follow.Controller"
        self.m = model_arguments(up_axis, height, dt, v_max, w_max, robot_radius, weights, what)
        self.K, self.T = _count(K, "K", MAX_ROLLOUTS, what), _count(T, "T", MAX_STEPS, what)
        try:
            sigma = tuple(sigma)
        except TypeError:
            sigma = ()
        if len(sigma) != 2:
            raise ValueError(f"{what}: sigma is (sigma_v, sigma_w) (got {sigma!r})")
        self.sigma = (_number(sigma[0], "sigma[0]", what), _number(sigma[1], "sigma[1]", what))
        self.lam = _number(lam, "lam", what, True)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise ValueError(f"{what}: seed must be an integer (got {seed!r})")
        (g,), snap_cells, _ = esdf.plan_arguments([goal], robot_radius, snap, None, what)
        self.esdf, self.device = esdf, esdf.device
        passable = esdf.passable(robot_radius, allow_unknown)
        self.goal_cell = _plan.snap_cell(passable, g, snap_cells)
        self.field = _plan.geodesic_field(passable, [] if self.goal_cell is None else [self.goal_cell])
        self.togo = self.field.cost
        self.dist = esdf.dist.contiguous()
        self.U = torch.zeros((self.T, 2), dtype=torch.float32, device=self.device)
        self._spare = torch.empty_like(self.U)
        if generator is None:
            generator = torch.Generator(device=self.device)
            generator.manual_seed(int(seed))
        self.generator = generator
        self._host = None

    def reset(self):
        """The nominal controls back to zeros."""
        self.U.zero_()

    @torch.no_grad()
    def step(self, state):
        """One tick from `state` (x, y, c, s): draws the noise, then gs_follow_rollouts, gs_follow_weights and
        gs_follow_update (shifted, into the spare buffer, which becomes `.U`), and one small read.  -> (v, w, info): the
        control to execute now and {"ess": the effective sample size, "hit_step": the step at which the cheapest rollout
        collided, T when it did not, "s_min": its cost}."""
        state = state_arguments(state, "Controller.step")
        m, dev = self.m, self.device
        nz = noise(self.K, self.T, self.sigma[0], self.sigma[1], self.generator, dev)
        roll = rollouts(self.dist, self.togo, self.esdf.lo, self.esdf.voxel, state, self.U, nz, m["up_axis"], m["height"],
                        m["dt"], m["v_max"], m["w_max"], m["robot_radius"], m["weights"])
        wt = weights(roll["S"], self.lam)
        new, u_exec = update(self.U, nz, wt["omega"], wt["stats"], m["v_max"], m["w_max"], True, self._spare)
        self.U, self._spare = new, self.U
        hit = roll["hit_step"][wt["best"].long()]
        v, w, ess, hit, s_min = torch.cat([u_exec.double(), wt["stats"][1:], hit.double(),
                                           wt["s_min"].double()]).cpu().tolist()                  # the tick's one read
        return v, w, {"ess": ess, "hit_step": int(hit), "s_min": s_min}

    def host_model(self):
        """The fields copied to the host once, for `drive`."""
        if self._host is None:
            self._host = _HostModel(self.dist.cpu().numpy(), self.togo.cpu().numpy(), self.esdf.lo, self.esdf.voxel, self.m)
        return self._host

    @torch.no_grad()
    def drive(self, start_state, max_ticks=400, goal_tolerance=DEFAULT_TOLERANCE):
        """The closed loop from `start_state`: every tick `step`, then the commanded control applied to the state on the
        host with the rollout's own step.  A commanded step that would itself collide under the rollout rule (no cell, or
        a nearest lattice point the robot's centre may not be at) is replaced by (0, 0) and counted in "stops".  It ends
        when the state's nearest lattice point has at most `goal_tolerance` milli-voxels of route left ("reached") or
        after `max_ticks`.  -> {"reached", "ticks", "trace": float32 [ticks + 1, 4] the states, the start first,
        "controls": float32 [ticks, 2], "length_m", "min_clearance_m": the smallest trilinear distance over the states
        moved to (inf without one), "stops", "ess_min"}.  A start that has no route to the goal gives reached False and
        empty traces, and nothing is launched."""
        what = "Controller.drive"
        state = [np.float32(v) for v in state_arguments(start_state, what)]
        max_ticks = _count(max_ticks, "max_ticks", 1 << 20, what)
        if isinstance(goal_tolerance, bool) or not isinstance(goal_tolerance, (int, np.integer)) \
                or not 0 <= int(goal_tolerance) < INF:
            raise ValueError(f"{what}: goal_tolerance must be an integer in [0, {INF}) milli-voxels (got {goal_tolerance!r})")
        out = no_drive()
        if self.goal_cell is None:
            return out
        host = self.host_model()
        at = host.cell(state[0], state[1])
        if at is None or int(host.togo[tuple(at[0])]) >= INF:
            return out
        trace, controls = [list(state)], []
        for _ in range(max_ticks):
            at = host.cell(state[0], state[1])
            if int(host.togo[tuple(at[0])]) <= goal_tolerance:
                out["reached"] = True
                break
            v, w, info = self.step(state)
            out["ess_min"] = min(out["ess_min"], info["ess"])
            nxt = host.step(state, v, w)
            to = host.cell(nxt[0], nxt[1])
            if to is None or int(host.togo[tuple(to[0])]) >= INF:
                out["stops"] += 1
                v = w = 0.0
            else:
                state = nxt
                out["length_m"] += float(np.float32(self.m["dt"]) * np.float32(v))
                out["min_clearance_m"] = min(out["min_clearance_m"], to[1])
            controls.append([v, w])
            trace.append(list(state))
        out.update(ticks=len(controls), trace=np.array(trace, dtype=np.float32).reshape(-1, 4),
                   controls=np.array(controls, dtype=np.float32).reshape(-1, 2))
        return out


CONTROLLER_KEYS = ("robot_radius", "allow_unknown", "snap", "K", "T", "dt", "v_max", "w_max", "sigma", "lam", "weights",
                   "seed")
CONFIG_KEYS = ("enable", "up_axis", "heading", "max_ticks", "goal_tolerance") + CONTROLLER_KEYS


def follow_config(value, what="tsdf.esdf.plan.follow"):
    """None when the config value (absent, or a dict with enable false) switches the controller off, else (up_axis, the
    dict of `ESDF.follow`'s further arguments); ValueError for anything else: no dict, an unknown key, a missing up_axis
    or a value `Controller` refuses.  Touches no device."""
    if value is None:
        return None
    if not isinstance(value, dict) or set(value) - set(CONFIG_KEYS) or not isinstance(value.get("enable", True), bool):
        raise ValueError(f"{what} must be a dict with keys among {list(CONFIG_KEYS)} and a bool enable (got {value!r})")
    if not value.get("enable", True):
        return None
    args = {k: v for k, v in value.items() if k not in ("enable", "up_axis")}
    model_arguments(value.get("up_axis"), 0.0, args.get("dt", 0.1), args.get("v_max", 0.5), args.get("w_max", 1.5),
                    args.get("robot_radius", 0.0), args.get("weights"), what)
    _count(args.get("K", 2048), "K", MAX_ROLLOUTS, what)
    _count(args.get("T", 32), "T", MAX_STEPS, what)
    _count(args.get("max_ticks", 400), "max_ticks", 1 << 20, what)
    _number(args.get("lam", 0.3), "lam", what, True)
    _number(args.get("snap", 0.0), "snap", what)
    sigma = args.get("sigma", (0.15, 0.6))
    if not isinstance(sigma, (list, tuple)) or len(sigma) != 2:
        raise ValueError(f"{what}: sigma is (sigma_v, sigma_w) (got {sigma!r})")
    for i in range(2):
        _number(sigma[i], f"sigma[{i}]", what)
    if not isinstance(args.get("allow_unknown", False), bool):
        raise ValueError(f"{what}: allow_unknown must be a bool (got {args['allow_unknown']!r})")
    for key in ("seed", "goal_tolerance"):
        if key in args and (isinstance(args[key], bool) or not isinstance(args[key], int)):
            raise ValueError(f"{what}: {key} must be an integer (got {args[key]!r})")
    if args.get("heading") is not None:
        h = args["heading"]
        if not isinstance(h, (list, tuple)) or len(h) != 2 or not all(
                isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in h) \
                or h[0] == 0 == h[1]:
            raise ValueError(f"{what}: heading is a direction (c, s) in the plane of motion (got {h!r})")
    return int(value["up_axis"]), args


FOLLOW_REPORT_ORDER = ("reached", "ticks", "length_m", "min_clearance_m", "stops", "ess_min", "n_states")
_FOLLOW_HEADER = "Closed-loop drive"


def follow_text(result):
    """The text of map/follow.txt for the dict of `Controller.drive` / `ESDF.follow`: two header lines,
    `name<TAB>repr(value)` for reached, ticks, length_m, min_clearance_m, stops, ess_min and n_states, then one line per
    state, `x y c s v w` with repr(): the state and the control executed from it (the last state's control is 0 0).
    Reading the file gives back the float32 numbers bit for bit."""
    trace = np.asarray(result["trace"], dtype=np.float32).reshape(-1, 4)
    controls = np.asarray(result["controls"], dtype=np.float32).reshape(-1, 2)
    head = {"reached": bool(result["reached"]), "ticks": int(result["ticks"]), "length_m": float(result["length_m"]),
            "min_clearance_m": float(result["min_clearance_m"]), "stops": int(result["stops"]),
            "ess_min": float(result["ess_min"]), "n_states": int(trace.shape[0])}
    lines = [_FOLLOW_HEADER + " of a differential-drive base down the cost-to-go field of map/path.txt's goal by the "
             "sampled-rollout controller, start to goal: the states [m, unit heading] on the plane of motion and the "
             "controls [m/s, rad/s] executed from them",
             "(reached: the goal's tolerance was met; ticks: controls executed; length_m: distance driven; min_clearance_m: "
             "the smallest distance to a surface over the states; stops: commands replaced by a halt; ess_min: the "
             "smallest effective sample size; then per state: x y c s v w)"]
    lines += [f"{k}\t{head[k]!r}" for k in FOLLOW_REPORT_ORDER]
    for i, s in enumerate(trace):
        u = controls[i] if i < controls.shape[0] else (0.0, 0.0)
        lines.append(" ".join(repr(float(v)) for v in (*s, *u)))
    return "\n".join(lines) + "\n"


def parse_follow(text):
    """follow_text's inverse: (the dict of FOLLOW_REPORT_ORDER, trace float32 [n,4], controls float32 [max(n - 1, 0), 2])."""
    lines = text.splitlines()
    if len(lines) < 2 + len(FOLLOW_REPORT_ORDER) or not lines[0].startswith(_FOLLOW_HEADER):
        raise ValueError("not a map/follow.txt")
    result = {}
    for key, line in zip(FOLLOW_REPORT_ORDER, lines[2:]):
        name, _, value = line.partition("\t")
        if name != key:
            raise ValueError(f"follow.txt: expected {key}, found {name}")
        if key == "reached":
            if value not in ("True", "False"):
                raise ValueError(f"follow.txt: reached is {value!r}")
            result[key] = value == "True"
        else:
            result[key] = int(value) if key in ("ticks", "stops", "n_states") else float(value)
    rows = [[float(v) for v in line.split(" ")] for line in lines[2 + len(FOLLOW_REPORT_ORDER):]]
    if len(rows) != result["n_states"] or any(len(r) != 6 for r in rows):
        raise ValueError("follow.txt: the states do not match n_states")
    rows = np.array(rows, dtype=np.float32).reshape(-1, 6)
    return result, rows[:, :4].copy(), rows[:max(rows.shape[0] - 1, 0), 4:].copy()
