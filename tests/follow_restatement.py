"""A plain numpy restatement of the sampled-rollout controller (include/goslam_hip.h, gs_follow_*).

Every quantity of a rollout is a numpy float32 and every line is one operation, so each result is rounded once, as the
kernel's is (-ffp-contract=off); the K rollouts are the elements of the arrays, the T steps a Python loop.  `weights` and
`update` are the fp64 formulas with numpy's own summation: their order is not the kernel's, which the tests' bound covers.
`Loop` is the closed loop of `follow.Controller.drive` on the host alone.
"""
import math

import numpy as np

INF = 0x3fffffff
f32 = np.float32


class Model:
    """The lattice, the two fields and the parameters of gs_follow_rollouts, all rounded to fp32 once."""

    def __init__(self, dist, togo, lo, voxel, up_axis, height, dt, v_max, w_max, robot_radius, margin, w_togo, w_clear,
                 w_turn, w_end, collision_cost):
        self.dist = np.ascontiguousarray(dist, dtype=np.float32)
        self.togo = np.ascontiguousarray(togo, dtype=np.int32)
        self.dims = self.dist.shape
        self.lo = [f32(v) for v in lo]
        self.voxel = f32(voxel)
        self.up_axis = int(up_axis)
        self.height = f32(height)
        self.dt, self.v_max, self.w_max = f32(dt), f32(v_max), f32(w_max)
        self.half_dt = f32(0.5) * self.dt
        self.margin = f32(margin)
        self.robot_radius = f32(robot_radius)
        self.reach = self.robot_radius + self.margin
        self.w_togo, self.w_clear, self.w_turn, self.w_end = f32(w_togo), f32(w_clear), f32(w_turn), f32(w_end)
        self.collision_cost = f32(collision_cost)
        self.metres_per_milli = self.voxel / f32(1000.0)


def control(m, u, nz):
    """u f32 [2], nz f32 [K,2] -> the applied controls (v [K], w [K])."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = u[0] + nz[:, 0]
        w = u[1] + nz[:, 1]
    v = np.where(np.isfinite(v), v, u[0]).astype(np.float32)
    w = np.where(np.isfinite(w), w, u[1]).astype(np.float32)
    v = np.where(v < 0, f32(0.0), np.where(v > m.v_max, m.v_max, v)).astype(np.float32)
    w = np.where(w < -m.w_max, -m.w_max, np.where(w > m.w_max, m.w_max, w)).astype(np.float32)
    return v, w


def step(m, x, y, c, s, v, w):
    """One Cayley step of length dt; arrays or scalars of float32."""
    h = m.half_dt * w
    hh = h * h
    den = f32(1.0) + hh
    cr = (f32(1.0) - hh) / den
    sr = (f32(2.0) * h) / den
    c1 = c * cr - s * sr
    s1 = s * cr + c * sr
    dv = m.dt * v
    return x + dv * c1, y + dv * s1, c1, s1


def _lerp(p, q, s):
    return p + s * (q - p)


def sample(m, x, y):
    """x, y f32 [K] -> (live bool [K], togo_term, cost, d f32 [K]; zeros where not live)."""
    x = np.asarray(x, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    K = x.shape[0]
    planar = iter((x, y))
    p = [np.full(K, m.height, dtype=np.float32) if a == m.up_axis else next(planar) for a in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        g = [(p[a] - m.lo[a]) / m.voxel for a in range(3)]
        a = [np.floor(g[i]) for i in range(3)]
        inside = np.ones(K, dtype=bool)
        for i in range(3):
            inside &= (a[i] >= 0) & (a[i] < f32(m.dims[i] - 1))
    # a point without a cell reads cell (0, 0, 0) below and is masked out afterwards
    g = [np.where(inside, g[i], f32(0.0)).astype(np.float32) for i in range(3)]
    a = [np.where(inside, a[i], f32(0.0)).astype(np.float32) for i in range(3)]
    near = [np.floor(g[i] + f32(0.5)).astype(np.int64) for i in range(3)]
    tv = m.togo[near[0], near[1], near[2]]
    live = inside & (tv < INF)
    i0, i1, i2 = (a[i].astype(np.int64) for i in range(3))
    sx, sy, sz = (g[i] - a[i] for i in range(3))
    v = m.dist
    z00, z01 = _lerp(v[i0, i1, i2], v[i0, i1, i2 + 1], sz), _lerp(v[i0, i1 + 1, i2], v[i0, i1 + 1, i2 + 1], sz)
    z10 = _lerp(v[i0 + 1, i1, i2], v[i0 + 1, i1, i2 + 1], sz)
    z11 = _lerp(v[i0 + 1, i1 + 1, i2], v[i0 + 1, i1 + 1, i2 + 1], sz)
    d = _lerp(_lerp(z00, z01, sy), _lerp(z10, z11, sy), sx)
    togo_term = m.w_togo * (tv.astype(np.float32) * m.metres_per_milli)
    with np.errstate(invalid="ignore", over="ignore"):
        cost = np.where(d < m.reach, togo_term + (m.w_clear * (m.reach - d)) / m.margin, togo_term)
    zero = f32(0.0)
    return (live, np.where(live, togo_term, zero).astype(np.float32), np.where(live, cost, zero).astype(np.float32),
            np.where(live, d, zero).astype(np.float32))


def rollouts(m, state, U, noise):
    """state four floats, U f32 [T,2], noise f32 [T,K,2] -> (S f32 [K], end f32 [K,4], hit_step i32 [K], min_dist f32
    [K]): gs_follow_rollouts."""
    U = np.asarray(U, dtype=np.float32)
    noise = np.asarray(noise, dtype=np.float32)
    T, K = noise.shape[0], noise.shape[1]
    x, y, c, s = (np.full(K, f32(v), dtype=np.float32) for v in state)
    live0, togo0, cost0, _ = sample(m, x, y)
    frozen = np.where(live0, cost0, f32(0.0)).astype(np.float32)
    last = togo0.copy()
    S = np.zeros(K, dtype=np.float32)
    hit = np.full(K, T, dtype=np.int32)
    closest = np.full(K, np.inf, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            going = hit == T
            v, w = control(m, U[t], noise[t])
            x1, y1, c1, s1 = step(m, x, y, c, s, v, w)
            live, togo_term, cost, d = sample(m, np.where(going, x1, x), np.where(going, y1, y))
            moved = going & live
            struck = going & ~live
            x, y = np.where(moved, x1, x), np.where(moved, y1, y)
            c, s = np.where(moved, c1, c), np.where(moved, s1, s)
            frozen = np.where(moved, cost + m.w_turn * (w * w), frozen).astype(np.float32)
            last = np.where(moved, togo_term, last)
            closest = np.where(moved & (d < closest), d, closest)
            hit = np.where(struck, t, hit).astype(np.int32)
            S = np.where(struck, S + m.collision_cost, S).astype(np.float32)
            S = (S + frozen).astype(np.float32)
        S = np.where(hit == T, S + m.w_end * last, S).astype(np.float32)
    return S, np.stack([x, y, c, s], axis=1).astype(np.float32), hit, closest.astype(np.float32)


def weights(S, lam):
    """S f32 [K] -> (s_min f32, best, omega f64 [K], eta, ess): gs_follow_weights in numpy's fp64."""
    S = np.asarray(S, dtype=np.float32)
    s_min = S.min()
    omega = np.exp(-(S.astype(np.float64) - np.float64(s_min)) / np.float64(f32(lam)))
    eta = omega.sum()
    return s_min, int(np.argmin(S)), omega, float(eta), float(eta * eta / (omega * omega).sum())


def deltas(m, U, noise):
    """The applied perturbations f32 [T,K,2]."""
    U = np.asarray(U, dtype=np.float32)
    out = np.empty(noise.shape, dtype=np.float32)
    for t in range(noise.shape[0]):
        v, w = control(m, U[t], noise[t])
        out[t, :, 0] = v - U[t, 0]
        out[t, :, 1] = w - U[t, 1]
    return out


def clamp_rows(m, rows):
    rows = np.asarray(rows, dtype=np.float32).copy()
    rows[:, 0] = np.minimum(np.maximum(rows[:, 0], f32(0.0)), m.v_max)
    rows[:, 1] = np.minimum(np.maximum(rows[:, 1], -m.w_max), m.w_max)
    return rows


def update(m, U, noise, omega, eta, shift):
    """-> (U_new f32 [T,2], u_exec f32 [2]): gs_follow_update, each delta's mean rounded to fp32 before it is added."""
    U = np.asarray(U, dtype=np.float32)
    mean = np.einsum("k,tkc->tc", omega, deltas(m, U, noise).astype(np.float64)) / eta
    rows = clamp_rows(m, U + mean.astype(np.float32))
    if shift:
        return np.concatenate([rows[1:], rows[-1:]], axis=0), rows[0].copy()
    return rows, rows[0].copy()


def make_noise(K, T, sigma_v, sigma_w, rng):
    """follow.noise with a numpy Generator: f32 [T,K,2], rollout 0 all zeros."""
    nz = rng.standard_normal((T, K, 2)).astype(np.float32) * np.array([sigma_v, sigma_w], dtype=np.float32)
    nz[:, 0, :] = 0
    return nz


def nearest(m, x, y):
    """The nearest lattice point of the state's position, or None when the point has no cell."""
    planar = iter((f32(x), f32(y)))
    p = [m.height if a == m.up_axis else next(planar) for a in range(3)]
    g = [(p[a] - m.lo[a]) / m.voxel for a in range(3)]
    if not all(0 <= np.floor(g[i]) < f32(m.dims[i] - 1) for i in range(3)):
        return None
    return [int(np.floor(g[i] + f32(0.5))) for i in range(3)]


class Loop:
    """The closed loop: every tick K rollouts, the weights, the shifted update, then the commanded step applied to the
    state with `step`; a commanded step that would collide under the rollout rule is replaced by (0, 0) and counted."""

    def __init__(self, model, K, T, sigma, lam, seed):
        self.m, self.K, self.T, self.sigma, self.lam = model, K, T, sigma, lam
        self.rng = np.random.default_rng(seed)
        self.U = np.zeros((T, 2), dtype=np.float32)

    def tick(self, state):
        nz = make_noise(self.K, self.T, self.sigma[0], self.sigma[1], self.rng)
        S, _, hit, _ = rollouts(self.m, state, self.U, nz)
        _, best, omega, eta, ess = weights(S, self.lam)
        self.U, u = update(self.m, self.U, nz, omega, eta, True)
        return u, ess, int(hit[best])

    def drive(self, state, max_ticks, goal_tolerance):
        m = self.m
        state = [f32(v) for v in state]
        trace, controls, stops, ess_min, reached, clearance, length = [list(state)], [], 0, math.inf, False, math.inf, 0.0
        for _ in range(max_ticks):
            cell = nearest(m, state[0], state[1])
            if cell is not None and int(m.togo[cell[0], cell[1], cell[2]]) <= goal_tolerance:
                reached = True
                break
            u, ess, _ = self.tick(state)
            ess_min = min(ess_min, ess)
            nxt = step(m, state[0], state[1], state[2], state[3], u[0], u[1])
            live, _, _, d = sample(m, np.array([nxt[0]]), np.array([nxt[1]]))
            if not live[0]:
                stops += 1
                u = np.zeros(2, dtype=np.float32)
            else:
                length += float(m.dt * u[0])
                clearance = min(clearance, float(d[0]))
                state = [f32(v) for v in nxt]
            controls.append([float(u[0]), float(u[1])])
            trace.append(list(state))
        return {"reached": reached, "ticks": len(controls), "trace": np.array(trace, dtype=np.float32).reshape(-1, 4),
                "controls": np.array(controls, dtype=np.float32).reshape(-1, 2), "length_m": length,
                "min_clearance_m": clearance, "stops": stops, "ess_min": ess_min}


def door_room(n0=48, n1=40, n2=4, voxel=0.05, wall=24, door=(26, 31), radius=0.08):
    """The issue's room: a wall at index `wall` of the first axis with a door at `door` (inclusive) of the second, the
    same on every layer, boundary walls around.  -> (solid bool, d2 int32 the squared distance in voxels to the nearest
    solid cell by brute force, dist f32 = voxel * sqrt(d2) in metres, passable bool: the cell is free and dist > radius,
    which is ESDF.passable's d2 > floor((radius / voxel)^2) for integer d2)."""
    solid = np.zeros((n0, n1, n2), dtype=bool)
    solid[0], solid[-1], solid[:, 0], solid[:, -1] = True, True, True, True
    solid[wall] = True
    solid[wall, door[0]:door[1] + 1] = False
    s2 = np.argwhere(solid[:, :, 0]).astype(np.float64)
    ii, jj = np.meshgrid(np.arange(n0), np.arange(n1), indexing="ij")
    d2 = ((ii[..., None] - s2[:, 0]) ** 2 + (jj[..., None] - s2[:, 1]) ** 2).min(axis=-1)
    dist2 = (np.sqrt(d2) * voxel).astype(np.float32)
    dist = np.ascontiguousarray(np.repeat(dist2[:, :, None], n2, axis=2))
    d2 = np.ascontiguousarray(np.repeat(d2[:, :, None], n2, axis=2).astype(np.int32))
    passable = ~solid & (dist > radius)
    return solid, d2, dist, passable


MOVES = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
WEIGHT = {1: 1000, 2: 1414, 3: 1732}


def togo_field(passable, goal):
    """The cost-to-go in milli-voxels by Dijkstra over the 26 moves that cut no corner (the rule of gs_geodesic_*)."""
    import heapq
    dims = passable.shape
    cost = np.full(dims, INF, dtype=np.int64)
    goal = tuple(int(v) for v in goal)
    if not passable[goal]:
        return cost.astype(np.int32)
    cost[goal] = 0
    heap = [(0, goal)]
    while heap:
        cst, at = heapq.heappop(heap)
        if cst > cost[at]:
            continue
        for mv in MOVES:
            to = (at[0] + mv[0], at[1] + mv[1], at[2] + mv[2])
            if not all(0 <= to[i] < dims[i] for i in range(3)):
                continue
            box = passable[min(at[0], to[0]):max(at[0], to[0]) + 1, min(at[1], to[1]):max(at[1], to[1]) + 1,
                           min(at[2], to[2]):max(at[2], to[2]) + 1]
            if not box.all():
                continue
            cand = cst + WEIGHT[sum(1 for v in mv if v)]
            if cand < cost[to]:
                cost[to] = cand
                heapq.heappush(heap, (cand, to))
    return cost.astype(np.int32)
