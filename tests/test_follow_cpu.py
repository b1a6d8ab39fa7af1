"""The sampled-rollout controller without a GPU: the restatement (tests/follow_restatement.py) against independent
fp64 formulas and hand-applied steps, the host side's refusals and the text file, and the restatement's closed loop
through the door room, whose tick counts are the reference of the GPU test's bound."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import follow_restatement as R                                 # noqa: E402

f32 = np.float32
U = 2.0 ** -24                                              # the unit roundoff of fp32; one ulp of 1.0 is 2 U
WEIGHTS = dict(w_togo=1.0, w_clear=1.0, w_turn=0.02, w_end=8.0, collision_cost=100.0, margin=0.1)
_REF = {}


def free_model(dims=(6, 5, 4), voxel=0.05, up_axis=2, height=0.075, radius=0.0, togo=None, dist=None, **over):
    """A lattice without obstacles: dist 1 m everywhere, togo the Manhattan distance to cell (0, 0, 0) in milli-voxels."""
    if dist is None:
        dist = np.ones(dims, dtype=np.float32)
    if togo is None:
        i, j, k = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
        togo = ((i + j + k) * 1000).astype(np.int32)
    args = dict(WEIGHTS)
    args.update(over)
    return R.Model(dist, togo, (0.0, 0.0, 0.0), voxel, up_axis, height, 0.1, 0.5, 1.5, radius, **args)


def door_model():
    """The door room of the issue with its cost-to-go to cell (40, 8, 1), once."""
    if "door" not in _REF:
        solid, d2, dist, passable = R.door_room()
        togo = R.togo_field(passable, (40, 8, 1))
        for a in (solid, d2, dist, passable, togo):
            a.setflags(write=False)
        _REF["door"] = (solid, d2, dist, passable, togo)
    solid, d2, dist, passable, togo = _REF["door"]
    return R.Model(dist, togo, (0.0, 0.0, 0.0), 0.05, 2, 0.075, 0.1, 0.5, 1.5, 0.08, **WEIGHTS), passable, togo


def test_cayley_step_against_the_fp64_unicycle():
    """One step turns the heading by 2 atan(h), h = w dt / 2.  atan's series alternates with shrinking terms for h < 1,
    so |2 atan(h) - w dt| <= 2 h^3 / 3 = |w dt|^3 / 12.  Rounding, to first order in U = 2^-24, for |w dt| <= 0.5 (h <=
    0.25, h^2 <= 1/16): h carries U, h^2 3U, and cr = (1 - h^2) / (1 + h^2) is one rounding each for numerator,
    denominator and quotient plus h^2's error scaled by h^2 (1 / (1 - h^2) + 1 / (1 + h^2)) <= 0.13, in all <= 3.4U; sr =
    2h / (1 + h^2) carries h's U and two roundings, 3U.  A product adds U: every product of c' = c cr - s sr and s' = s cr
    + c sr is within 4.4U of itself, and the difference adds U |c'|.  The heading angle moves by |c' ds' - s' dc'| <=
    4.4U (|s'| A + |c'| B) + 2U |c' s'| with A = |c cr| + |s sr| <= 1 and B = |s cr| + |c sr| <= 1 by Cauchy-Schwarz for
    unit (c, s) and (cr, sr), so by at most (4.4 sqrt 2 + 1) U = 7.3U = 3.6 ulp of 1: within the 4 ulp asserted.

    The norm: in exact arithmetic cr^2 + sr^2 = 1.  The worst case of the same roundings moves c^2 + s^2 by about 9U a
    step (2U from the denominator, 2.4U from numerator and quotient, and 2U (1 + sqrt(1 + 2 |cr sr|)) <= 4.8U from the
    products and differences), which only a run of 256 steps with every rounding falling the same way would reach;
    rounding to nearest is signed, and the drift asserted is T 2^-21 = 8U T."""
    m = free_model()
    rng = np.random.default_rng(0)
    worst_angle = 0.0
    for w in np.concatenate([rng.uniform(-5.0, 5.0, 64), [5.0, -5.0, 1.5, 1e-3, 0.0]]).astype(np.float32):
        th = rng.uniform(-math.pi, math.pi)
        c, s = f32(math.cos(th)), f32(math.sin(th))
        x1, y1, c1, s1 = R.step(m, f32(0.3), f32(-0.2), c, s, f32(0.4), w)
        assert all(v.dtype == np.float32 for v in (x1, y1, c1, s1))
        turn = float(w) * float(m.dt)                                          # |w dt| <= 0.5
        want = math.atan2(float(s), float(c)) + turn
        got = math.atan2(float(s1), float(c1))
        err = abs((got - want + math.pi) % (2 * math.pi) - math.pi)
        worst_angle = max(worst_angle, err - abs(turn) ** 3 / 12)
        assert err <= abs(turn) ** 3 / 12 + 4 * 2 * U, (w, err)
        # the position moves along the new heading by dt v
        assert abs(float(x1) - (0.3 + 0.1 * 0.4 * float(c1))) <= 4 * U and abs(float(y1) - (-0.2 + 0.1 * 0.4 * float(s1))) <= 4 * U
    T = 256
    c, s = f32(1.0), f32(0.0)
    x = y = f32(0.0)
    drift = 0.0
    ws = rng.uniform(-1.5, 1.5, T).astype(np.float32)
    for t in range(T):
        x, y, c, s = R.step(m, x, y, c, s, f32(0.5), ws[t])
        drift = max(drift, abs(float(c) ** 2 + float(s) ** 2 - 1.0))
    print("angle error beyond the series' term %.3g rad, norm drift over %d steps %.3g" % (worst_angle, T, drift))
    assert drift < T * 2.0 ** -21


def test_zero_noise_rollout_equals_hand_applied_steps():
    m = free_model(dims=(40, 40, 4), height=0.06)               # 1.2 voxels up: the nearest layer is 1
    T = 17
    Uc = np.stack([np.linspace(0.1, 0.5, T), np.linspace(-1.0, 1.5, T)], axis=1).astype(np.float32)
    start = [0.5, 0.6, 0.6, 0.8]
    S, end, hit, closest = R.rollouts(m, start, Uc, np.zeros((T, 3, 2), dtype=np.float32))
    state = [f32(v) for v in start]
    total = f32(0.0)
    for t in range(T):
        state = list(R.step(m, *state, Uc[t, 0], Uc[t, 1]))
        cell = [int(np.floor(v / m.voxel + f32(0.5))) for v in state[:2]]
        togo_term = f32(1.0) * (f32(m.togo[cell[0], cell[1], 1]) * m.metres_per_milli)
        total = total + (togo_term + f32(0.02) * (Uc[t, 1] * Uc[t, 1]))
    total = total + f32(8.0) * togo_term
    assert (hit == T).all() and np.array_equal(end, np.tile(np.array(state, dtype=np.float32), (3, 1)))
    assert S.dtype == np.float32 and (S == total).all() and (closest == 1.0).all()


def test_rollout_aimed_at_a_wall_collides_where_the_position_is_first_blocked():
    m, passable, togo = door_model()
    T = 32
    Uc = np.tile(np.array([[0.5, 0.0]], dtype=np.float32), (T, 1))
    start = [8 * 0.05, 10 * 0.05, 1.0, 0.0]                                     # straight at the wall, away from the door
    S, end, hit, closest = R.rollouts(m, start, Uc, np.zeros((T, 2, 2), dtype=np.float32))
    state, first = [f32(v) for v in start], None
    states = []
    for t in range(T):
        state = list(R.step(m, *state, f32(0.5), f32(0.0)))
        cell = R.nearest(m, state[0], state[1])
        if cell is None or togo[tuple(cell)] >= R.INF:
            first = t
            break
        states.append(state)
    assert first is not None and 0 < first < T and (hit == first).all()
    assert np.array_equal(end[0], np.array(states[-1], dtype=np.float32))           # frozen at the last good state
    live = R.rollouts(m, start, Uc[:first], np.zeros((first, 1, 2), dtype=np.float32))
    assert live[2][0] == first and float(S[0]) > 100.0                            # the same steps alone never collide
    assert closest[0] == live[3][0] > 0.08
    # collision on step 0: a start one step from leaving the lattice
    S0, end0, hit0, closest0 = R.rollouts(m, [0.02, 0.5, -1.0, 0.0], Uc, np.zeros((T, 1, 2), dtype=np.float32))
    assert hit0[0] == 0 and closest0[0] == np.inf and S0[0] == f32(100.0)           # the start itself is blocked: frozen 0
    assert np.array_equal(end0[0], np.array([0.02, 0.5, -1.0, 0.0], dtype=np.float32))


def test_nan_noise_leaves_the_rollout_on_the_nominal_control():
    m = free_model(dims=(40, 40, 4))
    T = 4
    Uc = np.tile(np.array([[0.3, 0.5]], dtype=np.float32), (T, 1))
    nz = np.zeros((T, 4, 2), dtype=np.float32)
    nz[1, 1, 0], nz[2, 2, 1], nz[0, 3, :] = np.nan, np.inf, (-np.inf, np.nan)
    S, end, hit, _ = R.rollouts(m, [0.5, 0.5, 1.0, 0.0], Uc, nz)
    assert np.array_equal(end[1], end[0]) and np.array_equal(end[2], end[0]) and np.array_equal(end[3], end[0])
    assert (S == S[0]).all() and (hit == T).all()
    assert (R.deltas(m, Uc, nz) == 0).all()
    v, w = R.control(m, np.array([0.3, 0.5], dtype=np.float32), np.array([[9.0, -9.0], [-9.0, 9.0]], dtype=np.float32))
    assert v.tolist() == [0.5, 0.0] and w.tolist() == [-1.5, 1.5]                  # the limits


def test_update_against_a_plain_fp64_formula():
    m = free_model(dims=(40, 40, 4))
    rng = np.random.default_rng(3)
    T, K = 5, 37
    Uc = np.stack([rng.uniform(0, 0.5, T), rng.uniform(-1.5, 1.5, T)], axis=1).astype(np.float32)
    nz = R.make_noise(K, T, 0.15, 0.6, rng)
    S = rng.uniform(3.0, 9.0, K).astype(np.float32)
    s_min, best, omega, eta, ess = R.weights(S, 0.3)
    assert s_min == S.min() and best == int(np.argmin(S)) and omega[best] == 1.0 and eta >= 1.0
    lam = float(f32(0.3))
    want = np.zeros((T, 2))
    for t in range(T):
        for k in range(K):
            a = [float(Uc[t, c]) + float(nz[t, k, c]) for c in range(2)]
            a = [min(max(a[0], 0.0), 0.5), min(max(a[1], -1.5), 1.5)]
            for c in range(2):
                want[t, c] += math.exp(-(float(S[k]) - float(s_min)) / lam) * (a[c] - float(Uc[t, c]))
    want = Uc.astype(np.float64) + want / sum(math.exp(-(float(S[k]) - float(s_min)) / lam) for k in range(K))
    want[:, 0], want[:, 1] = np.clip(want[:, 0], 0, 0.5), np.clip(want[:, 1], -1.5, 1.5)
    plain, u0 = R.update(m, Uc, nz, omega, eta, False)
    # the formula above adds and subtracts in fp64; the restatement rounds U + noise, the delta and the new row to fp32,
    # each within half an ulp of a magnitude below 4: 3 * 2^-23 in all
    assert np.abs(plain - want).max() <= 3 * 2.0 ** -23 and np.array_equal(u0, plain[0])
    shifted, u1 = R.update(m, Uc, nz, omega, eta, True)
    assert np.array_equal(shifted[:-1], plain[1:]) and np.array_equal(shifted[-1], plain[-1]) and np.array_equal(u1, u0)
    w2 = sum(math.exp(-(float(S[k]) - float(s_min)) / lam) ** 2 for k in range(K))
    assert abs(ess - eta * eta / w2) <= 1e-12 * ess and 1.0 <= ess <= K


def test_host_side_refusals_touch_no_device():
    from go_slam_amd import follow
    g = torch.Generator().manual_seed(0)
    nz = follow.noise(5, 3, 0.15, 0.6, g)
    assert nz.dtype == torch.float32 and tuple(nz.shape) == (3, 5, 2) and (nz[:, 0] == 0).all() and (nz[:, 1:] != 0).all()
    assert torch.equal(nz, follow.noise(5, 3, 0.15, 0.6, torch.Generator().manual_seed(0)))
    for bad in ((0, 3, 0.1, 0.1), (65537, 3, 0.1, 0.1), (4, 0, 0.1, 0.1), (4, 257, 0.1, 0.1), (4, 3, -0.1, 0.1),
                (4, 3, 0.1, math.nan), (4.0, 3, 0.1, 0.1), (True, 3, 0.1, 0.1)):
        with pytest.raises(ValueError, match="follow.noise"):
            follow.noise(*bad)
    dist = torch.ones((6, 5, 4))
    togo = torch.zeros((6, 5, 4), dtype=torch.int32)
    Uc = torch.zeros((3, 2))
    good = dict(dist=dist, togo=togo, lo=(0, 0, 0), voxel=0.05, state=(0.1, 0.1, 1.0, 0.0), U=Uc, noise=nz, up_axis=2,
                height=0.07, dt=0.1, v_max=0.5, w_max=1.5, robot_radius=0.05)
    for key, bad in (("dist", torch.ones((1, 5, 4))), ("dist", torch.ones((6, 5))), ("togo", togo.float()),
                     ("togo", togo[:5]), ("voxel", 0.0), ("voxel", math.inf), ("state", (0.1, 0.1, 1.0)),
                     ("state", (0.1, math.nan, 1.0, 0.0)), ("U", torch.zeros((4, 2))), ("U", Uc.double()),
                     ("noise", nz[:, :, 0]), ("noise", nz.double()), ("up_axis", 3), ("up_axis", 1.0),
                     ("height", math.nan), ("dt", 0.0), ("dt", -0.1), ("v_max", math.inf), ("w_max", 0.0),
                     ("robot_radius", -0.1), ("lo", (0, 0)), ("lo", (0, math.inf, 0)), ("weights", {"togo": -1.0}),
                     ("weights", {"margin": 0.0}), ("weights", {"speed": 1.0}), ("weights", {"clear": math.nan}),
                     ("weights", [1.0])):
        with pytest.raises(ValueError, match="follow.rollouts"):
            follow.rollouts(**{**good, key: bad})
    with pytest.raises(ValueError, match="follow.weights"):
        follow.weights(torch.zeros(4), 0.3)                                      # not on the GPU
    with pytest.raises(ValueError, match="follow.update"):
        follow.update(Uc, nz, torch.ones(5, dtype=torch.float64), torch.ones(2, dtype=torch.float64), 0.5, 1.5)
    for bad in ({"up_axis": 2, "K": 0}, {"up_axis": 5}, {"K": 256}, {"up_axis": 2, "speed": 1}, {"up_axis": 2, "dt": 0},
                {"up_axis": 2, "sigma": 0.1}, {"up_axis": 2, "weights": {"margin": -1}}, {"up_axis": 2, "enable": 1},
                {"up_axis": 2, "heading": [0, 0]}, {"up_axis": 2, "lam": 0.0}, {"up_axis": 2, "seed": 1.5}, True, [2]):
        with pytest.raises(ValueError, match="tsdf.esdf.plan.follow"):
            follow.follow_config(bad)
    assert follow.follow_config(None) is None and follow.follow_config({"enable": False, "up_axis": 9}) is None
    assert follow.follow_config({"up_axis": 1, "K": 256, "sigma": [0.1, 0.5]}) == (1, {"K": 256, "sigma": [0.1, 0.5]})


def test_follow_text_round_trips():
    from go_slam_amd import follow
    rng = np.random.default_rng(5)
    trace = rng.standard_normal((7, 4)).astype(np.float32)
    controls = rng.standard_normal((6, 2)).astype(np.float32)
    res = {"reached": True, "ticks": 6, "trace": trace, "controls": controls, "length_m": 1.25, "min_clearance_m": 0.1 + 0.2,
           "stops": 1, "ess_min": 3.3333333333333335}
    head, t2, c2 = follow.parse_follow(follow.follow_text(res))
    assert head == {"reached": True, "ticks": 6, "length_m": 1.25, "min_clearance_m": 0.1 + 0.2, "stops": 1,
                    "ess_min": 3.3333333333333335, "n_states": 7}
    assert np.array_equal(t2, trace) and np.array_equal(c2, controls) and t2.dtype == np.float32
    empty = {"reached": False, "ticks": 0, "trace": np.zeros((0, 4), np.float32), "controls": np.zeros((0, 2), np.float32),
             "length_m": 0.0, "min_clearance_m": math.inf, "stops": 0, "ess_min": math.inf}
    head, t2, c2 = follow.parse_follow(follow.follow_text(empty))
    assert head["reached"] is False and head["n_states"] == 0 and head["min_clearance_m"] == math.inf
    assert t2.shape == (0, 4) and c2.shape == (0, 2)
    with pytest.raises(ValueError):
        follow.parse_follow("Collision-free path through\n\n")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_closed_loop_of_the_restatement_reaches_the_goal_through_the_door(seed):
    """The issue's door room (48 x 40 x 4 cells of 0.05 m, wall at index 24 of the first axis, door at 26..31 of the
    second, robot radius 0.08 m: the cells 27..30 of the door pass), start cell (8, 30) heading along the first axis,
    goal cell (40, 8), the plane halfway between layers 1 and 2, K = 256, T = 32, dt = 0.1 s, the default weights and a
    goal tolerance of 2000 milli-voxels.  Measured here: seeds 0, 1, 2 reach the goal in 50, 50 and 50 ticks with stops
    == 0, 2.0 m driven, never closer than 0.12 m to a surface (seeds 3..9: 49 to 54 ticks); the door did not have to be
    widened.  The GPU test bounds Controller.drive's ticks by 1.5 times this run's count of the same seed."""
    m, passable, togo = door_model()
    res = R.Loop(m, 256, 32, (0.15, 0.6), 0.3, seed).drive([8 * 0.05, 30 * 0.05, 1.0, 0.0], 300, 2000)
    print("seed", seed, {k: v for k, v in res.items() if k not in ("trace", "controls")})
    assert res["reached"] and res["stops"] == 0
    assert res["ticks"] == len(res["controls"]) == len(res["trace"]) - 1
    assert 2.2 / (0.5 * 0.1) * 0.8 <= res["ticks"] <= 75        # 2.2 m of route at 0.5 m/s is 44 ticks; the goal has a tolerance
    for x, y in res["trace"][:, :2]:
        assert passable[tuple(R.nearest(m, x, y))]
    assert res["min_clearance_m"] > 0.08 and abs(res["length_m"] - 2.1) < 0.3
    last = R.nearest(m, *res["trace"][-1, :2])
    assert togo[tuple(last)] <= 2000
