"""The sampled-rollout controller on the MI355X (csrc/follow.hip, go_slam_amd/follow.py, ESDF.follow): the rollouts equal
the numpy restatement (tests/follow_restatement.py) with torch.equal, the weights and the update lie within a derived
bound of the fp64 restatement fed the kernel's own costs and are bitwise reproducible, the C entries refuse bad arguments
before anything is written, Controller.drive gets through the door room, and an only-tracking run with
tsdf.esdf.plan.follow ends with map/follow.txt."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import follow_restatement as R                                 # noqa: E402
import test_esdf_gpu as EG                                     # noqa: E402  (its only-tracking run)
import test_follow_cpu as FC                                   # noqa: E402  (the door room, once)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1
_REF = {}


def gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)             # a copy: the shared references are read-only


def small_lattice():
    """6 x 5 x 4 cells of 0.05 m with a lo that is no multiple of the voxel: distances on both sides of the radius plus
    margin, a fifth of the cells closed to the robot's centre."""
    if "small" not in _REF:
        rng = np.random.default_rng(11)
        dist = rng.uniform(-0.05, 0.4, (6, 5, 4)).astype(np.float32)
        togo = rng.integers(0, 9000, (6, 5, 4)).astype(np.int32)
        togo[rng.random((6, 5, 4)) < 0.2] = R.INF
        togo[2:4, 2:4, 1:3] = np.minimum(togo[2:4, 2:4, 1:3], 8999)              # the start's surroundings pass
        dist.setflags(write=False)
        togo.setflags(write=False)
        _REF["small"] = (dist, togo)
    return _REF["small"]


def scene(name):
    """(model, start state, U row, noise sigmas): `small_up1` on a layer of axis 1, `small_up0` between layers of axis 0,
    both with a speed limit that leaves the lattice in one step; `door`, the door room between two layers, and `door_on`,
    on one."""
    if name.startswith("small"):
        dist, togo = small_lattice()
        up, height = (1, 0.013 + 2 * 0.05) if name == "small_up1" else (0, -0.02 + 0.06 + 2 * 0.05)
        m = R.Model(dist, togo, (-0.02, 0.013, 0.1), 0.05, up, height, 0.1, 3.0, 4.0, 0.1, margin=0.15, w_togo=0.7,
                    w_clear=2.0, w_turn=0.05, w_end=3.0, collision_cost=50.0)
        start = [-0.02 + 0.13, 0.1 + 0.08, 0.6, 0.8] if up == 1 else [0.013 + 0.12, 0.1 + 0.07, 0.6, 0.8]
        return m, start, (0.2, 0.5), (1.0, 2.0)
    m, _, _ = FC.door_model()
    if name == "door_on":
        m = R.Model(m.dist, m.togo, (0.0, 0.0, 0.0), 0.05, 2, 0.1, 0.1, 0.5, 1.5, 0.08, **FC.WEIGHTS)
    return m, [11 * 0.05, 20 * 0.05, 1.0, 0.0], (0.3, 0.2), (0.3, 1.2)     # the nominal rollout stops short of the wall


def case(name, K, T):
    m, start, u, sigma = scene(name)
    rng = np.random.default_rng(1000 * K + T)
    U = np.tile(np.array([u], dtype=np.float32), (T, 1))
    nz = R.make_noise(K, T, sigma[0], sigma[1], rng)
    if K > 2:
        nz[0, K // 2, 0] = np.nan                               # that rollout keeps U[0]'s speed
        nz[T - 1, K - 1, 1] = np.inf
        nz[0, 2, 0] = 99.0                                      # the speed limit: on the small lattice out in one step
    return m, start, U, nz


def c_rollouts(m, start, U, nz, fill=-7):
    """gs_follow_rollouts straight from the C entry into buffers pre-filled with `fill`."""
    from go_slam_amd import _lib
    T, K = nz.shape[0], nz.shape[1]
    out = (torch.full((K,), fill, dtype=torch.float32, device=DEV), torch.full((K, 4), fill, dtype=torch.float32, device=DEV),
           torch.full((K,), fill, dtype=torch.int32, device=DEV), torch.full((K,), fill, dtype=torch.float32, device=DEV))
    dist, togo, Ud, nzd = gpu(m.dist), gpu(m.togo), gpu(U), gpu(nz)
    P = _lib.ptr
    rc = _lib.lib().gs_follow_rollouts(
        P(dist), P(togo), *m.dims, *[float(v) for v in m.lo], float(m.voxel), m.up_axis, float(m.height),
        *[float(np.float32(v)) for v in start], P(Ud), P(nzd), K, T, float(m.dt), float(m.v_max), float(m.w_max),
        float(m.robot_radius), float(m.margin), float(m.w_togo), float(m.w_clear), float(m.w_turn), float(m.w_end),
        float(m.collision_cost), *[P(t) for t in out], _lib.stream_ptr(DEV))
    assert rc == 0, _lib.lib().gs_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("T", [1, 2, 17])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["small_up1", "small_up0", "door", "door_on"])
def test_rollouts_equal_the_restatement(built_lib, name, K, T):
    m, start, U, nz = case(name, K, T)
    want = R.rollouts(m, start, U, nz)
    got = c_rollouts(m, start, U, nz)
    hit = want[2]
    print(name, K, T, "collided", int((hit < T).sum()), "on step 0", int((hit == 0).sum()), "S", float(want[0].min()),
          float(want[0].max()))
    for g, w, what in zip(got, want, ("S", "end", "hit_step", "min_dist")):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), what
    assert np.isfinite(want[0]).all()
    if K >= 63 and name.startswith("small"):                    # the cases hold what they are there for
        assert (hit == 0).any() and hit[2] == 0 and ((hit == T).any() or T == 17) and (want[3] < m.reach).any()
    elif K >= 63 and T == 17:
        assert (hit < T).any() and (hit == T).any() and (want[3] < m.reach).any()


def test_rollout_wrapper_and_the_nan_entry(built_lib):
    from go_slam_amd import follow
    m, start, U, nz = case("door", 65, 17)
    res = follow.rollouts(gpu(m.dist), gpu(m.togo), (0, 0, 0), 0.05, start, gpu(U), gpu(nz), 2, 0.075, 0.1, 0.5, 1.5, 0.08)
    want = R.rollouts(m, start, U, nz)
    for key, w in zip(("S", "end", "hit_step", "min_dist"), want):
        assert torch.equal(res[key].cpu(), torch.from_numpy(w)), key
    clean = nz.copy()
    clean[0, 32, 0], clean[16, 64, 1] = 0.0, 0.0                # a non-finite entry is the nominal control
    again = c_rollouts(m, start, U, clean)
    assert torch.equal(again[1][32], res["end"][32]) and torch.equal(again[0][64], res["S"][64])


# ---- weights and update ----------------------------------------------------------------------------------------------
def c_weights_update(S, U, nz, lam, v_max, w_max, shift):
    from go_slam_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    T, K = nz.shape[0], nz.shape[1]
    stream = _lib.stream_ptr(DEV)
    s_min = torch.full((1,), -7, dtype=torch.float32, device=DEV)
    best = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    omega = torch.full((K,), -7, dtype=torch.float64, device=DEV)
    stats = torch.full((2,), -7, dtype=torch.float64, device=DEV)
    U_new = torch.full((T, 2), -7, dtype=torch.float32, device=DEV)
    u_exec = torch.full((2,), -7, dtype=torch.float32, device=DEV)
    Sd, Ud, nzd = gpu(S), gpu(U), gpu(nz)
    assert L.gs_follow_weights(P(Sd), K, lam, P(s_min), P(best), P(omega), P(stats), stream) == 0, L.gs_last_error()
    assert L.gs_follow_update(P(Ud), P(nzd), P(omega), P(stats), K, T, v_max, w_max, shift, P(U_new), P(u_exec),
                              stream) == 0, L.gs_last_error()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (s_min, best, omega, stats, U_new, u_exec)]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("K", [1, 63, 255, 256, 257, 1023, 1024, 1025, 2051])
def test_weights_and_update_within_the_derived_bound(built_lib, K, shift):
    """Reference: the restatement's fp64 formulas (numpy's summation order) fed the kernel's own S.  Bound on U_new: the
    weights are positive and the best rollout weighs exp(0) = 1, so eta >= 1.  omega[k] differs from numpy's by a few
    ulp of exp, 2^-52 each, and a sum of K products in any order by at most K 2^-53 times the sum of their magnitudes,
    sum_k omega |delta| <= eta max|delta|; after the division by eta >= 1 the two means differ by at most
    K 2^-50 max|delta| with room for exp's ulps and the sums of eta itself.  Both sides then round the mean to fp32 and
    add it to U[t] in fp32, which can move the result by one fp32 ulp of it when the two means straddle a rounding
    boundary.  |U_new - want| <= ulp32(|want|) + K 2^-50 max|delta|; not tuned on the GPU's output.  S_min and best are
    exact (a minimum has no rounding), ess to 1e-12 relative (K 2^-52 twice), and two runs are bitwise equal."""
    T = 5
    m, start, U, nz = case("door", K, T)
    rng = np.random.default_rng(K)
    U = np.stack([rng.uniform(0, 0.5, T), rng.uniform(-1.5, 1.5, T)], axis=1).astype(np.float32)
    S = c_rollouts(m, start, U, nz)[0].cpu().numpy()
    lam = 0.3
    s_min, best, omega, stats, U_new, u_exec = c_weights_update(S, U, nz, lam, 0.5, 1.5, shift)
    w_min, w_best, w_omega, w_eta, w_ess = R.weights(S, lam)
    assert s_min[0] == w_min and best[0] == w_best
    assert stats[0] >= 1.0 and abs(stats[0] - w_eta) <= 1e-12 * w_eta and abs(stats[1] - w_ess) <= 1e-12 * w_ess
    assert np.abs(omega - w_omega).max() <= 8 * 2.0 ** -52 and omega[best[0]] == 1.0
    want, want_exec = R.update(m, U, nz, w_omega, w_eta, bool(shift))
    slack = K * 2.0 ** -50 * float(np.abs(R.deltas(m, U, nz)).max())
    err = np.abs(U_new.astype(np.float64) - want.astype(np.float64))
    bound = np.spacing(np.abs(want)).astype(np.float64) + slack
    print("K", K, "shift", shift, "eta", stats[0], "ess", stats[1], "largest error / bound", float((err / bound).max()))
    assert (err <= bound).all()
    assert (np.abs(u_exec.astype(np.float64) - want_exec) <= np.spacing(np.abs(want_exec)) + slack).all()
    if shift:
        assert np.array_equal(U_new[-1], U_new[-2]) or T == 1
    else:
        assert np.array_equal(u_exec, U_new[0])
    again = c_weights_update(S, U, nz, lam, 0.5, 1.5, shift)
    for a, b in zip((s_min, best, omega, stats, U_new, u_exec), again):
        assert a.tobytes() == b.tobytes()


def test_weights_and_update_wrappers(built_lib):
    from go_slam_amd import follow
    m, start, U, nz = case("door", 257, 17)
    S = c_rollouts(m, start, U, nz)[0]
    wt = follow.weights(S, 0.3)
    new, u_exec = follow.update(gpu(U), gpu(nz), wt["omega"], wt["stats"], 0.5, 1.5, shift=True)
    plain, u0 = follow.update(gpu(U), gpu(nz), wt["omega"], wt["stats"], 0.5, 1.5, shift=False)
    s_min, best, omega, stats, U_new, ue = c_weights_update(S.cpu().numpy(), U, nz, 0.3, 0.5, 1.5, 1)
    assert np.array_equal(new.cpu().numpy(), U_new) and np.array_equal(u_exec.cpu().numpy(), ue)
    assert torch.equal(new[:-1], plain[1:]) and torch.equal(new[-1], plain[-1]) and torch.equal(u0, plain[0])
    assert int(wt["best"].item()) == int(best[0]) and float(wt["s_min"].item()) == float(s_min[0])
    Ud = gpu(U)
    with pytest.raises(ValueError, match="another one than U"):
        follow.update(Ud, gpu(nz), wt["omega"], wt["stats"], 0.5, 1.5, out=Ud)


def test_c_abi_refusals_leave_the_outputs_untouched(built_lib):
    from go_slam_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    stream = _lib.stream_ptr(DEV)
    dims, K, T = (6, 5, 4), 8, 3
    dist = torch.ones(dims, dtype=torch.float32, device=DEV)
    togo = torch.zeros(dims, dtype=torch.int32, device=DEV)
    U = torch.zeros((T, 2), dtype=torch.float32, device=DEV)
    nz = torch.zeros((T, K, 2), dtype=torch.float32, device=DEV)
    S = torch.full((K,), -7, dtype=torch.float32, device=DEV)
    end = torch.full((K, 4), -7, dtype=torch.float32, device=DEV)
    hit = torch.full((K,), -7, dtype=torch.int32, device=DEV)
    closest = torch.full((K,), -7, dtype=torch.float32, device=DEV)
    s_min = torch.full((1,), -7, dtype=torch.float32, device=DEV)
    best = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    omega = torch.full((K,), -7, dtype=torch.float64, device=DEV)
    stats = torch.full((2,), -7, dtype=torch.float64, device=DEV)
    U_new = torch.full((T, 2), -7, dtype=torch.float32, device=DEV)
    u_exec = torch.full((2,), -7, dtype=torch.float32, device=DEV)
    good = dict(dist=P(dist), togo=P(togo), n0=6, n1=5, n2=4, lo_x=0.0, lo_y=0.0, lo_z=0.0, voxel=0.05, up_axis=2,
                height=0.07, x=0.1, y=0.1, c=1.0, s=0.0, U=P(U), noise=P(nz), K=K, T=T, dt=0.1, v_max=0.5, w_max=1.5,
                robot_radius=0.05, margin=0.1, w_togo=1.0, w_clear=1.0, w_turn=0.02, w_end=8.0, collision_cost=100.0,
                S=P(S), end=P(end), hit_step=P(hit), min_dist=P(closest))
    nan, inf = math.nan, math.inf
    bad_rollouts = [("n0", 1), ("n1", 1025), ("n2", -1), ("K", 0), ("K", 65537), ("T", 0), ("T", 257), ("voxel", 0.0),
                    ("voxel", inf), ("lo_x", nan), ("up_axis", 3), ("up_axis", -1), ("height", inf), ("x", nan), ("s", inf),
                    ("dt", 0.0), ("dt", nan), ("v_max", -0.5), ("v_max", inf), ("w_max", 0.0), ("robot_radius", -0.01),
                    ("margin", 0.0), ("margin", nan), ("w_togo", -1.0), ("w_clear", inf), ("w_turn", nan), ("w_end", -1.0),
                    ("collision_cost", inf)]
    bad_rollouts += [(k, None) for k in ("dist", "togo", "U", "noise", "S", "end", "hit_step", "min_dist")]
    bad_rollouts += [("U", _lib.ctypes.c_void_p(U.data_ptr() + 4)), ("noise", _lib.ctypes.c_void_p(nz.data_ptr() + 4))]
    for key, value in bad_rollouts:
        assert L.gs_follow_rollouts(*{**good, key: value}.values(), stream) == INVALID, (key, value)
    assert b"follow_rollouts" in L.gs_last_error()
    for args in ((None, K, 0.3, P(s_min), P(best), P(omega), P(stats)), (P(S), 0, 0.3, P(s_min), P(best), P(omega), P(stats)),
                 (P(S), 65537, 0.3, P(s_min), P(best), P(omega), P(stats)), (P(S), K, 0.0, P(s_min), P(best), P(omega), P(stats)),
                 (P(S), K, nan, P(s_min), P(best), P(omega), P(stats)), (P(S), K, inf, P(s_min), P(best), P(omega), P(stats)),
                 (P(S), K, 0.3, None, P(best), P(omega), P(stats)), (P(S), K, 0.3, P(s_min), None, P(omega), P(stats)),
                 (P(S), K, 0.3, P(s_min), P(best), None, P(stats)), (P(S), K, 0.3, P(s_min), P(best), P(omega), None)):
        assert L.gs_follow_weights(*args, stream) == INVALID, args
    upd = dict(U=P(U), noise=P(nz), omega=P(omega), stats=P(stats), K=K, T=T, v_max=0.5, w_max=1.5, shift=1, U_new=P(U_new),
               u_exec=P(u_exec))
    for key, value in [("U", None), ("noise", None), ("omega", None), ("stats", None), ("U_new", None), ("u_exec", None),
                       ("K", 0), ("K", 65537), ("T", 0), ("T", 257), ("v_max", 0.0), ("w_max", nan), ("shift", 2),
                       ("shift", -1), ("U_new", P(U))]:
        assert L.gs_follow_update(*{**upd, key: value}.values(), stream) == INVALID, (key, value)
    assert b"follow_update" in L.gs_last_error()
    torch.cuda.synchronize()
    for t in (S, end, hit, closest, s_min, best, omega, stats, U_new, u_exec):
        assert (t == -7).all()                                  # nothing was launched
    assert L.gs_follow_rollouts(*good.values(), stream) == 0
    torch.cuda.synchronize()
    assert (hit == T).all() and (closest == 1.0).all() and (S == 0).all()          # standing still on togo 0


# ---- the closed loop -------------------------------------------------------------------------------------------------
def door_esdf(closed=False):
    """The door room as an ESDF built by hand from the restatement's arrays (a closed door: the wall without a gap)."""
    from go_slam_amd.tsdf import ESDF
    if closed:
        solid, d2, dist, passable = R.door_room(door=(26, 25))
    else:
        m, passable, _ = FC.door_model()
        solid, d2, dist, _ = FC._REF["door"][:4]
    state = np.where(solid, 2, 1).astype(np.uint8)
    return ESDF(gpu(state), gpu(d2), gpu(dist), (0.0, 0.0, 0.0), 0.05, state.shape, 64), passable


START, GOAL = (8 * 0.05, 30 * 0.05, 0.075), (40 * 0.05, 8 * 0.05, 0.05)


def reference_ticks(seed):
    """The CPU restatement's closed loop of tests/test_follow_cpu.py for this seed, once."""
    if ("ticks", seed) not in _REF:
        m, _, _ = FC.door_model()
        res = R.Loop(m, 256, 32, (0.15, 0.6), 0.3, seed).drive([START[0], START[1], 1.0, 0.0], 300, 2000)
        assert res["reached"] and res["stops"] == 0
        _REF[("ticks", seed)] = res["ticks"]
    return _REF[("ticks", seed)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_controller_drives_through_the_door(built_lib, seed):
    """Ticks are bounded by 1.5 times the CPU restatement's count for the seed (the noise streams differ, and the
    restatement's counts varied by a tenth across ten seeds)."""
    field, passable = door_esdf()
    m, _, togo = FC.door_model()
    res = field.follow(START, GOAL, 2, heading=(1.0, 0.0), robot_radius=0.08, K=256, T=32, seed=seed, max_ticks=300)
    want = reference_ticks(seed)
    print("seed", seed, {k: v for k, v in res.items() if k not in ("trace", "controls")}, "restatement ticks", want)
    assert res["goal_cell"] == [40, 8, 1] and res["start_cell"][:2] == [8, 30]
    assert res["reached"] and res["stops"] == 0 and res["ticks"] <= 1.5 * want
    assert res["trace"].shape == (res["ticks"] + 1, 4) and res["controls"].shape == (res["ticks"], 2)
    assert res["trace"].dtype == np.float32 and np.array_equal(res["trace"][0], np.array([0.4, 1.5, 1.0, 0.0], np.float32))
    for x, y in res["trace"][:, :2]:
        assert passable[tuple(R.nearest(m, x, y))]
    assert togo[tuple(R.nearest(m, *res["trace"][-1, :2]))] <= 2000
    assert res["min_clearance_m"] > 0.08 and 1.0 <= res["ess_min"] <= 256
    assert (res["controls"][:, 0] >= 0).all() and (res["controls"][:, 0] <= 0.5).all()
    assert (np.abs(res["controls"][:, 1]) <= 1.5).all()
    assert abs(float(np.float32(0.1) * res["controls"][:, 0].astype(np.float64).sum()) - res["length_m"]) < 1e-4


def test_controller_fields_steps_and_default_heading(built_lib):
    from go_slam_amd import _lib, follow
    field, passable = door_esdf()
    _, _, togo = FC.door_model()
    ctl = follow.Controller(field, GOAL, 2, START[2], 0.08, K=2048, T=32, seed=0)
    assert torch.equal(ctl.togo, gpu(togo))                                     # the field the restatement drives down
    state = [START[0], START[1], 1.0, 0.0]
    with _lib.kernel_timer(DEV) as timer:
        v, w, info = ctl.step(state)
        torch.cuda.synchronize()
    launched = timer.read()
    assert {k: launched[k][1] for k in ("follow_rollouts", "follow_weights", "follow_update")} == \
        {"follow_rollouts": 1, "follow_weights": 1, "follow_update": 1}
    assert 0 <= v <= 0.5 and abs(w) <= 1.5 and 1.0 <= info["ess"] <= 2048 and 0 <= info["hit_step"] <= 32
    same = follow.Controller(field, GOAL, 2, START[2], 0.08, K=2048, T=32, seed=0)
    assert same.step(state)[:2] == (v, w) and torch.equal(same.U, ctl.U)            # the same seed, the same bits
    res = field.follow(START, GOAL, 2, robot_radius=0.08, K=256, seed=0, max_ticks=300)     # heading down the route
    print("default heading", res["trace"][0, 2:].tolist(), "ticks", res["ticks"], "first step", (v, w, info))
    assert res["reached"] and res["stops"] == 0
    c, s = res["trace"][0, 2:]
    assert abs(c * c + s * s - 1) < 1e-6 and c > 0 and s <= 0                  # the route leaves toward the door


def test_unreachable_goal_launches_nothing_beyond_the_field(built_lib):
    from go_slam_amd import _lib
    field, _ = door_esdf(closed=True)
    with _lib.kernel_timer(DEV) as timer:
        res = field.follow(START, GOAL, 2, heading=(1.0, 0.0), robot_radius=0.08, K=256)
        torch.cuda.synchronize()
    launched = set(timer.read())
    assert res["reached"] is False and res["ticks"] == 0 and res["trace"].shape == (0, 4) and res["controls"].shape == (0, 2)
    assert res["stops"] == 0 and res["goal_cell"] == [40, 8, 1]
    assert not launched & {"follow_rollouts", "follow_weights", "follow_update"} and "geodesic_relax" in launched


# ---- whole run ------------------------------------------------------------------------------------------------------
def test_only_tracking_run_ends_with_a_follow_file(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import follow
    from go_slam_amd.slam import SLAM
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    plan_cfg = {"enable": True, "robot_radius": 0.2, "snap": 1.0, "allow_unknown": True, "goal": [0.6, 0.0, 0.3]}

    def cfg(plan_cfg):
        return {"enable": True, "source": "sensor", "voxel_size": 0.1,
                "esdf": {"enable": True, "max_distance": 1.0, "plan": plan_cfg}}
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    EG.TG.whole_run(with_dir, cfg({**plan_cfg, "follow": {"enable": True, "up_axis": 1, "K": 256, "max_ticks": 80}}))
    stats = returned[0]
    head, trace, controls = follow.parse_follow(open(f"{with_dir}/map/follow.txt").read())
    print("map/follow.txt:", head)
    assert stats["tsdf_follow_reached"] == head["reached"] and stats["tsdf_follow_ticks"] == head["ticks"]
    assert stats["tsdf_follow_min_clearance_m"] == head["min_clearance_m"] and head["n_states"] == len(trace)
    if stats["tsdf_path_reachable"]:
        assert head["n_states"] == head["ticks"] + 1 == len(controls) + 1 and 0 <= head["ticks"] <= 80
        assert (controls[:, 0] >= 0).all() and (controls[:, 0] <= 0.5).all() and (np.abs(controls[:, 1]) <= 1.5).all()
        assert head["min_clearance_m"] > 0.2 or head["ticks"] == head["stops"]
    else:
        assert head["reached"] is False and head["n_states"] == 0 and head["ticks"] == 0
    EG.TG.whole_run(without_dir, cfg(plan_cfg))
    assert not any(k.startswith("tsdf_follow") for k in returned[1])
    assert returned[1]["tsdf_path_length_m"] == stats["tsdf_path_length_m"]
    written = os.path.join("map", "follow.txt")
    listed = EG.TG.listing(with_dir)
    assert written in listed and [p for p in listed if p != written] == EG.TG.listing(without_dir)
    assert open(f"{with_dir}/map/path.txt").read() == open(f"{without_dir}/map/path.txt").read()
