"""droid_backends.ba (go_slam_amd/csrc/ba.hip) against the fp64 Gauss-Newton step of tests/ba_restatement.py, which is
derived from the residual by autograd and shares no Jacobian formula with the kernel or with oracle/.

Every case runs ONE iteration (one assembled system; "17x19-mix-2it" runs two) at two damping levels: production
(lm 1e-4, ep 0.1) and a probe whose ep is 10^3 x the largest diagonal entry of the undamped fp64 system, so that the solve
has condition number ~1 (dx ~ b / ep) and the rounding of the assembled system is seen unamplified.

Metric: err(x) = max|x - x64| / max|x64| for dx and for dz.  Bound: err_gpu <= 4 max(err_oracle32, 2^-20), err_oracle32
being the same figure of the fp32 CPU oracle (oracle.droid_oracle.ba) on the same inputs, computed in the same test run;
the 4 is for the different order of the fp32 sums.  dx must also meet tests/test_track_gpu.py's rtol 1e-4 / atol 1e-6
against the fp64 step.  tests/test_ba_restatement_cpu.py shows that subtly wrong steps miss this bound 2e3 .. 2e5 times.

Cases (tests/ba_restatement.py: case): a 35-pixel map (a lone partial 256-lane chunk), 323 pixels (a full chunk and a ragged
one), 1221 pixels (a full 4 x 256 Schur trip and a partial one); sensor depth on part of every keyframe, none, motion-only;
54 edges on 9 depth rows (E = 6 M: the split accumulation) with out-degrees 0, 1, 2, 3, 5, 9, 11, 11, 12, stereo edges, a
source before the window and targets outside it; 30 of those edges (unsplit) and the same 30 padded with 24 zero-weight
edges (split) against ONE fp64 step; 1030 frames with the window at [1000, 1012) (the frame scan of the table kernel takes
two frames per thread).  Each case asserts on the CPU that no edge pixel's fp64 depth lies within 1e-4 of the z < 0.25 mask
and that at least 2% lie behind it.

Update stage, from the kernel's OWN dx and dz (conditioning does not enter): poses[t0:t1] equal the fp64 retraction of the
input poses by dx to 8 fp32 ulps of the largest pose component; disps[kx] equal disps_in[kx] + dz bit for bit; every other
frame and row is bit-identical to the input.  Three more problems scale a uniform target offset so that the rotations of dx
are ~1e-6, ~5e-5 (Taylor quaternion, translation without rotational terms: below theta^2 = 1e-8 and theta = 1e-4) and ~1e-3
(sinf / cosf and the rotational terms).

Measured on an MI355X (bound = 4 max(err_oracle32, 9.5e-7)); the retractions were within 1.5 ulp:

    case                damping      dx: err_gpu  err_oracle32  bound       dz: err_gpu  err_oracle32  bound
    5x7-mix             production   9.51e-07     1.15e-06      4.62e-06    1.07e-06     1.07e-06      4.26e-06
    5x7-mix             probe        6.93e-07     6.89e-07      3.81e-06    1.12e-06     1.12e-06      4.46e-06
    17x19-mono          production   1.44e-05     1.45e-05      5.80e-05    9.06e-07     8.85e-07      3.81e-06
    17x19-mono          probe        1.39e-05     1.40e-05      5.59e-05    9.41e-07     9.41e-07      3.81e-06
    33x37-mix           production   1.97e-05     1.84e-05      7.34e-05    4.23e-06     4.23e-06      1.69e-05
    33x37-mix           probe        3.17e-05     3.19e-05      1.27e-04    4.80e-06     4.80e-06      1.92e-05
    17x19-motion        production   3.89e-06     3.76e-06      1.50e-05    -            -             -
    17x19-motion        probe        2.25e-05     2.25e-05      9.01e-05    -            -             -
    17x19-mix-2it       production   4.04e-05     3.29e-05      1.32e-04    2.76e-06     2.62e-06      1.05e-05
    17x19-mix-2it       probe        7.49e-06     7.49e-06      2.99e-05    2.27e-06     2.27e-06      9.08e-06
    long-lists          production   9.48e-06     9.63e-06      3.85e-05    1.95e-06     1.96e-06      7.86e-06
    long-lists          probe        9.96e-06     1.01e-05      4.05e-05    1.89e-06     1.89e-06      7.56e-06
    short-lists         production   2.72e-06     2.51e-06      1.01e-05    1.22e-06     1.20e-06      4.80e-06
    short-lists         probe        5.07e-06     5.13e-06      2.05e-05    1.20e-06     1.18e-06      4.73e-06
    short-lists-padded  production   2.41e-06     2.51e-06      1.01e-05    1.20e-06     1.20e-06      4.80e-06
    short-lists-padded  probe        5.08e-06     5.13e-06      2.05e-05    1.18e-06     1.18e-06      4.73e-06
    1030-frames         production   1.77e-06     1.62e-06      6.47e-06    4.92e-07     4.92e-07      3.81e-06
    1030-frames         probe        1.36e-06     1.35e-06      5.42e-06    5.33e-07     5.33e-07      3.81e-06
"""
import functools

import numpy as np
import pytest
import torch

import ba_restatement as R

pytestmark = pytest.mark.gpu

DAMPINGS = ("production", "probe")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def db(built_lib):
    from go_slam_amd import droid_backends
    return droid_backends


@functools.lru_cache(maxsize=None)
def _oracle32(name, damping):
    """(dx, dz) of the fp32 CPU oracle on the case's own inputs."""
    from oracle import droid_oracle as O
    prob, motion_only, iters = R.case(name)
    _, lm, ep = R.reference(name, damping)
    return O.ba(prob["poses"].clone(), prob["disps"].clone(), prob["intrinsics"], prob["disps_sens"], prob["target"],
                prob["weight"], prob["eta"], prob["ii"], prob["jj"], prob["t0"], prob["t1"], iters, lm, ep, motion_only)


def _run(db, dev, prob, iters, lm, ep, motion_only):
    pg, dg = prob["poses"].clone().to(dev), prob["disps"].clone().to(dev)
    dx, dz = db.ba(pg, dg, prob["intrinsics"].to(dev), prob["disps_sens"].to(dev), prob["target"].to(dev),
                   prob["weight"].to(dev), prob["eta"].to(dev), prob["ii"].to(dev), prob["jj"].to(dev), prob["t0"],
                   prob["t1"], iters, lm, ep, motion_only)
    status = db.ba_status(dev)
    assert status == {"depth_keyframes": prob["eta"].shape[0], "depth_rows_mismatch": False, "cholesky_failures": 0}
    return dx.cpu(), None if dz is None else dz.cpu(), pg.cpu(), dg.cpu()


def _check_update_stage(prob, dx, dz, poses_out, disps_out, retraction=True):
    t0, t1 = prob["t0"], prob["t1"]
    kx = R.depth_rows(prob["ii"], t0, t1)
    outside = torch.ones(prob["poses"].shape[0], dtype=torch.bool)
    outside[t0:t1] = False
    assert torch.equal(poses_out[outside], prob["poses"][outside]), "a pose outside the window moved"
    rest = torch.ones(prob["disps"].shape[0], dtype=torch.bool)
    if dz is not None:
        rest[kx] = False
    assert torch.equal(disps_out[rest], prob["disps"][rest]), "a disparity row outside kx changed"
    if not retraction:
        return
    want = R.retract(dx, prob["poses"][t0:t1])
    ulp = float(np.spacing(np.float32(poses_out[t0:t1].abs().max())))
    worst = float((poses_out[t0:t1].double() - want).abs().max())
    print(f"    retraction: max |pose - fp64| = {worst:.2e} = {worst / ulp:.2f} ulp of the largest component")
    assert worst <= 8 * ulp
    if dz is not None:
        assert torch.equal(disps_out[kx], prob["disps"][kx] + dz.view(-1, *prob["disps"].shape[1:]))


@pytest.mark.parametrize("damping", DAMPINGS)
@pytest.mark.parametrize("name", R.CASES)
def test_ba_step_matches_the_derived_fp64_step(db, dev, name, damping):
    prob, motion_only, iters = R.case(name)
    ref, lm, ep = R.reference(name, damping)
    frac = R.check_inputs(ref["z"])
    dx, dz, pg, dg = _run(db, dev, prob, iters, lm, ep, motion_only)
    odx, odz = _oracle32(name, damping)
    figures = [("dx", R.err(dx, ref["dx"]), R.err(odx, ref["dx"]))]
    if not motion_only:
        figures.append(("dz", R.err(dz, ref["dz"]), R.err(odz, ref["dz"])))
    print(f"\n{name} {damping}: ep {ep:.4g}, {100 * frac:.1f}% of the edge pixels masked; "
          + "; ".join(f"{k}: err_gpu {g:.2e} err_oracle32 {o:.2e} bound {R.bound(o):.2e}" for k, g, o in figures))
    for k, g, o in figures:
        assert g <= R.bound(o), f"{k}: err_gpu {g:.3e} > 4 max(err_oracle32 {o:.3e}, 2^-20)"
    torch.testing.assert_close(dx.double(), ref["dx"], rtol=1e-4, atol=1e-6)
    if motion_only:
        assert dz is None
    _check_update_stage(prob, dx, dz, pg, dg, retraction=(iters == 1))
    if iters > 1:        # (the first iteration's dx is not returned: the end state against the fp64 end state instead)
        torch.testing.assert_close(pg.double(), ref["poses"], rtol=0, atol=1e-5)
        torch.testing.assert_close(dg.double(), ref["disps"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("theta", R.SMALL_ANGLE_TARGETS)
def test_retraction_on_both_sides_of_the_small_angle_thresholds(db, dev, theta):
    prob, ref = R.small_angle_case(theta)
    R.check_inputs(ref["z"])
    th64 = ref["dx"][:, 3:].norm(dim=-1)
    assert 0.9 * theta < float(th64.max()) < 1.1 * theta
    dx, dz, pg, dg = _run(db, dev, prob, 1, 1e-4, 0.1, False)
    th2 = (dx[:, 3:] * dx[:, 3:]).sum(-1)                       # fp32, as the kernel forms it
    print(f"\ntheta {theta:g}: rotation norms of the kernel's dx {[f'{t:.2e}' for t in th2.sqrt().tolist()]}")
    if theta < 1e-4:
        assert bool((th64 < 0.7e-4).all()) and bool((th2 < 0.5e-8).all()) and bool((th2.sqrt() < 0.7e-4).all())
    else:
        assert int((th64 > 2e-4).sum()) >= 4 and int(((th2 > 4e-8) & (th2.sqrt() > 2e-4)).sum()) >= 4
    _check_update_stage(prob, dx, dz, pg, dg)
