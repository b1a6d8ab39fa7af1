"""droid_backends.reproject / projmap / frame_distance / iproj / depth_filter (go_slam_amd/csrc/geom.hip, geom_common.h)
against the fp64 matrix model of tests/geom_restatement.py, which shares no formula with the kernels or with oracle/; and
the update step's glue kernels gs_motion_features / gs_ba_inputs (gru_gates.hip) and the motion features of
gs_lowmem_gather (lowmem_glue.hip) against the torch expressions they replace, bit for bit.

Cases (geom_restatement.case): maps of 35, 323 and 851 pixels (a lone partial 256-lane chunk; a full one and a ragged one;
three full and a ragged one, so four trips of frame_distance's loop and blockIdx.x > 0 in the other kernels); 10 frames, all
90 ordered pairs as edges and, for reproject, the 10 stereo edges; a frame turned 2.5 rad, one turned exactly pi (scalar part
~0), one quaternion stored negated; a distinct intrinsics row per frame for reproject; disparities log-uniform in [0.05, 4]
with exact zeros (a third of the projected points lie below Z = 0.1, hundreds between the cut-offs 0.1, 0.2 and 0.25);
depth_filter on noisy renderings of a wall and a floor, counts 0 to 6, at frames 0, 1, 4, 8, 9 of 10.

Metric: err(x) = max over unexcluded elements of |x - x64| / max(1, |x64|).  Bound: err_gpu <= 4 max(err_oracle32, 2^-20),
err_oracle32 being the same figure of the fp32 CPU oracle on the same inputs in the same run.  Exact, on every element
outside the model's ambiguity band (at most 1 % of a case): reproject's and projmap's valid, projmap's identity fallback
and zero third channel, depth_filter's counts, which edges of frame_distance return 1000.0.
tests/test_geom_restatement_cpu.py shows that eleven subtly wrong models miss these checks.

Measured on an MI355X (bound = 4 max(err_oracle32, 9.5e-7)).  The rerun with the negated quaternion stored un-negated
gave the same figures to the digits shown; the known answer at exactly 75 % valid came out 3.7e-8 from its fp64 value.

    case   check               err_gpu   err_oracle32  bound
    5x7    reproject coords    1.83e-06  1.83e-06      7.33e-06
    5x7    projmap coords      4.68e-06  4.68e-06      1.87e-05
    5x7    iproj               2.50e-07  2.50e-07      3.81e-06
    5x7    frame_distance 0.3  2.10e-07  1.39e-07      3.81e-06
    5x7    frame_distance 0.7  2.02e-07  1.26e-07      3.81e-06
    17x19  reproject coords    7.09e-06  7.09e-06      2.84e-05
    17x19  projmap coords      5.13e-05  5.13e-05      2.05e-04
    17x19  iproj               1.42e-06  1.42e-06      5.67e-06
    17x19  frame_distance 0.3  1.40e-07  1.27e-07      3.81e-06
    17x19  frame_distance 0.7  2.19e-07  1.44e-07      3.81e-06
    23x37  reproject coords    1.56e-05  1.56e-05      6.24e-05
    23x37  projmap coords      7.36e-05  7.36e-05      2.95e-04
    23x37  iproj               1.02e-06  1.02e-06      4.08e-06
    23x37  frame_distance 0.3  1.67e-07  1.27e-07      3.81e-06
    23x37  frame_distance 0.7  1.90e-07  1.34e-07      3.81e-06

The per-pixel kernels sit exactly on the oracle's figure (they round op by op like it); reproject divides by Z down to
0.1 and projmap by Z down to 0.01, which is what amplifies the rounding of Z in their figures.  frame_distance sums in fp32
in the kernel and in fp64 in the oracle.
"""
import pytest
import torch

import geom_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def db(built_lib):
    from go_slam_amd import droid_backends
    return droid_backends


_ORACLE = {}


def _oracle32(name):
    from oracle import droid_oracle as O
    if name not in _ORACLE:
        _ORACLE[name] = R.compare(R.run_all(O, R.case(name)), R.reference(name))
    return _ORACLE[name]


def _check(tag, got, name):
    ref = R.reference(name)
    for k, v in R.ambiguity_shares(ref).items():
        assert v <= R.AMBIGUITY_CAP, f"{k}: {100 * v:.2f}% of the results are ambiguous"
    unequal, errs = R.compare(got, ref)
    unequal_o, errs_o = _oracle32(name)
    print(f"\n{tag}:")
    for k in errs:
        print(f"    {k:20s} err_gpu {errs[k]:.2e}  err_oracle32 {errs_o[k]:.2e}  bound {R.bound(errs_o[k]):.2e}")
    assert all(v == 0 for v in unequal_o.values()), f"the oracle differs from the model: {unequal_o}"
    assert all(v == 0 for v in unequal.values()), f"unequal results outside the ambiguity band: {unequal}"
    for k in errs:
        assert errs[k] <= R.bound(errs_o[k]), f"{k}: err_gpu {errs[k]:.3e} > 4 max(err_oracle32 {errs_o[k]:.3e}, 2^-20)"


@pytest.mark.parametrize("name", R.CASES)
def test_kernels_match_the_fp64_model(db, dev, name):
    _check(name, R.run_all(db, R.case(name), dev), name)


@pytest.mark.parametrize("name", R.CASES)
def test_negated_quaternion_is_the_same_rotation(db, dev, name):
    c = dict(R.case(name))
    assert not torch.equal(c["poses"], c["poses_plain"])
    c["poses"] = c["poses_plain"]
    _check(f"{name} plain", R.run_all(db, c, dev), name)


def test_frame_distance_known_answer_at_exactly_75_percent(db, dev):
    ht, wd = R.KAT_HW
    k = R.frame_distance_kat()
    assert (ht, wd) == (16, 20) and k["share"] == 0.75
    args = lambda k: [k[n].to(dev) for n in ("poses", "disps", "intrinsics", "ii", "jj")] + [k["beta"]]   # noqa: E731
    out = float(db.frame_distance(*args(k)))
    print(f"\nexactly 75% valid: {out!r}, fp64 {k['answer']!r}, err {abs(out - k['answer']) / k['answer']:.2e}")
    assert out != R.FAR and abs(out - k["answer"]) <= R.bound(0.0) * k["answer"]
    k1 = R.frame_distance_kat(extra_far_pixels=1)
    assert k1["share"] == 0.75 - 1.0 / (ht * wd)
    assert float(db.frame_distance(*args(k1))) == R.FAR


def test_depth_filter_buffer_ends(db, dev):
    """Frames 0 and num-1 have only their three in-range neighbours (+3, +4, +5 and -1, -2, -3): their counts are those
    of a buffer cut down to the frame and those neighbours.  A one-frame buffer has no neighbour at all."""
    d = R.case("17x19")["df"]
    P, D, K = d["poses"].to(dev), d["disps"].to(dev), d["intrinsics"].to(dev)
    num = D.shape[0]
    th = torch.tensor([0.1, 0.1], device=dev)
    ends = db.depth_filter(P, D, K, torch.tensor([0, num - 1], device=dev), th).cpu()
    model = R.depth_filter(d["poses"], d["disps"], d["intrinsics"], torch.tensor([0, num - 1]), th.cpu())
    assert torch.equal(ends.double()[~model["amb"]], model["count"][~model["amb"]])
    assert 1 <= float(ends[0].max()) <= 3 and 1 <= float(ends[1].max()) <= 3
    head = db.depth_filter(P[:6].contiguous(), D[:6].contiguous(), K, torch.tensor([0], device=dev), th[:1]).cpu()
    tail = db.depth_filter(P[num - 4:].contiguous(), D[num - 4:].contiguous(), K, torch.tensor([3], device=dev), th[:1]).cpu()
    assert torch.equal(head[0], ends[0]) and torch.equal(tail[0], ends[1])
    # with every neighbour in range the same pixels collect more votes somewhere
    mid = db.depth_filter(P, D, K, torch.tensor([4], device=dev), th[:1]).cpu()
    assert float(mid.max()) > 3
    one = db.depth_filter(P[:1].contiguous(), D[:1].contiguous(), K, torch.tensor([0], device=dev), th[:1]).cpu()
    assert one.shape == (1,) + tuple(D.shape[1:]) and not bool(one.any())


# --------------------------------------------------------------------------------------------------- glue kernels ----
def _same_bits(got, want):
    """Equal bit for bit, a NaN standing for any NaN."""
    assert got.shape == want.shape and got.dtype == want.dtype
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "NaN in other places than the reference's"
    ints = {2: torch.int16, 4: torch.int32}[got.element_size()]
    return torch.equal(got.contiguous().view(ints)[~nan], want.contiguous().view(ints)[~nan])


def test_motion_features_equal_the_torch_expression_bit_for_bit(built_lib, dev):
    from go_slam_amd import _lib
    g = R.glue_case()
    E, ht, wd = R.GLUE_SHAPE
    want = R.motion_features_reference(g["coords0"], g["coords1"], g["target"])
    assert int(torch.isnan(want).sum()) >= 6 and int((want.float().abs() == 64).sum()) >= 8
    c1, tg = g["coords1"].to(dev), g["target"].to(dev)
    m4 = torch.empty(E, ht, wd, 4, dtype=torch.float16, device=dev)
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    _lib.check(L.gs_motion_features(_lib.ptr(c1), _lib.ptr(tg), _lib.ptr(m4), E, ht, wd, st), "motion_features")
    assert _same_bits(m4.permute(0, 3, 1, 2).cpu(), want)
    # the chunked update's gather carries the same arithmetic (its state rows are not under test here)
    sel = torch.tensor([2, 0, 1], device=dev)
    net = torch.zeros(E, ht, wd, 128, dtype=torch.float16, device=dev)
    c_out = torch.empty(E, ht, wd, 2, device=dev)
    m4g = torch.empty(E, ht, wd, 4, dtype=torch.float16, device=dev)
    net_out = torch.empty_like(net)
    _lib.check(L.gs_lowmem_gather(_lib.ptr(c1), _lib.ptr(tg), _lib.ptr(net), _lib.ptr(sel), _lib.ptr(c_out),
                                  _lib.ptr(m4g), _lib.ptr(net_out), E, ht, wd, st), "lowmem_gather")
    assert _same_bits(m4g.permute(0, 3, 1, 2).cpu(), want[sel.cpu()])
    assert _same_bits(c_out.cpu(), g["coords1"][sel.cpu()])


def test_ba_inputs_equal_the_torch_expression_bit_for_bit(built_lib, dev):
    from go_slam_amd import _lib
    g = R.glue_case()
    E, ht, wd = R.GLUE_SHAPE
    want_t, want_bt, want_bw = R.ba_inputs_reference(g["coords1"], g["delta"], g["weight"])
    c1, dl, wt = g["coords1"].to(dev), g["delta"].to(dev), g["weight"].to(dev)
    # the BA operands are written behind rows that belong to other edges: those must stay as they are
    pad = 2
    bt = torch.full((pad + E, 2, ht, wd), -7.0, device=dev)
    bw = torch.full((pad + E, 2, ht, wd), -7.0, device=dev)
    target = torch.empty_like(c1)
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    _lib.check(L.gs_ba_inputs(_lib.ptr(c1), _lib.ptr(dl), _lib.ptr(wt), _lib.ptr(target), bt[pad:].data_ptr(),
                              bw[pad:].data_ptr(), E, ht, wd, st), "ba_inputs")
    assert _same_bits(target.cpu(), want_t)
    assert _same_bits(bt[pad:].cpu(), want_bt) and _same_bits(bw[pad:].cpu(), want_bw)
    assert bool((bt[:pad] == -7.0).all()) and bool((bw[:pad] == -7.0).all())
