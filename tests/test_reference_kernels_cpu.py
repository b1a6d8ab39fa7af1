"""oracle/droid_oracle.py against the REFERENCE's OWN tracking kernels.

`oracle/build_ref.py` compiles the reference's src/lib/{droid_kernels,correlation_kernels,altcorr_kernel}.cu + droid.cpp --
the CUDA extension `droid_backends` of the reference -- for the CPU (oracle/ref_build/cuda_on_cpu.h: the blocks of a
launch run one after the other, the threads of a block are cooperative fibers, __syncthreads() is a real barrier) into
oracle/_ref/.  What runs here is the reference's code, statement for statement, except: the launch syntax, six
warp-synchronous statements and five one-warp hand-over points (rewritten at build time, see build_ref.py) and the
linear solve (Eigen is an empty submodule of the reference: a dense double Cholesky stands in).

Every GPU parity test of the tracking path judges the HIP kernels against the oracle; these tests judge the oracle against
the code it restates.  Integer / index / fp16-order work is compared bit for bit; the reductions of the geometry and BA
kernels (fp32 block reductions in the kernel, fp64 sums in the oracle) to fp32 rounding.

The reference's sources are not part of this repository, so the module's results for exactly the calls made here are
stored in tests/golden/reference_kernels_cpu.npz and replayed (`Recorded`): every call is looked up by a digest of its
arguments.  Outputs that are compared bit for bit (EXACT) are stored as a digest of their dtype, shape and bytes and
compared with `same`; the others are stored whole, and only those a test reads.  Where oracle/_ref exists, every replayed
result is also checked against the live module.  After a change to these tests' inputs, rewrite the fixture where
oracle/_ref can be built:

    GS_RECORD_REFERENCE_KERNELS=1 python -m pytest tests/test_reference_kernels_cpu.py"""
import hashlib
import os

import numpy as np
import pytest
import torch

from go_slam_amd import synth
from oracle import droid_oracle as DO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_kernels_cpu.npz")
EXACT = ("corr_index_forward", "corr_index_backward", "projmap", "iproj", "depth_filter")    # compared bit for bit below


def digest(t):
    h = hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode())
    h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


class Digest:
    """A stored output of an EXACT kernel: its dtype and digest()."""

    def __init__(self, text):
        dtype, self.hex = text.split(":")
        self.dtype = getattr(torch, dtype[len("torch."):])


def same(a, b):
    """torch.equal, where either side may be a stored Digest"""
    if isinstance(b, Digest):
        a, b = b, a
    if isinstance(a, Digest):
        return torch.is_tensor(b) and b.dtype == a.dtype and digest(b) == a.hex
    return torch.equal(a, b)


class _Outputs(list):
    """The outputs of one call of the live module; remembers which of them the test read."""

    def __init__(self, items):
        super().__init__(items)
        self.read = set()

    def __getitem__(self, i):
        self.read.add(i)
        return super().__getitem__(i)

    def __iter__(self):
        self.read.update(range(len(self)))
        return super().__iter__()


class Recorded:
    """Stand-in for the reference module: R.<kernel>(*args) returns the stored outputs of that kernel on those arguments
    and writes the stored post-call values into the tensor arguments the kernel updates in place (ba: poses, disps)."""

    def __init__(self, live=None, record=False):
        self.live, self.record = live, record
        self.store = {} if record else dict(np.load(GOLDEN))
        self.calls = []         # live module: (name, key, outputs, updated arguments) of every call

    def stored(self, key, kind):
        """{index: tensor or Digest} of the stored `kind` entries (out / arg) of one call"""
        p = f"{key}/{kind}"
        return {int(k[len(p):]): Digest(str(v)) if v.dtype.kind == "U" else torch.from_numpy(np.array(v))
                for k, v in self.store.items() if k.startswith(p)}

    def __getattr__(self, name):
        def call(*args):
            h = hashlib.sha256(name.encode())
            for a in args:
                h.update((digest(a) if torch.is_tensor(a) else repr(a)).encode())
            key = f"{name}.{h.hexdigest()[:20]}"
            if self.live is None:
                assert f"{key}/n" in self.store, f"{key}: no stored result for these arguments (re-record the fixture)"
                for i, a in self.stored(key, "arg").items():
                    args[i].copy_(a)
                outs, n = self.stored(key, "out"), int(self.store[f"{key}/n"])
                return [outs.get(i) for i in range(n)] if n else outs[0]
            before = [a.clone() if torch.is_tensor(a) else None for a in args]
            out = getattr(self.live, name)(*args)
            outs = _Outputs([o.clone() if torch.is_tensor(o) else o for o in out]) if isinstance(out, (list, tuple)) else None
            updated = {i: a.clone() for i, (a, b) in enumerate(zip(args, before)) if b is not None and not torch.equal(a, b)}
            self.calls.append((name, key, out.clone() if outs is None else outs, updated))
            if not self.record:
                stored = self.stored(key, "arg")
                assert stored.keys() == updated.keys() and all(torch.equal(updated[i], a) for i, a in stored.items()), \
                    f"{key}: the live module's in-place results differ from the fixture"
                for i, s in self.stored(key, "out").items():
                    assert same(s, out if outs is None else list.__getitem__(outs, i)), f"{key}: output {i} differs"
            return out if outs is None else outs
        return call

    def finish(self):
        """record: store every call's updated arguments and the outputs the tests read; otherwise check that all of
        these are in the fixture"""
        for name, key, outs, updated in self.calls:
            single = not isinstance(outs, _Outputs)
            read = {0: outs} if single else {i: list.__getitem__(outs, i) for i in outs.read}
            entries = {f"{key}/out{i}": np.array(f"{o.dtype}:{digest(o)}") if name in EXACT else o.numpy()
                       for i, o in read.items() if o is not None}
            entries.update({f"{key}/arg{i}": a.numpy() for i, a in updated.items()})
            entries[f"{key}/n"] = np.array(0 if single else len(outs))
            if self.record:
                self.store.update(entries)
            else:
                missing = sorted(set(entries) - set(self.store))
                assert not missing, f"the tests read results the fixture does not hold (re-record it): {missing[:4]}"
        if self.record:
            np.savez_compressed(GOLDEN, **self.store)


@pytest.fixture(scope="module")
def R():
    """The stored results, checked against oracle/_ref when it exists (a failure to build or load it is not an error:
    the fixture is what the tests need)."""
    from oracle import build_ref
    record = os.environ.get("GS_RECORD_REFERENCE_KERNELS") == "1"
    live = None
    try:
        build_ref.build()
        live = build_ref.load()
    except Exception as exc:      # noqa: BLE001
        if record:
            raise
        print(f"oracle/_ref not usable here ({exc!r:.200}); replaying the stored fixture")
    if record and live is None:
        pytest.fail("GS_RECORD_REFERENCE_KERNELS=1 needs oracle/_ref")
    rec = Recorded(live, record)
    yield rec
    rec.finish()


def _coords(n, h1, w1, h2, w2, seed, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h1, dtype=torch.float32), torch.arange(w1, dtype=torch.float32), indexing="ij")
    c = torch.stack([xs * (w2 / w1), ys * (h2 / h1)], 0)[None].repeat(n, 1, 1, 1)
    c = c + spread * torch.randn(n, 2, h1, w1, generator=g)
    c[:, :, 0, 0] = torch.tensor([-20.0, 3.0])[None]          # fully outside
    c[:, :, 0, 1] = torch.tensor([2.0, 2.0])[None]            # exact integer (weights 0 / 1)
    c[:, :, 1, 0] = torch.tensor([w2 - 1.5, h2 - 0.5])[None]  # straddles the far border
    c[:, :, 1, 1] = torch.tensor([-0.25, -0.75])[None]        # straddles the near border
    return c.contiguous()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
def test_corr_index_forward_and_backward_bit_exact(R, dtype):
    """correlation_kernels.cu:19-118 (the lookup of every corr level, and its backward): per-dtype accumulation in the
    kernel's (i, j) order -- the oracle claims that order, so the results must be identical."""
    n, h1, w1, h2, w2 = 3, 8, 12, 8, 12
    g = torch.Generator().manual_seed(2)
    vol = torch.randn(n, h1, w1, h2, w2, generator=g).to(dtype)
    c = _coords(n, h1, w1, h2, w2, seed=3)
    ref, = R.corr_index_forward(vol, c, 3)
    out, = DO.corr_index_forward(vol, c, 3)
    assert ref.dtype == out.dtype == dtype and same(ref, out)
    grad = torch.randn(n, 7, 7, h1, w1, generator=g).to(dtype)
    ref, = R.corr_index_backward(vol, c, grad, 3)
    out, = DO.corr_index_backward(vol, c, grad, 3)
    assert same(ref, out)


def test_altcorr_forward_and_backward_fp32(R):
    """altcorr_kernel.cu:27-149,151-283 in fp32 -- the only precision the reference calls it with
    (src/modules/corr.py:123: `CorrLayer.apply(fmap1_i.float(), fmap2_i.float(), ...)`).  The kernel adds 32-channel
    partial dot products into the output one chunk at a time, the oracle sums all channels at once: fp32 rounding."""
    g = torch.Generator().manual_seed(5)
    B, S, C, H, W = 2, 3, 64, 8, 16
    f1, f2 = torch.randn(B, H, W, C, generator=g), torch.randn(B, H // 2, W // 2, C, generator=g)
    co = _coords(B * S, H, W, H // 2, W // 2, seed=6).view(B, S, 2, H, W).permute(0, 1, 3, 4, 2).contiguous()
    ref, = R.altcorr_forward(f1, f2, co, 3)
    out, = DO.altcorr_forward(f1, f2, co, 3)
    torch.testing.assert_close(ref, out, rtol=1e-5, atol=1e-5)
    grad = torch.randn(B, S, 49, H, W, generator=g)
    rb = R.altcorr_backward(f1, f2, co, grad, 3)
    ob = DO.altcorr_backward(f1, f2, co, grad, 3)
    torch.testing.assert_close(rb[0], ob[0], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(rb[1], ob[1], rtol=1e-5, atol=1e-5)
    assert not bool(rb[2].any())                               # the kernel never writes coords_grad


def test_geometry_kernels(R):
    """droid_kernels.cu: projmap (:430-515), iproj (:790-840), depth_filter (:662-787) bit for bit; frame_distance
    (:518-657) to the rounding of its fp32 block reduction."""
    vid = synth.make_video(8, "tiny", seed=7)
    ii, jj = synth.make_graph(8, 24, seed=7)
    ii = torch.cat([ii, torch.tensor([2, 5])])
    jj = torch.cat([jj, torch.tensor([2, 5])])                  # two i == j edges
    P, D, K = vid["poses"], vid["disps"], vid["intrinsics"][0].contiguous()
    rc, rv = R.projmap(P, D, K, ii, jj)
    oc, ov = DO.projmap(P, D, K, ii, jj)
    assert same(rc, oc) and same(rv, ov)
    assert same(R.iproj(P, D, K), DO.iproj(P, D, K))
    ix, th = torch.tensor([1, 3, 4, 6]), torch.tensor([0.05, 0.01, 0.2, 0.005])
    assert same(R.depth_filter(P, D, K, ix, th), DO.depth_filter(P, D, K, ix, th))
    for beta in (0.3, 0.7):
        torch.testing.assert_close(R.frame_distance(P, D, K, ii, jj, beta), DO.frame_distance(P, D, K, ii, jj, beta),
                                   rtol=2e-6, atol=1e-6)


def _ba_problem(num_kf, num_edges, seed, rgbd=True, noise=0.5, shape="tiny"):
    p = synth.make_ba_problem(num_kf, num_edges, shape, seed, rgbd)
    c, _ = DO.reproject(p["poses"], p["disps"], p["intrinsics"], p["ii"], p["jj"])
    return synth.make_ba_problem(num_kf, num_edges, shape, seed, rgbd, noise_px=noise, coords=c[0])


def _run_pair(R, prob, iters, lm, ep, motion_only):
    K = prob["intrinsics"][0].contiguous()
    out = []
    for fn in (R.ba, DO.ba):
        p, d = prob["poses"].clone(), prob["disps"].clone()
        res = fn(p, d, K, prob["disps_sens"], prob["target"], prob["weight"], prob["eta"], prob["ii"], prob["jj"],
                 prob["t0"], prob["t1"], iters, lm, ep, motion_only)
        out.append((res, p, d))
    return out


@pytest.mark.parametrize("rgbd", [True, False])
def test_ba_two_iterations(R, rgbd):
    """ba_cuda (droid_kernels.cu:1314-1434): projective_transform_kernel's Jacobians and per-edge Hessian blocks, the
    accumulation into the pose system, schur_block's E Q E^T / E Q w products, the damped solve, EvT6x1, pose and
    disparity retraction -- two Gauss-Newton iterations, with and without the RGB-D prior."""
    prob = _ba_problem(7, 18, seed=11, rgbd=rgbd)
    (rr, pr, dr), (ro, po, do) = _run_pair(R, prob, 2, 1e-4, 0.1, False)
    assert float((pr - prob["poses"]).abs().max()) > 1e-3 and float((dr - prob["disps"]).abs().max()) > 1e-3
    torch.testing.assert_close(rr[0], ro[0], rtol=1e-4, atol=1e-6)          # dx of the last iteration
    torch.testing.assert_close(rr[1], ro[1], rtol=1e-4, atol=2e-6)          # dz
    torch.testing.assert_close(pr, po, rtol=0, atol=2e-6)
    torch.testing.assert_close(dr, do, rtol=0, atol=2e-6)


def test_ba_motion_only_window_and_stereo_edges(R):
    """motion_only (no depth unknowns), and a window that starts at t0 = 3 with i == j stereo edges: frames before t0
    stay fixed, the stereo baseline replaces the relative pose (:219-229), and the depth back-substitution skips terms
    with pose index <= 0 (EvT6x1_kernel :1104: the quirk the HIP path mirrors)."""
    prob = _ba_problem(7, 18, seed=17)
    (rr, pr, dr), (ro, po, do) = _run_pair(R, prob, 2, 1e-4, 0.1, True)
    torch.testing.assert_close(rr[0], ro[0], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(pr, po, rtol=0, atol=2e-6)
    assert torch.equal(dr, prob["disps"]) and torch.equal(do, prob["disps"])
    prob = _ba_problem(9, 24, seed=19)
    prob["ii"] = torch.cat([prob["ii"], torch.tensor([3, 6])])
    prob["jj"] = torch.cat([prob["jj"], torch.tensor([3, 6])])
    g = torch.Generator().manual_seed(3)
    ht, wd, _ = synth.SHAPES["tiny"]
    prob["target"] = torch.cat([prob["target"], prob["target"][:2] + 0.1], 0).contiguous()
    prob["weight"] = torch.cat([prob["weight"], torch.rand(2, 2, ht, wd, generator=g)], 0).contiguous()
    prob["t0"], prob["t1"] = 3, 9
    kx = torch.unique(torch.cat([torch.arange(3, 9), prob["ii"]]))
    prob["eta"] = 1e-2 * torch.rand(len(kx), ht, wd, generator=g) + 1e-4
    (rr, pr, dr), (ro, po, do) = _run_pair(R, prob, 2, 1e-4, 0.1, False)
    torch.testing.assert_close(rr[0], ro[0], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(pr, po, rtol=0, atol=2e-6)
    torch.testing.assert_close(dr, do, rtol=0, atol=2e-6)
    assert torch.equal(pr[:3], prob["poses"][:3])


def test_ba_cholesky_failure_gives_zero_pose_update(R):
    """lm = -2, ep = -1 make the damped system indefinite: the reference returns dx = 0 (:1207-1210) and goes on with the
    depth update; the oracle (and the HIP path) must do the same."""
    prob = _ba_problem(6, 14, seed=23)
    (rr, pr, dr), (ro, po, do) = _run_pair(R, prob, 1, -2.0, -1.0, False)
    assert not bool(rr[0].any()) and not bool(ro[0].any())
    assert torch.equal(pr, prob["poses"]) and torch.equal(po, prob["poses"])
    torch.testing.assert_close(dr, do, rtol=0, atol=2e-6)


def test_ba_at_the_bench_window(R):
    """The frontend window bench.py times (BASELINE configs[1]: 60x80 maps, P = 25 keyframes, E = 75 edges, RGB-D): two
    Gauss-Newton iterations of the reference's ba_cuda (26 s on the CPU) vs the oracle, at SURVEY 8c's tolerance for `ba`
    (dx rtol 1e-4 / atol 1e-6).  tools/reference_kernels_at_bench_shape.py adds the monocular window (P = 50, E = 100)
    and the lookup / geometry kernels at S480 (profiles/r04_reference_kernels_parity.json)."""
    prob = _ba_problem(25, 75, seed=31, shape="S480")
    (rr, pr, dr), (ro, po, do) = _run_pair(R, prob, 2, 1e-4, 0.1, False)
    assert float((pr - prob["poses"]).abs().max()) > 1e-2
    torch.testing.assert_close(ro[0], rr[0], rtol=1e-4, atol=2e-6)
    torch.testing.assert_close(po, pr, rtol=0, atol=3e-6)
    torch.testing.assert_close(do, dr, rtol=0, atol=4e-6)



def test_seeded_random_windows_ba_geometry_lookup(R):
    """20 seeded random windows (the loop of tools/fuzz_oracle_vs_reference_kernels.py, whose round-4 run of 108 problems is
    the source of the bounds): 4-9 keyframes with 1-3 edges per keyframe on 12x16 maps -- RGB-D and monocular alternating,
    motion-only every fifth, a window start t0 > 1 every third, 0-2 px of target noise -- two Gauss-Newton iterations of the
    reference's `ba_cuda` vs the oracle's, `frame_distance`, `projmap` (bit for bit) and the fp16 lookup on pyramid sizes
    12x16 / 15x20 / 7x10 / 3x5 (bit for bit)."""
    worst = {}

    def upd(k, a, b):
        worst[k] = max(worst.get(k, 0.0), float((a.double() - b.double()).abs().max()))
    for seed in range(100, 120):
        g = torch.Generator().manual_seed(seed)
        nkf = int(torch.randint(4, 10, (1,), generator=g))
        ne = int(torch.randint(nkf, 3 * nkf, (1,), generator=g))
        rgbd = bool(seed % 2)
        p = synth.make_ba_problem(nkf, ne, "tiny", seed, rgbd)
        c, _ = DO.reproject(p["poses"], p["disps"], p["intrinsics"], p["ii"], p["jj"])
        p = synth.make_ba_problem(nkf, ne, "tiny", seed, rgbd, noise_px=float(torch.rand(1, generator=g)) * 2, coords=c[0])
        if seed % 3 == 0 and nkf > 5:
            p["t0"] = int(torch.randint(1, nkf - 2, (1,), generator=g))
            kx = torch.unique(torch.cat([torch.arange(p["t0"], p["t1"]), p["ii"]]))
            ht, wd, _ = synth.SHAPES["tiny"]
            p["eta"] = 1e-2 * torch.rand(len(kx), ht, wd, generator=g) + 1e-4
        mo = seed % 5 == 0
        (rr, pr, dr), (ro, po, do) = _run_pair(R, p, 2, 1e-4, 0.1, mo)
        upd("poses", po, pr); upd("disps", do, dr); upd("dx", ro[0], rr[0])
        if not mo:
            upd("dz", ro[1], rr[1])
        K = p["intrinsics"][0].contiguous()
        ii, jj = p["ii"], p["jj"]
        upd("frame_distance", DO.frame_distance(p["poses"], p["disps"], K, ii, jj, 0.3),
            R.frame_distance(p["poses"], p["disps"], K, ii, jj, 0.3))
        assert same(DO.projmap(p["poses"], p["disps"], K, ii, jj)[0], R.projmap(p["poses"], p["disps"], K, ii, jj)[0]), seed
        h2, w2 = [(7, 10), (3, 5), (15, 20), (12, 16)][seed % 4]
        vol = torch.randn(2, 6, 9, h2, w2, generator=g).half()
        ys, xs = torch.meshgrid(torch.arange(6.), torch.arange(9.), indexing="ij")
        co = (torch.stack([xs * w2 / 9, ys * h2 / 6], 0)[None].repeat(2, 1, 1, 1) + 3 * torch.randn(2, 2, 6, 9, generator=g)).contiguous()
        assert same(DO.corr_index_forward(vol, co, 3)[0], R.corr_index_forward(vol, co, 3)[0]), seed
    # round-4 run over 108 windows: poses 1.1e-6, dx 9.8e-7, disparities / dz 1.6e-5, frame_distance 1.2e-7
    assert worst["poses"] <= 3e-6 and worst["dx"] <= 3e-6 and worst["disps"] <= 4e-5 and worst["dz"] <= 4e-5, worst
    assert worst["frame_distance"] <= 1e-6, worst
