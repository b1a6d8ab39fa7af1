"""SURVEY 8b Boundary 4 -- the `src/slam.py` import contract.

1. `go_slam_amd.dropin.install()` makes the reference tree's native imports -- `droid_backends`, `tinycudann`,
   `lietorch`, `torch_scatter` -- resolve to this package, and the `droid_backends` substitute exposes every function of
   the reference's extension (src/lib/droid.cpp:237-250).
2. This package's mirrors take the constructor signatures slam.py uses (same parameter names as the reference's
   classes), so swapping the sibling imports needs no call-site edits.  The reference's signatures are
   stored in tests/golden/reference_signatures.json (tests/golden/gen_golden.py::gen_signatures).
"""
import importlib
import inspect
import json
import os
import sys
import types

import pytest

SIGNATURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_signatures.json")


def test_dropin_installs_the_substitutes():
    import go_slam_amd.dropin as dropin
    import go_slam_amd.droid_backends as db
    from go_slam_amd import lietorch_shim
    from go_slam_amd.neus import tcnn_compat
    saved = dict(sys.modules)
    try:
        dropin.install()
        assert sys.modules["droid_backends"] is db and sys.modules["tinycudann"] is tcnn_compat
        assert sys.modules["lietorch"] is lietorch_shim
        assert callable(sys.modules["torch_scatter"].scatter_mean)
    finally:
        for k in [k for k in sys.modules if k not in saved]:
            del sys.modules[k]
    for name in ("ba", "frame_distance", "projmap", "depth_filter", "iproj", "corr_index_forward",
                 "corr_index_backward", "altcorr_forward", "altcorr_backward"):         # src/lib/droid.cpp:237-250
        assert callable(getattr(db, name)), name


def _cfg():
    return {"mode": "rgbd", "cam": {"H_out": 64, "W_out": 96}, "tracking": {"buffer": 12}}


MIRRORS = {  # reference module -> (class, this package's module)
    "src.depth_video": ("DepthVideo", "go_slam_amd.depth_video"),
    "src.factor_graph": ("FactorGraph", "go_slam_amd.factor_graph"),
    "src.frontend": ("Frontend", "go_slam_amd.frontend"),
    "src.backend": ("Backend", "go_slam_amd.backend"),
    "src.motion_filter": ("MotionFilter", "go_slam_amd.motion_filter"),
    "src.multiview_filter": ("MultiviewFilter", "go_slam_amd.multiview_filter"),
    "src.trajectory_filler": ("PoseTrajectoryFiller", "go_slam_amd.trajectory_filler"),
    "src.droid_net": ("DroidNet", "go_slam_amd.droid_net"),
    "src.InstantNeuS": ("InstantNeuS", "go_slam_amd.neus.instant_neus"),
}


@pytest.mark.parametrize("ref_mod", sorted(MIRRORS))
def test_mirror_constructors_accept_the_reference_call(ref_mod):
    """every positional / keyword argument the reference class takes is accepted, in the same position, by the mirror"""
    cls, mine = MIRRORS[ref_mod]
    with open(SIGNATURES) as f:
        rp = [types.SimpleNamespace(name=n, kind=getattr(inspect.Parameter, k), default=None if d else inspect.Parameter.empty)
              for n, k, d in json.load(f)[ref_mod]]
    m = getattr(importlib.import_module(mine), cls)
    mp = [p for p in inspect.signature(m.__init__).parameters.values() if p.name != "self"]
    if cls == "DepthVideo":                       # one polymorphic constructor: (cfg, args) or (h8, w8, ...)
        assert len(rp) == 2 and len(mp) >= 2
        v = m(_cfg(), types.SimpleNamespace(device="cpu"))
        assert v.ht == 64 and v.wd == 96 and tuple(v.disps.shape) == (12, 8, 12) and hasattr(v.counter, "value")
        return
    has_var_kw = any(p.kind is inspect.Parameter.VAR_KEYWORD for p in mp)
    mnames = [p.name for p in mp]
    for i, p in enumerate(rp):
        if p.kind in (inspect.Parameter.VAR_POSITIONAL, inspect.Parameter.VAR_KEYWORD):
            continue
        assert p.name in mnames or has_var_kw, f"{cls}: the mirror lacks parameter `{p.name}`"
        if p.default is inspect.Parameter.empty and p.name in mnames:
            assert mnames.index(p.name) == i, f"{cls}: positional parameter `{p.name}` is at a different position"
