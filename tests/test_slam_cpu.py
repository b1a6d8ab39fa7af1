"""go_slam_amd.config and the host side of go_slam_amd.slam against what the reference's own code returned
(tests/golden/slam.json, written by tests/golden/gen_golden_slam.py): config loading, update_cam, constructor
signatures, and the call order of SLAM.run with the workers replaced by recorders.  No GPU."""
import inspect
import json
import os
import types

import pytest
import torch

from go_slam_amd import config

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DEFAULT = os.path.join(GOLDEN, "configs", "go_slam.yaml")
REPLICA = os.path.join(GOLDEN, "configs", "Replica", "replica.yaml")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "slam.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def slam_mod(built_lib):
    from go_slam_amd import slam
    return slam


# ---- config -------------------------------------------------------------------------------------------------------
def test_load_config_reproduces_the_reference(golden):
    assert config.load_config(DEFAULT) == golden["load_config"]["default_alone"]
    assert config.load_config(REPLICA, DEFAULT) == golden["load_config"]["replica_over_default"]


def _place_chain(golden, tmp_path):
    import shutil
    shutil.copytree(os.path.join(GOLDEN, "configs"), tmp_path / "configs")
    for name, text in golden["chain_files"].items():
        (tmp_path / name).write_text(text.replace("{dir}", str(tmp_path)))
    return str(tmp_path / "top.yaml"), str(tmp_path / "configs" / "go_slam.yaml")


def test_load_config_follows_a_three_deep_chain(golden, tmp_path):
    top, default = _place_chain(golden, tmp_path)
    cfg = config.load_config(top, default)
    cfg["inherit_from"] = cfg["inherit_from"].replace(str(tmp_path), "{dir}")
    want = golden["load_config"]["three_deep_chain"]
    assert cfg == want
    # the chain's own overrides, from the nearest file; a list replaces, it does not merge
    assert cfg["tracking"]["frontend"]["window"] == 9 and cfg["tracking"]["buffer"] == 96
    assert cfg["mapping"]["bound"] == [[-1, 1], [-2, 2], [-3, 3]]
    assert cfg["tracking"]["warmup"] == 12 and cfg["mapping"]["pixels"] == 4400      # replica.yaml, go_slam.yaml


def test_save_then_load_round_trips(golden, tmp_path):
    top, default = _place_chain(golden, tmp_path)
    cfg = config.load_config(top, default)
    del cfg["inherit_from"]
    config.save_config(cfg, str(tmp_path / "cfg.yaml"))
    assert config.load_config(str(tmp_path / "cfg.yaml")) == cfg


def test_update_recursive_semantics():
    d1 = {"a": {"x": 1, "y": [1, 2]}, "b": 3}
    config.update_recursive(d1, {"a": {"y": [9], "z": {"deep": True}}, "b": 4, "c": {"n": 1}})
    assert d1 == {"a": {"x": 1, "y": [9], "z": {"deep": True}}, "b": 4, "c": {"n": 1}}


# ---- SLAM's host side ---------------------------------------------------------------------------------------------
def test_update_cam_equals_the_reference_exactly(golden, slam_mod):
    assert len(golden["update_cam"]) == 3
    for name, case in golden["update_cam"].items():
        holder = types.SimpleNamespace()
        slam_mod.SLAM.update_cam(holder, {"cam": case["cam"]})
        got = {k: getattr(holder, k) for k in ("fx", "fy", "cx", "cy", "H", "W")}
        assert got == case["result"], name           # the same fp64 Python arithmetic: equal, not close


def test_constructors_accept_the_reference_call(golden, slam_mod):
    for cls, want in golden["signatures"].items():
        sig = inspect.signature(getattr(slam_mod, cls).__init__)
        params = [p for p in sig.parameters.values() if p.name != "self"]
        required = [[p.name, p.kind.name] for p in params if p.default is inspect.Parameter.empty]
        assert required == [[n, k] for n, k, has_default in want if not has_default], cls
        sig.bind(None, *[object() for n, k, d in want])                       # the reference's positional call
        sig.bind(None, **{n: object() for n, k, d in want})                   # and by name
    doc = slam_mod.SLAM.__init__.__doc__
    assert "full_ba_every" in doc and "schedule choice" in doc and "not a measured number" in doc


class _Recorder:
    def __init__(self, log, name, effect=None):
        self.log, self.name, self.effect = log, name, effect

    def __call__(self, *args, **kwargs):
        self.log.append((self.name, args, kwargs))
        if self.effect:
            self.effect(*args, **kwargs)


def _recorded_slam(slam_mod, mode="rgbd", only_tracking=False, make_video=False, keyframes=(0, 1, 2, 4, 5, 6),
                   full_ba_every=2, post=3):
    """a SLAM whose workers only write down their calls; the recorded tracker promotes the frames of `keyframes`"""
    s = object.__new__(slam_mod.SLAM)
    log = []
    s.mode, s.only_tracking, s.make_video, s.full_ba_every = mode, only_tracking, make_video, full_ba_every
    s.post_processing_iters = post
    for name in slam_mod.FLAGS:
        setattr(s, name, torch.zeros(1).int())
    s.video = types.SimpleNamespace(counter=types.SimpleNamespace(value=0))

    def promote(timestamp, *rest):
        if timestamp in keyframes:
            s.video.counter.value += 1
    s.tracker = _Recorder(log, "tracker", promote)
    for name in ("ba", "multiview_filter", "mapper", "mesher"):
        setattr(s, name, _Recorder(log, name))
    return s, log


def _stream(n=7):
    return [(i, torch.zeros(1, 3, 8, 8), torch.ones(8, 8), torch.ones(4), torch.eye(4)) for i in range(n)]


def test_run_issues_the_documented_call_order(slam_mod):
    s, log = _recorded_slam(slam_mod)
    s.run(_stream(7))
    names = [n for n, _, _ in log]
    kf = ["tracker", "multiview_filter", "mapper"]
    want = (kf + kf + ["ba"]            # frames 0, 1: keyframes; the 2nd new keyframe brings the full BA
            + kf + ["tracker"]          # frame 2 a keyframe, frame 3 not: tracker only
            + kf + ["ba"]               # frame 4: the 4th keyframe
            + kf + kf + ["ba"]          # frames 5, 6
            + ["ba", "multiview_filter"] + ["mapper"] * 3)      # after the stream
    assert names == want
    assert [a[0] for n, a, _ in log if n == "tracker"] == list(range(7))
    assert all(a[2] is not None for n, a, _ in log if n == "tracker")          # rgbd: the depth goes through
    mapper_calls = [k for n, _, k in log if n == "mapper"]
    assert mapper_calls[:6] == [{}] * 6 and mapper_calls[6:] == [{"the_end": True}] * 3
    for flag in ("tracking_finished", "optimizing_finished", "mapping_finished", "meshing_finished",
                 "visualizing_finished"):
        assert int(getattr(s, flag)) == 1, flag


def test_run_only_tracking_calls_nothing_but_tracker_and_ba(slam_mod):
    s, log = _recorded_slam(slam_mod, only_tracking=True, make_video=True)
    s.run(_stream(7))
    names = [n for n, _, _ in log]
    assert set(names) == {"tracker", "ba"}
    assert names.count("tracker") == 7 and names.count("ba") == 3 + 1 and names[-1] == "ba"
    assert int(s.meshing_finished) == 1 and int(s.tracking_finished) == 1


def test_run_drops_the_depth_in_mono_mode(slam_mod):
    s, log = _recorded_slam(slam_mod, mode="mono")
    s.run(_stream(7))
    assert all(a[2] is None for n, a, _ in log if n == "tracker")
    assert all(a[1] is not None and a[3] is not None for n, a, _ in log if n == "tracker")


def test_run_meshes_every_50th_timestamp_with_make_video(slam_mod):
    s, log = _recorded_slam(slam_mod, make_video=True, keyframes=(), post=0)
    stream = [(i, None, None, None, None) for i in (0, 49, 50, 51, 100)]
    s.run(stream)
    names = [n for n, _, _ in log]
    assert names == ["tracker", "tracker", "tracker", "mesher", "tracker", "tracker", "mesher", "ba", "multiview_filter"]


def test_load_pretrained_cuts_the_heads_and_strips_prefixes(slam_mod, tmp_path, capsys):
    from go_slam_amd.droid_net import DroidNet
    torch.manual_seed(5)
    donor = DroidNet()
    state = {}
    for k, v in donor.state_dict().items():
        if k in ("update.weight.2.weight", "update.weight.2.bias", "update.delta.2.weight", "update.delta.2.bias"):
            v = torch.cat([v, torch.full_like(v[:1], 7.0)], dim=0)      # the checkpoint's third row
            assert v.shape[0] == 3
        state["module." + k] = v
    path = str(tmp_path / "droid.pth")
    torch.save(state, path)
    s = object.__new__(slam_mod.SLAM)
    torch.manual_seed(6)
    s.net = DroidNet()
    s.load_pretrained(path)
    for k, v in donor.state_dict().items():
        assert torch.equal(s.net.state_dict()[k], v), k
    before = {k: v.clone() for k, v in s.net.state_dict().items()}
    capsys.readouterr()
    for empty in (None, ""):
        s.load_pretrained(empty)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 2 and all("randomly initialised" in l for l in lines)       # one line per call
    assert all(torch.equal(before[k], v) for k, v in s.net.state_dict().items())


def test_run_py_takes_the_reference_arguments():
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_entry", os.path.join(os.path.dirname(HERE), "run.py"))
    src = open(spec.origin).read()
    for flag in ("--device", "--max_frames", "--only_tracking", "--make_video", "--input_folder", "--output",
                 "--image_size", "--calibration_txt", "--mode", "--default_config"):
        assert f'"{flag}"' in src, flag
    assert "./configs/go_slam.yaml" in src and "setup_seed(43)" in src
