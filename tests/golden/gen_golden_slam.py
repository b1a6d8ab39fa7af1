"""Fixtures of tests/test_slam_cpu.py, produced by the reference's own code (needs the reference tree; run from anywhere):

    python tests/golden/gen_golden_slam.py [path to the reference tree; default: gen_golden.REF]

  * tests/golden/configs/go_slam.yaml and tests/golden/configs/Replica/replica.yaml: verbatim copies of two of the
    reference's settings files (the second is loaded over the first);
  * tests/golden/slam.json:
      load_config      what the reference's src/config.py load_config returns for replica.yaml over go_slam.yaml, for
                       go_slam.yaml alone, and for a three-deep inherit_from chain (two small files written here, whose
                       texts are stored with {dir} for the folder they are placed in, over replica.yaml)
      update_cam       SLAM.update_cam's fx fy cx cy H W for three camera blocks (the default with its edge crop,
                       Replica's non-square resize, and one with both)
      signatures       the constructor parameters of SLAM, Tracker and BundleAdjustment
"""
import importlib
import importlib.util
import inspect
import json
import os
import shutil
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

CHAIN = {
    "mid.yaml": "inherit_from: {dir}/configs/Replica/replica.yaml\n"
                "tracking:\n  buffer: 96\n  frontend:\n    window: 12\nmeshing:\n  resolution: 64\n",
    "top.yaml": "inherit_from: {dir}/mid.yaml\n"
                "mode: mono\ntracking:\n  frontend:\n    window: 9\nmapping:\n  bound: [[-1, 1], [-2, 2], [-3, 3]]\n"
                "data:\n  output: out/top\n",
}
CAMERAS = {
    "default_edge_crop": None,            # go_slam.yaml's own cam block
    "replica_non_square_resize": None,    # replica.yaml's
    "both": {"H": 480, "W": 752, "fx": 458.654, "fy": 457.296, "cx": 367.215, "cy": 248.375, "H_edge": 12, "W_edge": 20,
             "H_out": 300, "W_out": 512},
}


def main(ref):
    import gen_golden as G
    ref = ref or G.REF
    from go_slam_amd.dropin import _torch_scatter
    G.install_stubs()
    sys.modules.setdefault("torch_scatter", _torch_scatter())
    for name in ("open3d", "cv2", "pyrender", "matplotlib", "matplotlib.pyplot", "evo", "tqdm"):
        try:
            importlib.import_module(name)
        except Exception:
            mod = types.ModuleType(name)
            mod.tqdm = lambda x, *a, **k: x
            sys.modules[name] = mod
    sys.path.insert(0, ref)
    spec = importlib.util.spec_from_file_location("ref_config", os.path.join(ref, "src", "config.py"))
    ref_config = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_config)
    slam_mod = importlib.import_module("src.slam")

    cfg_dir = os.path.join(HERE, "configs")
    os.makedirs(os.path.join(cfg_dir, "Replica"), exist_ok=True)
    shutil.copyfile(os.path.join(ref, "configs", "go_slam.yaml"), os.path.join(cfg_dir, "go_slam.yaml"))
    shutil.copyfile(os.path.join(ref, "configs", "Replica", "replica.yaml"), os.path.join(cfg_dir, "Replica", "replica.yaml"))
    default = os.path.join(cfg_dir, "go_slam.yaml")
    replica = os.path.join(cfg_dir, "Replica", "replica.yaml")

    out = {"load_config": {}, "update_cam": {}, "signatures": {}, "chain_files": CHAIN}
    out["load_config"]["default_alone"] = ref_config.load_config(default)
    out["load_config"]["replica_over_default"] = ref_config.load_config(replica, default)
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copytree(cfg_dir, os.path.join(tmp, "configs"))
        for name, text in CHAIN.items():
            with open(os.path.join(tmp, name), "w") as fh:
                fh.write(text.replace("{dir}", tmp))
        chain = ref_config.load_config(os.path.join(tmp, "top.yaml"), os.path.join(tmp, "configs", "go_slam.yaml"))
        chain["inherit_from"] = chain["inherit_from"].replace(tmp, "{dir}")
        out["load_config"]["three_deep_chain"] = chain

    blocks = dict(CAMERAS)
    blocks["default_edge_crop"] = out["load_config"]["default_alone"]["cam"]
    blocks["replica_non_square_resize"] = out["load_config"]["replica_over_default"]["cam"]
    for name, cam in blocks.items():
        holder = types.SimpleNamespace()
        slam_mod.SLAM.update_cam(holder, {"cam": cam})
        out["update_cam"][name] = {"cam": cam, "result": {k: getattr(holder, k) for k in ("fx", "fy", "cx", "cy", "H", "W")}}

    for cls in ("SLAM", "Tracker", "BundleAdjustment"):
        init = getattr(slam_mod, cls).__init__
        out["signatures"][cls] = [[p.name, p.kind.name, p.default is not inspect.Parameter.empty]
                                  for p in inspect.signature(init).parameters.values() if p.name != "self"]
    with open(os.path.join(HERE, "slam.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print("wrote slam.json", {k: list(v) for k, v in out.items() if isinstance(v, dict)})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
