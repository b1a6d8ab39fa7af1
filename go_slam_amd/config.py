"""YAML run configuration with inheritance (the semantics of the reference's src/config.py).

A config file may name a parent with `inherit_from`; the parent is loaded first, recursively, and the file's own
entries are merged over it.  A file without a parent is merged over `default_path` when one is given.  Dicts merge in
depth; every other value, lists included, replaces what was there.
"""
import yaml


def update_recursive(d1, d2):
    """Merge d2 into d1 in place: a dict value of d2 descends into d1's entry of that key (created empty when absent),
    any other value overwrites it."""
    for key, value in d2.items():
        if isinstance(value, dict):
            if key not in d1:
                d1[key] = {}
            update_recursive(d1[key], value)
        else:
            d1[key] = value


def _read(path):
    with open(path, "r") as fh:
        return yaml.full_load(fh)


def load_config(path, default_path=None):
    """The dict of `path` merged over its `inherit_from` chain, or over `default_path` where the chain ends."""
    own = _read(path)
    parent = own.get("inherit_from")
    if parent is not None:
        cfg = load_config(parent, default_path)
    elif default_path is not None:
        cfg = _read(default_path)
    else:
        cfg = {}
    update_recursive(cfg, own)
    return cfg


def save_config(cfg, path):
    with open(path, "w") as fh:
        yaml.dump(cfg, fh)
