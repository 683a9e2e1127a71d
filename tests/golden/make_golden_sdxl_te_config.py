#!/usr/bin/env python
"""Generates tests/golden/config_class_paths_sdxl_te.json: the `model:` tree of the reference's configs/sdxl/sdxl-te.example.yaml (both
text towers trained with the UNet) as DATA, in the format of config_class_paths.json (make_golden.py::config_case): for every node that
names a class, where it sits, its class_path, its init_args names (and their values when plain), and whether the path resolves in the
reference itself (with make_golden.py's stand-ins for the packages this image lacks, bitsandbytes among them).

    python tests/golden/make_golden_sdxl_te_config.py
"""
from __future__ import annotations

import importlib
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from tests.golden.make_golden import REF_SRC, import_reference  # noqa: E402

CONFIG = "configs/sdxl/sdxl-te.example.yaml"
OUT = Path(__file__).resolve().parent / "config_class_paths_sdxl_te.json"


def resolves(cp: str) -> bool:
    mod, _, name = cp.rpartition(".")
    try:
        return hasattr(importlib.import_module(mod), name)
    except Exception:
        return False


def plain(v) -> bool:
    if isinstance(v, dict):
        return "class_path" not in v and all(plain(e) for e in v.values())
    return isinstance(v, (int, float, str, bool, type(None))) or (isinstance(v, list) and all(isinstance(e, (int, float, str, bool)) for e in v))


def main():
    import yaml

    import_reference()
    cfg = yaml.safe_load(open(REF_SRC.parent / CONFIG))
    nodes = []

    def walk(node, where):
        if isinstance(node, dict):
            if "class_path" in node:
                ia = node.get("init_args", {}) or {}
                nodes.append({"where": where, "class_path": node["class_path"], "init_arg_names": sorted(ia.keys()),
                              "plain_init_args": {k: v for k, v in ia.items() if plain(v)}, "resolves_in_reference": resolves(node["class_path"])})
                for k, v in ia.items():
                    walk(v, f"{where}.init_args.{k}")
            else:
                for k, v in node.items():
                    walk(v, f"{where}.{k}")
        elif isinstance(node, list):
            for i, v in enumerate(node):
                walk(v, f"{where}[{i}]")

    walk(cfg["model"], "model")
    OUT.write_text(json.dumps({CONFIG: {"nodes": nodes}}, indent=1) + "\n")
    print(f"wrote {OUT}: {len(nodes)} nodes")


if __name__ == "__main__":
    main()
