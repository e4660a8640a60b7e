"""Mints the fixtures that stand in for the reference checkout in the tests that compare with it live:
tests/golden/reference_cfg.json (the reference's task and train YAML as the project's loaders resolve them, the fields
tests/test_config_yaml.py and tests/test_ppo_consumer.py compare) and tests/golden/reference_live.npz (the reference's
`Terrain` for tests/test_terrain.py::test_live_against_reference_when_present, and its reward / quaternion functions on the
inputs of tests/test_torch_twin.py::test_twin_is_bitwise_the_reference_on_cpu).  The cases themselves are in
tests/reference_cases.py.  The tests read these fixtures everywhere and compare live as well where the reference is mounted.
Test infrastructure; needs the reference checkout (oracle/ref_harness.py).
usage: python oracle/make_live_goldens.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reference_cases as RC                                           # noqa: E402
from isaacgymdyros_amd.model import load_model                        # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    cfg = {"task_yaml": RC.task_yaml_record(RC.task_yaml_path()), "train_yaml": RC.train_yaml_record(RC.train_yaml_path())}
    with open(os.path.join(GOLDEN, "reference_cfg.json"), "w") as f:
        json.dump(cfg, f, indent=1, sort_keys=True)
        f.write("\n")
    out = {}
    for seed in RC.TERRAIN_SEEDS:
        h, o = RC.reference_terrain(seed)
        out["terrain/%d/heightsamples" % seed], out["terrain/%d/env_origins" % seed] = h, o
    out.update(RC.reference_twin(load_model()))
    np.savez_compressed(os.path.join(GOLDEN, "reference_live.npz"), **out)
    for k, v in sorted(out.items()):
        print(k, v.dtype, v.shape)


if __name__ == "__main__":
    main()
