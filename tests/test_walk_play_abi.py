"""include/dyros_ppo.h, ABI version 10: dwp_play (there since 9) and dwp_play_work_floats are declared, mirrored in ppo_update.EXPORTS and exported by the built
library; the play kernels use no scratch, run their products on v_mfma_f32_16x16x4_f32 only, and no kernel name joins the sets other tests select
by substring (hipcc with the flags of build.py; no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

from isaacgymdyros_amd import build, ppo_update

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_ppo.hip"
TAKEN = ("k_mlp", "k_wgrad", "k_policy", "k_adam", "k_grad_stats", "k_finish", "k_gae", "k_roll_pre", "k_roll_post", "k_loss", "k_relu_bwd",
         "k_bias_relu", "k_stage_obs", "k_retile", "dw_k_amp", "dw_k_newwalk", "dw_k_body_positions", "dwd_k_", "dwa_play")


def test_play_is_declared_mirrored_and_exported():
    hdr = open(os.path.join(ROOT, "include", "dyros_ppo.h")).read()
    assert re.search(r"\bint dwp_play\s*\(", hdr) and re.search(r"\bint dwp_play_work_floats\s*\(", hdr)
    assert ppo_update.K["DWP_ABI_VERSION"] == 10
    assert {"play", "play_work_floats"} <= set(ppo_update.EXPORTS)
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "dwp_play") and hasattr(lib, "dwp_play_work_floats") and lib.dwp_abi_version() == 10
    f = lib.dwp_play_work_floats
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int32]
    assert f(1) == 2 * 256 and f(64) == 64 * 2 * 256 and f(65) == 0 and f(16384) == 0
    assert f(0) == -1 and f(-3) == -1


@pytest.fixture(scope="module")
def remarks():
    extra = dict(build.SOURCES)[SRC]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(build.CSRC, SRC)]
    return subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True).stderr


def test_play_kernels_no_scratch_and_names_stay_out_of_other_sets(remarks):
    names = re.findall(r"remark: Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    assert len(scratch) == len(names)
    play = [(n, s) for n, s in zip(names, scratch) if "k_wplay" in n]
    assert len(play) == 4, play          # k_wplay_rows, k_wplay_cols<1>, <2>, <3>
    assert all(s == 0 for _n, s in play), play
    for n, _s in play:
        assert not any(x in n for x in TAKEN), n


def test_play_kernels_run_on_the_fp32_matrix_cores_only(tmp_path):
    extra = dict(build.SOURCES)[SRC]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["--cuda-device-only", "-S", "-o", str(tmp_path / "p.s"), os.path.join(build.CSRC, SRC)]
    subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True)
    parts = re.split(r"^(_Z\S+):", open(tmp_path / "p.s").read(), flags=re.M)
    bodies = [(parts[i], parts[i + 1]) for i in range(1, len(parts) - 1, 2) if "k_wplay" in parts[i]]
    assert len(bodies) == 4, [b[0] for b in bodies]
    for name, body in bodies:
        mf = re.findall(r"\bv_mfma_\S+", body)
        assert mf and set(mf) == {"v_mfma_f32_16x16x4_f32"}, (name, sorted(set(mf)))
