"""include/dyros_amp_disc.h: the dwd_ functions are declared, mirrored in isaacgymdyros_amd/amp_disc.py and exported by the built library, and
the kernels of csrc/dw_amp_disc.hip use no scratch (hipcc -Rpass-analysis=kernel-resource-usage with the flags of build.py; no GPU needed)."""
import ctypes
import os
import re
import subprocess

from isaacgymdyros_amd import amp_disc, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    src = open(os.path.join(ROOT, "include", "dyros_amp_disc.h")).read()
    return sorted(set(re.findall(r"\b(dwd_[a-z_0-9]+)\s*\(", src)))


def test_header_python_and_library_agree():
    assert declared() == sorted("dwd_" + n for n in amp_disc.EXPORTS)
    assert ("dw_amp_disc.hip", []) in build.SOURCES
    lib = ctypes.CDLL(build.build())
    for fn in declared():
        assert hasattr(lib, fn), fn
    assert lib.dwd_abi_version() == amp_disc.K["DWD_ABI_VERSION"]
    lib.dwd_grad_workspace_bytes.restype = ctypes.c_int64
    assert lib.dwd_grad_workspace_bytes(68, 4, 4, 4) > 0
    assert lib.dwd_grad_workspace_bytes(69, 4, 4, 4) == -1 and lib.dwd_grad_workspace_bytes(374, 4, 4, 4) == -1


def test_disc_kernels_use_no_scratch():
    extra = dict(build.SOURCES)["dw_amp_disc.hip"]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                                                   os.path.join(build.CSRC, "dw_amp_disc.hip")]
    err = subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"remark: Function Name: (\S+)", err)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
    kernels = [n for n in names if "dwd_k_" in n]
    assert len(kernels) >= 9 and len(scratch) == len(names)
    for n, s in zip(names, scratch):
        assert s == 0, (n, s)
    # (test_kernel_resources.py picks its PPO and AMP sets by substring: none of these names may join them)
    for n in kernels:
        assert not any(x in n for x in ("k_mlp", "k_wgrad", "k_policy", "k_adam", "k_grad_stats", "k_finish", "k_gae", "k_roll_pre", "k_roll_post",
                                        "k_loss", "k_relu_bwd", "k_bias_relu", "k_stage_obs", "k_retile", "dw_k_amp")), n
