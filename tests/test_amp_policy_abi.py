"""include/dyros_amp_policy.h: the dwa_ functions are declared, mirrored in isaacgymdyros_amd/amp_policy.py and exported by the built library;
the kernels of csrc/dw_amp_policy.hip use no scratch, the product kernels run on the fp32 matrix cores, and no kernel name joins the sets
other tests select by substring (hipcc with the flags of build.py; no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

from isaacgymdyros_amd import amp_policy, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_amp_policy.hip"
TAKEN = ("k_mlp", "k_wgrad", "k_policy", "k_adam", "k_grad_stats", "k_finish", "k_gae", "k_roll_pre", "k_roll_post", "k_loss", "k_relu_bwd",
         "k_bias_relu", "k_stage_obs", "k_retile", "dw_k_amp", "dw_k_newwalk", "dw_k_body_positions", "dwd_k_")


def declared():
    src = open(os.path.join(ROOT, "include", "dyros_amp_policy.h")).read()
    return sorted(set(re.findall(r"\b(dwa_[a-z_0-9]+)\s*\(", src)))


def test_header_python_and_library_agree():
    assert declared() == sorted("dwa_" + n for n in amp_policy.EXPORTS)
    assert SRC in dict(build.SOURCES)
    lib = ctypes.CDLL(build.build())
    for fn in declared():
        assert hasattr(lib, fn), fn
    assert lib.dwa_abi_version() == amp_policy.K["DWA_ABI_VERSION"]
    lib.dwa_workspace_bytes.restype = ctypes.c_int64
    assert lib.dwa_workspace_bytes(4096, 468, 12, 1) > lib.dwa_workspace_bytes(4096, 468, 12, 0) > 0
    for bad in ((0, 468, 12, 0), (8, 0, 12, 0), (8, 513, 12, 0), (8, 468, 0, 0), (8, 468, 17, 1), (8, 468, 12, 2)):
        assert lib.dwa_workspace_bytes(*bad) == -1, bad
    assert amp_policy.num_params(468, 12) == 2 * (468 * 512 + 512 + 512 * 512 + 512) + 12 * 512 + 12 + 512 + 1


@pytest.fixture(scope="module")
def remarks():
    extra = dict(build.SOURCES)[SRC]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(build.CSRC, SRC)]
    return subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True).stderr


def test_policy_kernels_use_no_scratch(remarks):
    names = re.findall(r"remark: Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    assert len(names) >= 12 and len(scratch) == len(names)
    for n, s in zip(names, scratch):
        assert "dwa_" in n, n
        assert s == 0, (n, s)


def test_kernel_names_stay_out_of_other_tests_sets(remarks):
    for n in re.findall(r"remark: Function Name: (\S+)", remarks):
        assert not any(x in n for x in TAKEN), n


def test_product_kernels_run_on_the_fp32_matrix_cores(tmp_path):
    """The ISA of dwa_mm (every instantiation) holds v_mfma_f32_16x16x4_f32 and no other MFMA form (no downcast)."""
    extra = dict(build.SOURCES)[SRC]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["--cuda-device-only", "-S", "-o", str(tmp_path / "p.s"), os.path.join(build.CSRC, SRC)]
    subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True)
    asm = open(tmp_path / "p.s").read()
    parts = re.split(r"^(_Z\S+):", asm, flags=re.M)          # [preamble, label, body, label, body, ...]
    bodies = [(parts[i], parts[i + 1]) for i in range(1, len(parts) - 1, 2) if "dwa_mm" in parts[i]]
    assert len(bodies) == 3, [b[0] for b in bodies]
    for name, body in bodies:
        mf = re.findall(r"\bv_mfma_\S+", body)
        assert mf and set(mf) == {"v_mfma_f32_16x16x4_f32"}, (name, sorted(set(mf)))
    assert not re.search(r"v_mfma_\S*(f16|bf16|xf32|fp8|bf8)", asm)
