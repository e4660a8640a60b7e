"""include/dyros_gait.h: the dwg_ functions are declared, bound from the header by isaacgymdyros_amd/gait_profile.py and exported by the built
library; the kernels of csrc/dw_gait.hip use no scratch, the record kernel's LDS fits a workgroup's static limit, and no kernel name joins
the sets other tests select by substring (hipcc with the flags of build.py; no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

from isaacgymdyros_amd import build, cbind, gait_profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_gait.hip"
TAKEN = ("k_mlp", "k_wgrad", "k_policy", "k_adam", "k_grad_stats", "k_finish", "k_gae", "k_roll_pre", "k_roll_post", "k_loss", "k_relu_bwd",
         "k_bias_relu", "k_stage_obs", "k_retile", "dw_k_amp", "dw_k_newwalk", "dw_k_body_positions", "dwd_k_", "dws_k_", "dwt_k_", "dwm_k_")


def declared():
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dyros_gait.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dwg_[a-z_0-9]+)\s*\(", src)))


def test_header_python_and_library_agree():
    assert declared() == sorted("dwg_" + n for n in gait_profile.EXPORTS)
    assert {"dwg_abi_version", "dwg_last_error", "dwg_record", "dwg_clear", "dwg_summarize"} <= set(declared())
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_gait.h" in build.HEADERS
    lib = ctypes.CDLL(build.build())
    for fn in declared():
        assert hasattr(lib, fn), fn
    assert lib.dwg_abi_version() == gait_profile.K["DWG_ABI_VERSION"] == 1
    api = cbind.declare(lib, "dyros_gait.h", "dwg_")
    assert api["record"].argtypes == [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 11 and api["groups"].restype is ctypes.c_int64
    assert [api["groups"](n) for n in (1, 64, 65, 16384, 0, -3)] == [1, 1, 2, 256, -1, -1]
    # refused before any launch: a bin count outside the set, a missing buffer
    assert api["record"](8, 48, 0, 0, *[None] * 11) == -1 and b"bins must be one of" in api["last_error"]()
    assert api["record"](8, 72, 0, 0, *[None] * 11) == -1 and b"a buffer is missing" in api["last_error"]()
    assert api["clear"](0, 72, None, None, None) == -1 and api["summarize"](8, 72, None, None, None, None) == -1
    K = gait_profile.K
    assert K["DWG_W"] == 40 and K["DWG_R_TORQUE"] + K["DWG_LEG_JOINTS"] == K["DWG_W"] and K["DWG_ROWS"] % K["DWG_BINS_MAX"] == 0
    assert all(K["DWG_ROWS"] % b == 0 and edge % (K["DWG_ROWS"] // b) == 0 for b in gait_profile.BINS for edge in (300, 1500, 2100, 3300))


@pytest.fixture(scope="module")
def remarks():
    extra = dict(build.SOURCES)[SRC]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(build.CSRC, SRC)]
    return subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True).stderr


def test_kernels_use_no_scratch_and_the_table_fits(remarks):
    names = re.findall(r"remark: Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)]
    assert len(names) == 3 and len(scratch) == len(lds) == 3
    for n, s, l in zip(names, scratch, lds):
        assert "dwg_k_" in n and s == 0, (n, s)
        if "dwg_k_record" in n:          # the [144][40] int64 table and the staged joint words, under the 64 KB of a static allocation
            assert 144 * 40 * 8 <= l <= 64 * 1024, l


def test_kernel_names_stay_out_of_other_tests_sets(remarks):
    for n in re.findall(r"remark: Function Name: (\S+)", remarks):
        assert not any(x in n for x in TAKEN), n
