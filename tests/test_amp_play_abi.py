"""include/dyros_amp_policy.h, ABI version 2: dwa_play and dwa_play_workspace_bytes are declared, mirrored in amp_policy.EXPORTS and exported
by the built library; the play kernels use no scratch and run their products on v_mfma_f32_16x16x4_f32 only (hipcc with the flags of
build.py; no GPU needed)."""
import ctypes
import os
import re
import subprocess

from isaacgymdyros_amd import amp_policy, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_amp_policy.hip"


def test_play_is_declared_mirrored_and_exported():
    hdr = open(os.path.join(ROOT, "include", "dyros_amp_policy.h")).read()
    assert re.search(r"\bint dwa_play\s*\(", hdr) and re.search(r"\bint64_t dwa_play_workspace_bytes\s*\(", hdr)
    assert amp_policy.K["DWA_ABI_VERSION"] == 2
    assert {"play", "play_workspace_bytes"} <= set(amp_policy.EXPORTS)
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "dwa_play") and hasattr(lib, "dwa_play_workspace_bytes") and lib.dwa_abi_version() == 2
    f = lib.dwa_play_workspace_bytes
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int32] * 3
    assert f(1, 468, 12) == 2 * 512 * 4 and f(64, 468, 12) == 64 * 2 * 512 * 4 and f(65, 468, 12) == 0 and f(16384, 1, 1) == 0
    for bad in ((0, 468, 12), (8, 0, 12), (8, 513, 12), (8, 468, 0), (8, 468, 17)):
        assert f(*bad) == -1, bad


def test_play_kernels_no_scratch_fp32_mfma_only(tmp_path):
    extra = dict(build.SOURCES)[SRC]
    base = [build.hipcc()] + build.FLAGS + extra
    rem = subprocess.run(base + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(build.CSRC, SRC)],
                         cwd=build.CSRC, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"remark: Function Name: (\S+)", rem)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", rem)]
    play = [(n, s) for n, s in zip(names, scratch) if "dwa_play" in n]
    assert len(play) == 4, play          # dwa_play_rows, dwa_play_cols<0>, dwa_play_cols<1>, dwa_play_head
    assert all(s == 0 for _n, s in play), play
    subprocess.run(base + ["--cuda-device-only", "-S", "-o", str(tmp_path / "p.s"), os.path.join(build.CSRC, SRC)], cwd=build.CSRC,
                   capture_output=True, text=True, check=True)
    parts = re.split(r"^(_Z\S+):", open(tmp_path / "p.s").read(), flags=re.M)
    bodies = [(parts[i], parts[i + 1]) for i in range(1, len(parts) - 1, 2) if "dwa_play" in parts[i]]
    assert len(bodies) == 4
    for name, body in bodies:
        mf = re.findall(r"\bv_mfma_\S+", body)
        assert mf and set(mf) == {"v_mfma_f32_16x16x4_f32"}, (name, sorted(set(mf)))
