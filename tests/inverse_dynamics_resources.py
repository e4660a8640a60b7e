"""The resource remarks of csrc/dw_contact_inverse.hip, the one unit that holds dwi_k_solve and dwk_k_solve, read kernel by kernel; shared by
tests/test_contact_inverse_dynamics.py and tests/test_stance_inverse_dynamics.py.  Test helper."""
import os
import re
import subprocess

from isaacgymdyros_amd import build

SRC = "dw_contact_inverse.hip"
KEYS = {"vgprs": r" VGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "occ": r"Occupancy \[waves/SIMD\]: (\d+)", "lds": r"LDS Size \[bytes/block\]: (\d+)"}


def remarks(src):
    """hipcc's -Rpass-analysis=kernel-resource-usage remarks for a unit, built with the flags build.py gives it."""
    cmd = [build.hipcc()] + build.FLAGS + dict(build.SOURCES)[src] + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(build.CSRC, src)]
    return subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True).stderr


def kernels(src):
    """mangled kernel name -> {"vgprs", "scratch", "occ", "lds"} for every kernel of a unit."""
    out = {}
    for block in remarks(src).split("remark: Function Name: ")[1:]:
        found = {k: re.findall(rx, block) for k, rx in KEYS.items()}
        assert all(len(v) == 1 for v in found.values()), block
        out[block.split()[0]] = {k: int(v[0]) for k, v in found.items()}
    return out


def solve_kernels():
    """(dwi_k_solve's, dwk_k_solve's, dwn_k_inverse_dynamics's) resources; the unit holds exactly the first two, dw_dynamics.hip exactly the third."""
    ks, dwn = kernels(SRC), kernels("dw_dynamics.hip")
    assert sorted(re.sub(r".*(dw[ik]_k_solve).*", r"\1", k) for k in ks) == ["dwi_k_solve", "dwk_k_solve"] and len(dwn) == 1
    name = lambda s: next(k for k in ks if s in k)          # noqa: E731
    return (name("dwi_k_solve"), ks[name("dwi_k_solve")]), (name("dwk_k_solve"), ks[name("dwk_k_solve")]), next(iter(dwn.values()))
