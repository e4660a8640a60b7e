"""The device bits of dwi_solve and dwk_solve against a recorded file (tools/inverse_dynamics_bits.py, DESIGN.md sections 27 and 28): both
kernels are one body (csrc/dw_contact_inverse.hip), so dwk_solve with every contact on against dwi_solve on the device compares that body
with itself; this file holds both to bits recorded before they were one."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_device_bits_are_the_recorded_ones():
    """tests/golden/inverse_dynamics_bits.npz: 5 envs (two workgroups, the second holds one env), dwi_solve with 1, 2 and 4 contacts, dwk_solve
    with 2 and 4 and the envs in different stances (flight, single support, every contact on), both velocity modes, moments weighted 10 x,
    f_ref, mass_scale and dof_armature given; and one dwk_solve case standing still in the initial pose without f_ref, where feasible is 1 on
    both feet and 0 in flight and on one foot: every output of both entry points, bit for bit.

    The bits were recorded on an MI355X from a build of commit 9556a85 -- the last with dwi_k_solve and dwk_k_solve as two separate kernels
    (dw_contact_inverse.hip and dw_stance_inverse.hip), dwi_k_solve with section 27's plain row-ordered sums -- by hipcc --version = HIP version
    7.2.26015-fc0010cf6a, AMD clang version 22.0.0git (roc-7.2.0 26014 7b800a19466229b8479a78de19143dc33c3ab9b5).  The sums are the same terms
    in the same order under -ffp-contract=off, so a differing bit with that toolchain is a defect to be found, not a new baseline.  After a
    toolchain change the bits are re-recorded (--record) only once the float64 tests of tests/test_contact_inverse_dynamics_gpu.py and
    tests/test_stance_inverse_dynamics_gpu.py pass with the new toolchain."""
    spec = importlib.util.spec_from_file_location("inverse_dynamics_bits", os.path.join(ROOT, "tools", "inverse_dynamics_bits.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    bad = tool.differences(os.path.join(ROOT, "tests", "golden", "inverse_dynamics_bits.npz"))
    assert not bad, bad
