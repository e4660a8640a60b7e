"""The device-resident motion table (TocabiLowerMotionLib.device_table, include/dyros_walk.h DwMotionTable) on the CPU: the table, with the
float64 index math restated in numpy (tests/amp_motion_ref.py), reproduces get_motion_state bit for bit on every returned tensor."""
import numpy as np
import pytest
import torch

from isaacgymdyros_amd import motion_lib as ML
from tests import amp_motion_ref as MR

NAMES = ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel", "key_pos")


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("motions"))
    return ML.TocabiLowerMotionLib(MR.write_small(tmp), 33, "cpu"), ML.TocabiLowerMotionLib(MR.write_slerp_table(tmp), 33, "cpu")


def test_device_table_layout(libs):
    lib, _ = libs
    dt = lib.device_table()
    assert dt.rows.dtype == torch.float32 and tuple(dt.rows.shape) == (700 + 1300 + 1100, 43)
    assert dt.start.dtype == torch.int32 and dt.num_frames.dtype == torch.int32
    assert dt.length.dtype == dt.dt.dtype == dt.cum_weight.dtype == torch.float64
    assert dt.start.tolist() == [0, 700, 2000] and dt.num_frames.tolist() == [700, 1300, 1100]
    assert float(dt.dt[0]) < 0 < float(dt.dt[1])                     # motion 0 is played backwards: the signed dt
    assert np.array_equal(dt.cum_weight.numpy(), np.cumsum(lib._motion_weights)) and abs(float(dt.cum_weight[-1]) - 1.0) < 1e-15
    # positions rounded once, velocities scaled per motion in float64 and then rounded
    t = lib._table
    assert np.array_equal(dt.rows[:, 24:31].numpy(), t[:, 25:32].astype(np.float32))
    assert np.array_equal(dt.rows[700:2000, 12:24].numpy(), (t[700:2000, 13:25] * 0.0005 / lib._motion_dt[1]).astype(np.float32))


def test_table_reproduces_get_motion_state_bitwise(libs):
    lib, _ = libs
    tab = MR.HostTable(lib.device_table())
    ids, times = MR.queries(lib)
    assert (times == 0).any() and (times < 0).any() and any(times[i] == lib._motion_lengths[ids[i]] for i in range(len(ids)))
    f0, f1, bl = lib.frame_blend(ids, times)
    r0, r1, bl2, i0 = MR.frame_blend(tab, ids, times)
    assert np.array_equal(i0, f0) and np.array_equal(r1 - r0, f1 - f0) and np.array_equal(bl, bl2)
    assert (bl < 0).any()                                            # a time below zero extrapolates, as in the reference
    for name, mine, ref in zip(NAMES, MR.motion_state(tab, ids, times), lib.get_motion_state(ids, times)):
        assert mine.dtype == ref.dtype == torch.float32 and mine.shape == ref.shape, name
        assert np.array_equal(mine.numpy(), ref.numpy(), equal_nan=True), name


def test_slerp_branches_bitwise(libs):
    _, lib = libs
    tab = MR.HostTable(lib.device_table())
    dt = abs(float(lib._motion_dt[0]))
    times = np.array([(k + f) * dt for k in range(5) for f in (0.0, 0.25, 0.5, 0.8125)] + [-0.3 * dt, 5 * dt])
    ids = np.zeros(len(times), dtype=np.int64)
    br, neg = MR.slerp_branch(tab, ids, times)
    assert (br == 0).any() and (br == 1).any() and ((br == 2) & neg).any() and ((br == 2) & ~neg).any()
    for name, mine, ref in zip(NAMES, MR.motion_state(tab, ids, times), lib.get_motion_state(ids, times)):
        assert np.array_equal(mine.numpy(), ref.numpy(), equal_nan=True), name
    assert torch.isfinite(lib.get_motion_state(ids, times)[1]).all()
