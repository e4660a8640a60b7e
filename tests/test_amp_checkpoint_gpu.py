"""Checkpoints of the AMP learner on the HIP backend (isaacgymdyros_amd/amp_checkpoint.py): the round trip with the Adam moments and step
counts, across backends, resuming bit for bit, and examples/amp_consumer.py / examples/amp_player.py end to end in child processes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from isaacgymdyros_amd import amp_checkpoint as CK

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_amp_checkpoint as T          # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def test_hip_round_trip_and_across_backends(tmp_path):
    pol, disc = T.trained(2, backend="hip", device=DEV)
    for x in (pol, disc):
        st = x.optimizer_state()
        assert st["step"] == 2 and all(v.abs().sum() > 0 for v in st["exp_avg_sq"].values())
    path = CK.save(str(tmp_path / "h.pth"), pol, disc, epoch=2)
    p2, d2 = T.learners(seed=9, backend="hip", device=DEV)
    CK.restore(path, p2, d2)
    T.assert_same_learners(pol, disc, p2, d2)
    for a, b in ((pol, p2), (disc, d2)):
        T.same(a.m, b.m, "m")
        T.same(a.v, b.v, "v")
        T.same(a.state[12:14], b.state[12:14], "lr and step words")
    # HIP -> torch -> HIP
    pt, dt = T.learners(seed=4, backend="torch", device=DEV)
    CK.restore(path, pt, dt)
    T.assert_same_learners(pol, disc, pt, dt)
    path2 = CK.save(str(tmp_path / "t.pth"), pt, dt, epoch=2)
    p3, d3 = T.learners(seed=5, backend="hip", device=DEV)
    CK.restore(path2, p3, d3)
    T.assert_same_learners(pol, disc, p3, d3)
    for a, b in ((pol, p3), (disc, d3)):
        T.same(a.m, b.m, "m")
        T.same(a.v, b.v, "v")


def test_hip_resume_equivalence(tmp_path):
    pol, disc = T.trained(3, backend="hip", device=DEV)
    path = CK.save(str(tmp_path / "r.pth"), pol, disc, epoch=3)
    nxt = T.batch(99, device=DEV)
    p2, d2 = T.learners(seed=5, backend="hip", device=DEV)
    CK.restore(path, p2, d2)
    r2, m2 = T.update(p2, d2, nxt, lr=7e-5)
    torch.set_rng_state(torch.load(path, weights_only=True)[CK.OUR_KEY]["torch_rng_state"])
    r1, m1 = T.update(pol, disc, nxt, lr=7e-5)
    T.same(r1, r2, "replay draw")
    T.same(m1, m2, "demo draw")
    T.assert_same_learners(pol, disc, p2, d2)
    for a, b in ((pol, p2), (disc, d2)):
        T.same(a.p, b.p, "p")
        T.same(a.m, b.m, "m")
        T.same(a.v, b.v, "v")


def run(args, timeout):
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable] + args, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    return p.stdout


@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_consumer_saves_resumes_and_the_player_plays(tmp_path, backend):
    out = str(tmp_path / "runs")
    cons = [os.path.join(ROOT, "examples", "amp_consumer.py"), "--synthetic", "--num_envs", "256", "--policy_backend", backend]
    s1 = run(cons + ["--epochs", "2", "--save_frequency", "1", "--output_dir", out], 600)
    nn_dir = os.path.join(out, "TocabiAMPLower", "nn")
    assert sorted(os.listdir(nn_dir)) == ["TocabiAMPLower.pth", "TocabiAMPLower_1.pth", "TocabiAMPLower_2.pth"]
    assert [int(l.split()[1]) for l in s1.splitlines() if l.startswith("epoch ")] == [0, 1]
    last = os.path.join(nn_dir, "TocabiAMPLower.pth")
    ck = torch.load(last, weights_only=True)
    assert ck["epoch"] == 2 and ck["frame"] == 2 * 256 * 32
    s2 = run(cons + ["--epochs", "2", "--checkpoint", last, "--output_dir", str(tmp_path / "runs2")], 600)
    assert [int(l.split()[1]) for l in s2.splitlines() if l.startswith("epoch ")] == [2, 3]
    ck2 = torch.load(os.path.join(str(tmp_path / "runs2"), "TocabiAMPLower", "nn", "TocabiAMPLower.pth"), weights_only=True)
    assert ck2["epoch"] == 4
    # the learning rate of the last epoch (3) of an uninterrupted run: lr_min + (lr0 - lr_min) (max_epochs - 3) / max_epochs
    lr3 = 1e-6 + (1e-4 - 1e-6) * (5000 - 3) / 5000
    assert np.float32(ck2["optimizer"]["param_groups"][0]["lr"]) == np.float32(lr3)
    assert ck2["optimizer"]["state"][1]["step"] > ck["optimizer"]["state"][1]["step"]
    if backend != "hip":
        return
    exp = str(tmp_path / "export")
    s3 = run([os.path.join(ROOT, "examples", "amp_player.py"), "--checkpoint", last, "--synthetic", "--num_envs", "64", "--games", "64",
              "--export_dir", exp], 600)
    m = re.search(r"^av reward: (\S+) av steps: (\S+)$", s3, flags=re.M)
    assert m and np.isfinite(float(m.group(1))) and np.isfinite(float(m.group(2))) and float(m.group(2)) >= 1, s3[-2000:]
    assert any(l.startswith("reward: ") for l in s3.splitlines())
    names = set(os.listdir(exp))
    assert {k.replace(".", "_") + ".txt" for k in ck["model"]} <= names and "running_mean_std_count.txt" in names
    back = np.loadtxt(os.path.join(exp, "a2c_network_mu_weight.txt")).astype(np.float32)
    assert np.array_equal(back, ck["model"]["a2c_network.mu.weight"].numpy())
    s4 = run([os.path.join(ROOT, "examples", "amp_player.py"), "--checkpoint", last, "--synthetic", "--num_envs", "64", "--games", "8",
              "--stochastic", "--print_disc_prediction", "--policy_backend", "torch"], 600)
    assert "disc_pred: " in s4 and "av reward: " in s4
