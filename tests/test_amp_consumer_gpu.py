"""examples/amp_consumer.py end to end: two epochs of the AMP learner on TocabiAMPLower with the synthetic motion tables, in a child process
under a time limit."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_epochs_synthetic_256_envs():
    cmd = [sys.executable, os.path.join(ROOT, "examples", "amp_consumer.py"), "--synthetic", "--num_envs", "256", "--epochs", "2"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 2, p.stdout
    for l in lines:
        vals = dict(re.findall(r"(\w+) (-?[0-9.e+-]+|nan|inf)", l))
        for k in ("disc_r", "a_loss", "c_loss", "b_loss", "loss", "grad_penalty", "agent_acc", "demo_acc"):
            assert math.isfinite(float(vals[k])), (k, l)
