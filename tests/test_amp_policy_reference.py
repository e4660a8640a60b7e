"""The torch form of the AMP actor-critic's losses and GAE (isaacgymdyros_amd/amp_policy.py: loss_terms, torch_gae) against the reference's
own learner: tests/golden/amp_policy_ref.npz, minted by tools/make_amp_policy_goldens.py from learning/common_agent.py (_actor_loss,
_critic_loss, bound_loss, discount_values), and live against that file where the reference checkout is mounted.  Bit for bit, in fp32 and
in float64, with one CPU thread as the fixture was minted.  The torch form is the yardstick of the HIP kernels (tests/test_amp_policy_gpu.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from isaacgymdyros_amd import amp_policy as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "amp_policy_ref.npz")
_live = {}


def minter():
    spec = importlib.util.spec_from_file_location("make_amp_policy_goldens", os.path.join(ROOT, "tools", "make_amp_policy_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def records():
    out = [("fixture", dict(np.load(GOLDEN)))]
    mg = minter()
    if mg.available():
        if not _live:
            _live.update(mg.compute())
        out.append(("live", _live))
    return out


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_fixture_covers_the_cases():
    r = dict(np.load(GOLDEN))
    for tag in ("f32", "f64"):
        ratio = np.exp(r["in_old_nlp_" + tag] - r["in_nlp_" + tag])
        assert (ratio == 1).any() and (ratio > 1.2).any() and (ratio < 0.8).any()
        assert (r["in_mu_" + tag] > 1).any() and (r["in_mu_" + tag] < -1).any()
        d = r["in_dones_" + tag]
        assert d[:-1].any() and d.dtype == r["in_values_" + tag].dtype
        # the tie rows: the gradient of the surrogate there is -adv / B (two halves of -adv)
        tie = ratio == 1
        B = ratio.shape[0]
        g = r["d_a_nlp_" + tag][tie]
        assert np.allclose(g, r["in_adv_" + tag][tie] / B, rtol=1e-6)


@pytest.mark.parametrize("tag,dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_torch_form_matches_the_reference_bitwise(tag, dtype, one_thread):
    for src, r in records():
        x = {k[3:-4]: torch.from_numpy(v.copy()) for k, v in r.items() if k.startswith("in_") and k.endswith(tag)}
        assert all(t.dtype == dtype for t in x.values())
        nlp, mu, v = (x[k].clone().requires_grad_(True) for k in ("nlp", "mu", "value"))
        a_loss, c_loss, b_loss, clip = AP.loss_terms(x["old_nlp"], nlp, x["adv"], mu, v, x["ret"], 0.2)
        for name, t in (("a_loss", a_loss), ("c_loss", c_loss), ("b_loss", b_loss), ("clip_frac", clip)):
            ref = r["%s_%s" % (name, tag)]          # (a scalar, stored as one element)
            assert ref.size == 1 and np.array_equal(t.detach().numpy().reshape(1), ref.reshape(1)), (src, name)
        assert np.array_equal(torch.autograd.grad(a_loss, nlp)[0].numpy(), r["d_a_nlp_" + tag]), src
        assert np.array_equal(torch.autograd.grad(c_loss, v)[0].numpy(), r["d_c_value_" + tag]), src
        assert np.array_equal(torch.autograd.grad(b_loss, mu)[0].numpy(), r["d_b_mu_" + tag]), src
        adv = AP.torch_gae(x["dones"], x["values"], x["rewards"], x["next_values"], 0.99, 0.95)
        assert np.array_equal(adv.numpy(), r["gae_adv_" + tag]), src
