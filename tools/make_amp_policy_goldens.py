#!/usr/bin/env python3
"""Mint tests/golden/amp_policy_ref.npz from the reference's learner.  TEST INFRASTRUCTURE ONLY.

Runs only where the reference checkout is mounted.  Imported from where it lies, never copied: learning/common_agent.py, whose
CommonAgent._actor_loss, _critic_loss, bound_loss and discount_values are called unbound on a stub learner.  The names that module
imports and this script never calls are empty stand-ins: `rl_games.*` (A2CAgent = object), `gym.spaces`, `tensorboardX` and
`learning.amp_datasets`.

The inputs are seeded and cover what the policy kernels distinguish: rows inside the clip range with the ratio exactly 1 (where
torch.max splits the gradient between the two equal surrogate terms), rows outside it on both sides, mu beyond +-1 on both sides, and
dones inside the horizon.  For fp32 and float64 the file holds the inputs, the three loss means, the clip fraction, the gradients of
the losses with respect to neglogp, value and mu (torch autograd of the reference's expressions) and discount_values' advantages.
`compute()` is also what tests/test_amp_policy_reference.py calls live where the reference is mounted.

The fixture's provenance and what it pins are described in DESIGN.md section 13.

usage: python tools/make_amp_policy_goldens.py        (twice gives the same bytes: fixed seeds, one CPU thread, fixed zip dates)
"""
from __future__ import annotations

import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_harness as RH          # noqa: E402  (paths only)

LEARNING = os.path.join(RH.IGE, "learning")
OUT = os.path.join(ROOT, "tests", "golden", "amp_policy_ref.npz")
B, A, H, N = 203, 12, 32, 37          # rows of the losses, actions; horizon and envs of GAE
E_CLIP, GAMMA, TAU = 0.2, 0.99, 0.95          # cfg/train/TocabiAMPLowerPPO.yaml


def available() -> bool:
    return os.path.isfile(os.path.join(LEARNING, "common_agent.py"))


_ref = {}


def load_reference():
    """CommonAgent, imported from the checkout with stand-ins for what it imports (removed from sys.modules again afterwards)."""
    if _ref:
        return _ref["agent"]
    if not available():
        raise RuntimeError("reference checkout not present")
    before = dict(sys.modules)

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod("rl_games")
    mod("rl_games.algos_torch", a2c_continuous=mod("rl_games.algos_torch.a2c_continuous", A2CAgent=object),
        torch_ext=mod("rl_games.algos_torch.torch_ext"), central_value=mod("rl_games.algos_torch.central_value"),
        running_mean_std=mod("rl_games.algos_torch.running_mean_std", RunningMeanStd=None))
    mod("rl_games.common", a2c_common=mod("rl_games.common.a2c_common"), datasets=mod("rl_games.common.datasets"),
        schedulers=mod("rl_games.common.schedulers"), vecenv=mod("rl_games.common.vecenv"))
    mod("gym", spaces=mod("gym.spaces"))
    mod("tensorboardX", SummaryWriter=None)
    learning = mod("learning")
    learning.__path__ = [LEARNING]
    learning.amp_datasets = mod("learning.amp_datasets")
    try:
        ca = RH._load("learning.common_agent", os.path.join(LEARNING, "common_agent.py"))
    finally:
        for k in set(sys.modules) - set(before):
            del sys.modules[k]
        sys.modules.update(before)
    _ref["agent"] = ca.CommonAgent
    return _ref["agent"]


def inputs(dtype) -> dict:
    g = torch.Generator().manual_seed(20261015)
    nlp = torch.randn(B, generator=g, dtype=torch.float64) * 3 + 10
    shift = torch.randn(B, generator=g, dtype=torch.float64) * 0.4
    shift[::4] = 0.0          # ratio exactly 1
    mu = torch.randn(B, A, generator=g, dtype=torch.float64) * 1.2          # beyond +-1 on both sides
    x = {"nlp": nlp, "old_nlp": nlp + shift, "adv": torch.randn(B, generator=g, dtype=torch.float64), "mu": mu,
         "value": torch.randn(B, 1, generator=g, dtype=torch.float64), "ret": torch.randn(B, 1, generator=g, dtype=torch.float64),
         "dones": (torch.rand(H, N, generator=g, dtype=torch.float64) < 0.1).to(torch.float64),
         "values": torch.randn(H, N, 1, generator=g, dtype=torch.float64), "rewards": torch.randn(H, N, 1, generator=g, dtype=torch.float64),
         "next_values": torch.randn(H, N, 1, generator=g, dtype=torch.float64)}
    return {k: v.to(dtype) for k, v in x.items()}


def compute() -> dict:
    """The reference's losses, gradients and advantages for both dtypes, keyed '<name>_<f32|f64>'."""
    Agent = load_reference()
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    out = {}
    try:
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            x = inputs(dt)
            s = types.SimpleNamespace(ppo=True, bounds_loss_coef=10, ppo_device="cpu", horizon_length=H, gamma=GAMMA, tau=TAU)
            nlp, mu, v = (x[k].clone().requires_grad_(True) for k in ("nlp", "mu", "value"))
            ai = Agent._actor_loss(s, x["old_nlp"], nlp, x["adv"], E_CLIP)
            a_loss = ai["actor_loss"].mean()
            c_loss = Agent._critic_loss(s, None, v, E_CLIP, x["ret"], False)["critic_loss"].mean()
            b_loss = Agent.bound_loss(s, mu).mean()
            out["a_loss_" + tag] = a_loss.detach().numpy()
            out["c_loss_" + tag] = c_loss.detach().numpy()
            out["b_loss_" + tag] = b_loss.detach().numpy()
            out["clip_frac_" + tag] = ai["actor_clip_frac"].numpy()
            out["d_a_nlp_" + tag] = torch.autograd.grad(a_loss, nlp)[0].numpy()
            out["d_c_value_" + tag] = torch.autograd.grad(c_loss, v)[0].numpy()
            out["d_b_mu_" + tag] = torch.autograd.grad(b_loss, mu)[0].numpy()
            out["gae_adv_" + tag] = Agent.discount_values(s, x["dones"], x["values"], x["rewards"], x["next_values"]).numpy()
            for k, t in x.items():
                out["in_%s_%s" % (k, tag)] = t.numpy()
    finally:
        torch.set_num_threads(n)
    return out


def save(path: str, arrays: dict):
    """np.savez with fixed member dates, so the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


if __name__ == "__main__":
    save(OUT, compute())
    print(OUT, os.path.getsize(OUT))
