#!/usr/bin/env python3
"""Mint tests/golden/amp_learner_ref.npz from the reference's AMP learner.  TEST INFRASTRUCTURE ONLY.

Runs only where the reference checkout is mounted (oracle/ref_harness.py).  Imported from where they lie, never copied:

  learning/amp_continuous.py       AMPAgent._disc_loss, _disc_loss_neg / _pos, _compute_disc_acc, _calc_disc_rewards, _eval_disc,
                                   _preproc_amp_obs, _combine_rewards, _store_replay_amp_obs
  learning/amp_network_builder.py  AMPBuilder.Network.eval_disc, get_disc_weights, get_disc_logit_weights
  learning/replay_buffer.py        ReplayBuffer

The names those modules import and this script never calls are empty stand-ins: `rl_games.*`, `tensorboardX`,
`learning.common_agent` (CommonAgent = object) and `isaacgym.torch_utils`, whose only member used here, `to_torch`, is a one-line
helper of our own.  The reference's methods are called unbound on a stub learner whose `model.a2c_network` carries the
`_disc_mlp` / `_disc_logits` of an `isaacgymdyros_amd.amp_disc.DiscNet` and AMPBuilder.Network's own methods.

rl_games' RunningMeanStd is not in the reference's checkout, so the rows are normalised with `amp_disc.RunningMeanStd`, the
repository's restatement (tests/golden/README.md lists it under "Not pinned").  Everything downstream of the normalised rows is
the reference's own code: the fp32 loss and its gradient, the same in float64 on the same normalised rows, the rewards, the
buffers.  `compute()` is also what tests/test_amp_disc_reference.py calls live where the reference is mounted.

usage: python oracle/make_amp_learner_goldens.py        (twice gives the same bytes: fixed seeds, one CPU thread, fixed zip dates)
"""
from __future__ import annotations

import copy
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_harness as RH                                 # noqa: E402  (paths only)
from isaacgymdyros_amd import amp_disc as AD                          # noqa: E402

LEARNING = os.path.join(RH.IGE, "learning")
OUT = os.path.join(ROOT, "tests", "golden", "amp_learner_ref.npz")
DIMS = (34, 68)
ROWS = (67, 29, 38)          # agent, replay, demo: none a multiple of 4, 64 or 128
REWARD_ROWS = 61
COEF = dict(disc_coef=5.0, logit_reg=0.05, grad_penalty=0.1, weight_decay=1e-4)          # cfg/train/TocabiAMPLowerPPO.yaml
REWARD = dict(scale=2.0, task_w=0.7, disc_w=0.3)
REWARD_B3_SHIFT = 5.5          # the reward case's logit bias: the grad case's + this
# Units of each hidden layer that are live; the rest have zero weights and bias, so their pre-activation is exactly 0 on every row.  66 of
# 256, spread over both 128-wide tiles and including the first and last unit of each: the gradient has ~9 k non-zero entries at D = 68
# instead of ~84 k, which keeps the fixture small.
LIVE = tuple(i for i in range(AD.HID) if i % 4 == 3 or i % 128 == 0)
Q = 2.0 ** -10          # weights and raw rows are multiples of Q: exact in fp32, and short mantissas store compactly


def available() -> bool:
    return all(os.path.isfile(os.path.join(LEARNING, f)) for f in ("amp_continuous.py", "amp_network_builder.py", "replay_buffer.py"))


_ref = {}


def load_reference():
    """(AMPAgent, AMPBuilder.Network, the replay_buffer module), imported from the checkout with stand-ins for what they import.  The
    stand-ins are removed from sys.modules again afterwards, so nothing else in the process sees them."""
    if _ref:
        return _ref["agent"], _ref["network"], _ref["replay"]
    if not available():
        raise RuntimeError("reference checkout not present")
    before = dict(sys.modules)

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class A2CBuilder:
        class Network:
            pass
    mod("rl_games")
    mod("rl_games.algos_torch", torch_ext=mod("rl_games.algos_torch.torch_ext"), layers=mod("rl_games.algos_torch.layers"),
        network_builder=mod("rl_games.algos_torch.network_builder", A2CBuilder=A2CBuilder),
        running_mean_std=mod("rl_games.algos_torch.running_mean_std", RunningMeanStd=None))
    mod("rl_games.common", a2c_common=mod("rl_games.common.a2c_common"), schedulers=mod("rl_games.common.schedulers"),
        vecenv=mod("rl_games.common.vecenv"))

    def to_torch(x, dtype=torch.float, device="cuda:0", requires_grad=False):
        return torch.tensor(x, dtype=dtype, device=device, requires_grad=requires_grad)
    tu = mod("isaacgym.torch_utils", to_torch=to_torch)
    tu.__all__ = ["to_torch"]
    mod("isaacgym", torch_utils=tu)
    mod("tensorboardX", SummaryWriter=None)
    learning = mod("learning")
    learning.__path__ = [LEARNING]
    learning.common_agent = mod("learning.common_agent", CommonAgent=object)
    try:
        rb = RH._load("learning.replay_buffer", os.path.join(LEARNING, "replay_buffer.py"))
        nb = RH._load("learning.amp_network_builder", os.path.join(LEARNING, "amp_network_builder.py"))
        ac = RH._load("learning.amp_continuous", os.path.join(LEARNING, "amp_continuous.py"))
    finally:
        for k in set(sys.modules) - set(before):
            del sys.modules[k]
        sys.modules.update(before)
    _ref.update(agent=ac.AMPAgent, network=nb.AMPBuilder.Network, replay=rb)
    return _ref["agent"], _ref["network"], _ref["replay"]


def stub_learner(net: AD.DiscNet, rms=None):
    """A learner carrying only what the called methods read; `net`'s layers on an a2c_network with AMPBuilder.Network's methods."""
    Agent, Network, _ = load_reference()

    class A2CNetwork(torch.nn.Module):
        eval_disc = Network.eval_disc
        get_disc_weights = Network.get_disc_weights
        get_disc_logit_weights = Network.get_disc_logit_weights

    a2c = A2CNetwork()
    a2c._disc_mlp, a2c._disc_logits = net._disc_mlp, net._disc_logits
    s = types.SimpleNamespace(model=types.SimpleNamespace(a2c_network=a2c), ppo_device="cpu", _normalize_amp_input=rms is not None,
                              _amp_input_mean_std=rms, _disc_logit_reg=COEF["logit_reg"], _disc_grad_penalty=COEF["grad_penalty"],
                              _disc_weight_decay=COEF["weight_decay"], _disc_coef=COEF["disc_coef"], _disc_reward_scale=REWARD["scale"],
                              _task_reward_w=REWARD["task_w"], _disc_reward_w=REWARD["disc_w"])
    for name in ("_disc_loss_neg", "_disc_loss_pos", "_compute_disc_acc", "_eval_disc", "_preproc_amp_obs"):
        setattr(s, name, types.MethodType(getattr(Agent, name), s))
    return s


def lively_net(D: int, seed: int) -> AD.DiscNet:
    """Weights a few times the initial scale (multiples of Q), non-zero biases, the units outside LIVE dead, and a logit bias that centres
    the logits so that both signs, the 1e-4 floor of the reward and large negative logits all occur."""
    g = torch.Generator().manual_seed(seed)
    net = AD.DiscNet(D)
    with torch.no_grad():
        for lin, fan in ((net._disc_mlp[0], D), (net._disc_mlp[2], AD.HID)):
            dead = torch.ones(AD.HID, dtype=torch.bool)
            dead[list(LIVE)] = False
            lin.weight.copy_(quantise((torch.rand(lin.weight.shape, generator=g) * 2 - 1) * 2.0 / np.sqrt(len(LIVE) if fan == AD.HID else fan)))
            lin.bias.copy_(quantise((torch.rand(lin.bias.shape, generator=g) * 2 - 1) * 0.3))
            lin.weight[dead] = 0.0
            lin.bias[dead] = 0.0
            if fan == AD.HID:
                lin.weight[:, dead] = 0.0          # (inputs from dead units carry nothing; a non-zero weight would only add weight decay)
        net._disc_logits.weight.copy_(quantise(torch.rand(net._disc_logits.weight.shape, generator=g) * 2 - 1))
        net._disc_logits.bias.fill_(-4.0)
    return net


def quantise(x):
    return torch.round(x / Q) * Q if torch.is_tensor(x) else (np.round(x / Q) * Q).astype(np.float32)


def params(net):
    return [net._disc_mlp[0].weight, net._disc_mlp[0].bias, net._disc_mlp[2].weight, net._disc_mlp[2].bias, net._disc_logits.weight,
            net._disc_logits.bias]


def flat(ts):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in ts])


def ref_loss(net, an, rn, dn):
    """calc_gradients' discriminator share as the reference writes it: logits by eval_disc per set, _disc_loss, disc_coef * disc_loss,
    autograd to every parameter.  Returns (flat gradient, the logged values)."""
    Agent, _, _ = load_reference()
    s = stub_learner(net)
    a2c = s.model.a2c_network
    dn = dn.detach().clone().requires_grad_(True)          # (calc_gradients: amp_obs_demo.requires_grad_(True) after the normalisation)
    agent_logit = torch.cat([a2c.eval_disc(an), a2c.eval_disc(rn)], dim=0)
    demo_logit = a2c.eval_disc(dn)
    info = Agent._disc_loss(s, agent_logit, demo_logit, dn)
    total = s._disc_coef * info["disc_loss"]
    grads = torch.autograd.grad(total, params(net))
    with torch.no_grad():
        pred = 0.5 * (s._disc_loss_neg(agent_logit) + s._disc_loss_pos(demo_logit))
        wd = torch.sum(torch.square(torch.cat(a2c.get_disc_weights(), dim=-1)))
        acc_a, acc_d = s._compute_disc_acc(agent_logit, demo_logit)
    vals = {"disc_loss": info["disc_loss"], "disc_grad_penalty": info["disc_grad_penalty"], "disc_logit_loss": info["disc_logit_loss"],
            "total": total, "pred": pred, "weight_decay_sum": wd, "agent_logit_mean": agent_logit.mean(), "demo_logit_mean": demo_logit.mean(),
            "agent_acc": acc_a, "demo_acc": acc_d}
    return flat(grads), {k: v.detach().numpy() for k, v in vals.items()}, agent_logit.detach().numpy()[:, 0], demo_logit.detach().numpy()[:, 0]


def grad_case(D: int, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    na, nr, nd = ROWS
    net = lively_net(D, seed)
    rms = AD.RunningMeanStd(D)
    with torch.no_grad():
        rms.running_mean.copy_(torch.from_numpy(rng.normal(size=D) * 0.5))
        rms.running_var.copy_(torch.from_numpy(rng.uniform(0.3, 3.0, size=D)))
        rms.count.fill_(2000.0)
    mu, sd = rms.running_mean.numpy().copy(), np.sqrt(rms.running_var.numpy())

    def rows(n, shift):
        return quantise(mu + sd * (rng.normal(size=(n, D)) * 1.5 + shift))
    a, r, d = rows(na, -0.4), rows(nr, -0.1), rows(nd, 0.5)
    a[:5] = quantise(mu + sd * rng.normal(size=(5, D)) * 40)          # rows clamped at +-5 after the normalisation
    d[:3] = quantise(mu + sd * rng.normal(size=(3, D)) * 40)
    out = {"p": flat(params(net)), "stats_in": np.concatenate([rms.running_mean.numpy(), rms.running_var.numpy(), rms.count.numpy()[None]]),
           "agent": a, "replay": r, "demo": d}
    # train mode, as calc_gradients: each set updates the statistics, then is normalised with what that update left
    rms.train()
    for name, x in (("agent", a), ("replay", r), ("demo", d)):
        with torch.no_grad():
            out["xn_" + name] = rms(torch.from_numpy(x)).numpy()
        out["stats_" + name] = np.concatenate([rms.running_mean.numpy(), rms.running_var.numpy(), rms.count.numpy()[None]])
    an, rn, dn = (torch.from_numpy(out["xn_" + k]) for k in ("agent", "replay", "demo"))
    assert (an.abs() == 5).any() and (dn.abs() == 5).any()
    out["grad32"], vals32, la, ld = ref_loss(net, an, rn, dn)
    out["agent_logit32"], out["demo_logit32"] = la, ld
    out["grad64"], vals64, _, _ = ref_loss(copy.deepcopy(net).double(), an.double(), rn.double(), dn.double())
    for k in vals32:
        out["val32_" + k], out["val64_" + k] = vals32[k], vals64[k]
    assert (la < 0).any() and (la > 0).any() and (ld < 0).any() and (ld > 0).any()
    return out


def reward_case(D: int, seed: int, g: dict) -> dict:
    """_calc_disc_rewards + _combine_rewards in eval mode on raw rows, with the network of the grad case (its logit bias raised by
    REWARD_B3_SHIFT, so that the 1e-4 floor is reached) and its last statistics snapshot, fp32 (the reference) and float64 (the same methods
    on the fp32-normalised rows, normalisation off)."""
    rng = np.random.default_rng(seed)
    net = lively_net(D, 1000 + D)
    with torch.no_grad():
        net._disc_logits.bias += REWARD_B3_SHIFT
    rms = AD.RunningMeanStd(D)
    st = g["stats_demo"]
    with torch.no_grad():
        rms.running_mean.copy_(torch.from_numpy(st[:D]))
        rms.running_var.copy_(torch.from_numpy(st[D:2 * D]))
        rms.count.fill_(float(st[2 * D]))
    rms.eval()
    B = REWARD_ROWS
    x = quantise(st[:D] + np.sqrt(st[D:2 * D]) * rng.normal(size=(B, D)) * 1.5)
    x[:4] = quantise(st[:D] + np.sqrt(st[D:2 * D]) * rng.normal(size=(4, D)) * 40)
    task = rng.normal(size=(B, 1)).astype(np.float32)
    return dict(reward_eval(net, rms, x, task), reward_b3=net._disc_logits.bias.detach().numpy().copy(), reward_x=x, reward_task=task,
                reward_stats=np.concatenate([rms.running_mean.numpy(), rms.running_var.numpy(), rms.count.numpy()[None]]))


def reward_eval(net, rms, x, task):
    Agent, _, _ = load_reference()
    s = stub_learner(net, rms)
    X, T = torch.from_numpy(x), torch.from_numpy(task)
    r32 = Agent._calc_disc_rewards(s, X)
    c32 = Agent._combine_rewards(s, T, {"disc_rewards": r32})
    with torch.no_grad():
        xn = rms(X)
        l32 = s.model.a2c_network.eval_disc(xn)
    s64 = stub_learner(copy.deepcopy(net).double())
    xn64 = xn.double()
    r64 = Agent._calc_disc_rewards(s64, xn64)
    c64 = Agent._combine_rewards(s64, T.double(), {"disc_rewards": r64})
    with torch.no_grad():
        l64 = s64.model.a2c_network.eval_disc(xn64)
    return {"reward_xn": xn.numpy(), "reward_logit32": l32.numpy()[:, 0], "reward_logit64": l64.numpy()[:, 0], "disc_r32": r32.numpy()[:, 0],
            "combined32": c32.numpy()[:, 0], "disc_r64": r64.numpy()[:, 0], "combined64": c64.numpy()[:, 0]}


def probe_case() -> dict:
    """A network whose logit is exactly 4 x_0 (x_0 normalised with mean 0 and var + 1e-5 == 1 in fp32, so unchanged but clamped at +-5):
    logits -20 .. 20 through the floor, large negative values and values near 0, identical in fp32 and float64, so that the reward
    formula is what is compared."""
    D = 34
    net = AD.DiscNet(D)
    with torch.no_grad():
        for t in params(net):
            t.zero_()
        net._disc_mlp[0].weight[0, 0], net._disc_mlp[0].weight[1, 0] = 1.0, -1.0
        net._disc_mlp[2].weight[0, 0], net._disc_mlp[2].weight[1, 1] = 1.0, 1.0
        net._disc_logits.weight[0, 0], net._disc_logits.weight[0, 1] = 4.0, -4.0
    rms = AD.RunningMeanStd(D)
    with torch.no_grad():
        rms.running_var.fill_(float(np.float32(1.0 - AD.RMS_EPS)))
        rms.count.fill_(100.0)
    rms.eval()
    x0 = np.concatenate([[-5.0, -4.0, -3.0, -1.0, -0.25, -1e-3, -1e-6, 0.0, 1e-6, 1e-3, 0.25, 1.0, 2.0, 2.25, 2.29, 2.3, 2.3025, 2.31,
                          2.35, 2.5, 3.0, 4.0, 5.0], np.linspace(-5, 5, 41)]).astype(np.float32)
    B = len(x0)
    rng = np.random.default_rng(7)
    x = rng.normal(size=(B, D)).astype(np.float32)
    x[:, 0] = x0
    task = rng.normal(size=(B, 1)).astype(np.float32)
    out = reward_eval(net, rms, x, task)
    assert np.array_equal(out["reward_logit32"], 4 * x0) and np.array_equal(out["reward_logit64"], 4 * x0.astype(np.float64))
    out = {"probe_" + k[len("reward_"):] if k.startswith("reward_") else "probe_" + k: v for k, v in out.items()}
    out.update(probe_p=flat(params(net)), probe_x=x, probe_task=task,
               probe_stats=np.concatenate([rms.running_mean.numpy(), rms.running_var.numpy(), rms.count.numpy()[None]]))
    return out


def replay_case() -> dict:
    """A store / sample / wrap sequence of the reference's ReplayBuffer and _store_replay_amp_obs' keep-probability path, under the
    seeded global torch generator (what the reference draws its permutations and Bernoulli draws from)."""
    Agent, _, RB = load_reference()
    out = {}
    torch.manual_seed(20261015)
    buf = RB.ReplayBuffer(23, "cpu")
    out["replay_perm0"] = buf._sample_idx.numpy().copy()
    rows = torch.arange(200, dtype=torch.float32)[:, None] * torch.tensor([[1.0, -1.0, 0.5]])
    seq, k, samples = [("store", 9), ("sample", 5), ("sample", 7), ("store", 10), ("sample", 12), ("store", 8), ("sample", 6),
                       ("sample", 17), ("store", 22), ("sample", 23), ("sample", 4)], 0, []
    for op, n in seq:
        if op == "store":
            buf.store({"amp_obs": rows[k:k + n]})
            k += n
        else:
            samples.append(buf.sample(n)["amp_obs"].numpy())
    out["replay_seq"] = np.array([[op == "store", n] for op, n in seq], np.int64)
    out["replay_samples"] = np.concatenate(samples)
    out["replay_data"] = buf._data_buf["amp_obs"].numpy().copy()
    out["replay_head"] = np.array([buf._head, buf._total_count, buf._sample_head], np.int64)
    # _store_replay_amp_obs: once more rows have been stored than the buffer holds, each row is kept with amp_replay_keep_prob
    torch.manual_seed(20261016)
    s = types.SimpleNamespace(_amp_replay_buffer=RB.ReplayBuffer(50, "cpu"), _amp_replay_keep_prob=0.25, ppo_device="cpu")
    keep_rows = torch.arange(30 * 5, dtype=torch.float32).reshape(5, 30, 1) + 1000
    counts = []
    for i in range(5):
        Agent._store_replay_amp_obs(s, keep_rows[i])
        counts.append(s._amp_replay_buffer.get_total_count())
    out["keep_counts"] = np.array(counts, np.int64)
    out["keep_data"] = s._amp_replay_buffer._data_buf["amp_obs"].numpy().copy()
    out["keep_head"] = np.array(s._amp_replay_buffer._head, np.int64)
    return out


def compute() -> dict:
    """Every array of the fixture (keys "<D>/<name>" per dimension, the rest flat)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # (one summation order for the CPU products, wherever this runs)
    try:
        out = {}
        for D in DIMS:
            g = grad_case(D, 1000 + D)
            g.update(reward_case(D, 2000 + D, g))
            out.update({"%d/%s" % (D, k): np.asarray(v) for k, v in g.items()})
        out.update({k: np.asarray(v) for k, v in probe_case().items()})
        out.update({k: np.asarray(v) for k, v in replay_case().items()})
        return out
    finally:
        torch.set_num_threads(threads)


def save(path: str, arrays: dict):
    """np.savez_compressed's format with a fixed member date and order, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, b.getvalue())


def main():
    out = compute()
    save(OUT, out)
    for D in DIMS:
        la, ld, lr = out["%d/agent_logit32" % D], out["%d/demo_logit32" % D], out["%d/reward_logit32" % D]
        print("D=%d: agent logits %.2f .. %.2f, demo %.2f .. %.2f, reward logits %.2f .. %.2f (%d at the floor), |g64| max %.3g" % (
            D, la.min(), la.max(), ld.min(), ld.max(), lr.min(), lr.max(), int((lr > np.log(1e4)).sum()), np.abs(out["%d/grad64" % D]).max()))
    print("%s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
