"""The actor-critic's loss and its analytic backward (CPU): tests/amp_policy_truth.py against torch autograd in float64, and the torch
backend of AmpActorCritic against examples/amp_consumer.py's inline minibatch loop, bit for bit."""
import importlib.util
import math
import os
import sys

import pytest
import torch

from isaacgymdyros_amd import amp_disc as AD
from isaacgymdyros_amd import amp_policy as AP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amp_policy_truth as T          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def consumer():
    spec = importlib.util.spec_from_file_location("amp_consumer_example", os.path.join(ROOT, "examples", "amp_consumer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case(B, D, A, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = AP.ActorCritic(D, A, [512, 512], -1.6).double()
    with torch.no_grad():
        net.mu.bias[:] = torch.tensor([1.2, -1.2] * A, dtype=torch.float64)[:A]          # mu beyond +-1
        net.mu.weight.mul_(8.0)
    xn = torch.randn(B, D, generator=g, dtype=torch.float64)
    P = net.params_in_layout()
    with torch.no_grad():
        _, _, _, _, mu, _ = T.forward(xn, P)
        act = mu + 0.2 * torch.randn(B, A, generator=g, dtype=torch.float64)
        nlp = net.neglogp(act, mu)
    shift = torch.randn(B, generator=g, dtype=torch.float64) * 0.3
    shift[: B // 4] = 0.0          # ratio exactly 1: inside the clip range, the two surrogate terms tie
    old = nlp + shift
    adv = torch.randn(B, generator=g, dtype=torch.float64)
    ret = torch.randn(B, generator=g, dtype=torch.float64)
    return net, xn, act, old, adv, ret


@pytest.mark.parametrize("B,D,A", [(64, 20, 4), (97, 33, 12), (40, 1, 1)])
def test_analytic_backward_matches_autograd_float64(B, D, A):
    net, xn, act, old, adv, ret = case(B, D, A, seed=B + D)
    P = net.params_in_layout()
    loss, logs, grads, scales, peaks = T.loss_and_grad(xn, [p.detach() for p in P], net.sigma.detach(), act, old, adv, ret)
    for p, s, pk in zip(P, scales, peaks):
        assert s.numel() == p.numel() and pk.numel() == p.numel()
    # torch autograd of the consumer's expressions on the same (already normalised) rows
    mu = net.mu(net.actor_mlp(xn))
    v = net.value(net.critic_mlp(xn))
    ratio = torch.exp(old - net.neglogp(act, mu))
    a_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - 0.2, 1 + 0.2)).mean()
    c_loss = ((ret.view(-1, 1) - v) ** 2).mean()
    b_loss = ((torch.clamp(mu - 1.0, min=0) ** 2 + torch.clamp(mu + 1.0, max=0) ** 2).sum(-1)).mean()
    ref = a_loss + 5 * c_loss + 10 * b_loss
    ref_g = torch.autograd.grad(ref, P)
    assert abs(loss.item() - ref.item()) <= 1e-12 * max(1.0, abs(ref.item()))
    for x, y in zip(logs[:3], (a_loss, c_loss, b_loss)):
        assert abs(x.item() - y.item()) <= 1e-12 * max(1.0, abs(y.item()))
    for i, (h, r) in enumerate(zip(grads, ref_g)):
        h = h.reshape(r.shape)
        scale = r.abs().max().item()
        assert scale > 0 or i in (0, 1, 6, 7), i
        assert (h - r).abs().max().item() <= 1e-10 * max(scale, 1e-300), (i, (h - r).abs().max().item(), scale)
    # the cases the kernel distinguishes are all present
    with torch.no_grad():
        r = torch.exp(old - net.neglogp(act, mu))
        assert bool((r == 1).any()) and bool((r > 1.2).any()) and bool((r < 0.8).any())
        assert bool((mu.abs() > 1).any()) and (A == 1 or (bool((mu > 1).any()) and bool((mu < -1).any())))


def test_torch_update_equals_the_consumers_inline_loop():
    C = consumer()
    D, A, B, nmb = 24, 5, 64, 3
    g = torch.Generator().manual_seed(11)
    obs = torch.randn(nmb * B, D, generator=g) * 2 + 0.5
    act = torch.randn(nmb * B, A, generator=g)
    nlp_b = torch.randn(nmb * B, generator=g)
    adv_b = torch.randn(nmb * B, 1, generator=g)
    ret_n = torch.randn(nmb * B, 1, generator=g)
    lr, e_clip = 3e-4, 0.2
    torch.manual_seed(7)
    model = C.ActorCritic(D, A, [512, 512], -1.6)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, eps=1e-8)
    for pg in opt.param_groups:
        pg["lr"] = lr
    model.train()
    model.value_rms.eval()
    losses = []
    for i in range(0, nmb * B, B):          # (examples/amp_consumer.py train(), the minibatch loop)
        s = slice(i, i + B)
        mu, v = model(obs[s])
        ratio = torch.exp(nlp_b[s] - model.neglogp(act[s], mu))
        a = adv_b[s].view(-1)
        a_loss = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - e_clip, 1 + e_clip)).mean()
        c_loss = ((ret_n[s] - v) ** 2).mean()
        b_loss = ((torch.clamp(mu - 1.0, min=0) ** 2 + torch.clamp(mu + 1.0, max=0) ** 2).sum(-1)).mean()
        loss = a_loss + 5.0 * c_loss + 10.0 * b_loss
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(torch.stack([a_loss.detach(), c_loss.detach(), b_loss.detach()]))
    pol = AP.AmpActorCritic(D, A, "cpu", backend="torch", seed=7)
    for i in range(0, nmb * B, B):
        s = slice(i, i + B)
        pol.update(obs[s], act[s], nlp_b[s], adv_b[s].reshape(-1), ret_n[s].reshape(-1), lr=lr)
    ref = model.state_dict()
    got = pol.state_dict()
    assert sorted(ref) == sorted(got)
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
    info = pol.pop_info()
    al, cl, bl = torch.stack(losses).mean(0).tolist()
    assert math.isclose(info["a_loss"], al, rel_tol=1e-6) and math.isclose(info["c_loss"], cl, rel_tol=1e-6)
    assert math.isclose(info["b_loss"], bl, rel_tol=1e-6, abs_tol=1e-12)


def test_checkpoints_load_across_forms():
    C = consumer()
    torch.manual_seed(3)
    model = C.ActorCritic(30, 6, [512, 512], -1.6)
    pol = AP.AmpActorCritic(30, 6, "cpu", backend="torch", seed=4)
    pol.load_state_dict(model.state_dict())
    for k, v in model.state_dict().items():
        assert torch.equal(pol.state_dict()[k], v), k
    model.load_state_dict(pol.state_dict())


def test_torch_gae_is_the_consumers_loop():
    H, N, gamma, tau = 8, 5, 0.99, 0.95
    g = torch.Generator().manual_seed(2)
    done = (torch.rand(H, N, generator=g) < 0.3).float()
    val, rew, nxt = (torch.randn(H, N, 1, generator=g) for _ in range(3))
    adv, ret = AP.gae(done, val, rew, nxt, gamma, tau, backend="torch")
    ref = torch.zeros_like(rew)
    last = torch.zeros(N, 1)
    for t in reversed(range(H)):
        delta = rew[t] + gamma * nxt[t] - val[t]
        last = delta + gamma * tau * (1.0 - done[t]).view(N, 1) * last
        ref[t] = last
    assert torch.equal(adv, ref) and torch.equal(ret, ref + val)


def test_argument_checks_on_the_cpu():
    with pytest.raises(ValueError):
        AP.AmpActorCritic(0, 4, "cpu", backend="torch")
    with pytest.raises(ValueError):
        AP.AmpActorCritic(20, 4, "cpu", backend="hip")
    with pytest.raises(ValueError):
        AP.AmpActorCritic(20, 4, "cpu", backend="jax")
    cfg = {"network": dict(AD.TRAIN_CFG["network"], mlp_units=[256, 256]), "config": AD.TRAIN_CFG["config"]}
    with pytest.raises(ValueError):
        AP.AmpActorCritic(20, 4, "cpu", cfg=cfg, backend="torch")
    pol = AP.AmpActorCritic(20, 4, "cpu", backend="torch", seed=0)
    with pytest.raises(ValueError):
        pol.act(torch.zeros(3, 20), torch.zeros(3, 5))
    with pytest.raises(ValueError):
        pol.update_value_stats(torch.zeros(3, 1), torch.zeros(4, 1))
