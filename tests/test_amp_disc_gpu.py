"""The HIP discriminator (dwd_reward, dwd_stats, dwd_grad, dwd_opt) against the torch form of isaacgymdyros_amd/amp_disc.py on an MI355X."""
import copy

import numpy as np
import pytest
import torch

from isaacgymdyros_amd import amp_disc as AD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def pair(D, cfg=None, seed=0):
    h = AD.AmpDiscriminator(D, DEV, cfg, backend="hip", seed=seed)
    t = AD.AmpDiscriminator(D, DEV, cfg, backend="torch", seed=seed + 1)
    t.load_state_dict(h.state_dict())
    return h, t


def set_stats(d, rng):
    D = d.D
    sd = d.state_dict()
    sd["_amp_input_mean_std.running_mean"] = torch.from_numpy(rng.normal(size=D) * 0.3)
    sd["_amp_input_mean_std.running_var"] = torch.from_numpy(rng.uniform(0.2, 3.0, size=D))
    sd["_amp_input_mean_std.count"] = torch.tensor(1000.0, dtype=torch.float64)
    d.load_state_dict(sd)


def abs_logit64(d, xn):
    """The logit computed with |W|, |b| and |x| in float64: S = sum |a b| through the three layers.  A fp32 evaluation of the network in any
    summation order differs from the exact one by at most about (D + 2 * 256 + 8) u S (first order in u = 2^-24, nested dot products)."""
    sd = {k: v.double().abs() for k, v in d.state_dict().items()}
    h1 = torch.relu(xn.double().abs() @ sd["_disc_mlp.0.weight"].T.to(xn.device) + sd["_disc_mlp.0.bias"].to(xn.device))
    h2 = h1 @ sd["_disc_mlp.2.weight"].T.to(xn.device) + sd["_disc_mlp.2.bias"].to(xn.device)
    return h2 @ sd["_disc_logits.weight"].T.to(xn.device) + sd["_disc_logits.bias"].to(xn.device)


@pytest.mark.parametrize("D", [34, 68, 102, 136, 340])
@pytest.mark.parametrize("B", [1, 17, 4096, 131072])
def test_reward_matches_torch(B, D):
    h, t = pair(D, seed=B + D)
    rng = np.random.default_rng(B * 7 + D)
    set_stats(h, rng)
    t.load_state_dict(h.state_dict())
    x = torch.from_numpy(rng.normal(size=(1, B, D)).astype(np.float32) * 2).to(DEV)
    task = torch.from_numpy(rng.normal(size=(1, B, 1)).astype(np.float32)).to(DEV)
    if B >= 17:
        x[0, :5] *= 40.0                                   # rows clamped at +-5 after normalisation
    ch, rh, lh = h.rewards(x, task, return_logits=True)
    ct, rt, lt = t.rewards(x, task, return_logits=True)
    t.rms.eval()
    bound = 2 * (D + 2 * 256 + 8) * U * abs_logit64(h, t.rms(x[0]))
    assert (lh[0].double() - lt[0].double()).abs().le(bound + 1e-30).all(), float(((lh[0] - lt[0]).abs() / bound).max())
    # disc_r and combined: the same fp32 formula on logits that agree within the bound
    assert torch.allclose(rh, rt, rtol=1e-4, atol=1e-4 + float(bound.max()) * 2)
    assert torch.allclose(ch, ct, rtol=1e-4, atol=1e-4 + float(bound.max()) * 2)
    # the 1e-4 floor: a logit bias far past it gives -log(1e-4) * scale exactly as torch computes it
    sd = h.state_dict()
    sd["_disc_logits.bias"] = torch.tensor([40.0])
    h.load_state_dict(sd)
    t.load_state_dict(sd)
    ch, rh = h.rewards(x, task)
    ct, rt = t.rewards(x, task)
    assert torch.equal(rh, rt) and float(rh[0, 0, 0]) == pytest.approx(-np.log(np.float32(1e-4)) * 2, rel=1e-6)
    assert torch.allclose(ch, ct, rtol=0, atol=1e-6)


def test_stats_three_updates():
    h, t = pair(68)
    rng = np.random.default_rng(1)
    for n in (513, 4096, 77):
        x = torch.from_numpy((rng.normal(size=(n, 68)) * 3 + rng.normal(size=68)).astype(np.float32)).to(DEV)
        h._check(h.api["stats"](x.data_ptr(), n, 68, h.stats.data_ptr(), h.stats.data_ptr(), h._swork.data_ptr(), h._stream()))
        t.rms.train()
        t.rms(x.double())                                 # the restatement on fp64 moments: what the kernel accumulates in
        assert torch.allclose(h.stats[:68], t.rms.running_mean, rtol=1e-9, atol=1e-12)
        assert torch.allclose(h.stats[68:136], t.rms.running_var, rtol=1e-9, atol=0)
        assert float(h.stats[136]) == float(t.rms.count)


def batch(rng, n, D, shift):
    return torch.from_numpy((rng.normal(size=(n, D)) + shift).astype(np.float32)).to(DEV)


def cfg_with(**kw):
    return {"network": AD.TRAIN_CFG["network"], "config": dict(AD.TRAIN_CFG["config"], **kw)}


def grads_agree(h, t, a, r, d):
    h.accumulate_grad(a, r, d)
    t.accumulate_grad(a, r, d)
    assert torch.allclose(h.stats, t.stats, rtol=1e-5, atol=1e-6)
    o = 0
    for p in h._params_in_layout():
        n = p.numel()
        gh, gt = h.g[o:o + n], t.g[o:o + n]
        tol = 2e-4 * float(gt.abs().max()) + 1e-7
        assert float((gh - gt).abs().max()) <= tol, (o, float((gh - gt).abs().max()), tol)
        o += n
    sh, st = h.state[:10], t.state[:10]
    assert torch.allclose(sh, st, rtol=1e-3, atol=1e-4), (sh, st)


@pytest.mark.parametrize("term", ["pred", "logit_reg", "grad_penalty", "weight_decay", "full"])
def test_grad_terms_against_autograd(term):
    zero = dict(disc_logit_reg=0.0, disc_grad_penalty=0.0, disc_weight_decay=0.0)
    cfg = cfg_with(**(zero if term == "pred" else {} if term == "full" else dict(zero, **{"disc_" + term: AD.TRAIN_CFG["config"]["disc_" + term]})))
    h, t = pair(68, cfg, seed=3)
    rng = np.random.default_rng(4)
    a, r, d = batch(rng, 1000, 68, -0.3), batch(rng, 700, 68, -0.1), batch(rng, 900, 68, 0.4)
    grads_agree(h, t, a, r, d)


def test_grad_at_the_yaml_minibatch_shape():
    """amp_minibatch_size 131 072 with numAMPObsSteps 2 (cfg/train/TocabiAMPLowerPPO.yaml): 3 x 131 072 rows at D = 68, 64 slabs.  (Against
    float64: tests/test_amp_disc_reference_gpu.py.)"""
    h, t = pair(68, seed=13)
    rng = np.random.default_rng(14)
    grads_agree(h, t, batch(rng, 131072, 68, -0.2), batch(rng, 131072, 68, 0.0), batch(rng, 131072, 68, 0.3))


def test_grad_at_8192_rows_d102():
    h, t = pair(102, seed=5)
    rng = np.random.default_rng(6)
    grads_agree(h, t, batch(rng, 8192, 102, -0.2), batch(rng, 8192, 102, 0.0), batch(rng, 8192, 102, 0.3))


def test_adam_five_steps():
    h, t = pair(68, seed=7)
    rng = np.random.default_rng(8)
    for k in range(5):
        g = torch.from_numpy(rng.normal(size=h.g.numel()).astype(np.float32) * 1e-2).to(DEV)
        h.g.copy_(g)
        t.g.copy_(g)
        h.step(1e-4 * (5 - k))
        t.step(1e-4 * (5 - k))
        assert torch.allclose(h.p, t.p, rtol=1e-6, atol=1e-8), float((h.p - t.p).abs().max())
        assert not h.g.any()
    assert float(h.state[AD.K["DWD_S_STEP"]]) == 5


def test_learns_two_separable_clouds():
    h = AD.AmpDiscriminator(68, DEV, backend="hip", seed=9)
    g = torch.Generator(device=DEV).manual_seed(0)
    for i in range(300):
        a = torch.randn(512, 68, generator=g, device=DEV) - 0.5
        dm = torch.randn(512, 68, generator=g, device=DEV) + 0.5
        h.update(a, h.replay_batch(a), dm, lr=1e-4)
        if i == 199:
            h.pop_info()
    info = h.pop_info()
    assert all(np.isfinite(v) for v in info.values()), info
    assert info["disc_agent_acc"] > 0.9 and info["disc_demo_acc"] > 0.9, info
    assert torch.isfinite(h.p).all()


def test_graph_replay_is_bit_identical_to_eager():
    """dwd_reward + one update (three dwd_stats, dwd_grad, dwd_opt) captured on one stream, replayed: the same bits as the eager launches."""
    rng = np.random.default_rng(10)
    H, N, D = 4, 256, 68
    x = torch.from_numpy(rng.normal(size=(H, N, D)).astype(np.float32)).to(DEV)
    task = torch.from_numpy(rng.normal(size=(H, N, 1)).astype(np.float32)).to(DEV)
    a, r, d = batch(rng, 512, D, -0.2), batch(rng, 512, D, 0.0), batch(rng, 512, D, 0.3)
    h = AD.AmpDiscriminator(D, DEV, backend="hip", seed=11)
    h.set_lr(1e-4)
    start = copy.deepcopy(h.state_dict())
    # eager
    c0, r0 = h.rewards(x, task)
    h.update(a, r, d)
    eager = (c0.clone(), r0.clone(), h.p.clone(), h.m.clone(), h.v.clone(), h.stats.clone(), h.state.clone())
    # capture (warm-up on a side stream as torch.cuda.graph wants, then back to the start)
    h.load_state_dict(start)
    for t_ in (h.m, h.v, h.g):
        t_.zero_()
    h.state.zero_()
    h.set_lr(1e-4)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        h.rewards(x, task)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c1, r1 = h.rewards(x, task)
        h.update(a, r, d)
    torch.cuda.synchronize()
    h.load_state_dict(start)
    for t_ in (h.m, h.v, h.g):
        t_.zero_()
    h.state.zero_()
    h.set_lr(1e-4)
    graph.replay()
    torch.cuda.synchronize()
    got = (c1, r1, h.p, h.m, h.v, h.stats, h.state)
    for e, g_ in zip(eager, got):
        assert torch.equal(e, g_)


def test_bad_arguments_raise_value_error():
    h = AD.AmpDiscriminator(68, DEV, backend="hip", seed=12)
    x = torch.zeros(2, 8, 68, device=DEV)
    task = torch.zeros(2, 8, 1, device=DEV)
    rows = torch.zeros(16, 68, device=DEV)
    bad = [lambda: h.rewards(x.double(), task), lambda: h.rewards(x.cpu(), task), lambda: h.rewards(x[:, :, :34], task),
           lambda: h.rewards(x.transpose(0, 1), task), lambda: h.rewards(x, task[:, :4]), lambda: h.rewards(x, task.half()),
           lambda: h.rewards(x[0], task), lambda: h.update(rows.half(), rows, rows), lambda: h.update(rows, rows[:, :34], rows),
           lambda: h.update(rows, rows, rows.t().contiguous().t()), lambda: h.update(rows, rows, rows[:1]), lambda: h.update(rows, rows.cpu(), rows),
           lambda: h.update(rows, rows, [[0.0] * 68] * 16)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert not h.g.any() and float(h.state[AD.K["DWD_S_UPDATES"]]) == 0
