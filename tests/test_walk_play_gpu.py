"""dwp_play (include/dyros_ppo.h) and WalkPolicy on the GPU: against float64 truth at every row-count edge of its two forms, the clamp and the noise
bit for bit, the row form against dwp_policy's mu, the torch backend, graph replay, and its argument errors."""
import importlib.util
import os

import pytest
import torch

from isaacgymdyros_amd import ppo_update as U
from isaacgymdyros_amd import walk_policy as WP

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 2, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 16384]


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def make(seed=0, backend="hip"):
    """A WalkPolicy with lively weights: mu reaches beyond +-1 in many rows, so the clamp acts."""
    g = torch.Generator().manual_seed(seed)
    net = WP.Actor()
    with torch.no_grad():
        for _name, p in net.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / p.shape[1] ** 0.5))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        net.mu.bias.mul_(2.5)
        net.sigma.fill_(-1.2)
    pol = WP.WalkPolicy(DEV, backend=backend)
    pol.load_state_dict(net.state_dict())
    return pol


def call(pol, obs, noise=None, with_mu=True):
    """dwp_play with NaN-filled outputs and workspace: (rc, clamped, mu)."""
    api, N = pol.api, obs.shape[0]
    cl = torch.full((N, U.ACT), float("nan"), device=DEV)
    mu = torch.full((N, U.ACT), float("nan"), device=DEV)
    nw = api["play_work_floats"](N)
    w = torch.full((max(nw, 1),), float("nan"), device=DEV)
    rc = api["play"](pol.p.data_ptr(), pol.p32f.data_ptr(), pol.logstd.data_ptr(), obs.data_ptr(), None if noise is None else noise.data_ptr(), N,
                     cl.data_ptr(), mu.data_ptr() if with_mu else None, w.data_ptr(), w.numel(), stream())
    return rc, cl, mu


def truth(pol, obs, dtype):
    net = WP.Actor().to(DEV)
    net.load_state_dict(pol.state_dict())
    net = net.to(dtype).eval()
    with torch.no_grad():
        return net(obs.to(dtype))


def within_128x(hip, f32, f64, what):
    e_hip = (hip.double() - f64).abs().max().item()
    e_32 = (f32.double() - f64).abs().max().item()
    assert e_hip <= 128 * e_32 + 1e-6 * max(f64.abs().max().item(), 1e-3), (what, e_hip, e_32)


def test_play_against_float64_clamp_and_noise():
    pol = make(1)
    for N in NS:
        g = torch.Generator().manual_seed(N)
        obs = (torch.randn(N, U.IN, generator=g) * 1.5).to(DEV)
        noise = torch.randn(N, U.ACT, generator=g).to(DEV)
        rc, cl, mu = call(pol, obs)
        assert rc == 0, pol.api["last_error"]()
        torch.cuda.synchronize()
        assert torch.isfinite(mu).all() and torch.isfinite(cl).all(), N
        within_128x(mu, truth(pol, obs, torch.float32), truth(pol, obs, torch.float64), N)
        if N >= 16:
            assert (mu.abs() > 1).any(), N          # (the clamp is exercised)
        assert torch.equal(cl, torch.clamp(mu, -1.0, 1.0)), N
        rc, cl2, mu2 = call(pol, obs, noise)
        assert rc == 0
        assert torch.equal(mu2, mu), N
        assert torch.equal(cl2, torch.clamp(mu2 + torch.exp(pol.logstd) * noise, -1.0, 1.0)), N
        rc, cl3, _ = call(pol, obs, with_mu=False)
        assert rc == 0 and torch.equal(cl3, cl), N


@pytest.mark.parametrize("N", [65, 4095, 4097, 16384])
def test_row_form_mu_is_dwp_policys_mu(N):
    pol = make(2)
    g = torch.Generator().manual_seed(N + 1)
    obs = (torch.randn(N, U.IN, generator=g) * 1.5).to(DEV)
    _rc, _cl, mu = call(pol, obs)
    mu_p, val = torch.full((N, U.ACT), float("nan"), device=DEV), torch.empty(N, 1, device=DEV)
    assert pol.api["policy"](obs.data_ptr(), pol.p.data_ptr(), pol.p32f.data_ptr(), N, mu_p.data_ptr(), val.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(mu, mu_p)


def test_a_fused_learners_weights_play_without_repacking():
    """FusedPpoUpdate's own p / p32f are what dwp_play reads: WalkPolicy.from_module of its network gives the same bits."""
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    ppo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ppo)
    torch.manual_seed(3)
    net = ppo.DyrosActorCritic(U.IN, U.ACT, ppo.TRAIN_CFG["network"]).to(DEV)
    fu = U.FusedPpoUpdate(net, ppo.TRAIN_CFG["config"], 1024, 4, DEV)
    pol = WP.WalkPolicy.from_module(net)
    obs = torch.randn(300, U.IN, device=DEV)
    a = torch.empty(300, U.ACT, device=DEV)
    assert fu.api["play"](fu.p.data_ptr(), fu.p32f.data_ptr(), net.sigma.data_ptr(), obs.data_ptr(), None, 300, a.data_ptr(), None, None, 0,
                          stream()) == 0
    cl, _mu = pol.play(obs)
    torch.cuda.synchronize()
    assert torch.equal(a, cl)


@pytest.mark.parametrize("N", [1, 64, 65, 4096, 16384])
def test_torch_backend_agrees(N):
    pol = make(4)
    tor = make(4, backend="torch")
    g = torch.Generator().manual_seed(N + 5)
    obs, noise = (torch.randn(N, U.IN, generator=g) * 1.5).to(DEV), torch.randn(N, U.ACT, generator=g).to(DEV)
    cl, mu = pol.play(obs)
    tcl, tmu = tor.play(obs)
    within_128x(mu, tmu, truth(pol, obs, torch.float64), N)
    assert torch.equal(tcl, torch.clamp(tmu, -1.0, 1.0)) and torch.equal(cl, torch.clamp(mu, -1.0, 1.0))
    scl, smu = pol.play(obs, noise)
    assert torch.equal(smu, mu) and torch.equal(scl, torch.clamp(mu + torch.exp(pol.logstd) * noise, -1.0, 1.0))
    tscl, _ = tor.play(obs, noise)
    assert torch.equal(tscl, torch.clamp(tmu + torch.exp(tor.logstd) * noise, -1.0, 1.0))


@pytest.mark.parametrize("N", [17, 4097])
def test_play_graph_replay_is_bitwise_eager(N):
    pol = make(5)
    g = torch.Generator().manual_seed(N)
    obs, noise = (torch.randn(N, U.IN, generator=g) * 1.5).to(DEV), torch.randn(N, U.ACT, generator=g).to(DEV)
    eager = [t.clone() for t in pol.play(obs, noise)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pol.play(obs, noise)          # (the workspace exists before the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pol.play(obs, noise)
    for t in out:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, out):
        assert torch.equal(e, r)


def test_play_bad_arguments():
    pol = make(6)
    api = pol.api
    obs = torch.zeros(8, U.IN, device=DEV)
    out = torch.zeros(8, U.ACT, device=DEV)
    nz = torch.zeros(8, U.ACT, device=DEV)
    w = torch.zeros(api["play_work_floats"](8), device=DEV)
    p, pf, ls, o, c, wp, nw = pol.p.data_ptr(), pol.p32f.data_ptr(), pol.logstd.data_ptr(), obs.data_ptr(), out.data_ptr(), w.data_ptr(), w.numel()
    cases = [((p, pf, ls, o, None, 0, c, None, wp, nw), "bad argument"),
             ((None, pf, ls, o, None, 8, c, None, wp, nw), "bad argument"),
             ((p, None, ls, o, None, 8, c, None, wp, nw), "bad argument"),
             ((p, pf, ls, None, None, 8, c, None, wp, nw), "bad argument"),
             ((p, pf, ls, o, None, 8, None, None, wp, nw), "bad argument"),
             ((p, pf, None, o, nz.data_ptr(), 8, c, None, wp, nw), "bad argument"),
             ((p, pf, ls, o, None, 8, c, None, wp, nw - 1), "workspace too small"),
             ((p, pf, ls, o, None, 8, c, None, None, nw), "workspace too small")]
    for args, msg in cases:
        out.fill_(5.0)
        assert api["play"](*args, stream()) == -1, args
        assert msg in api["last_error"]().decode(), (args, api["last_error"]())
        torch.cuda.synchronize()
        assert bool((out == 5.0).all()), args          # (nothing was launched)
    with pytest.raises(ValueError):
        pol.play(torch.zeros(8, U.IN - 1, device=DEV))
    with pytest.raises(ValueError):
        pol.play(obs, torch.zeros(8, U.ACT - 1, device=DEV))
    with pytest.raises(ValueError):
        pol.play(obs.double())
