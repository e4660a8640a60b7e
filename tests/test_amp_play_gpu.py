"""dwa_play (include/dyros_amp_policy.h) on the GPU: against float64 truth at every row-count edge of its two forms, the clamp and the noise
bit for bit, against dwa_act's mu, under graph replay, and its argument errors."""
import pytest
import torch

from isaacgymdyros_amd import amp_policy as AP

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NS = [1, 2, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 16384]


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def make(D, A, seed=0):
    pol = AP.AmpActorCritic(D, A, DEV, backend="hip", seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        pol.obs_stats[:D] = (torch.randn(D, generator=g, dtype=torch.float64) * 0.5).to(DEV)
        pol.obs_stats[D:2 * D] = (torch.rand(D, generator=g, dtype=torch.float64) * 2 + 0.2).to(DEV)
        pol.obs_stats[2 * D] = 1000.0
        pol.net.mu.bias[:] = (torch.randn(A, generator=g) * 0.8).to(DEV)          # (mu beyond +-1 in some rows: the clamp acts)
    return pol


def call(pol, obs, noise=None, with_mu=True):
    """dwa_play with NaN-filled outputs (and workspace): (rc, clamped, mu)."""
    api, N = AP._api(), obs.shape[0]
    cl = torch.full((N, pol.A), float("nan"), device=DEV)
    mu = torch.full((N, pol.A), float("nan"), device=DEV)
    nb = api["play_workspace_bytes"](N, pol.D, pol.A)
    w = torch.full((max(nb, 4) // 4,), float("nan"), device=DEV)
    rc = api["play"](pol.p.data_ptr(), pol.obs_stats.data_ptr(), pol.net.sigma.data_ptr(), obs.data_ptr(),
                     None if noise is None else noise.data_ptr(), N, pol.D, pol.A, cl.data_ptr(), mu.data_ptr() if with_mu else None,
                     w.data_ptr(), w.numel() * 4, stream())
    return rc, cl, mu


def truth(pol, obs, dtype):
    net = AP.ActorCritic(pol.D, pol.A, [AP.HID, AP.HID], -1.6).to(DEV)
    net.load_state_dict(pol.state_dict())
    net = net.to(dtype).eval()
    with torch.no_grad():
        return net(obs.to(dtype))[0]


def within_128x(hip, f32, f64, what):
    e_hip = (hip.double() - f64).abs().max().item()
    e_32 = (f32.double() - f64).abs().max().item()
    assert e_hip <= 128 * e_32 + 1e-6 * max(f64.abs().max().item(), 1e-3), (what, e_hip, e_32)


@pytest.mark.parametrize("A", [1, 12, 16])
@pytest.mark.parametrize("D", [1, 468, 512])
def test_play_against_float64(D, A):
    pol = make(D, A, seed=D + A)
    for N in NS:
        g = torch.Generator().manual_seed(N)
        obs = (torch.randn(N, D, generator=g) * 1.5).to(DEV)
        noise = torch.randn(N, A, generator=g).to(DEV)
        rc, cl, mu = call(pol, obs)
        assert rc == 0, AP._api()["last_error"]()
        torch.cuda.synchronize()
        assert torch.isfinite(mu).all() and torch.isfinite(cl).all(), (N, D, A)
        within_128x(mu, truth(pol, obs, torch.float32), truth(pol, obs, torch.float64), (N, D, A))
        assert torch.equal(cl, torch.clamp(mu, -1.0, 1.0)), (N, D, A)
        rc, cl2, mu2 = call(pol, obs, noise)
        assert rc == 0
        assert torch.equal(mu2, mu), (N, D, A)
        assert torch.equal(cl2, torch.clamp(mu2 + torch.exp(pol.net.sigma) * noise, -1.0, 1.0)), (N, D, A)
        rc, cl3, _ = call(pol, obs, with_mu=False)
        assert rc == 0 and torch.equal(cl3, cl), (N, D, A)


@pytest.mark.parametrize("N", [1, 64, 65, 4096, 16384])
def test_play_against_act_and_torch_backend(N):
    pol = make(468, 12)
    tor = AP.AmpActorCritic(468, 12, DEV, backend="torch")
    tor.load_state_dict(pol.state_dict())
    g = torch.Generator().manual_seed(N + 5)
    obs, noise = (torch.randn(N, 468, generator=g) * 1.5).to(DEV), torch.randn(N, 12, generator=g).to(DEV)
    cl, mu = pol.play(obs)
    _a, _ac, mu_act, _nlp, _v = pol.act(obs, noise)
    tcl, tmu = tor.play(obs)
    f64 = truth(pol, obs, torch.float64)
    within_128x(mu, mu_act, f64, "play vs act")
    within_128x(mu, tmu, f64, "play vs torch")
    assert torch.equal(tcl, torch.clamp(tmu, -1.0, 1.0))
    scl, smu = pol.play(obs, noise)
    assert torch.equal(smu, mu) and torch.equal(scl, torch.clamp(mu + torch.exp(pol.net.sigma) * noise, -1.0, 1.0))


@pytest.mark.parametrize("N", [17, 4097])
def test_play_graph_replay_is_bitwise_eager(N):
    pol = make(468, 12)
    g = torch.Generator().manual_seed(N)
    obs, noise = (torch.randn(N, 468, generator=g) * 1.5).to(DEV), torch.randn(N, 12, generator=g).to(DEV)
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
    pol = make(468, 12)
    api = AP._api()
    obs = torch.zeros(8, 468, device=DEV)
    out = torch.zeros(8, 12, device=DEV)
    w = torch.zeros(api["play_workspace_bytes"](8, 468, 12) // 4, device=DEV)
    p, st, ls = pol.p.data_ptr(), pol.obs_stats.data_ptr(), pol.net.sigma.data_ptr()
    cases = [(None, st, ls, obs.data_ptr(), None, 8, 468, 12, out.data_ptr(), None, w.data_ptr(), w.numel() * 4, "bad argument"),
             (p, st, ls, obs.data_ptr(), None, 0, 468, 12, out.data_ptr(), None, w.data_ptr(), w.numel() * 4, "bad argument"),
             (p, st, None, obs.data_ptr(), out.data_ptr(), 8, 468, 12, out.data_ptr(), None, w.data_ptr(), w.numel() * 4, "bad argument"),
             (p, st, ls, obs.data_ptr(), None, 8, 468, 17, out.data_ptr(), None, w.data_ptr(), w.numel() * 4, "A in [1, 16]"),
             (p, st, ls, obs.data_ptr(), None, 8, 468, 12, out.data_ptr(), None, w.data_ptr(), 16, "workspace too small"),
             (p, st, ls, obs.data_ptr(), None, 8, 468, 12, out.data_ptr(), None, None, w.numel() * 4, "workspace too small")]
    for c in cases:
        assert api["play"](*c[:-1], stream()) == -1, c
        assert c[-1] in api["last_error"]().decode()
    with pytest.raises(ValueError):
        pol.play(torch.zeros(8, 467, device=DEV))
    with pytest.raises(ValueError):
        pol.play(obs, torch.zeros(8, 11, device=DEV))
