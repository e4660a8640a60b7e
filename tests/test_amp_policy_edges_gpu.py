"""dwa_act, dwa_critic and dwa_grad (csrc/dw_amp_policy.hip) through the C ABI at the smallest shapes that reach each edge of dwa_mm's 128 x 128
tile, its four 64 x 64 waves, the 16-row MFMA tiles its `live` count gates, the 32-deep k slices, the split of K = B into slabs and
dwa_heads_bwd's grid-stride loop -- stage by stage against the float64 truth of tests/amp_policy_stages.py, computed on the GPU from the
operands the kernels had, with the bounds derived there.  The workspace is NaN before every call and g / state hold nonzero values, so a word
the kernels should not write, a ones column they should, and `=` in place of `+=` all show.  tests/test_amp_policy_edges.py shows on the CPU
that these checks reject a dropped slab row, tile row, bias column or k tail, a wrong mask, a misplaced dv and a skipped grid-stride trip.

A line `amp-edges ...` per call reports each stage's worst error as a fraction of its bound (pytest -s shows them); DESIGN.md section 13
has the table."""
import pytest
import torch

import amp_policy_stages as S
from isaacgymdyros_amd import amp_policy as AP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [c[:3] for c in S.CASES]
IDS = ["%d-%d-%d" % c for c in CASES]
NAN = float("nan")
_cases, _acts = {}, {}


def api():
    return AP._api()


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def case(B, D, A, seed=None):
    key = (B, D, A, seed)
    if key not in _cases:
        _cases[key] = S.case(B, D, A, seed=seed, device=DEV)
    return _cases[key]


def workspace(c, grad, rows=None):
    nb = api()["workspace_bytes"](rows or c["B"], c["D"], c["A"], grad)
    assert nb > 0 and nb % 4 == 0
    return torch.full((nb // 4,), NAN, device=DEV), nb


def prefill(c, updates=3.0):
    g = torch.Generator().manual_seed(c["B"])
    g0 = (1e-3 * torch.randn(c["p"].numel(), generator=g)).to(DEV)
    state0 = torch.zeros(AP.K["DWA_S_WORDS"])
    state0[:5] = torch.tensor([0.25, -0.5, 0.125, 0.75, updates])
    state0[AP.K["DWA_S_LR"]], state0[AP.K["DWA_S_STEP"]] = 3e-4, 7.0
    return g0, state0.to(DEV)


def run_act(c):
    """dwa_act on the case's rows, once per case for the whole module: (workspace, its byte count, the five outputs)."""
    key = (c["B"], c["D"], c["A"], c["p"].data_ptr())
    if key not in _acts:
        N, D, A = c["B"], c["D"], c["A"]
        W, nb = workspace(c, 0)
        a, ac, mu = (torch.full((N, A), NAN, device=DEV) for _ in range(3))
        nlp, val = torch.full((N,), NAN, device=DEV), torch.full((N, 1), NAN, device=DEV)
        rc = api()["act"](c["p"].data_ptr(), c["obs_stats"].data_ptr(), c["val_stats"].data_ptr(), c["logstd"].data_ptr(), c["obs"].data_ptr(),
                          c["noise"].data_ptr(), N, D, A, a.data_ptr(), ac.data_ptr(), mu.data_ptr(), nlp.data_ptr(), val.data_ptr(), W.data_ptr(),
                          nb, stream())
        assert rc == 0, api()["last_error"]()
        torch.cuda.synchronize()
        _acts[key] = (W, nb, (a, ac, mu, nlp, val))
    return _acts[key]


def run_critic(c):
    N, D, A = c["B"], c["D"], c["A"]
    W, nb = workspace(c, 0)
    val = torch.full((N, 1), NAN, device=DEV)
    rc = api()["critic"](c["p"].data_ptr(), c["obs_stats"].data_ptr(), c["val_stats"].data_ptr(), c["obs"].data_ptr(), c["term"].data_ptr(), N, D, A,
                         val.data_ptr(), W.data_ptr(), nb, stream())
    assert rc == 0, api()["last_error"]()
    torch.cuda.synchronize()
    return W, nb, val


def run_grad(c, g, state, W, nbytes):
    """dwa_grad into g and state as they are (in place)."""
    rc = api()["grad"](c["p"].data_ptr(), c["obs_stats"].data_ptr(), c["logstd"].data_ptr(), c["obs"].data_ptr(), c["act"].data_ptr(),
                       c["old"].data_ptr(), c["adv"].data_ptr(), c["ret"].data_ptr(), c["B"], c["D"], c["A"], AP.DwaLoss(*S.COEF), g.data_ptr(),
                       state.data_ptr(), W.data_ptr(), nbytes, stream())
    assert rc == 0, api()["last_error"]()
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,D,A", CASES, ids=IDS)
def test_grad_stage_by_stage_at_tile_and_slab_edges(B, D, A):
    """S1 .. S7 of tests/amp_policy_stages.py, the layer-1 slabs one by one where there are several, the layout's self-checks, the logged sums
    and the update count; h1 from dwa_act on the same rows after its h2 proved bit-identical to dwa_grad's."""
    c = case(B, D, A)
    assert c["altered"] <= 0.01 * B
    Wa, nba, _ = run_act(c)
    Wg, nbg = workspace(c, 1)
    g0, state0 = prefill(c)
    g, state = g0.clone(), state0.clone()
    run_grad(c, g, state, Wg, nbg)
    wo = S.check_grad(c, Wg, Wa, g, g0, state, state0, nbg, nba)
    assert float(state[AP.K["DWA_S_UPDATES"]]) == 4.0
    assert {"xn", "h1", "h2", "dmu", "dv", "logs", "dz2", "g_heads", "g_layer2", "dz1", "slab1", "g_layer1"} <= set(wo)
    print(wo.line())


SMALL = [c for c in CASES if c[0] <= 4097]


@pytest.mark.parametrize("B,D,A", SMALL, ids=["%d-%d-%d" % c for c in SMALL])
def test_act_and_critic_stage_by_stage(B, D, A):
    """S1 .. S3 of dwa_act and dwa_critic; dwa_critic's h2 at the critic's offset, the actor's half of its workspace still NaN."""
    c = case(B, D, A)
    Wa, nba, out = run_act(c)
    wa = S.check_act(c, Wa, out, nba)
    Wc, nbc, val = run_critic(c)
    wc = S.check_critic(c, Wc, val, nbc)
    assert nba == nbc
    v = S.views(Wc, B, D, 0)
    assert torch.equal(v["h2"][1][:, :S.HID], S.views(Wa, B, D, 0)["h2"][1][:, :S.HID])          # (the same forward() for the critic alone)
    live = c["term"] == 0
    assert torch.equal(val.reshape(-1)[live], out[4].reshape(-1)[live])
    print(wa.line()), print(wc.line())


def test_two_calls_accumulate_into_one_g_and_reuse_one_workspace():
    """dwa_grad with B = 65, then B = 129, into the same g and state through one workspace sized for the larger (so the second call finds the
    first one's words, not NaN).  Sums are in slab order and `+=` is one fp32 addition, so g must be bit for bit fl(g after the first + the
    second's gradient alone), the first call's g that of a run with a fresh workspace, and the logged sums likewise; the update count is 2.
    The second call also passes every stage check from the g and state it found."""
    D, A, seed = 32, 16, 4242
    c1, c2 = case(65, D, A, seed), case(129, D, A, seed)
    assert torch.equal(c1["p"], c2["p"]) and torch.equal(c1["obs_stats"], c2["obs_stats"])
    W, nb = workspace(c2, 1)
    assert api()["workspace_bytes"](65, D, A, 1) < nb
    g0, state0 = prefill(c1, updates=0.0)
    g, state = g0.clone(), state0.clone()
    run_grad(c1, g, state, W, nb)
    g1, state1 = g.clone(), state.clone()
    run_grad(c2, g, state, W, nb)
    assert float(state[AP.K["DWA_S_UPDATES"]]) == 2.0
    # each call alone, with a workspace of its own
    ga, sa = g0.clone(), state0.clone()
    run_grad(c1, ga, sa, *workspace(c1, 1))
    gb, sb = torch.zeros_like(g0), torch.zeros_like(state0)
    run_grad(c2, gb, sb, *workspace(c2, 1))
    assert torch.equal(g1, ga) and torch.equal(state1, sa)
    assert torch.equal(g, g1 + gb) and torch.equal(state[:4], state1[:4] + sb[:4])
    assert bool((gb != 0).any()) and bool((g1 != g0).any())
    Wa, nba, _ = run_act(c2)
    wo = S.check_grad(c2, W, Wa, g, g1, state, state1, None, nba, layout_checks=False)
    print(wo.line())
