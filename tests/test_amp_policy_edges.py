"""tests/amp_policy_stages.py -- the stage-wise float64 truth of dwa_act / dwa_critic / dwa_grad and the mirror of their workspace -- held to
things independent of it, and shown to reject defects: float64 autograd and amp_policy_truth.loss_and_grad for the composed stages, the
arithmetic of csrc/dw_amp_policy.hip (and the built library, where it loads) for the byte counts, the generator's 1 % condition for every
case of tests/test_amp_policy_edges_gpu.py, and tests/amp_policy_emul.py (a float32 CPU restatement with injectable faults) for the stage
checks themselves.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

import amp_policy_emul as E
import amp_policy_stages as S
import amp_policy_truth as T
from isaacgymdyros_amd import amp_policy as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [c[:3] for c in S.CASES]
CHEAP = [c for c in CASES if c[0] <= 257] + [(4097, 511, 1)]          # the slab switch at the smallest parameter count (A = 1) of the two
_cache = {}


def case(B, D, A):
    """One generated case per shape for the whole module (read-only)."""
    if (B, D, A) not in _cache:
        _cache[(B, D, A)] = S.case(B, D, A)
    return _cache[(B, D, A)]


def prefill(c):
    g = torch.Generator().manual_seed(c["B"])
    g0 = 1e-3 * torch.randn(c["p"].numel(), generator=g)
    state0 = torch.zeros(AP.K["DWA_S_WORDS"])
    state0[:5] = torch.tensor([0.25, -0.5, 0.125, 0.75, 3.0])
    state0[AP.K["DWA_S_LR"]], state0[AP.K["DWA_S_STEP"]] = 3e-4, 7.0
    return g0, state0


@pytest.mark.parametrize("B,D,A", [(40, 1, 1), (97, 33, 12), (65, 32, 16)])
def test_composed_stages_agree_with_the_analytic_backward_and_autograd(B, D, A):
    c = case(B, D, A)
    P = [t.double().clone().requires_grad_(True) for t in c["P"]]
    xn, _ = S.norm(c["obs"], c["obs_stats"], D)
    args = (c["logstd"].double(), c["act"].double(), c["old"].double(), c["adv"].double(), c["ret"].double())
    H = S.composed_loss(xn, P, *args)
    auto = torch.autograd.grad(H["loss"], P)
    with torch.no_grad():
        loss, logs, grads, _, _ = T.loss_and_grad(xn, [t.detach() for t in P], *args)
    assert abs(float(H["loss"].detach()) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    for i in range(4):
        assert abs(float(H["sums"][0][i]) - float(logs[i])) <= 1e-12 * max(1.0, abs(float(logs[i])))
    for name, a, t in zip(S.NAMES, auto, grads):
        t = t.reshape(a.shape)
        assert float((a - t).abs().max()) <= 1e-12 * max(float(t.abs().max()), 1e-30), name
    # and torch's own statement of the loss (amp_policy.loss_terms on an nn.Module), through autograd
    net = AP.ActorCritic(D, A, [AP.HID, AP.HID], -1.6).double()
    with torch.no_grad():
        for t, src in zip(net.params_in_layout(), c["P"]):
            t.copy_(src.double())
    mu = net.mu(net.actor_mlp(xn))
    v = net.value(net.critic_mlp(xn))
    a_loss, c_loss, b_loss, _ = AP.loss_terms(args[2], net.neglogp(args[1], mu), args[3], mu, v, args[4], S.COEF[0])
    ref = torch.autograd.grad(a_loss + S.COEF[1] * c_loss + S.COEF[2] * b_loss, net.params_in_layout())
    for name, a, t in zip(S.NAMES, auto, ref):
        assert float((a - t).abs().max()) <= 1e-9 * max(float(t.abs().max()), 1e-30), name          # (e_clip: 0.2 against fp32's 0.2 moves no row here)
    # the stage-wise dmu / dv are the gradients of the loss at the heads
    assert not bool(H["near"].any())


def _source_constants():
    src = open(os.path.join(ROOT, "isaacgymdyros_amd", "csrc", "dw_amp_policy.hip")).read()
    pick = lambda pat: re.search(pat, src).group(1)          # noqa: E731
    return {"HL_extra": int(pick(r"constexpr int HL = HID \+ (\d+);")), "DL": int(pick(r"constexpr int DL = (\d+);")),
            "HEAD_BLOCKS": int(pick(r"constexpr int HEAD_BLOCKS = (\d+);")), "RW": int(pick(r"constexpr int RW = (\d+);")),
            "TK": int(pick(r"TK = (\d+),")), "src": src}


def test_layout_mirror_reproduces_the_source_and_the_library():
    k = _source_constants()
    assert (S.HL - S.HID, S.DL, S.HEAD_BLOCKS, S.RW, S.TK) == (k["HL_extra"], k["DL"], k["HEAD_BLOCKS"], k["RW"], k["TK"])
    assert "int xl_of(int D) { return (D + 1 + 3) / 4 * 4; }" in k["src"]
    assert "int slabs_of(int B) { return B <= 4096 ? 1 : (B + 4095) / 4096 > 16 ? 16 : (B + 4095) / 4096; }" in k["src"]
    assert "H.dd[(size_t)r * DL + 16] = dv;" in k["src"] and S.DV_COL == 16
    try:          # dwa_workspace_bytes is host code: the library answers without a GPU wherever it loads
        from isaacgymdyros_amd import build
        lib = ctypes.CDLL(build.build())
        lib.dwa_workspace_bytes.restype = ctypes.c_int64
        ask = lib.dwa_workspace_bytes
    except OSError:
        ask = None          # (the library does not load here: the comparison with it is left to tests/test_amp_policy_edges_gpu.py)
    for B, D, A in CASES + [(131072, 468, 12), (65537, 512, 16), (70000, 1, 1)]:
        for grad in (0, 1):
            # the arithmetic of layout(), written out once more
            r64 = lambda x: (x + 63) // 64 * 64          # noqa: E731
            end = r64(r64(r64(B * ((D + 4) // 4 * 4)) + 2 * B * 516) + 2 * B * 516)
            if grad:
                nz = 1 if B <= 4096 else min(-(-B // 4096), 16)
                end = r64(r64(r64(r64(end + 2 * B * 516) + B * 32) + 2048 * 4) + 2 * nz * 512 * 513)
            assert S.workspace_bytes(B, D, A, grad) == 4 * end, (B, D, A, grad)
            if ask is not None:
                assert ask(B, D, A, grad) == 4 * end, (B, D, A, grad)
    assert [S.slab_rows(B) for B in (1, 4096)] == [[(0, 1)], [(0, 4096)]]
    assert S.slab_rows(4097) == [(0, 2080), (2080, 4097)] and S.slab_rows(8193) == [(0, 2752), (2752, 5504), (5504, 8193)]
    assert S.heads_trips(8192) == (2048, 1) and S.heads_trips(8193) == (2048, 2) and S.heads_trips(5) == (2, 1)


@pytest.mark.parametrize("B,D,A", CASES, ids=["%d-%d-%d" % c for c in CASES])
def test_generator_moves_at_most_one_percent_of_the_rows(B, D, A):
    """S.case asserts the condition itself (float64 alone); here for every case of the GPU test, with the cover the cases are meant to have."""
    c = case(B, D, A)
    assert c["altered"] <= 0.01 * B
    xn, _ = S.norm(c["obs"], c["obs_stats"], D)
    _, h2a, _, h2c, mu, _ = T.forward(xn, [t.double() for t in c["P"]])
    H = S.heads(h2a, h2c, [t.double() for t in c["P"]], c["logstd"], c["act"], c["old"], c["adv"], c["ret"])
    assert not bool(H["near"].any())
    if B >= 63:
        r = H["ratio"]
        assert bool((r < S.LO32).any()) and bool((r > S.HI32).any()) and (A == 1 or bool((mu > 1.0).any()) and bool((mu < -1.0).any()))
        tie = torch.arange(B) % 4 == 1
        assert float((r[tie] - 1.0).abs().max()) < 1e-5 and float(H["margin"].max()) < 5e-3


def _run(c, fault=None):
    g0, state0 = prefill(c)
    Wa, out = E.act(c, fault)
    Wg, g, state = E.grad(c, g0, state0, fault=fault)
    return Wa, out, Wg, g, g0, state, state0


@pytest.mark.parametrize("B,D,A", CHEAP, ids=["%d-%d-%d" % c for c in CHEAP])
def test_unfaulted_emulation_passes_every_stage_check(B, D, A):
    c = case(B, D, A)
    Wa, out, Wg, g, g0, state, state0 = _run(c)
    nb = [S.workspace_bytes(B, D, A, k) for k in (0, 1)]
    wo = S.check_act(c, Wa, out, nb[0])
    wg = S.check_grad(c, Wg, Wa, g, g0, state, state0, nb[1], nb[0])
    Wc, val = E.critic(c)
    wc = S.check_critic(c, Wc, val, nb[0])
    assert float(state[AP.K["DWA_S_UPDATES"]]) == 4.0
    assert {"xn", "h1", "h2", "mu", "action", "neglogp", "value"} <= set(wo) and {"xn", "h1", "h2", "value"} <= set(wc)
    assert {"xn", "h1", "h2", "dmu", "dv", "logs", "dz2", "g_heads", "g_layer2", "dz1", "slab1", "g_layer1"} <= set(wg)
    print(wo.line()), print(wc.line()), print(wg.line())


# fault -> the smallest case of the list at which it is reachable
REACH = {"slab_last_row": (1, 1, 1), "tile_last_row": (1, 1, 1), "bias_column": (1, 1, 1), "g_assign": (1, 1, 1), "critic_mask": (1, 1, 1),
         "dv_column": (1, 1, 1), "k_tail": (1, 1, 1), "heads_second_trip": (8193, 468, 12)}


# fault -> the check that has to reject it (a stage's name in Worst.note's message, or check_layout's for a word that kept or lost its NaN)
REJECTED_BY = {"slab_last_row": "g_", "tile_last_row": "'h1'", "bias_column": "g_", "g_assign": "g_", "critic_mask": "'dz2'", "dv_column": "dd:",
               "k_tail": "'h1'", "heads_second_trip": "dd:"}


def _rejects(c, fault):
    Wa, out, Wg, g, g0, state, state0 = _run(c, fault)
    with pytest.raises(AssertionError) as e:
        S.check_act(c, Wa, out)
        S.check_grad(c, Wg, Wa, g, g0, state, state0)
    assert REJECTED_BY[fault] in str(e.value), (fault, str(e.value))


@pytest.mark.parametrize("fault", E.FAULTS)
def test_every_injected_fault_is_rejected(fault):
    assert set(REACH) == set(E.FAULTS) == set(REJECTED_BY)
    _rejects(case(*REACH[fault]), fault)


@pytest.mark.parametrize("fault,shape", [("slab_last_row", (4097, 511, 1)), ("tile_last_row", (17, 33, 1)), ("bias_column", (257, 512, 16)),
                                         ("k_tail", (17, 33, 1)), ("dv_column", (63, 31, 12)), ("critic_mask", (65, 32, 16)),
                                         ("slab_last_row", (129, 128, 12))])
def test_faults_are_rejected_at_the_edges_they_belong_to(fault, shape):
    """The same defects where the kernel would meet them: one row of 4097 (the second slab's last), the one-row second tile, the fifth column
    tile's single column, the one-word second k slice."""
    _rejects(case(*shape), fault)


def test_a_fault_that_a_case_cannot_reach_leaves_it_passing():
    """dv_column at A = 16 writes column 16 all the same; k_tail at D = 32 has no partial slice: the emulation and the checks agree on that."""
    c = case(65, 32, 16)
    for fault in ("dv_column", "k_tail"):
        Wa, out, Wg, g, g0, state, state0 = _run(c, fault)
        S.check_grad(c, Wg, Wa, g, g0, state, state0)
