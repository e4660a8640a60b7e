"""tests/ppo_rollout_truth.py -- the float64 restatement of the walk learner's rollout kernels with its derived bounds, and the fp32 restatement as
launched -- held to something independent of it: examples/ppo_consumer.py's neglogp and discount_values and the torch module's forward in
float64; then the checks themselves: the clean restatement passes every one, and every injected fault is rejected by at least one.  No GPU."""
import numpy as np
import pytest
import torch

import ppo_rollout_truth as T

PPO = T.consumer()
REL = 1e-12


def _run_pre(N, H, nobs, n, layout, fault=None, seed=0):
    rng = np.random.default_rng(seed)
    inp = T.pre_inputs(rng, N, H, nobs, n, layout)
    before = T.alloc_pre(N, H, nobs, layout)
    return T.check_pre(inp, before, T.launched_pre(inp, before, fault))


def _run_post(N, H, nobs, n, fault=None, seed=0, **kw):
    rng = np.random.default_rng(seed)
    inp = T.post_inputs(rng, N, H, nobs, n, **kw)
    before = T.alloc_post(inp, rng)
    return T.check_post(inp, before, T.launched_post(inp, before, fault))


def _run_gae(N, H, pattern, fault=None, seed=0, p=0.05):
    inp = T.gae_inputs(np.random.default_rng(seed), N, H, pattern, p)
    before = T.alloc_gae(N, H)
    return T.check_gae(inp, before, T.launched_gae(inp, before, fault))


@pytest.fixture(scope="module")
def policy_case():
    net = T.policy_net(1)
    W, obs = T.weights_of(net), T.policy_obs(70, 1)
    return net, W, obs, T.policy_truth(W, obs)


def _run_policy(case, N, fault=None):
    _net, W, obs, truth = case
    before = T.alloc_policy(N)
    return T.check_policy(N, before, T.launched_policy(W, obs[:N], before, fault), truth)


# ------------------------------------------------------------------------------------------------ the truth against the consumer's own functions
def test_nlp_truth_is_the_consumers_neglogp():
    rng = np.random.default_rng(3)
    inp = T.pre_inputs(rng, 37, 1, 16, 0, "step")
    a = (inp["mu"] + np.exp(inp["logstd"]) * inp["noise"]).astype(np.float32)
    t, b = T.nlp_truth(a, inp["mu"], inp["noise"], inp["logstd"])
    d = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))          # noqa: E731
    ls = d(inp["logstd"])
    ref = PPO.neglogp(d(a), d(inp["mu"]), torch.exp(ls), ls.expand(37, T.ACT)).numpy()
    assert np.abs(t - ref).max() <= REL * np.abs(ref).max()
    ta, ba = T.act_truth(inp["mu"], inp["noise"], inp["logstd"])
    assert np.abs(ta - (d(inp["mu"]) + torch.exp(ls) * d(inp["noise"])).numpy()).max() <= REL * np.abs(ta).max()
    # the bounds are of the size the derivation says: a few u of the action, and of 2 b / sigma -- not of the result -- in neglogp
    assert (ba <= 8 * T.U * (np.abs(ta) + 1.0)).all() and (ba >= T.U * np.abs(ta)).all()
    assert (b <= 1e-3).all() and (b >= T.U * np.abs(t)).all()


@pytest.mark.parametrize("pattern", T.DONE_PATTERNS)
def test_gae_truth_is_discount_values_in_float64(pattern):
    """gamma = 63/64 and tau = 15/16: their product is an fp32 number, so the launcher's rounded gamma * tau is the reference's Python product."""
    inp = T.gae_inputs(np.random.default_rng(5), 19, 7, pattern, p=0.3)
    g, tau = 63.0 / 64.0, 15.0 / 16.0
    assert T.gae_scalars(g, tau) == (g, g * tau)
    t, e = T.gae_truth(inp["fdones"], inp["last_values"], inp["mb_fdones"], inp["mb_values"], inp["mb_rewards"], g, tau)
    d = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))          # noqa: E731
    ref = PPO.discount_values(d(inp["fdones"]), d(inp["last_values"]).unsqueeze(1), d(inp["mb_fdones"]), d(inp["mb_values"]).unsqueeze(2),
                              d(inp["mb_rewards"]).unsqueeze(2), g, tau).squeeze(2).numpy()
    assert np.abs(t - ref).max() <= REL * np.abs(ref).max()
    assert (e >= 6 * T.U * np.abs(t)).all() and (e <= 6 * T.U * 8 * (1.0 + np.abs(inp["mb_rewards"]).max() + 2 * np.abs(inp["mb_values"]).max()) / (1 - g * tau)).all()


def test_gae_scalars_are_the_launchers():
    g, gt = T.gae_scalars(0.99, 0.95)
    assert g == float(np.float32(0.99)) and gt == float(np.float32(np.float64(np.float32(0.99)) * np.float64(np.float32(0.95))))


def test_policy_truth_is_the_modules_float64_forward(policy_case):
    net, W, obs, (mu, v, bmu, bv) = policy_case
    net64 = T.policy_net(1).double()
    with torch.no_grad():
        mu_t, _, v_t = net64(torch.from_numpy(obs).double())
    assert np.abs(mu - mu_t.numpy()).max() <= REL * np.abs(mu).max() and np.abs(v - v_t.numpy()[:, 0]).max() <= REL * np.abs(v).max()
    with torch.no_grad():          # (the dead units are dead, the rest is lively)
        h1 = net64.actor_mlp[:2](torch.from_numpy(obs).double())
    assert float(h1[:, list(T.DEAD_UNITS)].abs().max()) == 0.0 and float((h1 > 0).double().mean()) > 0.3
    assert np.abs(obs[2]).max() == 0.0 and np.abs(obs[0]).max() > 1e3
    assert (bmu > 0).all() and (bv > 0).all() and (bmu >= 2 * (T.IN + 2 * T.HID + 8) * T.U * np.abs(mu)).all()


def test_terms_and_reward_truth_are_the_plain_formulas():
    rng = np.random.default_rng(7)
    inp = T.post_inputs(rng, 300, 2, 16, 1, nterms=15)
    t, b = T.rew_truth(inp["rew"], inp["value"], inp["time_outs"], 0.5, 0.99)
    assert np.array_equal(t, inp["rew"].astype(np.float64) * 0.5 + float(np.float32(0.99)) * inp["value"].astype(np.float64) * inp["time_outs"])
    assert (b <= 4 * T.U * (np.abs(t) + np.abs(inp["rew"]) + np.abs(inp["value"])) + 1e-37).all()
    t0 = rng.standard_normal(15).astype(np.float32)
    t, b = T.terms_truth(t0, inp["stacked"], 15, 300)
    assert np.abs(t - (t0 + inp["stacked"][:, :15].astype(np.float64).mean(0))).max() <= REL
    assert (b <= (11 + 2 * 2) * T.U * 1.01 * (np.abs(t0) + np.abs(inp["stacked"]).astype(np.float64).mean(0)[:15]) + 1e-37).all()


# ------------------------------------------------------------------------------------------------ the launchers' grids
def test_the_grid_covers_every_item_and_the_copy_alone_does_not():
    assert 256 * T.pre_blocks(1024, 16, largest=False) == 4096 < 1024 * T.ACT <= 256 * T.pre_blocks(1024, 16)
    for nobs in (13, 16, 48, 51, 52, 487, 488, 512):
        for N in (4, 252, 255, 256, 257, 260, 1024, 1028):
            if (N * nobs) % 4:
                continue
            need = max(N * nobs // 4, N * T.ACT, N * ((nobs + 7) // 8))
            assert 256 * T.pre_blocks(N, nobs) >= need
            short = 256 * T.pre_blocks(N, nobs, largest=False) < need
            # (the copy's count rounds up to whole workgroups: it is short exactly where those hold fewer threads than N * ACT action words --
            #  never from 52 words per row on, and below that for all but a handful of envs)
            assert short == (256 * ((N * nobs // 4 + 255) // 256) < N * T.ACT), (N, nobs)
            assert not (short and nobs >= 52), (N, nobs)
            for same in (False, True):
                assert 256 * T.post_blocks(N, nobs, same) >= (N if same else max(N, N * nobs // 4))
    assert 256 * T.post_blocks(1024, 2, False, largest=False) < 1024


# ------------------------------------------------------------------------------------------------ the clean restatement passes
@pytest.mark.parametrize("layout", ["step", "env", "half"])
@pytest.mark.parametrize("nobs", [13, 16, 48, 52, 487, 488, 512])
def test_clean_rollout_pre_passes(layout, nobs):
    for N, H, n in ((4, 1, 0), (260, 3, 1), (1028, 3, 2), (256, 1, 0), (260, 3, -1), (260, 3, 3)):
        res = _run_pre(N, H, nobs, n, layout, seed=N + nobs)
        assert T.failures(res) == [], (N, H, n, res)


@pytest.mark.parametrize("nobs", [13, 16, 487, 512])
def test_clean_rollout_post_passes(nobs):
    for N in (4, 256, 260, 1028):
        for kw in (dict(), dict(time_outs=False), dict(same=True), dict(nterms=1), dict(nterms=64, ncols=70), dict(nterms=0), dict(same=True, nterms=0, time_outs=False)):
            for H, n in ((1, 0), (3, 1), (3, 3), (3, -1)):
                res = _run_post(N, H, nobs, n, seed=N + nobs, **kw)
                assert T.failures(res) == [], (N, H, n, kw, res)


@pytest.mark.parametrize("pattern", T.DONE_PATTERNS)
def test_clean_gae_passes(pattern):
    for N in (1, 255, 256, 257, 513):
        for H in (1, 2, 128):
            res = _run_gae(N, H, pattern, seed=N + H)
            assert T.failures(res) == [], (N, H, res)


def test_clean_policy_passes(policy_case):
    for N in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 70):
        res = _run_policy(policy_case, N)
        assert T.failures(res) == [], (N, res)


# ------------------------------------------------------------------------------------------------ every fault is rejected
def test_short_grid_is_rejected():
    for nobs in (13, 16, 48):
        for N in (256, 260, 1024, 1028):
            for layout in ("step", "env", "half"):
                bad = T.failures(_run_pre(N, 3, nobs, 1, layout, fault="short_grid"))
                assert {"mb_act", "mb_mu"} <= set(bad), (N, nobs, layout, bad)          # (act is the clamp of what was stored: NaN for NaN)
                assert T.failures(_run_pre(N, 3, nobs, 3, layout, fault="short_grid")) == ["act"]          # (past the rows: the env's action alone)
    for N, nobs in ((16, 16), (4, 13), (1028, 52), (1028, 487)):          # (where the copy's count covers the rest, the old grid was enough)
        assert T.failures(_run_pre(N, 3, nobs, 1, "half", fault="short_grid")) == []
    bad = T.failures(_run_post(1024, 3, 2, 1, fault="short_grid"))
    assert {"mb_rew", "g_dones", "terms"} <= set(bad), bad
    assert T.failures(_run_post(1024, 3, 2, 1)) == []


@pytest.mark.parametrize("layout", ["env", "half"])
def test_swapped_env_major_index_is_rejected(layout):
    for N, nobs in ((4, 13), (260, 487), (260, 16)):
        assert T.failures(_run_pre(N, 3, nobs, 1, layout, fault="swap_env_major")) == ["mb_obs"]


def test_unzeroed_fp16_tail_is_rejected():
    for nobs in (13, 52, 487):
        assert T.failures(_run_pre(260, 3, nobs, 1, "half", fault="half_tail")) == ["mb_obs"]
    for nobs in (16, 48, 488, 512):          # (a full last piece has no tail)
        assert T.failures(_run_pre(260, 3, nobs, 1, "half", fault="half_tail")) == []


def test_dropped_bootstrap_is_rejected():
    assert T.failures(_run_post(260, 3, 16, 1, fault="no_bootstrap")) == ["mb_rew"]
    assert T.failures(_run_post(260, 3, 16, 1, fault="no_bootstrap", time_outs=False)) == []


def test_gae_wrong_step_is_rejected():
    assert T.failures(_run_gae(257, 3, "random", fault="gae_wrong_step", p=0.3)) == ["advs"]
    assert T.failures(_run_gae(257, 3, "last_step", fault="gae_wrong_step")) == ["advs"]


def test_terms_divided_by_256_is_rejected():
    for N in (4, 252, 260, 1028):
        assert T.failures(_run_post(N, 3, 16, 1, fault="terms_div_256")) == ["terms"]


def test_a_stored_row_past_n_is_rejected(policy_case):
    for N in (1, 15, 33, 65):
        assert T.failures(_run_policy(policy_case, N, fault="row_past_n")) == ["mu_guards", "value_guards"]
    assert T.failures(_run_policy(policy_case, 64, fault="row_past_n")) == []          # (a full tile has no row past the end)
    assert "advs_guards" in T.failures(_run_gae(255, 2, "random", fault="row_past_n"))


def test_swapped_policy_rows_are_rejected(policy_case):
    for N in (2, 17, 65):
        assert T.failures(_run_policy(policy_case, N, fault="policy_rows_swapped")) == ["mu", "value"]

