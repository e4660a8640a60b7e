"""tests/ppo_update_truth.py -- the float64 restatement of the fused PPO update, with derived error bounds -- held to something
independent of it: float64 autograd through examples/ppo_consumer.py's own loss functions, torch.nn.utils.clip_grad_norm_ and two
torch.optim.Adam instances, and for dwp_wgrad's slabs the plain statement that they tile the k-blocks.  No GPU."""
import math

import pytest
import torch

import ppo_update_truth as T

PPO = T.consumer()
C = dict(PPO.TRAIN_CFG["config"])
REL = 1e-12


def _same(a, b, rel=REL):
    a, b = T.f64(a), T.f64(b)
    return bool(((a - b).abs() <= rel * b.abs()).all())


def _same_sums(a, b, rel=REL):
    """Gradients that are sums of signed terms, taken in another order: to `rel` of the largest entry of their tensor."""
    o = 0
    for n in (T.NW1, T.NW2, T.NW3, T.NB1, T.NB2, T.NB3):
        for half in (slice(o, o + n // 2), slice(o + n // 2, o + n)):
            x, y = T.f64(a)[half], T.f64(b)[half]
            if not bool(torch.isfinite(y).all()):
                continue
            if float((x - y).abs().max()) > rel * float(y.abs().max()):
                return False
        o += n
    return True


def _loss_rows(n=96, seed=0):
    """Rows with the ratio on both sides of and inside the clip range under both signs of the advantage, advantages of exactly zero (both
    signs of zero) and action means beyond the bound loss's 1.1."""
    g = torch.Generator().manual_seed(seed)
    mu = 0.9 * torch.randn(n, T.ACT, generator=g, dtype=torch.float64)
    value = torch.randn(n, dtype=torch.float64, generator=g)
    logstd = torch.full((T.ACT,), -2.302585, dtype=torch.float64) + 0.05 * torch.randn(T.ACT, generator=g, dtype=torch.float64)
    sigma = torch.exp(logstd)
    act = mu + sigma * torch.randn(n, T.ACT, generator=g, dtype=torch.float64)
    old_mu = mu + 0.1 * sigma * torch.randn(n, T.ACT, generator=g, dtype=torch.float64)
    nlp = PPO.neglogp(act, mu, sigma, logstd.expand_as(mu))
    targets = torch.tensor([0.5, 0.7, 0.79, 0.81, 0.9, 1.0, 1.1, 1.19, 1.21, 1.3, 2.0, 5.0], dtype=torch.float64)
    old_nlp = nlp + torch.log(targets[torch.arange(n) % len(targets)])
    adv = torch.randn(n, generator=g, dtype=torch.float64)
    adv[:48] = adv[:48].abs() * torch.where(torch.arange(48) % 24 < 12, 1.0, -1.0).double()          # every target under both signs, twice
    adv[48:60] = 0.0          # ... and under an advantage of zero
    adv[60:72] = -0.0
    ret = torch.randn(n, generator=g, dtype=torch.float64)
    return mu, value, logstd, act, old_mu, old_nlp, adv, ret


def _out_of(mu, value):
    out = torch.zeros(2, mu.shape[0], T.OUTP, dtype=mu.dtype)
    out[0, :, :T.ACT], out[1, :, 0] = mu, value
    return out


def test_loss_and_output_gradients_equal_float64_autograd_on_the_consumers_functions():
    mu, value, logstd, act, old_mu, old_nlp, adv, ret = _loss_rows()
    e, coef, scale = C["e_clip"], C["critic_coef"], 1536.0
    L = T.loss(_out_of(mu, value), act, old_nlp, old_mu, adv, ret, logstd, scale, e, coef)
    # the data is what the docstring says
    r = L["ratio"]
    for sign in (1.0, -1.0):
        s = adv * sign > 0
        assert bool((s & (r < 1 - e)).any()) and bool((s & (r > 1 + e)).any()) and bool((s & (r > 1 - e) & (r < 1 + e)).any())
    assert int((adv == 0).sum()) == 24 and bool((mu.abs() > 1.1).any())
    mu_g, v_g = mu.clone().requires_grad_(), value.clone().requires_grad_()
    sigma = torch.exp(logstd)
    nlp = PPO.neglogp(act, mu_g, sigma, logstd.expand_as(mu_g))
    a_rows, cf = PPO.actor_loss(old_nlp, nlp, adv, e)
    c_rows = PPO.critic_loss(None, v_g.unsqueeze(1), e, ret.unsqueeze(1), False)
    al, cl = a_rows.mean(), c_rows.mean()
    (scale * (al + 0.5 * cl * coef)).backward()
    assert _same(L["nlp"], nlp) and _same(L["a_rows"], a_rows) and _same(L["a_loss"], al) and _same(L["c_loss"], cl)
    assert _same(L["b_loss"], PPO.bound_loss(mu).mean()) and float(L["b_loss"]) > 0.0
    assert round(float(L["clip_frac"]) * len(adv)) == round(float(cf) * len(adv)) == 56          # (the consumer's is an fp32 mean of a count)
    assert _same(L["kl"], PPO.policy_kl(mu, sigma.expand_as(mu), old_mu, sigma.expand_as(mu)))
    assert _same(L["dmu"], mu_g.grad) and _same(L["dvalue"], v_g.grad)
    assert float(L["dmu"][adv == 0].abs().max()) == 0.0 and float(L["dmu"].abs().max()) > 0.0
    assert bool((L["dmu_bound"] >= T.SUB16).all()) and bool((L["dmu_bound"] <= 1e-3 * L["dmu"].abs() + T.SUB16).all())


def test_a_ratio_that_overflows_fp32_poisons_the_actor_only():
    """old_nlp - nlp beyond log(FLT_MAX): the ratio is inf in fp32, autograd's mu gradient of that row is not finite (0 * inf through exp's
    backward), and the helper says the same: found_inf for the actor, not for the critic."""
    n = 96
    mu, value, logstd, act, old_mu, old_nlp, adv, ret = _loss_rows(n, seed=1)
    row = 5
    old_nlp = old_nlp.clone(); adv = adv.clone()
    adv[row] = 1.0
    f32 = lambda t: t.float()          # noqa: E731
    mu_g, v_g = f32(mu).requires_grad_(), f32(value).requires_grad_()
    nlp = PPO.neglogp(f32(act), mu_g, torch.exp(f32(logstd)), f32(logstd).expand_as(mu_g))
    old_nlp[row] = float(nlp[row].detach()) + T.LOG_FLT_MAX + 1.0          # (finite in float64's exp, inf in fp32's)
    assert math.isfinite(math.exp(float(old_nlp[row]) - float(nlp[row].detach())))
    a_rows, _ = PPO.actor_loss(f32(old_nlp), nlp, f32(adv), C["e_clip"])
    c_rows = PPO.critic_loss(None, v_g.unsqueeze(1), C["e_clip"], f32(ret).unsqueeze(1), False)
    (a_rows.mean() + 0.5 * c_rows.mean() * C["critic_coef"]).backward()
    assert not bool(torch.isfinite(mu_g.grad[row]).all()) and bool(torch.isfinite(v_g.grad).all())
    keep = torch.arange(n) != row
    assert bool(torch.isfinite(mu_g.grad[keep]).all())
    L = T.loss(_out_of(mu, value), act, old_nlp, old_mu, adv, ret, logstd, 512.0, C["e_clip"], C["critic_coef"])
    assert math.isinf(float(L["ratio"][row])) and math.isfinite(float(L["a_loss"]))
    assert not bool(torch.isfinite(L["dmu"][row]).any()) and bool(torch.isfinite(L["dmu"][keep]).all()) and bool(torch.isfinite(L["dvalue"]).all())
    # through the rest of the backward: every gradient the poisoned row reaches belongs to the actor
    g = torch.Generator().manual_seed(2)
    h2 = torch.rand(2, n, T.HID, generator=g, dtype=torch.float64)
    gW3, _ = T.wgrad(T.dout_of(L), h2)
    gb3, _ = T.bgrad(T.dout_of(L))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)          # noqa: E731
    gfull = T.flat(z(2, T.HID, T.INP), z(2, T.HID, T.HID), gW3, z(2, T.HID), z(2, T.HID), gb3)
    assert T.found_inf(gfull) == [True, False]


def _padded(net):
    """The module's float64 parameters in the fused layout (padding zero): W1 [2][HID][INP], W2, W3 [2][OUTP][HID], b1, b2, b3 [2][OUTP]."""
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)          # noqa: E731
    W1, W2, W3, b1, b2, b3 = z(2, T.HID, T.INP), z(2, T.HID, T.HID), z(2, T.OUTP, T.HID), z(2, T.HID), z(2, T.HID), z(2, T.OUTP)
    for k, (trunk, head) in enumerate(((net.actor_mlp, net.mu), (net.critic_mlp, net.value))):
        W1[k, :, :T.IN], b1[k], W2[k], b2[k] = trunk[0].weight, trunk[0].bias, trunk[2].weight, trunk[2].bias
        W3[k, :head.weight.shape[0]], b3[k, :head.bias.shape[0]] = head.weight, head.bias
    return [t.detach().clone() for t in (W1, W2, W3, b1, b2, b3)]


def _helper_gradient(P, batch, logstd, scale, operands=False):
    """The helper's stages chained (no rounding anywhere: float64 operands): the scaled gradient in the flat layout, and the loss dict
    (operands: and the three layers' (dz, activation) pairs, what a GPU test reads back from the fused buffers)."""
    W1, W2, W3, b1, b2, b3 = P
    obs, act, old_nlp, old_mu, adv, ret = batch
    x = torch.zeros(obs.shape[0], T.INP, dtype=torch.float64)
    x[:, :T.IN] = obs
    h1 = torch.relu(T.linear(x, W1, b1)[0])
    h2 = torch.relu(T.linear(h1, W2, b2)[0])
    out = T.linear(h2, W3, b3)[0]
    L = T.loss(out, act, old_nlp, old_mu, adv, ret, logstd, scale, C["e_clip"], C["critic_coef"])
    d3 = T.dout_of(L)
    dz2 = T.masked(T.linear(d3, W3.transpose(1, 2))[0], h2)
    dz1 = T.masked(T.linear(dz2, W2.transpose(1, 2))[0], h1)
    pairs = ((dz1, x.expand(2, -1, -1)), (dz2, h1), (d3, h2))
    g = T.flat(*[T.wgrad(dz, a)[0] for dz, a in pairs], *[T.bgrad(dz)[0] for dz, _ in pairs])
    return (g, L, pairs) if operands else (g, L)


def test_gradients_clip_and_adam_equal_autograd_clip_grad_norm_and_two_adams():
    """Three updates of the full 487 -> 256 -> 256 -> 13 / 1 pair at B = 32 in float64; the second has a row that poisons the actor, whose
    optimiser is then skipped (GradScaler.step) -- so the two nets' step counts differ in the third."""
    B, scale, lrs = 32, 512.0, (3e-5, 5e-5)
    net, batches = T.make_case(PPO, 3 * B, seed=21)
    net = net.double()
    batches = [t.double() for t in batches]
    batches[2] = batches[2].clone(); batches[4] = batches[4].clone()
    batches[2][B + 3], batches[4][B + 3] = 2000.0, 1.0          # (exp overflows float64 too: the same row is inf on both sides)
    opt_a = torch.optim.Adam(net.actor_parameters(), lr=lrs[0], eps=1e-8)
    opt_c = torch.optim.Adam(net.critic_parameters(), lr=lrs[1], eps=1e-8)
    P = _padded(net)
    p = T.flat(*P)
    m, v, steps = torch.zeros_like(p), torch.zeros_like(p), [0, 0]
    mask = T.actor_mask()
    assert int(mask.sum()) == T.NP // 2
    founds = []
    for i in range(3):
        obs, act, old_nlp, old_mu, adv, ret = (t[i * B:(i + 1) * B] for t in batches)
        g, L = _helper_gradient(P, (obs, act, old_nlp, old_mu, adv, ret), net.sigma.double(), scale)
        R = T.clip_adam(g, scale, p, m, v, steps, lrs, C["grad_norm"])
        # torch
        mu, logstd, value = net(obs)
        nlp = PPO.neglogp(act, mu, torch.exp(logstd), logstd)
        a_rows, _ = PPO.actor_loss(old_nlp, nlp, adv, C["e_clip"])
        c_rows = PPO.critic_loss(None, value, C["e_clip"], ret.unsqueeze(1), False)
        for q in net.parameters():
            q.grad = None
        (a_rows.mean() + 0.5 * c_rows.mean() * C["critic_coef"]).backward()
        grads = _padded_grads(net)
        bad = [not all(bool(torch.isfinite(q.grad).all()) for q in ps) for ps in (net.actor_parameters(), net.critic_parameters())]
        founds.append(R["found"])
        assert R["found"] == bad
        if not bad[0]:
            assert _same_sums(g / scale, T.flat(*grads))
            norm = torch.nn.utils.clip_grad_norm_(net.actor_parameters(), C["grad_norm"])
            assert R["norm"] == pytest.approx(float(norm), rel=REL) and R["coef"] < 1.0
            opt_a.step()
        else:
            assert _same_sums(g / scale, T.flat(*grads)) and bool(torch.isfinite(g[~mask]).all())          # (the actor's halves are skipped: not finite)
        opt_c.step()
        p, m, v, steps = R["p"], R["m"], R["v"], R["steps"]
        P = _padded(net)
        # (Adam normalises the step: an entry whose gradient is a cancelled sum carries the summation order's 1e-9 of it into the step -- the
        #  parameters agree to 1e-7 of one step's size)
        assert float((p - T.flat(*P)).abs().max()) <= 1e-7 * min(lrs), (i, float((p - T.flat(*P)).abs().max()))
        # (the helper's own p goes on; the module's parameters are within 1e-12 of it and take its place as the next forward's operands)
        for o, name in ((opt_a, "actor"), (opt_c, "critic")):
            st = [o.state[q] for q in o.param_groups[0]["params"] if q in o.state]
            assert all(int(s["step"]) == steps[name == "critic"] for s in st)
    assert founds == [[False, False], [True, False], [False, False]] and steps == [2, 3]
    moments = _padded_moments(net, opt_a, opt_c)
    assert _same_sums(m, T.flat(*moments[0])) and _same_sums(v, T.flat(*moments[1]))


def _padded_like(net, get):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)          # noqa: E731
    W1, W2, W3, b1, b2, b3 = z(2, T.HID, T.INP), z(2, T.HID, T.HID), z(2, T.OUTP, T.HID), z(2, T.HID), z(2, T.HID), z(2, T.OUTP)
    for k, (trunk, head) in enumerate(((net.actor_mlp, net.mu), (net.critic_mlp, net.value))):
        W1[k, :, :T.IN], b1[k], W2[k], b2[k] = get(trunk[0].weight), get(trunk[0].bias), get(trunk[2].weight), get(trunk[2].bias)
        W3[k, :head.weight.shape[0]], b3[k, :head.bias.shape[0]] = get(head.weight), get(head.bias)
    return [W1, W2, W3, b1, b2, b3]


def _padded_grads(net):
    return _padded_like(net, lambda q: q.grad)


def _padded_moments(net, opt_a, opt_c):
    st = dict(opt_a.state)
    st.update(opt_c.state)
    return _padded_like(net, lambda q: st[q]["exp_avg"]), _padded_like(net, lambda q: st[q]["exp_avg_sq"])


@pytest.mark.parametrize("R", [2, 3])
def test_the_average_of_the_ranks_gradients_is_the_gradient_of_the_mean_loss_over_the_union(R):
    """What the sharded update's "average" means (tests/test_ppo_sharded_gpu.py): R ranks with B_r rows each; float64 autograd on the consumer's
    own loss functions gives every rank the gradient of ITS mean loss, and the mean of those over the ranks is the gradient of the mean loss
    over all R B_r rows.  `rank_bucket` is a rank's gradient times the loss scale / R and `bucket_sum` of the ranks' buckets is that
    average, times the scale; their bounds are first-order sums of |terms| and vanish only where every term does."""
    B, scale = 32, 512.0
    net, batch = T.make_case(PPO, R * B, seed=40 + R)
    net = net.double()
    batch = [t.double() for t in batch]
    P = _padded(net)

    def autograd(rows):
        obs, act, old_nlp, old_mu, adv, ret = (t[rows] for t in batch)
        mu, logstd, value = net(obs)
        a_rows, _ = PPO.actor_loss(old_nlp, PPO.neglogp(act, mu, torch.exp(logstd), logstd), adv, C["e_clip"])
        c_rows = PPO.critic_loss(None, value, C["e_clip"], ret.unsqueeze(1), False)
        for q in net.parameters():
            q.grad = None
        (a_rows.mean() + 0.5 * c_rows.mean() * C["critic_coef"]).backward()
        return T.flat(*_padded_grads(net))
    own = [autograd(slice(r * B, (r + 1) * B)) for r in range(R)]
    union = autograd(slice(0, R * B))
    average = sum(own) / R
    assert _same_sums(average, union) and float(union.abs().max()) > 0.0
    assert not _same_sums(sum(own), union) and not _same_sums(own[0], union)          # (neither the sum nor one rank's own)
    buckets, bounds = [], []
    for r in range(R):
        g, _, pairs = _helper_gradient(P, [t[r * B:(r + 1) * B] for t in batch], net.sigma.double(), scale, operands=True)
        t, bound = T.rank_bucket(pairs, B, R)
        assert _same_sums(t, g / R) and _same_sums(t / scale, own[r] / R)
        assert bool((bound >= T.U32 * t.abs()).all()) and bool(((bound == 0) == (g == 0)).all())
        buckets.append(t); bounds.append(bound)
    total, reduce_bound = T.bucket_sum(buckets)
    assert _same_sums(total / scale, average) and _same_sums(total / scale, union)
    assert torch.equal(total, sum(buckets[1:], buckets[0])) and torch.equal(reduce_bound, (R - 1) * T.U32 * sum(b.abs() for b in buckets))
    # the emulated all-reduce in fp32 stays inside its bound
    got = buckets[0].float()
    for b in buckets[1:]:
        got = got + b.float()
    exact, rb = T.bucket_sum([b.float() for b in buckets])
    assert bool(((T.f64(got) - exact).abs() <= rb).all())


def test_scaler_moves_as_gradscaler_does():
    s, gr = 65536.0, 0
    s, gr = T.scaler_update(s, gr, True, 3)
    assert (s, gr) == (32768.0, 0)
    hist = []
    for _ in range(7):
        s, gr = T.scaler_update(s, gr, False, 3)
        hist.append((s, gr))
    assert hist == [(32768.0, 1), (32768.0, 2), (65536.0, 0), (65536.0, 1), (65536.0, 2), (131072.0, 0), (131072.0, 1)]
    assert T.scaler_update(s, 2, True, 3) == (65536.0, 0)


# ------------------------------------------------------------------------------------------------ dwp_wgrad's slabs
def test_wgrad_slabs_tile_the_k_blocks_exactly():
    """k_wgrad's per / kb0 / kb1 (csrc/dw_ppo.hip), restated: for every nkb = B / 32 in 1 .. 64 the four slabs are consecutive, start at 0, end
    at nkb, none longer than per, and an empty slab has kb0 = kb1 = nkb."""
    for nkb in range(1, 65):
        tab = T.wgrad_slabs(nkb)
        per = -(-nkb // T.WG_SLABS)
        assert len(tab) == T.WG_SLABS and tab[0][0] == 0 and tab[-1][1] == nkb
        for s, (a, b) in enumerate(tab):
            assert 0 <= a <= b <= nkb and b - a <= per
            if s:
                assert a == tab[s - 1][1]
        assert sorted(k for a, b in tab for k in range(a, b)) == list(range(nkb))
        assert T.slab_nk(32 * nkb) == [b - a for a, b in tab]


def test_the_gpu_tests_sizes_are_the_ring_and_bucket_edges():
    """The minibatch sizes at which the matrix-core form takes another path come out of `edge_sizes`; per size, the k-steps per slab."""
    assert {B: nk for B, (nk, _) in T.edge_sizes().items()} == {
        32: [1, 0, 0, 0], 96: [1, 1, 1, 0], 160: [2, 2, 1, 0], 416: [4, 4, 4, 1], 640: [5, 5, 5, 5], 672: [6, 6, 6, 3], 1056: [9, 9, 9, 6],
        1312: [11, 11, 11, 8]}
    assert T.wgrad_slabs(5)[3] == (5, 5)          # (3 * per = 6 is past the end: kb0 is clamped)
    assert T.slab_nk(4096) == [32] * 4            # (what tests/test_ppo_gpu.py runs)


def _fp32_slabs(dz, act, table):
    """Per-slab partial gradients as an fp32 accumulation gives them (the stand-in for the kernel in the two tests below)."""
    return torch.stack([(dz[..., r, :].float().transpose(-1, -2) @ act[..., r, :].float()) for r in T.slab_rows(dz.shape[-2], table)])


@pytest.mark.parametrize("B", [32, 160, 672, 1312])
def test_per_slab_comparison_rejects_a_mis_tiled_slab_table(B):
    """Sensitivity: partial gradients formed with the right slabs pass the per-slab comparison; formed with the last k-block of a slab dropped
    whenever nk % RD == 1 (the refill guard `k + RD - 1 < nk` off by one would do that) -- or compared against such a table -- they miss the
    bound by orders of magnitude, and an empty slab that is not zero is rejected outright."""
    g = torch.Generator().manual_seed(B)
    dz = torch.randn(2, B, T.OUTP, generator=g).half()
    act = torch.rand(2, B, T.HID, generator=g).half()
    good = T.wgrad_slabs(B // 32)
    bad = [(a, b - 1) if (b - a) % T.WG_RD == 1 else (a, b) for a, b in good]
    assert bad != good
    right = _fp32_slabs(dz, act, good)
    assert T.worst_slab_fraction(right, dz, act) <= 1.0
    assert T.worst_slab_fraction(_fp32_slabs(dz, act, bad), dz, act) > 1e3
    if all(b > a for a, b in bad):          # (the helper given the wrong table: it must not agree with a right kernel either)
        assert T.worst_slab_fraction(right, dz, act, table=bad) > 1e3
    if 0 in T.slab_nk(B):
        s = T.slab_nk(B).index(0)
        right[s, 0, 3, 7] = 1e-30
        assert T.worst_slab_fraction(right, dz, act) == math.inf


def test_linear_bound_holds_for_an_fp32_accumulation_and_is_not_vacuous():
    g = torch.Generator().manual_seed(4)
    a, w, b = torch.randn(65, T.INP, generator=g).half(), (0.06 * torch.randn(T.HID, T.INP, generator=g)).half(), (0.1 * torch.randn(T.HID, generator=g)).half()
    t, bound = T.linear(a, w, b)
    got = (a.float() @ w.float().T + b.float()).half()
    frac = float(((T.f64(got) - t).abs() / bound).max())
    assert 0.05 < frac <= 1.0, frac
    # the library-GEMM form's two roundings
    t2, bound2 = T.linear(a, w, b, double_rounded=True)
    got2 = ((a.float() @ w.float().T).half().float() + b.float()).half()
    assert float(((T.f64(got2) - t2).abs() / bound2).max()) <= 1.0 and bool((bound2 >= bound).all())
    # one flipped low bit of an fp16 result is outside it
    off = (got.view(torch.int16) ^ 2).view(torch.float16)
    assert float(((T.f64(off) - t).abs() / bound).max()) > 1.0


def test_ring_depth_is_the_kernels():
    """`edge_sizes` is built on wgrad_block's ring depth: the helper's WG_RD is the kernel's `constexpr int RD`, read from the source."""
    import os
    import re
    src = open(os.path.join(T.ROOT, "isaacgymdyros_amd", "csrc", "dw_ppo.hip")).read()
    body = src[src.index("void wgrad_block("):src.index("struct WgradArgs")]
    assert [int(x) for x in re.findall(r"constexpr int RD = (\d+);", body)] == [T.WG_RD]
    assert "for (int i = 0; i < RD - 1; ++i) if (nk > i) request(i, kb0 + i);" in body and "if (k + RD - 1 < nk)" in body


def test_dmu_bound_holds_for_an_fp32_evaluation_of_the_consumers_loss_and_is_not_vacuous():
    """The output gradients' derived bound against something that rounds: the consumer's loss functions and autograd in fp32 on fp16 head
    outputs, the gradient then rounded to fp16 -- within the bound at every sample off the clip boundary, not far inside it, and a result
    two fp16 ulps off is outside."""
    B = 672
    net, (obs, act, nlp_old, mu_old, adv, ret) = T.make_case(PPO, B, 31)
    out = T.emulated_out(net, obs)
    scale = 16.0 * B
    L = T.loss(out, act, nlp_old, mu_old, adv, ret, net.sigma, scale, C["e_clip"], C["critic_coef"])
    mu, v = out[0, :, :T.ACT].float().requires_grad_(), out[1, :, :1].float().requires_grad_()
    logstd = net.sigma.expand_as(mu)
    nlp = PPO.neglogp(act, mu, torch.exp(logstd), logstd)
    a_rows, _ = PPO.actor_loss(nlp_old, nlp, adv, C["e_clip"])
    c_rows = PPO.critic_loss(None, v, C["e_clip"], ret.unsqueeze(1), False)
    (scale * (a_rows.mean() + 0.5 * c_rows.mean() * C["critic_coef"])).backward()
    keep = L["margin"].abs() >= T.CLIP_MARGIN
    assert int((~keep).sum()) == 0
    got_mu, got_v = mu.grad.half(), v.grad.half().reshape(-1)
    fm = float(((T.f64(got_mu) - L["dmu"]).abs() / L["dmu_bound"])[keep].max())
    fv = float(((T.f64(got_v) - L["dvalue"]).abs() / L["dvalue_bound"]).max())
    assert 0.3 < fm <= 1.0 and 0.3 < fv <= 1.0, (fm, fv)
    big = L["dmu"].abs() > 1e-2          # (normal fp16 numbers; the bound is between half an ulp and one: two ulps off is outside)
    off = (got_mu.view(torch.int16) ^ 2).view(torch.float16)
    assert float(((T.f64(off) - L["dmu"]).abs() / L["dmu_bound"])[big].min()) > 1.0


# ------------------------------------------------------------------------------------------------ the GPU tests' cases and checks, without a GPU
def _emulated(form, B, fault=None):
    import ppo_update_emul as E
    import test_ppo_edges_gpu as G
    net, batch = T.make_case(PPO, T.NMB * B, T.case_seed(form, B))
    return E.EmulatedUpdate(net, C, B, batch, 16.0 * B, G.LR, mfma=form == "mfma", fault=fault), net, batch


def test_the_gpu_cases_have_at_most_two_samples_on_the_clip_boundary():
    """tests/test_ppo_edges_gpu.py may leave a sample whose float64 |ratio - 1| is within 1e-5 of e_clip out of the dmu and clip-fraction
    comparisons (fp32 may put it on the other side): at most one per case, two over all cases.  The cases' seeds (`case_seed`) meet that on
    the reference alone, over all FOUR updates of a case (the parameters, and with them the ratios, move after the first): the update
    emulated on the CPU (tests/ppo_update_emul.py) brings no sample of any case that close."""
    left, nearest = set(), math.inf
    for form, B in [("mfma", B) for B in T.edge_sizes()] + [("gemm", B) for B in T.GEMM_SIZES]:
        f, _, _ = _emulated(form, B)
        for it in range(4):
            mb = int(f.state[T.K["DWP_S_MB"]])
            f.update()
            near = (f.L["margin"].abs() < T.CLIP_MARGIN).nonzero().reshape(-1).tolist()
            left |= {(form, B, mb, r) for r in near}
            nearest = min(nearest, float(f.L["margin"].abs().min()))
            cf = float(f.L["clip_frac"])
            assert B < 256 or 0.05 < cf < 0.95, (form, B, cf)
        assert len([k for k in left if k[:2] == (form, B)]) <= 1, sorted(left)
    assert len(left) <= 2, sorted(left)
    assert not left and nearest > T.CLIP_MARGIN, (sorted(left), nearest)


@pytest.mark.parametrize("form,B", [("mfma", 32), ("mfma", 160), ("gemm", 65)])
def test_the_gpu_checks_pass_an_emulated_update(form, B, monkeypatch):
    """tests/test_ppo_edges_gpu.py's stage-by-stage checks, run here on the CPU emulation of the update over a case's four updates: they pass
    arithmetic that rounds where the kernels round."""
    import types
    import test_ppo_edges_gpu as G
    monkeypatch.setattr(G, "DEV", "cpu")
    monkeypatch.setattr(G, "LEFT_OUT", set())
    f, net, batch = _emulated(form, B)
    U, worst = types.SimpleNamespace(K=T.K), {}
    for _ in range(G.UPDATES):
        snap = G._snapshot(U, f)
        f.update()
        G._check_update(U, "emulated", f, net, batch, snap, worst)
    assert int(f.state[T.K["DWP_S_MB"]]) == 1 and max(worst.values()) <= 1.0 and max(worst.values()) > 0.5


@pytest.mark.parametrize("fault", ["dropped_k_block", "empty_slab_not_cleared", "bucket_not_cleared", "dz1_not_masked", "actor_stepped_twice"])
def test_the_gpu_checks_reject_an_emulated_update_with_a_fault(fault, monkeypatch):
    """... and they do not pass the same update with one fault put in: a k-block dropped from every slab, an empty slab's copy of the gradient
    left with a stale word, an accumulator bucket not cleared, dz1 stored without its relu mask, a step count off by one.  (The kernels are
    never broken for this: the fault is in the CPU stand-in.)"""
    import types
    import test_ppo_edges_gpu as G
    import ppo_update_emul as E
    assert fault in E.FAULTS
    monkeypatch.setattr(G, "DEV", "cpu")
    monkeypatch.setattr(G, "LEFT_OUT", set())
    f, net, batch = _emulated("mfma", 160, fault)
    U = types.SimpleNamespace(K=T.K)
    snap = G._snapshot(U, f)
    f.update()
    with pytest.raises(AssertionError):
        G._check_update(U, "emulated", f, net, batch, snap, {})
