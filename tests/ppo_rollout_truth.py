"""The walk learner's rollout kernels (include/dyros_ppo.h, csrc/dw_ppo.hip: dwp_rollout_pre / _post, dwp_gae, dwp_policy) restated twice, on the
CPU, in numpy:

  * in float64, stage by stage, from the fp32 operands THE KERNEL HAD, each with an error bound that follows from the arithmetic in the source
    and not from what a kernel was seen to give (`act_truth`, `nlp_truth`, `rew_truth`, `terms_truth`, `gae_truth`, `policy_truth`), and the
    checks that hold a call's buffers -- the whole allocation, guard rows included, before and after the call -- to that truth
    (`check_pre`, `check_post`, `check_gae`, `check_policy`).  tests/test_ppo_rollout_edges_gpu.py runs them on the kernels;
  * in fp32 AS LAUNCHED (`launched_pre`, `launched_post`, `launched_gae`, `launched_policy`): the items are served by a grid of the
    launcher's size (`pre_blocks`, `post_blocks`: the formulas of the launchers in csrc/dw_ppo.hip), so a grid that is short of the items
    leaves them unwritten here as it does on the GPU.  Each takes a `fault` (FAULTS); tests/test_ppo_rollout_truth.py shows that the
    checks pass the clean restatement and reject every fault.

Arithmetic model.  u = 2^-24: one fp32 rounding to nearest is a relative error of at most u.  expf is taken to be within 2 ulp = 4 u; a
division within 1 ulp = 2 u; an atomic add of the memory side within 1 ulp = 2 u.  Bounds are first order in u; the factor SECOND covers the
products of two such terms (the longest chain here has about a thousand roundings: (1 + u)^1000 - 1 exceeds 1000 u by 3e-5 of itself), and FLT_MIN
is added for a result in the subnormal range, which the hardware may flush.

Buffers.  Every output of a call is allocated with guard rows: [1 + rows + 1] rows of which the kernel is handed row 1 on (`alloc_pre`,
`alloc_post`, `alloc_gae`; `alloc_policy`: 1 + N + 32 rows, a whole row tile past the end), all filled with NaN (fp16: the NaN 0x7e00, which
also stands as the sentinel of the padding no call writes).  A check compares the WHOLE allocation: bit for bit where the result is a copy,
within the bound where it is arithmetic, and bit for bit with `before` everywhere else.  A check returns {name: worst error / bound}; an exact
comparison gives 0 or inf; `failures` lists the names above 1."""
from __future__ import annotations

import importlib.util
import math
import os

import numpy as np

from isaacgymdyros_amd import cbind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = cbind.constants("dyros_ppo.h", "dwp_")
IN, INP, HID, OUTP, ACT = K["DWP_IN"], K["DWP_INP"], K["DWP_HID"], K["DWP_OUTP"], K["DWP_ACT"]
TERMS_MAX = K["DWP_ROLL_TERMS_MAX"]
MT = 32                      # k_policy's rows per workgroup (csrc/dw_ppo.hip `MT = 16 * MR`, MR = 2)
POLICY_GUARD = MT            # guard rows after a policy output: a whole row tile
U = 2.0 ** -24
EXP_REL, DIV_REL, ATOMIC_REL = 4 * U, 2 * U, 2 * U
FLT_MIN = 2.0 ** -126
SECOND = 1.0 + 2.0 ** -13
F32, F64 = np.float32, np.float64
FAULTS = ("short_grid", "swap_env_major", "half_tail", "no_bootstrap", "gae_wrong_step", "terms_div_256", "row_past_n", "policy_rows_swapped")


def consumer():
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def f64(a):
    return np.asarray(a, dtype=F64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def exact(got, want) -> float:
    """0 where two arrays are the same bits (NaN payloads included), inf otherwise."""
    return 0.0 if got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want)) else math.inf


def ratio(got, t, bound) -> float:
    """max |got - t| / bound; inf where anything is not finite."""
    r = np.abs(f64(got) - t) / bound
    return float(r.max()) if r.size and bool(np.isfinite(r).all()) else (math.inf if r.size else 0.0)


def failures(res: dict) -> list:
    return sorted(k for k, v in res.items() if not v <= 1.0)


def nan32(*shape):
    return np.full(shape, np.nan, dtype=F32)


# ------------------------------------------------------------------------------------------------ float64 truth and derived bounds
def act_truth(mu, noise, logstd):
    """a = mu + exp(logstd) * noise and the bound of its fp32 value.  The kernel forms s = expf(logstd) (4 u), then either p = fl(s * noise) (u)
    and fl(mu + p) (u |mu + p|), or one fused fl(mu + s * noise) (u |a|): in both |a32 - a| <= u |a| + (4 u + u) |sigma noise| to first order
    (the unfused form's u |mu + p| is u |a| plus a second-order term)."""
    sg = np.exp(f64(logstd))
    p = sg * f64(noise)
    t = f64(mu) + p
    return t, (U * np.abs(t) + (EXP_REL + U) * np.abs(p)) * SECOND + FLT_MIN


def nlp_truth(a_stored, mu, noise, logstd):
    """neglogp (models_dyros.py:59-62) of the STORED action, and its bound.  z = (a - mu) / sigma: in float64 the difference of the two fp32
    words is exact.  The kernel's thread does not read the stored word, it evaluates mu + s * noise a second time, in another expression that
    the compiler may contract differently from the one that was stored: both are within `act_truth`'s bound b of the same float64 value, so
    the a that enters z is within 2 b of the stored one -- an ABSOLUTE error that the cancellation in a - mu does not shrink, 2 b / sigma in z.
    On top: the subtraction u, expf 4 u, the division 2 u, relative to |z|.  dz = 7 u |z| + 2 b / sigma.
    sq = sum of 13 z^2, accumulated in order: 2 |z| dz + dz^2 per term, one product and at most 12 additions -> 14 u sq.
    lsum = sum of 13 logstd: 13 u sum |logstd|.  The constant 0.5 log(2 pi) 13 is an fp32 literal times 13: 2 u of it.  0.5 sq is exact,
    + constant: u (0.5 sq + c), + lsum: u |result|."""
    sg, ls = np.exp(f64(logstd)), f64(logstd)
    z = (f64(a_stored) - f64(mu)) / sg
    _, b = act_truth(mu, noise, logstd)
    dz = (U + EXP_REL + DIV_REL) * np.abs(z) + 2.0 * b / sg
    sq = (z * z).sum(-1)
    c = 0.5 * math.log(2.0 * math.pi) * ACT
    t = 0.5 * sq + c + ls.sum()
    e_sq = (2.0 * np.abs(z) * dz + dz * dz).sum(-1) + (ACT + 1) * U * sq
    bound = (0.5 * e_sq + 2 * U * c + ACT * U * np.abs(ls).sum() + U * (0.5 * sq + c) + U * np.abs(t)) * SECOND
    return t, bound


def rew_truth(rew, value, time_outs, scale, gamma):
    """mb_rew = rew * scale (+ gamma * value * time_outs, the bootstrap of a2c_common_dyros.py:656-659) from the fp32 scalars the launcher was
    handed.  Without time_outs: one rounding, u |rew scale|.  With them, three: r = fl(rew scale) (u |rew scale|), fl(gamma value) (u |boot|; the
    factor time_outs is 0 or 1 and then exact -- a second u |boot| is allowed for another integer), and the sum (u |result|, fused or not)."""
    rs = f64(rew) * float(F32(scale))
    if time_outs is None:
        return rs, U * np.abs(rs) * SECOND + FLT_MIN
    boot = float(F32(gamma)) * f64(value) * f64(time_outs)
    t = rs + boot
    return t, U * (np.abs(rs) + 2.0 * np.abs(boot) + np.abs(t)) * SECOND + FLT_MIN


def terms_truth(t0, stacked, nterms, N):
    """terms[c] = t0[c] + mean over the envs of column c.  A workgroup of 256 envs: the wave's butterfly of 6 levels (6 u of the wave's sum of
    |.|), the four waves' partials in order (3 u), the division by N (2 u): its share of the mean is within 11 u of its sum |.| / N.  Then
    B = ceil(N / 256) atomic adds onto t0 in any order: every partial sum is at most |t0| + A, A = sum |.| / N, so B * 2 u (|t0| + A)."""
    s = f64(stacked)[:, :nterms]
    A = np.abs(s).sum(0) / N
    B = (N + 255) // 256
    t0 = f64(t0)
    return t0 + s.sum(0) / N, ((6 + 3) * U + DIV_REL) * A * SECOND + ATOMIC_REL * B * (np.abs(t0) + A) * SECOND + FLT_MIN


def gae_scalars(gamma, tau):
    """(gamma, gamma * tau) as k_gae has them: the C float gamma, and the launcher's (float)((double)gamma * (double)tau)."""
    g, t = float(F32(gamma)), float(F32(tau))
    return g, float(F32(g * t))


def gae_truth(fdones, last_values, mb_fdones, mb_values, mb_rewards, gamma, tau):
    """`discount_values` (a2c_common_dyros.py:485-500) in float64 from the fp32 inputs, [H][N], with k_gae's two scalars, and its bound E.
    Per step, with nn = 1 - done of the step after (u |nn|: exact for flags of 0 and 1), G = |gamma tau nn| and
    A = |rew| + |gamma nextvalue nn| + |val|:
      delta = fl(fl(rew + fl(fl(gamma nextvalue) nn)) - val): three roundings in the product (nn's own included), one per sum: at most 5 u A;
      lam   = fl(delta + fl(fl(gamma_tau nn) lam')): 3 u G |lam'| in the product, u (|delta| + G |lam'|) in the sum, and lam' itself carries E'.
    With Labs = A + G Labs' >= |lam| (the same recursion on absolute values): local error <= 6 u A + 4 u G Labs' and E = 6 u Labs + G E'.
    The 2 u G Labs' that the last step leaves unused is what a reference loop may spend on a gamma * tau rounded differently (a Python
    product of two doubles, rounded to fp32 by the multiply: one ulp from the launcher's)."""
    g, gt = gae_scalars(gamma, tau)
    fd, lv, mfd, mv, mr = f64(fdones).reshape(-1), f64(last_values).reshape(-1), f64(mb_fdones), f64(mb_values), f64(mb_rewards)
    H, N = mr.shape[0], fd.shape[0]
    mfd, mv, mr = mfd.reshape(H, N), mv.reshape(H, N), mr.reshape(H, N)
    adv, E = np.zeros((H, N)), np.zeros((H, N))
    lam, labs, e, nn, nv = np.zeros(N), np.zeros(N), np.zeros(N), 1.0 - fd, lv
    for t in range(H - 1, -1, -1):
        delta = mr[t] + g * nv * nn - mv[t]
        A = np.abs(mr[t]) + np.abs(g * nv * nn) + np.abs(mv[t])
        G = np.abs(gt * nn)
        lam = delta + gt * nn * lam
        labs = A + G * labs
        e = 6 * U * labs * SECOND + G * e + FLT_MIN
        adv[t], E[t] = lam, e
        nn, nv = 1.0 - mfd[t], mv[t]
    return adv, E


POLICY_C = 2.0


def policy_bound(S):
    """c (IN + 2 HID + 8) u S for an fp32 evaluation of the three layers in any summation order, S = the forward with the absolute value of
    every operand (`policy_truth`).  A dot product of K terms and its bias: every term passes through its product's rounding, at most K - 1
    additions and the bias's, K + 1 roundings, so the layer is within (K + 1) e S_layer, e the error of one operation; relu and the next layers'
    |W| carry that to the output as (K + 1) e S.  Three layers: (IN + 1) + (HID + 1) + (HID + 1) = IN + 2 HID + 3 <= IN + 2 HID + 8 (the zero
    padding of the 487 inputs to 512 adds exact zeros).  e: the matrix instruction's rounding of its inner sums is not specified to be to
    nearest; a truncating adder is within one ulp = 2 u.  Hence c = 2."""
    return POLICY_C * (IN + 2 * HID + 8) * U * S * SECOND + FLT_MIN


def weights_of(net) -> dict:
    """The fp32 parameters of a DyrosActorCritic (examples/ppo_consumer.py) as numpy: W1 [2][HID][IN], b1 [2][HID], W2, b2, W3 / b3: lists
    (actor [ACT][HID] / [ACT], critic [1][HID] / [1])."""
    np_ = lambda p: p.detach().cpu().float().numpy().copy()          # noqa: E731
    tr = [[m for m in t if hasattr(m, "weight")] for t in (net.actor_mlp, net.critic_mlp)]
    return {"W1": np.stack([np_(t[0].weight) for t in tr]), "b1": np.stack([np_(t[0].bias) for t in tr]),
            "W2": np.stack([np_(t[1].weight) for t in tr]), "b2": np.stack([np_(t[1].bias) for t in tr]),
            "W3": [np_(net.mu.weight), np_(net.value.weight)], "b3": [np_(net.mu.bias), np_(net.value.bias)]}


def _forward(W, obs, dtype, absolute=False):
    a = (lambda x: np.abs(x)) if absolute else (lambda x: x)
    outs = []
    for k in range(2):
        x = a(np.asarray(obs, dtype=dtype))
        for w, b in ((W["W1"][k], W["b1"][k]), (W["W2"][k], W["b2"][k])):
            x = np.maximum(x @ a(w.astype(dtype)).T + a(b.astype(dtype)), 0)
        outs.append(x @ a(W["W3"][k].astype(dtype)).T + a(W["b3"][k].astype(dtype)))
    return outs[0], outs[1][:, 0]


def policy_truth(W, obs):
    """(mu [N][ACT], value [N], bound of mu, bound of value) in float64 from the fp32 weights and observations."""
    mu, v = _forward(W, obs, F64)
    smu, sv = _forward(W, obs, F64, absolute=True)
    return mu, v, policy_bound(smu), policy_bound(sv)


# ------------------------------------------------------------------------------------------------ buffers with guard rows
def alloc_pre(N, H, nobs, layout):
    """layout: "step" mb_obs [H][N][nobs] fp32, "env" [N][H][nobs] fp32, "half" [N][H][INP] fp16 (as uint16 words).  One guard row (a step's
    row, or one env-step's row in the env-major forms) before and after; the kernel gets row 1 on."""
    obs = nan32(H + 2, N * nobs) if layout == "step" else nan32(N * H + 2, nobs) if layout == "env" else \
        np.full((N * H + 2, INP), np.nan, dtype=np.float16).view(np.uint16)
    return {"mb_obs": obs, "mb_act": nan32(H + 2, N * ACT), "mb_mu": nan32(H + 2, N * ACT), "mb_nlp": nan32(H + 2, N), "mb_val": nan32(H + 2, N),
            "mb_done": nan32(H + 2, N), "act": nan32(3, N * ACT)}


def alloc_post(inp, rng):
    """The g_obs == new_obs form (inp["same"]): the env's own buffer, `new_obs` [3][N * nobs] with the observations in row 1, is handed over
    as both and must come back as it was.  terms (nterms > 0): row 1 holds the epoch's sums so far."""
    N, H, nobs, nterms = inp["N"], inp["H"], inp["nobs"], inp["nterms"]
    b = {"mb_rew": nan32(H + 2, N), "g_dones": nan32(3, N)}
    if inp["same"]:
        b["new_obs"] = nan32(3, N * nobs)
        b["new_obs"][1] = inp["new_obs"].reshape(-1)
    else:
        b["g_obs"] = nan32(3, N * nobs)
    if nterms:
        b["terms"] = nan32(3, nterms)
        b["terms"][1] = rng.standard_normal(nterms).astype(F32)
    return b


def alloc_gae(N, H):
    return {"advs": nan32(H + 2, N)}


def alloc_policy(N):
    return {"mu": nan32(1 + N + POLICY_GUARD, ACT), "value": nan32(1 + N + POLICY_GUARD)}


def pre_inputs(rng, N, H, nobs, n, layout):
    r = lambda *s: rng.standard_normal(s).astype(F32)          # noqa: E731
    obs = r(N, nobs) * F32(3.0)
    obs[rng.random((N, nobs)) < 0.02] *= F32(1e-6)          # (fp16 subnormals and zeros among the halves)
    return {"mu": r(N, ACT), "value": r(N), "noise": r(N, ACT), "obs": obs, "dones": (rng.random(N) < 0.2).astype(F32),
            "logstd": (F32(-2.3) + F32(0.3) * r(ACT)), "n": int(n), "N": N, "nobs": nobs, "H": H, "layout": layout}


def post_inputs(rng, N, H, nobs, n, nterms=15, ncols=None, time_outs=True, same=False, scale=0.3, gamma=0.99):
    r = lambda *s: rng.standard_normal(s).astype(F32)          # noqa: E731
    ncols = (nterms + 3 if ncols is None else ncols) if nterms else 0
    return {"rew": r(N), "value": r(N), "time_outs": (rng.random(N) < 0.3).astype(np.int64) if time_outs else None,
            "stacked": r(N, ncols) + F32(0.5) if nterms else None, "ncols": ncols, "nterms": nterms, "done": (rng.random(N) < 0.2).astype(np.int64),
            "new_obs": r(N, nobs), "n": int(n), "N": N, "nobs": nobs, "H": H, "scale": scale, "gamma": gamma, "same": bool(same)}


DONE_PATTERNS = ("never", "always", "last_step", "random", "fdones")


def gae_inputs(rng, N, H, pattern, p=0.05):
    """never / always: mb_fdones all 0 / all 1; last_step: 1 in row H - 1 only; random: p of the flags; fdones: random, and the flags after the
    last step (fdones) all set."""
    r = lambda *s: rng.standard_normal(s).astype(F32)          # noqa: E731
    mfd = np.zeros((H, N), F32)
    if pattern == "always":
        mfd[:] = 1
    elif pattern == "last_step":
        mfd[H - 1] = 1
    elif pattern in ("random", "fdones"):
        mfd = (rng.random((H, N)) < p).astype(F32)
    fd = np.ones(N, F32) if pattern == "fdones" else (rng.random(N) < p).astype(F32) if pattern == "random" else np.zeros(N, F32)
    return {"fdones": fd, "last_values": r(N), "mb_fdones": mfd, "mb_values": r(H, N), "mb_rewards": r(H, N), "gamma": 0.99, "tau": 0.95, "N": N, "H": H}


DEAD_UNITS = (3, 100, 255)


def policy_net(seed=0):
    """A DyrosActorCritic (CPU, fp32) with lively weights -- orthogonal with gain 1 instead of the yaml's 0.01, biases in +-0.1 -- and a few
    dead units in both hidden layers of both nets (a zero weight row under a bias of -1: relu gives 0 for every input)."""
    import torch
    ppo = consumer()
    torch.manual_seed(seed)
    net = ppo.DyrosActorCritic(IN, ACT, ppo.TRAIN_CFG["network"])
    with torch.no_grad():
        for p in net.parameters():
            if p.requires_grad and p.dim() == 2:
                torch.nn.init.orthogonal_(p, gain=1.0)
            elif p.requires_grad:
                p.uniform_(-0.1, 0.1)
        for trunk in (net.actor_mlp, net.critic_mlp):
            for lin in (trunk[0], trunk[2]):
                for d in DEAD_UNITS:
                    lin.weight[d].zero_()
                    lin.bias[d] = -1.0
    return net


def policy_big_rows(rows):
    return [r for r in range(rows) if r == 0 or r % 256 == 14]


def policy_obs(rows, seed=0):
    """[rows][IN] fp32: row 0 and every row 14 + 256 k scaled by 1e3 (`policy_big_rows`), rows 2 and rows - 1 (the last row, the one a tile past
    the end re-reads) all zero."""
    obs = np.random.default_rng(seed).standard_normal((rows, IN)).astype(F32)
    obs[policy_big_rows(rows)] *= F32(1e3)
    for r in (2, rows - 1):
        if 0 < r < rows:
            obs[r] = 0
    return obs


def half_row_words(nobs):
    return 8 * ((nobs + 7) // 8)          # a row's fp16 words up to the end of its last 16-byte piece


# ------------------------------------------------------------------------------------------------ the checks
def _outside_row(got, before, row) -> float:
    """Every row but `row` (None: every row) is what it was."""
    g, b = got.copy(), before
    if row is not None:
        g[row] = b[row]
    return exact(g, b)


def check_pre(inp, before, after) -> dict:
    N, H, nobs, n, layout = inp["N"], inp["H"], inp["nobs"], inp["n"], inp["layout"]
    in_rows = 0 <= n < H
    row = 1 + n if in_rows else None
    want = {k: before[k].copy() for k in ("mb_obs", "mb_mu", "mb_val", "mb_done")}
    if in_rows:
        want["mb_mu"][row], want["mb_val"][row], want["mb_done"][row] = inp["mu"].reshape(-1), inp["value"].reshape(-1), inp["dones"]
        if layout == "step":
            want["mb_obs"][row] = inp["obs"].reshape(-1)
        else:
            rows = 1 + np.arange(N) * H + n
            if layout == "env":
                want["mb_obs"][rows] = inp["obs"]
            else:          # obs.half(), zeros up to the end of the row's last 16-byte piece, and nothing after it
                w = half_row_words(nobs)
                want["mb_obs"][rows, :w] = 0
                want["mb_obs"][rows, :nobs] = inp["obs"].astype(np.float16).view(np.uint16)
    res = {k: exact(after[k], want[k]) for k in want}
    t, b = act_truth(inp["mu"], inp["noise"], inp["logstd"])
    for k in ("mb_act", "mb_nlp"):
        res[k + "_rest"] = _outside_row(after[k], before[k], row)
    res["act_guards"] = _outside_row(after["act"], before["act"], 1)
    if in_rows:
        stored = after["mb_act"][row].reshape(N, ACT)
        res["mb_act"] = ratio(stored, t, b)
        res["act"] = exact(after["act"][1], np.clip(stored, F32(-1), F32(1)).reshape(-1))          # clip_actions of the STORED action
        tn, bn = nlp_truth(stored, inp["mu"], inp["noise"], inp["logstd"])
        res["mb_nlp"] = ratio(after["mb_nlp"][row], tn, bn)
    else:          # (nothing is recorded; the env still gets its action: clamp is 1-Lipschitz)
        res["act"] = ratio(after["act"][1].reshape(N, ACT), np.clip(t, -1.0, 1.0), b)
    return res


def check_post(inp, before, after) -> dict:
    N, H, n = inp["N"], inp["H"], inp["n"]
    in_rows = 0 <= n < H
    row = 1 + n if in_rows else None
    res = {}
    want = before["g_dones"].copy()
    want[1] = inp["done"].astype(F32)
    res["g_dones"] = exact(after["g_dones"], want)
    if inp["same"]:
        res["g_obs"] = exact(after["new_obs"], before["new_obs"])
    else:
        want = before["g_obs"].copy()
        want[1] = inp["new_obs"].reshape(-1)
        res["g_obs"] = exact(after["g_obs"], want)
    res["mb_rew_rest"] = _outside_row(after["mb_rew"], before["mb_rew"], row)
    if in_rows:
        t, b = rew_truth(inp["rew"], inp["value"], inp["time_outs"], inp["scale"], inp["gamma"])
        res["mb_rew"] = ratio(after["mb_rew"][row], t, b)
    if "terms" in before:
        res["terms_guards"] = _outside_row(after["terms"], before["terms"], 1)
        if in_rows:
            t, b = terms_truth(before["terms"][1], inp["stacked"], inp["nterms"], N)
            res["terms"] = ratio(after["terms"][1], t, b)
        else:
            res["terms"] = exact(after["terms"][1], before["terms"][1])
    return res


def check_gae(inp, before, after, truth=None) -> dict:
    H = inp["H"]
    t, e = truth if truth is not None else gae_truth(inp["fdones"], inp["last_values"], inp["mb_fdones"], inp["mb_values"], inp["mb_rewards"], inp["gamma"], inp["tau"])
    g = after["advs"].copy()
    g[1:1 + H] = before["advs"][1:1 + H]
    return {"advs_guards": exact(g, before["advs"]), "advs": ratio(after["advs"][1:1 + H], t, e)}


def check_policy(N, before, after, truth) -> dict:
    """truth: `policy_truth` of (at least) the N rows."""
    mu, v, bmu, bv = (x[:N] for x in truth)
    res = {}
    for k, t, b in (("mu", mu, bmu), ("value", v, bv)):
        g = after[k].copy()
        g[1:1 + N] = before[k][1:1 + N]
        res[k + "_guards"] = exact(g, before[k])
        res[k] = ratio(after[k][1:1 + N], t, b)
    return res


# ------------------------------------------------------------------------------------------------ fp32, as launched
def pre_blocks(N, nobs, largest=True):
    """dwp_rollout_pre's grid in workgroups of 256: a thread serves four observation words, one action word and one 16-byte piece of an fp16
    row; largest=False: the observation copy's count alone (the launcher before it was sized by the largest of the three)."""
    work = N * nobs // 4
    if largest:
        work = max(work, N * ACT, N * ((nobs + 7) // 8))
    return (work + 255) // 256


def post_blocks(N, nobs, same, largest=True):
    """dwp_rollout_post's grid: the envs alone in the g_obs == new_obs form, else the larger of the copy's 16-byte pieces and the envs
    (largest=False: the copy's alone)."""
    work = N if same else max(N * nobs // 4, N) if largest else N * nobs // 4
    return (work + 255) // 256


def launched_pre(inp, before, fault=None):
    N, H, nobs, n, layout = inp["N"], inp["H"], inp["nobs"], inp["n"], inp["layout"]
    o = {k: v.copy() for k, v in before.items()}
    T = 256 * pre_blocks(N, nobs, fault != "short_grid")
    mu, noise, obs = inp["mu"].reshape(-1), inp["noise"].reshape(-1), inp["obs"]
    sg = np.exp(inp["logstd"].astype(F32))
    a = (mu + sg[np.arange(N * ACT) % ACT] * noise).astype(F32)
    na, ne, nw = min(T, N * ACT), min(T, N), 4 * min(T, N * nobs // 4)
    if not 0 <= n < H:
        o["act"][1, :na] = np.clip(a[:na], F32(-1), F32(1))
        return o
    row_of = (lambda e: 1 + n * N + e) if fault == "swap_env_major" else (lambda e: 1 + e * H + n)          # (the fault: [H][N] rows in an [N][H] buffer)
    if layout == "half":
        ppr = (nobs + 7) // 8
        src = np.zeros((N, 8 * ppr), F32)
        src[:, :nobs] = obs
        i = np.arange(min(T, N * ppr))
        e, c = i // ppr, i % ppr
        cols = 8 * c[:, None] + np.arange(8)[None, :]
        rows = np.broadcast_to(row_of(e)[:, None], cols.shape)
        pieces = src.astype(np.float16).view(np.uint16).reshape(N * ppr, 8)[:len(i)]
        if fault == "half_tail":
            pieces = np.where(cols >= nobs, o["mb_obs"][rows, cols], pieces)
        o["mb_obs"][rows, cols] = pieces
    elif layout == "env":
        w = np.arange(nw)
        o["mb_obs"][row_of(w // nobs), w % nobs] = obs.reshape(-1)[:nw]
    else:
        o["mb_obs"][1 + n, :nw] = obs.reshape(-1)[:nw]
    o["mb_act"][1 + n, :na], o["mb_mu"][1 + n, :na] = a[:na], mu[:na]
    o["act"][1, :na] = np.clip(a[:na], F32(-1), F32(1))
    A, M = a.reshape(N, ACT), inp["mu"].reshape(N, ACT)
    sq, lsum = np.zeros(N, F32), F32(0)
    for k in range(ACT):
        z = ((A[:, k] - M[:, k]) / sg[k]).astype(F32)
        sq = (sq + z * z).astype(F32)
        lsum = F32(lsum + inp["logstd"][k])
    nlp = ((F32(0.5) * sq + F32(F32(0.5) * F32(1.8378770664093453) * F32(ACT))) + lsum).astype(F32)
    o["mb_nlp"][1 + n, :ne], o["mb_val"][1 + n, :ne], o["mb_done"][1 + n, :ne] = nlp[:ne], inp["value"].reshape(-1)[:ne], inp["dones"][:ne]
    return o


def launched_post(inp, before, fault=None):
    N, H, nobs, n, same = inp["N"], inp["H"], inp["nobs"], inp["n"], inp["same"]
    o = {k: v.copy() for k, v in before.items()}
    blocks = post_blocks(N, nobs, same, fault != "short_grid")
    T = 256 * blocks
    in_rows = 0 <= n < H
    if not same:
        nw = 4 * min(T, N * nobs // 4)
        o["g_obs"][1, :nw] = inp["new_obs"].reshape(-1)[:nw]
    ne = min(T, N)
    r = (inp["rew"] * F32(inp["scale"])).astype(F32)
    if inp["time_outs"] is not None and fault != "no_bootstrap":
        r = (r + (F32(inp["gamma"]) * inp["value"]).astype(F32) * inp["time_outs"].astype(F32)).astype(F32)
    if in_rows:
        o["mb_rew"][1 + n, :ne] = r[:ne]
    o["g_dones"][1, :ne] = inp["done"].astype(F32)[:ne]
    if "terms" in o and in_rows:
        nb = min(blocks, (N + 255) // 256)          # (workgroups that hold envs)
        x = np.zeros((nb * 256, inp["nterms"]), F32)
        m = min(N, nb * 256)
        x[:m] = inp["stacked"][:m, :inp["nterms"]]
        x = x.reshape(nb, 4, 64, -1)
        for w in (32, 16, 8, 4, 2, 1):          # the butterfly, as lane 0 sees it
            x = (x[:, :, :w] + x[:, :, w:2 * w]).astype(F32)
        x = x[:, :, 0]
        part = (((x[:, 0] + x[:, 1]).astype(F32) + x[:, 2]).astype(F32) + x[:, 3]).astype(F32) / F32(256 if fault == "terms_div_256" else N)
        for b in range(nb):
            o["terms"][1] = (o["terms"][1] + part[b].astype(F32)).astype(F32)
    return o


def launched_gae(inp, before, fault=None):
    N, H = inp["N"], inp["H"]
    o = {k: v.copy() for k, v in before.items()}
    g, gt = (F32(x) for x in gae_scalars(inp["gamma"], inp["tau"]))
    last = N + 1 if fault == "row_past_n" else N          # (the fault: one thread past the envs stores too -- it re-reads env N - 1)
    src = np.minimum(np.arange(last), N - 1)
    lam, nn, nv = np.zeros(last, F32), (F32(1) - inp["fdones"][src]).astype(F32), inp["last_values"].reshape(-1)[src]
    flat = o["advs"].reshape(-1)
    for t in range(H - 1, -1, -1):
        val = inp["mb_values"][t][src]
        delta = ((inp["mb_rewards"][t][src] + ((g * nv).astype(F32) * nn).astype(F32)).astype(F32) - val).astype(F32)
        lam = (delta + ((gt * nn).astype(F32) * lam).astype(F32)).astype(F32)
        flat[(1 + t) * N:(1 + t) * N + last] = lam
        nn = (F32(1) - inp["mb_fdones"][t - 1 if fault == "gae_wrong_step" and t > 0 else t][src]).astype(F32)
        nv = val
    return o


def launched_policy(W, obs, before, fault=None):
    """k_policy's tiles of MT rows: a tile past the end re-reads the last row (`rmax`) and stores only rows below N."""
    N = obs.shape[0]
    o = {k: v.copy() for k, v in before.items()}
    tiles = (N + MT - 1) // MT
    src = np.minimum(np.arange(tiles * MT), N - 1)
    mu, v = _forward(W, obs[src].astype(F32), F32)
    keep = tiles * MT if fault == "row_past_n" else N
    if fault == "policy_rows_swapped" and N >= 2:
        mu[[0, 1]], v[[0, 1]] = mu[[1, 0]], v[[1, 0]]
    o["mu"][1:1 + keep], o["value"][1:1 + keep] = mu[:keep], v[:keep]
    return o
