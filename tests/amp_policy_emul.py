"""dwa_act, dwa_critic and dwa_grad (csrc/dw_amp_policy.hip) restated in float32 torch on the CPU: something the stage checks of
tests/amp_policy_stages.py can run on without a GPU.  It is NOT the kernels -- torch's products add in another order -- but it fills a workspace
image in the mirrored layout, g and state the way the kernels do: K = B products split into slabs of kc rows (kc rounded up to a k slice) that
are added in slab order, the ones columns, dv in column 16 of a dd row, NaN left wherever nothing is written.

`fault=` injects ONE defect, so that tests/test_amp_policy_edges.py can show that the stage checks reject it:
  slab_last_row      the last row of every slab is left out of the K = B products
  tile_last_row      the forward leaves the accumulators of the last 16-row tile's last row at zero (a `live` count one tile short)
  bias_column        the last column of the weight-gradient products (N = D + 1 or 513: the bias gradient) is left out
  g_assign           g = instead of g +=
  critic_mask        the critic's dZ2 is masked with the actor's h2
  dv_column          dv is written to column A of a dd row instead of column 16
  k_tail             the partial last k slice of layer 1 (D % 32 != 0) is read as zeros
  heads_second_trip  dwa_heads_bwd's grid-stride loop stops after its first trip (rows >= 8192 are left out)"""
from __future__ import annotations

import torch

import amp_policy_stages as S

FAULTS = ("slab_last_row", "tile_last_row", "bias_column", "g_assign", "critic_mask", "dv_column", "k_tail", "heads_second_trip")
NAN = float("nan")


def workspace(R, D, A, grad):
    return torch.full((S.workspace_bytes(R, D, A, grad) // 4,), NAN)


def _forward(c, W, grad, nets, fault):
    R, D, P = c["B"], c["D"], c["P"]
    v = S.views(W, R, D, grad)
    mu, var = c["obs_stats"][:D].float(), c["obs_stats"][D:2 * D].float()
    xn = v["xn"]
    xn[:, :D] = torch.clamp((c["obs"] - mu) / torch.sqrt(var + torch.tensor(1e-5)), -S.NORM_CLIP, S.NORM_CLIP)
    xn[:, D] = 1.0
    xn[:, D + 1:] = 0.0
    if grad:
        v["h1"][:, :, S.HID] = 1.0
        v["h2"][:, :, S.HID] = 1.0
    for n in nets:
        W1, b1, W2, b2 = (P[i] for i in S.NET[n][:4])
        x = xn[:, :D].clone()
        if fault == "k_tail" and D % S.TK:
            x[:, D // S.TK * S.TK:] = 0.0
        pre1 = x @ W1.T
        if fault == "tile_last_row":
            pre1[R - 1] = 0.0
        h1 = torch.relu(pre1 + b1)
        pre2 = h1 @ W2.T
        if fault == "tile_last_row":
            pre2[R - 1] = 0.0
        v["h1"][n][:, :S.HID] = h1
        v["h2"][n][:, :S.HID] = torch.relu(pre2 + b2)
    return v


def _unnorm(v, val_stats):
    return v * torch.sqrt(val_stats[1].float() + torch.tensor(1e-5)) + val_stats[0].float()


def act(c, fault=None):
    """(workspace image, (action, clamped, mu, neglogp, value [N, 1]))."""
    N, D, A, P = c["B"], c["D"], c["A"], c["P"]
    W = workspace(N, D, A, 0)
    v = _forward(c, W, 0, (0, 1), fault)
    mu = v["h2"][0][:, :S.HID] @ P[4].T + P[5]
    val = v["h2"][1][:, :S.HID] @ P[10].T + P[11]
    sd = torch.exp(c["logstd"])
    action = mu + sd * c["noise"]
    nlp = 0.5 * (((action - mu) / sd) ** 2).sum(-1) + torch.tensor(S.HALF_LOG_2PI * A) + c["logstd"].sum()
    return W, (action, torch.clamp(action, -1.0, 1.0), mu, nlp, _unnorm(val, c["val_stats"]))


def critic(c, fault=None):
    N, D, A, P = c["B"], c["D"], c["A"], c["P"]
    W = workspace(N, D, A, 0)
    v = _forward(c, W, 0, (1,), fault)
    val = v["h2"][1][:, :S.HID] @ P[10].T + P[11]
    return W, _unnorm(val, c["val_stats"]) * (1.0 - c["term"]).view(N, 1)


def _wgrad(X, M, Y, B, gw, gb, slab, fault):
    """wgrad(): X [2][B, >= M[n]], Y [2][B, N] (the last column the ones); the slabs of both nets into `slab`, their in-order sums into gw / gb."""
    rows = S.slab_rows(B)
    nz, N = len(rows), Y[0].shape[1]
    zs = max(M) * N
    for n in (0, 1):
        s = torch.zeros(M[n], N)
        for z, (r0, r1) in enumerate(rows):
            if fault == "slab_last_row":
                r1 -= 1
            part = X[n][r0:r1, :M[n]].T @ Y[n][r0:r1]
            if fault == "bias_column":
                part[:, -1] = 0.0
            o = (n * nz + z) * zs
            slab[o:o + M[n] * N] = part.reshape(-1)
            s = s + part
        if fault == "g_assign":
            gw[n].copy_(s[:, :-1].reshape(gw[n].shape))
            gb[n].copy_(s[:, -1].reshape(gb[n].shape))
        else:
            gw[n] += s[:, :-1].reshape(gw[n].shape)
            gb[n] += s[:, -1].reshape(gb[n].shape)


def grad(c, g0, state0, W=None, fault=None, coef=S.COEF):
    """(workspace image, g, state) after one dwa_grad from g0 / state0 (W: a workspace to reuse, as it is)."""
    B, D, A, P = c["B"], c["D"], c["A"], c["P"]
    W = workspace(B, D, A, 1) if W is None else W
    g, state = g0.clone(), state0.clone()
    G = S.split(g, D, A)
    v = _forward(c, W, 1, (0, 1), fault)
    h2a, h2c = v["h2"][0][:, :S.HID], v["h2"][1][:, :S.HID]
    # ---- dwa_heads_bwd
    e, cc, bc = (torch.tensor(x) for x in coef)
    lo, hi = torch.tensor(S.LO32), torch.tensor(S.HI32)
    invB = torch.tensor(1.0) / B
    mu, val = h2a @ P[4].T + P[5], (h2c @ P[10].T + P[11]).reshape(-1)
    sd = torch.exp(c["logstd"])
    z = (c["act"] - mu) / sd
    nlp = 0.5 * (z * z).sum(-1) + torch.tensor(S.HALF_LOG_2PI * A) + c["logstd"].sum()
    ratio, adv, ret = torch.exp(c["old"] - nlp), c["adv"], c["ret"]
    x1, x2 = -adv * ratio, -adv * torch.clamp(ratio, lo, hi)
    g1 = torch.where(x1 > x2, 1.0, torch.where(x1 == x2, 0.5, 0.0))
    inside = ((ratio >= lo) & (ratio <= hi)).float()
    dratio = (g1 * -adv + (1.0 - g1) * inside * -adv) * invB
    dnlp = -ratio * dratio
    dv = cc * invB * 2.0 * (val - ret)
    hi1, lo1 = torch.clamp(mu - 1.0, min=0.0), torch.clamp(mu + 1.0, max=0.0)
    dmu = dnlp[:, None] * (-z / sd) + bc * invB * 2.0 * (hi1 + lo1)
    rows4 = torch.stack([torch.maximum(x1, x2), (ret - val) ** 2, (hi1 * hi1 + lo1 * lo1).sum(-1), ((ratio - 1.0).abs() > e).float()], 1)
    live = B if fault != "heads_second_trip" else min(B, S.HEAD_BLOCKS * S.RW)
    dd, z2 = v["dd"], v["z2"]
    dd[:live, :A] = dmu[:live]
    dd[:live, A if fault == "dv_column" else S.DV_COL] = dv[:live]
    z2[0][:live, :S.HID] = ((h2a > 0).float() * (dmu @ P[4]))[:live]
    z2[1][:live, :S.HID] = (((h2a if fault == "critic_mask" else h2c) > 0).float() * (dv[:, None] * P[10].reshape(1, -1)))[:live]
    nb = S.heads_blocks(B)
    part = torch.zeros(nb, 4)
    part.index_add_(0, (torch.arange(live) // S.RW) % nb, rows4[:live])
    v["part"][:nb] = part
    state[:4] += part.sum(0) / B
    state[4] += 1.0
    # ---- the weight gradients
    slab = v["slab"]
    _wgrad([dd, dd[:, S.DV_COL:]], [A, 1], [v["h2"][0][:, :S.HID + 1], v["h2"][1][:, :S.HID + 1]], B, [G[4], G[10]], [G[5], G[11]], slab, fault)
    h1 = [v["h1"][n][:, :S.HID + 1] for n in (0, 1)]
    _wgrad([z2[0], z2[1]], [S.HID, S.HID], h1, B, [G[2], G[8]], [G[3], G[9]], slab, fault)
    for n in (0, 1):
        hn = v["h1"][n][:, :S.HID]
        hn.copy_((hn > 0).float() * (z2[n][:, :S.HID] @ P[S.NET[n][2]]))
    dz1 = [v["h1"][n] for n in (0, 1)]
    x1c = v["xn"][:, :D + 1]
    _wgrad(dz1, [S.HID, S.HID], [x1c, x1c], B, [G[0], G[6]], [G[1], G[7]], slab, fault)
    return W, g, state
