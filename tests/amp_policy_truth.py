"""The analytic backward of the AMP actor-critic's loss (include/dyros_amp_policy.h, dwa_grad), restated with plain tensor products and no
autograd: the float64 truth of the GPU tests and the statement the CPU test holds against torch autograd.

Inputs are the normalised observations xn [B, D], the parameters as a list in the layout order (amp_policy.ActorCritic.params_in_layout),
the fixed log-sigma [A] and the rows' act / old_nlp / adv / ret_n.  Returns (loss, the four logged values, the gradients in layout order,
per gradient the sum of the absolute terms of its last product, |dZ|^T |[h | 1]| (the scale of its rounding error), and per gradient
max_rows |dZ| max_rows |[h | 1]| (a bound of one row's term: what a relu mask decided the other way at one row can change))."""
from __future__ import annotations

import math

import torch


def forward(xn, P):
    a1w, a1b, a2w, a2b, mw, mb, c1w, c1b, c2w, c2b, vw, vb = P
    ha1 = torch.relu(xn @ a1w.T + a1b)
    ha2 = torch.relu(ha1 @ a2w.T + a2b)
    hc1 = torch.relu(xn @ c1w.T + c1b)
    hc2 = torch.relu(hc1 @ c2w.T + c2b)
    return ha1, ha2, hc1, hc2, ha2 @ mw.T + mb, (hc2 @ vw.T + vb).reshape(-1)


def loss_and_grad(xn, P, logstd, act, old_nlp, adv, ret_n, e_clip=0.2, critic_coef=5.0, bounds_coef=10.0):
    a1w, a1b, a2w, a2b, mw, mb, c1w, c1b, c2w, c2b, vw, vb = P
    B, A = act.shape
    ha1, ha2, hc1, hc2, mu, v = forward(xn, P)
    sd = torch.exp(logstd)
    z = (act - mu) / sd
    nlp = 0.5 * (z ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * A + logstd.sum()
    ratio = torch.exp(old_nlp - nlp)
    lo, hi = 1.0 - e_clip, 1.0 + e_clip
    x1, x2 = -adv * ratio, -adv * torch.clamp(ratio, lo, hi)
    a_rows = torch.maximum(x1, x2)
    hi1, lo1 = torch.clamp(mu - 1.0, min=0), torch.clamp(mu + 1.0, max=0)
    a_loss, c_loss, b_loss = a_rows.mean(), ((ret_n - v) ** 2).mean(), (hi1 ** 2 + lo1 ** 2).sum(-1).mean()
    clip = (torch.abs(ratio - 1.0) > e_clip).to(xn.dtype).mean()
    loss = a_loss + critic_coef * c_loss + bounds_coef * b_loss
    # the surrogate: torch.max splits the gradient of equal arguments in halves, clamp passes it inside [lo, hi]
    g1 = torch.where(x1 > x2, 1.0, torch.where(x1 == x2, 0.5, 0.0)).to(xn.dtype)
    inside = ((ratio >= lo) & (ratio <= hi)).to(xn.dtype)
    dratio = (g1 * -adv + (1.0 - g1) * inside * -adv) / B
    dnlp = -ratio * dratio
    dmu = dnlp[:, None] * (-z / sd) + bounds_coef / B * 2.0 * (hi1 + lo1)
    dv = critic_coef / B * 2.0 * (v - ret_n)
    one = torch.ones(B, 1, dtype=xn.dtype, device=xn.device)
    peaks = []

    def wg(dz, h):
        hb = torch.cat([h, one], 1)
        g, s = dz.T @ hb, dz.abs().T @ hb.abs()
        pk = dz.abs().amax(0)[:, None] * hb.abs().amax(0)[None, :]
        peaks.extend([pk[:, :-1], pk[:, -1]])
        return g[:, :-1], g[:, -1], s[:, :-1], s[:, -1]

    gm_w, gm_b, sm_w, sm_b = wg(dmu, ha2)
    gv_w, gv_b, sv_w, sv_b = wg(dv[:, None], hc2)
    dza2 = (ha2 > 0).to(xn.dtype) * (dmu @ mw)
    dzc2 = (hc2 > 0).to(xn.dtype) * (dv[:, None] @ vw)
    ga2w, ga2b, sa2w, sa2b = wg(dza2, ha1)
    gc2w, gc2b, sc2w, sc2b = wg(dzc2, hc1)
    dza1 = (ha1 > 0).to(xn.dtype) * (dza2 @ a2w)
    dzc1 = (hc1 > 0).to(xn.dtype) * (dzc2 @ c2w)
    ga1w, ga1b, sa1w, sa1b = wg(dza1, xn)
    gc1w, gc1b, sc1w, sc1b = wg(dzc1, xn)
    grads = [ga1w, ga1b, ga2w, ga2b, gm_w, gm_b, gc1w, gc1b, gc2w, gc2b, gv_w.reshape(1, -1), gv_b]
    scales = [sa1w, sa1b, sa2w, sa2b, sm_w, sm_b, sc1w, sc1b, sc2w, sc2b, sv_w.reshape(1, -1), sv_b]
    order = [8, 9, 4, 5, 0, 1, 10, 11, 6, 7, 2, 3]          # (wg's calls: mu, v, a2, c2, a1, c1 -> the layout order)
    peaks = [peaks[i] for i in order]
    peaks[10] = peaks[10].reshape(1, -1)
    return loss, (a_loss, c_loss, b_loss, clip), grads, scales, peaks
