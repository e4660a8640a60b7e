"""The fused PPO minibatch update (include/dyros_ppo.h, csrc/dw_ppo.hip) restated in float64 on the CPU, one function per stage: the truth a
GPU test of the update at small and odd minibatch sizes compares the kernels with, stage by stage.  tests/test_ppo_update_truth.py holds it
against torch autograd, clip_grad_norm_ and torch.optim.Adam.

Every function takes the operands THE KERNEL HAD -- the fp16 / fp32 words read back from the fused buffers, exact in float64 -- and returns
the exact result with an error bound that follows from the arithmetic, not from what the kernels were seen to give:

  u16 = 2^-11 (half an fp16 ulp, relative), u32 = 2^-24 (the same for fp32), SUB16 = 2^-24 (the spacing of the fp16 subnormals).
  A sum of K products accumulated in fp32 in any order is within K u32 S of the exact sum t, S = sum of the |terms| (first order in u32).
  Stored as fp16 that is  u16 |t| + (K + 1) u32 S, never below SUB16.  Where the library-GEMM form rounds the bare product to fp16 before the
  bias is added and the sum rounded again (dwp_bias_relu, dwp_loss), u16 |product| comes on top.
  A weight gradient left in fp32 per slab of n samples: (n + 1) u32 S of that slab; the sum over the 4 slabs: (B + 4) u32 S.
  A bias gradient, fp32 atomic adds into 32 buckets that are then summed: (B + 32) u32 sum |.|.
  The loss kernel's output gradient: the fp32 evaluation's relative error (`loss`, derived there) next to the fp16 rounding.

Tensors may live on any device; everything is computed in float64 on the CPU."""
from __future__ import annotations

import importlib.util
import math
import os

import torch

from isaacgymdyros_amd import cbind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = cbind.constants("dyros_ppo.h", "dwp_")
IN, INP, HID, OUTP, ACT = K["DWP_IN"], K["DWP_INP"], K["DWP_HID"], K["DWP_OUTP"], K["DWP_ACT"]
NW1, NW2, NW3 = 2 * HID * INP, 2 * HID * HID, 2 * OUTP * HID
NWT = NW1 + NW2 + NW3
NB1, NB2, NB3 = 2 * HID, 2 * HID, 2 * OUTP
NP = NWT + NB1 + NB2 + NB3
WG_SLABS, WG_RD, PBUF_BUCKETS = K["DWP_WGRAD_SLABS"], 5, K["DWP_PBUF_BUCKETS"]          # WG_RD: wgrad_block's `constexpr int RD` (csrc/dw_ppo.hip; tests/test_ppo_update_truth.py reads it there)
U16, U32, SUB16 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -24
LOG_FLT_MAX = math.log(3.4028234663852886e38)
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
CLIP_MARGIN = 1e-5          # a sample whose float64 |ratio - 1| is this close to e_clip may fall on either side in fp32


def f64(t):
    return t.detach().to("cpu", torch.float64)


def consumer():
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ------------------------------------------------------------------------------------------------ dwp_wgrad's slabs of samples
def wgrad_slabs(nkb: int, slabs: int = WG_SLABS):
    """k_wgrad's [kb0, kb1) per slab for nkb = B / 32 k-blocks of 32 samples: per = ceil(nkb / slabs), both bounds clamped to nkb."""
    per = (nkb + slabs - 1) // slabs
    out = []
    for s in range(slabs):
        kb0 = s * per if s * per < nkb else nkb
        kb1 = kb0 + per if kb0 + per < nkb else nkb
        out.append((kb0, kb1))
    return out


def slab_nk(B: int):
    return [b - a for a, b in wgrad_slabs(B // 32)]


def slab_rows(B: int, table=None):
    """The sample rows of each slab as slices (a k-block is 32 consecutive samples: one workgroup of dwp_mlp)."""
    return [slice(32 * a, 32 * b) for a, b in (table if table is not None else wgrad_slabs(B // 32))]


def edge_sizes():
    """The minibatch sizes at which dwp_wgrad's ring of WG_RD requests and dwp_mlp's 32 buckets take another path, found by scanning
    nkb = 1 .. 64 with `wgrad_slabs` (smallest nkb of each kind): {B: (nk per slab, what it is)}."""
    first = {}

    def put(key, nkb, note):
        if key not in first:
            first[key] = (32 * nkb, note)
    for nkb in range(1, 65):
        nk = [b - a for a, b in wgrad_slabs(nkb)]
        per = max(nk)
        if nkb == 1:
            put("one", nkb, "a single workgroup, three empty slabs")
        if nk.count(0) == 1 and per == 1:
            put("empty", nkb, "one empty slab")
        if nk.count(0) == 1 and per == 2 and 0 < nk[2] < per:
            put("clamped", nkb, "an uneven slab before an empty one whose kb0 is clamped")
        for k, note in ((WG_RD - 1, "RD - 1: the priming loads are all there are"), (WG_RD + 1, "RD + 1: one refill, one wrap of the ring"),
                        (2 * WG_RD + 1, "2 RD + 1: the unrolled group runs a third time")):
            if per == k:
                put("per%d" % k, nkb, note)
        if nk == [WG_RD] * WG_SLABS:
            put("ring", nkb, "RD in every slab: exactly one unrolled group")
        if nkb == PBUF_BUCKETS + 1:
            put("wrap", nkb, "33 workgroups: the bucket index wraps for the first time")
    return {B: (slab_nk(B), note) for B, note in sorted(first.values())}


# ------------------------------------------------------------------------------------------------ the case recipe (tests/test_ppo_gpu.py's, on the CPU)
NMB = 3                           # minibatches of an edge case (four updates: the index visits 1 and 2 and wraps to 0)
GEMM_SIZES = (1, 63, 65, 100)     # the library-GEMM form's edge sizes: below, at either side of and between its kernels' 64-row blocks


def case_seed(form: str, B: int) -> int:
    return (1000 if form == "mfma" else 2000) + B


def make_case(ppo, rows: int, seed: int):
    """(net, (obs, act, nlp_old, mu_old, adv, ret)) on the CPU: `_lively` and `_batch` of tests/test_ppo_gpu.py themselves, with a CPU
    generator, so that the same numbers can be looked at without a GPU."""
    import sys
    from test_ppo_gpu import _batch, _lively
    torch.manual_seed(seed)
    net = ppo.DyrosActorCritic(IN, ACT, ppo.TRAIN_CFG["network"])
    _lively(net)
    return net, _batch(ppo, net, sys.modules[__name__], rows, "cpu", seed=seed)


def emulated_out(net, obs):
    """The heads' fp16 outputs [2, rows, OUTP] as the update's forward forms them -- fp16 operands, exact sums, one rounding per layer --
    from a CPU module: what the clip margins of a case can be looked at with before it runs on a GPU."""
    h = lambda t: f64(t.detach().half())          # noqa: E731
    out = torch.zeros(2, obs.shape[0], OUTP, dtype=torch.float64)
    for k, (trunk, head) in enumerate(((net.actor_mlp, net.mu), (net.critic_mlp, net.value))):
        x = h(obs)
        for lin in (trunk[0], trunk[2]):
            x = torch.relu(x @ h(lin.weight).T + h(lin.bias)).half().double()
        y = (x @ h(head.weight).T + h(head.bias)).half().double()
        out[k, :, :y.shape[1]] = y
    return out


# ------------------------------------------------------------------------------------------------ forward and input gradients
def linear(a, w, bias=None, double_rounded=False):
    """t = a . w' (+ bias) for fp16 operands a [.., B, K], w [.., N, K], bias [.., N]; returns (t, bound of an fp16 result of an fp32-accumulated
    sum).  double_rounded: the library-GEMM form's hidden layers and heads (product -> fp16, + bias, -> fp16)."""
    a, w = f64(a), f64(w)
    prod = a @ w.transpose(-1, -2)
    S = a.abs() @ w.abs().transpose(-1, -2)
    t = prod
    if bias is not None:
        b = f64(bias).unsqueeze(-2)
        t, S = prod + b, S + b.abs()
    bound = U16 * t.abs() + (a.shape[-1] + 1) * U32 * S
    if double_rounded:
        bound = bound + U16 * prod.abs()
    return t, torch.clamp(bound, min=SUB16)


def masked(t, h):
    """relu's backward: the kernel's mask is its own stored activation, h > 0."""
    return t * (f64(h) > 0).double()


# ------------------------------------------------------------------------------------------------ the loss on the heads' stored outputs
def loss(out, act, old_nlp, old_mu, adv, ret, logstd, scale, e_clip, critic_coef):
    """From out [2, B, OUTP] as stored (row i of [0]: the 13 action means, word 0 of row i of [1]: the value) and the minibatch's rows: the
    formulas of examples/ppo_consumer.py (neglogp, actor_loss, critic_loss, bound_loss, policy_kl) and the gradient of
    scale * (mean(surrogate) + 0.5 critic_coef mean((ret - v)^2)) at the outputs, torch.max's tie rule included (half the gradient to each
    branch; clamp passes it on its closed range).  The ratio overflows where fp32's would: exp of more than log(FLT_MAX) is inf.

    Bounds of the fp16 output gradients.  dvalue: five fp32 roundings (v - ret, the three factors, 1 / B) next to the fp16 one: (u16 + 8 u32) |t|.
    dmu: z = (a - mu) / sigma carries 4 u32 (one subtraction, expf to 2 ulp, one division), its square 9, the sum of 13 over four exchanges 13;
    log sigma's sum 4 u32; neglogp = 0.5 sq + c + lsum then has an ABSOLUTE error below 16 u32 M, M = 0.5 sq + c + sum |log sigma|; the
    difference old - new adds u32 (|old| + M); expf turns that absolute error into a relative one of the ratio and adds 2 u32 (1 + |old - new|) of
    its own; the remaining factors (A, scale / B, (a - mu) / sigma^2) 14 u32.  Together below 20 u32 (1 + M + |old|) =: rel, and the bound
    is (u16 + rel) |t|.  Neither is ever below SUB16."""
    out = f64(out)
    mu, v = out[0, :, :ACT], out[1, :, 0]
    B = mu.shape[0]
    act, old_nlp, old_mu, adv, ret, ls = (f64(t) for t in (act, old_nlp, old_mu, adv, ret, logstd))
    ret = ret.reshape(-1)
    sg = torch.exp(ls)
    z = (act - mu) / sg
    sq = (z ** 2).sum(-1)
    c = 0.5 * math.log(2.0 * math.pi) * ACT
    nlp = 0.5 * sq + c + ls.sum()
    d = old_nlp - nlp
    ratio = torch.where(d > LOG_FLT_MAX, torch.full_like(d, math.inf), torch.exp(d))
    lo, hi = 1.0 - e_clip, 1.0 + e_clip
    x1, x2 = -adv * ratio, -adv * torch.clamp(ratio, lo, hi)
    a_rows = torch.maximum(x1, x2)
    half = lambda p, q: torch.where(p > q, 1.0, torch.where(p == q, 0.5, 0.0)).double()          # noqa: E731
    inside = ((ratio >= lo) & (ratio <= hi)).double()
    w = half(x1, x2) + inside * half(x2, x1)
    dnlp = adv * ratio * w
    dmu = (scale / B) * dnlp[:, None] * (-(act - mu) / sg ** 2)
    dv = (scale / B) * critic_coef * (v - ret)
    M = 0.5 * sq + c + ls.abs().sum()
    rel = 20.0 * U32 * (1.0 + M + old_nlp.abs())
    b_rows = (torch.clamp(mu - 1.1, max=0.0) ** 2 + torch.clamp(-mu + 1.1, max=0.0) ** 2).sum(-1)
    kl_rows = (torch.log(sg / sg + 1e-5) + (sg ** 2 + (old_mu - mu) ** 2) / (2.0 * (sg ** 2 + 1e-5)) - 0.5).sum(-1)
    return {"nlp": nlp, "ratio": ratio, "a_rows": a_rows, "a_loss": a_rows.mean(), "c_loss": ((ret - v) ** 2).mean(), "b_loss": b_rows.mean(),
            "kl": kl_rows.mean(), "clip_frac": ((ratio - 1.0).abs() > e_clip).double().mean(), "margin": (ratio - 1.0).abs() - e_clip,
            "dmu": dmu, "dvalue": dv,
            "dmu_bound": torch.clamp((U16 + rel)[:, None] * dmu.abs(), min=SUB16), "dvalue_bound": torch.clamp((U16 + 8.0 * U32) * dv.abs(), min=SUB16)}


def dout_of(L):
    """The loss's two output gradients as the padded [2, B, OUTP] the kernels store."""
    B = L["dmu"].shape[0]
    d = torch.zeros(2, B, OUTP, dtype=torch.float64)
    d[0, :, :ACT], d[1, :, 0] = L["dmu"], L["dvalue"]
    return d


# ------------------------------------------------------------------------------------------------ weight and bias gradients
def wgrad(dz, act, rows=None):
    """(dz' . act, |dz|' . |act|) over the samples (or the slice `rows` of them): dz [.., B, O], act [.., B, I] as stored."""
    dz, act = f64(dz), f64(act)
    if rows is not None:
        dz, act = dz[..., rows, :], act[..., rows, :]
    return dz.transpose(-1, -2) @ act, dz.abs().transpose(-1, -2) @ act.abs()


def wgrad_slab_bound(S, n):
    return (n + 1) * U32 * S


def wgrad_sum_bound(S, B):
    return (B + WG_SLABS) * U32 * S


def wgrad_fp16_bound(g, S, B):
    """The library-GEMM form's weight gradient: the sum over B samples accumulated in fp32 and stored as fp16."""
    return torch.clamp(U16 * g.abs() + (B + 1) * U32 * S, min=SUB16)


def worst_slab_fraction(g_slabs, dz, act, table=None):
    """max over the slabs and entries of |g_slabs[s] - (dz' . act restricted to slab s's rows)| / bound, for per-slab partial gradients
    g_slabs [slabs, .., O, I]; an empty slab's copy must be exactly zero (inf otherwise).  table: the slab bounds (default: `wgrad_slabs`)."""
    B = dz.shape[-2]
    worst = 0.0
    for s, rows in enumerate(slab_rows(B, table)):
        got = f64(g_slabs[s])
        n = rows.stop - rows.start
        if n <= 0:
            worst = max(worst, 0.0 if float(got.abs().max()) == 0.0 else math.inf)
            continue
        g, S = wgrad(dz, act, rows)
        worst = max(worst, float(((got - g).abs() / torch.clamp(wgrad_slab_bound(S, n), min=1e-300)).max()))
    return worst


def bgrad(dz):
    """(column sums of the stored fp16 gradient, their bound as fp32 atomics into 32 buckets)."""
    dz = f64(dz)
    return dz.sum(-2), (dz.shape[-2] + PBUF_BUCKETS) * U32 * dz.abs().sum(-2)


def flat(gW1, gW2, gW3, gb1, gb2, gb3):
    """The parameter layout: W1 [2][HID][INP] | W2 [2][HID][HID] | W3 [2][OUTP][HID] | b1 [2][HID] | b2 [2][HID] | b3 [2][OUTP]."""
    return torch.cat([f64(t).reshape(-1) for t in (gW1, gW2, gW3, gb1, gb2, gb3)])


def tensor_spans():
    """[(name, first word, words)] of the six tensors of `flat`; the actor's half of each comes first."""
    out, o = [], 0
    for name, n in (("W1", NW1), ("W2", NW2), ("W3", NW3), ("b1", NB1), ("b2", NB2), ("b3", NB3)):
        out.append((name, o, n))
        o += n
    return out


# ------------------------------------------------------------------------------------------------ the sharded form: one bucket per rank, their sum
def rank_bucket(pairs, B, world):
    """One rank's bucket [weights | biases] as dwp_grad_bucket leaves it: (t, bound) in the layout of `flat`.  pairs: ((dz1, x), (dz2, h1),
    (dout, h2)) as that rank stored them (x expanded to [2, B, INP]), B its minibatch.  t = the rank's still-scaled gradient / world.  The
    fp32 sum of the slabs (or of the 32 buckets of a bias) carries its own bound, which the multiply by 1 / world scales with the word; the
    multiply then rounds once: u32 |t| (nothing at all for a power of two).  fl(1 / 3) itself is a third of an ulp off, 2^-25.6 relative:
    that is taken from the first term, of which a sum in fp32 uses a small part (its K u32 S counts every addition at full size)."""
    ts, bs = [], []
    for dz, a in pairs:
        g, S = wgrad(dz, a)
        ts.append(g / world); bs.append(wgrad_sum_bound(S, B) / world)
    for dz, _ in pairs:
        g, b = bgrad(dz)
        ts.append(g / world); bs.append(b / world)
    t, bound = flat(*ts), flat(*bs)
    return t, bound + U32 * t.abs()


def bucket_sum(buckets):
    """The all-reduce as the one-GPU tests emulate it: ((b_0 + b_1) + b_2) + ... in ascending rank order -- exact here; R - 1 fp32 additions of
    partial sums no larger than sum |b_r| add at most (R - 1) u32 sum |b_r| on the GPU.  Returns (sum, that bound)."""
    bs = [f64(b) for b in buckets]
    total, mag = bs[0].clone(), bs[0].abs()
    for b in bs[1:]:
        total, mag = total + b, mag + b.abs()
    return total, (len(bs) - 1) * U32 * mag


def actor_mask():
    m = torch.zeros(NP, dtype=torch.bool)
    o = 0
    for n in (NW1, NW2, NW3, NB1, NB2, NB3):
        m[o:o + n // 2] = True
        o += n
    return m


# ------------------------------------------------------------------------------------------------ unscale, clip, Adam, GradScaler
def found_inf(g_scaled, mask=None):
    """unscale_'s found_inf per net, [actor, critic]: a non-finite entry among that net's (still scaled) gradients."""
    mask = actor_mask() if mask is None else mask
    bad = ~torch.isfinite(f64(g_scaled))
    return [bool(bad[mask].any()), bool(bad[~mask].any())]


def clip_adam(g_scaled, scale, p0, m0, v0, steps, lrs, max_norm, mask=None):
    """GradScaler.unscale_ of both optimisers, clip_grad_norm_(actor, max_norm), then Adam (betas (0.9, 0.999), eps 1e-8, no weight decay) per net
    with its own step count and learning rate -- skipped for a net whose gradient is not finite.  steps: the counts BEFORE this update.
    Returns dict(found, norm, coef, p, m, v, steps)."""
    mask = actor_mask() if mask is None else mask
    g, p0, m0, v0 = f64(g_scaled) / scale, f64(p0), f64(m0), f64(v0)
    found = found_inf(g, mask)
    norm = float(torch.sqrt((g[mask] ** 2).sum()))
    coef = min(1.0, max_norm / (norm + 1e-6))
    g = torch.where(mask, g * coef, g)
    p, m, v, steps = p0.clone(), m0.clone(), v0.clone(), list(steps)
    for net, sel in ((0, mask), (1, ~mask)):
        if found[net]:
            continue
        steps[net] += 1
        t = steps[net]
        m1 = BETA1 * m0[sel] + (1.0 - BETA1) * g[sel]
        v1 = BETA2 * v0[sel] + (1.0 - BETA2) * g[sel] ** 2
        m[sel], v[sel] = m1, v1
        p[sel] = p0[sel] - (lrs[net] / (1.0 - BETA1 ** t)) * (m1 / (v1.sqrt() / math.sqrt(1.0 - BETA2 ** t) + ADAM_EPS))
    return {"found": found, "norm": norm, "coef": coef, "p": p, "m": m, "v": v, "steps": steps}


def scaler_update(scale, growth, found_any, growth_interval=2000):
    """torch.amp.GradScaler.update: backoff 0.5 on any inf, growth 2.0 after growth_interval clean updates in a row.  Returns (scale, growth tracker)."""
    if found_any:
        return scale * 0.5, 0
    growth += 1
    return (scale * 2.0, 0) if growth == growth_interval else (scale, growth)
