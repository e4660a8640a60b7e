"""dwa_act, dwa_critic and dwa_grad (include/dyros_amp_policy.h, csrc/dw_amp_policy.hip) stage by stage in float64: the truth a test of the
kernels at tile and slab edges compares them with.  Every function takes the operands THE CODE UNDER TEST HAD -- the fp32 words read back from
its workspace, exact in float64 -- and returns the exact result with an elementwise error bound that follows from the arithmetic, never from
what the kernels were seen to give.  Because every stage starts from the stored output of the one before it, no relu decision is ambiguous
(the mask is the stored activation's) and tests/test_amp_policy_gpu.py's allowance for flipped masks is not needed.
tests/test_amp_policy_edges.py holds the composition of these stages to amp_policy_truth.loss_and_grad and to torch autograd.

Rounding unit: U = 2^-24 per fp32 operation.  v_mfma_f32_16x16x4_f32 is documented as bit for bit a k-ordered chain of fp32 fmaf, one rounding
per product and no wider accumulation, which is round to nearest; the vector unit's +, *, fma are IEEE round to nearest as well.  All bounds
are first order in U, with the constants rounded up to cover the second order.
  * a chain of K fma from zero, or any order of adding K terms: K U S, S the sum of the absolute terms.
  * linear stage relu(a W' + b): (K + 2) U (|a| |W|' + |b|): the chain, the bias's addition, one spare; relu is 1-Lipschitz.
  * a head (mu, v) in dwa_act_out / dwa_heads_bwd: 8 fma per lane, six exchange levels, the bias: 16 U S.
  * a K = B product per slab of n rows: (n + 1) U S_slab; the slabs added in order: nz U S more; the `+=` into g: U |g|.
  * expf: no accuracy table of the device library is installed with this ROCm, so 2 ulp = 4 U relative is ASSUMED; `/` and sqrtf are
    correctly rounded (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt), U each.
The chains through nlp, ratio = exp(old - nlp) and the surrogate are derived in `heads`.

The workspace mirror (`layout`, `xl_of`, `slabs_of`, `slab_rows`) restates the host side of dw_amp_policy.hip; `check_layout` verifies it on
every use: the byte count, the ones columns, the NaN prefill in every word the kernels never write.

The surrogate is discontinuous where ratio = 1 -+ e_clip.  `case` sets the shift of the rows near either boundary to zero; `heads` reports
the rows whose ratio -- from the h2 the kernel had -- is within its own error of a boundary, and the checks require that there are none."""
from __future__ import annotations

import math

import torch

import amp_policy_truth as T
from isaacgymdyros_amd import amp_policy as AP

U = 2.0 ** -24
HID, D_MAX, A_MAX = AP.HID, AP.D_MAX, AP.A_MAX
HL, DL, HEAD_BLOCKS, RW, TK = HID + 4, 32, 2048, 4, 32          # dw_amp_policy.hip: HL, DL, HEAD_BLOCKS, RW, TK
DV_COL = 16                                                     # dv's column of a dd row
SLAB_ROWS, MAX_SLABS = 4096, 16
HALF_LOG_2PI = 0.9189385332046727


def f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


NORM_EPS, NORM_CLIP = f32(1e-5), 5.0
COEF = (0.2, 5.0, 10.0)          # DwaLoss as the learner passes it: e_clip, critic_coef, bounds_coef
E32 = f32(COEF[0])
LO32, HI32 = f32(1.0 - E32), f32(1.0 + E32)          # dwa_heads_bwd: lo = (float)(1.0 - (double)e), hi = (float)(1.0 + (double)e)
GEN_MARGIN = 2.0          # `case` clears rows within this many derived margins: its float64 forward is not the fp32 forward the kernel ran

# (B, D, A, what it reaches)
CASES = [(1, 1, 1, "one row, one k, one action"),
         (5, 3, 16, "XL = 4; second heads workgroup with one row; A = 16 next to dv"),
         (17, 33, 1, "second MFMA row tile with one row; second k slice with one word"),
         (63, 31, 12, "wave edge from below; k slice from below"),
         (65, 32, 16, "wave edge from above; exactly one k slice"),
         (127, 127, 12, "tile edge from below; N = 128 in the layer-1 gradient"),
         (129, 128, 12, "second row tile with one row; N = 129"),
         (257, 512, 16, "D_MAX; N = 513"),
         (4096, 468, 12, "last one-slab size"),
         (4097, 511, 1, "two slabs, the second ragged; N = 512"),
         (8193, 468, 12, "three slabs; the heads' second grid-stride trip for one row")]


def case_seed(B, D, A):
    return 100000 + 1000 * A + 7 * D + B


def f64(t):
    return t.to(torch.float64)


# ------------------------------------------------------------------------------------------------ the workspace mirror
def xl_of(D):
    return (D + 1 + 3) // 4 * 4


def slabs_of(B):
    return 1 if B <= SLAB_ROWS else min((B + SLAB_ROWS - 1) // SLAB_ROWS, MAX_SLABS)


def slab_rows(B):
    """wgrad's split of the B rows: nz slabs of kc rows, kc rounded up to a k slice; the last one takes what is left."""
    nz = slabs_of(B)
    kc = ((B + nz - 1) // nz + TK - 1) // TK * TK
    return [(z * kc, min(B, (z + 1) * kc)) for z in range(nz)]


def up(x):
    return (x + 63) // 64 * 64


def layout(R, D, grad):
    """Float offsets of the workspace's regions, and the words of each that a call may write (`used`)."""
    w = {"xn": 0}
    w["h1"] = up(R * xl_of(D))
    w["h2"] = up(w["h1"] + 2 * R * HL)
    end = up(w["h2"] + 2 * R * HL)
    used = {"xn": R * xl_of(D), "h1": 2 * R * HL, "h2": 2 * R * HL}
    if grad:
        w["z2"] = end
        w["dd"] = up(w["z2"] + 2 * R * HL)
        w["part"] = up(w["dd"] + R * DL)
        w["slab"] = up(w["part"] + HEAD_BLOCKS * 4)
        end = up(w["slab"] + 2 * slabs_of(R) * HID * (HID + 1))
        used.update({"z2": 2 * R * HL, "dd": R * DL, "part": HEAD_BLOCKS * 4, "slab": 2 * slabs_of(R) * HID * (HID + 1)})
    w["end"] = end
    return w, used


def workspace_bytes(R, D, A, grad):
    return layout(R, D, grad)[0]["end"] * 4


def views(W, R, D, grad):
    w, _ = layout(R, D, grad)
    v = {"xn": W[:R * xl_of(D)].view(R, xl_of(D)), "h1": W[w["h1"]:w["h1"] + 2 * R * HL].view(2, R, HL),
         "h2": W[w["h2"]:w["h2"] + 2 * R * HL].view(2, R, HL)}
    if grad:
        v["z2"] = W[w["z2"]:w["z2"] + 2 * R * HL].view(2, R, HL)
        v["dd"] = W[w["dd"]:w["dd"] + R * DL].view(R, DL)
        v["part"] = W[w["part"]:w["part"] + HEAD_BLOCKS * 4].view(HEAD_BLOCKS, 4)
        v["slab"] = W[w["slab"]:w["end"]]
    return v


def heads_blocks(B):
    return min((B + RW - 1) // RW, HEAD_BLOCKS)


def _all_nan(t):
    return bool(torch.isnan(t).all())


def check_layout(W, R, D, A, grad, nbytes=None, nets=(0, 1)):
    """The mirror against a workspace that was NaN everywhere before ONE call of dwa_act / dwa_critic (grad = 0; nets: those it ran) or
    dwa_grad (grad = 1).  nbytes: dwa_workspace_bytes(R, D, A, grad) where it could be asked.  Only dwa_grad asks dwa_norm_rows for the ones
    columns of h1 and h2 (its weight-gradient products read them); after dwa_act / dwa_critic column 512 is as unwritten as 513..515."""
    w, used = layout(R, D, grad)
    if nbytes is not None:
        assert w["end"] * 4 == nbytes, ("workspace size", w["end"] * 4, nbytes)
    assert W.numel() >= w["end"]
    order = ["xn", "h1", "h2"] + (["z2", "dd", "part", "slab"] if grad else [])
    for i, name in enumerate(order):          # the padding between the regions
        nxt = w[order[i + 1]] if i + 1 < len(order) else w["end"]
        assert w[name] + used[name] <= nxt, name
        assert _all_nan(W[w[name] + used[name]:nxt]), ("padding after", name)
    v = views(W, R, D, grad)
    XL = xl_of(D)
    assert bool((v["xn"][:, D] == 1.0).all()) and bool((v["xn"][:, D + 1:XL] == 0.0).all()), "xn: the ones column and the padding"
    assert bool(torch.isfinite(v["xn"]).all())
    if grad:
        dd = v["dd"]
        assert bool(torch.isfinite(dd[:, :A]).all()) and bool(torch.isfinite(dd[:, DV_COL]).all()), "dd: dmu and dv"
        assert _all_nan(dd[:, A:DV_COL]) and _all_nan(dd[:, DV_COL + 1:]), "dd: columns A..15 and 17..31"
        assert bool(torch.isfinite(v["z2"][:, :, :HID]).all()) and _all_nan(v["z2"][:, :, HID:]), "z2: columns 512..515"
        nb = heads_blocks(R)
        assert bool(torch.isfinite(v["part"][:nb]).all()) and _all_nan(v["part"][nb:]), "part"
    for name in ("h1", "h2"):
        for n in (0, 1):
            h = v[name][n]
            if n not in nets:
                assert _all_nan(h), (name, n, "a net the call did not run")
                continue
            assert bool(torch.isfinite(h[:, :HID]).all()), (name, n)
            if grad:
                assert bool((h[:, HID] == 1.0).all()), (name, n, "ones column")
                assert _all_nan(h[:, HID + 1:]), (name, n, "columns 513..515")
            else:
                assert _all_nan(h[:, HID:]), (name, n, "columns 512..515")


# ------------------------------------------------------------------------------------------------ parameters
def split(flat, D, A):
    """The flat parameter (or gradient) buffer as views in the layout order of amp_policy.ActorCritic.params_in_layout."""
    shapes = [(HID, D), (HID,), (HID, HID), (HID,), (A, HID), (A,), (HID, D), (HID,), (HID, HID), (HID,), (1, HID), (1,)]
    out, o = [], 0
    for s in shapes:
        n = math.prod(s)
        out.append(flat[o:o + n].view(s))
        o += n
    assert o == flat.numel() == AP.num_params(D, A)
    return out


NAMES = ["a_W1", "a_b1", "a_W2", "a_b2", "mu_W", "mu_b", "c_W1", "c_b1", "c_W2", "c_b2", "v_w", "v_b"]
# index into `split` of (W1, b1, W2, b2, head W, head b) per net
NET = ((0, 1, 2, 3, 4, 5), (6, 7, 8, 9, 10, 11))


# ------------------------------------------------------------------------------------------------ S1: normalisation
def norm(obs, stats, D):
    """dwa_norm_rows: clamp((x - (float)mean) / sqrtf((float)var + 1e-5f), +-5).  One rounding each for the subtraction, var + eps, sqrtf
    (half of its operand's error) and the division: 3.5 U, stated as 4 U |y|; the clamp is monotone and 1-Lipschitz, and a y further than
    that beyond +-5 is clamped whatever its rounding."""
    mu, var = f64(stats[:D].float()), f64(stats[D:2 * D].float())
    y = (f64(obs) - mu) / torch.sqrt(var + NORM_EPS)
    bound = torch.where(y.abs() * (1.0 - 4.0 * U) > NORM_CLIP, torch.zeros_like(y), 4.0 * U * y.abs())
    return torch.clamp(y, -NORM_CLIP, NORM_CLIP), bound


# ------------------------------------------------------------------------------------------------ S2, S6: linear stages
def linear(a, w, b=None):
    """t = a w' (+ b) and (K + 2) U (|a| |w|' + |b|) for the stored a [R, K], w [N, K], b [N]."""
    a, w = f64(a), f64(w)
    t, S = a @ w.T, a.abs() @ w.abs().T
    if b is not None:
        t, S = t + f64(b), S + f64(b).abs()
    return t, (a.shape[1] + 2) * U * S


def hidden(a, w, b):
    t, bound = linear(a, w, b)
    return torch.relu(t), bound


def masked(t, h):
    """relu's backward with the mask of the stored activation."""
    return t * (f64(h) > 0).double()


# ------------------------------------------------------------------------------------------------ S3: heads
def head(h2, w, b):
    """A head of dwa_act_out / dwa_critic_out / dwa_heads_bwd: 8 fma per lane, six exchange levels, the bias: 16 U S."""
    h2, w, b = f64(h2), f64(w), f64(b)
    return h2 @ w.T + b, 16.0 * U * (h2.abs() @ w.abs().T + b.abs())


def unnorm(v, e_v, val_stats):
    """ActorCritic.unnorm_value, unfused: v * sqrtf((float)var + eps) + (float)mean.  The factor carries 1.5 U (the sum, half of it through
    sqrtf, sqrtf itself), the product U, the sum U |value|."""
    s = math.sqrt(float(val_stats[1].float()) + NORM_EPS)
    val = v * s + float(val_stats[0].float())
    return val, e_v * s + 4.0 * U * v.abs() * s + U * val.abs()


def act_out(h2a, h2c, P, logstd, noise, val_stats, mu_k, act_k):
    """dwa_act_out from the stored h2 of both nets; the action from the mu it wrote (mu_k), neglogp from the action and mu it wrote.
    action = mu + sd * noise: sd = expf(logstd) 4 U, the product U, the sum U: 6 U |sd noise| + U |action| (one spare).
    neglogp: z = (a - mu) / sd carries 6 U (subtraction, sd, division), its square 13 U, the in-order sum over A another A U: (A + 13) U sq;
    the constant's rounding, the A - 1 additions of logstd and the two last sums: together below (A + 16) U M, M = 0.5 sq + c + sum |logstd|."""
    ls, noise, mu_k, act_k = f64(logstd), f64(noise), f64(mu_k), f64(act_k)
    A = ls.numel()
    sd = torch.exp(ls)
    mu, e_mu = head(h2a, P[4], P[5])
    v, e_v = head(h2c, P[10], P[11])
    action = mu_k + sd * noise
    e_action = 6.0 * U * (sd * noise).abs() + U * action.abs()
    sq = (((act_k - mu_k) / sd) ** 2).sum(-1)
    c = HALF_LOG_2PI * A
    nlp = 0.5 * sq + c + ls.sum()
    e_nlp = (A + 16.0) * U * (0.5 * sq + c + ls.abs().sum())
    value, e_value = unnorm(v.reshape(-1), e_v.reshape(-1), val_stats)
    return {"mu": (mu, e_mu), "action": (action, e_action), "neglogp": (nlp, e_nlp), "value": (value, e_value)}


def heads_trips(B):
    nb = heads_blocks(B)
    return nb, (B + nb * RW - 1) // (nb * RW)


def heads(h2a, h2c, P, logstd, act, old, adv, ret, coef=COEF, rounded=True):
    """dwa_heads_bwd from the stored h2 of both nets (any float type; computed in float64).  Absolute errors e_*, first order:
      mu, v        16 U S (`head`)
      z            (a - mu) / sd: e_z = e_mu / sd + 6 U |z|          (subtraction U, sd = expf 4 U, division U)
      sq           sum z^2 in order: e_sq = sum(2 |z| e_z + e_z^2) + (A + 1) U sq
      nlp          0.5 sq + c + lsum: e_nlp = 0.5 e_sq + (A + 3) U M, M = 0.5 sq + c + sum |logstd|
      ratio        expf(old - nlp): the difference carries e_d = e_nlp + U |old - nlp|, expf turns it into the relative expm1(e_d) and adds
                   4 U of its own: e_r = ratio (expm1(e_d) + 4 U)
      boundaries   a row whose |ratio - lo| or |ratio - hi| is within e_r + 2 U (lo, hi as the kernel rounds them; the clip fraction compares
                   with 1 -+ e_clip unrounded) is `near`: its branch is not determined.  For every other row the weight w of -adv in
                   dratio is exact: 1 inside [lo, hi] (the tie: halves of both branches), else 1 or 0 by the sign of adv.
      dratio       w (-adv) / B: 1 / B and the product, 2 U; dnlp = -ratio dratio: relative rho + 3 U, rho = e_r / ratio
      dmu          dnlp q + c2 (hi1 + lo1), q = -z / sd (e_q = e_z / sd + 5 U |q|), c2 = 2 bounds_coef / B (2 U):
                   e = |t1| (rho + 9 U) + |dnlp| e_z / sd + c2 e_mu + 6 U |t2| + U |dmu|
      dv           cv (v - ret), cv = 2 critic_coef / B: e = cv e_v + 4 U |dv|
      rows' losses a: |adv| e_r + 2 U |a|; c: 2 |ret - v| e_v + e_v^2 + 3 U c; b: sum(2 (|hi1| + |lo1|) e_mu + 2 e_mu^2) + (2 A + 4) U b
      logged sums  the rows' errors, plus (trips + RW + blocks + 2) U sum |rows| for the adds (wave, workgroup, dwa_log_sum's sequential
                   loop) and the division by B; the caller adds U |state| for the `+=`."""
    h2a, h2c, ls, act, old, adv, ret = (f64(t) for t in (h2a, h2c, logstd, act, old, adv, ret))
    B, A = act.shape
    e_clip, critic_coef, bounds_coef = coef
    lo, hi = 1.0 - e_clip, 1.0 + e_clip
    if rounded:          # the coefficients as fp32 words, lo and hi as the kernel rounds them (else: the formulas in exact arithmetic)
        e_clip, critic_coef, bounds_coef = f32(coef[0]), f32(coef[1]), f32(coef[2])
        lo, hi = f32(1.0 - e_clip), f32(1.0 + e_clip)
    sd = torch.exp(ls)
    mu, e_mu = head(h2a, P[4], P[5])
    v, e_v = head(h2c, P[10], P[11])
    v, e_v = v.reshape(-1), e_v.reshape(-1)
    z = (act - mu) / sd
    e_z = e_mu / sd + 6.0 * U * z.abs()
    sq = (z ** 2).sum(-1)
    e_sq = (2.0 * z.abs() * e_z + e_z ** 2).sum(-1) + (A + 1.0) * U * sq
    c = HALF_LOG_2PI * A
    M = 0.5 * sq + c + ls.abs().sum()
    nlp = 0.5 * sq + c + ls.sum()
    e_nlp = 0.5 * e_sq + (A + 3.0) * U * M
    d = old - nlp
    e_d = e_nlp + U * d.abs()
    ratio = torch.exp(d)
    rho = torch.expm1(e_d) + 4.0 * U
    e_r = ratio * rho
    margin = e_r + 2.0 * U
    near = ((ratio - lo).abs() <= margin) | ((ratio - hi).abs() <= margin)
    inside = (ratio >= lo) & (ratio <= hi)
    x1, x2 = -adv * ratio, -adv * torch.clamp(ratio, lo, hi)
    g1 = torch.where(inside, 0.5, torch.where(x1 > x2, 1.0, torch.where(x1 == x2, 0.5, 0.0))).double()
    w = g1 + (1.0 - g1) * inside.double()
    dratio = w * -adv / B
    dnlp = -ratio * dratio
    q = -z / sd
    t1 = dnlp[:, None] * q
    hi1, lo1 = torch.clamp(mu - 1.0, min=0.0), torch.clamp(mu + 1.0, max=0.0)
    c2, cv = 2.0 * bounds_coef / B, 2.0 * critic_coef / B
    t2 = c2 * (hi1 + lo1)
    dmu = t1 + t2
    e_dmu = t1.abs() * (rho[:, None] + 9.0 * U) + dnlp.abs()[:, None] * e_z / sd + c2 * e_mu + 6.0 * U * t2.abs() + U * dmu.abs()
    dv = cv * (v - ret)
    e_dv = cv * e_v + 4.0 * U * dv.abs()
    a_rows = torch.maximum(x1, x2)
    e_a = adv.abs() * e_r + 2.0 * U * a_rows.abs()
    c_rows = (ret - v) ** 2
    e_c = 2.0 * (ret - v).abs() * e_v + e_v ** 2 + 3.0 * U * c_rows
    b_rows = (hi1 ** 2 + lo1 ** 2).sum(-1)
    e_b = (2.0 * (hi1.abs() + lo1.abs()) * e_mu + 2.0 * e_mu ** 2).sum(-1) + (2.0 * A + 4.0) * U * b_rows
    f_rows = ((ratio - 1.0).abs() > e_clip).double()
    nb, trips = heads_trips(B)
    adds = (trips + RW + nb + 2.0) * U
    sums, e_sums = [], []
    for rows, e in ((a_rows, e_a), (c_rows, e_c), (b_rows, e_b), (f_rows, torch.zeros_like(f_rows))):
        sums.append(rows.sum() / B)
        e_sums.append(e.sum() / B + adds * rows.abs().sum() / B)
    return {"mu": mu, "v": v, "nlp": nlp, "ratio": ratio, "e_r": e_r, "margin": margin, "near": near, "dmu": (dmu, e_dmu), "dv": (dv, e_dv),
            "sums": (torch.stack(sums), torch.stack(e_sums)), "loss": sums[0] + critic_coef * sums[1] + bounds_coef * sums[2]}


def dz2(dd, h2a, h2c, P, A):
    """dZ2 of both nets from the dd rows the kernel wrote and its own h2: the actor's an fma chain over A terms, (A + 1) U sum |dmu| |muW|;
    the critic's one product, U |dv w|; zero where the stored h2 is."""
    dmu, dv = f64(dd[:, :A]), f64(dd[:, DV_COL])
    mw, vw = f64(P[4]), f64(P[10]).reshape(-1)
    ta, ba = dmu @ mw, (A + 1.0) * U * (dmu.abs() @ mw.abs())
    tc = dv[:, None] * vw[None, :]
    ma, mc = (f64(h2a) > 0).double(), (f64(h2c) > 0).double()
    return (ta * ma, ba * ma), (tc * mc, U * tc.abs() * mc)


# ------------------------------------------------------------------------------------------------ S4, S5, S7: K = B products
def wgrad(x, y, B):
    """[dW | db] = x' y over the B rows for the stored x [B, M] and y [B, N] (y's last column the ones), slab by slab as `slab_rows` splits them:
    ([(g_s, (n_s + 1) U S_s)], g, bound of the in-order sum of the slabs = sum of the slabs' bounds + nz U S)."""
    x, y = f64(x), f64(y)
    slabs, g, bound, S_all = [], 0.0, 0.0, 0.0
    rows = slab_rows(B)
    for r0, r1 in rows:
        gs, Ss = x[r0:r1].T @ y[r0:r1], x[r0:r1].abs().T @ y[r0:r1].abs()
        bs = (r1 - r0 + 1.0) * U * Ss
        slabs.append((gs, bs))
        g, bound, S_all = g + gs, bound + bs, S_all + Ss
    return slabs, g, bound + len(rows) * U * S_all


# ------------------------------------------------------------------------------------------------ the checks
class Worst(dict):
    """Per stage the worst |got - truth| / bound; `note` asserts it is at most 1 (and that nothing is NaN)."""

    def __init__(self, label):
        super().__init__()
        self.label = label

    def note(self, name, got, t, bound, extra=None):
        got = f64(got)
        if extra is not None:
            bound = bound + extra
        assert got.shape == t.shape, (self.label, name, got.shape, t.shape)
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(t).all()) and bool(torch.isfinite(bound).all()), (self.label, name, "not finite")
        err = (got - t).abs()
        fr = float(torch.where(err > 0, err / torch.clamp(bound, min=1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.0
        self[name] = max(self.get(name, 0.0), fr)
        assert fr <= 1.0, (self.label, name, "error / bound", fr, "worst error", float(err.max()))

    def line(self):
        return "amp-edges %s: " % self.label + ", ".join("%s %.3f" % kv for kv in self.items())


def _forward_checks(wo, c, v, nets):
    """S1 and S2 on a workspace's views: xn from the observations, h1 from the stored xn, h2 from the stored h1."""
    D, P = c["D"], c["P"]
    t, bound = norm(c["obs"], c["obs_stats"], D)
    wo.note("xn", v["xn"][:, :D], t, bound)
    for n in nets:
        W1, b1, W2, b2 = (P[i] for i in NET[n][:4])
        t, bound = hidden(v["xn"][:, :D], W1, b1)
        wo.note("h1", v["h1"][n][:, :HID], t, bound)
        t, bound = hidden(v["h1"][n][:, :HID], W2, b2)
        wo.note("h2", v["h2"][n][:, :HID], t, bound)


def check_act(c, W, out, nbytes=None):
    """dwa_act: W the workspace (NaN before the call), out = (action, clamped, mu, neglogp, value)."""
    N, D, A = c["B"], c["D"], c["A"]
    wo = Worst("act N=%d D=%d A=%d" % (N, D, A))
    check_layout(W, N, D, A, 0, nbytes)
    v = views(W, N, D, 0)
    _forward_checks(wo, c, v, (0, 1))
    action, clamped, mu, nlp, value = out
    R = act_out(v["h2"][0][:, :HID], v["h2"][1][:, :HID], c["P"], c["logstd"], c["noise"], c["val_stats"], mu, action)
    wo.note("mu", mu, *R["mu"])
    wo.note("action", action, *R["action"])
    wo.note("neglogp", nlp, *R["neglogp"])
    wo.note("value", value.reshape(-1), *R["value"])
    assert torch.equal(clamped, torch.clamp(action, -1.0, 1.0))
    return wo


def check_critic(c, W, value, nbytes=None):
    """dwa_critic: its h2 sits at the critic's offset, the actor's half of the workspace keeps its prefill; the terminate mask is exact."""
    N, D, A = c["B"], c["D"], c["A"]
    wo = Worst("critic N=%d D=%d A=%d" % (N, D, A))
    check_layout(W, N, D, A, 0, nbytes, nets=(1,))
    v = views(W, N, D, 0)
    _forward_checks(wo, c, v, (1,))
    t, e = head(v["h2"][1][:, :HID], c["P"][10], c["P"][11])
    t, e = unnorm(t.reshape(-1), e.reshape(-1), c["val_stats"])
    live = c["term"] == 0
    value = value.reshape(-1)
    assert bool((value[~live] == 0.0).all())
    wo.note("value", value[live], t[live], e[live])
    return wo


def check_grad(c, Wg, Wa, g, g0, state, state0, nbytes=None, nbytes_act=None, layout_checks=True):
    """dwa_grad: Wg its workspace, Wa that of dwa_act on the same rows (h1's source: dwa_grad overwrites its own with dZ1), g / state after
    and g0 / state0 before the call.  layout_checks False: Wg was not NaN before this call (a reused workspace)."""
    B, D, A, P = c["B"], c["D"], c["A"], c["P"]
    wo = Worst("grad B=%d D=%d A=%d" % (B, D, A))
    if layout_checks:
        check_layout(Wg, B, D, A, 1, nbytes)
    check_layout(Wa, B, D, A, 0, nbytes_act)
    vg, va = views(Wg, B, D, 1), views(Wa, B, D, 0)
    # the two calls ran the same forward(): the same bits, which is what makes dwa_act's h1 the operand dwa_grad had
    assert torch.equal(vg["xn"], va["xn"]) and torch.equal(vg["h2"][:, :, :HID], va["h2"][:, :, :HID]), "dwa_act and dwa_grad: different forward bits"
    _forward_checks(wo, c, va, (0, 1))
    h1, h2, z2, dd = va["h1"][:, :, :HID], vg["h2"], vg["z2"][:, :, :HID], vg["dd"]
    assert bool((h2[:, :, HID] == 1.0).all()) and bool((vg["h1"][:, :, HID] == 1.0).all()), "ones columns"
    # ---- S3
    H = heads(h2[0][:, :HID], h2[1][:, :HID], P, c["logstd"], c["act"], c["old"], c["adv"], c["ret"])
    assert int(H["near"].sum()) == 0, ("rows on a clip boundary", H["near"].nonzero().reshape(-1).tolist())
    wo.note("dmu", dd[:, :A], *H["dmu"])
    wo.note("dv", dd[:, DV_COL], *H["dv"])
    ds = f64(state[:4]) - f64(state0[:4])
    wo.note("logs", ds, *H["sums"], extra=U * f64(state[:4]).abs())
    want = state0.clone()
    want[AP.K["DWA_S_UPDATES"]] += 1.0
    assert torch.equal(state[4:], want[4:]), "state: the update count, and the words dwa_grad does not own"
    (ta, ba), (tc, bc) = dz2(dd, h2[0][:, :HID], h2[1][:, :HID], P, A)
    wo.note("dz2", z2[0], ta, ba)
    wo.note("dz2", z2[1], tc, bc)
    # ---- S4, S5, S7: g - g0 per parameter
    G, G0 = split(g, D, A), split(g0, D, A)

    def acc(name, iw, ib, total, bound):
        for i, sl in ((iw, slice(None, -1)), (ib, -1)):
            got = f64(G[i]) - f64(G0[i])
            wo.note(name, got.reshape(total[:, sl].shape), total[:, sl], bound[:, sl], extra=U * f64(G[i]).abs().reshape(total[:, sl].shape))

    _, t, bound = wgrad(dd[:, :A], h2[0][:, :HID + 1], B)
    acc("g_heads", 4, 5, t, bound)
    _, t, bound = wgrad(dd[:, DV_COL:DV_COL + 1], h2[1][:, :HID + 1], B)
    acc("g_heads", 10, 11, t, bound)
    one = torch.ones(B, 1, dtype=torch.float64, device=h1.device)
    XL = xl_of(D)
    nz, zs = slabs_of(B), HID * (D + 1)
    for n in (0, 1):
        _, t, bound = wgrad(z2[n], torch.cat([f64(h1[n]), one], 1), B)
        acc("g_layer2", NET[n][2], NET[n][3], t, bound)
        # ---- S6
        t, bound = linear(z2[n], P[NET[n][2]].T)
        dz1 = vg["h1"][n][:, :HID]
        wo.note("dz1", dz1, masked(t, h1[n]), bound * (f64(h1[n]) > 0).double())
        # ---- S7, slab by slab as they lie in the workspace, then summed
        slabs, t, bound = wgrad(dz1, vg["xn"][:, :D + 1], B)
        assert D + 1 <= XL
        for z, (ts, bs) in enumerate(slabs):
            o = (n * nz + z) * zs
            wo.note("slab1", vg["slab"][o:o + zs].view(HID, D + 1), ts, bs)
        acc("g_layer1", NET[n][0], NET[n][1], t, bound)
    return wo


# ------------------------------------------------------------------------------------------------ composed truth (for the CPU test)
def composed_loss(xn, P, logstd, act, old, adv, ret):
    """The loss as these stages compose it, differentiable in float64: hidden -> hidden -> heads' formulas (tests/test_amp_policy_edges.py
    holds its autograd gradient against amp_policy_truth.loss_and_grad)."""
    h2 = []
    for n in (0, 1):
        W1, b1, W2, b2 = (P[i] for i in NET[n][:4])
        h2.append(torch.relu(torch.relu(xn @ W1.T + b1) @ W2.T + b2))
    return heads(h2[0], h2[1], P, logstd, act, old, adv, ret, rounded=False)


# ------------------------------------------------------------------------------------------------ the input generator
def case(B, D, A, seed=None, device="cpu"):
    """One case as tests/test_amp_policy_gpu.py::grad_case makes them: nn.Linear's initialisation, nontrivial statistics, a mu bias that puts
    mu beyond +-1 in many rows, actions 0.2 sigma-units... around mu, old_nlp = nlp + 0.3 randn (ratios inside and beyond the clip range on both
    sides), every fourth row with shift 0 (ratio 1 to rounding: the tie of the surrogate's two terms).  Random numbers come from CPU
    generators; the float64 forward that places act and old_nlp runs on `device`.  Rows whose float64 ratio is within GEN_MARGIN derived
    margins (`heads`) of 1 -+ e_clip get shift 0 too; at most 1 % of the rows may be altered that way (asserted).  Returns a dict of tensors
    on `device` (fp32 unless noted): p, P (views of p), obs_stats / val_stats (float64), logstd, obs, act, old, adv, ret, noise, term, and
    `altered`."""
    seed = case_seed(B, D, A) if seed is None else seed
    torch.manual_seed(seed)
    net = AP.ActorCritic(D, A, [HID, HID], -1.6)
    g = torch.Generator().manual_seed(seed + 1)
    r64 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    obs_stats = torch.cat([r64(D) * 0.5, torch.rand(D, generator=g, dtype=torch.float64) * 2 + 0.2, torch.tensor([1000.0], dtype=torch.float64)])
    val_stats = torch.tensor([0.7, 2.5, 1000.0], dtype=torch.float64)
    with torch.no_grad():
        net.mu.bias[:] = torch.randn(A, generator=g) * 1.5
    p = torch.cat([t.detach().reshape(-1) for t in net.params_in_layout()]).float()
    obs = torch.randn(B, D, generator=g) * 1.5
    da, shift = 0.2 * r64(B, A), 0.3 * r64(B)
    shift[torch.arange(B) % 4 == 1] = 0.0
    adv, ret, noise = torch.randn(B, generator=g), torch.randn(B, generator=g), torch.randn(B, A, generator=g)
    term = (torch.rand(B, generator=g) < 0.3).float()
    logstd = net.sigma.detach().clone().float()
    c = {"B": B, "D": D, "A": A, "p": p, "obs_stats": obs_stats, "val_stats": val_stats, "logstd": logstd, "obs": obs, "adv": adv, "ret": ret,
         "noise": noise, "term": term}
    c = {k: (t.to(device) if torch.is_tensor(t) else t) for k, t in c.items()}
    c["P"] = split(c["p"], D, A)
    da, shift = da.to(device), shift.to(device)
    P64 = [f64(t) for t in c["P"]]
    xn, _ = norm(c["obs"], c["obs_stats"], D)
    _, h2a, _, h2c, mu, _ = T.forward(xn, P64)
    c["act"] = (mu + da).float().contiguous()
    ls = logstd.to(device)
    nlp = heads(h2a, h2c, P64, ls, c["act"], torch.zeros_like(c["adv"]), c["adv"], c["ret"])["nlp"]
    H = heads(h2a, h2c, P64, ls, c["act"], (nlp + shift).float(), c["adv"], c["ret"])
    margin = GEN_MARGIN * H["margin"]
    near = ((H["ratio"] - LO32).abs() <= margin) | ((H["ratio"] - HI32).abs() <= margin)
    shift[near] = 0.0
    c["old"] = (nlp + shift).float().contiguous()
    c["altered"] = int(near.sum())
    assert c["altered"] <= 0.01 * B, ("rows moved off the clip boundaries", c["altered"], B)
    return c
