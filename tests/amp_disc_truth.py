"""Float64 truth and fp32 error bounds for the AMP discriminator's kernels (tests/test_amp_disc_gpu.py, tests/test_amp_disc_reference_gpu.py).

The truth is autograd through amp_disc.torch_disc_loss in float64 (the restatement tests/test_amp_disc_reference.py holds bit for bit to
the reference's own _disc_loss), on the rows the kernels see after their fp32 normalisation.  The per-entry bound is the `abs_logit64` idea
carried through the whole gradient: the analytic gradient (csrc/dw_amp_disc.hip, head comment) evaluated with the absolute value of every
operand and the true relu masks, T, so that an fp32 evaluation in any summation order whose longest chain of dependent roundings is n
differs from the exact value by at most about n u T (first order in u = 2^-24)."""
import math

import torch

from isaacgymdyros_amd import amp_disc as AD

U = 2.0 ** -24
HID = AD.HID
C = AD.TRAIN_CFG["config"]
COEF = dict(disc_coef=float(C["disc_coef"]), logit_reg=float(C["disc_logit_reg"]), grad_penalty=float(C["disc_grad_penalty"]),
            weight_decay=float(C["disc_weight_decay"]))
SIZES = lambda D: [D * HID, HID, HID * HID, HID, HID, 1]          # noqa: E731  (the parameter layout of include/dyros_amp_disc.h)


def split(p, D):
    out, o = [], 0
    for n, shape in zip(SIZES(D), [(HID, D), (HID,), (HID, HID), (HID,), (HID,), (1,)]):
        out.append(p[o:o + n].view(shape))
        o += n
    return out


def normalise(x, st, D):
    """The eval-mode RunningMeanStd output the kernels compute: fp32 statistics, (x - mean) / sqrt(var + 1e-5), clamped at +-5."""
    return torch.clamp((x - st[:D].float()) / torch.sqrt(st[D:2 * D].float() + AD.RMS_EPS), -5.0, 5.0)


def loss_grad(p, D, an, rn, dn, dtype, coef=COEF):
    """(flat gradient of disc_coef * disc_loss, the nine logged values in LOG_NAMES order as float64) by autograd in `dtype`."""
    net = AD.DiscNet(D).to(device=p.device, dtype=dtype)
    ps = [net._disc_mlp[0].weight, net._disc_mlp[0].bias, net._disc_mlp[2].weight, net._disc_mlp[2].bias, net._disc_logits.weight,
          net._disc_logits.bias]
    with torch.no_grad():
        for t, s in zip(ps, split(p, D)):
            t.copy_(s.reshape(t.shape))
    total, vals = AD.torch_disc_loss(net, an.to(dtype), rn.to(dtype), dn.to(dtype).detach().clone(), **coef)
    g = torch.autograd.grad(total, ps)
    return torch.cat([x.reshape(-1) for x in g]).detach(), torch.stack([v.detach().double() for v in vals])


def slab_chain(R):
    """The longest chain of dependent fp32 roundings dwd_grad's row sums take (csrc/dw_amp_disc.hip: slabs_for, the gemm's kc, the column
    sums' four phases over S3 = 4 S slabs), for R rows."""
    S = 1 if R <= 1024 else min(R // 1024, 64)
    kc = (math.ceil(R / S) + 15) // 16 * 16
    kc3 = math.ceil(R / (4 * S))
    return max(kc + S, kc3 // 4 + 4 + 4 * S)


def bounds(p, D, xa, xd, l32=None, coef=COEF):
    """The per-entry fp32 error bound of dwd_grad's gradient on normalised agent + replay rows xa and demo rows xd, and what the logged
    values' tolerances need.  Every matrix is float64 on p's device."""
    W1, b1, W2, b2, w3, b3 = (t.double() for t in split(p, D))
    X = torch.cat([xa, xd]).double()
    R, nA = X.shape[0], xa.shape[0]
    nd = R - nA
    demo = torch.arange(R, device=X.device) >= nA
    h1 = torch.relu(X @ W1.T + b1)
    h2 = torch.relu(h1 @ W2.T + b2)
    l = h2 @ w3 + b3
    m1, m2 = (h1 > 0).double(), (h2 > 0).double()
    aW1, aW2, aw3 = W1.abs(), W2.abs(), w3.abs()
    H1 = X.abs() @ aW1.T + b1.abs()
    H2 = H1 @ aW2.T + b2.abs()
    lb = 2 * (D + 2 * HID + 8) * U * (H2 @ aw3 + b3.abs())          # the logit bound (abs_logit64)
    # what the logit's error does to dl: with lively weights lb is far above any real fp32 error, so where an fp32 evaluation of the
    # logits (l32) is at hand its observed error, times 16, stands in for lb in dl
    dlb = lb if l32 is None else 16 * (l32.double() - l).abs() + 64 * U * (1 + l.abs())
    c = torch.where(demo, 0.5 * coef["disc_coef"] / nd, 0.5 * coef["disc_coef"] / max(nA, 1))
    sig = torch.sigmoid(l)
    dl = c * (sig - demo.double())
    ddl = c * (sig * (1 - sig) * dlb + 4 * U)          # dl's own error: the logit's through the sigmoid's slope, and the sigmoid's
    n = slab_chain(R) + D + 4 * HID + 64
    alpha = 2 * coef["disc_coef"] * coef["grad_penalty"] / nd
    U2 = m2 * aw3
    U1 = m1 * (U2 @ aW2)
    GX = U1[nA:] @ aW1
    DV1 = m1[nA:] * ((alpha * GX) @ aW1.T)
    E2 = m2[nA:] * (DV1 @ aW2.T)

    def through(DL):          # the part of the gradient linear in dl, with |operands|
        return [U1.T @ (DL[:, None] * X.abs()), U1.T @ DL, U2.T @ (DL[:, None] * H1), U2.T @ DL, DL @ H2, DL.sum().reshape(1)]
    wreg = 2 * coef["disc_coef"] * coef["weight_decay"]
    rest = [U1[nA:].T @ (alpha * GX) + wreg * aW1, 0, U2[nA:].T @ DV1 + wreg * aW2, 0,
            E2.sum(0) + 2 * coef["disc_coef"] * (coef["logit_reg"] + coef["weight_decay"]) * aw3, 0]
    T = [2 * n * U * (a + r) + 2 * e for a, r, e in zip(through(dl.abs()), rest, through(ddl))]
    gx = ((m1[nA:] * (((m2[nA:] * w3) @ W2))) @ W1)
    return {"entry": torch.cat([t.reshape(-1) for t in T]), "logit": l, "logit_bound": lb, "gx": gx,
            "gx_bound": 2 * (D + 2 * HID + 8) * U * GX, "nA": nA, "nd": nd}


def logged_tolerance(v64, b, coef=COEF):
    """|state word - float64 value| bounds, LOG_NAMES order, from the logit and input-gradient bounds (`bounds`).  The state words are fp32
    casts of float64 sums: 16 u |v| on top."""
    nA, nd, lb, l = b["nA"], b["nd"], b["logit_bound"], b["logit"]
    la, ld, ba, bd = l[:nA], l[nA:], lb[:nA], lb[nA:]
    pred = 0.5 * (float(ba.mean()) + float(bd.mean()))
    gp = 2.0 * float((b["gx"].abs() * b["gx_bound"]).sum()) / nd
    lsq, wd = 0.0, 0.0
    loss = coef["disc_coef"] * (pred + coef["logit_reg"] * lsq + coef["grad_penalty"] * gp + coef["weight_decay"] * wd)
    acc_a = float((la.abs() <= ba).double().sum()) / nA
    acc_d = float((ld.abs() <= bd).double().sum()) / nd
    tol = torch.tensor([loss, pred, lsq, gp, wd, float(ba.mean()), float(bd.mean()), acc_a, acc_d], dtype=torch.float64, device=v64.device)
    return tol + 16 * U * v64.abs()


def tensor_errors(g, g64, D):
    """max |g - g64| per parameter tensor (W1, b1, W2, b2, w3, b3)."""
    out, o = [], 0
    for n in SIZES(D):
        out.append(float((g[o:o + n].double() - g64[o:o + n]).abs().max()))
        o += n
    return out


def logits(p, D, X, dtype):
    W1, b1, W2, b2, w3, b3 = (t.to(dtype) for t in split(p, D))
    X = X.to(dtype)
    return torch.relu(torch.relu(X @ W1.T + b1) @ W2.T + b2) @ w3 + b3


def reward_params(g, case):
    """The parameters of a reward case of tests/golden/amp_learner_ref.npz: the probe network's, or the grad case's with the logit bias of
    the reward case."""
    if case == "probe":
        return g["probe_p"]
    p = g[case + "/p"].copy()
    p[-1:] = g[case + "/reward_b3"]
    return p
