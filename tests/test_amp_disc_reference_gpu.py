"""The HIP discriminator against float64 truth on an MI355X: the reference's own float64 gradients and rewards (tests/golden/
amp_learner_ref.npz, fed through the C-ABI as raw rows and statistics snapshots, so that dwd_stats does not enter), dwd_grad over the
shapes where its tiles and slabs switch (D = 34 / 68 / 340, 2047 / 2048 / 65 535 / 65 536 rows, one demo row, no agent or no replay rows),
and dwd_stats against float64 two-pass moments.

Tolerances (tests/amp_disc_truth.py): per parameter tensor, the kernel's error against float64 is at most GRAD_MULT times the error of an
fp32 evaluation of the same loss (the reference's own fp32 run for the fixture, torch_disc_loss in fp32 on the GPU elsewhere); per entry,
it is within the abs-value bound `bounds()`; every logged state word is within the bound `logged_tolerance()` derives from the logit and
input-gradient bounds.  The workspace is filled with NaN before each call, so a read of a word no kernel wrote shows."""
import os

import numpy as np
import pytest
import torch

import amp_disc_truth as T
from isaacgymdyros_amd import amp_disc as AD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = T.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "amp_learner_ref.npz")
# The kernel's per-tensor error may be this multiple of a same-precision (fp32) evaluation's.  Measured on an MI355X: up to 86 (b2 at D = 340,
# 2047 rows, one slab).  dwd_grad sums each slab's rows in one fp32 fma chain (up to 6144 rows), and the dl column of the bias gradients
# cancels between the agent and the demo rows; torch's blocked reductions round less.  The per-entry bound is the check that bites.
GRAD_MULT = 128.0
REWARD = dict(scale=2.0, task_w=0.7, disc_w=0.3)          # oracle/make_amp_learner_goldens.py
_api = {}


def api():
    if not _api:
        from isaacgymdyros_amd import _lib
        _api.update(AD.declare(_lib.load()[0]))
    return _api


def stream():
    return torch.cuda.current_stream().cuda_stream


def hip_grad(D, p, a, r, d, sa, sr, sd, coef=T.COEF):
    """dwd_grad through the C-ABI (a / r may be None: n_agent / n_replay = 0) -> (g, state)."""
    A = api()
    na, nr, nd = (0 if x is None else x.shape[0] for x in (a, r, d))
    nb = A["grad_workspace_bytes"](D, na, nr, nd)
    assert nb > 0
    work = torch.full(((nb + 3) // 4,), float("nan"), device=DEV)
    g = torch.zeros_like(p)
    state = torch.zeros(AD.K["DWD_S_WORDS"], device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    rc = A["grad"](p.data_ptr(), ptr(a), na, ptr(r), nr, d.data_ptr(), nd, D, ptr(sa), ptr(sr), sd.data_ptr(), AD.DwdLoss(**coef), g.data_ptr(),
                   state.data_ptr(), work.data_ptr(), work.numel() * 4, stream())
    assert rc == 0, A["last_error"]().decode()
    torch.cuda.synchronize()
    return g, state


def check_grad(D, p, g, state, xa, xd, g64, v64, g32):
    """The three criteria of the module docstring.  xa: the normalised agent + replay rows, xd: the demo rows (fp32, as the kernel's)."""
    l32 = T.logits(p, D, torch.cat([xa, xd]), torch.float32)
    b = T.bounds(p, D, xa, xd, l32)
    err = (g.double() - g64).abs()
    worst = int(torch.argmax(err / b["entry"].clamp_min(1e-300)))
    assert bool((err <= b["entry"]).all()), ("entry", worst, float(g[worst]), float(g64[worst]), float(b["entry"][worst]))
    eh, e32 = T.tensor_errors(g, g64, D), T.tensor_errors(g32, g64, D)
    for i, (x, y) in enumerate(zip(eh, e32)):
        o = sum(T.SIZES(D)[:i])
        floor = 4 * U * float(g64[o:o + T.SIZES(D)[i]].abs().max())
        assert x <= GRAD_MULT * y + floor, ("tensor", i, x, y, floor)
    tol = T.logged_tolerance(v64, b)
    s = state[:9].double()
    assert bool(((s - v64).abs() <= tol).all()), ((s - v64).abs() / tol).tolist()
    assert float(state[AD.K["DWD_S_UPDATES"]]) == 1.0


# ----------------------------------------------------------------------------------------------------- the reference's fixture
@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("D", [34, 68])
def test_grad_against_the_references_float64(D, fixture):
    g_ = fixture
    t = lambda k: torch.from_numpy(g_["%d/%s" % (D, k)]).to(DEV)          # noqa: E731
    p = t("p")
    g, state = hip_grad(D, p, t("agent"), t("replay"), t("demo"), t("stats_agent"), t("stats_replay"), t("stats_demo"))
    xa, xd = torch.cat([t("xn_agent"), t("xn_replay")]), t("xn_demo")
    names = ["total", "pred", "disc_logit_loss", "disc_grad_penalty", "weight_decay_sum", "agent_logit_mean", "demo_logit_mean", "agent_acc",
             "demo_acc"]
    v64 = torch.tensor([float(g_["%d/val64_%s" % (D, k)].reshape(-1)[0]) for k in names], dtype=torch.float64, device=DEV)
    check_grad(D, p, g, state, xa, xd, t("grad64"), v64, t("grad32"))


def reward_bound(l64, r64, lb, scale):
    """|disc_r(fp32) - disc_r(float64)| for a logit off by at most lb: the slope scale * sigmoid, the fp32 rounding of p, of 1 - p (which
    cancels as p nears 1, up to the 1e-4 floor) and of logf."""
    p = torch.sigmoid(l64)
    return 2 * scale * (p * lb + 4 * U * p / torch.clamp(1 - p, min=1e-4) + 2 * U + 2 * U * r64.abs() / scale)


@pytest.mark.parametrize("case", ["34", "68", "probe"])
def test_reward_against_the_references_float64(case, fixture):
    """dwd_reward on the fixture's raw rows and eval-mode statistics against the reference's float64 _calc_disc_rewards / _combine_rewards.
    The probe network's logits are exact (4 x_0), so there only the reward formula's rounding is allowed."""
    pre = "probe_" if case == "probe" else case + "/reward_"
    out = "probe_" if case == "probe" else case + "/"
    D = 34 if case == "probe" else int(case)
    t = lambda k: torch.from_numpy(fixture[k]).to(DEV)          # noqa: E731
    p = torch.from_numpy(T.reward_params(fixture, case)).to(DEV)
    st, x, task = t(pre + "stats"), t(pre + "x"), t(pre + "task")
    B = x.shape[0]
    dr, comb, lg = (torch.full((B,), float("nan"), device=DEV) for _ in range(3))
    rc = api()["reward"](p.data_ptr(), st.data_ptr(), x.data_ptr(), task.data_ptr(), B, D, REWARD["scale"], REWARD["task_w"], REWARD["disc_w"],
                         dr.data_ptr(), comb.data_ptr(), lg.data_ptr(), stream())
    assert rc == 0
    torch.cuda.synchronize()
    l64, r64, c64 = t(pre + "logit64"), t(out + "disc_r64"), t(out + "combined64")
    xn = t(pre + "xn")
    lb = 2 * (D + 2 * T.HID + 8) * U * T.logits(p.abs(), D, xn.abs(), torch.float64)          # abs_logit64
    if case == "probe":
        assert torch.equal(lg.double(), l64)
        lb = torch.zeros_like(lb)
    assert bool(((lg.double() - l64).abs() <= lb).all())
    rb = reward_bound(l64, r64, lb, REWARD["scale"])
    assert bool(((dr.double() - r64).abs() <= rb).all()), float(((dr.double() - r64).abs() / rb).max())
    cb = REWARD["disc_w"] * rb + 2 * U * (REWARD["task_w"] * task.double().abs()[:, 0] + REWARD["disc_w"] * r64.abs())
    assert bool(((comb.double() - c64).abs() <= cb).all()), float(((comb.double() - c64).abs() / cb).max())


# ----------------------------------------------------------------------------------------------------- dwd_grad over its shapes
def stats_snapshot(rng, D, shift):
    return torch.from_numpy(np.concatenate([rng.normal(size=D) * 0.4 + shift, rng.uniform(0.3, 2.5, size=D), [3000.0]])).to(DEV)


def rows_of(rng, n, D, shift):
    if n == 0:
        return None
    x = rng.normal(size=(n, D)) * 1.3 + shift
    x[: max(1, n // 50)] *= 30.0          # rows clamped at +-5 after the normalisation
    return torch.from_numpy(x.astype(np.float32)).to(DEV)


def lively_p(rng, D):
    """Weights about twice the initial scale, non-zero biases, four dead units in each hidden layer (pre-activation exactly 0)."""
    W1 = rng.uniform(-2, 2, size=(T.HID, D)) / np.sqrt(D)
    W2 = rng.uniform(-2, 2, size=(T.HID, T.HID)) / 16
    b1, b2 = rng.uniform(-0.2, 0.2, size=T.HID), rng.uniform(-0.2, 0.2, size=T.HID)
    W1[:4], b1[:4], W2[:4], b2[:4] = 0, 0, 0, 0
    return torch.from_numpy(np.concatenate([W1.ravel(), b1, W2.ravel(), b2, rng.uniform(-1, 1, size=T.HID), [0.3]]).astype(np.float32)).to(DEV)


def grad_case(D, na, nr, nd, seed):
    rng = np.random.default_rng(seed)
    p = lively_p(rng, D)
    a, r, d = rows_of(rng, na, D, -0.3), rows_of(rng, nr, D, 0.0), rows_of(rng, nd, D, 0.4)
    sa, sr, sd = stats_snapshot(rng, D, -0.1), stats_snapshot(rng, D, 0.0), stats_snapshot(rng, D, 0.1)
    g, state = hip_grad(D, p, a, r, d, sa if na else None, sr if nr else None, sd)
    empty = torch.zeros(0, D, device=DEV)
    an = empty if a is None else T.normalise(a, sa, D)
    rn = empty if r is None else T.normalise(r, sr, D)
    dn = T.normalise(d, sd, D)
    g64, v64 = T.loss_grad(p.double(), D, an, rn, dn, torch.float64)
    g32, _ = T.loss_grad(p, D, an, rn, dn, torch.float32)
    check_grad(D, p, g, state, torch.cat([an, rn]), dn, g64, v64, g32)


@pytest.mark.parametrize("D", [34, 68, 340])
@pytest.mark.parametrize("rows", [(700, 600, 747), (700, 600, 748), (21845, 21845, 21845), (21845, 21845, 21846)],
                         ids=["R2047", "R2048", "R65535", "R65536"])
def test_grad_across_the_slab_switches(D, rows):
    """R = 2047 / 2048 (one slab / two) and 65 535 / 65 536 (63 / 64 slabs); none of the counts a multiple of 128, most not of 4 or 64."""
    grad_case(D, *rows, seed=D * 7 + rows[2])


@pytest.mark.parametrize("D,rows", [(68, (1000, 1001, 1)), (34, (0, 517, 389)), (340, (611, 0, 259)), (68, (131, 67, 5)),
                                    (340, (3, 2, 2))], ids=["one_demo_row", "no_agent_rows", "no_replay_rows", "odd_rows", "tiny"])
def test_grad_at_the_row_edges(D, rows):
    grad_case(D, *rows, seed=sum(rows) + D)


def test_grad_at_the_yaml_minibatch_against_float64():
    """amp_minibatch_size 131 072 of cfg/train/TocabiAMPLowerPPO.yaml with numAMPObsSteps 2: 3 x 131 072 rows at D = 68, the capped 64-slab
    split (kc = 6144) and 256 column-sum slabs."""
    grad_case(68, 131072, 131072, 131072, seed=131072)


# ----------------------------------------------------------------------------------------------------- dwd_stats
@pytest.mark.parametrize("D", [34, 340])
@pytest.mark.parametrize("B", [2, 3, 1023, 131072])
def test_stats_against_float64_two_pass(D, B):
    """The RunningMeanStd update against float64 two-pass batch moments combined with the same parallel formula; a column with mean 300
    and spread 0.05 (the one-pass sums cancel), a constant column; stats_out == stats_in.  Bound: the one-pass sums' chain of
    ceil(B / 1024) + 1024 float64 roundings on sums of |x| and x^2."""
    rng = np.random.default_rng(B + D)
    x = rng.normal(size=(B, D)) * rng.uniform(0.1, 3, size=D) + rng.normal(size=D) * 2
    x[:, 1] = 300.0 + 0.05 * rng.normal(size=B)
    x[:, D - 1] = 0.7
    x = torch.from_numpy(x.astype(np.float32)).to(DEV)
    st = torch.from_numpy(np.concatenate([rng.normal(size=D), rng.uniform(0.5, 2, size=D), [1000.0 if B > 2 else AD.RMS_EPS]])).to(DEV)
    st[1], st[D + 1] = 299.0, 0.01
    work = torch.full((api()["stats_workspace_bytes"](D) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    s0 = st.clone()
    assert api()["stats"](x.data_ptr(), B, D, st.data_ptr(), st.data_ptr(), work.data_ptr(), stream()) == 0          # in place
    torch.cuda.synchronize()
    xd = x.double()
    bm = xd.mean(0)
    bv = ((xd - bm) ** 2).sum(0) / (B - 1)
    m, v, n = AD.RunningMeanStd.combine(s0[:D], s0[D:2 * D], s0[2 * D], bm, bv, B)
    k = (B + 1023) // 1024 + 1024 + 8
    e = 2.0 ** -53
    tol_m = 4 * k * e * (xd.abs().mean(0) + s0[:D].abs()) + 1e-300
    tol_v = 4 * k * e * ((xd ** 2).sum(0) / (B - 1) + s0[D:2 * D] + (bm - s0[:D]) ** 2 + s0[:D] ** 2) + 1e-300
    assert bool(((st[:D] - m).abs() <= tol_m).all()), float(((st[:D] - m).abs() / tol_m).max())
    assert bool(((st[D:2 * D] - v).abs() <= tol_v).all()), float(((st[D:2 * D] - v).abs() / tol_v).max())
    assert float(st[2 * D]) == float(n)
