"""The fused PPO update (isaacgymdyros_amd/ppo_update.py, csrc/dw_ppo.hip) at the small and odd minibatch sizes a debugging run lands on, stage by
stage against the float64 restatement tests/ppo_update_truth.py with the error bounds derived there (tests/test_ppo_update_truth.py holds that
restatement to float64 autograd).  Every case builds one FusedPpoUpdate over NMB = 3 minibatches and runs FOUR updates: the minibatch index
visits 1 and 2 and wraps to 0.  The loss scale starts at 16 B -- per sample the scale / B = 16 of tests/test_ppo_gpu.py's 65536 / 4096 -- so
that no case overflows fp16 by its size alone (the overflow paths are test_loss_edges').

A line `ppo-edges ...` per case reports the worst error of each stage as a fraction of its bound (pytest -s shows them).  Measured on an
MI355X: the fp16-stored stages sit where half an ulp puts them (dz2 0.995 .. 0.997 at every size, the library-GEMM form's fp16 weight gradients
0.96 .. 0.997), the fp32-stored ones far inside (a slab's partial weight gradient at most 0.117, bias gradients 0.011); no sample was left out."""
import math

import pytest
import torch

import ppo_update_truth as T

PPO = T.consumer()
C = dict(PPO.TRAIN_CFG["config"])
DEV = "cuda:0"
LR = (3e-5, 5e-5)
UPDATES = 4
MFMA_SIZES = list(T.edge_sizes())
LEFT_OUT = set()          # (case, minibatch, row) of every sample left out for sitting on the clip boundary: two over the whole module at most


def _build(U, B, seed, scale=None, guard=False, **kw):
    """(fused, net, batch on the GPU) from tests/ppo_update_truth.make_case.  guard: the batch tensors carry one more row than the NMB * B the update
    is bound to, filled with a sentinel."""
    net, batch = T.make_case(PPO, T.NMB * B, seed)
    net = net.to(DEV)
    fused = U.FusedPpoUpdate(net, C, B, T.NMB, DEV, **kw)
    fused.set_learning_rates(*LR)
    fused.state[U.K["DWP_S_SCALE"]] = 16.0 * B if scale is None else scale
    whole = []
    for t in batch:
        w = torch.full((t.shape[0] + 1,) + tuple(t.shape[1:]), 7.0e4, device=DEV) if guard else torch.empty_like(t, device=DEV)
        w[:t.shape[0]] = t.to(DEV)
        whole.append(w)
    batch = [w[:T.NMB * B] for w in whole]
    fused.bind_batch(*batch)
    return fused, net, batch, whole


def _frac(got, t, bound):
    """max |got - t| / bound over the entries (both finite everywhere: these cases do not overflow)."""
    got = T.f64(got)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(t).all())
    return float(((got - t).abs() / bound).max())


def _snapshot(U, f):
    st = f.state.cpu().tolist()
    return {"W": {k: t.clone() for k, t in f.views16.items()}, "p": f.p.clone(), "m": f.m.clone(), "v": f.v.clone(), "scale": st[U.K["DWP_S_SCALE"]],
            "growth": st[U.K["DWP_S_GROWTH"]], "steps": [int(st[U.K["DWP_S_STEP"]]), int(st[U.K["DWP_S_STEP"] + 1])], "mb": int(st[U.K["DWP_S_MB"]])}


def _check_gradients(U, case, f, net, batch, snap, worst, left_out=None, sharded=False):
    """The forward-to-gradient half of one update of `f`, already run and synchronised, against the helper: every stage from the operands the
    kernels had, up to the slabs' partial weight gradients and the bias gradients.  Returns (the summed weight gradients by layer, the bias
    gradients' (truth, bound) by layer, the (dz, activation) pairs of the three layers).  left_out: the module's set of samples left out for
    sitting on the clip boundary (tests/test_ppo_sharded_gpu.py keeps its own, with the same caps).  sharded: dwp_grad_bucket took the bias
    gradients out of pbuf instead of dwp_grad_stats, so gb holds none (that file holds them in the bucket)."""
    B, gemm = f.B, not f.mfma
    left_out = LEFT_OUT if left_out is None else left_out
    mb, scale, W = snap["mb"], snap["scale"], snap["W"]
    sl = slice(mb * B, (mb + 1) * B)
    obs, act, nlp_old, mu_old, adv, ret = (t[sl] for t in batch)
    lg = f.logged().cpu().tolist()
    assert lg[6] == scale

    def note(name, got, t, bound):
        fr = _frac(got, t, bound)
        worst[name] = max(worst.get(name, 0.0), fr)
        assert fr <= 1.0, (case, mb, name, fr)

    # ---- forward
    assert torch.equal(f.x16[:, :T.IN], obs.half()) and float(f.x16[:, T.IN:].abs().max()) == 0.0
    assert float(W["W1"][:, :, T.IN:].abs().max()) == 0.0 and float(W["W3"][0, T.ACT:].abs().max()) == 0.0 and float(W["W3"][1, 1:].abs().max()) == 0.0
    t, bound = T.linear(f.x16[:, :T.IN], W["W1"][:, :, :T.IN], W["b1"], double_rounded=gemm)
    note("h1", f.h1, torch.relu(t), bound)
    t, bound = T.linear(f.h1, W["W2"], W["b2"], double_rounded=gemm)
    note("h2", f.h2, torch.relu(t), bound)
    t, bound = T.linear(f.h2, W["W3"], W["b3"], double_rounded=gemm)
    note("out", f.out, t, bound)
    assert float(f.out[0, :, T.ACT:].abs().max()) == 0.0 and float(f.out[1, :, 1:].abs().max()) == 0.0
    # ---- the loss on the heads' outputs as stored
    L = T.loss(f.out, act, nlp_old, mu_old, adv, ret, net.sigma, scale, C["e_clip"], C["critic_coef"])
    near = (L["margin"].abs() < T.CLIP_MARGIN).nonzero().reshape(-1).tolist()
    for r in near:
        left_out.add((case, mb, r))
    assert len([k for k in left_out if k[0] == case]) <= 1 and len(left_out) <= 2, sorted(left_out)
    keep = torch.ones(B, dtype=torch.bool)
    keep[near] = False
    assert lg[0] == pytest.approx(float(L["a_loss"]), rel=1e-5, abs=1e-6) and lg[1] == pytest.approx(float(L["c_loss"]), rel=1e-5)
    assert lg[2] == pytest.approx(float(L["b_loss"]), rel=1e-5) and lg[4] == pytest.approx(float(L["kl"]), rel=1e-4)
    assert lg[3] == pytest.approx(float(L["clip_frac"]), abs=(0.5 + len(near)) / B)
    note("dmu", f.dout[0, :, :T.ACT][keep.to(DEV)], L["dmu"][keep], L["dmu_bound"][keep])
    note("dvalue", f.dout[1, :, 0], L["dvalue"], L["dvalue_bound"])
    assert float(f.dout[0, :, T.ACT:].abs().max()) == 0.0 and float(f.dout[1, :, 1:].abs().max()) == 0.0
    # ---- backward: input gradients with the kernels' own relu masks, weight gradients per slab and summed, bias gradients
    t, bound = T.linear(f.dout, W["W3"].transpose(1, 2))
    note("dz2", f.dh2, T.masked(t, f.h2), bound)
    assert float(f.dh2[f.h2 <= 0].abs().max()) == 0.0
    t, bound = T.linear(f.dh2, W["W2"].transpose(1, 2))
    note("dz1", f.dh1, T.masked(t, f.h1), bound)
    assert float(f.dh1[f.h1 <= 0].abs().max()) == 0.0
    x2 = f.x16.unsqueeze(0).expand(2, B, T.INP)
    pairs = (("W1", f.dh1, x2), ("W2", f.dh2, f.h1), ("W3", f.dout, f.h2))
    if gemm:
        g_own = {}
        for name, dz, a in pairs:
            g, S = T.wgrad(dz, a)
            g_own[name] = f.gviews[name]
            note("g" + name, g_own[name], g, T.wgrad_fp16_bound(g, S, B))
    else:
        nk = T.slab_nk(B)
        g32 = f.g32
        gsum = ((g32[0] + g32[1]) + g32[2]) + g32[3]          # (dwp_grad_stats' and dwp_adam's order, in fp32)
        g_own = {}
        for name, dz, a in pairs:
            o, n, shape = f._gshape[name]
            slabs = g32[:, o:o + n].view((T.WG_SLABS,) + shape)
            for s in range(T.WG_SLABS):
                if nk[s] == 0:
                    assert float(slabs[s].abs().max()) == 0.0, (case, name, s)
            fr = T.worst_slab_fraction(slabs, dz, a)
            worst["g%s/slab" % name] = max(worst.get("g%s/slab" % name, 0.0), fr)
            assert fr <= 1.0, (case, mb, name, fr)
            g, S = T.wgrad(dz, a)
            g_own[name] = gsum[o:o + n].view(shape)
            note("g" + name, g_own[name], g, torch.clamp(T.wgrad_sum_bound(S, B), min=1e-300))
        assert float(f.pbuf.abs().max()) == 0.0          # (all 32 buckets of both nets: summed and cleared, also those no workgroup wrote)
    assert float(g_own["W1"][:, :, T.IN:].abs().max()) == 0.0 and float(g_own["W3"][0, T.ACT:].abs().max()) == 0.0 and float(g_own["W3"][1, 1:].abs().max()) == 0.0
    gb = [T.bgrad(dz) for dz in (f.dh1, f.dh2, f.dout)]
    if not gemm and not sharded:          # (dwp_grad_stats leaves the buckets' sums in gb; the library-GEMM form's dwp_finish clears it: its biases are held by m, v, p below)
        o = 0
        for name, (t, bound) in zip(("gb1", "gb2", "gb3"), gb):
            got = f.gb[o:o + t.numel()].view(t.shape)
            note(name, got, t, torch.clamp(bound, min=1e-300))
            o += t.numel()
    return g_own, gb, [(dz, a) for _, dz, a in pairs]


def _check_update(U, case, f, net, batch, snap, worst):
    """One update of `f`, already run and synchronised, against the helper: every stage from the operands the kernels had."""
    g_own, gb, _ = _check_gradients(U, case, f, net, batch, snap, worst)
    # ---- unscale, clip, Adam, scaler: from the gradients in the fused buffers (bias gradients: the column sums)
    gfull = T.flat(g_own["W1"], g_own["W2"], g_own["W3"], gb[0][0], gb[1][0], gb[2][0])
    _check_tail(U, f, snap, gfull)          # (these cases are sized not to overflow)


def _check_tail(U, f, snap, gfull, found=(False, False)):
    """The second half of one update of `f`: unscale, clip, Adam and the scaler from the still-scaled gradient `gfull` (the layout of
    ppo_update_truth.flat) and the snapshot taken before the update.  found: what unscale_'s found_inf must come to, [actor, critic]."""
    K, mb, scale = U.K, snap["mb"], snap["scale"]
    lg = f.logged().cpu().tolist()
    R = T.clip_adam(gfull, scale, snap["p"], snap["m"], snap["v"], snap["steps"], LR, C["grad_norm"])
    assert R["found"] == list(found) and lg[7] == float(any(found)) and lg[6] == scale
    if math.isfinite(R["norm"]):
        assert lg[5] == pytest.approx(R["norm"], rel=1e-4)
    else:
        assert not math.isfinite(lg[5])          # (a non-finite word of the actor's: the logged norm says so too)
    m, v, p = T.f64(f.m), T.f64(f.v), T.f64(f.p)
    assert float((m - R["m"]).abs().max()) <= 1e-5 * float(R["m"].abs().max()) + 1e-12
    assert float((v - R["v"]).abs().max()) <= 1e-4 * float(R["v"].abs().max()) + 1e-20
    assert float((p - R["p"]).abs().max()) <= 0.02 * LR[0]
    assert torch.equal(f.p16, f.p.half())
    st = f.state.cpu().tolist()
    new_scale, new_growth = T.scaler_update(scale, snap["growth"], any(R["found"]))
    assert st[K["DWP_S_SCALE"]] == new_scale and st[K["DWP_S_GROWTH"]] == new_growth
    assert [st[K["DWP_S_STEP"]], st[K["DWP_S_STEP"] + 1]] == R["steps"] and st[K["DWP_S_MB"]] == (mb + 1) % T.NMB
    assert st[:8] == [0.0] * 8          # (the logged sums and the flags: cleared for the next update)
    assert float(f.views["W3"][0, T.ACT:].abs().max()) == 0.0 and float(f.views["W3"][1, 1:].abs().max()) == 0.0 and float(f.views["b3"][0, T.ACT:].abs().max()) == 0.0
    assert float(f.views["b3"][1, 1:].abs().max()) == 0.0 and float(f.views["W1"][:, :, T.IN:].abs().max()) == 0.0


def _report(case, worst):
    print("ppo-edges %s: " % case + ", ".join("%s %.3f" % (k, x) for k, x in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("B", MFMA_SIZES, ids=["B%d_nk%s" % (B, "-".join(map(str, T.slab_nk(B)))) for B in MFMA_SIZES])
def test_matrix_core_form_stage_by_stage_at_the_ring_and_bucket_edges(B):
    """dwp_mlp | dwp_wgrad | dwp_grad_stats | dwp_adam_finish with rowmajor=True at the sizes of ppo_update_truth.edge_sizes (per size the k-steps
    of dwp_wgrad's four slabs, in the test's id): every stage within its derived bound, the partial gradient of an empty slab exactly zero, every
    slab's partial gradient the product over that slab's rows, all 32 accumulator buckets zero afterwards, padding zero, minibatch index, step
    counts and scaler words as the helper has them, p16 the rounded masters.  Logged scalars and m, v, p: the tolerances of
    tests/test_ppo_gpu.py::test_fused_update_piece_by_piece_against_torch, against float64.
    Samples left out of the dmu / clip-fraction comparison for sitting within 1e-5 of the clip boundary: none expected (seeds 1000 + B: the update
    emulated on the CPU brings none that close in four updates, tests/test_ppo_update_truth.py); the cap of one per case, two in all, is asserted."""
    from isaacgymdyros_amd import ppo_update as U
    case = "mfma%d" % B
    f, net, batch, _ = _build(U, B, T.case_seed("mfma", B))
    assert f.mfma and f.rowmajor
    worst, mbs = {}, []
    for _ in range(UPDATES):
        snap = _snapshot(U, f)
        mbs.append(snap["mb"])
        f.update()
        torch.cuda.synchronize()
        _check_update(U, case, f, net, batch, snap, worst)
    assert mbs == [0, 1, 2, 0] and f.state[U.K["DWP_S_STEP"]:U.K["DWP_S_STEP"] + 2].tolist() == [4.0, 4.0]
    _report(case, worst)


GUARD16 = -7.0


def _guarded(t):
    """The same tensor with HID more words behind it that hold a sentinel: (view of t's shape, the guard words)."""
    flat = torch.full((t.numel() + T.HID,), GUARD16 if t.dtype == torch.float16 else 7.0e4, dtype=t.dtype, device=t.device)
    flat[:t.numel()] = t.reshape(-1)
    return flat[:t.numel()].view(t.shape), flat[t.numel():]


@pytest.mark.gpu
@pytest.mark.parametrize("mfma,B", [(False, B) for B in T.GEMM_SIZES] + [(True, 100)], ids=["gemm%d" % B for B in T.GEMM_SIZES] + ["mfma_asked100"])
def test_library_gemm_form_stage_by_stage_at_sizes_off_its_blocks(mfma, B):
    """The seventeen-launch form where dwp_loss's 64-sample blocks, dwp_relu_bwd's 64-row blocks and dwp_stage_obs's flat bound end inside a block:
    B = 1, 63, 65, 100 -- and mfma=True at B = 100, which is no multiple of 32 and must run this form.  Stage by stage as above, with the
    two roundings of product and bias in the bound.  Nothing is read or written past row B: the batch tensors and every activation / gradient
    buffer carry guard words behind their last row that still hold their sentinel afterwards (a guard row that was read would also show: 7e4 is
    inf in fp16).  Samples left out for sitting on the clip boundary: none expected (seeds 2000 + B), as above."""
    from isaacgymdyros_amd import ppo_update as U
    case = "gemm%d%s" % (B, "m" if mfma else "")
    f, net, batch, whole = _build(U, B, T.case_seed("gemm", B), guard=True, mfma=mfma)
    assert f.mfma is False and f.rowmajor
    guards = {}
    for name in ("x16", "h1", "h2", "out", "dout", "dh2", "dh1"):
        view, guards[name] = _guarded(getattr(f, name))
        setattr(f, name, view)
    worst, mbs = {}, []
    for _ in range(UPDATES):
        snap = _snapshot(U, f)
        mbs.append(snap["mb"])
        f.update()
        torch.cuda.synchronize()
        _check_update(U, case, f, net, batch, snap, worst)
        for name, gd in guards.items():
            assert bool((gd == GUARD16).all()), (case, name)
        for w in whole:
            assert bool((w[T.NMB * B] == 7.0e4).all())
    assert mbs == [0, 1, 2, 0] and f.state[U.K["DWP_S_STEP"]:U.K["DWP_S_STEP"] + 2].tolist() == [4.0, 4.0]
    _report(case, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("obs16", [False, True], ids=["fp32_obs", "fp16_obs"])
@pytest.mark.parametrize("B", [32, 160, 1056])
def test_trainers_form_equals_its_rowmajor_twin(B, obs16):
    """rowmajor=False -- what examples/ppo_consumer.py builds: dwp_mlp writes the operand-order copies only and masks dz1 without the row-major
    image's barrier -- with fp32 observations and with the fp16 [rows, 512] batch, against a rowmajor=True twin (fp32 observations) started from the
    same parameters before each update: out, dout, the slabs' partial gradients, the weights' part of p / m / v / p16, both operand-order copies
    and the scaler's words are the same bits; bias gradients differ by the order of their fp32 atomic adds (each within (B + 32) u32 sum |.| of
    the truth, so twice that apart), and m / v / p of the biases by what that does to them."""
    from isaacgymdyros_amd import ppo_update as U
    K = U.K
    seed = T.case_seed("mfma", B)
    fa, _, batch, _ = _build(U, B, seed)
    fb, _, _, _ = _build(U, B, seed, rowmajor=False)
    assert fa.rowmajor and not fb.rowmajor and fb.mfma
    if obs16:
        o16 = torch.zeros(T.NMB * B, T.INP, device=DEV, dtype=torch.float16)
        o16[:, :T.IN] = batch[0].half()
        fb.bind_batch(o16, *batch[1:])
    nw = T.NWT
    scaler = [K["DWP_S_FOUND_INF"], K["DWP_S_FOUND_INF"] + 1, K["DWP_S_SCALE"], K["DWP_S_GROWTH"], K["DWP_S_STEP"], K["DWP_S_STEP"] + 1, K["DWP_S_MB"], K["DWP_S_G16"]]
    for it in range(UPDATES):
        with torch.no_grad():
            fb.p.copy_(fa.p); fb.m.copy_(fa.m); fb.v.copy_(fa.v); fb.p16.copy_(fa.p16); fb.p16t.copy_(fa.p16t); fb.p32f.copy_(fa.p32f)
        scale = float(fa.state[K["DWP_S_SCALE"]])
        fa.update(); fb.update()
        torch.cuda.synchronize()
        for name in ("out", "dout", "g32", "p16t", "p32f"):
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
        for name in ("p", "m", "v", "p16"):
            assert torch.equal(getattr(fa, name)[:nw], getattr(fb, name)[:nw]), (it, name)
        assert torch.equal(fa.state[scaler], fb.state[scaler]) and fa.logged()[7].item() == 0.0
        assert torch.allclose(fa.logged()[:6], fb.logged()[:6], rtol=1e-5, atol=1e-7)
        assert float(fb.pbuf.abs().max()) == 0.0
        for name in ("x16", "h1", "h2", "dh2", "dh1"):          # (the trainer's form leaves the row-major images alone)
            assert float(getattr(fb, name).abs().max()) == 0.0, name
        # biases
        E = 2.0 * torch.cat([T.bgrad(dz)[1].reshape(-1) for dz in (fa.dh1, fa.dh2, fa.dout)])
        dg = T.f64(fa.gb - fb.gb).abs()
        assert bool((dg <= E).all()), (it, float((dg / torch.clamp(E, min=1e-300)).max()))
        g = T.f64(fa.gb).abs() / scale
        e = E / scale          # (unscaled; the actor's clip coefficient is at most 1)
        dm, dv = T.f64(fa.m[nw:] - fb.m[nw:]).abs(), T.f64(fa.v[nw:] - fb.v[nw:]).abs()
        assert bool((dm <= 0.1 * e + 8 * T.U32 * (T.f64(fa.m[nw:]).abs() + g)).all())
        assert bool((dv <= 0.001 * (2 * g * e + e * e) + 8 * T.U32 * (T.f64(fa.v[nw:]).abs() + g * g)).all())
        assert float((fa.p[nw:] - fb.p[nw:]).abs().max()) <= 1e-7          # (as every twin comparison of tests/test_ppo_gpu.py holds the biases)
    assert fa.state[K["DWP_S_STEP"]:K["DWP_S_STEP"] + 2].tolist() == [4.0, 4.0] and float(fa.state[K["DWP_S_MB"]]) == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("mfma", [True, False], ids=["mfma", "gemm"])
def test_loss_edges_zero_advantages_and_an_overflow_in_the_actor_only(mfma):
    """B = 64.  Rows whose advantage is exactly zero (either sign of zero): s1 == sc, the tie weights 0.5 + 0.5 apply and their dmu rows are
    exactly zero; a_loss matches the helper.  One row of minibatch 0 whose old_nlp - nlp exceeds log(FLT_MAX): its ratio is inf, dnlp =
    A * inf * 0 = NaN (autograd's exp backward gives the same: tests/test_ppo_update_truth.py) -- GradScaler's contract for the OTHER net than
    tests/test_ppo_gpu.py::test_fused_update_skips_and_backs_off_on_overflow poisons: the actor's step is skipped, the critic's is taken, the scale
    halves; the next, clean minibatch steps both."""
    from isaacgymdyros_amd import ppo_update as U
    K, B = U.K, 64
    net, batch = T.make_case(PPO, T.NMB * B, 3064)
    batch = [t.clone() for t in batch]
    zero = [2, 17, 40, B + 1, B + 33, B + 63]
    batch[4][zero] = 0.0
    batch[4][[17, B + 33]] = -0.0
    poison = 9
    batch[2][poison], batch[4][poison] = 1000.0, 1.0
    net = net.to(DEV)
    f = U.FusedPpoUpdate(net, C, B, T.NMB, DEV, mfma=mfma)
    f.set_learning_rates(*LR)
    f.state[K["DWP_S_SCALE"]] = 16.0 * B
    batch = [t.to(DEV) for t in batch]
    f.bind_batch(*batch)
    mask = T.actor_mask().to(DEV)
    for mb, (skipped, steps, scale_after) in enumerate(((1.0, [0.0, 1.0], 8.0 * B), (0.0, [1.0, 2.0], 8.0 * B))):
        p0, scale = f.p.clone(), float(f.state[K["DWP_S_SCALE"]])
        f.update()
        torch.cuda.synchronize()
        sl = slice(mb * B, (mb + 1) * B)
        lg = f.logged().cpu().tolist()
        L = T.loss(f.out, *(t[sl] for t in batch[1:]), net.sigma, scale, C["e_clip"], C["critic_coef"])
        rows = [z - mb * B for z in zero if mb * B <= z < (mb + 1) * B]
        assert len(rows) == 3 and float(L["dmu"][rows].abs().max()) == 0.0 and float(f.dout[0, rows].abs().max()) == 0.0
        assert lg[0] == pytest.approx(float(L["a_loss"]), rel=1e-5, abs=1e-6) and lg[1] == pytest.approx(float(L["c_loss"]), rel=1e-5)
        assert lg[7] == skipped and lg[6] == scale and float(f.state[K["DWP_S_SCALE"]]) == scale_after
        assert f.state[K["DWP_S_STEP"]:K["DWP_S_STEP"] + 2].tolist() == steps
        moved = f.p != p0
        assert bool((moved & ~mask).any()) and bool((moved & mask).any()) == (skipped == 0.0)
        if mb == 0:
            assert math.isinf(float(L["ratio"][poison])) and not bool(torch.isfinite(L["dmu"][poison]).any())
            assert not bool(torch.isfinite(f.dout[0, poison, :T.ACT].float()).any()) and bool(torch.isfinite(f.dout[1].float()).all())
            keep = torch.arange(B) != poison
            assert bool(torch.isfinite(f.dout[0][keep.to(DEV)].float()).all())
        else:
            assert bool(torch.isfinite(f.dout.float()).all())
        assert bool(torch.isfinite(f.p).all()) and torch.equal(f.p16, f.p.half())
        if f.mfma:
            assert float(f.pbuf.abs().max()) == 0.0          # (the NaN the poisoned row left in a bucket is gone with the rest)
