"""The sharded form of the fused PPO update (isaacgymdyros_amd/ppo_update.py `collective=True`, csrc/dw_ppo.hip k_grad_bucket, k_grad_stats<1>,
k_adam<., 1>) at world > 1, with the ranks emulated in ONE process on one GPU: the kernels do not care which process wrote the bucket.  R
FusedPpoUpdate objects with the same initial weights each take their own rows of one case (tests/ppo_update_truth.make_case); one emulated
update is every rank's update_head(), the fp32 sum ((b_0 + b_1) + b_2) + ... of their buckets formed by torch in the all-reduce's place and
copied into every rank's bucket, then every rank's update_tail().  Truth and bounds: tests/ppo_update_truth.py (`rank_bucket`, `bucket_sum`),
which tests/test_ppo_update_truth.py holds to float64 autograd on examples/ppo_consumer.py's loss functions.  The forward-to-gradient checks
of every rank are tests/test_ppo_edges_gpu._check_gradients, the tail's are its _check_tail.

Not run here, because they need several GPUs: RCCL itself, the collective captured inside a hipGraph, the capture fall-back when ranks
disagree, and any broadcast of parameters.

The per-sample loss scale is 16 on every learner (rank: 16 B_r / B_r; the unsharded learner over the union: 16 R B_r / (R B_r)), and the
kernels' fl(scale * fl(1 / B)) is exactly 16.0f at every size used (asserted): a row's activations and gradients then do not depend on
which learner holds it, which is what `rows` below compares bit for bit.

A line `ppo-sharded <case>: <stage> <worst fraction of its bound>, ...` per case (pytest -s).  Measured on an MI355X, worst over a case's
four updates and all its ranks (R2_B32 | R2_B160 | R3_B32 | R3_B160 | R8_B32):
  a rank's bucket, weights (`bucketW`)          0.091 | 0.020 | 0.114 | 0.025 | 0.098      (1 / 3 rounds: the two R3 cases sit a little higher)
  a rank's bucket, biases (`bucketb`)           0.011 | 0.004 | 0.030 | 0.007 | 0.015
  the buckets' sum, unscaled (`sum`)            0.094 | 0.017 | 0.101 | 0.017 | 0.076
  the unsharded learner's gradient (`big`)      0.052 | 0.009 | 0.035 | 0.006 | 0.012
  the ranks' own stages as in tests/test_ppo_edges_gpu.py: the fp16-stored ones where half an ulp puts them (dz2 0.993 .. 0.997, dvalue 0.933 ..
  0.975, h2 0.885 .. 0.916), a slab's partial weight gradient at most 0.110, the summed weight gradients at most 0.101.
Every bit-for-bit comparison held: the bucket's weight words, the rows of the ranks against the unsharded learner's at R = 2, 3 and 8, and
the ranks against each other after every update.  No sample was left out for sitting on the clip boundary."""
import copy
import math

import pytest
import torch

import ppo_update_truth as T
import test_ppo_edges_gpu as G

PPO, C, DEV, LR = G.PPO, G.C, G.DEV, G.LR
UPDATES = 4
WORLDS = [(2, 32), (2, 160), (3, 32), (3, 160), (8, 32)]          # (ranks, rank minibatch): 1 / 2 exact, 1 / 3 rounds, 8 = a node; one workgroup / uneven slabs
LEFT_OUT = set()          # as tests/test_ppo_edges_gpu.LEFT_OUT, for this module's cases: one per case, two in all, at the most
NAMES = ("p", "m", "v", "p16", "p16t", "p32f")
ROWS = ("x16", "h1", "h2", "out", "dout", "dh2", "dh1")
PB_ST = 2 * T.HID + T.OUTP          # csrc/dw_ppo.hip: a row of pbuf is b1 | b2 | b3 columns, then the logged sums


def _seed(R, B):
    return 5000 + 8 * B + R


def _per_sample_scale(scale, B):
    """The kernels' fl(scale * fl(1 / B)) (csrc/dw_ppo.hip: `scale * invB`, invB = 1.0f / (float)B)."""
    f32 = lambda x: torch.tensor(float(x), dtype=torch.float32)          # noqa: E731
    return float(f32(scale) * (f32(1.0) / f32(B)))


def _ranks(U, R, B, seed, edit=None, **kw):
    """R ranks over one case of R * NMB * B rows; rank r binds rows [r NMB B, (r + 1) NMB B).  Returns (ranks, their nets, their batches on the
    GPU, the common initial net, the whole batch on the CPU).  edit: a function that changes the whole batch (a list of tensors) in place."""
    net, batch = T.make_case(PPO, R * T.NMB * B, seed)
    batch = [t.clone() for t in batch]
    if edit is not None:
        edit(batch)
    net = net.to(DEV)
    fs, nets, batches = [], [], []
    for r in range(R):
        rows = slice(r * T.NMB * B, (r + 1) * T.NMB * B)
        nr = copy.deepcopy(net)
        f = U.FusedPpoUpdate(nr, C, B, T.NMB, DEV, collective=True, **kw)
        f.set_learning_rates(*LR)
        f.state[U.K["DWP_S_SCALE"]] = 16.0 * B
        f.world = R          # (update_head reads it at each call; allreduce() is never called here: it would reach for torch.distributed)
        b = [t[rows].to(DEV).contiguous() for t in batch]
        f.bind_batch(*b)
        fs.append(f); nets.append(nr); batches.append(b)
    assert _per_sample_scale(16.0 * B, B) == 16.0
    return fs, nets, batches, net, batch


def _heads(fs):
    for f in fs:
        f.update_head()
    torch.cuda.synchronize()
    return [f.bucket.clone() for f in fs]


def _sum(buckets):
    """The all-reduce's stand-in: fp32, on the GPU, in ascending rank order."""
    total = buckets[0].clone()
    for b in buckets[1:]:
        total = total + b
    return total


def _tails(fs, total):
    for f in fs:
        f.bucket.copy_(total)
        f.update_tail()
    torch.cuda.synchronize()


def _in_step(U, fs, where):
    """(d): every copy of the weights, the moments and every state word but each rank's own five logged means, bit for bit across the ranks."""
    o = U.K["DWP_S_OUT"]
    keep = [i for i in range(U.K["DWP_S_WORDS"]) if not (o <= i < o + 5)]
    for r, f in enumerate(fs[1:], 1):
        for name in NAMES:
            assert torch.equal(getattr(fs[0], name), getattr(f, name)), (where, r, name)
        assert torch.equal(fs[0].state[keep].view(torch.int32), f.state[keep].view(torch.int32)), (where, r, fs[0].state.tolist(), f.state.tolist())


def _rounded(total):
    """What the tail makes of the bucket under DWP_S_G16: the weight part through fp16, the bias part as it is."""
    t = total.clone()
    t[:T.NWT] = total[:T.NWT].half().float()
    return t


def _note(worst, where, name, got, t, bound):
    fr = G._frac(got, t, torch.clamp(bound, min=1e-300))
    worst[name] = max(worst.get(name, 0.0), fr)
    assert fr <= 1.0, (where, name, fr)


def _padding_is_zero(flat_words):
    W1 = flat_words[:T.NW1].view(2, T.HID, T.INP)
    W3 = flat_words[T.NW1 + T.NW2:T.NWT].view(2, T.OUTP, T.HID)
    return float(W1[:, :, T.IN:].abs().max()) == 0.0 and float(W3[0, T.ACT:].abs().max()) == 0.0 and float(W3[1, 1:].abs().max()) == 0.0


def _report(case, worst):
    left = sorted(k for k in LEFT_OUT if k[0].startswith(case + "/"))
    print("ppo-sharded %s: " % case + ", ".join("%s %.3f" % (k, x) for k, x in worst.items()) + ", left out %r" % (left,))


@pytest.mark.gpu
@pytest.mark.parametrize("R,B", WORLDS, ids=["R%d_B%d" % w for w in WORLDS])
def test_ranks_buckets_their_sum_and_the_tail_against_float64(R, B):
    """Four updates of R ranks (minibatch index 0, 1, 2, 0) next to ONE unsharded learner over the same rows (minibatch R B, scale 16 R B, its
    minibatch k = the ranks' minibatches k one after the other), which takes rank 0's weights and moments before every update.
    (a) every rank's bucket after update_head: its weight words ARE fl(fl(fl(fl(g32[0] + g32[1]) + g32[2]) + g32[3]) * fl(1 / R)); weights and
        biases within `rank_bucket`'s bound of the float64 gradient of the rank's own stored operands / R; the bias columns of pbuf and the
        bucket's padding words zero; every stage of the rank's forward and backward, and its logged means (the rank's OWN rows), as
        tests/test_ppo_edges_gpu holds an unsharded update.
    (b) rows: every rank's rows of x16 .. dh1 carry the bits of the same rows of the big learner; the unscaled sum of the buckets and the
        big learner's unscaled gradient are each within their own bound of the same float64 gradient of the union.  (p is NOT compared
        between them: Adam's first steps are lr sign(g), and where |g| is within its rounding error two honest gradients step 2 lr apart.)
    (c) the tail of rank 0 against clip_adam / scaler_update on the exact fp32 words of the sum, tolerances of tests/test_ppo_edges_gpu.
    (d) after every update the ranks hold the same bits."""
    from isaacgymdyros_amd import ppo_update as U
    K, case = U.K, "R%d_B%d" % (R, B)
    fs, nets, batches, net, batch = _ranks(U, R, B, _seed(R, B))
    big = U.FusedPpoUpdate(copy.deepcopy(net), C, R * B, T.NMB, DEV)
    big.set_learning_rates(*LR)
    big.state[K["DWP_S_SCALE"]] = 16.0 * R * B
    assert _per_sample_scale(16.0 * R * B, R * B) == 16.0
    idx = torch.cat([torch.arange(r * T.NMB * B + k * B, r * T.NMB * B + (k + 1) * B) for k in range(T.NMB) for r in range(R)])
    big.bind_batch(*[t[idx].to(DEV).contiguous() for t in batch])
    assert all(f.mfma and f.rowmajor and f.collective for f in fs) and big.mfma and not big.collective
    inv_world = torch.tensor(1.0 / R, dtype=torch.float32, device=DEV)
    worst, mbs = {}, []
    for it in range(UPDATES):
        with torch.no_grad():
            for name in NAMES:
                getattr(big, name).copy_(getattr(fs[0], name))
        snaps = [G._snapshot(U, f) for f in fs]
        mbs.append(snaps[0]["mb"])
        own = _heads(fs)
        for r, f in enumerate(fs):          # (a), the part that the tail would destroy
            g32 = f.g32
            assert torch.equal(own[r][:T.NWT], (((g32[0] + g32[1]) + g32[2]) + g32[3]) * inv_world), (case, it, r)
            assert float(f.pbuf[:, :, :PB_ST].abs().max()) == 0.0 and _padding_is_zero(own[r]), (case, it, r)
        total = _sum(own)
        _tails(fs, total)
        big.update()
        torch.cuda.synchronize()
        ts, bounds = [], []
        for r, f in enumerate(fs):          # (a) against float64, and the rank's own logged means
            _, _, pairs = G._check_gradients(U, "%s/%d" % (case, r), f, nets[r], batches[r], snaps[r], worst, left_out=LEFT_OUT, sharded=True)
            t, bound = T.rank_bucket(pairs, B, R)
            _note(worst, (case, it, r), "bucketW", own[r][:T.NWT], t[:T.NWT], bound[:T.NWT])
            _note(worst, (case, it, r), "bucketb", own[r][T.NWT:], t[T.NWT:], bound[T.NWT:])
            ts.append(t); bounds.append(bound)
            for name in ROWS:          # (b) rows are independent
                mine, theirs = getattr(f, name), getattr(big, name)
                theirs = theirs[r * B:(r + 1) * B] if name == "x16" else theirs[:, r * B:(r + 1) * B]
                assert torch.equal(mine.view(torch.int16), theirs.view(torch.int16)), (case, it, r, name)
        # (b) the unscaled gradients of both sides against the float64 gradient of the union (scaled: 16 per sample on both sides)
        x2 = big.x16.unsqueeze(0).expand(2, R * B, T.INP)
        bp = ((big.dh1, x2), (big.dh2, big.h1), (big.dout, big.h2))
        gS = [T.wgrad(dz, a) for dz, a in bp]
        gB = [T.bgrad(dz) for dz, _ in bp]
        union = T.flat(*[g for g, _ in gS], *[g for g, _ in gB])
        bound_big = T.flat(*[T.wgrad_sum_bound(S, R * B) for _, S in gS], *[b for _, b in gB])
        gsum = ((big.g32[0] + big.g32[1]) + big.g32[2]) + big.g32[3]
        _note(worst, (case, it), "big", T.f64(torch.cat([gsum, big.gb])) / (16.0 * R * B), union / (16.0 * R * B), bound_big / (16.0 * R * B))
        t_sum, reduce_bound = T.bucket_sum(own)
        bound_sum = sum(bounds) + reduce_bound
        _note(worst, (case, it), "sum", T.f64(total) / (16.0 * B), union / R / (16.0 * B), bound_sum / (16.0 * B))
        assert bool(((t_sum - T.f64(total)).abs() <= reduce_bound).all()) and _padding_is_zero(total)
        # (c), (d)
        G._check_tail(U, fs[0], snaps[0], total)
        _in_step(U, fs, (case, it))
    assert mbs == [0, 1, 2, 0] and all(f.state[K["DWP_S_STEP"]:K["DWP_S_STEP"] + 2].tolist() == [4.0, 4.0] for f in fs)
    _report(case, worst)


@pytest.mark.gpu
def test_an_overflow_on_one_rank_skips_the_critic_on_every_rank():
    """R = 2, B_r = 32.  The returns of rank 1's minibatch 1 are 3.0e4 (tests/test_ppo_gpu.py's recipe): its critic's output gradient overflows
    fp16.  Before the sum rank 0's slabs and bucket are finite and rank 1's critic words are not (its actor words are); after the tail BOTH
    ranks found [False, True]: the critic's p, m, v and step count keep their bits, the actor stepped, the scale is halved, the growth tracker 0,
    skipped logged -- and the ranks are still in step.  The next update is clean."""
    from isaacgymdyros_amd import ppo_update as U
    K, R, B = U.K, 2, 32

    def edit(batch):
        batch[5][T.NMB * B + B:T.NMB * B + 2 * B] = 3.0e4
    fs, _, _, _, _ = _ranks(U, R, B, _seed(R, B) + 100, edit=edit)
    mask = T.actor_mask().to(DEV)
    for it, found in enumerate(((False, False), (False, True), (False, False))):
        snaps = [G._snapshot(U, f) for f in fs]
        own = _heads(fs)
        assert bool(torch.isfinite(fs[0].g32).all()) and bool(torch.isfinite(own[0]).all())
        assert bool(torch.isfinite(own[1][mask]).all()) and bool(torch.isfinite(own[1][~mask]).all()) == (it != 1)
        total = _sum(own)
        _tails(fs, total)
        for f, snap in zip(fs, snaps):
            G._check_tail(U, f, snap, total, found=found)
            st = f.state.cpu().tolist()
            moved = f.p != snap["p"]
            assert bool((moved & mask).any()) and bool((moved & ~mask).any()) == (it != 1)
            if it == 1:
                for name in ("p", "m", "v"):
                    assert torch.equal(getattr(f, name)[~mask], snap[name][~mask]), name
                assert [st[K["DWP_S_STEP"]], st[K["DWP_S_STEP"] + 1]] == [2.0, 1.0]
                assert st[K["DWP_S_SCALE"]] == 8.0 * B and st[K["DWP_S_GROWTH"]] == 0.0 and f.logged()[7].item() == 1.0
        _in_step(U, fs, it)
    assert all(f.state[K["DWP_S_STEP"]:K["DWP_S_STEP"] + 2].tolist() == [3.0, 2.0] and f.logged()[7].item() == 0.0 for f in fs)


class _Saved:
    """Everything an update_tail changes (and the accumulators it clears), to run several tails from one head."""
    WHAT = NAMES + ("state", "pbuf", "part", "g32")

    def __init__(self, fs):
        self.fs, self.kept = fs, [{name: getattr(f, name).clone() for name in self.WHAT} for f in fs]

    def restore(self):
        with torch.no_grad():
            for f, kept in zip(self.fs, self.kept):
                for name, t in kept.items():
                    getattr(f, name).copy_(t)


def _skipped_alone(f, snap, mask, found):
    """Only the nets of `found` kept their bits; the others moved."""
    moved = f.p != snap["p"]
    for net, sel in ((0, mask), (1, ~mask)):
        if found[net]:
            assert torch.equal(f.p[sel], snap["p"][sel]) and torch.equal(f.m[sel], snap["m"][sel]) and torch.equal(f.v[sel], snap["v"][sel])
        else:
            assert bool((moved & sel).any())


@pytest.mark.gpu
def test_a_non_finite_word_anywhere_in_the_sum_skips_its_net_alone():
    """`net_of` and the index cover of k_grad_stats<1> and k_adam<true, 1>.  R = 2, B_r = 32, one clean head; then, from the same snapshot each
    time, +inf in ONE word of the sum: the first and the last word of the actor's and of the critic's half of each of the six tensors (24
    words, among them NWT - 1, NWT and NP - 1).  found is ppo_update_truth.found_inf of that sum, the net of the word alone is skipped (bits
    kept), the other steps as clip_adam says, scale, step counts and minibatch index follow, the ranks stay in step.  And +inf on rank 0
    with -inf on rank 1 in the same actor word: their sum is NaN, which is no inf, and is found all the same."""
    from isaacgymdyros_amd import ppo_update as U
    R, B = 2, 32
    fs, _, _, _, _ = _ranks(U, R, B, _seed(R, B) + 200)
    mask_cpu = T.actor_mask()
    mask = mask_cpu.to(DEV)
    own = _heads(fs)
    saved, snap = _Saved(fs), G._snapshot(U, fs[0])
    words = []
    for _, o, n in T.tensor_spans():
        words += [o, o + n // 2 - 1, o + n // 2, o + n - 1]
    assert len(words) == 24 and {T.NWT - 1, T.NWT, T.NP - 1} <= set(words) and [bool(mask_cpu[w]) for w in words] == [True, True, False, False] * 6

    def run(total, want):
        saved.restore()
        _tails(fs, total)
        found = T.found_inf(total)
        assert found == want, (found, want)
        G._check_tail(U, fs[0], snap, total, found=found)          # (rank 1: the same bits, _in_step)
        for f in fs:
            _skipped_alone(f, snap, mask, found)
        _in_step(U, fs, want)

    run(_sum(own), [False, False])
    for w in words:
        total = _sum(own)
        total[w] = math.inf
        run(total, [bool(mask_cpu[w]), not bool(mask_cpu[w])])
    w = T.NW1 + 5 * T.HID + 3          # (the actor's W2)
    b0, b1 = own[0].clone(), own[1].clone()
    b0[w], b1[w] = math.inf, -math.inf
    total = _sum([b0, b1])
    assert math.isnan(float(total[w])) and int((~torch.isfinite(total)).sum()) == 1
    run(total, [True, False])


@pytest.mark.gpu
def test_fp16_grads_round_the_averaged_weights_after_the_sum_and_leave_the_biases():
    """fp16_grads=True (DWP_S_G16) in the sharded form, R = 2, B_r = 32.  Two updates: the tail is clip_adam on the sum with its WEIGHT part
    rounded through fp16 and its bias part untouched.  Then from one head: a weight word of 7.0e4 in the sum (inf in fp16) is found; a BIAS
    word of 7.0e4 is not; and the order the code ships: rank 0's gradient word 1.0e5 (beyond fp16), rank 1's 0 -- the average 5.0e4 is
    finite in fp16 and the update is NOT skipped (rounding each rank's gradient before the average would skip it)."""
    from isaacgymdyros_amd import ppo_update as U
    K, R, B = U.K, 2, 32
    fs, _, _, _, _ = _ranks(U, R, B, _seed(R, B) + 300, fp16_grads=True)
    assert all(float(f.state[K["DWP_S_G16"]]) == 1.0 for f in fs)
    for it in range(2):
        snap = G._snapshot(U, fs[0])
        total = _sum(_heads(fs))
        assert not torch.equal(_rounded(total), total)
        _tails(fs, total)
        G._check_tail(U, fs[0], snap, _rounded(total))
        _in_step(U, fs, it)
    own = _heads(fs)
    saved, snap = _Saved(fs), G._snapshot(U, fs[0])
    mask = T.actor_mask().to(DEV)
    wc = T.NW1 + T.NW2 // 2 + 7 * T.HID + 11          # (the critic's W2)
    for w, found in ((wc, [False, True]), (T.NWT + 3, [False, False]), (T.NWT + T.NB1 + T.NB2 // 2 + 2, [False, False])):
        saved.restore()
        total = _sum(own)
        total[w] = 7.0e4
        _tails(fs, total)
        assert T.found_inf(_rounded(total)) == found
        G._check_tail(U, fs[0], snap, _rounded(total), found=found)
        for f in fs:
            _skipped_alone(f, snap, mask, found)
        _in_step(U, fs, w)
    # the order: the ranks' gradients go into the sum unrounded
    saved.restore()
    s = torch.cuda.current_stream(DEV).cuda_stream
    for r, f in enumerate(fs):
        f.g32[:, wc] = 0.0
        if r == 0:
            f.g32[0, wc] = 1.0e5
        f._chk(f.api["grad_bucket"](f.g32.data_ptr(), f.pbuf.data_ptr(), f.bucket.data_ptr(), 1.0 / R, s))
        torch.cuda.synchronize()
        assert float(f.bucket[T.NWT:].abs().max()) == 0.0          # (the head's dwp_grad_bucket cleared the bias columns of pbuf ...)
        f.bucket[T.NWT:] = own[r][T.NWT:]                          # (... so its bias sums are put back)
        assert float(f.bucket[wc]) == (5.0e4 if r == 0 else 0.0) and torch.equal(f.bucket[:wc], own[r][:wc]) and torch.equal(f.bucket[wc + 1:], own[r][wc + 1:])
    total = _sum([f.bucket for f in fs])
    assert float(total[wc]) == 5.0e4 and math.isinf(float(torch.tensor(1.0e5).half())) and math.isfinite(float(total[wc].half()))
    _tails(fs, total)
    G._check_tail(U, fs[0], snap, _rounded(total), found=[False, False])
    _in_step(U, fs, "order")


@pytest.mark.gpu
def test_grad_bucket_refuses_bad_arguments_and_touches_nothing():
    """dwp_grad_bucket with inv_world 0, negative, above 1 (1.5, inf) and NaN, and with each pointer NULL in turn: -1, its own message in
    dwp_last_error(), and the sentinel-filled bucket and pbuf as they were."""
    from isaacgymdyros_amd import _lib, ppo_update as U
    api = U.declare(_lib.load()[0])
    g32 = torch.zeros(T.WG_SLABS, T.NWT, device=DEV)
    pbuf = torch.full((T.PBUF_BUCKETS, 2, T.K["DWP_PBUF_WORDS"]), 7.0, device=DEV)
    bucket = torch.full((T.NP,), -3.0, device=DEV)
    s = torch.cuda.current_stream(DEV).cuda_stream
    ptrs = [g32.data_ptr(), pbuf.data_ptr(), bucket.data_ptr()]
    calls = [ptrs + [x] for x in (0.0, -0.5, 1.5, math.inf, math.nan)] + [ptrs[:k] + [None] + ptrs[k + 1:] + [0.5] for k in range(3)]
    for args in calls:
        assert api["finish"](None, None, 1, 1, 1, None, s) == -1 and b"dwp_finish" in api["last_error"]()          # (another message first)
        assert api["grad_bucket"](*args, s) == -1, args
        assert b"dwp_grad_bucket" in api["last_error"](), (args, api["last_error"]())
    torch.cuda.synchronize()
    assert bool((bucket == -3.0).all()) and bool((pbuf == 7.0).all())
    assert api["grad_bucket"](*ptrs, 0.5, s) == 0          # (and a good call goes through: the sums of the sentinels, halved)
    torch.cuda.synchronize()
    assert bool((bucket[:T.NWT] == 0.0).all()) and bool((bucket[T.NWT:] == 0.5 * 7.0 * T.PBUF_BUCKETS).all()) and bool((pbuf[:, :, :PB_ST] == 0.0).all())
    assert bool((pbuf[:, :, PB_ST:] == 7.0).all())
