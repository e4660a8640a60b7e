"""The torch form of the AMP discriminator (isaacgymdyros_amd/amp_disc.py, backend="torch") against the reference's own AMP learner:
tests/golden/amp_learner_ref.npz, minted by oracle/make_amp_learner_goldens.py from learning/amp_continuous.py, amp_network_builder.py and
replay_buffer.py, and live against those files where the reference checkout is mounted.

The torch form is the yardstick of the HIP kernels (tests/test_amp_disc_gpu.py, tests/test_amp_disc_reference_gpu.py); these tests tie
it to the reference.  Where the arithmetic is the same op for op (the loss, its autograd gradient, the reward formula, the buffers) the
comparison is bit for bit, in float64 and in fp32, with one CPU thread as the fixture was minted."""
import os

import numpy as np
import pytest
import torch

import amp_disc_truth as T
from isaacgymdyros_amd import amp_disc as AD
from oracle import make_amp_learner_goldens as ML

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "amp_learner_ref.npz")
_live = {}


def records():
    """The fixture, and the reference's own run where it is mounted."""
    out = [("fixture", dict(np.load(GOLDEN)))]
    if ML.available():
        if not _live:
            _live.update(ML.compute())
        out.append(("live", _live))
    return out


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_fixture_is_what_the_reference_computes_now():
    """Live only: every array of the committed fixture equals a fresh run of the minting script (the stand-ins, seeds and cases)."""
    if not ML.available():
        assert os.path.exists(GOLDEN)          # (without the checkout the fixture alone is the record)
        return
    g = records()[0][1]
    live = records()[1][1]
    assert sorted(g) == sorted(live)
    for k in g:
        assert np.array_equal(g[k], live[k]), k


def disc_of(D, p, stats=None, cfg=None):
    d = AD.AmpDiscriminator(D, "cpu", cfg, backend="torch", seed=0)
    with torch.no_grad():
        d.p.copy_(torch.from_numpy(p))
        if stats is not None:
            d.stats.copy_(torch.from_numpy(stats))
    return d


def net_of(D, p, dtype):
    d = disc_of(D, p)
    net = d.net.to(dtype)
    return net


@pytest.mark.parametrize("D", ML.DIMS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_torch_disc_loss_is_the_reference(D, dtype, one_thread):
    """amp_disc.torch_disc_loss on the normalised rows: total, every logged value and the gradient of disc_coef * disc_loss with respect to
    every parameter, bit for bit (same ops in the same order as _disc_loss + autograd)."""
    s = "64" if dtype == torch.float64 else "32"
    for src, g in records():
        net = net_of(D, g["%d/p" % D], dtype)
        an, rn, dn = (torch.from_numpy(g["%d/xn_%s" % (D, k)]).to(dtype) for k in ("agent", "replay", "demo"))
        total, vals = AD.torch_disc_loss(net, an, rn, dn, **ML.COEF)
        n = net
        ps = [n._disc_mlp[0].weight, n._disc_mlp[0].bias, n._disc_mlp[2].weight, n._disc_mlp[2].bias, n._disc_logits.weight, n._disc_logits.bias]
        grad = torch.cat([x.reshape(-1) for x in torch.autograd.grad(total, ps)]).detach().numpy()
        assert np.array_equal(grad, g["%d/grad%s" % (D, s)]), (src, np.abs(grad - g["%d/grad%s" % (D, s)]).max())
        names = ["total", "pred", "disc_logit_loss", "disc_grad_penalty", "weight_decay_sum", "agent_logit_mean", "demo_logit_mean",
                 "agent_acc", "demo_acc"]
        for name, v in zip(names, vals):
            assert float(v) == float(g["%d/val%s_%s" % (D, s, name)]), (src, name, float(v), float(g["%d/val%s_%s" % (D, s, name)]))


@pytest.mark.parametrize("D", ML.DIMS)
def test_float32_baseline_is_a_few_ulp_of_float64(D):
    """The fixture's own precision statement: the reference's fp32 gradient is close to the float64 one and not equal to it (the baseline
    the GPU tests scale their per-tensor tolerance by is a real, non-zero error)."""
    g = dict(np.load(GOLDEN))
    e = np.abs(g["%d/grad32" % D] - g["%d/grad64" % D])
    assert 0 < e.max() <= 1e-5 * np.abs(g["%d/grad64" % D]).max()


@pytest.mark.parametrize("D", ML.DIMS)
def test_torch_backend_minibatch_is_the_reference(D, one_thread):
    """The torch form's whole minibatch from the raw rows: train-mode statistics (three snapshots), normalised rows, gradient, logged
    values, bit for bit the fixture's fp32 record (the statistics restatement is the one the fixture was minted with; see the README)."""
    for src, g in records():
        d = disc_of(D, g["%d/p" % D], g["%d/stats_in" % D])
        seen = []
        orig = d.rms.forward

        def spy(x):
            y = orig(x)
            seen.append((y.detach().numpy().copy(), d.stats.numpy().copy()))
            return y
        d.rms.forward = spy
        d.accumulate_grad(*(torch.from_numpy(g["%d/%s" % (D, k)]) for k in ("agent", "replay", "demo")))
        for (xn, st), k in zip(seen, ("agent", "replay", "demo")):
            assert np.array_equal(xn, g["%d/xn_%s" % (D, k)]), (src, k)
            assert np.array_equal(st, g["%d/stats_%s" % (D, k)]), (src, k)
        assert np.array_equal(d.g.numpy(), g["%d/grad32" % D]), src
        assert float(d.state[AD.K["DWD_S_LOSS"]]) == float(g["%d/val32_total" % D])
        assert float(d.state[AD.K["DWD_S_GRAD_PEN"]]) == float(g["%d/val32_disc_grad_penalty" % D])


@pytest.mark.parametrize("case", ["34", "68", "probe"])
def test_rewards_are_the_reference(case, one_thread):
    """_calc_disc_rewards + _combine_rewards in eval mode: logits, disc_r and combined bit for bit in fp32 (the same ops: eval-mode
    normalisation, nn.Linear, 1 / (1 + exp(-l)), the 1e-4 floor, * disc_reward_scale, 0.7 task + 0.3 disc).  The probe network's logit is
    exactly 4 x_0: it takes the formula across the floor, to -20 and through 0."""
    cfg = {"network": AD.TRAIN_CFG["network"], "config": dict(AD.TRAIN_CFG["config"], disc_reward_scale=ML.REWARD["scale"],
                                                              task_reward_w=ML.REWARD["task_w"], disc_reward_w=ML.REWARD["disc_w"])}
    for src, g in records():
        pre = "probe_" if case == "probe" else case + "/reward_"
        out = "probe_" if case == "probe" else case + "/"
        D = 34 if case == "probe" else int(case)
        d = disc_of(D, T.reward_params(g, case), g[pre + "stats"], cfg)
        x, task = torch.from_numpy(g[pre + "x"]), torch.from_numpy(g[pre + "task"])
        c, r, l = d.rewards(x[None], task[None], return_logits=True)
        assert np.array_equal(l[0, :, 0].numpy(), g[pre + "logit32"]), src
        assert np.array_equal(r[0, :, 0].numpy(), g[out + "disc_r32"]), src
        assert np.array_equal(c[0, :, 0].numpy(), g[out + "combined32"]), src
        if case == "probe":
            assert (g[pre + "logit32"] > np.log(1e4)).sum() >= 10 and (g[pre + "logit32"] <= -16).any() and (np.abs(g[pre + "logit32"]) < 1e-5).any()


def test_replay_buffer_is_the_reference():
    """learning/replay_buffer.py's store / sample / wrap sequence under the seeded global generator: the permutation, every sample, the
    stored rows and the heads."""
    for src, g in records():
        torch.manual_seed(20261015)
        buf = AD.ReplayBuffer(23, "cpu")
        assert np.array_equal(buf._sample_idx.numpy(), g["replay_perm0"])
        rows = torch.arange(200, dtype=torch.float32)[:, None] * torch.tensor([[1.0, -1.0, 0.5]])
        k, samples = 0, []
        for is_store, n in g["replay_seq"]:
            if is_store:
                buf.store(rows[k:k + n])
                k += n
            else:
                samples.append(buf.sample(int(n)).numpy())
        assert np.array_equal(np.concatenate(samples), g["replay_samples"]), src
        assert np.array_equal(buf._data.numpy(), g["replay_data"]), src
        assert [buf._head, buf._total_count, buf._sample_head] == g["replay_head"].tolist(), src


def test_store_replay_keep_probability_is_the_reference():
    """_store_replay_amp_obs: five stores of 30 rows into a buffer of 50 with keep probability 0.25 -- all kept while the count has not
    passed the size, then the reference's Bernoulli draws from the global generator; the counts and the stored rows."""
    cfg = {"network": AD.TRAIN_CFG["network"], "config": dict(AD.TRAIN_CFG["config"], amp_replay_buffer_size=50, amp_replay_keep_prob=0.25)}
    for src, g in records():
        d = AD.AmpDiscriminator(34, "cpu", cfg, backend="torch", seed=0)
        torch.manual_seed(20261016)
        d.replay_buffer = AD.ReplayBuffer(50, "cpu")
        rows = torch.arange(30 * 5, dtype=torch.float32).reshape(5, 30, 1) + 1000
        counts = []
        for i in range(5):
            d.store_replay(rows[i])
            counts.append(d.replay_buffer.get_total_count())
        assert counts == g["keep_counts"].tolist(), (src, counts)
        assert np.array_equal(d.replay_buffer._data.numpy(), g["keep_data"]), src
        assert d.replay_buffer._head == int(g["keep_head"][()])
