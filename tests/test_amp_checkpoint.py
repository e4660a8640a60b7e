"""isaacgymdyros_amd/amp_checkpoint.py on the CPU (torch backend): the reference learner's checkpoint layout, the merged Adam state, save /
restore, resuming, and the play path's text export."""
import copy
import os
import re

import numpy as np
import torch
import torch.nn as nn

from isaacgymdyros_amd import amp_checkpoint as CK
from isaacgymdyros_amd import amp_disc as AD
from isaacgymdyros_amd import amp_policy as AP
from oracle import ref_harness as RH

D, A, DA = 468, 12, 68          # TocabiAMPLower: num_obs, num_actions, num_amp_obs (2 steps of 34)
REF = os.path.join(RH.IGE, "learning")          # the reference checkout (oracle/ref_harness.py: paths only)
CFG = copy.deepcopy(AD.TRAIN_CFG)
CFG["config"].update(amp_obs_demo_buffer_size=512, amp_replay_buffer_size=1024, amp_batch_size=64)


def learners(seed=0, backend="torch", device="cpu"):
    pol = AP.AmpActorCritic(D, A, device, CFG, backend=backend, seed=seed)
    disc = AD.AmpDiscriminator(DA, device, CFG, backend=backend, seed=seed + 100)
    return pol, disc


def batch(seed, B=64, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    t = lambda *s: torch.randn(*s, generator=g).to(device)          # noqa: E731
    return dict(obs=t(B, D) * 1.5, act=t(B, A) * 0.5, nlp=t(B) + 10.0, adv=t(B), ret=t(B), amp=t(B, DA))


def fill(disc, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    disc.init_demo_buffer(lambda n: torch.randn(n, DA, generator=g).to(device))
    disc.store_replay(torch.randn(300, DA, generator=g).to(device))


def update(pol, disc, b, lr):
    """One minibatch of both learners as examples/amp_consumer.py takes it; returns the replay and demo draws."""
    replay, demo = disc.replay_batch(b["amp"]), disc.demo_buffer.sample(b["amp"].shape[0])
    pol.update(b["obs"], b["act"], b["nlp"], b["adv"], b["ret"], lr=lr)
    disc.update(b["amp"], replay.contiguous(), demo.contiguous(), lr=lr)
    disc.store_replay(b["amp"])
    return replay, demo


def trained(steps=2, seed=0, backend="torch", device="cpu"):
    pol, disc = learners(seed, backend, device)
    fill(disc, seed + 1, device)
    for k in range(steps):
        update(pol, disc, batch(10 + k, device=device), lr=1e-4 * (1 - 0.1 * k))
    return pol, disc


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a.cpu(), b.cpu()), what


def assert_same_learners(p1, d1, p2, d2):
    for k, v in p1.state_dict().items():
        same(v, p2.state_dict()[k], k)
    for k, v in d1.state_dict().items():
        same(v, d2.state_dict()[k], k)
    for x, y in ((p1, p2), (d1, d2)):
        ox, oy = x.optimizer_state(), y.optimizer_state()
        assert ox["step"] == oy["step"] and np.float32(ox["lr"]) == np.float32(oy["lr"])          # (one lr in the merged state)
        for part in ("exp_avg", "exp_avg_sq"):
            assert ox[part].keys() == oy[part].keys()
            for k in ox[part]:
                same(ox[part][k], oy[part][k], (part, k))


def test_layout_keys_order_shapes_dtypes():
    pol, disc = trained(1)
    ck = CK.state(pol, disc, epoch=3, frame=3 * 64)
    assert set(ck) == set(CK.TOP_KEYS) | {CK.OUR_KEY}
    expect = [("sigma", (A,))] + [(n + "." + k, s) for n, (i, h) in (("actor_mlp", (D, 512)), ("critic_mlp", (D, 512)))
                                  for k, s in (("0.weight", (512, i)), ("0.bias", (512,)), ("2.weight", (512, 512)), ("2.bias", (512,)))] + \
        [("value.weight", (1, 512)), ("value.bias", (1,)), ("mu.weight", (A, 512)), ("mu.bias", (A,)),
         ("_disc_mlp.0.weight", (256, DA)), ("_disc_mlp.0.bias", (256,)), ("_disc_mlp.2.weight", (256, 256)), ("_disc_mlp.2.bias", (256,)),
         ("_disc_logits.weight", (1, 256)), ("_disc_logits.bias", (1,))]
    assert list(ck["model"]) == ["a2c_network." + k for k, _ in expect]
    for k, s in expect:
        t = ck["model"]["a2c_network." + k]
        assert tuple(t.shape) == s and t.dtype == torch.float32, (k, t.shape, t.dtype)
    for key, n in (("running_mean_std", D), ("reward_mean_std", 1), ("amp_input_mean_std", DA)):
        st = ck[key]
        assert list(st) == ["running_mean", "running_var", "count"]
        assert st["running_mean"].shape == (n,) and st["running_var"].shape == (n,) and st["count"].shape == ()
        assert all(v.dtype == torch.float64 for v in st.values())
    assert ck["epoch"] == 3 and ck["frame"] == 192 and ck["last_mean_rewards"] == -100500 and ck["env_state"] is None
    pg = ck["optimizer"]["param_groups"]
    assert len(pg) == 1 and pg[0]["params"] == list(range(len(expect)))
    assert tuple(pg[0]["betas"]) == (0.9, 0.999) and pg[0]["eps"] == 1e-8 and pg[0]["weight_decay"] == 0 and pg[0]["lr"] == pol.optimizer_state()["lr"]
    assert 0 not in ck["optimizer"]["state"] and sorted(ck["optimizer"]["state"]) == list(range(1, len(expect)))
    for i, (k, s) in enumerate(expect[1:], 1):
        e = ck["optimizer"]["state"][i]
        assert float(e["step"]) == 1 and e["exp_avg"].shape == s and e["exp_avg_sq"].shape == s
    ours = ck[CK.OUR_KEY]
    assert {"demo_buffer", "replay_buffer", "torch_rng_state", "lr0", "lr_min", "max_epochs"} <= set(ours)


def test_layout_follows_the_reference_sources():
    """The table above rests on these lines of the reference; where its checkout is present, they are read."""
    if not os.path.isdir(REF):
        return
    a2c = open(os.path.join(REF, "rl_games_custom", "a2c_common_dyros.py")).read()
    for k in ("running_mean_std", "reward_mean_std", "model", "epoch", "optimizer", "frame", "last_mean_rewards", "env_state"):
        assert "state['%s']" % k in a2c, k
    assert "weights.get('last_mean_rewards', -100500)" in a2c
    assert "state['amp_input_mean_std']" in open(os.path.join(REF, "amp_continuous.py")).read()
    nb = open(os.path.join(REF, "rl_games_custom", "network_builder_dyros.py")).read()
    pos = [nb.index(s) for s in ("self.actor_mlp = self._build_mlp", "self.critic_mlp = self._build_mlp", "self.value = torch.nn.Linear",
                                 "self.mu = torch.nn.Linear", "self.sigma = nn.Parameter")]
    assert pos == sorted(pos)
    amp = open(os.path.join(REF, "amp_network_builder.py")).read()
    assert amp.index("super().__init__(params, **kwargs)") < amp.index("self._build_disc(") < amp.index("self._disc_mlp = self._build_mlp") \
        < amp.index("self._disc_logits = torch.nn.Linear")
    player = open(os.path.join(REF, "amp_players.py")).read()
    assert "checkpoint['amp_input_mean_std']" in player and '"running_mean_std_" + name + ".txt"' in player


def test_optimizer_loads_into_a_plain_adam_in_model_order():
    pol, disc = trained(2)
    ck = CK.state(pol, disc, epoch=1)

    class Net(nn.Module):          # the registration order of AMPBuilder.Network
        def __init__(self):
            super().__init__()
            self.sigma = nn.Parameter(torch.zeros(A), requires_grad=False)
            self.actor_mlp = nn.Sequential(nn.Linear(D, 512), nn.ReLU(), nn.Linear(512, 512), nn.ReLU())
            self.critic_mlp = nn.Sequential(nn.Linear(D, 512), nn.ReLU(), nn.Linear(512, 512), nn.ReLU())
            self.value = nn.Linear(512, 1)
            self.mu = nn.Linear(512, A)
            self._disc_mlp = nn.Sequential(nn.Linear(DA, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU())
            self._disc_logits = nn.Linear(256, 1)

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.a2c_network = Net()

    m = Model()
    assert list(m.state_dict()) == list(ck["model"])
    m.load_state_dict(ck["model"])
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, eps=1e-08, weight_decay=0)
    opt.load_state_dict(ck["optimizer"])
    params = list(m.parameters())
    assert opt.param_groups[0]["lr"] == ck["optimizer"]["param_groups"][0]["lr"]
    po, do = pol.optimizer_state(), disc.optimizer_state()
    for i, k in enumerate(CK.MODEL_KEYS):
        if k == "sigma":
            assert params[i] not in opt.state
            continue
        src = do if k in CK.DISC_KEYS else po
        same(opt.state[params[i]]["exp_avg"], src["exp_avg"][k], k)
        same(opt.state[params[i]]["exp_avg_sq"], src["exp_avg_sq"][k], k)
    # and it steps: one Adam step of the merged optimiser moves every trained parameter
    for p in params[1:]:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in params]
    opt.step()
    assert all(not torch.equal(b, p) for b, p in zip(before[1:], params[1:]))


def test_save_restore_bit_identical(tmp_path):
    pol, disc = trained(2)
    path = CK.save(str(tmp_path / "nn" / "x.pth"), pol, disc, epoch=2, frame=128, lr0=1e-4, lr_min=1e-6, max_epochs=5000)
    rng = torch.get_rng_state()
    torch.manual_seed(1234)          # (restore brings the generator back)
    p2, d2 = learners(seed=7)
    c = CK.restore(path, p2, d2)
    assert c == {"epoch": 2, "frame": 128, "last_mean_rewards": -100500, "lr0": 1e-4, "lr_min": 1e-6, "max_epochs": 5000}
    assert torch.equal(torch.get_rng_state(), rng)
    assert_same_learners(pol, disc, p2, d2)
    for name in ("demo_buffer", "replay_buffer"):
        b1, b2 = getattr(disc, name), getattr(d2, name)
        assert (b1._head, b1._total_count, b1._sample_head) == (b2._head, b2._total_count, b2._sample_head)
        same(b1._sample_idx, b2._sample_idx, name)
        same(b1._data, b2._data, name)
    # a file without our key (the reference learner's) restores the weights and the optimiser, the buffers stay
    ck = torch.load(path, weights_only=True)
    del ck[CK.OUR_KEY]
    p3, d3 = learners(seed=8)
    c = CK.restore(ck, p3, d3)
    assert c["epoch"] == 2 and c["lr0"] is None
    assert_same_learners(pol, disc, p3, d3)
    assert d3.replay_buffer.get_total_count() == 0


def test_resume_equivalence(tmp_path):
    pol, disc = trained(3)
    path = CK.save(str(tmp_path / "r.pth"), pol, disc, epoch=3)
    nxt = batch(99)
    p2, d2 = learners(seed=5)
    torch.manual_seed(77)
    CK.restore(path, p2, d2)          # (the generator as it was at the save: the next draws repeat)
    r2, m2 = update(p2, d2, nxt, lr=7e-5)
    torch.set_rng_state(torch.load(path, weights_only=True)[CK.OUR_KEY]["torch_rng_state"])
    r1, m1 = update(pol, disc, nxt, lr=7e-5)
    same(r1, r2, "replay draw")
    same(m1, m2, "demo draw")
    assert_same_learners(pol, disc, p2, d2)
    same(pol.p, p2.p, "policy p")
    same(disc.p, d2.p, "disc p")


def test_torch_learner_adapter_round_trip():
    """examples/amp_consumer.py's inline model and Adam through CK.TorchLearner: the same checkpoint as AmpActorCritic's torch backend."""
    pol, disc = trained(2)
    ck = CK.state(pol, disc, epoch=2)
    net = AP.ActorCritic(D, A, [512, 512], -1.6)
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4, eps=1e-8)
    tl = CK.TorchLearner(net, opt)
    _p, d2 = learners(seed=3)
    CK.restore(ck, tl, d2)
    ck2 = CK.state(tl, d2, epoch=2)
    for k, v in ck["model"].items():
        same(v, ck2["model"][k], k)
    for i, e in ck["optimizer"]["state"].items():
        for part in ("step", "exp_avg", "exp_avg_sq"):
            same(e[part], ck2["optimizer"]["state"][i][part], (i, part))


def test_export_txt_names_and_values(tmp_path):
    pol, disc = trained(1)
    ck = CK.state(pol, disc, epoch=1)
    out = CK.export_txt(ck, str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    expect = sorted([k.replace(".", "_") + ".txt" for k in ck["model"]] +
                    ["running_mean_std_running_mean.txt", "running_mean_std_running_var.txt", "running_mean_std_count.txt"])
    assert names == expect and sorted(os.path.basename(p) for p in out) == expect
    assert "a2c_network_actor_mlp_0_weight.txt" in names and "a2c_network__disc_logits_bias.txt" in names
    for k, t in ck["model"].items():
        back = np.loadtxt(tmp_path / (k.replace(".", "_") + ".txt"), dtype=np.float64).astype(np.float32).reshape(t.shape)
        assert np.array_equal(back.view(np.uint32), t.numpy().view(np.uint32)), k
    for k, t in ck["running_mean_std"].items():
        back = np.loadtxt(tmp_path / ("running_mean_std_" + k + ".txt"), dtype=np.float64).reshape(-1)
        assert np.array_equal(back, t.reshape(-1).numpy()), k
    # np.savetxt's defaults: '%.18e', one row per line, space separated
    line = open(tmp_path / "a2c_network_mu_weight.txt").readline().split()
    assert len(line) == 512 and all(re.fullmatch(r"-?\d\.\d{18}e[+-]\d\d", x) for x in line)
