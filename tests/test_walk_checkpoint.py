"""isaacgymdyros_amd/ppo_checkpoint.py on the CPU (the eager learner of examples/ppo_consumer.py): the reference learner's checkpoint layout, the two
Adam states in the reference's parameter order, the fused update's layout cut per parameter, save / restore, resuming, the text export of the play
path, and train()'s --output-dir / --checkpoint."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from isaacgymdyros_amd import ppo_checkpoint as PK
from isaacgymdyros_amd import ppo_update as U
from isaacgymdyros_amd import walk_policy as WP
from oracle import ref_harness as RH

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.path.join(RH.IGE, "learning", "rl_games_custom")          # the reference checkout (oracle/ref_harness.py: paths only)
D, A, H = U.IN, U.ACT, U.HID


def _mod():
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


PPO = _mod()
C = PPO.TRAIN_CFG["config"]


def learner(seed=0):
    torch.manual_seed(seed)
    net = PPO.DyrosActorCritic(D, A, PPO.TRAIN_CFG["network"])
    with torch.no_grad():          # (orthogonal init at gain 0.01 leaves gradients tiny: larger weights make every update visible)
        for p in net.actor_parameters() + net.critic_parameters():
            p.add_(torch.randn_like(p) * 0.05)
    opt_a = torch.optim.Adam(net.actor_parameters(), lr=C["learning_rate"], eps=1e-8)
    opt_c = torch.optim.Adam(net.critic_parameters(), lr=C["critic_lr"], eps=1e-8)
    scaler = torch.amp.GradScaler("cuda", enabled=False)          # (what train() makes on a CPU device)
    return net, opt_a, opt_c, scaler


def batch(seed, B=64):
    g = torch.Generator().manual_seed(seed)
    t = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    return dict(obs=t(B, D), act=t(B, A) * 0.3, nlp=t(B) + 20.0, mu=t(B, A) * 0.1, adv=t(B), ret=t(B), val=t(B, 1))


def update(net, opt_a, opt_c, scaler, b, lr):
    """One minibatch of train()'s eager update (minibatch_update of examples/ppo_consumer.py, autocast off on the CPU)."""
    for g in opt_a.param_groups:
        g["lr"] = lr
    mu, logstd, value = net(b["obs"])
    sigma = torch.exp(logstd)
    a_loss, _cf = PPO.actor_loss(b["nlp"], PPO.neglogp(b["act"], mu, sigma, logstd), b["adv"], C["e_clip"])
    c_loss = PPO.critic_loss(b["val"], value, C["e_clip"], b["ret"].unsqueeze(1), C["clip_value"])
    loss = a_loss.mean() + 0.5 * c_loss.mean() * C["critic_coef"]
    for p in net.parameters():
        p.grad = None
    scaler.scale(loss).backward()
    scaler.unscale_(opt_a); scaler.unscale_(opt_c)
    nn.utils.clip_grad_norm_(net.actor_parameters(), C["grad_norm"])
    scaler.step(opt_a); scaler.step(opt_c); scaler.update()


def trained(steps=2, seed=0):
    L = learner(seed)
    for k in range(steps):
        update(*L, batch(10 + k), lr=1e-5 * (1 - 0.1 * k))
    return L


def same(a, b, what):
    assert torch.is_tensor(a) and torch.is_tensor(b), what
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a.cpu(), b.cpu()), what


def assert_same(L1, L2):
    (n1, a1, c1, _), (n2, a2, c2, _) = L1, L2
    for k, v in n1.state_dict().items():
        same(v, n2.state_dict()[k], k)
    for o1, o2 in ((a1, a2), (c1, c2)):
        s1, s2 = o1.state_dict(), o2.state_dict()
        assert s1["param_groups"][0]["lr"] == s2["param_groups"][0]["lr"]
        assert sorted(s1["state"]) == sorted(s2["state"])
        for i in s1["state"]:
            for part in ("step", "exp_avg", "exp_avg_sq"):
                same(s1["state"][i][part], s2["state"][i][part], (i, part))


EXPECT = [("sigma", (A,))] + [(n + "." + k, s) for n in ("actor_mlp", "critic_mlp")
                              for k, s in (("0.weight", (H, D)), ("0.bias", (H,)), ("2.weight", (H, H)), ("2.bias", (H,)))] + \
    [("value.weight", (1, H)), ("value.bias", (1,)), ("mu.weight", (A, H)), ("mu.bias", (A,))]


def test_layout_keys_order_shapes_dtypes():
    net, oa, oc, sc = trained(1)
    ck = PK.state(net, epoch=3, frame=3 * 64, opt_actor=oa, opt_critic=oc, scaler=sc, lr0=1e-5, lr_min=3e-6, max_epochs=5000)
    assert list(ck) == ["scaler", "model", "epoch", "optimizer_actor", "optimizer_critic", "frame", "last_mean_rewards", "env_state", PK.OUR_KEY]
    assert list(ck["model"]) == ["a2c_network." + k for k, _ in EXPECT]
    for k, s in EXPECT:
        t = ck["model"]["a2c_network." + k]
        assert tuple(t.shape) == s and t.dtype == torch.float32 and t.is_contiguous() and t.device.type == "cpu", (k, t.shape, t.dtype)
    assert ck["scaler"] == {}          # (a disabled GradScaler's state_dict)
    assert ck["epoch"] == 3 and ck["frame"] == 192 and ck["last_mean_rewards"] == -100500 and ck["env_state"] is None
    for key, lr in (("optimizer_actor", 1e-5), ("optimizer_critic", 5e-4)):
        pg = ck[key]["param_groups"]
        assert len(pg) == 1 and pg[0]["params"] == list(range(6)) and pg[0]["lr"] == lr
        assert tuple(pg[0]["betas"]) == (0.9, 0.999) and pg[0]["eps"] == 1e-8 and pg[0]["weight_decay"] == 0
        assert not pg[0]["capturable"] and not pg[0]["fused"]
        assert sorted(ck[key]["state"]) == list(range(6))
    names = dict(EXPECT)
    for key, keys in (("optimizer_actor", PK.ACTOR_OPT_KEYS), ("optimizer_critic", PK.CRITIC_OPT_KEYS)):
        for i, k in enumerate(keys):
            e = ck[key]["state"][i]
            assert float(e["step"]) == 1 and tuple(e["exp_avg"].shape) == names[k] and tuple(e["exp_avg_sq"].shape) == names[k], (key, k)
    ours = ck[PK.OUR_KEY]
    assert ours == {"lr0": 1e-5, "lr_min": 3e-6, "max_epochs": 5000, "sigma_init": net.sigma_init, "sigma_last": net.sigma_last, "backend": "torch"}


def test_layout_follows_the_reference_sources():
    """The order above rests on these lines of the reference; where its checkout is present, they are read."""
    if not os.path.isdir(REF):
        pytest.skip("the reference checkout is not mounted")
    a2c = open(os.path.join(REF, "a2c_common_dyros.py")).read()
    full = a2c[a2c.index("def get_full_state_weights"):a2c.index("def set_full_state_weights")]
    order = ["state['epoch']", "state['optimizer_actor']", "state['optimizer_critic']", "state['frame']", "state['last_mean_rewards']", "state['env_state']"]
    pos = [full.index(s) for s in order]
    assert pos == sorted(pos)
    weights = a2c[a2c.index("def get_weights"):a2c.index("def set_stats_weights")]
    assert weights.index("get_stats_weights()") < weights.index("state['model']")
    assert "if self.mixed_precision:\n            state['scaler'] = self.scaler.state_dict()" in weights
    assert "weights.get('last_mean_rewards', -100500)" in a2c
    sep = open(os.path.join(REF, "a2c_continuous_seperate.py")).read()
    assert "list(self.model.a2c_network.actor_mlp.parameters()) + list(self.model.a2c_network.mu.parameters())" in sep
    assert "list(self.model.a2c_network.critic_mlp.parameters()) + list(self.model.a2c_network.value.parameters())" in sep
    assert "lr=float(5e-4), eps=1e-08" in sep
    nb = open(os.path.join(REF, "network_builder_dyros.py")).read()
    pos = [nb.index(s) for s in ("self.actor_cnn = nn.Sequential()", "self.actor_mlp = nn.Sequential()", "self.critic_mlp = nn.Sequential()",
                                 "self.value = torch.nn.Linear", "self.mu = torch.nn.Linear", "self.sigma = nn.Parameter")]
    assert pos == sorted(pos)
    runner = open(os.path.join(REF, "torch_runner_dyros.py")).read()
    assert 'name= name.replace(".","_")' in runner and "np.savetxt(weight_file_name, param.data)" in runner


class RefNet(nn.Module):
    """The registration order of network_builder_dyros.py's Network (empty cnns, then the trunks and heads; sigma a direct parameter)."""

    def __init__(self):
        super().__init__()
        self.actor_cnn, self.critic_cnn = nn.Sequential(), nn.Sequential()
        self.actor_mlp = nn.Sequential(nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU())
        self.critic_mlp = nn.Sequential(nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU())
        self.value = nn.Linear(H, 1)
        self.mu = nn.Linear(H, A)
        self.sigma = nn.Parameter(torch.zeros(A), requires_grad=False)


class RefModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.a2c_network = RefNet()


def test_optimizers_load_into_plain_adams_in_the_reference_order():
    net, oa, oc, sc = trained(2)
    ck = PK.state(net, epoch=2, opt_actor=oa, opt_critic=oc, scaler=sc)
    m = RefModel()
    assert list(m.state_dict()) == list(ck["model"])
    m.load_state_dict(ck["model"])
    r = m.a2c_network
    ra = torch.optim.Adam(list(r.actor_mlp.parameters()) + list(r.mu.parameters()), lr=1.0, eps=1e-08)
    rc = torch.optim.Adam(list(r.critic_mlp.parameters()) + list(r.value.parameters()), lr=float(5e-4), eps=1e-08)
    ra.load_state_dict(ck["optimizer_actor"]); rc.load_state_dict(ck["optimizer_critic"])
    assert ra.param_groups[0]["lr"] == oa.param_groups[0]["lr"]
    for ours, ref in ((net.actor_parameters(), ra), (net.critic_parameters(), rc)):
        for p_own, p_ref in zip(ours, ref.param_groups[0]["params"]):
            for part in ("exp_avg", "exp_avg_sq"):
                same(ref.state[p_ref][part], oa.state[p_own][part] if ref is ra else oc.state[p_own][part], part)
    # and they step: one Adam step on the reference's module equals one on ours
    for opt in (ra, rc):
        for p in opt.param_groups[0]["params"]:
            p.grad = torch.full_like(p, 0.01)
    for p in net.actor_parameters() + net.critic_parameters():
        p.grad = torch.full_like(p, 0.01)
    ra.step(); rc.step(); oa.step(); oc.step()
    for k, v in net.state_dict().items():
        same(v, m.state_dict()["a2c_network." + k], k)


class FusedStub:
    """FusedPpoUpdate's checkpoint surface on the CPU: its state words, moments in the padded layout, and the calls restore makes."""

    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.dev = torch.device("cpu")
        self.state = torch.zeros(U.K["DWP_S_WORDS"])
        self.m, self.v = torch.zeros(U.NP), torch.zeros(U.NP)
        for flat in (self.m, self.v):
            for k, t in WP.tensor_views(flat).items():
                t.copy_(torch.rand(t.shape, generator=g) * 1e-3)
        S = U.K
        self.state[S["DWP_S_SCALE"]], self.state[S["DWP_S_GROWTH"]] = 32768.0, 17.0
        self.state[S["DWP_S_STEP"]], self.state[S["DWP_S_STEP"] + 1] = 40.0, 42.0
        self.state[S["DWP_S_LR"]], self.state[S["DWP_S_LR"] + 1] = 9.5e-6, 5e-4
        self.synced = False

    def load_state_dict(self, d):
        self.m.copy_(d["m"]); self.v.copy_(d["v"])
        self.state[U.K["DWP_S_SCALE"]], self.state[U.K["DWP_S_GROWTH"]] = d["scale"], d["growth"]
        self.state[U.K["DWP_S_STEP"]:U.K["DWP_S_STEP"] + 2] = torch.tensor(d["steps"])

    def set_learning_rates(self, a, c):
        self.state[U.K["DWP_S_LR"]:U.K["DWP_S_LR"] + 2] = torch.tensor([a, c])

    def sync_policy_copy(self):
        self.synced = True


def test_fused_layout_is_cut_per_parameter_and_back():
    net, _oa, _oc, _sc = learner(1)
    fu = FusedStub(3)
    ck = PK.state(net, epoch=5, frame=10, fused=fu)
    assert ck[PK.OUR_KEY]["backend"] == "fused"
    assert ck["scaler"] == {"scale": 32768.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 17}
    assert np.float32(ck["optimizer_actor"]["param_groups"][0]["lr"]) == np.float32(9.5e-6)
    mv = WP.tensor_views(fu.m)
    for key, keys, step in (("optimizer_actor", PK.ACTOR_OPT_KEYS, 40.0), ("optimizer_critic", PK.CRITIC_OPT_KEYS, 42.0)):
        for i, k in enumerate(keys):
            e = ck[key]["state"][i]
            assert float(e["step"]) == step and e["exp_avg"].is_contiguous()
            same(e["exp_avg"], mv[k].contiguous(), (key, k))
    # ... into the eager optimisers (a plain GradScaler takes the scaler dict) and back into a fresh stub: the same words, pads zero
    net2, oa2, oc2, _ = learner(2)
    sc2 = torch.amp.GradScaler("cuda", enabled=False)
    PK.restore(ck, net2, opt_actor=oa2, opt_critic=oc2, scaler=sc2)
    ck2 = PK.state(net2, epoch=5, opt_actor=oa2, opt_critic=oc2)
    fu2 = FusedStub(4)
    fu2.m.fill_(7.0); fu2.v.fill_(7.0)          # (pads must come back zero)
    PK.restore(ck2, net2, fused=fu2)
    fu2.state[U.K["DWP_S_SCALE"]], fu2.state[U.K["DWP_S_GROWTH"]] = 32768.0, 17.0          # (a CPU-side file has no scaler: the stub keeps its own)
    same(fu2.m, fu.m, "m"); same(fu2.v, fu.v, "v")
    assert fu2.synced
    assert fu2.state[U.K["DWP_S_STEP"]:U.K["DWP_S_STEP"] + 2].tolist() == [40.0, 42.0]
    assert np.float32(float(fu2.state[U.K["DWP_S_LR"]])) == np.float32(9.5e-6)


def test_save_restore_bit_identical(tmp_path):
    L = trained(2)
    net, oa, oc, sc = L
    path = PK.save(str(tmp_path / "nn" / "x.pth"), net, epoch=2, frame=128, opt_actor=oa, opt_critic=oc, scaler=sc, lr0=1e-5, lr_min=3e-6,
                   max_epochs=5000)
    L2 = learner(seed=7)
    c = PK.restore(path, L2[0], opt_actor=L2[1], opt_critic=L2[2], scaler=L2[3])
    assert c == {"epoch": 2, "frame": 128, "last_mean_rewards": -100500, "lr0": 1e-5, "lr_min": 3e-6, "max_epochs": 5000}
    assert_same(L, L2)
    # a file without our key (the reference learner's) restores weights and optimisers
    ck = torch.load(path, weights_only=True)
    del ck[PK.OUR_KEY]
    L3 = learner(seed=8)
    c = PK.restore(ck, L3[0], opt_actor=L3[1], opt_critic=L3[2], scaler=L3[3])
    assert c["epoch"] == 2 and c["lr0"] is None
    assert_same(L, L3)


def test_resume_equivalence(tmp_path):
    L = trained(3)
    path = PK.save(str(tmp_path / "r.pth"), L[0], epoch=3, opt_actor=L[1], opt_critic=L[2], scaler=L[3])
    L2 = learner(seed=5)
    PK.restore(path, L2[0], opt_actor=L2[1], opt_critic=L2[2], scaler=L2[3])
    nxt = batch(99)
    update(*L, nxt, lr=7e-6)
    update(*L2, nxt, lr=7e-6)
    assert_same(L, L2)


def test_export_txt_names_and_values(tmp_path):
    net, oa, oc, sc = trained(1)
    ck = PK.state(net, epoch=1, opt_actor=oa, opt_critic=oc, scaler=sc)
    out = PK.export_txt(ck, str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    expect = sorted("a2c_network_" + k.replace(".", "_") + ".txt" for k, _ in EXPECT)
    assert len(expect) == 13 and names == expect and sorted(os.path.basename(p) for p in out) == expect
    assert "a2c_network_actor_mlp_0_weight.txt" in names and "a2c_network_sigma.txt" in names and "a2c_network_value_bias.txt" in names
    for k, t in ck["model"].items():
        back = np.loadtxt(tmp_path / (k.replace(".", "_") + ".txt"), dtype=np.float64).astype(np.float32).reshape(t.shape)
        assert np.array_equal(back.view(np.uint32), t.numpy().view(np.uint32)), k
    line = open(tmp_path / "a2c_network_mu_weight.txt").readline().split()          # np.savetxt's defaults: '%.18e', space separated
    assert len(line) == H and all(re.fullmatch(r"-?\d\.\d{18}e[+-]\d\d", x) for x in line)


def test_load_policy_torch_backend_plays_the_actor(tmp_path):
    net, oa, oc, sc = trained(1)
    path = PK.save(str(tmp_path / "p.pth"), net, epoch=1, opt_actor=oa, opt_critic=oc, scaler=sc)
    pol = PK.load_policy(path, "cpu", backend="torch")
    obs, noise = torch.randn(5, D), torch.randn(5, A)
    with torch.no_grad():
        mu = net.mu(net.actor_mlp(obs))
    cl, pm = pol.play(obs)
    same(pm, mu, "mu")
    same(cl, torch.clamp(mu, -1.0, 1.0), "clamped")
    cl, _ = pol.play(obs, noise)
    same(cl, torch.clamp(mu + torch.exp(net.sigma) * noise, -1.0, 1.0), "stochastic")
    with pytest.raises(ValueError):
        pol.play(torch.zeros(5, D - 1))


class PlumbingEnv:
    """The VecTask surface train() touches; dynamics = noise (as tests/test_ppo_consumer.py's sharded test)."""
    num_envs, num_obs, num_acts = 32, U.IN, U.ACT

    def __init__(self):
        self.g = torch.Generator().manual_seed(100)
        self.extras = {}
        self.episodes_finished = torch.zeros(32)
        self.epi_len_log = torch.zeros(32)

    def reset(self):
        return {"obs": torch.zeros(32, self.num_obs)}

    def step(self, a):
        o = torch.randn(32, self.num_obs, generator=self.g) + a.sum(1, keepdim=True)
        return {"obs": o}, o[:, 0].tanh(), (torch.rand(32, generator=self.g) < 0.05).long(), {}


def test_train_saves_and_resumes_on_cpu(tmp_path):
    cfg = {"network": PPO.TRAIN_CFG["network"], "config": dict(C, horizon_length=8, minibatch_size=128, mini_epochs=1)}
    lines = []
    full = PPO.train(epochs=2, device="cpu", cfg=cfg, env=PlumbingEnv(), log=lines.append, output_dir=str(tmp_path), save_frequency=1)
    nn_dir = tmp_path / "DyrosDynamicWalk" / "nn"
    assert sorted(os.listdir(nn_dir)) == ["DyrosDynamicWalk.pth", "DyrosDynamicWalk_1.pth", "DyrosDynamicWalk_2.pth"]
    for name, ep in (("DyrosDynamicWalk_1.pth", 1), ("DyrosDynamicWalk_2.pth", 2), ("DyrosDynamicWalk.pth", 2)):
        ck = torch.load(nn_dir / name, weights_only=True)
        assert ck["epoch"] == ep and ck["frame"] == ep * 8 * 32 and ck["scaler"] == {} and ck[PK.OUR_KEY]["backend"] == "torch"
        assert ck[PK.OUR_KEY]["max_epochs"] == C["max_epochs"] and ck[PK.OUR_KEY]["lr0"] == C["learning_rate"]
        assert float(ck["optimizer_actor"]["state"][0]["step"]) == ep * (8 * 32 // 128)
    assert [s["frame"] for s in full] == [256, 512]
    lines2 = []
    res = PPO.train(epochs=1, device="cpu", cfg=cfg, env=PlumbingEnv(), log=lines2.append, checkpoint=str(nn_dir / "DyrosDynamicWalk_1.pth"))
    assert [s["epoch"] for s in res] == [2] and any(x.startswith("epoch 2:") for x in lines2), lines2
    assert res[0]["lr"] == full[1]["lr"] and res[0]["sigma"] == full[1]["sigma"] and res[0]["frame"] == full[1]["frame"]
    assert math.isfinite(res[0]["a_loss"])
    assert len(os.listdir(nn_dir)) == 3          # (no output_dir: nothing written)
