"""The AMP discriminator of TocabiAMPLower's learner (include/dyros_amp_disc.h, csrc/dw_amp_disc.hip).

Reference (python/IsaacGymEnvs/isaacgymenvs/): learning/amp_continuous.py with cfg/train/TocabiAMPLowerPPO.yaml (`algo: amp_continuous`).
  * network (learning/amp_network_builder.py:74-110): `_disc_mlp` = Linear(D, 256), ReLU, Linear(256, 256), ReLU; `_disc_logits` =
    Linear(256, 1); fp32 (`mixed_precision: False`).  The MLP weights get the yaml's `initializer: default`, which in rl_games' init factory
    is `nn.Identity()` applied to the weight: a no-op, so they keep torch's own nn.Linear initialisation (kaiming_uniform_ with a = sqrt(5),
    i.e. U(-1/sqrt(fan_in), 1/sqrt(fan_in))); the MLP biases are zeroed.  The logit weight is U(-1, 1) (DISC_LOGIT_INIT_SCALE), its bias 0.
  * input normalisation (`normalize_amp_input: True`): rl_games' RunningMeanStd, which is not part of the reference's checkout; restated
    here (`RunningMeanStd`): per-feature running mean and variance kept in fp64; a batch contributes its mean and UNBIASED variance (torch.var)
    combined with the running values by count (parallel-variance formula); the initial count is the epsilon 1e-5 (mean 0, var 1); the output
    is (x - mean) / sqrt(var + 1e-5) with the statistics cast to fp32, clamped to +-5.  In train mode every call updates first, then
    normalises: `calc_gradients` (amp_continuous.py:273-280) therefore normalises the agent rows, then the replay rows, then the demo rows,
    each with the statistics left by the update with its own rows.  In `play_steps` (eval mode) the statistics do not move.
  * reward (`_calc_disc_rewards`, :522-532, `_combine_rewards`, :505-509): disc_r = -log(max(1 - sigmoid(logit), 1e-4)) * disc_reward_scale,
    combined = task_reward_w * task_reward + disc_reward_w * disc_r.
  * loss (`_disc_loss`, :404-457): 0.5 (BCE(agent + replay logits, 0) + BCE(demo logits, 1)) + disc_logit_reg sum(w_logit^2) +
    disc_grad_penalty mean_rows |d logit / d x_demo|^2 (x_demo normalised, create_graph=True) + disc_weight_decay sum(every weight^2), times
    disc_coef; Adam (eps 1e-8) at the learner's learning rate, no gradient clipping (`truncate_grads: False`).
  * buffers (learning/replay_buffer.py, amp_continuous.py:470-498, 534-543): `ReplayBuffer`.

Two backends of one class: `backend="hip"` (the product: dwd_reward, dwd_stats, dwd_grad, dwd_opt) and `backend="torch"` (the reference's own
arithmetic with nn.Linear, BCEWithLogitsLoss and autograd.grad(create_graph=True): the yardstick of the tests and the CPU form).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import cbind

K = cbind.constants("dyros_amp_disc.h", "dwd_")
HID, OBS_STEP, D_MAX = K["DWD_HID"], K["DWD_OBS_STEP"], K["DWD_D_MAX"]
LOG_NAMES = ["disc_loss", "disc_pred_loss", "disc_logit_loss", "disc_grad_penalty", "disc_weight_decay", "disc_agent_logit", "disc_demo_logit",
             "disc_agent_acc", "disc_demo_acc"]
DISC_LOGIT_INIT_SCALE = 1.0
RMS_EPS = 1e-5

# cfg/train/TocabiAMPLowerPPO.yaml, the keys this learner reads
TRAIN_CFG = {
    "network": {"mlp_units": [512, 512], "activation": "relu", "disc_units": [256, 256], "disc_activation": "relu", "sigma_init": -1.6,
                "sigma_last": -2.99, "fixed_sigma": True, "learn_sigma": False},
    "config": {"mixed_precision": False, "normalize_input": True, "normalize_value": True, "value_bootstrap": True, "reward_scale": 1,
               "normalize_advantage": True, "gamma": 0.99, "tau": 0.95, "learning_rate": 1e-4, "lr_schedule": "linear", "kl_threshold": 0.008,
               "max_epochs": 5000, "grad_norm": 1.0, "entropy_coef": 0.0, "truncate_grads": False, "e_clip": 0.2, "horizon_length": 32,
               "minibatch_size": 131072, "mini_epochs": 6, "critic_coef": 5, "clip_value": False, "bounds_loss_coef": 10,
               "amp_obs_demo_buffer_size": 200000, "amp_replay_buffer_size": 1000000, "amp_replay_keep_prob": 0.01, "amp_batch_size": 512,
               "amp_minibatch_size": 131072, "disc_coef": 5, "disc_logit_reg": 0.05, "disc_grad_penalty": 0.1, "disc_reward_scale": 2,
               "disc_weight_decay": 0.0001, "normalize_amp_input": True, "task_reward_w": 0.7, "disc_reward_w": 0.3},
}


def load_train_yaml(path: str, **root_overrides) -> dict:
    """TRAIN_CFG's keys from the reference's cfg/train/TocabiAMPLowerPPO.yaml (interpolations resolved as examples/ppo_consumer.py does)."""
    import yaml
    from .config import ROOT_DEFAULTS, _resolve
    root = dict(ROOT_DEFAULTS, checkpoint="", experiment="", max_iterations="", multi_gpu=False, **root_overrides)
    root["task"] = {"env": {"numEnvs": root.get("num_envs") or 4096}}

    def walk(x):
        if isinstance(x, dict):
            return {k: walk(v) for k, v in x.items()}
        if isinstance(x, list):
            return [walk(v) for v in x]
        if isinstance(x, str) and "task.env.numEnvs" in x:
            return root["task"]["env"]["numEnvs"]
        if isinstance(x, str) and ".name}" in x:
            return x
        return _resolve(x, root)
    p = walk(yaml.safe_load(open(path)))["params"]
    net, c = p["network"], p["config"]
    sp = net["space"]["continuous"]
    out = {"network": {"mlp_units": net["mlp"]["units"], "activation": net["mlp"]["activation"], "disc_units": net["disc"]["units"],
                       "disc_activation": net["disc"]["activation"], "sigma_init": sp["sigma_init"]["val"], "sigma_last": sp["sigma_last"]["val"],
                       "fixed_sigma": sp["fixed_sigma"], "learn_sigma": sp["learn_sigma"]},
           "config": {k: c[k] for k in TRAIN_CFG["config"] if k != "reward_scale"}}
    out["config"]["reward_scale"] = c["reward_shaper"]["scale_value"]
    out["config"]["learning_rate"] = float(out["config"]["learning_rate"])
    out["config"]["max_epochs"] = int(out["config"]["max_epochs"])
    return out


class RunningMeanStd(nn.Module):
    """rl_games' RunningMeanStd as the reference uses it (restated: rl_games is not in the reference's checkout; see the module docstring)."""

    def __init__(self, insize: int, epsilon: float = RMS_EPS):
        super().__init__()
        self.epsilon = epsilon
        self.register_buffer("running_mean", torch.zeros(insize, dtype=torch.float64))
        self.register_buffer("running_var", torch.ones(insize, dtype=torch.float64))
        self.register_buffer("count", torch.full((), epsilon, dtype=torch.float64))

    @staticmethod
    def combine(mean, var, count, batch_mean, batch_var, batch_count):
        delta = batch_mean - mean
        tot = count + batch_count
        new_mean = mean + delta * batch_count / tot
        m2 = var * count + batch_var * batch_count + delta ** 2 * count * batch_count / tot
        return new_mean, m2 / tot, tot

    def forward(self, x):
        if self.training:
            m, v, n = self.combine(self.running_mean, self.running_var, self.count, x.mean(0), x.var(0), x.shape[0])
            self.running_mean.copy_(m)
            self.running_var.copy_(v)
            self.count.copy_(torch.as_tensor(n, dtype=torch.float64))
        y = (x - self.running_mean.float()) / torch.sqrt(self.running_var.float() + self.epsilon)
        return torch.clamp(y, min=-5.0, max=5.0)


class DiscNet(nn.Module):
    """_disc_mlp / _disc_logits of AMPBuilder.Network (parameter names as the reference's state_dict has them)."""

    def __init__(self, num_amp_obs: int, units=(HID, HID)):
        super().__init__()
        layers, n = [], num_amp_obs
        for u in units:
            layers += [nn.Linear(n, u), nn.ReLU()]
            n = u
        self._disc_mlp = nn.Sequential(*layers)
        self._disc_logits = nn.Linear(n, 1)
        for m in self._disc_mlp.modules():
            if isinstance(m, nn.Linear):          # (initializer `default`: the weight keeps nn.Linear's own initialisation)
                nn.init.zeros_(m.bias)
        nn.init.uniform_(self._disc_logits.weight, -DISC_LOGIT_INIT_SCALE, DISC_LOGIT_INIT_SCALE)
        nn.init.zeros_(self._disc_logits.bias)

    def forward(self, x):
        return self._disc_logits(self._disc_mlp(x))

    def weights(self):
        return [m.weight for m in self._disc_mlp.modules() if isinstance(m, nn.Linear)] + [self._disc_logits.weight]


def torch_disc_loss(net: DiscNet, an, rn, dn, disc_coef, logit_reg, grad_penalty, weight_decay):
    """disc_coef * _disc_loss (amp_continuous.py:404-457) on normalised agent / replay / demo rows, in the module's dtype: (total, the logged
    values in the order of LOG_NAMES).  dn gets requires_grad here (the gradient penalty is taken with respect to it)."""
    dn.requires_grad_(True)
    agent_logit = torch.cat([net(an), net(rn)], dim=0)
    demo_logit = net(dn)
    bce = nn.BCEWithLogitsLoss()
    pred = 0.5 * (bce(agent_logit, torch.zeros_like(agent_logit)) + bce(demo_logit, torch.ones_like(demo_logit)))
    logit_loss = torch.sum(torch.square(net._disc_logits.weight.flatten()))
    loss = pred + logit_reg * logit_loss
    gd = torch.autograd.grad(demo_logit, dn, grad_outputs=torch.ones_like(demo_logit), create_graph=True, retain_graph=True, only_inputs=True)[0]
    gp = torch.mean(torch.sum(torch.square(gd), dim=-1))
    loss = loss + grad_penalty * gp
    wd = torch.sum(torch.square(torch.cat([w.flatten() for w in net.weights()])))
    if weight_decay != 0:
        loss = loss + weight_decay * wd
    total = disc_coef * loss
    # the accuracies as _compute_disc_acc takes them: means of fp32 flags whatever the module's dtype
    return total, [total, pred, logit_loss, gp, wd, agent_logit.mean(), demo_logit.mean(), (agent_logit < 0).float().mean(),
                   (demo_logit > 0).float().mean()]


class ReplayBuffer:
    """learning/replay_buffer.py for one key (`amp_obs`): a circular store; `sample(n)` walks a random permutation of the buffer's slots from
    a moving head and, while the buffer has never been filled, takes the slot modulo the write head.  `generator`: the torch.Generator of the
    permutations (the reference draws from torch's global one)."""

    def __init__(self, buffer_size: int, device, generator: torch.Generator = None):
        self._head, self._total_count, self._buffer_size = 0, 0, int(buffer_size)
        self._device, self._gen = device, generator
        self._data = None
        self._sample_idx = torch.randperm(self._buffer_size, generator=generator)
        self._sample_head = 0

    def get_buffer_size(self):
        return self._buffer_size

    def get_total_count(self):
        return self._total_count

    def store(self, x: torch.Tensor):
        if self._data is None:
            self._data = torch.zeros((self._buffer_size,) + tuple(x.shape[1:]), device=self._device)
        n = x.shape[0]
        if not n < self._buffer_size:
            raise ValueError("ReplayBuffer.store: %d rows do not fit a buffer of %d" % (n, self._buffer_size))
        k = min(n, self._buffer_size - self._head)
        self._data[self._head:self._head + k] = x[:k]
        if n > k:
            self._data[0:n - k] = x[k:]
        self._head = (self._head + n) % self._buffer_size
        self._total_count += n

    def sample_indices(self, n: int) -> torch.Tensor:
        idx = torch.arange(self._sample_head, self._sample_head + n) % self._buffer_size
        rand_idx = self._sample_idx[idx]
        if self._total_count < self._buffer_size:
            rand_idx = rand_idx % self._head
        self._sample_head += n
        if self._sample_head >= self._buffer_size:
            self._sample_idx[:] = torch.randperm(self._buffer_size, generator=self._gen)
            self._sample_head = 0
        return rand_idx

    def sample(self, n: int) -> torch.Tensor:
        return self._data[self.sample_indices(n).to(self._data.device)]


def _req(name, t, dtype, device, shape):
    """A tensor whose data_ptr() goes to a kernel: exactly this dtype, contiguous, on this device, of this shape -- or ValueError."""
    if not torch.is_tensor(t):
        raise ValueError("%s: a tensor is required, got %r" % (name, type(t).__name__))
    if t.dtype != dtype:
        raise ValueError("%s: dtype %s, expected %s" % (name, t.dtype, dtype))
    if not t.is_contiguous():
        raise ValueError("%s: must be contiguous (shape %r, strides %r)" % (name, tuple(t.shape), t.stride()))
    if t.device != device:
        raise ValueError("%s: must live on %s (it is on %s)" % (name, device, t.device))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: shape %r, expected %r" % (name, tuple(t.shape), tuple(shape)))
    return t


DwdLoss = cbind.structs("dyros_amp_disc.h", "dwd_")["DwdLoss"]
EXPORTS = list(cbind.signatures("dyros_amp_disc.h", "dwd_"))


def declare(lib: C.CDLL) -> dict:
    return cbind.declare(lib, "dyros_amp_disc.h", "dwd_")


class AmpDiscriminator:
    """The discriminator, its input statistics, its optimiser state and the two AMP buffers of amp_continuous.

    cfg: TRAIN_CFG (or load_train_yaml's dict); backend "hip" (the kernels; a CUDA device) or "torch" (the reference's arithmetic)."""

    def __init__(self, num_amp_obs: int, device, cfg: dict = None, backend: str = "hip", seed: int = None):
        cfg = cfg or TRAIN_CFG
        c, net = cfg["config"], cfg["network"]
        D = int(num_amp_obs)
        if D < OBS_STEP or D > D_MAX or D % OBS_STEP:
            raise ValueError("num_amp_obs %d: must be a multiple of %d up to %d (numAMPObsSteps <= 10)" % (D, OBS_STEP, D_MAX))
        if list(net.get("disc_units", [HID, HID])) != [HID, HID] or net.get("disc_activation", "relu") != "relu":
            raise ValueError("the discriminator is fixed at units [256, 256] with relu (cfg/train/TocabiAMPLowerPPO.yaml)")
        if c.get("mixed_precision", False):
            raise ValueError("the discriminator runs in fp32 only (mixed_precision: False)")
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        self.device, self.D, self.backend = torch.device(device), D, backend
        if backend == "hip" and self.device.type != "cuda":
            raise ValueError("backend 'hip' needs a GPU device (use backend='torch' on the CPU)")
        self.coef = dict(disc_coef=float(c["disc_coef"]), logit_reg=float(c["disc_logit_reg"]), grad_penalty=float(c["disc_grad_penalty"]),
                         weight_decay=float(c["disc_weight_decay"]))
        self.reward_scale, self.task_w, self.disc_w = float(c["disc_reward_scale"]), float(c["task_reward_w"]), float(c["disc_reward_w"])
        self.normalize = bool(c.get("normalize_amp_input", True))
        if not self.normalize:
            raise ValueError("normalize_amp_input: False is not supported (the yaml has True)")
        if seed is not None:
            torch.manual_seed(seed)
        self.net = DiscNet(D)
        self.rms = RunningMeanStd(D)
        NP = D * HID + HID + HID * HID + HID + HID + 1
        assert NP == sum(t.numel() for t in self.net.parameters())
        # one flat fp32 buffer in the layout of include/dyros_amp_disc.h; the module's parameters are views of it
        self.p = torch.cat([t.detach().reshape(-1) for t in self._params_in_layout()]).to(self.device)
        self.net.to(self.device)
        o = 0
        for t in self._params_in_layout():
            t.data = self.p[o:o + t.numel()].view_as(t)
            o += t.numel()
        self.g, self.m, self.v = (torch.zeros_like(self.p) for _ in range(3))
        self.stats = torch.cat([self.rms.running_mean, self.rms.running_var, self.rms.count.reshape(1)]).to(self.device)
        self.rms.to(self.device)
        self.rms.running_mean, self.rms.running_var, self.rms.count = self.stats[:D], self.stats[D:2 * D], self.stats[2 * D]
        self.snap = torch.zeros(2, 2 * D + 1, dtype=torch.float64, device=self.device)          # agent / replay snapshots of one update
        self.state = torch.zeros(K["DWD_S_WORDS"], dtype=torch.float32, device=self.device)
        self.state[K["DWD_S_LR"]] = float(c["learning_rate"])
        self._work, self._work_key = None, None
        if backend == "hip":
            from . import _lib
            self.lib = _lib.load()[0]
            self.api = declare(self.lib)
            self._swork = torch.empty(self.api["stats_workspace_bytes"](D) // 8, dtype=torch.float64, device=self.device)
        else:
            self.opt = torch.optim.Adam(self.net.parameters(), lr=float(c["learning_rate"]), eps=1e-8)
        self.demo_buffer = ReplayBuffer(int(c["amp_obs_demo_buffer_size"]), self.device)
        self.replay_buffer = ReplayBuffer(int(c["amp_replay_buffer_size"]), self.device)
        self.replay_keep_prob, self.amp_batch_size = float(c["amp_replay_keep_prob"]), int(c["amp_batch_size"])

    def _params_in_layout(self):
        n = self.net
        return [n._disc_mlp[0].weight, n._disc_mlp[0].bias, n._disc_mlp[2].weight, n._disc_mlp[2].bias, n._disc_logits.weight, n._disc_logits.bias]

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, rc):
        cbind.check(self.api, rc)

    # ------------------------------------------------------------------------------------------------------------- the reward
    def rewards(self, amp_obs: torch.Tensor, task_rewards: torch.Tensor, return_logits: bool = False):
        """amp_obs [H, N, D], task_rewards [H, N, 1] -> (combined [H, N, 1], disc_r [H, N, 1]) (+ logits [H, N, 1]); the statistics stay."""
        if not torch.is_tensor(amp_obs) or amp_obs.dim() != 3:
            raise ValueError("amp_obs: a [H, N, D] tensor is required")
        H, N = int(amp_obs.shape[0]), int(amp_obs.shape[1])
        _req("amp_obs", amp_obs, torch.float32, self.device, (H, N, self.D))
        _req("task_rewards", task_rewards, torch.float32, self.device, (H, N, 1))
        if H * N < 1:
            raise ValueError("amp_obs: no rows")
        if self.backend == "torch":
            with torch.no_grad():
                self.rms.eval()
                logits = self.net(self.rms(amp_obs))
                prob = 1 / (1 + torch.exp(-logits))
                disc_r = -torch.log(torch.maximum(1 - prob, torch.tensor(0.0001, device=self.device))) * self.reward_scale
                combined = self.task_w * task_rewards + self.disc_w * disc_r
        else:
            disc_r, combined, logits = (torch.empty(H, N, 1, device=self.device) for _ in range(3))
            self._check(self.api["reward"](self.p.data_ptr(), self.stats.data_ptr(), amp_obs.data_ptr(), task_rewards.data_ptr(), H * N, self.D,
                                           self.reward_scale, self.task_w, self.disc_w, disc_r.data_ptr(), combined.data_ptr(),
                                           logits.data_ptr(), self._stream()))
        return (combined, disc_r, logits) if return_logits else (combined, disc_r)

    # ------------------------------------------------------------------------------------------------------------- one minibatch
    def _rows(self, name, x, allow_empty=False):
        if not torch.is_tensor(x) or x.dim() != 2:
            raise ValueError("%s: a [B, D] tensor is required" % name)
        _req(name, x, torch.float32, self.device, (x.shape[0], self.D))
        if x.shape[0] < (0 if allow_empty else 2):
            raise ValueError("%s: at least 2 rows are required (the running statistics take an unbiased variance)" % name)
        return x

    def accumulate_grad(self, amp_obs, amp_obs_replay, amp_obs_demo):
        """g += d(disc_coef * disc_loss) / dp for one minibatch (train mode: the statistics move three times); the logged values are added to
        `state`.  No optimiser step."""
        a, r, d = self._rows("amp_obs", amp_obs), self._rows("amp_obs_replay", amp_obs_replay), self._rows("amp_obs_demo", amp_obs_demo)
        if self.backend == "torch":
            return self._torch_grad(a, r, d)
        api, s, D = self.api, self._stream(), self.D
        key = (a.shape[0], r.shape[0], d.shape[0])
        if self._work_key != key:
            nb = api["grad_workspace_bytes"](D, *key)
            if nb < 0:
                raise ValueError("dwd_grad: rows %r" % (key,))
            self._work, self._work_key = torch.empty((nb + 3) // 4, dtype=torch.float32, device=self.device), key
        st, sn, sw = self.stats.data_ptr(), self.snap.data_ptr(), self._swork.data_ptr()
        s1 = sn + 8 * (2 * D + 1)
        self._check(api["stats"](a.data_ptr(), a.shape[0], D, st, sn, sw, s))
        self._check(api["stats"](r.data_ptr(), r.shape[0], D, sn, s1, sw, s))
        self._check(api["stats"](d.data_ptr(), d.shape[0], D, s1, st, sw, s))
        self._check(api["grad"](self.p.data_ptr(), a.data_ptr(), a.shape[0], r.data_ptr(), r.shape[0], d.data_ptr(), d.shape[0], D, sn, s1, st,
                                DwdLoss(**self.coef), self.g.data_ptr(), self.state.data_ptr(), self._work.data_ptr(), self._work.numel() * 4, s))

    def _torch_grad(self, a, r, d):
        """amp_continuous.calc_gradients' discriminator share, as the reference writes it."""
        self.rms.train()
        an, rn, dn = self.rms(a), self.rms(r), self.rms(d)
        total, vals = torch_disc_loss(self.net, an, rn, dn, **self.coef)
        grads = torch.autograd.grad(total, self._params_in_layout())
        with torch.no_grad():
            self.g += torch.cat([x.reshape(-1) for x in grads])
            self.state[:len(vals)] += torch.stack([v.detach().float() for v in vals])
            self.state[K["DWD_S_UPDATES"]] += 1

    def step(self, lr: float = None):
        """One Adam step with g (lr: written to the device word first; None: the word as it is, e.g. inside a replayed graph), then g = 0."""
        if lr is not None:
            self.set_lr(lr)
        if self.backend == "torch":
            for pg in self.opt.param_groups:
                pg["lr"] = float(self.state[K["DWD_S_LR"]])
            o = 0
            for t in self._params_in_layout():
                t.grad = self.g[o:o + t.numel()].view_as(t).clone()
                o += t.numel()
            self.opt.step()
            self.g.zero_()
            self.state[K["DWD_S_STEP"]] += 1
            return
        self._check(self.api["opt"](self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.state.data_ptr(), self.D,
                                    self._stream()))

    def set_lr(self, lr: float):
        self.state[K["DWD_S_LR"]] = float(lr)

    def update(self, amp_obs, amp_obs_replay, amp_obs_demo, lr: float = None) -> dict:
        """One minibatch of the discriminator: statistics (agent, replay, demo), loss gradient, Adam step.  Returns the logged sums so far
        (device tensors; `pop_info` turns them into means and clears them)."""
        self.accumulate_grad(amp_obs, amp_obs_replay, amp_obs_demo)
        self.step(lr)
        return {k: self.state[i] for i, k in enumerate(LOG_NAMES)}

    def pop_info(self) -> dict:
        """The logged values averaged over the minibatches since the last call (one host sync), then cleared."""
        s = self.state[:K["DWD_S_UPDATES"] + 1].cpu().numpy().copy()
        n = max(float(s[K["DWD_S_UPDATES"]]), 1.0)
        self.state[:K["DWD_S_UPDATES"] + 1] = 0
        return {k: float(s[i]) / n for i, k in enumerate(LOG_NAMES)}

    # ------------------------------------------------------------------------------------------------------------- buffers
    def init_demo_buffer(self, fetch_amp_obs_demo):
        """_init_amp_demo_buf (amp_continuous.py:485-493): fill the demo buffer in amp_batch_size pieces."""
        for _ in range(int(np.ceil(self.demo_buffer.get_buffer_size() / self.amp_batch_size))):
            self.demo_buffer.store(fetch_amp_obs_demo(self.amp_batch_size))

    def update_demos(self, fetch_amp_obs_demo):
        """_update_amp_demos (:495-498)."""
        self.demo_buffer.store(fetch_amp_obs_demo(self.amp_batch_size))

    def replay_batch(self, amp_obs: torch.Tensor) -> torch.Tensor:
        """train_epoch (:193-196): the current batch on the first epoch, a sample of the replay buffer after."""
        if self.replay_buffer.get_total_count() == 0:
            return amp_obs
        return self.replay_buffer.sample(amp_obs.shape[0])

    def store_replay(self, amp_obs: torch.Tensor):
        """_store_replay_amp_obs (:534-543): once more rows have been stored than the buffer holds, keep each with amp_replay_keep_prob."""
        if self.replay_buffer.get_total_count() > self.replay_buffer.get_buffer_size():
            keep = torch.bernoulli(torch.full((amp_obs.shape[0],), self.replay_keep_prob, device=amp_obs.device)) == 1.0
            amp_obs = amp_obs[keep]
        self.replay_buffer.store(amp_obs)

    # ------------------------------------------------------------------------------------------------------------- checkpoints
    def state_dict(self) -> dict:
        """The reference's names: _disc_mlp.*, _disc_logits.*, _amp_input_mean_std.{running_mean, running_var, count}."""
        sd = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        sd.update({"_amp_input_mean_std." + k: v.detach().clone() for k, v in self.rms.state_dict().items()})
        return sd

    def load_state_dict(self, sd: dict):
        with torch.no_grad():
            for k, v in self.net.state_dict().items():
                v.copy_(sd[k])
            for k, v in self.rms.state_dict().items():
                v.copy_(sd["_amp_input_mean_std." + k])

    def optimizer_state(self) -> dict:
        """The Adam state in amp_policy's backend-neutral form ({"lr", "step", "exp_avg", "exp_avg_sq"} by parameter name): hip: m, v and the
        DWD_S_LR / DWD_S_STEP words; torch: torch.optim.Adam's state."""
        from .amp_policy import _adam_state
        return _adam_state(self.backend, getattr(self, "opt", None), self._named_params(), self.m, self.v, self.state, K["DWD_S_LR"],
                           K["DWD_S_STEP"])

    def load_optimizer_state(self, st: dict):
        """optimizer_state()'s dict, written by either backend."""
        from .amp_policy import _load_adam_state
        _load_adam_state(self.backend, getattr(self, "opt", None), self._named_params(), self.m, self.v, self.state, K["DWD_S_LR"],
                         K["DWD_S_STEP"], st)

    def _named_params(self):
        names = {id(t): n for n, t in self.net.named_parameters()}
        out, o = [], 0
        for t in self._params_in_layout():
            out.append((names[id(t)], t, o))
            o += t.numel()
        return out
