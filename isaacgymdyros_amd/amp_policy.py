"""The actor-critic of TocabiAMPLower's AMP learner (include/dyros_amp_policy.h, csrc/dw_amp_policy.hip).

Reference (python/IsaacGymEnvs/isaacgymenvs/): learning/amp_continuous.py and learning/common_agent.py with cfg/train/TocabiAMPLowerPPO.yaml.
  * network: separate actor and critic MLPs (`separate: True`), units [512, 512], relu, a linear mu head and a linear value head, a fixed
    log-sigma (sigma_init -1.6, `learn_sigma: False`); fp32 (`mixed_precision: False`); nn.Linear's own initialisation.
  * normalisation: rl_games' RunningMeanStd (amp_disc.RunningMeanStd) of the observations (train mode during the minibatch updates: each
    minibatch updates the statistics first, then normalises) and of the values (two train-mode updates in prepare_dataset, values then
    returns; eval mode elsewhere).
  * play_steps (:91-167): get_action_values in eval mode; the bootstrap values through _eval_critic, zeroed on `terminate`; GAE as
    common_agent.discount_values (:413-425).
  * calc_gradients (:260-329): the clipped surrogate (e_clip 0.2), the critic loss (critic_coef 5, clip_value False), the soft bound loss
    (bounds_loss_coef 10), no entropy term (entropy_coef 0), Adam (eps 1e-8) without clipping (truncate_grads False).

Two backends of one class: `backend="hip"` (the product: dwa_stats, dwa_act, dwa_critic, dwa_grad, dwa_opt, dwa_gae, dwa_play) and `backend="torch"`
(the arithmetic of examples/amp_consumer.py's inline loop: the yardstick of the tests and the CPU form).  Parameter names are those of the
consumer's ActorCritic, so a state_dict of either backend loads into the other.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn as nn

from . import amp_disc as AD
from . import cbind
from .amp_disc import _req

K = cbind.constants("dyros_amp_policy.h", "dwa_")
HID, D_MAX, A_MAX = K["DWA_HID"], K["DWA_D_MAX"], K["DWA_A_MAX"]
LOG_NAMES = ["a_loss", "c_loss", "b_loss", "clip_frac"]


def num_params(D: int, A: int) -> int:
    net = D * HID + HID + HID * HID + HID
    return net + A * HID + A + net + HID + 1


def _mlp(n_in, units):
    layers = []
    for u in units:
        layers += [nn.Linear(n_in, u), nn.ReLU()]
        n_in = u
    return nn.Sequential(*layers), n_in


class ActorCritic(nn.Module):
    """examples/amp_consumer.py's ActorCritic: the same modules in the same order (so the same initial values from the same seed) and names."""

    def __init__(self, num_obs, num_act, units, sigma_init):
        super().__init__()
        self.actor_mlp, n = _mlp(num_obs, units)
        self.critic_mlp, _ = _mlp(num_obs, units)
        self.mu, self.value = nn.Linear(n, num_act), nn.Linear(n, 1)
        self.sigma = nn.Parameter(torch.full((num_act,), float(sigma_init)), requires_grad=False)
        self.obs_rms, self.value_rms = AD.RunningMeanStd(num_obs), AD.RunningMeanStd(1)

    def forward(self, obs):
        x = self.obs_rms(obs)
        return self.mu(self.actor_mlp(x)), self.value(self.critic_mlp(x))

    def neglogp(self, a, mu):
        s = self.sigma
        return 0.5 * (((a - mu) / torch.exp(s)) ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * a.shape[-1] + s.sum()

    def unnorm_value(self, v):
        r = self.value_rms
        return v * torch.sqrt(r.running_var.float() + r.epsilon) + r.running_mean.float()

    def params_in_layout(self):
        a, c = self.actor_mlp, self.critic_mlp
        return [a[0].weight, a[0].bias, a[2].weight, a[2].bias, self.mu.weight, self.mu.bias,
                c[0].weight, c[0].bias, c[2].weight, c[2].bias, self.value.weight, self.value.bias]


def torch_losses(net: ActorCritic, obs, act, old_nlp, adv, ret_n, e_clip):
    """calc_gradients' policy share as the consumer writes it: (a_loss, c_loss, b_loss, clip_frac); obs_rms moves if net is in train mode."""
    mu, v = net(obs)
    return loss_terms(old_nlp, net.neglogp(act, mu), adv, mu, v, ret_n, e_clip)


def loss_terms(old_nlp, nlp, adv, mu, v, ret_n, e_clip):
    """The three losses and the clip fraction from the rows' neglogp, mu and value (the expressions of the consumer's loop)."""
    ratio = torch.exp(old_nlp - nlp)
    a = adv.view(-1)
    a_loss = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - e_clip, 1 + e_clip)).mean()
    c_loss = ((ret_n.view(-1, 1) - v) ** 2).mean()
    b_loss = ((torch.clamp(mu - 1.0, min=0) ** 2 + torch.clamp(mu + 1.0, max=0) ** 2).sum(-1)).mean()
    clip_frac = (torch.abs(ratio - 1.0) > e_clip).float().mean()          # (fp32 whatever the dtype, as _actor_loss)
    return a_loss, c_loss, b_loss, clip_frac


DwaLoss = cbind.structs("dyros_amp_policy.h", "dwa_")["DwaLoss"]
EXPORTS = list(cbind.signatures("dyros_amp_policy.h", "dwa_"))


def declare(lib: C.CDLL) -> dict:
    return cbind.declare(lib, "dyros_amp_policy.h", "dwa_")


def _api():
    from . import _lib
    return declare(_lib.load()[0])


def _check(rc):
    cbind.check(_api(), rc)


def torch_gae(done, values, rewards, next_values, gamma: float, tau: float):
    """The consumer's GAE loop (discount_values' operations in its order), in the tensors' dtype: the advantages [H, N, 1]."""
    H, N = int(values.shape[0]), int(values.shape[1])
    adv = torch.zeros_like(rewards)
    last = torch.zeros(N, 1, dtype=rewards.dtype, device=rewards.device)
    for t in reversed(range(H)):
        delta = rewards[t] + gamma * next_values[t] - values[t]
        last = delta + gamma * tau * (1.0 - done[t]).view(N, 1) * last
        adv[t] = last
    return adv


def gae(done, values, rewards, next_values, gamma: float, tau: float, backend: str = "hip"):
    """common_agent.discount_values with mb_next_values: done [H, N], values / rewards / next_values [H, N, 1] -> (adv, ret = adv + values)."""
    if backend not in ("hip", "torch"):
        raise ValueError("backend must be 'hip' or 'torch'")
    if not torch.is_tensor(values) or values.dim() != 3 or values.shape[2] != 1:
        raise ValueError("values: a [H, N, 1] tensor is required")
    H, N = int(values.shape[0]), int(values.shape[1])
    dev = values.device
    _req("done", done, torch.float32, dev, (H, N))
    for name, t in (("values", values), ("rewards", rewards), ("next_values", next_values)):
        _req(name, t, torch.float32, dev, (H, N, 1))
    if H < 1 or N < 1:
        raise ValueError("gae: no rows")
    if backend == "torch":
        adv = torch_gae(done, values, rewards, next_values, gamma, tau)
        return adv, adv + values
    if dev.type != "cuda":
        raise ValueError("backend 'hip' needs a GPU device")
    adv, ret = torch.empty_like(values), torch.empty_like(values)
    _check(_api()["gae"](done.data_ptr(), values.data_ptr(), rewards.data_ptr(), next_values.data_ptr(), H, N, float(gamma), float(gamma * tau),
                         adv.data_ptr(), ret.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return adv, ret


class AmpActorCritic:
    """The actor-critic, its two normalisers and its optimiser state.

    cfg: amp_disc.TRAIN_CFG (or amp_disc.load_train_yaml's dict); backend "hip" (the kernels; a CUDA device) or "torch" (the consumer's
    arithmetic)."""

    def __init__(self, num_obs: int, num_actions: int, device, cfg: dict = None, backend: str = "hip", seed: int = None):
        cfg = cfg or AD.TRAIN_CFG
        c, netc = cfg["config"], cfg["network"]
        D, A = int(num_obs), int(num_actions)
        if not 1 <= D <= D_MAX:
            raise ValueError("num_obs %d: must be in [1, %d]" % (D, D_MAX))
        if not 1 <= A <= A_MAX:
            raise ValueError("num_actions %d: must be in [1, %d]" % (A, A_MAX))
        if list(netc.get("mlp_units", [HID, HID])) != [HID, HID] or netc.get("activation", "relu") != "relu":
            raise ValueError("the actor-critic is fixed at units [512, 512] with relu (cfg/train/TocabiAMPLowerPPO.yaml)")
        if c.get("mixed_precision", False):
            raise ValueError("the actor-critic runs in fp32 only (mixed_precision: False)")
        if c.get("clip_value", False) or float(c.get("entropy_coef", 0.0)) != 0.0 or c.get("truncate_grads", False):
            raise ValueError("clip_value, entropy_coef and truncate_grads are not supported (the yaml has False, 0, False)")
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        self.device, self.D, self.A, self.backend = torch.device(device), D, A, backend
        if backend == "hip" and self.device.type != "cuda":
            raise ValueError("backend 'hip' needs a GPU device (use backend='torch' on the CPU)")
        self.e_clip, self.critic_coef, self.bounds_coef = float(c["e_clip"]), float(c["critic_coef"]), float(c["bounds_loss_coef"])
        if seed is not None:
            torch.manual_seed(seed)
        self.net = ActorCritic(D, A, [HID, HID], netc["sigma_init"])
        assert num_params(D, A) == sum(t.numel() for t in self.net.params_in_layout())
        # one flat fp32 buffer in the layout of include/dyros_amp_policy.h; the module's parameters are views of it
        self.p = torch.cat([t.detach().reshape(-1) for t in self.net.params_in_layout()]).to(self.device)
        self.net.to(self.device)
        o = 0
        for t in self.net.params_in_layout():
            t.data = self.p[o:o + t.numel()].view_as(t)
            o += t.numel()
        self.g, self.m, self.v = (torch.zeros_like(self.p) for _ in range(3))
        self.obs_stats, self.val_stats = (torch.cat([r.running_mean, r.running_var, r.count.reshape(1)]).clone()
                                          for r in (self.net.obs_rms, self.net.value_rms))
        for r, st, n in ((self.net.obs_rms, self.obs_stats, D), (self.net.value_rms, self.val_stats, 1)):
            r.running_mean, r.running_var, r.count = st[:n], st[n:2 * n], st[2 * n]
        self.state = torch.zeros(K["DWA_S_WORDS"], dtype=torch.float32, device=self.device)
        self.state[K["DWA_S_LR"]] = float(c["learning_rate"])
        self._work = {}
        if backend == "hip":
            self.api = _api()
            self._swork = torch.empty(self.api["stats_workspace_bytes"](D) // 8, dtype=torch.float64, device=self.device)
        else:
            self.opt = torch.optim.Adam([t for t in self.net.parameters() if t.requires_grad], lr=float(c["learning_rate"]), eps=1e-8)

    # ------------------------------------------------------------------------------------------------------------- helpers
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _ws(self, rows: int, grad: int):
        key = (rows, grad)
        if key not in self._work:
            nb = self.api["workspace_bytes"](rows, self.D, self.A, grad)
            if nb < 0:
                raise ValueError("dwa: %d rows" % rows)
            self._work[key] = torch.empty((nb + 3) // 4, dtype=torch.float32, device=self.device)
        w = self._work[key]
        return w.data_ptr(), w.numel() * 4

    def _rows(self, name, x, width):
        if not torch.is_tensor(x) or x.dim() != 2:
            raise ValueError("%s: a [N, %d] tensor is required" % (name, width))
        _req(name, x, torch.float32, self.device, (x.shape[0], width))
        if x.shape[0] < 1:
            raise ValueError("%s: no rows" % name)
        return int(x.shape[0])

    # ------------------------------------------------------------------------------------------------------------- rollout
    def act(self, obs, noise):
        """get_action_values in eval mode with the caller's standard-normal draws: (action, clamped action, mu, neglogp, value [N, 1])."""
        N = self._rows("obs", obs, self.D)
        _req("noise", noise, torch.float32, self.device, (N, self.A))
        if self.backend == "torch":
            with torch.no_grad():
                self.net.eval()
                mu, v = self.net(obs)
                a = mu + torch.exp(self.net.sigma) * noise
                return a, torch.clamp(a, -1.0, 1.0), mu, self.net.neglogp(a, mu), self.net.unnorm_value(v)
        a, ac, mu = (torch.empty(N, self.A, device=self.device) for _ in range(3))
        nlp, val = torch.empty(N, device=self.device), torch.empty(N, 1, device=self.device)
        w, nb = self._ws(N, 0)
        _check(self.api["act"](self.p.data_ptr(), self.obs_stats.data_ptr(), self.val_stats.data_ptr(), self.net.sigma.data_ptr(), obs.data_ptr(),
                               noise.data_ptr(), N, self.D, self.A, a.data_ptr(), ac.data_ptr(), mu.data_ptr(), nlp.data_ptr(), val.data_ptr(),
                               w, nb, self._stream()))
        return a, ac, mu, nlp, val

    def play(self, obs, noise=None):
        """The player's get_action (eval mode, the actor only): (clamped [N, A], mu [N, A]).  noise None: clamped = clamp(mu, -1, 1), the
        deterministic player; else [N, A] standard-normal draws: clamped = clamp(mu + exp(sigma) noise, -1, 1).  No statistic moves."""
        N = self._rows("obs", obs, self.D)
        if noise is not None:
            _req("noise", noise, torch.float32, self.device, (N, self.A))
        if self.backend == "torch":
            with torch.no_grad():
                self.net.eval()
                mu = self.net.mu(self.net.actor_mlp(self.net.obs_rms(obs)))
                a = mu if noise is None else mu + torch.exp(self.net.sigma) * noise
                return torch.clamp(a, -1.0, 1.0), mu
        clamped, mu = torch.empty(N, self.A, device=self.device), torch.empty(N, self.A, device=self.device)
        key = ("play", N)
        if key not in self._work:
            nb = self.api["play_workspace_bytes"](N, self.D, self.A)
            if nb < 0:
                raise ValueError("dwa_play: %d rows" % N)
            self._work[key] = torch.empty(max(nb, 4) // 4, dtype=torch.float32, device=self.device)
        w = self._work[key]
        _check(self.api["play"](self.p.data_ptr(), self.obs_stats.data_ptr(), self.net.sigma.data_ptr(), obs.data_ptr(),
                                None if noise is None else noise.data_ptr(), N, self.D, self.A, clamped.data_ptr(), mu.data_ptr(), w.data_ptr(),
                                w.numel() * 4, self._stream()))
        return clamped, mu

    def eval_critic(self, obs, terminate):
        """_eval_critic for the bootstrap: the unnormalised value [N, 1] times (1 - terminate [N])."""
        N = self._rows("obs", obs, self.D)
        _req("terminate", terminate, torch.float32, self.device, (N,))
        if self.backend == "torch":
            with torch.no_grad():
                self.net.eval()
                return self.net.unnorm_value(self.net(obs)[1]) * (1.0 - terminate.view(N, 1))
        val = torch.empty(N, 1, device=self.device)
        w, nb = self._ws(N, 0)
        _check(self.api["critic"](self.p.data_ptr(), self.obs_stats.data_ptr(), self.val_stats.data_ptr(), obs.data_ptr(), terminate.data_ptr(), N,
                                  self.D, self.A, val.data_ptr(), w, nb, self._stream()))
        return val

    def update_value_stats(self, values, returns):
        """prepare_dataset's two train-mode updates of the value normaliser (values, then returns): the normalised returns [B, 1]."""
        for name, t in (("values", values), ("returns", returns)):
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 1:
                raise ValueError("%s: a [B, 1] tensor is required" % name)
            _req(name, t, torch.float32, self.device, (values.shape[0], 1))
        if values.shape[0] < 2:
            raise ValueError("values: at least 2 rows are required (the running statistics take an unbiased variance)")
        r = self.net.value_rms
        if self.backend == "torch":
            with torch.no_grad():
                r.train()
                r(values)
                ret_n = r(returns)
                r.eval()
            return ret_n
        vs, w, s = self.val_stats.data_ptr(), self._swork.data_ptr(), self._stream()
        _check(self.api["stats"](values.data_ptr(), values.shape[0], 1, vs, vs, w, s))
        _check(self.api["stats"](returns.data_ptr(), returns.shape[0], 1, vs, vs, w, s))
        r.eval()
        with torch.no_grad():
            return r(returns)          # (the normalisation itself: RunningMeanStd.forward's arithmetic on B words)

    # ------------------------------------------------------------------------------------------------------------- one minibatch
    def accumulate_grad(self, obs, act, old_nlp, adv, ret_n):
        """g += d(a_loss + critic_coef c_loss + bounds_coef b_loss) / dp for one minibatch (the observation statistics move first, as in
        train mode); the logged values are added to `state`.  No optimiser step."""
        B = self._rows("obs", obs, self.D)
        _req("act", act, torch.float32, self.device, (B, self.A))
        for name, t in (("old_nlp", old_nlp), ("adv", adv), ("ret_n", ret_n)):
            _req(name, t, torch.float32, self.device, (B,))
        if B < 2:
            raise ValueError("obs: at least 2 rows are required (the running statistics take an unbiased variance)")
        if self.backend == "torch":
            self.net.train()
            self.net.value_rms.eval()
            a_loss, c_loss, b_loss, clip = torch_losses(self.net, obs, act, old_nlp, adv, ret_n, self.e_clip)
            loss = a_loss + self.critic_coef * c_loss + self.bounds_coef * b_loss
            grads = torch.autograd.grad(loss, self.net.params_in_layout())
            with torch.no_grad():
                self.g += torch.cat([x.reshape(-1) for x in grads])
                self.state[:4] += torch.stack([a_loss.detach(), c_loss.detach(), b_loss.detach(), clip])
                self.state[K["DWA_S_UPDATES"]] += 1
            return
        api, s, st = self.api, self._stream(), self.obs_stats.data_ptr()
        _check(api["stats"](obs.data_ptr(), B, self.D, st, st, self._swork.data_ptr(), s))
        w, nb = self._ws(B, 1)
        _check(api["grad"](self.p.data_ptr(), st, self.net.sigma.data_ptr(), obs.data_ptr(), act.data_ptr(), old_nlp.data_ptr(), adv.data_ptr(),
                           ret_n.data_ptr(), B, self.D, self.A, DwaLoss(self.e_clip, self.critic_coef, self.bounds_coef), self.g.data_ptr(),
                           self.state.data_ptr(), w, nb, s))

    def step(self, lr: float = None):
        """One Adam step with g (lr: written to the device word first; None: the word as it is, e.g. inside a replayed graph), then g = 0."""
        if lr is not None:
            self.set_lr(lr)
        if self.backend == "torch":
            for pg in self.opt.param_groups:
                pg["lr"] = float(self.state[K["DWA_S_LR"]])
            o = 0
            for t in self.net.params_in_layout():
                t.grad = self.g[o:o + t.numel()].view_as(t).clone()
                o += t.numel()
            self.opt.step()
            self.g.zero_()
            self.state[K["DWA_S_STEP"]] += 1
            return
        _check(self.api["opt"](self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.state.data_ptr(), self.D, self.A,
                               self._stream()))

    def set_lr(self, lr: float):
        self.state[K["DWA_S_LR"]] = float(lr)

    def update(self, obs, act, old_nlp, adv, ret_n, lr: float = None) -> dict:
        """One minibatch: observation statistics, loss gradient, Adam step.  Returns the logged sums so far (device tensors)."""
        if self.backend == "torch":
            return self._torch_update(obs, act, old_nlp, adv, ret_n, lr)
        self.accumulate_grad(obs, act, old_nlp, adv, ret_n)
        self.step(lr)
        return {k: self.state[i] for i, k in enumerate(LOG_NAMES)}

    def _torch_update(self, obs, act, old_nlp, adv, ret_n, lr):
        """The consumer's inline minibatch step, operation for operation (zero_grad, backward, Adam.step)."""
        B = self._rows("obs", obs, self.D)
        _req("act", act, torch.float32, self.device, (B, self.A))
        for name, t in (("old_nlp", old_nlp), ("adv", adv), ("ret_n", ret_n)):
            _req(name, t, torch.float32, self.device, (B,))
        if B < 2:
            raise ValueError("obs: at least 2 rows are required (the running statistics take an unbiased variance)")
        if lr is not None:
            self.set_lr(lr)
        for pg in self.opt.param_groups:
            pg["lr"] = float(self.state[K["DWA_S_LR"]]) if lr is None else lr
        self.net.train()
        self.net.value_rms.eval()
        a_loss, c_loss, b_loss, clip = torch_losses(self.net, obs, act, old_nlp, adv, ret_n, self.e_clip)
        loss = a_loss + self.critic_coef * c_loss + self.bounds_coef * b_loss
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        with torch.no_grad():
            self.state[:4] += torch.stack([a_loss.detach(), c_loss.detach(), b_loss.detach(), clip])
            self.state[K["DWA_S_UPDATES"]] += 1
            self.state[K["DWA_S_STEP"]] += 1
        return {k: self.state[i] for i, k in enumerate(LOG_NAMES)}

    def pop_info(self) -> dict:
        """The logged values averaged over the minibatches since the last call (one host sync), then cleared."""
        s = self.state[:K["DWA_S_UPDATES"] + 1].cpu().numpy().copy()
        n = max(float(s[K["DWA_S_UPDATES"]]), 1.0)
        self.state[:K["DWA_S_UPDATES"] + 1] = 0
        return {k: float(s[i]) / n for i, k in enumerate(LOG_NAMES)}

    # ------------------------------------------------------------------------------------------------------------- checkpoints
    def state_dict(self) -> dict:
        """examples/amp_consumer.py's ActorCritic names: actor_mlp.*, critic_mlp.*, mu.*, value.*, sigma, obs_rms.*, value_rms.*."""
        return {k: v.detach().clone() for k, v in self.net.state_dict().items()}

    def load_state_dict(self, sd: dict):
        with torch.no_grad():
            for k, v in self.net.state_dict().items():
                v.copy_(sd[k])

    def optimizer_state(self) -> dict:
        """The Adam state in a backend-neutral form: {"lr", "step", "exp_avg": {name: tensor}, "exp_avg_sq": {name: tensor}} over the trained
        parameters (state_dict names, sigma excluded).  hip: m, v and the DWA_S_LR / DWA_S_STEP words; torch: torch.optim.Adam's state."""
        return _adam_state(self.backend, getattr(self, "opt", None), self._named_params(), self.m, self.v, self.state, K["DWA_S_LR"], K["DWA_S_STEP"])

    def load_optimizer_state(self, st: dict):
        """optimizer_state()'s dict, written by either backend."""
        _load_adam_state(self.backend, getattr(self, "opt", None), self._named_params(), self.m, self.v, self.state, K["DWA_S_LR"], K["DWA_S_STEP"], st)

    def _named_params(self):
        """(name, parameter, offset into p) of the trained parameters in the layout order."""
        names = {id(t): n for n, t in self.net.named_parameters()}
        out, o = [], 0
        for t in self.net.params_in_layout():
            out.append((names[id(t)], t, o))
            o += t.numel()
        return out


def _adam_state(backend, opt, named, m, v, state, i_lr, i_step) -> dict:
    """optimizer_state() of a learner: named = [(name, parameter, offset into the flat m / v)]."""
    if backend == "torch":
        lr = float(opt.param_groups[0]["lr"])
        step = 0
        ea, es = {}, {}
        for n, t, _o in named:
            s = opt.state.get(t, {})
            step = max(step, int(float(s["step"]))) if "step" in s else step
            ea[n] = s["exp_avg"].detach().clone() if "exp_avg" in s else torch.zeros_like(t.detach())
            es[n] = s["exp_avg_sq"].detach().clone() if "exp_avg_sq" in s else torch.zeros_like(t.detach())
        return {"lr": lr, "step": step, "exp_avg": ea, "exp_avg_sq": es}
    sv = state.cpu()
    return {"lr": float(sv[i_lr]), "step": int(sv[i_step]),
            "exp_avg": {n: m[o:o + t.numel()].view_as(t).clone() for n, t, o in named},
            "exp_avg_sq": {n: v[o:o + t.numel()].view_as(t).clone() for n, t, o in named}}


def _load_adam_state(backend, opt, named, m, v, state, i_lr, i_step, st: dict):
    step, lr = int(st["step"]), float(st["lr"])
    with torch.no_grad():
        state[i_lr], state[i_step] = lr, float(step)
        if backend == "torch":
            for pg in opt.param_groups:
                pg["lr"] = lr
            opt.state.clear()
            if step > 0:
                for n, t, _o in named:
                    opt.state[t] = {"step": torch.tensor(float(step)), "exp_avg": st["exp_avg"][n].to(t.device, torch.float32).clone(),
                                    "exp_avg_sq": st["exp_avg_sq"][n].to(t.device, torch.float32).clone()}
            return
        for n, t, o in named:
            m[o:o + t.numel()].copy_(st["exp_avg"][n].reshape(-1))
            v[o:o + t.numel()].copy_(st["exp_avg_sq"][n].reshape(-1))
