"""Checkpoints of TocabiAMPLower's AMP learner in the reference learner's layout, and the play path's text export.

A checkpoint is one torch.save dict with the top-level keys rl_games 1.1.4 writes for `amp_continuous` (restated by the reference in
python/IsaacGymEnvs/isaacgymenvs/learning/: rl_games_custom/a2c_common_dyros.py:550-609 get_weights / get_stats_weights /
get_full_state_weights, amp_continuous.py:79-88 amp_input_mean_std, amp_players.py:47-51 what the player reads):
  model               ModelAMPContinuous.Network's state_dict: MODEL_KEYS, each prefixed `a2c_network.`
  running_mean_std    the observation normaliser   {running_mean, running_var, count}, float64, count 0-d
  reward_mean_std     the value normaliser         (same form)
  amp_input_mean_std  the discriminator's input normaliser (same form)
  optimizer           torch.optim.Adam(model.parameters()).state_dict(): ONE Adam over the policy and the discriminator (common_agent.py:77).
                      Adam works per parameter and both of our optimisers step once per minibatch at one learning rate, so the two states
                      merge into it exactly and split back exactly; sigma (no gradient) has an index and no state
  epoch               rl_games' epoch_num: the epochs completed
  frame, last_mean_rewards (-100500 by default, a2c_common_dyros.py:582), env_state (None)
  isaacgymdyros_amd   what the reference does not save: the demo and replay buffers with their heads and counts, the state of the generator
                      their permutations draw from, the learning-rate schedule (lr0, lr_min, max_epochs).  The reference's restore ignores it.
"""
from __future__ import annotations

import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import amp_disc as AD
from . import amp_policy as AP

PREFIX = "a2c_network."
# module registration order of AMPBuilder.Network (amp_network_builder.py:46-57, 93-115 on rl_games' A2CBuilder.Network, restated by
# network_builder_dyros.py:14-106): the direct parameter sigma first, then actor_mlp, critic_mlp, value, mu, _disc_mlp, _disc_logits
POLICY_KEYS = ["sigma", "actor_mlp.0.weight", "actor_mlp.0.bias", "actor_mlp.2.weight", "actor_mlp.2.bias", "critic_mlp.0.weight",
               "critic_mlp.0.bias", "critic_mlp.2.weight", "critic_mlp.2.bias", "value.weight", "value.bias", "mu.weight", "mu.bias"]
DISC_KEYS = ["_disc_mlp.0.weight", "_disc_mlp.0.bias", "_disc_mlp.2.weight", "_disc_mlp.2.bias", "_disc_logits.weight", "_disc_logits.bias"]
MODEL_KEYS = POLICY_KEYS + DISC_KEYS
STATS_KEYS = ["running_mean", "running_var", "count"]
TOP_KEYS = ["running_mean_std", "reward_mean_std", "amp_input_mean_std", "model", "epoch", "optimizer", "frame", "last_mean_rewards",
            "env_state"]
OUR_KEY = "isaacgymdyros_amd"
LAST_MEAN_REWARDS = -100500
# cfg/train/TocabiAMPLowerPPO.yaml: params.config.save_frequency and the name its `name` interpolation resolves to
SAVE_FREQUENCY = 100
NAME = "TocabiAMPLower"


class TorchLearner:
    """An nn.Module with the policy's state_dict names and the torch.optim.Adam over its trained parameters, seen as this module sees a
    learner (state_dict, load_state_dict, optimizer_state, load_optimizer_state): examples/amp_consumer.py's inline torch loop."""

    def __init__(self, module: nn.Module, opt: torch.optim.Adam):
        self.module, self.opt = module, opt
        self._named = [(n, t, 0) for n, t in module.named_parameters() if t.requires_grad]
        self._state = torch.zeros(2)

    def state_dict(self) -> dict:
        return {k: v.detach().clone() for k, v in self.module.state_dict().items()}

    def load_state_dict(self, sd: dict):
        with torch.no_grad():
            for k, v in self.module.state_dict().items():
                v.copy_(sd[k])

    def optimizer_state(self) -> dict:
        return AP._adam_state("torch", self.opt, self._named, None, None, self._state, 0, 1)

    def load_optimizer_state(self, st: dict):
        AP._load_adam_state("torch", self.opt, self._named, None, None, self._state, 0, 1, st)


def _stats(sd: dict, prefix: str) -> dict:
    out = OrderedDict()
    for k in STATS_KEYS:
        out[k] = sd[prefix + k].detach().to("cpu", torch.float64).clone()
    out["count"] = out["count"].reshape(())
    return out


def _buffer_state(b: AD.ReplayBuffer) -> dict:
    n = min(b._total_count, b._buffer_size)
    return {"head": int(b._head), "total_count": int(b._total_count), "buffer_size": int(b._buffer_size), "sample_idx": b._sample_idx.clone(),
            "sample_head": int(b._sample_head), "data": None if b._data is None else b._data[:n].detach().cpu().clone(),
            "row_shape": None if b._data is None else list(b._data.shape[1:]),
            "generator": None if b._gen is None else b._gen.get_state()}


def _load_buffer(b: AD.ReplayBuffer, st: dict):
    if int(st["buffer_size"]) != b._buffer_size:
        raise ValueError("checkpoint: a buffer of %d rows, this learner's holds %d" % (st["buffer_size"], b._buffer_size))
    b._head, b._total_count, b._sample_head = int(st["head"]), int(st["total_count"]), int(st["sample_head"])
    b._sample_idx = st["sample_idx"].clone()
    if st["data"] is None:
        b._data = None
    else:
        b._data = torch.zeros([b._buffer_size] + list(st["row_shape"]), device=b._device)
        b._data[:st["data"].shape[0]] = st["data"].to(b._device)
    if st["generator"] is not None and b._gen is not None:
        b._gen.set_state(st["generator"])


def _merge_optimizer(po: dict, do: dict, model: dict) -> dict:
    """The policy's and the discriminator's optimizer_state() as one torch.optim.Adam state_dict over MODEL_KEYS."""
    shell = torch.optim.Adam([nn.Parameter(torch.zeros(1)) for _ in MODEL_KEYS], lr=float(po["lr"]), eps=1e-8, weight_decay=0)
    sd = shell.state_dict()
    for i, k in enumerate(MODEL_KEYS):
        src = do if k in DISC_KEYS else po
        if k == "sigma" or int(src["step"]) == 0:
            continue
        sd["state"][i] = {"step": torch.tensor(float(src["step"])), "exp_avg": src["exp_avg"][k].detach().cpu().clone(),
                          "exp_avg_sq": src["exp_avg_sq"][k].detach().cpu().clone()}
    return sd


def _split_optimizer(osd: dict, model: dict):
    """_merge_optimizer's inverse: (policy, discriminator) optimizer_state() dicts."""
    lr = float(osd["param_groups"][0]["lr"])
    out = []
    for keys in (POLICY_KEYS, DISC_KEYS):
        st = {"lr": lr, "step": 0, "exp_avg": {}, "exp_avg_sq": {}}
        for k in keys:
            if k == "sigma":
                continue
            s = osd["state"].get(MODEL_KEYS.index(k), osd["state"].get(str(MODEL_KEYS.index(k))))
            z = torch.zeros_like(model[PREFIX + k])
            if s:
                st["step"] = int(float(s["step"]))
            st["exp_avg"][k] = s["exp_avg"] if s else z
            st["exp_avg_sq"][k] = s["exp_avg_sq"] if s else z
        out.append(st)
    return out[0], out[1]


def state(policy, disc, epoch: int, frame: int = 0, last_mean_rewards: float = LAST_MEAN_REWARDS, lr0: float = None, lr_min: float = None,
          max_epochs: int = None) -> dict:
    """The checkpoint dict of a policy (AmpActorCritic or TorchLearner) and an AmpDiscriminator."""
    psd, dsd = policy.state_dict(), disc.state_dict()
    model = OrderedDict((PREFIX + k, (dsd if k in DISC_KEYS else psd)[k].detach().cpu().clone()) for k in MODEL_KEYS)
    ck = {"running_mean_std": _stats(psd, "obs_rms."), "reward_mean_std": _stats(psd, "value_rms."),
          "amp_input_mean_std": _stats(dsd, "_amp_input_mean_std."), "model": model, "epoch": int(epoch),
          "optimizer": _merge_optimizer(policy.optimizer_state(), disc.optimizer_state(), model), "frame": int(frame),
          "last_mean_rewards": last_mean_rewards, "env_state": None}
    ck[OUR_KEY] = {"demo_buffer": _buffer_state(disc.demo_buffer), "replay_buffer": _buffer_state(disc.replay_buffer),
                   "torch_rng_state": torch.get_rng_state(), "lr0": lr0, "lr_min": lr_min, "max_epochs": max_epochs}
    return ck


def save(path: str, policy, disc, epoch: int, frame: int = 0, **kw) -> str:
    """torch.save of state(...) to path (directories made as needed); returns path."""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    torch.save(state(policy, disc, epoch, frame, **kw), path)
    return path


def load(path_or_state):
    if isinstance(path_or_state, dict):
        return path_or_state
    return torch.load(path_or_state, map_location="cpu", weights_only=True)


def _policy_sd(ck: dict) -> dict:
    sd = {k: ck["model"][PREFIX + k] for k in POLICY_KEYS}
    for name, key in (("obs_rms.", "running_mean_std"), ("value_rms.", "reward_mean_std")):
        sd.update({name + k: v for k, v in ck[key].items()})
    return sd


def _disc_sd(ck: dict) -> dict:
    sd = {k: ck["model"][PREFIX + k] for k in DISC_KEYS}
    sd.update({"_amp_input_mean_std." + k: v for k, v in ck["amp_input_mean_std"].items()})
    return sd


def restore(path_or_state, policy, disc) -> dict:
    """Load a checkpoint (ours, or the reference learner's without our key) into a policy and an AmpDiscriminator of matching shapes: weights,
    normalisers, both Adam states and, where saved, the buffers and the generator state.  Returns the counters: epoch, frame,
    last_mean_rewards, lr0, lr_min, max_epochs (None where not saved)."""
    ck = load(path_or_state)
    policy.load_state_dict(_policy_sd(ck))
    disc.load_state_dict(_disc_sd(ck))
    po, do = _split_optimizer(ck["optimizer"], ck["model"])
    policy.load_optimizer_state(po)
    disc.load_optimizer_state(do)
    ours = ck.get(OUR_KEY) or {}
    if ours:
        _load_buffer(disc.demo_buffer, ours["demo_buffer"])
        _load_buffer(disc.replay_buffer, ours["replay_buffer"])
        torch.set_rng_state(ours["torch_rng_state"])
    return {"epoch": int(ck.get("epoch", 0)), "frame": int(ck.get("frame", 0)), "last_mean_rewards": ck.get("last_mean_rewards", LAST_MEAN_REWARDS),
            "lr0": ours.get("lr0"), "lr_min": ours.get("lr_min"), "max_epochs": ours.get("max_epochs")}


def load_policy(path_or_state, device, backend: str = "hip", with_disc: bool = False, cfg: dict = None):
    """For play: an AmpActorCritic with the checkpoint's weights and normalisers (and an AmpDiscriminator when with_disc)."""
    ck = load(path_or_state)
    D, A = int(ck["running_mean_std"]["running_mean"].shape[0]), int(ck["model"][PREFIX + "sigma"].shape[0])
    pol = AP.AmpActorCritic(D, A, device, cfg, backend=backend)
    pol.load_state_dict({k: v.to(pol.device) for k, v in _policy_sd(ck).items()})
    if not with_disc:
        return pol
    disc = AD.AmpDiscriminator(int(ck["amp_input_mean_std"]["running_mean"].shape[0]), device, cfg, backend=backend)
    disc.load_state_dict({k: v.to(disc.device) for k, v in _disc_sd(ck).items()})
    return pol, disc


def export_txt(path_or_state, out_dir: str) -> list:
    """The files the reference's play path writes (torch_runner_dyros.py:143-149, amp_players.py:53-61): every model tensor as
    <name with . -> _>.txt and running_mean_std_{running_mean, running_var, count}.txt (count as one value), by np.savetxt's defaults.
    Returns the paths written."""
    ck = load(path_or_state)
    os.makedirs(out_dir, exist_ok=True)
    out = []
    for name, t in ck["model"].items():
        out.append(os.path.join(out_dir, name.replace(".", "_") + ".txt"))
        np.savetxt(out[-1], t.detach().cpu().numpy())
    for name, t in ck["running_mean_std"].items():
        t = t.detach().cpu()
        if t.ndim == 0:
            t = t.reshape(1)
        out.append(os.path.join(out_dir, "running_mean_std_" + name.replace(".", "_") + ".txt"))
        np.savetxt(out[-1], t.numpy())
    return out
