"""Checkpoints of the DyrosDynamicWalk PPO learner in the reference learner's layout, and the play path's text export.

A checkpoint is one torch.save dict with the top-level keys, in this order, that the reference's learner writes for this task (paths relative to
python/IsaacGymEnvs/isaacgymenvs/learning/rl_games_custom/: a2c_continuous_seperate.py:97-103 save -> a2c_common_dyros.py:550-602
get_full_state_weights -> get_weights -> get_stats_weights):
  scaler              GradScaler.state_dict(), written because mixed_precision is True (get_stats_weights).  normalize_input and normalize_value
                      are False, so there is no running_mean_std and no reward_mean_std.  A disabled scaler (a CPU run) writes {}
  model               ModelA2CContinuousLogStdDYROS.Network's state_dict: MODEL_KEYS, each under `a2c_network.` (models_dyros.py:17-20)
  epoch               the epochs completed
  optimizer_actor     separate_opt: Adam(actor_mlp + mu), lr the schedule's; Adam(critic_mlp + value), lr 5e-4; eps 1e-8
  optimizer_critic    (a2c_continuous_seperate.py:50-54).  torch.optim.Adam state_dicts: a plain Adam over those parameters loads them and steps
  frame, last_mean_rewards (-100500 by default; the best mean episode return so far when the learner runs its game meter,
                      isaacgymdyros_amd/game_meter.py), env_state (None: the env keeps no state the reference saves)
  isaacgymdyros_amd   what the reference does not save: the learning-rate schedule (lr0, lr_min, max_epochs), sigma_init / sigma_last and the
                      backend that wrote the file.  The reference's restore (set_full_state_weights) reads keys by name and ignores it.
MODEL_KEYS' order is the module registration order of network_builder_dyros.py:14-127: state_dict lists a module's direct parameters before its
submodules, so `sigma` (a direct nn.Parameter, :104) comes first although it is assigned last; then the submodules in the order their attributes
are first assigned: actor_cnn and critic_cnn (:21-22, empty Sequentials: no keys), actor_mlp and critic_mlp (:23-24, filled at :76-78 as
Linear, activation, Linear, activation: indices 0 and 2), value (:80), mu (:92).  The activation modules hold no parameters.

Two forms of the learner are served: the eager one (the network, the two torch.optim.Adam and the GradScaler of examples/ppo_consumer.py) and
FusedPpoUpdate, whose moments are cut out of its padded layout per parameter (the pads stay zero on load), whose DWP_S_STEP / DWP_S_LR words give
each optimiser's step and lr and whose DWP_S_SCALE / DWP_S_GROWTH words fill the scaler dict.  A file of either form loads into the other.
"""
from __future__ import annotations

import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

PREFIX = "a2c_network."
MODEL_KEYS = ["sigma", "actor_mlp.0.weight", "actor_mlp.0.bias", "actor_mlp.2.weight", "actor_mlp.2.bias", "critic_mlp.0.weight", "critic_mlp.0.bias",
              "critic_mlp.2.weight", "critic_mlp.2.bias", "value.weight", "value.bias", "mu.weight", "mu.bias"]
ACTOR_OPT_KEYS = ["actor_mlp.0.weight", "actor_mlp.0.bias", "actor_mlp.2.weight", "actor_mlp.2.bias", "mu.weight", "mu.bias"]
CRITIC_OPT_KEYS = ["critic_mlp.0.weight", "critic_mlp.0.bias", "critic_mlp.2.weight", "critic_mlp.2.bias", "value.weight", "value.bias"]
TOP_KEYS = ["scaler", "model", "epoch", "optimizer_actor", "optimizer_critic", "frame", "last_mean_rewards", "env_state"]
OUR_KEY = "isaacgymdyros_amd"
LAST_MEAN_REWARDS = -100500
# torch.amp.GradScaler's defaults, which the fused update's scaler follows (include/dyros_ppo.h dwp_finish), and its growth interval
GROWTH_FACTOR, BACKOFF_FACTOR, GROWTH_INTERVAL = 2.0, 0.5, 2000
CRITIC_LR = 5e-4
# cfg/train/DyrosDynamicWalkPPO.yaml: params.config.save_frequency, and the experiment name its `name` resolves to
SAVE_FREQUENCY = 100
SAVE_BEST_AFTER = 200          # params.config.save_best_after
SCORE_TO_WIN = 20000           # params.config.score_to_win
NAME = "DyrosDynamicWalk"


def _cpu(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu").clone(memory_format=torch.contiguous_format)


def _adam_shell(lr: float, n: int = 6) -> dict:
    """The state_dict of a fresh torch.optim.Adam over n parameters (lr, eps 1e-8): the param_group fields this torch writes."""
    return torch.optim.Adam([nn.Parameter(torch.zeros(1)) for _ in range(n)], lr=float(lr), eps=1e-8).state_dict()


HYPER = ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize")          # what a file carries over; the execution flags stay the optimiser's own


def _plain_optimizer(opt: torch.optim.Optimizer) -> dict:
    """opt.state_dict() as a plain Adam's (the reference's): host tensors, a float lr, the execution flags (capturable, fused, foreach) of a fresh
    Adam -- a capturable, fused Adam keeps lr and step on the device."""
    sd = opt.state_dict()
    out = {"state": {i: {k: (_cpu(v) if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in sd["state"].items()}, "param_groups": []}
    for g in sd["param_groups"]:
        ng = _adam_shell(1.0, len(g["params"]))["param_groups"][0]
        ng.update({k: g[k] for k in HYPER if k in g})
        ng["lr"], ng["params"] = float(g["lr"]), list(g["params"])
        out["param_groups"].append(ng)
    return out


def _load_optimizer(opt: torch.optim.Optimizer, sd: dict):
    """opt.load_state_dict(sd) with the optimiser's own execution flags kept (torch would take the file's), and a device lr tensor kept where the
    optimiser has one (what a captured step reads): the file's lr is written into it in place."""
    keep = [dict(g) for g in opt.param_groups]
    groups = []
    for g, own in zip(sd["param_groups"], keep):
        ng = {k: v for k, v in own.items() if k != "params"}
        ng.update({k: g[k] for k in HYPER if k in g})
        ng["lr"], ng["params"] = float(g["lr"]), g["params"]
        groups.append(ng)
    opt.load_state_dict({"state": sd["state"], "param_groups": groups})
    for g, own in zip(opt.param_groups, keep):
        if torch.is_tensor(own["lr"]):
            own["lr"].fill_(float(g["lr"]))
            g["lr"] = own["lr"]


def _fused_optimizers(fused) -> tuple:
    """(optimizer_actor, optimizer_critic, scaler) from a FusedPpoUpdate's device state."""
    from . import ppo_update as U
    from .walk_policy import tensor_views
    st = fused.state.detach().to("cpu")
    m, v = tensor_views(fused.m.detach()), tensor_views(fused.v.detach())
    opts = []
    for net, keys in ((0, ACTOR_OPT_KEYS), (1, CRITIC_OPT_KEYS)):
        sd = _adam_shell(float(st[U.K["DWP_S_LR"] + net]))
        step = float(st[U.K["DWP_S_STEP"] + net])
        if step > 0:
            sd["state"] = {i: {"step": torch.tensor(step), "exp_avg": _cpu(m[k]), "exp_avg_sq": _cpu(v[k])} for i, k in enumerate(keys)}
        opts.append(sd)
    scaler = {"scale": float(st[U.K["DWP_S_SCALE"]]), "growth_factor": GROWTH_FACTOR, "backoff_factor": BACKOFF_FACTOR,
              "growth_interval": GROWTH_INTERVAL, "_growth_tracker": int(st[U.K["DWP_S_GROWTH"]])}
    return opts[0], opts[1], scaler


def _load_fused(fused, opt_actor: dict, opt_critic: dict, scaler: dict):
    """The two Adam state_dicts and the scaler dict into a FusedPpoUpdate (moments in its padded layout with zero pads, steps, lrs, scale, tracker)."""
    from .walk_policy import tensor_views
    from . import ppo_update as U
    m, v = torch.zeros(U.NP), torch.zeros(U.NP)
    mv, vv = tensor_views(m), tensor_views(v)
    steps, lrs = [], []
    for osd, keys in ((opt_actor, ACTOR_OPT_KEYS), (opt_critic, CRITIC_OPT_KEYS)):
        step = 0.0
        for i, k in enumerate(keys):
            s = osd["state"].get(i, osd["state"].get(str(i)))
            if not s:
                continue
            step = float(s["step"])
            mv[k].copy_(s["exp_avg"].reshape(mv[k].shape)); vv[k].copy_(s["exp_avg_sq"].reshape(vv[k].shape))
        steps.append(step)
        lrs.append(float(osd["param_groups"][0]["lr"]))
    st = fused.state.detach().to("cpu")
    scale = float(scaler["scale"]) if scaler else float(st[U.K["DWP_S_SCALE"]])
    growth = float(scaler["_growth_tracker"]) if scaler else float(st[U.K["DWP_S_GROWTH"]])
    fused.load_state_dict({"m": m.to(fused.dev), "v": v.to(fused.dev), "scale": scale, "growth": growth, "steps": steps})
    fused.set_learning_rates(lrs[0], lrs[1])
    fused.sync_policy_copy()


def state(net, epoch: int, frame: int = 0, fused=None, opt_actor=None, opt_critic=None, scaler=None, last_mean_rewards: float = LAST_MEAN_REWARDS,
          lr0: float = None, lr_min: float = None, max_epochs: int = None) -> OrderedDict:
    """The checkpoint dict of a network (DyrosActorCritic, or any module with these state_dict names) and its optimiser side: `fused` (a
    FusedPpoUpdate) or opt_actor / opt_critic (torch.optim.Adam) with scaler (torch.amp.GradScaler, or None: {})."""
    sd = net.state_dict()
    model = OrderedDict((PREFIX + k, _cpu(sd[k])) for k in MODEL_KEYS)
    if fused is not None:
        oa, oc, sc = _fused_optimizers(fused)
        backend = "fused"
    else:
        if opt_actor is None or opt_critic is None:
            raise ValueError("ppo_checkpoint.state: pass fused= or both opt_actor= and opt_critic=")
        oa, oc = _plain_optimizer(opt_actor), _plain_optimizer(opt_critic)
        sc = scaler.state_dict() if scaler is not None else {}
        backend = "torch"
    ck = OrderedDict()
    ck["scaler"] = sc
    ck["model"] = model
    ck["epoch"] = int(epoch)
    ck["optimizer_actor"], ck["optimizer_critic"] = oa, oc
    ck["frame"] = int(frame)
    ck["last_mean_rewards"] = last_mean_rewards
    ck["env_state"] = None
    ck[OUR_KEY] = {"lr0": lr0, "lr_min": lr_min, "max_epochs": max_epochs, "sigma_init": getattr(net, "sigma_init", None),
                   "sigma_last": getattr(net, "sigma_last", None), "backend": backend}
    return ck


def save(path: str, net, epoch: int, frame: int = 0, **kw) -> str:
    """torch.save of state(net, epoch, frame, **kw) to path (directories made as needed); returns path."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(state(net, epoch, frame, **kw), path)
    return path


def load(path_or_state):
    if isinstance(path_or_state, dict):
        return path_or_state
    return torch.load(path_or_state, map_location="cpu", weights_only=True)


def restore(path_or_state, net, fused=None, opt_actor=None, opt_critic=None, scaler=None) -> dict:
    """Load a checkpoint (ours, or the reference learner's without our key) into a network and its optimiser side: the weights, then either a
    FusedPpoUpdate (`fused`: moments, steps, lrs, scale and tracker; its fp16 and operand-order copies are refreshed) or the torch optimisers and
    GradScaler (a scaler dict of {} -- a disabled scaler's -- leaves the scaler as it is).  Returns the counters: epoch, frame, last_mean_rewards,
    lr0, lr_min, max_epochs (None where not saved)."""
    ck = load(path_or_state)
    sd = net.state_dict()
    for k in MODEL_KEYS:
        t = ck["model"][PREFIX + k]
        if tuple(t.shape) != tuple(sd[k].shape):
            raise ValueError("checkpoint: %s is %r, this network's is %r" % (k, tuple(t.shape), tuple(sd[k].shape)))
    with torch.no_grad():
        for k in MODEL_KEYS:
            sd[k].copy_(ck["model"][PREFIX + k].to(sd[k].device))
    sc = ck.get("scaler") or {}
    if fused is not None:
        _load_fused(fused, ck["optimizer_actor"], ck["optimizer_critic"], sc)
    else:
        if opt_actor is not None:
            _load_optimizer(opt_actor, ck["optimizer_actor"])
        if opt_critic is not None:
            _load_optimizer(opt_critic, ck["optimizer_critic"])
        if scaler is not None and sc and scaler.is_enabled():
            scaler.load_state_dict(sc)
    ours = ck.get(OUR_KEY) or {}
    return {"epoch": int(ck.get("epoch", 0)), "frame": int(ck.get("frame", 0)), "last_mean_rewards": ck.get("last_mean_rewards", LAST_MEAN_REWARDS),
            "lr0": ours.get("lr0"), "lr_min": ours.get("lr_min"), "max_epochs": ours.get("max_epochs")}


def load_policy(path_or_state, device, backend: str = "hip"):
    """For play: a WalkPolicy (isaacgymdyros_amd/walk_policy.py) with the checkpoint's actor."""
    from .walk_policy import WalkPolicy
    ck = load(path_or_state)
    pol = WalkPolicy(device, backend=backend)
    pol.load_state_dict(ck["model"])
    return pol


def export_txt(path_or_state, out_dir: str) -> list:
    """The files the reference's play path writes (torch_runner_dyros.py:143-149): every model tensor as <name with . -> _>.txt by np.savetxt's
    defaults -- 13 files.  Returns the paths written."""
    ck = load(path_or_state)
    os.makedirs(out_dir, exist_ok=True)
    out = []
    for name, t in ck["model"].items():
        out.append(os.path.join(out_dir, name.replace(".", "_") + ".txt"))
        np.savetxt(out[-1], t.detach().cpu().numpy())
    return out
