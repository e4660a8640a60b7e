"""The DyrosDynamicWalk actor at play time: the reference player's deterministic or stochastic action from a trained
network, clamp(mu, -1, 1) or clamp(mu + exp(sigma) * noise, -1, 1), mu = mu(actor_mlp(obs)) in fp32 and eval mode.

backend="hip" runs dwp_play (include/dyros_ppo.h) on the DWP parameter layout: `p` holds the fp32 parameters of both nets as FusedPpoUpdate keeps
them (W1 padded to 512 columns, the heads to 16 rows, all pads zero; the critic's part stays zero here) and `p32f` the weights in dwp_policy's
operand order, so a network trained by the fused update plays without repacking.  backend="torch" runs the module's own forward in fp32.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from . import ppo_update as U
from .ppo_update import ACT, HID, IN, INP, NBT, NP, NWT, OUTP, _req

PREFIX = "a2c_network."
ACTOR_KEYS = ["sigma", "actor_mlp.0.weight", "actor_mlp.0.bias", "actor_mlp.2.weight", "actor_mlp.2.bias", "mu.weight", "mu.bias"]


def param_views(flat: torch.Tensor) -> dict:
    """Views of a flat [NP] tensor in the DWP parameter layout: W1 [2, HID, INP], W2 [2, HID, HID], W3 [2, OUTP, HID], b1, b2 [2, HID], b3 [2, OUTP]
    (index 0 the actor, 1 the critic)."""
    if tuple(flat.shape) != (NP,):
        raise ValueError("param_views: a flat tensor of %d elements is required, got %r" % (NP, tuple(flat.shape)))
    out, o = {}, 0
    for name, shape in (("W1", (2, HID, INP)), ("W2", (2, HID, HID)), ("W3", (2, OUTP, HID)), ("b1", (2, HID)), ("b2", (2, HID)), ("b3", (2, OUTP))):
        n = shape[0] * shape[1] * (shape[2] if len(shape) > 2 else 1)
        out[name] = flat[o:o + n].view(shape)
        o += n
    assert o == NWT + NBT
    return out


def tensor_views(flat: torch.Tensor) -> dict:
    """The network's state_dict names (both nets, sigma excluded) as views of a flat [NP] tensor in the DWP layout, pads left out."""
    v = param_views(flat)
    out = {}
    for k, (trunk, head, rows) in enumerate((("actor_mlp", "mu", ACT), ("critic_mlp", "value", 1))):
        out[trunk + ".0.weight"], out[trunk + ".0.bias"] = v["W1"][k, :, :IN], v["b1"][k]
        out[trunk + ".2.weight"], out[trunk + ".2.bias"] = v["W2"][k], v["b2"][k]
        out[head + ".weight"], out[head + ".bias"] = v["W3"][k, :rows], v["b3"][k, :rows]
    return out


class Actor(nn.Module):
    """The actor's half of examples/ppo_consumer.py's DyrosActorCritic, with its state_dict names."""

    def __init__(self, num_obs: int = IN, num_act: int = ACT, units: int = HID):
        super().__init__()
        self.actor_mlp = nn.Sequential(nn.Linear(num_obs, units), nn.ReLU(), nn.Linear(units, units), nn.ReLU())
        self.mu = nn.Linear(units, num_act)
        self.sigma = nn.Parameter(torch.zeros(num_act), requires_grad=False)

    def forward(self, obs):
        return self.mu(self.actor_mlp(obs))


class WalkPolicy:
    """play(obs, noise=None) -> (clamped, mu) of the walk actor; see the module docstring for the two backends."""

    def __init__(self, device="cuda:0", backend: str = "hip"):
        if backend not in ("hip", "torch"):
            raise ValueError("WalkPolicy: backend must be 'hip' or 'torch', got %r" % (backend,))
        self.device, self.backend = torch.device(device), backend
        self.net = Actor().to(self.device).eval()
        self.num_obs, self.num_acts = IN, ACT
        if backend == "hip":
            if self.device.type != "cuda":
                raise ValueError("WalkPolicy: backend 'hip' needs a GPU device, got %s" % self.device)
            self.api = U.declare(_lib.load()[0])
            self.p = torch.zeros(NP, device=self.device)
            self.p32f = torch.zeros(U.K["DWP_P32F_WORDS"], device=self.device)
            self._work = torch.zeros(1, device=self.device)
        self._pack()

    @property
    def logstd(self) -> torch.Tensor:
        return self.net.sigma.data

    @classmethod
    def from_module(cls, net: nn.Module, device=None, backend: str = "hip") -> "WalkPolicy":
        """From DyrosActorCritic, or any module with actor_mlp (Linear, ReLU, Linear, ReLU), mu and sigma."""
        pol = cls(device if device is not None else net.mu.weight.device, backend)
        sd = net.state_dict()
        pol.load_state_dict({k: sd[k] for k in ACTOR_KEYS})
        return pol

    def state_dict(self) -> dict:
        return {k: v.detach().clone() for k, v in self.net.state_dict().items()}

    def load_state_dict(self, sd: dict):
        """The actor's tensors by name: the network's own names, or the checkpoint's `a2c_network.` names (other keys are ignored)."""
        sd = {(k[len(PREFIX):] if k.startswith(PREFIX) else k): v for k, v in sd.items()}
        own = self.net.state_dict()
        missing = [k for k in ACTOR_KEYS if k not in sd]
        if missing:
            raise KeyError("WalkPolicy.load_state_dict: missing %s" % missing)
        for k in ACTOR_KEYS:
            if tuple(sd[k].shape) != tuple(own[k].shape):
                raise ValueError("WalkPolicy.load_state_dict: %s is %r, this actor's is %r" % (k, tuple(sd[k].shape), tuple(own[k].shape)))
        with torch.no_grad():
            for k in ACTOR_KEYS:
                own[k].copy_(sd[k].to(device=self.device, dtype=torch.float32))
        self._pack()

    def _pack(self):
        """The HIP backend's copies of the module: p in the DWP layout (pads zero), then p32f (dwp_retile32)."""
        if self.backend != "hip":
            return
        tv = tensor_views(self.p)
        with torch.no_grad():
            self.p.zero_()
            for k, v in self.net.state_dict().items():
                if k != "sigma":
                    tv[k].copy_(v)
        s = torch.cuda.current_stream(self.device).cuda_stream
        self._chk(self.api["retile32"](self.p.data_ptr(), self.p32f.data_ptr(), s))

    def _chk(self, rc):
        _lib.check(self.api, rc)

    def work_floats(self, n: int) -> int:
        return int(self.api["play_work_floats"](int(n)))

    def play(self, obs: torch.Tensor, noise: torch.Tensor = None):
        """(clamped [N, 13], mu [N, 13]) for obs [N, 487]: clamp(mu, -1, 1), or clamp(mu + exp(sigma) * noise, -1, 1) with noise [N, 13]."""
        if not (torch.is_tensor(obs) and obs.dim() == 2 and obs.shape[1] == IN and obs.shape[0] >= 1):
            raise ValueError("WalkPolicy.play: obs must be [N, %d], got %r" % (IN, tuple(obs.shape) if torch.is_tensor(obs) else type(obs).__name__))
        N = int(obs.shape[0])
        if noise is not None and not (torch.is_tensor(noise) and tuple(noise.shape) == (N, ACT)):
            raise ValueError("WalkPolicy.play: noise must be [%d, %d]" % (N, ACT))
        if self.backend == "torch":
            with torch.no_grad():
                mu = self.net(obs.to(torch.float32))
                a = mu if noise is None else mu + torch.exp(self.net.sigma) * noise
                return torch.clamp(a, -1.0, 1.0), mu
        _req("WalkPolicy.play: obs", obs, torch.float32, shape=(N, IN))
        if noise is not None:
            _req("WalkPolicy.play: noise", noise, torch.float32, shape=(N, ACT))
        logstd = _req("WalkPolicy.play: sigma", self.logstd, torch.float32, ACT)
        need = self.work_floats(N)
        if need < 0:
            raise ValueError("WalkPolicy.play: no workspace size for %d rows" % N)
        if self._work.numel() < need:
            self._work = torch.zeros(need, device=self.device)          # (a captured play needs it to exist before the capture)
        work = _req("WalkPolicy.play: workspace", self._work, torch.float32)
        clamped, mu = torch.empty(N, ACT, device=self.device), torch.empty(N, ACT, device=self.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        self._chk(self.api["play"](self.p.data_ptr(), self.p32f.data_ptr(), logstd.data_ptr(), obs.data_ptr(),
                                   None if noise is None else noise.data_ptr(), N, clamped.data_ptr(), mu.data_ptr(), work.data_ptr(),
                                   int(work.numel()), s))
        return clamped, mu

