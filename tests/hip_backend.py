"""Replay backend over the real HIP library (through the product's host class).  GPU tests only."""
import numpy as np
import torch

from isaacgymdyros_amd import abi
from isaacgymdyros_amd.config import default_cfg
from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk


def make_env(N, **mi):
    cfg = default_cfg(N, "cuda:0")
    dr = mi.pop("randomize", True)
    cfg["task"]["randomize"] = dr
    if mi.pop("friction_dr", False):
        from isaacgymdyros_amd.config import with_friction_randomization
        cfg = with_friction_randomization(cfg)
    terrain = mi.pop("terrain", None)
    if terrain:
        from isaacgymdyros_amd.config import with_terrain
        cfg = with_terrain(cfg, **terrain)
    seed = mi.pop("seed", None)
    if seed is not None:
        cfg["seed"] = seed
    # env / sim / physx: overrides of the YAML's own sections (deathCost, episodeLength, dt, gravity, solver iterations, ...)
    cfg["env"].update(mi.pop("env", {}))
    cfg["sim"]["physx"].update(mi.pop("physx", {}))
    cfg["sim"].update(mi.pop("sim", {}))
    cfg["sim"]["mi355"].update(mi)
    return DyrosDynamicWalk(cfg, "cuda:0", 0, True)


class HipBackend:
    def __init__(self, N, **mi):
        self.env = make_env(N, **mi)

    def load_buffers(self, bufs):
        for k, v in bufs.items():
            t = self.env._buf[k]
            t.copy_(torch.from_numpy(np.ascontiguousarray(v)).to(t.device).view(t.shape))

    def write_state(self, root, dof, cf):
        self.load_buffers({"root_states": root, "dof_state": dof, "contact_forces": cf})

    def step(self, a, nz, t):
        self.env._step_count = t
        noise = None if nz is None else torch.from_numpy(np.ascontiguousarray(nz)).cuda()
        self.env.step(torch.from_numpy(np.ascontiguousarray(a)).cuda(), noise)
        torch.cuda.synchronize()

    def read_buffers(self):
        return {k: v.cpu().numpy() for k, v in self.env._buf.items()}


class HipSim:
    """The HIP library behind the same driver as OracleSim / EmulSim, from a DwConfig given field by field (fields the
    host class pins, max_angular_velocity among them, included): numpy buffers in `buf`, mirrored to device tensors
    before every call and read back after it."""

    def __init__(self, num_envs, task_const=None, terrain=None, **cfg_over):
        import ctypes as C
        from isaacgymdyros_amd import _lib
        from isaacgymdyros_amd.dyros_dynamic_walk import _TORCH_DT
        from oracle.oracle import OracleSim
        # the oracle's driver builds config, model, task constants and initial buffers; only the library differs
        self._host = OracleSim(num_envs, task_const=task_const, terrain=terrain, **cfg_over)
        self.cfg, self.N, self.buf = self._host.cfg, num_envs, self._host.buf
        self.lib, self.api = _lib.load()
        self._dev = {k: torch.zeros(v.shape, dtype=_TORCH_DT[v.dtype.str[1:]], device="cuda:0") for k, v in self.buf.items()}
        tptr = C.byref(self._host._task_keep[0]) if self._host._task_keep is not None else None
        self.h = C.c_void_p()
        _lib.check(self.api, self.api["create"](C.byref(self.cfg), C.byref(self._host.cmodel), tptr, C.byref(self.h)))
        db = abi.DwBuffers()
        for name in abi.BUFFER_NAMES:
            setattr(db, name, self._dev[name].data_ptr())
        self._up()          # dw_bind reads height_samples (the coarse bound table of the field is built there): the samples first
        torch.cuda.synchronize()
        _lib.check(self.api, self.api["bind"](self.h, C.byref(db)))

    def _up(self):
        for k, v in self.buf.items():
            self._dev[k].copy_(torch.from_numpy(v))

    def _down(self):
        torch.cuda.synchronize()
        for k, v in self.buf.items():
            v[...] = self._dev[k].cpu().numpy()

    def simulate(self, tau, push=None):
        from isaacgymdyros_amd import _lib
        assert tau.shape == (self.N, 33)
        self._up()
        t = torch.from_numpy(np.ascontiguousarray(tau, dtype=np.float32)).cuda()
        p = None if push is None else torch.from_numpy(np.ascontiguousarray(push, dtype=np.float32)).cuda()
        _lib.check(self.api, self.api["simulate"](self.h, t.data_ptr(), 0 if p is None else p.data_ptr(), torch.cuda.current_stream().cuda_stream))
        self._down()

    def step(self, actions, noise=None, step_index=0):
        from isaacgymdyros_amd import _lib
        assert actions.shape == (self.N, 13)
        self._up()
        a = torch.from_numpy(np.ascontiguousarray(actions, dtype=np.float32)).cuda()
        nz = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)).cuda()
        _lib.check(self.api, self.api["step"](self.h, a.data_ptr(), 0 if nz is None else nz.data_ptr(), step_index, torch.cuda.current_stream().cuda_stream))
        self._down()

    def reset_idx(self, env_ids, noise=None, step_index=0):
        from isaacgymdyros_amd import _lib
        self._up()
        ids = torch.from_numpy(np.ascontiguousarray(env_ids, dtype=np.int32)).cuda()
        nz = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)).cuda()
        _lib.check(self.api, self.api["reset_idx"](self.h, ids.data_ptr(), ids.numel(), 0 if nz is None else nz.data_ptr(), step_index,
                                                   torch.cuda.current_stream().cuda_stream))
        self._down()

    def terrain_log(self):
        """[N, 15 + terrain types] (dw_terrain_log), after a step."""
        from isaacgymdyros_amd import _lib
        out = torch.zeros((self.N, abi.K["DW_NUM_REW"] + int(self.cfg.terrain_num_types)), dtype=torch.float32, device="cuda:0")
        _lib.check(self.api, self.api["terrain_log"](self.h, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def close(self):
        if self.h is not None:
            torch.cuda.synchronize()
            self.api["destroy"](self.h)
            self.h = None
            self._host = None          # (drops the oracle handle that came with the driver)
