"""What the *_time.py tools of the model tensors and the recorders measure with: an env with one cfg sim.mi355 key set, a kernel's time in
a captured chain, an eager call's time, and an eager env.step()'s.  Every time is taken with device events."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def make_env(n, key, spec, alias_obs=False):
    """A DyrosDynamicWalk of n envs with cfg sim.mi355[key] = spec (None: the key stays absent)."""
    from isaacgymdyros_amd.config import default_cfg
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, DEV)
    if spec is not None:
        cfg["sim"]["mi355"][key] = spec
    if alias_obs:
        cfg["sim"]["mi355"]["alias_obs"] = True
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def make_amp_env(n, mi355, env=None):
    """A TocabiAMPLower of n envs with cfg sim.mi355 = mi355 and cfg env updated with env."""
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"]["mi355"] = dict(mi355)
    cfg["env"].update(env or {})
    return TocabiAMPLower(cfg, DEV, 0, True)


def actions(n, cols=13, scale=1.0):
    """Eight action tensors in [-scale, scale], seed 0: step t takes number t % 8."""
    g = torch.Generator(device=DEV).manual_seed(0)
    return [(torch.rand(n, cols, generator=g, device=DEV) * 2 - 1) * scale for _ in range(8)]


def chain_us(fn, launches, chain=100):
    """Microseconds per fn() from device events around replays of a captured chain of fn(), so that the host's launch rate does not bound it."""
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        for _ in range(chain):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches // chain):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (launches // chain * chain) * 1e3


def eager_us(fn, calls):
    """Microseconds per eager fn(), the host's launch cost included."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def loop_ms(step, steps, warm):
    """Milliseconds per eager step(t), t = 0 .. steps - 1, after warm calls."""
    for t in range(warm):
        step(t)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(steps):
        step(t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def step_ms(n, key, spec, steps, warm, flag=False):
    """The row of an eager env.step() in milliseconds with cfg sim.mi355[key] = spec; flag: the row says whether the key is set, not the spec."""
    env = make_env(n, key, spec)
    g = torch.Generator(device=DEV).manual_seed(0)
    a = (torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05
    ms = loop_ms(lambda t: env.step(a), steps, warm)
    env.close()
    return {"eager_step": True, key: spec is not None if flag else spec, "num_envs": n, "steps": steps, "ms_per_step": ms}
