"""What the *_time.py tools of the model tensors and the gait profile measure with: an env with one cfg sim.mi355 key set, a kernel's time in
a captured chain, an eager call's time, and an eager env.step()'s."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def make_env(n, key, spec):
    """A DyrosDynamicWalk of n envs with cfg sim.mi355[key] = spec (None: the key stays absent)."""
    from isaacgymdyros_amd.config import default_cfg
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, DEV)
    if spec is not None:
        cfg["sim"]["mi355"][key] = spec
    return DyrosDynamicWalk(cfg, DEV, 0, True)


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


def step_ms(n, key, spec, steps, warm, flag=False):
    """The row of an eager env.step() in milliseconds with cfg sim.mi355[key] = spec; flag: the row says whether the key is set, not the spec."""
    env = make_env(n, key, spec)
    g = torch.Generator(device=DEV).manual_seed(0)
    a = (torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05
    for _ in range(warm):
        env.step(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        env.step(a)
    e1.record()
    torch.cuda.synchronize()
    env.close()
    return {"eager_step": True, key: spec is not None if flag else spec, "num_envs": n, "steps": steps, "ms_per_step": e0.elapsed_time(e1) / steps}
