"""The forward dynamics on an MI355X (include/dyros_forward_dynamics.h, csrc/dw_forward_dynamics.hip): the HIP kernel
against the float64 reference of tests/forward_dynamics_ref.py under its measured tolerance at the workgroup's edges, with the output buffers
filled with NaN, too long, and their tails watched; the derived backward-error bound against dwj_mass_matrix's own M; the ways to choose
outputs; unaligned outputs; the counts of right-hand sides; agreement with the shipped dwn_inverse_dynamics and dwj_mass_matrix; the outputs'
exact properties; a live env with resets; a captured step plus every call; TocabiAMPLower; the player's files."""
import numpy as np
import pytest
import torch

import dynamics_ref as DR
import forward_dynamics_ref as FR
from isaacgymdyros_amd import forward_dynamics as FM
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd.model import load_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = FM.GROUP          # envs per workgroup
RMAX = FM.MAX_RHS
PAD = 64
F, U = np.float32, np.uint32
OUTS = ("x", "factor", "minv")


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return __import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0]


@pytest.fixture(scope="module")
def api():
    return FM.declare(lib())


@pytest.fixture(scope="module")
def table(api):
    return torch.from_numpy(FM.pack_table(api, load_model()).view(np.int32)).to(DEV)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t, offset=0):
    return None if t is None else t.data_ptr() + 4 * offset


def run(api, table, root, dof, ms, arm, vel_at_com, rhs=None, sub=None, outs=OUTS, offset=0, finite=True, expect=0, nrhs=None):
    """One launch into NaN-filled buffers PAD words too long (and `offset` words past their start); returns the outputs named as a dict (the
    others None): every word written (when the inputs were finite), none outside."""
    n = len(root)
    r = (0 if rhs is None else rhs.shape[1]) if nrhs is None else nrhs
    words = {"x": (0 if rhs is None else rhs.shape[1]) * 39, "factor": 1521, "minv": 1521}
    shape = {"x": (n, 0 if rhs is None else rhs.shape[1], 39), "factor": (n, 39, 39), "minv": (n, 39, 39)}
    d = [dev(root), dev(dof), dev(ms), dev(arm), dev(rhs), dev(sub)]
    buf = {k: torch.full((offset + n * words[k] + PAD,), float("nan"), device=DEV) if k in outs and words[k] > 0 else None for k in OUTS}
    assert all(b is None or b.data_ptr() % 16 == 0 for b in buf.values())
    rc = api["solve"](n, table.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), vel_at_com, ptr(d[4]), r, ptr(d[5]),
                      ptr(buf["x"], offset), ptr(buf["factor"], offset), ptr(buf["minv"], offset), stream())
    torch.cuda.synchronize()          # (d is freed after this)
    assert rc == expect, api["last_error"]()
    out = {}
    for k in OUTS:
        if buf[k] is None:
            out[k] = None
            continue
        h, w = buf[k].cpu().numpy(), n * words[k]
        if rc != 0:
            assert np.isnan(h).all()          # nothing was launched
            out[k] = None
            continue
        assert np.isnan(h[:offset]).all() and np.isnan(h[offset + w:]).all(), "a word outside %s was written" % k
        o = h[offset:offset + w]
        if finite:
            assert np.isfinite(o).all(), "%d words of %s were not written" % (int(np.isnan(o).sum()), k)
        out[k] = o.reshape(shape[k]).copy()
    return out


def mass_matrix(table, root, dof, ms, arm, vel_at_com):
    """dwj_mass_matrix's M of the same inputs (the first DWJ_TABLE_WORDS words of the table are dwj_pack_table's)."""
    n = len(root)
    d = [dev(root), dev(dof), dev(ms), dev(arm)]
    M = torch.zeros(n, 39, 39, device=DEV)
    assert JM.declare(lib())["mass_matrix"](n, table.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), vel_at_com, M.data_ptr(), None, stream()) == 0
    torch.cuda.synchronize()
    return M.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(a.view(U), b.view(U))


# ---------------------------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("n", [1, G - 1, G, G + 1, 3 * G + 5])
def test_kernel_against_float64(api, table, n, vel_at_com):
    """n = 1: one env in one workgroup; G - 1, G, G + 1: the group's edge; 3 G + 5: four whole groups and a partial one.  Every channel within
    4 d; L' D L, formed in float64 from the factor, against dwj_mass_matrix's own M within 2 gamma_18 (|L'| |D| |L|)_ij."""
    root, dof, ms, arm, _acc = DR.seeded(n, 100 * n + vel_at_com)
    rhs = FR.rhs_of(root, dof, vel_at_com, ms, arm, 2, 7 + n)
    sub = DR.evaluate(root, dof, vel_at_com, ms, arm)["bias"].astype(F)
    o = run(api, table, root, dof, ms, arm, vel_at_com, rhs, sub)
    ex = FR.excess(o, root, dof, ms, arm, vel_at_com, rhs, sub, report="gpu n=%d vel_at_com=%d" % (n, vel_at_com))
    assert len(ex) == len(FR.CHANNELS) and FR.within(ex), ex
    be = FR.backward_error(o["factor"], mass_matrix(table, root, dof, ms, arm, vel_at_com))
    print("gpu: L' D L against dwj_mass_matrix: %.3f of 2 gamma_18 |L'| |D| |L|" % be)
    assert be <= 1.0
    # the factor's zeros and minv's symmetry, with the buffers filled with NaN beforehand
    assert (o["factor"].view(U)[:, ~FR.MASK] == 0).all() and same_bits(o["minv"], np.ascontiguousarray(np.swapaxes(o["minv"], 1, 2)))


def test_output_selection_and_unaligned_outputs(api, table):
    """Every single output, every pair, all three, with and without mass scale and armature, every count of right-hand sides, and every output
    4 bytes past a 16-byte boundary: the same bits where the same is asked."""
    n = 2 * G + 3
    root, dof, ms, arm, _acc = DR.seeded(n, 10)
    rhs = FR.rhs_of(root, dof, 0, ms, arm, RMAX, 12)
    full = run(api, table, root, dof, ms, arm, 0, rhs)
    for k in OUTS:
        one = run(api, table, root, dof, ms, arm, 0, rhs if k == "x" else None, outs=(k,))
        assert same_bits(one[k], full[k]), k
        rest = run(api, table, root, dof, ms, arm, 0, None if k == "x" else rhs, outs=tuple(j for j in OUTS if j != k))
        assert all(same_bits(rest[j], full[j]) for j in OUTS if j != k), k
    off = run(api, table, root, dof, ms, arm, 0, rhs, offset=1)
    assert all(same_bits(off[k], full[k]) for k in OUTS)
    # column r is the same bits at nrhs = 1, 2 and the maximum, beside M^-1's columns or alone
    for k in (1, 2):
        ok = run(api, table, root, dof, ms, arm, 0, np.ascontiguousarray(rhs[:, :k]), outs=("x",))
        assert same_bits(ok["x"], np.ascontiguousarray(full["x"][:, :k])), k
    last = run(api, table, root, dof, ms, arm, 0, np.ascontiguousarray(rhs[:, RMAX - 1:]), outs=("x", "minv"))
    assert same_bits(last["x"][:, 0], full["x"][:, RMAX - 1]) and same_bits(last["minv"], full["minv"])
    # column c of minv is the solve of the identity's column c
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(39, dtype=F)[:RMAX], (n, RMAX, 39)))
    oe = run(api, table, root, dof, ms, arm, 0, eye, outs=("x",))
    assert all(same_bits(np.ascontiguousarray(oe["x"][:, c, c:]), np.ascontiguousarray(full["minv"][:, c:, c])) for c in range(RMAX))
    # sub NULL equals sub of zeros; a zero right-hand side gives zeros
    oz = run(api, table, root, dof, ms, arm, 0, rhs, np.zeros((n, 39), F), outs=("x",))
    assert same_bits(oz["x"], full["x"])
    assert (run(api, table, root, dof, ms, arm, 0, np.zeros((n, 2, 39), F), outs=("x",))["x"] == 0).all()
    # with the armature off, M's diagonal lacks it: the last row of M is eliminated by no other, so D[38] = M[38][38]
    na = run(api, table, root, dof, ms, None, 0, outs=("factor",))
    M_na, M = mass_matrix(table, root, dof, ms, None, 0), mass_matrix(table, root, dof, ms, arm, 0)
    assert same_bits(na["factor"][:, 38, 38], M_na[:, 38, 38]) and same_bits(full["factor"][:, 38, 38], M[:, 38, 38])
    assert same_bits(M_na[:, 38, 38] + arm[:, 32], M[:, 38, 38])
    assert FR.backward_error(na["factor"], M_na) <= 1.0
    # nominal masses, no armature, vel_at_com: another matrix, under the d measured for it
    r1 = FR.rhs_of(root, dof, 1, None, None, 1, 14)
    nom = run(api, table, root, dof, None, None, 1, r1)
    ex = FR.excess(nom, root, dof, None, None, 1, r1, report="gpu, nominal masses, no armature")
    assert FR.within(ex), ex
    assert FR.backward_error(nom["factor"], mass_matrix(table, root, dof, None, None, 1)) <= 1.0
    # refused before any launch: nothing is written
    assert run(api, table, root, dof, ms, arm, 0, rhs, nrhs=RMAX + 1, expect=-1)["x"] is None and b"nrhs" in api["last_error"]()
    assert run(api, table, root, dof, ms, arm, 0, rhs, nrhs=0, expect=-1)["minv"] is None and b"nrhs" in api["last_error"]()


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_residual_against_the_shipped_mass_matrix(api, table, vel_at_com):
    """dwj_mass_matrix's M times x, formed in float64, returns the right-hand side within the factorisation's derived bound scaled by |x|:
    |M x - b|_i <= sum_j 2 gamma_18 (|L'| |D| |L|)_ij |x_j|."""
    n = 3 * G + 5
    root, dof, ms, arm, _acc = DR.seeded(n, 13 + vel_at_com)
    rhs = FR.rhs_of(root, dof, vel_at_com, ms, arm, 2, 15)
    o = run(api, table, root, dof, ms, arm, vel_at_com, rhs, outs=("x", "factor"))
    M = mass_matrix(table, root, dof, ms, arm, vel_at_com).astype(np.float64)
    f = o["factor"].astype(np.float64)
    i = np.arange(39)
    D, L = f[:, i, i], np.tril(f, -1)
    L[:, i, i] = 1
    bound = 2 * FR.gamma(18) * np.einsum("nki,nk,nkj->nij", np.abs(L), np.abs(D), np.abs(L))
    x = o["x"].astype(np.float64)
    err = np.abs(np.einsum("nab,nrb->nra", M, x) - rhs.astype(np.float64))
    allow = np.einsum("nab,nrb->nra", bound, np.abs(x))
    print("M x against rhs: %.2e on values up to %.0f, %.3f of the bound" % (err.max(), np.abs(rhs).max(), (err / allow).max()))
    assert (err <= allow).all()


def test_exact_properties(api, table):
    n = 2 * G + 3
    root, dof, ms, arm, _acc = DR.seeded(n, 8)
    rhs = FR.rhs_of(root, dof, 1, ms, arm, 2, 9)
    o = run(api, table, root, dof, ms, arm, 1, rhs)
    # 640 m out: the same bits
    far = root.copy()
    far[:, 0:2] += np.array([640.0, -640.0], F)
    of = run(api, table, far, dof, ms, arm, 1, rhs)
    assert all(same_bits(of[k], o[k]) for k in OUTS)
    # a NaN stays in its env; one in a right-hand side reaches that column of x alone
    bad_r, bad_d, bad_b = root.copy(), dof.copy(), rhs.copy()
    bad_r[2, 4], bad_d[G + 1, 20, 0], bad_b[7, 1, 7] = np.nan, np.inf, np.nan
    on = run(api, table, bad_r, bad_d, ms, arm, 1, bad_b, finite=False)
    keep = [e for e in range(n) if e not in (2, G + 1, 7)]
    for k in OUTS:
        assert same_bits(on[k][keep], o[k][keep]), k
        assert np.isnan(on[k][2]).any() and np.isnan(on[k][G + 1]).any(), k
    assert np.isnan(on["x"][7, 1]).any() and same_bits(on["x"][7, 0], o["x"][7, 0]) and all(same_bits(on[k][7], o[k][7]) for k in ("factor", "minv"))


# ---------------------------------------------------------------------------------------------- envs
def make_env(n, spec=None, **mi):
    from isaacgymdyros_amd.config import default_cfg
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, DEV)
    cfg["seed"] = 42
    cfg["env"]["episodeLength"] = 0.1          # (seconds; 0.004 s per policy step: every env meets the time limit at step 25)
    cfg["sim"]["mi355"]["device_step_counter"] = True
    cfg["sim"]["mi355"]["alias_obs"] = True
    cfg["sim"]["mi355"].update(mi)
    if spec is not None:
        cfg["sim"]["mi355"]["forward_dynamics"] = spec
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def actions(n, steps, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.tensor([0.0, 0.05, 0.3, 1.0], device=DEV)[torch.arange(n, device=DEV) % 4].view(1, n, 1)
    return ((torch.rand(steps, n, 13, generator=g, device=DEV) * 2 - 1) * amp).contiguous()


def bits(*ts):
    return torch.cat([t.contiguous().reshape(-1).view(torch.uint8) for t in ts])


def buffers(env, n):
    b = env._buf
    return tuple(b[k].cpu().numpy().reshape(s) for k, s in (("root_states", (n, 13)), ("dof_state", (n, 33, 2)), ("mass_scale", (n, 38)), ("dof_armature", (n, 33))))


def test_forward_of_inverse_returns_the_acceleration():
    """forward_dynamics(gen_force = dynamics.inverse_dynamics(a)) == a on a stepped env.  The allowance is the sum of both: 4 d of x for the
    solve of an exact right-hand side, and what dwn_inverse_dynamics' own allowances (4 d of tau, and 4 d of bias for the h that the solve
    subtracts) become through |M^-1|, formed in float64."""
    n = 64
    env = make_env(n, {"rhs": 2}, dynamics={"inverse_dynamics": True})
    fd, dy = env.forward_dynamics, env.dynamics
    a = torch.zeros(n, 13, device=DEV)
    acts = actions(n, 6, seed=5)
    for i in range(6):
        a.copy_(acts[i])
        env.step(a)
    acc = DR.accel_of(n, 77)
    tau = dy.inverse_dynamics(torch.from_numpy(acc).to(DEV))
    got = fd.forward_dynamics(gen_force=tau).cpu().numpy().astype(np.float64)
    assert fd.accel.shape == (n, 39) and fd.forward_dynamics(gen_force=tau) is fd.accel
    root, dof, ms, arm = buffers(env, n)
    v = fd.vel_at_com
    dn, dx = DR.measured(v), FR.measured(v)
    Minv = np.abs(np.linalg.inv(FR.mass_matrix(root, dof, v, ms, arm)))
    row = np.array([dn["tau_lin"] + dn["bias_lin"]] * 3 + [dn["tau_ang"] + dn["bias_ang"]] * 3 + [dn["tau_joint"] + dn["bias_joint"]] * 33)
    own = np.array([dx["x_lin"]] * 3 + [dx["x_ang"]] * 3 + [dx["x_joint"]] * 33)
    allow = FR.FACTOR * own[None, :] + DR.FACTOR * (Minv @ row)
    err = np.abs(got - acc.astype(np.float64))
    print("forward(inverse(a)) - a: %.2e with |a| up to %.0f, %.3f of the allowance" % (err.max(), np.abs(acc).max(), (err / allow).max()))
    assert (err <= allow).all()
    # tau_joint and gen_force add up: [0; tau[6:]] + [tau[0:6]; 0] is the same right-hand side
    gf = tau.clone()
    gf[:, 6:] = 0
    again = fd.forward_dynamics(tau_joint=tau[:, 6:], gen_force=gf).cpu().numpy()
    assert same_bits(again, got.astype(F))
    # solve(): [N, R, 39]; column 0 of two is the bits of a fresh launch with one
    rhs = FR.rhs_of(root, dof, v, ms, arm, 2, 79)
    x = fd.solve(torch.from_numpy(rhs).to(DEV))
    assert x is fd.x and x.shape == (n, 2, 39) and fd.rhs.shape == (n, 2, 39) and fd.factor is None and fd.minv is None
    ex = FR.excess({"x": x.cpu().numpy()}, root, dof, ms, arm, v, rhs)
    env.close()
    assert FR.within(ex), ex


def test_live_env_with_resets(api, table):
    n, steps = 64, 40
    acts = actions(n, steps)
    runs = {}
    every = {"rhs": 2, "factor": True, "minv": True, "auto": True}
    for name, spec, mi in (("off", None, {}), ("auto", every, {}), ("beside", {"minv": True, "auto": True, "armature": False}, {"episode_stats": True})):
        env = make_env(n, spec, **mi)
        a, h, resets = torch.zeros(n, 13, device=DEV), [], 0
        if spec is None:
            assert env.forward_dynamics is None
        for i in range(steps):
            a.copy_(acts[i])
            o, r, d, _ex = env.step(a)
            h.append(bits(o["obs"], r, d, env._buf["root_states"], env._buf["env_state"]))
            resets += int(d.sum())
            if name == "auto" and (i % 3 == 0 or i == steps - 1):
                fd = env.forward_dynamics
                held = {k: getattr(fd, k).cpu().numpy().copy() for k in ("factor", "minv")}
                root, dof, ms, arm = buffers(env, n)
                rhs = FR.rhs_of(root, dof, fd.vel_at_com, ms, arm, 2, i)
                x = fd.solve(torch.from_numpy(rhs).to(DEV)).cpu().numpy()
                fresh = run(api, table, root, dof, ms, arm, fd.vel_at_com, rhs)
                assert all(same_bits(held[k], fresh[k]) for k in held) and same_bits(x, fresh["x"]), i
                if i % 12 == 0 or i == steps - 1:
                    ex = FR.excess(fresh, root, dof, ms, arm, fd.vel_at_com, rhs)
                    assert FR.within(ex), (i, ex)
        if name == "auto":
            assert fd.vel_at_com == 1 and fd.dof_names == load_model().dof_names and fd.nrhs == 2
            assert fd.factor.shape == fd.minv.shape == (n, 39, 39) and fd.x.shape == fd.rhs.shape == (n, 2, 39)
            # reset_idx refreshes too: the tensors are those of the buffers after it
            before = fd.minv.clone()
            env.reset_idx(torch.arange(0, n, 2, device=DEV))
            held = fd.minv.clone()
            fd.refresh()
            assert torch.equal(fd.minv, held) and not torch.equal(held[0::2], before[0::2]) and torch.equal(held[1::2], before[1::2])
        if name == "beside":
            fd = env.forward_dynamics
            assert fd.factor is None and fd.minv.shape == (n, 39, 39) and fd.nrhs == 1
            root, dof, ms, arm = buffers(env, n)
            fresh = run(api, table, root, dof, ms, None, fd.vel_at_com, outs=("minv",))
            assert same_bits(fd.minv.cpu().numpy(), fresh["minv"])
        runs[name] = torch.stack(h).cpu()
        env.close()
        assert resets > 0          # (the time limit alone resets every env)
    # the feature only reads: the same bits with the key absent, on, and on beside another recorder in a rebuilt env
    assert torch.equal(runs["off"], runs["auto"]) and torch.equal(runs["off"], runs["beside"])


def test_captured_step_plus_every_call_replays_the_eager_bits():
    """Step, refresh() (auto), solve() and forward_dynamics() recorded in one graph on one stream (a linear chain), replayed 10 times, against
    10 eager steps from the same state."""
    n = 64
    acts = actions(n, 11, seed=3)
    g = torch.Generator(device=DEV).manual_seed(4)
    rhss = torch.randn(11, n, 1, 39, generator=g, device=DEV) * 50
    taus = torch.randn(11, n, 33, generator=g, device=DEV) * 20
    outs = []
    for captured in (False, True):
        env = make_env(n, {"factor": True, "minv": True, "auto": True})
        fd = env.forward_dynamics
        a, tau = torch.zeros(n, 13, device=DEV), torch.zeros(n, 33, device=DEV)
        a.copy_(acts[0])
        env.step(a)                            # (the first step is eager on both sides)
        fd.solve(rhss[0])
        fd.forward_dynamics(tau_joint=tau)
        torch.cuda.synchronize()
        h = []
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            gr = torch.cuda.CUDAGraph()
            a.copy_(acts[1])
            with torch.cuda.graph(gr, stream=side):
                env.step(a)
                fd.solve()
                fd.forward_dynamics(tau_joint=tau)
            # (the capture itself ran nothing: replay the recorded step for each of the 10 actions)
        for i in range(1, 11):
            a.copy_(acts[i])
            tau.copy_(taus[i])
            fd.rhs.copy_(rhss[i])
            if captured:
                gr.replay()
            else:
                env.step(a)
                fd.solve()
                fd.forward_dynamics(tau_joint=tau)
            h.append(bits(fd.factor, fd.minv, fd.x, fd.accel, env._buf["root_states"]))
        torch.cuda.synchronize()
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1])


def test_tocabi_amp_lower():
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    n = 32
    cfg = default_amp_cfg(n, DEV)
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert amp.forward_dynamics is None
    amp.close()
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"].setdefault("mi355", {})["amp_forward_dynamics"] = {"factor": True, "minv": True, "auto": True}
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert isinstance(amp.forward_dynamics, FM.ForwardDynamics) and amp._phys.forward_dynamics is None
    fd = amp.forward_dynamics
    assert fd.vel_at_com == int(amp._phys._ccfg.root_vel_at_com)
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(20):
        amp.step((torch.rand(n, amp.num_actions, generator=g, device=DEV) * 2 - 1) * 0.1)
    root, dof, ms, arm = buffers(amp._phys, n)
    rhs = FR.rhs_of(root, dof, fd.vel_at_com, ms, arm, 1, 7)
    x = fd.solve(torch.from_numpy(rhs[:, 0]).to(DEV))          # ([N, 39] for one right-hand side)
    assert x is fd.x
    got = {k: getattr(fd, k).cpu().numpy() for k in OUTS}          # (factor, minv: what the last step's auto refresh left)
    ex = FR.excess(got, root, dof, ms, arm, fd.vel_at_com, rhs, report="TocabiAMPLower")
    amp.close()
    assert len(ex) == len(FR.CHANNELS) and FR.within(ex), ex


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_accelerations(tmp_path):
    import importlib.util
    import os
    import subprocess
    import sys
    from isaacgymdyros_amd import ppo_checkpoint as PK
    from isaacgymdyros_amd import ppo_update as UP
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(root, "examples", "ppo_consumer.py"))
    ppo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ppo)
    torch.manual_seed(3)
    net = ppo.DyrosActorCritic(UP.IN, UP.ACT, ppo.TRAIN_CFG["network"]).to(DEV)          # an untrained policy
    c = ppo.TRAIN_CFG["config"]
    ck = PK.save(str(tmp_path / "p.pth"), net, epoch=0, opt_actor=torch.optim.Adam(net.actor_parameters(), lr=c["learning_rate"]),
                 opt_critic=torch.optim.Adam(net.critic_parameters(), lr=c["critic_lr"]))
    files = {}
    for name, flag in (("plain", []), ("accel", ["--dynamics-accel", "--dynamics-forces"])):
        out = tmp_path / name
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64",
                            "--games", "64", "--max-steps", "60", "--episode-length", "0.1", "--dynamics-dir", str(out), "--dynamics-envs", "2"] + flag,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["dynamics_env0.npz", "dynamics_env1.npz"]
        files[name] = np.load(out / "dynamics_env1.npz")
    plain, z = files["plain"], files["accel"]
    old = ["names", "dof_names", "dt", "jacobian", "mass_matrix", "com_jacobian"]
    assert sorted(plain.files) == sorted(old) and sorted(z.files) == sorted(old + ["bias", "gravity", "momentum", "minv", "accel_zero_torque"])
    assert all(np.array_equal(plain[k], z[k]) for k in old)          # (the same seed: the files are what they were, plus the new arrays)
    T = z["jacobian"].shape[0]
    assert 20 <= T <= 60 and z["minv"].shape == (T, 39, 39) and z["accel_zero_torque"].shape == (T, 39)
    assert np.isfinite(z["minv"]).all() and np.isfinite(z["accel_zero_torque"]).all() and same_bits(z["minv"], np.ascontiguousarray(np.swapaxes(z["minv"], 1, 2)))
    # M^-1 (-h) with the files' own M and h (the bits the kernel factored and subtracted), solved in float64: within 4 d of x, which also pays
    # for the chain and for forming M, scaled to the size of a falling robot's accelerations (forward_dynamics_ref.x_allowance)
    M, hb = z["mass_matrix"].astype(np.float64), z["bias"].astype(np.float64)
    want = np.linalg.solve(M, -hb[..., None])[..., 0]
    allow = FR.x_allowance(want, 1)
    err = np.abs(z["accel_zero_torque"].astype(np.float64) - want)
    print("the player's accel_zero_torque: %.3f of the allowance" % (err / allow).max())
    assert (err <= allow).all()
