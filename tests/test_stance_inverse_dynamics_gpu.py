"""The stance inverse dynamics on an MI355X (include/dyros_stance_inverse_dynamics.h, csrc/dw_contact_inverse.hip): the HIP
kernel against the float64 reference of tests/stance_inverse_dynamics_ref.py under its measured tolerance at the workgroup's edges, with the
four envs of a workgroup in four different stances (flight among them), the output buffers filled with NaN, too long, and their tails
watched; the exact properties against dwi_solve on the device; the ways to choose outputs; a misaligned table; a live env with resets and
stance_from_phase(); a captured step; TocabiAMPLower; the player's files."""
import numpy as np
import pytest
import torch

import contact_dynamics_ref as CR
import contact_inverse_dynamics_ref as IR
import dynamics_ref as DR
import stance_inverse_dynamics_ref as SR
from isaacgymdyros_amd import contact_inverse_dynamics as IM
from isaacgymdyros_amd import stance_inverse_dynamics as SM
from isaacgymdyros_amd.model import load_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = SM.GROUP          # envs per workgroup
PAD = 64
F, U = np.float32, np.uint32
OUTS, IOUTS = SR.OUTS, IR.OUTS
GRAV = DR.GRAVITY
W10 = IR.MOMENTS_10


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return __import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0]


@pytest.fixture(scope="module")
def api():
    return SM.declare(lib())


@pytest.fixture(scope="module")
def iapi():
    return IM.declare(lib())


@pytest.fixture(scope="module")
def tables(api):
    """(K, unit or moments weighted 10 x) -> the device table, the model's soles, mu = 1."""
    model, out = load_model(), {}
    for K in (2, 4):
        cs = SR.SETS[K]
        for w in (None, W10):
            t = SM.pack_table(api, model, CR.ids_of(cs), [p for _, p in cs], None if w is None else np.tile(np.asarray(w, F), K), SR.soles_of(cs), 1.0)
            out[K, w] = torch.from_numpy(t.view(np.int32)).to(DEV)
    return out


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def shapes(n, K):
    return {"tau_joint": (n, 33), "force": (n, 6 * K), "contact_accel": (n, 6 * K), "tau_full": (n, 39), "base_residual": (n, 6), "margins": (n, K, 4), "feasible": (n,)}


def run(api, tables, K, root, dof, ms, arm, vel_at_com, stance=None, accel=None, f_ref=None, weights=None, outs=OUTS, finite=True, expect=0, table=None):
    """One launch into NaN-filled buffers (feasible: 255) PAD words too long; returns the outputs named as a dict (the others None): every
    word written (when the inputs were finite), none outside.  table: a pointer in place of the packed table's."""
    n = len(root)
    shape = shapes(n, K)
    words = {k: int(np.prod(s)) for k, s in shape.items()}
    d = [dev(root), dev(dof), dev(ms), dev(arm), dev(accel), dev(f_ref), dev(None if stance is None else np.asarray(stance, np.uint8))]
    buf = {k: (torch.full((words[k] + PAD,), 255, dtype=torch.uint8, device=DEV) if k == "feasible" else torch.full((words[k] + PAD,), float("nan"), device=DEV))
           if k in outs else None for k in OUTS}
    rc = api["solve"](n, tables[K, weights].data_ptr() if table is None else table, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), *GRAV, ptr(d[4]), ptr(d[5]), ptr(d[6]),
                      vel_at_com, *[ptr(buf[k]) for k in OUTS], stream())
    torch.cuda.synchronize()          # (d is freed after this)
    assert rc == expect, api["last_error"]()
    out = {}
    for k in OUTS:
        if buf[k] is None:
            out[k] = None
            continue
        h, w = buf[k].cpu().numpy(), words[k]
        untouched = (lambda x: (x == 255).all()) if k == "feasible" else (lambda x: np.isnan(x).all())
        if rc != 0:
            assert untouched(h)          # nothing was launched
            out[k] = None
            continue
        assert untouched(h[w:]), "a word outside %s was written" % k
        if finite:
            assert (h[:w] <= 1).all() if k == "feasible" else np.isfinite(h[:w]).all(), "words of %s were not written" % k
        out[k] = h[:w].reshape(shape[k]).copy()
    return out


def irun(iapi, K, contacts, root, dof, ms, arm, vel_at_com, accel=None, f_ref=None, weights=None):
    """dwi_solve on the device for a contact set: section 27's four outputs."""
    n, m = len(root), 6 * len(contacts)
    t = IM.pack_table(iapi, load_model(), CR.ids_of(contacts), [p for _, p in contacts], None if weights is None else np.tile(np.asarray(weights, F), len(contacts)))
    table = torch.from_numpy(t.view(np.int32)).to(DEV)
    d = [dev(root), dev(dof), dev(ms), dev(arm), dev(accel), dev(f_ref)]
    buf = {k: torch.full(s, float("nan"), device=DEV) for k, s in (("tau_joint", (n, 33)), ("force", (n, m)), ("contact_accel", (n, m)), ("tau_full", (n, 39)))}
    assert iapi["solve"](n, table.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), *GRAV, ptr(d[4]), ptr(d[5]), vel_at_com, *[ptr(buf[k]) for k in IOUTS], stream()) == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in buf.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_feasible(got, want, allow):
    clear = (~(want["stance"][:, :, None] != 0) | (np.abs(want["margins"]) > allow)).all((1, 2))
    assert np.array_equal(got[clear], want["feasible"][clear]) and (got[want["stance"].sum(1) == 0] == 0).all()


# ---------------------------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 14])
def test_kernel_against_float64(api, tables, n, K, vel_at_com):
    """A group holds four envs.  n = 1: a lone env; 4: a full group; 5: a group plus one; 2, 3, 14: ragged tails.  Env e takes stance pattern
    (e + s) mod 2^K: the four envs of a workgroup hold four different patterns, the empty one among them.  Unit weights without f_ref and
    moments weighted 10 x with it: every channel within 4 d."""
    root, dof, ms, arm, acc = DR.seeded(n, 100 * n + 10 * K + vel_at_com)
    for s, (w, fr) in enumerate(((None, None), (W10, IR.fref_of(n, 6 * K, n + K)))):
        st = SR.stance_cycle(n, K, 3 * s + (1 << K) - 1)          # (s = 0: the first env stands on every contact, the second is in flight)
        o = run(api, tables, K, root, dof, ms, arm, vel_at_com, st, acc, fr, w)
        want = SR.evaluate(root, dof, vel_at_com, ms, arm, SR.SETS[K], st, acc, w, fr)
        ex = SR.excess(o, want, vel_at_com, K, w, fr is not None, report="gpu n=%d K=%d vel_at_com=%d weights %s" % (n, K, vel_at_com, "unit" if w is None else "10 x"))
        assert len(ex) == len(SR.CHANNELS) and SR.within(ex), ex
        check_feasible(o["feasible"], want, SR.allowance(want, vel_at_com, K, "margins", w, fr is not None))
        flight = st.sum(1) == 0
        assert (o["force"][flight].view(U) == 0).all() and same_bits(o["tau_joint"][flight], o["tau_full"][flight, 6:]) and same_bits(o["base_residual"][flight], o["tau_full"][flight, 0:6])


def test_output_selection_and_a_misaligned_table(api, tables):
    """Every single output alone, all but it, all together: the same bits where the same is asked.  A table 4 bytes off a 16-byte boundary is
    refused before any launch."""
    n, K = 2 * G + 3, 2
    root, dof, ms, arm, acc = DR.seeded(n, 10)
    fr, st = IR.fref_of(n, 12, 12), SR.stance_cycle(n, K, 1)
    full = run(api, tables, K, root, dof, ms, arm, 0, st, acc, fr, W10)
    for k in OUTS:
        one = run(api, tables, K, root, dof, ms, arm, 0, st, acc, fr, W10, outs=(k,))
        assert same_bits(one[k], full[k]) and all(one[j] is None for j in OUTS if j != k), k
        rest = run(api, tables, K, root, dof, ms, arm, 0, st, acc, fr, W10, outs=tuple(j for j in OUTS if j != k))
        assert rest[k] is None and all(same_bits(rest[j], full[j]) for j in OUTS if j != k), k
    longer = torch.zeros(SM.TABLE_WORDS + 4, dtype=torch.int32, device=DEV)
    longer[1:1 + SM.TABLE_WORDS].copy_(tables[K, W10])
    assert longer.data_ptr() % 16 == 0
    off = run(api, tables, K, root, dof, ms, arm, 0, st, acc, fr, W10, expect=-1, table=longer.data_ptr() + 4)
    assert all(off[k] is None for k in OUTS) and b"16-byte aligned" in api["last_error"]()
    assert run(api, tables, K, root, dof, ms, arm, 0, st, acc, fr, W10, outs=(), expect=-1)["force"] is None and b"no output" in api["last_error"]()


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_exact_properties(api, iapi, tables, vel_at_com):
    n, v = 2 * G + 3, vel_at_com
    root, dof, ms, arm, acc = DR.seeded(n, 8)
    for K in (2, 4):
        cs, m = SR.SETS[K], 6 * K
        fr = IR.fref_of(n, m, 9)
        # an all-ones, NULL or 255 stance: dwi_solve's bits in all four outputs
        inv = irun(iapi, K, cs, root, dof, ms, arm, v, acc, fr, W10)
        for st in (None, np.ones((n, K), np.uint8), np.full((n, K), 255, np.uint8)):
            o = run(api, tables, K, root, dof, ms, arm, v, st, acc, fr, W10)
            assert all(same_bits(o[k], inv[k]) for k in IOUTS)
        # a byte of 255 equals 1 in a mixed stance too
        st = SR.stance_cycle(n, K, 2)
        o = run(api, tables, K, root, dof, ms, arm, v, st, acc, fr, W10)
        o255 = run(api, tables, K, root, dof, ms, arm, v, st * 255, acc, fr, W10)
        assert all(same_bits(o[k], o255[k]) for k in OUTS)
        # one active contact i with unit weights: dwi_solve's bits on the one-contact table of contact i; the other rows' f_ref (NaN) is not read
        for i in range(K):
            st = np.zeros((n, K), np.uint8)
            st[:, i] = 1
            bad = np.full((n, m), np.nan, F)
            bad[:, 6 * i:6 * i + 6] = fr[:, 6 * i:6 * i + 6]
            for ref, sub in ((bad, np.ascontiguousarray(fr[:, 6 * i:6 * i + 6])), (None, None)):
                o1 = run(api, tables, K, root, dof, ms, arm, v, st, acc, ref)
                one = irun(iapi, 1, cs[i:i + 1], root, dof, ms, arm, v, acc, sub)
                assert same_bits(o1["force"][:, 6 * i:6 * i + 6], one["force"]) and same_bits(o1["tau_joint"], one["tau_joint"]), (K, i)
                assert (np.delete(o1["force"], np.s_[6 * i:6 * i + 6], 1).view(U) == 0).all() and (np.delete(o1["margins"], i, 1).view(U) == 0).all()
        # flight
        o0 = run(api, tables, K, root, dof, ms, arm, v, np.zeros((n, K), np.uint8), acc, np.full((n, m), np.nan, F), W10)
        assert (o0["force"].view(U) == 0).all() and (o0["margins"].view(U) == 0).all() and (o0["feasible"] == 0).all()
        assert same_bits(o0["tau_joint"], o0["tau_full"][:, 6:]) and same_bits(o0["base_residual"], o0["tau_full"][:, 0:6]) and same_bits(o0["tau_full"], inv["tau_full"])
        # 640 m out: the same bits
        far = root.copy()
        far[:, 0:2] += np.array([640.0, -640.0], F)
        st = SR.stance_cycle(n, K, 2)
        of = run(api, tables, K, far, dof, ms, arm, v, st, acc, fr, W10)
        assert all(same_bits(of[k], o[k]) for k in OUTS)
    # a NaN stays in its env
    K, fr, st = 2, IR.fref_of(n, 12, 9), SR.stance_cycle(n, 2)          # (env 2 stands on the right foot, G + 1 on the left, 7 on both)
    o = run(api, tables, K, root, dof, ms, arm, v, st, acc, fr, W10)
    bad_r, bad_d, bad_a = root.copy(), dof.copy(), acc.copy()
    bad_r[2, 4], bad_d[G + 1, 4, 0], bad_a[7, 7] = np.nan, np.inf, np.nan          # (DoF 4 drives moving body 5, on the left foot's path)
    on = run(api, tables, K, bad_r, bad_d, ms, arm, v, st, bad_a, fr, W10, finite=False)
    keep = [e for e in range(n) if e not in (2, G + 1, 7)]
    for k in OUTS:
        assert same_bits(on[k][keep], o[k][keep]), k
    assert all(np.isnan(on[k][e]).any() for k in ("tau_joint", "force", "tau_full") for e in (2, G + 1, 7)) and (on["feasible"][[2, G + 1, 7]] == 0).all()


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
        cfg["sim"]["mi355"]["stance_inverse_dynamics"] = spec
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


KEPT = (("tau_joint", "tau_joint"), ("force", "force_all"), ("contact_accel", "contact_accel"), ("tau_full", "tau_full"), ("base_residual", "base_residual"),
        ("margins", "margins"), ("feasible", "feasible"))


def test_live_env_with_resets(api, tables):
    """40 steps at 64 envs with resets, "auto" and stance_from_phase() every step: the tensors equal a fresh launch bit for bit; obs, rew, done,
    root_states and env_state are the same bits with the key absent."""
    n, steps = 64, 40
    acts = actions(n, steps)
    runs, seen = {}, set()
    every = {"weights": list(W10), "tau_full": True, "auto": True}
    for name, spec in (("off", None), ("auto", every)):
        env = make_env(n, spec)
        sd = env.stance_inverse_dynamics
        a, h, resets = torch.zeros(n, 13, device=DEV), [], 0
        if spec is None:
            assert sd is None
        else:
            assert sd.stance.dtype == torch.uint8 and sd.stance.shape == (n, 2) and bool((sd.stance == 1).all())
            # the env's mocap rows spread over the gait: every window is met
            from isaacgymdyros_amd import abi
            idx = abi.es_view(env._buf["env_state"], "mocap_data_idx")
            idx[:, 0] = (torch.arange(n, device=DEV, dtype=torch.int32) * 57) % 3600
        for i in range(steps):
            a.copy_(acts[i])
            if sd is not None:
                sd.stance_from_phase()          # (the stance the step's auto refresh solves under)
            o, r, d, _ex = env.step(a)
            h.append(bits(o["obs"], r, d, env._buf["root_states"], env._buf["env_state"]))
            resets += int(d.sum())
            if sd is not None and (i % 3 == 0 or i == steps - 1):
                held = {k: getattr(sd, attr).cpu().numpy().copy() for k, attr in KEPT}
                root, dof, ms, arm = buffers(env, n)
                st_h, acc_h, fr_h = sd.stance.cpu().numpy(), sd.accel.cpu().numpy(), sd.force_ref.cpu().numpy()
                seen |= {tuple(x) for x in st_h}
                fresh = run(api, tables, 2, root, dof, ms, arm, sd.vel_at_com, st_h, acc_h, fr_h, W10)
                assert all(same_bits(held[k], fresh[k]) for k in OUTS), i
                if i % 12 == 0:
                    want = SR.evaluate(root, dof, sd.vel_at_com, ms, arm, SR.SETS[2], st_h, acc_h, W10, fr_h)
                    assert SR.within(SR.excess(fresh, want, sd.vel_at_com, 2, W10, True)), i
                sd.accel.copy_(torch.from_numpy(DR.accel_of(n, i)).to(DEV))
                sd.force_ref.copy_(torch.from_numpy(IR.fref_of(n, 12, i)).to(DEV))
        if sd is not None:
            assert seen == {(1, 1), (1, 0), (0, 1)}          # (double support, left only, right only)
            # stance_from_phase is the windows of the record's index, and stance_from_load the contact forces' sign
            idx = abi.es_view(env._buf["env_state"], "mocap_data_idx")[:, 0].cpu().numpy()
            left, right = SM.phase_stance(idx)
            assert np.array_equal(sd.stance_from_phase().cpu().numpy(), np.stack([left, right], 1).astype(np.uint8))
            fz = env.contact_forces.view(n, 38, 3)[:, [8, 16], 2].cpu().numpy()
            assert np.array_equal(sd.stance_from_load(5.0).cpu().numpy(), (fz > 5.0).astype(np.uint8))
            # solve() copies what it is given; a stance of any non-zero value is 1
            tj = sd.solve(torch.zeros(n, 39, device=DEV), torch.zeros(n, 2, 6, device=DEV), torch.full((n, 2), 7, dtype=torch.uint8, device=DEV))
            assert tj is sd.tau_joint and bool((sd.stance == 1).all()) and sd.force.shape == (n, 2, 6) and sd.force.data_ptr() == sd.force_all.data_ptr()
            assert sd.margins.shape == (n, 2, 4) and sd.base_residual.shape == (n, 6) and sd.feasible.shape == (n,) and sd.feasible.dtype == torch.uint8
            assert sd.names == ["L_Foot_Link", "R_Foot_Link"] and sd.index("R_Foot_Link") == 1 and sd.friction == 1.0 and sd.soles == [[0.03, 0.0, -0.1585, 0.15, 0.085]] * 2
            # reset_idx refreshes too
            before = sd.tau_joint.clone()
            env.reset_idx(torch.arange(0, n, 2, device=DEV))
            held = sd.tau_joint.clone()
            sd.refresh()
            assert torch.equal(sd.tau_joint, held) and not torch.equal(held[0::2], before[0::2]) and torch.equal(held[1::2], before[1::2])
        runs[name] = torch.stack(h).cpu()
        env.close()
        assert resets > 0
    assert torch.equal(runs["off"], runs["auto"])


def test_captured_step_plus_stance_from_phase_and_refresh_replays_the_eager_bits():
    """Step, stance_from_phase() and refresh() recorded in one graph on one stream (a linear chain), replayed 10 times, against 10 eager steps
    from the same state."""
    n = 64
    acts = actions(n, 11, seed=3)
    outs = []
    for captured in (False, True):
        env = make_env(n, {"tau_full": True, "weights": list(W10)})
        sd = env.stance_inverse_dynamics
        from isaacgymdyros_amd import abi
        abi.es_view(env._buf["env_state"], "mocap_data_idx")[:, 0] = (torch.arange(n, device=DEV, dtype=torch.int32) * 57) % 3600
        a = torch.zeros(n, 13, device=DEV)
        a.copy_(acts[0])
        env.step(a)                            # (the first step is eager on both sides)
        sd.stance_from_phase()
        sd.refresh()
        torch.cuda.synchronize()
        h = []
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            gr = torch.cuda.CUDAGraph()
            a.copy_(acts[1])
            with torch.cuda.graph(gr, stream=side):
                env.step(a)
                sd.stance_from_phase()
                sd.refresh()
        for i in range(1, 11):
            a.copy_(acts[i])
            if captured:
                gr.replay()
            else:
                env.step(a)
                sd.stance_from_phase()
                sd.refresh()
            h.append(bits(sd.stance, sd.tau_joint, sd.force, sd.contact_accel, sd.tau_full, sd.base_residual, sd.margins, sd.feasible, env._buf["root_states"]))
        torch.cuda.synchronize()
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1])


def test_tocabi_amp_lower():
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    n = 32
    cfg = default_amp_cfg(n, DEV)
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert amp.stance_inverse_dynamics is None
    amp.close()
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"].setdefault("mi355", {})["amp_stance_inverse_dynamics"] = {"auto": True}
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    sd = amp.stance_inverse_dynamics
    assert isinstance(sd, SM.StanceInverseDynamics) and amp._phys.stance_inverse_dynamics is None and sd.vel_at_com == int(amp._phys._ccfg.root_vel_at_com)
    with pytest.raises(ValueError, match="DyrosDynamicWalk only"):
        sd.stance_from_phase()
    st = SR.stance_cycle(n, 2, 1)
    sd.stance.copy_(torch.from_numpy(st).to(DEV))
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(20):
        amp.step((torch.rand(n, amp.num_actions, generator=g, device=DEV) * 2 - 1) * 0.1)
    root, dof, ms, arm = buffers(amp._phys, n)
    got = {k: getattr(sd, a).cpu().numpy() for k, a in KEPT if a != "tau_full"}          # (the last step's auto refresh)
    want = SR.evaluate(root, dof, sd.vel_at_com, ms, arm, SR.SETS[2], st)
    ex = SR.excess(got, want, sd.vel_at_com, 2, report="TocabiAMPLower")
    amp.close()
    assert len(ex) == len(SR.CHANNELS) and SR.within(ex), ex
    check_feasible(got["feasible"], want, SR.allowance(want, sd.vel_at_com, 2, "margins"))


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_stance_arrays(tmp_path):
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
    for name, flag in (("plain", []), ("stance", ["--dynamics-stance"])):
        out = tmp_path / name
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64",
                            "--games", "64", "--max-steps", "60", "--episode-length", "0.1", "--dynamics-dir", str(out), "--dynamics-envs", "2"] + flag,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["dynamics_env0.npz", "dynamics_env1.npz"]
        files[name] = np.load(out / "dynamics_env1.npz")
    plain, z = files["plain"], files["stance"]
    old = ["names", "dof_names", "dt", "jacobian", "mass_matrix", "com_jacobian"]
    new = ["stance", "stance_torque", "stance_force", "stance_margins"]
    assert sorted(plain.files) == sorted(old) and sorted(z.files) == sorted(old + new)
    assert all(np.array_equal(plain[k], z[k]) for k in old)          # (the same seed: the files are what they were, plus the new arrays)
    T = z["jacobian"].shape[0]
    assert 20 <= T <= 60 and z["stance"].shape == (T, 2) and z["stance_torque"].shape == (T, 33) and z["stance_force"].shape == (T, 2, 6) and z["stance_margins"].shape == (T, 2, 4)
    assert all(np.isfinite(z[k]).all() for k in new) and set(np.unique(z["stance"])) <= {0, 1} and (z["stance"].sum(1) >= 1).all()
    # an unloaded foot carries nothing
    offm = z["stance"] == 0
    assert (z["stance_force"][offm] == 0).all() and (z["stance_margins"][offm] == 0).all()
