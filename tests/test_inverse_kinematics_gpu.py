"""The inverse kinematics on an MI355X (include/dyros_inverse_kinematics.h, csrc/dw_inverse_kinematics.hip): the HIP
kernel against the float64 reference of tests/inverse_kinematics_ref.py under its measured tolerance at the workgroup's edges, for one, two
and four targets, a fixed and a free base, one step and to convergence, with the output buffers filled with NaN, too long, and their tails
watched; a misaligned table; the ways to choose outputs; the outputs' exact properties; a live env with resets; a captured step plus
solve(); TocabiAMPLower; the player's files."""
import numpy as np
import pytest
import torch

import body_states_ref as R
import contact_dynamics_ref as CR
import inverse_kinematics_ref as QR
from isaacgymdyros_amd import contact_dynamics as CM
from isaacgymdyros_amd import inverse_kinematics as QM
from isaacgymdyros_amd.model import load_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = QM.GROUP          # envs per workgroup
SIZES = [1, G - 1, G, G + 1, 3 * G + 2]
PAD = 64
F, U = np.float32, np.uint32
OUTS = QR.OUTS
TYPES = {"q": torch.float32, "root": torch.float32, "residual": torch.float32, "err": torch.float32, "iters": torch.int32, "converged": torch.uint8}
FILL = {torch.float32: float("nan"), torch.int32: -7, torch.uint8: 9}


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return __import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0]


@pytest.fixture(scope="module")
def api():
    return QM.declare(lib())


_tables = {}


def table_of(api, P):
    """The device table of a reference problem, packed once."""
    key = QR._key(P)
    if key not in _tables:
        cs = P["contacts"]
        prm = QM.params_struct({"iterations": P["iterations"], "damping": float(P["damping"]), "max_step": float(P["max_step"]), "tol_pos": float(P["tol_pos"]),
                                "tol_ang": float(P["tol_ang"]), "base": P["base"], "limits": P["limits"], "target_frame": "root" if P["rel_root"] else "world"})
        t = QM.pack_table(api, load_model(), CM.contacts_struct(CR.ids_of(cs), [p for _, p in cs]), None, P["rows"].astype(np.uint8), P["w"], P["dofs"].astype(np.uint8),
                          QR.LOWER, QR.UPPER, prm)
        _tables[key] = torch.from_numpy(t.view(np.int32)).to(DEV)
    return _tables[key]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def dof_of(q, other=False):
    """dof_state rows [n, 33, 2] with seeded rates, which the solve never reads; other: positions that are not q."""
    d = np.random.default_rng(9).uniform(-4, 4, (len(q), 33, 2)).astype(F)
    d[:, :, 0] = q[::-1] + F(0.1) if other else q
    return d


def run(api, P, root, q0, tgt, outs=OUTS, pass_q0=False, finite=True, expect=0, table=None):
    """One launch into filled buffers PAD words too long; returns the outputs named as a dict (the others None): every word written (when the
    inputs were good), none outside.  pass_q0: q0 as the q0 argument over rows that hold other positions; table: a pointer in place of the
    packed table's."""
    n, m = len(root), P["m"]
    shape = {"q": (n, 33), "root": (n, 7), "residual": (n, m), "err": (n, 2), "iters": (n,), "converged": (n,)}
    words = {k: int(np.prod(s)) for k, s in shape.items()}
    d = [dev(root), dev(dof_of(q0, pass_q0)), dev(q0) if pass_q0 else None, dev(tgt)]
    buf = {k: torch.full((words[k] + PAD,), FILL[TYPES[k]], dtype=TYPES[k], device=DEV) if k in outs else None for k in OUTS}
    rc = api["solve"](n, table_of(api, P).data_ptr() if table is None else table, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), *[ptr(buf[k]) for k in OUTS], stream())
    torch.cuda.synchronize()          # (d is freed after this)
    assert rc == expect, api["last_error"]()
    out = {}
    for k in OUTS:
        if buf[k] is None:
            out[k] = None
            continue
        h, w = buf[k].cpu().numpy(), words[k]
        untouched = (lambda x: np.isnan(x).all()) if TYPES[k] == torch.float32 else (lambda x, k=k: (x == FILL[TYPES[k]]).all())
        if rc != 0:
            assert untouched(h)          # nothing was launched
            out[k] = None
            continue
        assert untouched(h[w:]), "a word outside %s was written" % k
        if TYPES[k] != torch.float32:
            assert (h[:w] != FILL[TYPES[k]]).all(), "words of %s were not written" % k
        elif finite:
            assert np.isfinite(h[:w]).all(), "%d words of %s were not written" % (int(np.isnan(h[:w]).sum()), k)
        out[k] = h[:w].reshape(shape[k]).copy()
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---------------------------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize("base", [False, True])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_one_step_against_float64(api, K, base):
    """iterations = 1 at n = 1, G - 1, G, G + 1 and 3 G + 2 (a lone env, a ragged group, a full one, a group plus one, three and a tail): every
    channel within 4 d of the float64 lstsq step; unit weights with every row, orientation rows weighted 10 x under a row mask."""
    for w, rows in ((None, None), (QR.ORI_10, QR.MIXED[K])):
        P = QR.problem(K, rows=rows, weights=w, base=base, iterations=1)
        root, q0, tgt, _ = QR.case(SIZES[-1], 100 + 10 * K + base, P)
        want = QR.step(root, q0, tgt, P)
        for n in SIZES:
            o = run(api, P, root[:n], q0[:n], tgt[:n])
            assert (o["iters"] == 1).all() and (o["converged"] == 0).all()
            part = {k: v[:n] for k, v in want.items()}
            ex = QR.excess(o, part, root[:n], tgt[:n], P, report="gpu one step n=%d K=%d base=%d weights %s" % (n, K, base, "unit" if w is None else "10 x, masked"))
            assert len(ex) == len(QR.CHANNELS) and QR.within(ex), ex


@pytest.mark.parametrize("base", [False, True])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_convergence(api, K, base):
    """iterations = 8, reachable targets, the same sizes: the float64 reference converges on every case (checked first); the kernel reports
    converged on every case; its residual, recomputed in float64 from the returned q, is within 4 d of the reference's and within the tolerances
    plus that; with both feet on a fixed base q is within 4 d of the float64 solution."""
    P, root, q0, tgt, want = QR.conv_case(K, base)
    assert len(root) == SIZES[-1] and (want["converged"] == 1).all() and want["iters"].max() <= P["iterations"]
    d = QR.measured(P)
    keep = ("rq_pos", "rq_ang") + (("q",) if K == 2 and not base else ())
    for n in SIZES:
        o = run(api, P, root[:n], q0[:n], tgt[:n])
        assert (o["converged"] == 1).all() and (o["iters"] >= 2).all() and (o["iters"] <= P["iterations"]).all()
        assert (o["err"][:, 0] <= P["tol_pos"]).all() and (o["err"][:, 1] <= P["tol_ang"]).all()
        ex = QR.excess(o, {k: v[:n] for k, v in want.items()}, root[:n], tgt[:n], P, report="gpu convergence n=%d K=%d base=%d" % (n, K, base))
        ex = {k: v for k, v in ex.items() if k in keep}
        assert len(ex) == len(keep) and QR.within(ex), ex
        res = QR.residual64(o, root[:n], tgt[:n], P).reshape(n, K, 6)
        assert np.abs(res[..., 0:3]).max() <= P["tol_pos"] + QR.FACTOR * d["rq_pos"] and np.abs(res[..., 3:6]).max() <= P["tol_ang"] + QR.FACTOR * d["rq_ang"]


def test_output_selection_and_a_misaligned_table(api):
    """Every single output alone, all but it, all together: the same bits where the same is asked.  A table 4 bytes off a 16-byte boundary is
    refused before any launch, and so is a call without an output."""
    n = 2 * G + 3
    P = QR.problem(2, base=True, iterations=5)
    root, q0, tgt, _ = QR.case(n, 10, P)
    full = run(api, P, root, q0, tgt)
    for k in OUTS:
        one = run(api, P, root, q0, tgt, outs=(k,))
        assert same_bits(one[k], full[k]) and all(one[j] is None for j in OUTS if j != k), k
        rest = run(api, P, root, q0, tgt, outs=tuple(j for j in OUTS if j != k))
        assert rest[k] is None and all(same_bits(rest[j], full[j]) for j in OUTS if j != k), k
    longer = torch.zeros(QM.TABLE_WORDS + 4, dtype=torch.int32, device=DEV)
    longer[1:1 + QM.TABLE_WORDS].copy_(table_of(api, P))
    assert longer.data_ptr() % 16 == 0
    off = run(api, P, root, q0, tgt, expect=-1, table=longer.data_ptr() + 4)
    assert all(off[k] is None for k in OUTS) and b"16-byte aligned" in api["last_error"]()
    assert run(api, P, root, q0, tgt, outs=(), expect=-1)["q"] is None and b"no output" in api["last_error"]()


@pytest.mark.parametrize("base", [False, True])
def test_exact_properties(api, base):
    n = 2 * G + 3
    for K in (1, 2, 4):
        P = QR.problem(K, base=base, iterations=6)
        root, q0, tgt, _ = QR.case(n, 23, P)
        o = run(api, P, root, q0, tgt)
        # unmasked joints return q0's bits; a fixed base returns the root's bits
        assert same_bits(o["q"][:, ~P["dofs"]], q0[:, ~P["dofs"]]) and same_bits(o["root"], np.ascontiguousarray(root[:, 0:7])) == (not base)
        # a NULL q0 and a q0 that holds dof_state's positions: the same bits
        assert all(same_bits(run(api, P, root, q0, tgt, pass_q0=True)[k], o[k]) for k in OUTS)
        # targets made from the state: no update, q0's bits
        z = run(api, P, root, q0, QR.targets_of(root, q0, P))
        assert (z["iters"] == 0).all() and (z["converged"] == 1).all() and same_bits(z["q"], q0) and same_bits(z["root"], np.ascontiguousarray(root[:, 0:7]))
        # targets in the root's frame: an env moved 640 m gets the same bits
        Pr = dict(P, rel_root=True)
        rel = tgt.copy()
        rel[..., 0:3] -= root[:, None, 0:3]
        far = root.copy()
        far[:, 0:2] += np.array([640.0, -640.0], F)
        a, b = run(api, Pr, root, q0, rel), run(api, Pr, far, q0, rel)
        assert all(same_bits(a[k], b[k]) for k in OUTS if k != "root") and same_bits(a["root"][:, 2:7], b["root"][:, 2:7])
        # a position-only target leaves its orientation rows +0.0
        Pp = QR.problem(K, rows=("position",) * K, base=base, iterations=3)
        p = run(api, Pp, root, q0, tgt)
        assert (p["residual"].reshape(n, K, 6)[..., 3:6].view(U) == 0).all() and (p["err"][:, 1].view(U) == 0).all() and (p["err"][:, 0] > 0).all()
    # a target 3 m away: finite, inside the limits, within max_step an update, never converged
    P = QR.problem(2, base=base, iterations=12, max_step=0.25)
    root, q0, tgt, _ = QR.case(n, 37, P)
    tgt[:, 0, 0:3] += np.array([3.0, 0.0, 0.0], F)
    tgt[:, 1, 0:3] += np.array([0.0, -2.0, 2.0], F)
    o = run(api, P, root, q0, tgt)
    q = o["q"][:, P["dofs"]]
    assert (o["converged"] == 0).all() and (o["iters"] == 12).all() and (q >= QR.LOWER[P["dofs"]]).all() and (q <= QR.UPPER[P["dofs"]]).all()
    assert np.abs(o["q"] - q0).max() <= 12 * 0.25 * (1 + 1e-6) and same_bits(o["q"][:, ~P["dofs"]], q0[:, ~P["dofs"]])
    one = run(api, dict(P, iterations=1), root, q0, tgt)
    assert np.abs(one["q"] - q0).max() <= 0.25 * (1 + 1e-6) and (one["iters"] == 1).all()
    # a bad target spoils its env only
    P = QR.problem(2, base=base, iterations=5)
    root, q0, tgt, _ = QR.case(n, 41, P)
    o0 = run(api, P, root, q0, tgt)
    bad = tgt.copy()
    bad[1, 0, 1], bad[G, 1, 3:7], bad[G + 2, 0, 3:7] = np.nan, 0.0, bad[G + 2, 0, 3:7] * F(1.02)
    o = run(api, P, root, q0, bad, finite=False)
    dead = [1, G, G + 2]
    keep = [e for e in range(n) if e not in dead]
    for e in dead:
        assert all(np.isnan(o[k][e]).all() for k in ("q", "root", "residual", "err")) and o["iters"][e] == 0 and o["converged"][e] == 0
    assert all(same_bits(o[k][keep], o0[k][keep]) for k in OUTS)


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
        cfg["sim"]["mi355"]["inverse_kinematics"] = spec
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def actions(n, steps, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.tensor([0.0, 0.05, 0.3, 1.0], device=DEV)[torch.arange(n, device=DEV) % 4].view(1, n, 1)
    return ((torch.rand(steps, n, 13, generator=g, device=DEV) * 2 - 1) * amp).contiguous()


def bits(*ts):
    return torch.cat([t.contiguous().reshape(-1).view(torch.uint8) for t in ts])


def state_of(env, n):
    b = env._buf
    return b["root_states"].cpu().numpy().reshape(n, 13), b["dof_state"].cpu().numpy().reshape(n, 33, 2)


def held(ik):
    return {"q": ik.q.cpu().numpy(), "root": ik.root.cpu().numpy(), "residual": ik.residual.cpu().numpy(), "err": ik.err.cpu().numpy(),
            "iters": ik.iters.cpu().numpy(), "converged": ik.converged.cpu().numpy()}


def test_live_env_with_resets(api):
    """40 steps of 64 envs with "auto": True: what a step's refresh leaves are the bits of a launch through the C ABI for the buffers as they
    stand; targets_from_bodies() gives a problem with no update; solve(q0 = the initial angles) brings both feet to their played poses; and the
    run's observations are the same bits with the key on and off."""
    n, steps = 64, 40
    acts = actions(n, steps)
    runs = {}
    P = QR.problem(2, rel_root=True)          # (targets as offsets from the base: an env's place on the grid costs them nothing)
    for name, spec in (("off", None), ("auto", {"auto": True, "target_frame": "root"})):
        env = make_env(n, spec)
        a, h, resets = torch.zeros(n, 13, device=DEV), [], 0
        ik = env.inverse_kinematics
        if spec is None:
            assert ik is None
        else:
            assert ik.names == ["L_Foot_Link", "R_Foot_Link"] and ik.index("R_Foot_Link") == 1 and ik.rows == 12 and ik.dofs == list(range(12))
            assert ik.targets.shape == (n, 2, 7) and ik.q.shape == (n, 33) and ik.root.shape == (n, 7) and ik.residual.shape == (n, 12) and ik.err.shape == (n, 2)
            assert ik.iters.dtype == torch.int32 and ik.converged.dtype == torch.uint8 and ik.dof_mask.cpu().numpy().tolist() == [True] * 12 + [False] * 21
            with pytest.raises(ValueError):
                ik.index("Head_Link")
        for i in range(steps):
            a.copy_(acts[i])
            o, r, d, _ex = env.step(a)
            h.append(bits(o["obs"], r, d, env._buf["root_states"], env._buf["env_state"]))
            resets += int(d.sum())
            if ik is not None and i == 5:
                ik.targets_from_bodies()          # (the poses of step 5: the later steps' refreshes solve for them from where the robot then is)
                root5, dof5 = state_of(env, n)
                want_t = QR.targets_of(root5, dof5[:, :, 0], P)
                got_t = ik.targets.cpu().numpy()
                assert np.abs(got_t[..., 0:3] - want_t[..., 0:3]).max() <= QR.FACTOR * R.measured(0)["off"] + 2e-7 and np.abs(np.abs((got_t[..., 3:7] * want_t[..., 3:7]).sum(-1)) - 1).max() <= 1e-6
                ik.refresh()
                z = held(ik)
                assert (z["iters"] == 0).all() and (z["converged"] == 1).all() and same_bits(z["q"], np.ascontiguousarray(dof5[:, :, 0]))
            if ik is not None and i > 5 and (i % 6 == 0 or i == steps - 1):
                root, dof = state_of(env, n)
                tg = ik.targets.cpu().numpy()
                fresh = run(api, P, root, dof[:, :, 0], tg)
                now = held(ik)
                assert all(same_bits(now[k], fresh[k]) for k in OUTS), i
                if i == steps - 1:
                    want = QR.solve(root, dof[:, :, 0], tg, P)
                    ok = (want["converged"] == 1) & (fresh["converged"] == 1)
                    res = QR.residual64(fresh, root, tg, P)[ok]
                    assert ok.any() and np.abs(res).max() <= 1e-5 + QR.FACTOR * max(QR.measured(P)["rq_pos"], QR.measured(P)["rq_ang"])
        if ik is not None:
            # the played feet from the model's initial angles
            ik.targets_from_bodies()
            q = ik.solve(q0=env.initial_dof_pos)
            assert q is ik.q
            root, dof = state_of(env, n)
            fresh = run(api, P, root, env.initial_dof_pos.cpu().numpy().astype(F), ik.targets.cpu().numpy(), pass_q0=True)
            now = held(ik)
            assert all(same_bits(now[k], fresh[k]) for k in ("q", "residual", "err", "iters", "converged"))
            # reset_idx refreshes too
            ik.refresh()
            before = ik.q.clone()
            env.reset_idx(torch.arange(0, n, 2, device=DEV))
            kept = ik.q.clone()
            ik.refresh()
            assert torch.equal(ik.q, kept) and not torch.equal(kept[0::2], before[0::2]) and torch.equal(kept[1::2], before[1::2])
        runs[name] = torch.stack(h).cpu()
        env.close()
        assert resets > 0          # (the time limit alone resets every env)
    assert torch.equal(runs["off"], runs["auto"])


def test_captured_step_plus_solve_replays_the_eager_bits():
    """step() and solve() recorded in one graph on one stream, replayed 10 times, against 10 eager steps from the same state: q, and every
    other output, bit for bit."""
    n = 64
    acts = actions(n, 11, seed=3)
    outs = []
    for captured in (False, True):
        env = make_env(n, {"base": True, "iterations": 8, "auto": True})
        ik = env.inverse_kinematics
        a = torch.zeros(n, 13, device=DEV)
        a.copy_(acts[0])
        env.step(a)                            # (the first step is eager on both sides)
        ik.targets_from_bodies()
        ik.targets[..., 0:3] += 0.02
        ik.solve()
        torch.cuda.synchronize()
        h = []
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            gr = torch.cuda.CUDAGraph()
            a.copy_(acts[1])
            with torch.cuda.graph(gr, stream=side):
                env.step(a)
                ik.solve()
        for i in range(1, 11):
            a.copy_(acts[i])
            if captured:
                gr.replay()
            else:
                env.step(a)
                ik.solve()
            h.append(bits(ik.q, ik.root, ik.residual, ik.err, ik.iters, ik.converged, env._buf["root_states"]))
        torch.cuda.synchronize()
        assert int(ik.iters.max()) >= 1
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1])


def test_tocabi_amp_lower(api):
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    n = 32
    cfg = default_amp_cfg(n, DEV)
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert amp.inverse_kinematics is None
    amp.close()
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"].setdefault("mi355", {})["amp_inverse_kinematics"] = {"auto": True, "iterations": 4}
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert isinstance(amp.inverse_kinematics, QM.InverseKinematics) and amp._phys.inverse_kinematics is None
    ik = amp.inverse_kinematics
    g = torch.Generator(device=DEV).manual_seed(1)
    for i in range(20):
        amp.step((torch.rand(n, amp.num_actions, generator=g, device=DEV) * 2 - 1) * 0.1)
        if i == 9:
            ik.targets_from_bodies()
    P = QR.problem(2, iterations=4)
    root, dof = state_of(amp._phys, n)
    tg, now = ik.targets.cpu().numpy(), held(ik)          # (the last step's auto refresh: the feet of step 10 from the state of step 20)
    fresh = run(api, P, root, dof[:, :, 0], tg)
    want = QR.solve(root, dof[:, :, 0], tg, P)
    amp.close()
    assert all(same_bits(now[k], fresh[k]) for k in OUTS)
    ex = QR.excess(fresh, want, root, tg, P, report="TocabiAMPLower")
    assert len(ex) == len(QR.CHANNELS) and QR.within(ex), ex


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_solved_angles(tmp_path):
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
    for name, flag in (("plain", []), ("ik", ["--dynamics-ik"])):
        out = tmp_path / name
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64",
                            "--games", "64", "--max-steps", "60", "--episode-length", "0.1", "--dynamics-dir", str(out), "--dynamics-envs", "2"] + flag,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["dynamics_env0.npz", "dynamics_env1.npz"]
        files[name] = np.load(out / "dynamics_env1.npz")
    plain, z = files["plain"], files["ik"]
    old = ["names", "dof_names", "dt", "jacobian", "mass_matrix", "com_jacobian"]
    new = ["ik_q", "ik_err", "ik_converged"]
    assert sorted(plain.files) == sorted(old) and sorted(z.files) == sorted(old + new)
    assert all(np.array_equal(plain[k], z[k]) for k in old)          # (the same seed: the files are what they were, plus the new arrays)
    T = z["jacobian"].shape[0]
    assert 20 <= T <= 60 and z["ik_q"].shape == (T, 33) and z["ik_err"].shape == (T, 2) and z["ik_converged"].shape == (T,) and z["ik_converged"].dtype == np.uint8
    assert all(np.isfinite(z[k]).all() for k in new)
    # the arms and the waist are not on the feet's paths: they keep the model's initial angles; where the solve converged the feet are there
    from isaacgymdyros_amd.task_constants import INITIAL_DOF_POS
    assert np.array_equal(z["ik_q"][:, 12:], np.broadcast_to(np.asarray(INITIAL_DOF_POS, F)[12:], (T, 21)))
    ok = z["ik_converged"] == 1
    assert ok.any() and (z["ik_err"][ok] <= 1e-5).all()
