"""The contact inverse dynamics on an MI355X (include/dyros_contact_inverse_dynamics.h, csrc/dw_contact_inverse.hip): the
HIP kernel against the float64 reference of tests/contact_inverse_dynamics_ref.py under its measured tolerance at the workgroup's edges, for
one, two and four contacts, with the output buffers filled with NaN, too long, and their tails watched; a misaligned table; the ways to choose
outputs; the outputs' exact properties; tau_joint against dwc_solve's jc; the round trip through the contact-consistent forward dynamics; a
live env with resets; a captured step plus refresh() and solve(); TocabiAMPLower; the player's files."""
import numpy as np
import pytest
import torch

import contact_dynamics_ref as CR
import contact_inverse_dynamics_ref as IR
import dynamics_ref as DR
from isaacgymdyros_amd import contact_dynamics as CM
from isaacgymdyros_amd import contact_inverse_dynamics as IM
from isaacgymdyros_amd import dynamics as DM
from isaacgymdyros_amd.model import load_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = IM.GROUP          # envs per workgroup
PAD = 64
F, U = np.float32, np.uint32
OUTS = IR.OUTS
GRAV = DR.GRAVITY
W10 = IR.MOMENTS_10


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return __import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0]


@pytest.fixture(scope="module")
def api():
    return IM.declare(lib())


@pytest.fixture(scope="module")
def tables(api):
    """(K or "base", unit or moments weighted 10 x) -> the device table."""
    model, out = load_model(), {}
    for key, cs in list(IR.SETS.items()) + [("base", IR.BASE)]:
        for w in (None, W10):
            t = IM.pack_table(api, model, CR.ids_of(cs), [p for _, p in cs], None if w is None else np.tile(np.asarray(w, F), len(cs)))
            out[key, w] = torch.from_numpy(t.view(np.int32)).to(DEV)
    return out


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t, offset=0):
    return None if t is None else t.data_ptr() + 4 * offset


def run(api, tables, K, root, dof, ms, arm, vel_at_com, accel=None, f_ref=None, weights=None, outs=OUTS, finite=True, expect=0, table=None):
    """One launch into NaN-filled buffers PAD words too long; returns the outputs named as a dict (the others None): every word written (when
    the inputs were finite), none outside.  table: a pointer in place of the packed table's."""
    n, m = len(root), 6 * (1 if K == "base" else K)
    shape = {"tau_joint": (n, 33), "force": (n, m), "contact_accel": (n, m), "tau_full": (n, 39)}
    words = {k: int(np.prod(s)) for k, s in shape.items()}
    d = [dev(root), dev(dof), dev(ms), dev(arm), dev(accel), dev(f_ref)]
    buf = {k: torch.full((words[k] + PAD,), float("nan"), device=DEV) if k in outs else None for k in OUTS}
    rc = api["solve"](n, tables[K, weights].data_ptr() if table is None else table, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), *GRAV, ptr(d[4]), ptr(d[5]),
                      vel_at_com, *[ptr(buf[k]) for k in OUTS], stream())
    torch.cuda.synchronize()          # (d is freed after this)
    assert rc == expect, api["last_error"]()
    out = {}
    for k in OUTS:
        if buf[k] is None:
            out[k] = None
            continue
        h, w = buf[k].cpu().numpy(), words[k]
        if rc != 0:
            assert np.isnan(h).all()          # nothing was launched
            out[k] = None
            continue
        assert np.isnan(h[w:]).all(), "a word outside %s was written" % k
        if finite:
            assert np.isfinite(h[:w]).all(), "%d words of %s were not written" % (int(np.isnan(h[:w]).sum()), k)
        out[k] = h[:w].reshape(shape[k]).copy()
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(U), np.ascontiguousarray(b).view(U))


def same_but_zero_signs(a, b):
    return bool(np.isfinite(a).all() and np.isfinite(b).all() and np.array_equal(a, b))


# ---------------------------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 14])
def test_kernel_against_float64(api, tables, n, K, vel_at_com):
    """A group holds four envs.  n = 1: a lone env; 4: a full group; 5: a group plus one; 2, 3, 14: ragged tails.  Unit weights without f_ref
    and moments weighted 10 x with it: every channel within 4 d (force and tau_joint: d scaled with the solution)."""
    root, dof, ms, arm, acc = DR.seeded(n, 100 * n + 10 * K + vel_at_com)
    for w, fr in ((None, None), (W10, IR.fref_of(n, 6 * K, n + K))):
        o = run(api, tables, K, root, dof, ms, arm, vel_at_com, acc, fr, w)
        want = IR.evaluate(root, dof, vel_at_com, ms, arm, IR.SETS[K], acc, w, fr)
        ex = IR.excess(o, want, vel_at_com, K, w, fr is not None, report="gpu n=%d K=%d vel_at_com=%d weights %s" % (n, K, vel_at_com, "unit" if w is None else "10 x"))
        assert len(ex) == len(IR.CHANNELS) and IR.within(ex), ex


def test_output_selection_and_a_misaligned_table(api, tables):
    """Every single output alone, all but it, all together: the same bits where the same is asked.  A table 4 bytes off a 16-byte boundary is
    refused before any launch."""
    n, K = 2 * G + 3, 2
    root, dof, ms, arm, acc = DR.seeded(n, 10)
    fr = IR.fref_of(n, 12, 12)
    full = run(api, tables, K, root, dof, ms, arm, 0, acc, fr, W10)
    for k in OUTS:
        one = run(api, tables, K, root, dof, ms, arm, 0, acc, fr, W10, outs=(k,))
        assert same_bits(one[k], full[k]) and all(one[j] is None for j in OUTS if j != k), k
        rest = run(api, tables, K, root, dof, ms, arm, 0, acc, fr, W10, outs=tuple(j for j in OUTS if j != k))
        assert rest[k] is None and all(same_bits(rest[j], full[j]) for j in OUTS if j != k), k
    # nominal masses and no armature
    nom = run(api, tables, K, root, dof, None, None, 1, acc, fr, W10)
    ex = IR.excess(nom, IR.evaluate(root, dof, 1, None, None, IR.SETS[K], acc, W10, fr), 1, K, W10, True, report="gpu, nominal masses, no armature")
    assert len(ex) == len(IR.CHANNELS) and IR.within(ex), ex
    longer = torch.zeros(IM.TABLE_WORDS + 4, dtype=torch.int32, device=DEV)
    longer[1:1 + IM.TABLE_WORDS].copy_(tables[K, W10])
    assert longer.data_ptr() % 16 == 0
    off = run(api, tables, K, root, dof, ms, arm, 0, acc, fr, W10, expect=-1, table=longer.data_ptr() + 4)
    assert all(off[k] is None for k in OUTS) and b"16-byte aligned" in api["last_error"]()
    assert run(api, tables, K, root, dof, ms, arm, 0, acc, fr, W10, outs=(), expect=-1)["force"] is None and b"no output" in api["last_error"]()


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_exact_properties(api, tables, vel_at_com):
    n, v = 2 * G + 3, vel_at_com
    root, dof, ms, arm, acc = DR.seeded(n, 8)
    d = [dev(root), dev(dof), dev(ms), dev(arm), dev(acc)]
    napi = DM.declare(lib())
    ntable = torch.from_numpy(DM.pack_table(napi, load_model()).view(np.int32)).to(DEV)
    tau = torch.full((n, 39), float("nan"), device=DEV)
    assert napi["inverse_dynamics"](n, ntable.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), *GRAV, ptr(d[4]), v, None, None, tau.data_ptr(), None, stream()) == 0
    torch.cuda.synchronize()
    tau = tau.cpu().numpy()
    zeros39 = np.zeros((n, 39), F)
    # one contact on base_link at its origin: with origin velocities G is the identity, force and tau_joint are dwn_inverse_dynamics's tau
    b = run(api, tables, "base", root, dof, ms, arm, v, acc)
    assert same_bits(b["tau_full"], tau)
    if not v:
        assert same_but_zero_signs(b["force"], tau[:, 0:6]) and same_but_zero_signs(b["tau_joint"], tau[:, 6:])
    for K in (1, 2, 4):
        m = 6 * K
        fr = IR.fref_of(n, m, 9)
        o = run(api, tables, K, root, dof, ms, arm, v, acc, fr, W10)
        assert same_bits(o["tau_full"], tau)
        # accel NULL equals zeros, f_ref NULL equals zeros
        on, oz = run(api, tables, K, root, dof, ms, arm, v, None, fr, W10), run(api, tables, K, root, dof, ms, arm, v, zeros39, fr, W10)
        assert all(same_but_zero_signs(on[k], oz[k]) for k in OUTS) and not same_bits(on["force"], o["force"])
        fn, fz = run(api, tables, K, root, dof, ms, arm, v, acc, None, W10), run(api, tables, K, root, dof, ms, arm, v, acc, np.zeros((n, m), F), W10)
        assert all(same_bits(fn[k], fz[k]) for k in OUTS)
        # one contact: the same bits for any weights
        plain = run(api, tables, K, root, dof, ms, arm, v, acc)
        assert all(same_bits(plain[k], fn[k]) for k in OUTS) == (K == 1)
        # 640 m out: the same bits
        far = root.copy()
        far[:, 0:2] += np.array([640.0, -640.0], F)
        of = run(api, tables, K, far, dof, ms, arm, v, acc, fr, W10)
        assert all(same_bits(of[k], o[k]) for k in OUTS)
    # a NaN stays in its env
    fr = IR.fref_of(n, 12, 9)
    o = run(api, tables, 2, root, dof, ms, arm, v, acc, fr, W10)
    bad_r, bad_d, bad_a = root.copy(), dof.copy(), acc.copy()
    bad_r[2, 4], bad_d[G + 1, 4, 0], bad_a[7, 7] = np.nan, np.inf, np.nan          # (DoF 4 drives moving body 5, on the left foot's path)
    on = run(api, tables, 2, bad_r, bad_d, ms, arm, v, bad_a, fr, W10, finite=False)
    keep = [e for e in range(n) if e not in (2, G + 1, 7)]
    for k in OUTS:
        assert same_bits(on[k][keep], o[k][keep]), k
        assert np.isnan(on[k][2]).any() and np.isnan(on[k][G + 1]).any(), k
    assert all(np.isnan(on[k][7]).any() for k in ("tau_joint", "force", "tau_full"))


@pytest.mark.parametrize("K", [2, 4])
def test_tau_joint_against_the_contact_jacobian_of_section_26(api, tables, K):
    """tau_joint = tau_full[6:] - jc[:, :, 6:]' force, recomputed in float64 from dwc_solve's jc and this launch's force and tau_full, within
    tau_joint's allowance; and jc's base columns carry the base rows: jc[:, :, 0:6]' force = tau_full[0:6] within what the force's allowance
    becomes through the columns."""
    n, v = 2 * G + 3, 1
    root, dof, ms, arm, acc = DR.seeded(n, 30 + K)
    fr = IR.fref_of(n, 6 * K, 31)
    o = run(api, tables, K, root, dof, ms, arm, v, acc, fr, W10)
    capi, cs = CM.declare(lib()), IR.SETS[K]
    ctable = torch.from_numpy(CM.pack_table(capi, load_model(), CR.ids_of(cs), [p for _, p in cs]).view(np.int32)).to(DEV)
    d = [dev(root), dev(dof)]
    jc = torch.full((n, 6 * K, 39), float("nan"), device=DEV)
    assert capi["solve"](n, ctable.data_ptr(), ptr(d[0]), ptr(d[1]), None, None, v, None, 0, None, None, jc.data_ptr(), *([None] * 6), stream()) == 0
    torch.cuda.synchronize()
    jc = jc.cpu().numpy().astype(np.float64)
    f, r = o["force"].astype(np.float64), o["tau_full"].astype(np.float64)
    want = IR.evaluate(root, dof, v, ms, arm, cs, acc, W10, fr)
    res = np.abs(r[:, 6:] - np.einsum("nrj,nr->nj", jc[:, :, 6:], f) - o["tau_joint"].astype(np.float64))
    assert (res <= IR.allowance(want, v, K, "tau_joint", W10, True)).all()
    res = np.abs(np.einsum("nrk,nr->nk", jc[:, :, 0:6], f) - r[:, 0:6])
    dn = DR.measured(v)
    allow = (np.einsum("nrk,nr->nk", np.abs(jc[:, :, 0:6]), IR.allowance(want, v, K, "force", W10, True)) + IR.FACTOR * np.array([dn["tau_lin"]] * 3 + [dn["tau_ang"]] * 3))
    assert (res <= allow).all()


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
        cfg["sim"]["mi355"]["contact_inverse_dynamics"] = spec
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


def test_round_trip_through_the_contact_consistent_forward_dynamics():
    """On a stepped env: contact_dynamics.forward_dynamics(tau_joint, contact_accel=contact_accel) returns the accel that was asked for and
    the force that was found, within the sum of the two features' allowances, formed in float64: section 26's 4 d of accel and of force at its
    own float64 solution of what it was fed, and what this feature's 4 d of tau_joint and of contact_accel and dwn's 4 d of the bias forces
    become through |KKT^-1|; for the force also this feature's own 4 d of force."""
    n = 64
    env = make_env(n, {"weights": list(W10)}, contact_dynamics={"jacobian": False, "lambda": False})
    ci, cd = env.contact_inverse_dynamics, env.contact_dynamics
    a = torch.zeros(n, 13, device=DEV)
    acts = actions(n, 6, seed=5)
    for i in range(6):
        a.copy_(acts[i])
        env.step(a)
    acc = DR.accel_of(n, 6)
    fr = IR.fref_of(n, 12, 7)
    tj = ci.solve(torch.from_numpy(acc).to(DEV), torch.from_numpy(fr).to(DEV).view(n, 2, 6))
    assert tj is ci.tau_joint and tj.shape == (n, 33) and ci.force.shape == (n, 2, 6) and ci.contact_accel.shape == (n, 12) and ci.tau_full is None
    back = cd.forward_dynamics(tau_joint=tj, contact_accel=ci.contact_accel).cpu().numpy().astype(np.float64)
    fback = cd.force.reshape(n, 12).cpu().numpy().astype(np.float64)
    root, dof, ms, arm = buffers(env, n)
    v = ci.vel_at_com
    assert v == cd.vel_at_com
    tj_h, ca_h, f_h = tj.cpu().numpy(), ci.contact_accel.cpu().numpy(), ci.force_all.cpu().numpy()
    want_i = IR.evaluate(root, dof, v, ms, arm, IR.SETS[2], acc, W10, fr)
    ex = IR.excess({"tau_joint": tj_h, "force": f_h, "contact_accel": ca_h}, want_i, v, 2, W10, True, report="the env's solve")
    assert len(ex) == len(IR.CHANNELS) and IR.within(ex), ex
    rhs = np.concatenate([np.zeros((n, 6), F), tj_h], 1)[:, None]
    want_c = CR.evaluate(root, dof, v, ms, arm, CR.SETS[2], rhs, cd._bias.bias.cpu().numpy(), ca_h)
    dn = DR.measured(v)
    db = IR.FACTOR * np.array([dn["bias_lin"]] * 3 + [dn["bias_ang"]] * 3 + [dn["bias_joint"]] * 33)
    side = np.concatenate([db + np.concatenate([np.zeros((n, 6)), IR.allowance(want_i, v, 2, "tau_joint", W10, True)], 1),
                           IR.allowance(want_i, v, 2, "contact_accel", W10, True)], 1)
    through = np.einsum("nab,nb->na", np.abs(np.linalg.inv(want_c["KKT"])), side)
    ea = np.abs(back - acc.astype(np.float64)) / (CR.allowance(want_c, v, 2, "accel")[:, 0] + through[:, :39])
    ef = np.abs(fback - f_h.astype(np.float64)) / (CR.allowance(want_c, v, 2, "force")[:, 0] + through[:, 39:] + IR.allowance(want_i, v, 2, "force", W10, True))
    print("round trip: accel %.3f and force %.3f of the allowances (|accel| up to %.0f, |force| up to %.0f)" % (ea.max(), ef.max(), np.abs(acc).max(), np.abs(f_h).max()))
    env.close()
    assert ea.max() <= 1.0 and ef.max() <= 1.0


def test_live_env_with_resets(api, tables):
    n, steps = 64, 40
    acts = actions(n, steps)
    runs = {}
    every = {"weights": list(W10), "contact_accel": True, "tau_full": True, "auto": True}
    kept = ("tau_joint", "force_all", "contact_accel", "tau_full")
    names = {"tau_joint": "tau_joint", "force_all": "force", "contact_accel": "contact_accel", "tau_full": "tau_full"}
    for name, spec, mi in (("off", None, {}), ("auto", every, {}), ("beside", {"auto": True, "armature": False, "contacts": [{"body": "L_Foot_Link", "pos": [0, 0, -0.09]}]},
                                                                     {"episode_stats": True})):
        env = make_env(n, spec, **mi)
        a, h, resets = torch.zeros(n, 13, device=DEV), [], 0
        if spec is None:
            assert env.contact_inverse_dynamics is None
        for i in range(steps):
            a.copy_(acts[i])
            o, r, d, _ex = env.step(a)
            h.append(bits(o["obs"], r, d, env._buf["root_states"], env._buf["env_state"]))
            resets += int(d.sum())
            if name == "auto" and (i % 3 == 0 or i == steps - 1):
                ci = env.contact_inverse_dynamics
                held = {names[k]: getattr(ci, k).cpu().numpy().copy() for k in kept}          # (what the step's auto refresh left: accel and force_ref as they stood)
                root, dof, ms, arm = buffers(env, n)
                acc_h, fr_h = ci.accel.cpu().numpy(), ci.force_ref.cpu().numpy()
                fresh = run(api, tables, 2, root, dof, ms, arm, ci.vel_at_com, acc_h, fr_h, W10)
                assert all(same_bits(held[k], fresh[k]) for k in OUTS), i
                if i % 12 == 0 or i == steps - 1:
                    want = IR.evaluate(root, dof, ci.vel_at_com, ms, arm, IR.SETS[2], acc_h, W10, fr_h)
                    ex = IR.excess(fresh, want, ci.vel_at_com, 2, W10, True)
                    assert IR.within(ex), (i, ex)
                # the next steps' refreshes solve for another acceleration and prior
                ci.accel.copy_(torch.from_numpy(DR.accel_of(n, i)).to(DEV))
                ci.force_ref.copy_(torch.from_numpy(IR.fref_of(n, 12, i)).to(DEV))
        if name == "auto":
            assert ci.vel_at_com == 1 and ci.names == ["L_Foot_Link", "R_Foot_Link"] and ci.index("R_Foot_Link") == 1 and ci.rows == 12
            assert ci.accel.shape == ci.tau_full.shape == (n, 39) and ci.force_ref.shape == ci.force_all.shape == ci.contact_accel.shape == (n, 12)
            assert ci.force.shape == (n, 2, 6) and ci.force.data_ptr() == ci.force_all.data_ptr() and ci.weights == list(W10) * 2
            with pytest.raises(ValueError):
                ci.index("Head_Link")
            # reset_idx refreshes too: the tensors are those of the buffers after it
            ci.refresh()          # (accel and force_ref changed after the last step's refresh)
            before = ci.tau_joint.clone()
            env.reset_idx(torch.arange(0, n, 2, device=DEV))
            held = ci.tau_joint.clone()
            ci.refresh()
            assert torch.equal(ci.tau_joint, held) and not torch.equal(held[0::2], before[0::2]) and torch.equal(held[1::2], before[1::2])
        if name == "beside":
            ci = env.contact_inverse_dynamics
            assert ci.tau_full is None and ci.force.shape == (n, 1, 6) and ci.weights is None
            root, dof, ms, arm = buffers(env, n)
            fresh = run(api, tables, 1, root, dof, ms, None, ci.vel_at_com, np.zeros((n, 39), F), np.zeros((n, 6), F), outs=("tau_joint", "force", "contact_accel"))
            assert (same_bits(ci.tau_joint.cpu().numpy(), fresh["tau_joint"]) and same_bits(ci.force_all.cpu().numpy(), fresh["force"])
                    and same_bits(ci.contact_accel.cpu().numpy(), fresh["contact_accel"]))
        runs[name] = torch.stack(h).cpu()
        env.close()
        assert resets > 0          # (the time limit alone resets every env)
    # the feature only reads: the same bits with the key absent, on, and on beside another recorder in a rebuilt env
    assert torch.equal(runs["off"], runs["auto"]) and torch.equal(runs["off"], runs["beside"])


def test_captured_step_plus_every_call_replays_the_eager_bits():
    """Step, refresh() (auto) and solve() recorded in one graph on one stream (a linear chain), replayed 10 times, against 10 eager steps from
    the same state."""
    n = 64
    acts = actions(n, 11, seed=3)
    g = torch.Generator(device=DEV).manual_seed(4)
    accs = torch.randn(11, n, 39, generator=g, device=DEV) * 20
    frefs = torch.randn(11, n, 12, generator=g, device=DEV) * 100
    outs = []
    for captured in (False, True):
        env = make_env(n, {"tau_full": True, "auto": True, "weights": list(W10)})
        ci = env.contact_inverse_dynamics
        a = torch.zeros(n, 13, device=DEV)
        a.copy_(acts[0])
        env.step(a)                            # (the first step is eager on both sides)
        ci.solve(accs[0], frefs[0])
        torch.cuda.synchronize()
        h = []
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            gr = torch.cuda.CUDAGraph()
            a.copy_(acts[1])
            with torch.cuda.graph(gr, stream=side):
                env.step(a)
                ci.solve()
            # (the capture itself ran nothing: replay the recorded step for each of the 10 actions)
        for i in range(1, 11):
            a.copy_(acts[i])
            ci.accel.copy_(accs[i])
            ci.force_ref.copy_(frefs[i])
            if captured:
                gr.replay()
            else:
                env.step(a)
                ci.solve()
            h.append(bits(ci.tau_joint, ci.force, ci.contact_accel, ci.tau_full, env._buf["root_states"]))
        torch.cuda.synchronize()
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1])


def test_tocabi_amp_lower():
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    n = 32
    cfg = default_amp_cfg(n, DEV)
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert amp.contact_inverse_dynamics is None
    amp.close()
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"].setdefault("mi355", {})["amp_contact_inverse_dynamics"] = {"tau_full": True, "auto": True}
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert isinstance(amp.contact_inverse_dynamics, IM.ContactInverseDynamics) and amp._phys.contact_inverse_dynamics is None
    ci = amp.contact_inverse_dynamics
    assert ci.vel_at_com == int(amp._phys._ccfg.root_vel_at_com)
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(20):
        amp.step((torch.rand(n, amp.num_actions, generator=g, device=DEV) * 2 - 1) * 0.1)
    root, dof, ms, arm = buffers(amp._phys, n)
    got = {k: getattr(ci, a).cpu().numpy() for k, a in (("tau_joint", "tau_joint"), ("force", "force_all"), ("contact_accel", "contact_accel"))}          # (the last step's auto refresh)
    tau_full = ci.tau_full.cpu().numpy()
    want = IR.evaluate(root, dof, ci.vel_at_com, ms, arm, IR.SETS[2])
    ex = IR.excess(got, want, ci.vel_at_com, 2, report="TocabiAMPLower")
    amp.close()
    assert len(ex) == len(IR.CHANNELS) and IR.within(ex), ex
    assert DR.within(DR.excess({"tau": tau_full}, root, dof, ms, arm, np.zeros((n, 39), F), ci.vel_at_com))


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_holding_torques(tmp_path):
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
    for name, flag in (("plain", []), ("inverse", ["--dynamics-inverse", "--dynamics-forces"])):
        out = tmp_path / name
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64",
                            "--games", "64", "--max-steps", "60", "--episode-length", "0.1", "--dynamics-dir", str(out), "--dynamics-envs", "2"] + flag,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["dynamics_env0.npz", "dynamics_env1.npz"]
        files[name] = np.load(out / "dynamics_env1.npz")
    plain, z = files["plain"], files["inverse"]
    old = ["names", "dof_names", "dt", "jacobian", "mass_matrix", "com_jacobian"]
    new = ["hold_torque", "hold_force"]
    assert sorted(plain.files) == sorted(old) and sorted(z.files) == sorted(old + ["bias", "gravity", "momentum"] + new)
    assert all(np.array_equal(plain[k], z[k]) for k in old)          # (the same seed: the files are what they were, plus the new arrays)
    T = z["jacobian"].shape[0]
    assert 20 <= T <= 60 and z["hold_torque"].shape == (T, 33) and z["hold_force"].shape == (T, 2, 6) and all(np.isfinite(z[k]).all() for k in new)
    # holding nu_dot = 0 means carrying the bias forces: the feet's Jacobians of the same file (rows 1, 2; origin-to-sole arm r = R [0, 0, -0.09]
    # enters the moment only) give J' f = bias on the base's linear rows, where the feet's forces simply add up: within the K = 2 allowance of
    # the forces' sum and 4 d of dwn's bias
    total = z["hold_force"][:, :, 0:3].astype(np.float64).sum(1)
    d, dn = IR.measured(1, 2), DR.measured(1)
    scale = np.maximum(1.0, np.abs(z["hold_force"]).reshape(T, -1).max(-1, keepdims=True) / d["force_scale"])
    allow = 2 * IR.FACTOR * d["force_f"] * scale + IR.FACTOR * dn["bias_lin"]
    err = np.abs(total - z["bias"][:, 0:3].astype(np.float64))
    print("the player's hold_force summed against bias[0:3]: %.2e, %.3f of the allowance" % (err.max(), (err / allow).max()))
    assert (err <= allow).all()
