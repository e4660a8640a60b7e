"""The contact-consistent dynamics on an MI355X (include/dyros_contact_dynamics.h, csrc/dw_contact_dynamics.hip): the
HIP kernel against the float64 reference of tests/contact_dynamics_ref.py under its measured tolerance at the workgroup's edges, for one, two
and four contacts and one and eight right-hand sides, with the output buffers filled with NaN, too long, and their tails watched; the ways
to choose outputs; unaligned outputs; minv_jt against dwl_solve bit for bit; the outputs' exact properties; composition with the shipped
forward dynamics; a live env with resets; a captured step plus refresh() and forward_dynamics(); TocabiAMPLower; the player's files."""
import numpy as np
import pytest
import torch

import contact_dynamics_ref as CR
import dynamics_ref as DR
import forward_dynamics_ref as FR
from isaacgymdyros_amd import contact_dynamics as CM
from isaacgymdyros_amd import forward_dynamics as FM
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd.model import load_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = CM.GROUP          # envs per workgroup
RMAX = CM.MAX_RHS
PAD = 64
F, U = np.float32, np.uint32
OUTS = CR.OUTS
NEED_RHS = ("accel", "force")


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return __import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0]


@pytest.fixture(scope="module")
def api():
    return CM.declare(lib())


@pytest.fixture(scope="module")
def tables(api):
    model = load_model()
    return {K: torch.from_numpy(CM.pack_table(api, model, CR.ids_of(cs), [p for _, p in cs]).view(np.int32)).to(DEV) for K, cs in CR.SETS.items()}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t, offset=0):
    return None if t is None else t.data_ptr() + 4 * offset


def run(api, tables, K, root, dof, ms, arm, vel_at_com, rhs=None, sub=None, gamma=None, outs=OUTS, offset=0, finite=True, expect=0, nrhs=None):
    """One launch into NaN-filled buffers PAD words too long (and `offset` words past their start); returns the outputs named as a dict (the
    others None): every word written (when the inputs were finite), none outside."""
    n, m = len(root), 6 * K
    R = 0 if rhs is None else rhs.shape[1]
    r = R if nrhs is None else nrhs
    shape = {"jc": (n, m, 39), "jdnu": (n, m), "minv_jt": (n, m, 39), "lambda_inv": (n, m, m), "lambda": (n, m, m), "accel": (n, R, 39), "force": (n, R, m)}
    words = {k: int(np.prod(s)) for k, s in shape.items()}
    d = [dev(root), dev(dof), dev(ms), dev(arm), dev(rhs), dev(sub), dev(gamma)]
    buf = {k: torch.full((offset + words[k] + PAD,), float("nan"), device=DEV) if k in outs and words[k] > 0 else None for k in OUTS}
    assert all(b is None or b.data_ptr() % 16 == 0 for b in buf.values())
    rc = api["solve"](n, tables[K].data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), vel_at_com, ptr(d[4]), r, ptr(d[5]), ptr(d[6]),
                      *[ptr(buf[k], offset) for k in OUTS], stream())
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
        assert np.isnan(h[:offset]).all() and np.isnan(h[offset + w:]).all(), "a word outside %s was written" % k
        o = h[offset:offset + w]
        if finite:
            assert np.isfinite(o).all(), "%d words of %s were not written" % (int(np.isnan(o).sum()), k)
        out[k] = o.reshape(shape[k]).copy()
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(U), np.ascontiguousarray(b).view(U))


def inputs(n, K, vel_at_com, seed, nrhs):
    root, dof, ms, arm, _acc = DR.seeded(n, seed)
    rhs, sub = CR.rhs_of(root, dof, vel_at_com, ms, arm, nrhs, seed + 3)
    return root, dof, ms, arm, rhs, sub, CR.gamma_of(n, 6 * K, seed + 5)


# ---------------------------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("n", [1, G - 1, G, G + 1, 3 * G + 5])
def test_kernel_against_float64(api, tables, n, K, vel_at_com):
    """n = 1: one env in one workgroup; G - 1, G, G + 1: the group's edge; 3 G + 5: four whole groups and a partial one.  Eight right-hand sides
    and one: every channel within 4 d (accel and force: d scaled with the solution)."""
    root, dof, ms, arm, rhs, sub, gamma = inputs(n, K, vel_at_com, 100 * n + 10 * K + vel_at_com, RMAX)
    want = CR.evaluate(root, dof, vel_at_com, ms, arm, CR.SETS[K], rhs, sub, gamma)
    o = run(api, tables, K, root, dof, ms, arm, vel_at_com, rhs, sub, gamma)
    ex = CR.excess(o, root, dof, ms, arm, vel_at_com, K, rhs, sub, gamma, report="gpu n=%d K=%d vel_at_com=%d R=%d" % (n, K, vel_at_com, RMAX), want=want)
    assert len(ex) == len(CR.CHANNELS) and CR.within(ex), ex
    one = run(api, tables, K, root, dof, ms, arm, vel_at_com, np.ascontiguousarray(rhs[:, :1]), sub, gamma)
    w1 = dict(want, accel=want["accel"][:, :1], force=want["force"][:, :1])
    ex = CR.excess(one, root, dof, ms, arm, vel_at_com, K, rhs[:, :1], sub, gamma, report="gpu n=%d K=%d vel_at_com=%d R=1" % (n, K, vel_at_com), want=w1)
    assert len(ex) == len(CR.CHANNELS) and CR.within(ex), ex
    # the same bits at one right-hand side and eight; lambda and lambda_inv symmetric, with the buffers filled with NaN beforehand
    assert all(same_bits(one[k], o[k][:, :1] if k in NEED_RHS else o[k]) for k in OUTS)
    assert all(same_bits(o[k], np.swapaxes(o[k], 1, 2)) for k in ("lambda", "lambda_inv"))


def test_output_selection_and_unaligned_outputs(api, tables):
    """Every single output alone, all but it, all together, every output 4 bytes past a 16-byte boundary, and the counts of right-hand sides:
    the same bits where the same is asked."""
    n, K = 2 * G + 3, 2
    root, dof, ms, arm, rhs, sub, gamma = inputs(n, K, 0, 10, RMAX)
    full = run(api, tables, K, root, dof, ms, arm, 0, rhs, sub, gamma)
    for k in OUTS:
        one = run(api, tables, K, root, dof, ms, arm, 0, *((rhs, sub, gamma) if k in NEED_RHS else (None, None, None)), outs=(k,))
        assert same_bits(one[k], full[k]) and all(one[j] is None for j in OUTS if j != k), k
        rest = run(api, tables, K, root, dof, ms, arm, 0, rhs, sub, gamma, outs=tuple(j for j in OUTS if j != k))
        assert all(same_bits(rest[j], full[j]) for j in OUTS if j != k), k
    off = run(api, tables, K, root, dof, ms, arm, 0, rhs, sub, gamma, offset=1)
    assert all(same_bits(off[k], full[k]) for k in OUTS)
    for k in (2,):
        ok = run(api, tables, K, root, dof, ms, arm, 0, np.ascontiguousarray(rhs[:, :k]), sub, gamma, outs=NEED_RHS)
        assert all(same_bits(ok[j], full[j][:, :k]) for j in NEED_RHS), k
    last = run(api, tables, K, root, dof, ms, arm, 0, np.ascontiguousarray(rhs[:, RMAX - 1:]), sub, gamma, outs=("force", "lambda"))
    assert same_bits(last["force"][:, 0], full["force"][:, RMAX - 1]) and same_bits(last["lambda"], full["lambda"])
    # gamma NULL equals a gamma of zeros, sub NULL a sub of zeros
    on = run(api, tables, K, root, dof, ms, arm, 0, rhs, None, None, outs=NEED_RHS)
    oz = run(api, tables, K, root, dof, ms, arm, 0, rhs, np.zeros((n, 39), F), np.zeros((n, 6 * K), F), outs=NEED_RHS)
    assert all(same_bits(on[j], oz[j]) for j in NEED_RHS) and not same_bits(on["force"], full["force"])
    # nominal masses, no armature, vel_at_com: another matrix, under the d measured for it
    r1, s1 = CR.rhs_of(root, dof, 1, None, None, 1, 14)
    nom = run(api, tables, K, root, dof, None, None, 1, r1, s1, gamma)
    ex = CR.excess(nom, root, dof, None, None, 1, K, r1, s1, gamma, report="gpu, nominal masses, no armature")
    assert len(ex) == len(CR.CHANNELS) and CR.within(ex), ex
    # refused before any launch: nothing is written
    assert run(api, tables, K, root, dof, ms, arm, 0, rhs, nrhs=RMAX + 1, expect=-1)["accel"] is None and b"nrhs" in api["last_error"]()
    assert run(api, tables, K, root, dof, ms, arm, 0, rhs, nrhs=0, expect=-1)["lambda"] is None and b"nrhs" in api["last_error"]()


@pytest.mark.parametrize("K", [2, 4])
def test_exact_properties(api, tables, K):
    n, m, v = 2 * G + 3, 6 * K, 1
    cs = CR.SETS[K]
    root, dof, ms, arm, rhs, sub, gamma = inputs(n, K, v, 8, 2)
    o = run(api, tables, K, root, dof, ms, arm, v, rhs, sub, gamma)
    # minv_jt[e, r] is dwl_solve's x with rhs = jc[e, r], on the device, six rows to a call (the table's first words are dwl_pack_table's)
    d = [dev(root), dev(dof), dev(ms), dev(arm)]
    fapi = FM.declare(lib())
    for i in range(K):
        rows, x = dev(o["jc"][:, 6 * i:6 * i + 6]), torch.full((n, 6, 39), float("nan"), device=DEV)
        assert fapi["solve"](n, tables[K].data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), v, rows.data_ptr(), 6, None, x.data_ptr(), None, None, stream()) == 0
        torch.cuda.synchronize()
        assert same_bits(x.cpu().numpy(), o["minv_jt"][:, 6 * i:6 * i + 6]), i
    # 640 m out: the same bits
    far = root.copy()
    far[:, 0:2] += np.array([640.0, -640.0], F)
    of = run(api, tables, K, far, dof, ms, arm, v, rhs, sub, gamma)
    assert all(same_bits(of[k], o[k]) for k in OUTS)
    # jc: +0.0 off the path from the base to the carrying body, the identity blocks 1.0 and +0.0
    mask = np.repeat(JM.dof_mask(CR.ids_of(cs), load_model()), 6, 0)
    assert (o["jc"].view(U)[:, ~mask] == 0).all()
    jc4 = o["jc"].reshape(n, K, 6, 39)
    eye3 = np.where(np.eye(3, dtype=bool), np.float32(1.0).view(U), U(0))
    assert (jc4[:, :, 0:3, 0:3].view(U) == eye3).all() and (jc4[:, :, 3:6, 3:6].view(U) == eye3).all() and (jc4[:, :, 3:6, 0:3].view(U) == 0).all()
    # b = 0, gamma = 0 and nu = 0 give zeros
    still_root, still_dof = root.copy(), dof.copy().reshape(n, 33, 2)
    still_root[:, 7:13] = 0
    still_dof[:, :, 1] = 0
    oz = run(api, tables, K, still_root, np.ascontiguousarray(still_dof.reshape(dof.shape)), ms, arm, v, np.zeros((n, 2, 39), F), None, None)
    assert (oz["accel"] == 0).all() and (oz["force"] == 0).all() and (oz["jdnu"] == 0).all()
    # a NaN stays in its env; one in a right-hand side reaches that column of accel and force alone
    bad_r, bad_d, bad_b = root.copy(), dof.copy(), rhs.copy()
    bad_r[2, 4], bad_d[G + 1, 4, 0], bad_b[7, 1, 7] = np.nan, np.inf, np.nan          # (DoF 4 drives moving body 5, on the left foot's path)
    on = run(api, tables, K, bad_r, bad_d, ms, arm, v, bad_b, sub, gamma, finite=False)
    keep = [e for e in range(n) if e not in (2, G + 1, 7)]
    for k in OUTS:
        assert same_bits(on[k][keep], o[k][keep]), k
        assert np.isnan(on[k][2]).any() and np.isnan(on[k][G + 1]).any(), k
    for k in NEED_RHS:
        assert np.isnan(on[k][7, 1]).any() and same_bits(on[k][7, 0], o[k][7, 0]), k
    assert all(same_bits(on[k][7], o[k][7]) for k in OUTS if k not in NEED_RHS)


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
        cfg["sim"]["mi355"]["contact_dynamics"] = spec
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


def test_composition_with_the_shipped_forward_dynamics():
    """On a stepped env: the free-flight forward dynamics with the ground reaction put back, forward_dynamics.forward_dynamics(tau, gen_force =
    jc' force), returns the constrained accel; and jc accel + jdnu = gamma.  Both within the sum of the allowances involved, formed in float64:
    4 d of x for dwl_solve's own solve and 4 d of accel for this one (each scaled with the solution), and what 4 d of force and 4 d of jc
    become through |M^-1| |J_c'|; for the constraint what 4 d of accel, of jc and of jdnu become through the row."""
    n = 64
    env = make_env(n, {"jacobian": True, "lambda": False}, forward_dynamics=True)
    cd, fd = env.contact_dynamics, env.forward_dynamics
    a = torch.zeros(n, 13, device=DEV)
    acts = actions(n, 6, seed=5)
    for i in range(6):
        a.copy_(acts[i])
        env.step(a)
    g = torch.Generator(device=DEV).manual_seed(6)
    tau = torch.randn(n, 33, generator=g, device=DEV) * 20
    gamma = torch.from_numpy(CR.gamma_of(n, 12, 7)).to(DEV)
    cd.refresh()
    acc = cd.forward_dynamics(tau_joint=tau, contact_accel=gamma)
    assert acc is cd.accel and acc.shape == (n, 39) and cd.force.shape == (n, 2, 6) and cd.jc.shape == (n, 12, 39) and cd.lambda_ is None
    gen = torch.bmm(cd.jc.transpose(1, 2), cd.force.reshape(n, 12, 1))[:, :, 0]
    free = fd.forward_dynamics(tau_joint=tau, gen_force=gen).cpu().numpy().astype(np.float64)
    got, force = acc.cpu().numpy().astype(np.float64), cd.force.reshape(n, 12).cpu().numpy().astype(np.float64)
    root, dof, ms, arm = buffers(env, n)
    v = cd.vel_at_com
    sub = cd._bias.bias.cpu().numpy()
    rhs = np.concatenate([np.zeros((n, 6), F), tau.cpu().numpy()], 1)[:, None]
    want = CR.evaluate(root, dof, v, ms, arm, CR.SETS[2], rhs, sub, gamma.cpu().numpy())
    d = CR.measured(v, 2)
    dj = CR.FACTOR * max(d["jc_lin"], d["jc_ang"])
    Minv, Jt = np.abs(np.linalg.inv(want["M"])), np.abs(np.swapaxes(want["jc"], 1, 2))
    through = np.einsum("nab,nb->na", Minv, np.einsum("ncr,nr->nc", Jt, CR.allowance(want, v, 2, "force")[:, 0]) + dj * np.abs(want["force"][:, 0]).sum(-1, keepdims=True))
    allow = FR.x_allowance(want["accel"][:, 0], v) + CR.allowance(want, v, 2, "accel")[:, 0] + through
    err = np.abs(free - got)
    print("forward_dynamics(tau, jc' force) - accel: %.2e with |accel| up to %.0f, %.3f of the allowance" % (err.max(), np.abs(got).max(), (err / allow).max()))
    assert (err <= allow).all()
    jc, jd = cd.jc.cpu().numpy().astype(np.float64), cd.jdnu.cpu().numpy().astype(np.float64)
    res = np.abs(np.einsum("nrc,nc->nr", jc, got) + jd - gamma.cpu().numpy().astype(np.float64))
    allow = (np.einsum("nrc,nc->nr", np.abs(want["jc"]), CR.allowance(want, v, 2, "accel")[:, 0]) + dj * np.abs(want["accel"][:, 0]).sum(-1, keepdims=True)
             + CR.FACTOR * max(d["jdnu_lin"], d["jdnu_ang"]))
    print("jc accel + jdnu - gamma: %.2e, %.3f of the allowance" % (res.max(), (res / allow).max()))
    assert (res <= allow).all()
    # accel and force against the float64 reference, and contact_accel None is a gamma of zeros
    ex = CR.excess({"accel": got[:, None], "force": force[:, None]}, root, dof, ms, arm, v, 2, rhs, sub, gamma.cpu().numpy(), want=want)
    z1 = cd.forward_dynamics(tau_joint=tau).clone()
    z2 = cd.forward_dynamics(tau_joint=tau, contact_accel=torch.zeros(n, 12, device=DEV))
    same = torch.equal(z1, z2)
    env.close()
    assert CR.within(ex) and same, ex


def test_live_env_with_resets(api, tables):
    n, steps = 64, 40
    acts = actions(n, steps)
    runs = {}
    every = {"rhs": 2, "jacobian": True, "lambda": True, "lambda_inv": True, "minv_jt": True, "auto": True}
    kept = ("jc", "jdnu", "lambda_", "lambda_inv", "minv_jt")
    for name, spec, mi in (("off", None, {}), ("auto", every, {}), ("beside", {"auto": True, "armature": False, "contacts": [{"body": "L_Foot_Link", "pos": [0, 0, -0.09]}]},
                                                                     {"episode_stats": True})):
        env = make_env(n, spec, **mi)
        a, h, resets = torch.zeros(n, 13, device=DEV), [], 0
        if spec is None:
            assert env.contact_dynamics is None
        for i in range(steps):
            a.copy_(acts[i])
            o, r, d, _ex = env.step(a)
            h.append(bits(o["obs"], r, d, env._buf["root_states"], env._buf["env_state"]))
            resets += int(d.sum())
            if name == "auto" and (i % 3 == 0 or i == steps - 1):
                cd = env.contact_dynamics
                held = {k.rstrip("_"): getattr(cd, k).cpu().numpy().copy() for k in kept}
                root, dof, ms, arm = buffers(env, n)
                rhs, _sub = CR.rhs_of(root, dof, cd.vel_at_com, ms, arm, 2, i)
                gamma = CR.gamma_of(n, 12, i)
                cd.gamma.copy_(torch.from_numpy(gamma).to(DEV))
                acc = cd.solve(torch.from_numpy(rhs).to(DEV)).cpu().numpy()
                fresh = run(api, tables, 2, root, dof, ms, arm, cd.vel_at_com, rhs, None, gamma)
                assert all(same_bits(held[k], fresh[k]) for k in held) and same_bits(acc, fresh["accel"]) and same_bits(cd.force_all.cpu().numpy(), fresh["force"]), i
                if i % 12 == 0 or i == steps - 1:
                    ex = CR.excess(fresh, root, dof, ms, arm, cd.vel_at_com, 2, rhs, None, gamma)
                    assert CR.within(ex), (i, ex)
        if name == "auto":
            assert cd.vel_at_com == 1 and cd.nrhs == 2 and cd.names == ["L_Foot_Link", "R_Foot_Link"] and cd.index("R_Foot_Link") == 1
            assert cd.jc.shape == cd.minv_jt.shape == (n, 12, 39) and cd.lambda_.shape == cd.lambda_inv.shape == (n, 12, 12) and cd.jdnu.shape == (n, 12)
            assert cd.rhs.shape == cd.accel_all.shape == (n, 2, 39) and cd.force_all.shape == (n, 2, 12) and cd.gamma.shape == (n, 12)
            with pytest.raises(ValueError):
                cd.index("Head_Link")
            # reset_idx refreshes too: the tensors are those of the buffers after it
            before = cd.lambda_.clone()
            env.reset_idx(torch.arange(0, n, 2, device=DEV))
            held = cd.lambda_.clone()
            cd.refresh()
            assert torch.equal(cd.lambda_, held) and not torch.equal(held[0::2], before[0::2]) and torch.equal(held[1::2], before[1::2])
        if name == "beside":
            cd = env.contact_dynamics
            assert cd.lambda_inv is None and cd.minv_jt is None and cd.lambda_.shape == (n, 6, 6) and cd.jc.shape == (n, 6, 39) and cd.nrhs == 1
            root, dof, ms, arm = buffers(env, n)
            fresh = run(api, tables, 1, root, dof, ms, None, cd.vel_at_com, outs=("jc", "jdnu", "lambda"))
            assert same_bits(cd.lambda_.cpu().numpy(), fresh["lambda"]) and same_bits(cd.jc.cpu().numpy(), fresh["jc"]) and same_bits(cd.jdnu.cpu().numpy(), fresh["jdnu"])
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
        env = make_env(n, {"lambda_inv": True, "minv_jt": True, "auto": True})
        cd = env.contact_dynamics
        a, tau = torch.zeros(n, 13, device=DEV), torch.zeros(n, 33, device=DEV)
        a.copy_(acts[0])
        env.step(a)                            # (the first step is eager on both sides)
        cd.solve(rhss[0])
        cd.forward_dynamics(tau_joint=tau)
        torch.cuda.synchronize()
        h = []
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            gr = torch.cuda.CUDAGraph()
            a.copy_(acts[1])
            with torch.cuda.graph(gr, stream=side):
                env.step(a)
                cd.solve()
                cd.forward_dynamics(tau_joint=tau)
            # (the capture itself ran nothing: replay the recorded step for each of the 10 actions)
        for i in range(1, 11):
            a.copy_(acts[i])
            tau.copy_(taus[i])
            cd.rhs.copy_(rhss[i])
            if captured:
                gr.replay()
            else:
                env.step(a)
                cd.solve()
                cd.forward_dynamics(tau_joint=tau)
            h.append(bits(cd.jc, cd.jdnu, cd.lambda_, cd.lambda_inv, cd.minv_jt, cd.accel_all, cd.force_all, cd.accel, cd.force, env._buf["root_states"]))
        torch.cuda.synchronize()
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1])


def test_tocabi_amp_lower(api, tables):
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    n = 32
    cfg = default_amp_cfg(n, DEV)
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert amp.contact_dynamics is None
    amp.close()
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"].setdefault("mi355", {})["amp_contact_dynamics"] = {"lambda_inv": True, "minv_jt": True, "auto": True}
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert isinstance(amp.contact_dynamics, CM.ContactDynamics) and amp._phys.contact_dynamics is None
    cd = amp.contact_dynamics
    assert cd.vel_at_com == int(amp._phys._ccfg.root_vel_at_com)
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(20):
        amp.step((torch.rand(n, amp.num_actions, generator=g, device=DEV) * 2 - 1) * 0.1)
    root, dof, ms, arm = buffers(amp._phys, n)
    rhs, _sub = CR.rhs_of(root, dof, cd.vel_at_com, ms, arm, 1, 7)
    acc = cd.solve(torch.from_numpy(rhs[:, 0]).to(DEV))          # ([N, 39] for one right-hand side)
    assert acc is cd.accel_all
    got = {k.rstrip("_"): getattr(cd, k).cpu().numpy() for k in ("jc", "jdnu", "lambda_", "lambda_inv", "minv_jt")}          # (what the last step's auto refresh left)
    got.update(accel=acc.cpu().numpy(), force=cd.force_all.cpu().numpy())
    ex = CR.excess(got, root, dof, ms, arm, cd.vel_at_com, 2, rhs, None, np.zeros((n, 12), F), report="TocabiAMPLower")
    amp.close()
    assert len(ex) == len(CR.CHANNELS) and CR.within(ex), ex


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_contact_arrays(tmp_path):
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
    for name, flag in (("plain", []), ("contact", ["--dynamics-contact", "--dynamics-forces"])):
        out = tmp_path / name
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64",
                            "--games", "64", "--max-steps", "60", "--episode-length", "0.1", "--dynamics-dir", str(out), "--dynamics-envs", "2"] + flag,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["dynamics_env0.npz", "dynamics_env1.npz"]
        files[name] = np.load(out / "dynamics_env1.npz")
    plain, z = files["plain"], files["contact"]
    old = ["names", "dof_names", "dt", "jacobian", "mass_matrix", "com_jacobian"]
    new = ["contact_jacobian", "contact_lambda", "contact_force_zero_torque"]
    assert sorted(plain.files) == sorted(old) and sorted(z.files) == sorted(old + ["bias", "gravity", "momentum"] + new)
    assert all(np.array_equal(plain[k], z[k]) for k in old)          # (the same seed: the files are what they were, plus the new arrays)
    T = z["jacobian"].shape[0]
    assert 20 <= T <= 60 and z["contact_jacobian"].shape == (T, 12, 39) and z["contact_lambda"].shape == (T, 12, 12) and z["contact_force_zero_torque"].shape == (T, 2, 6)
    assert all(np.isfinite(z[k]).all() for k in new) and same_bits(z["contact_lambda"], np.swapaxes(z["contact_lambda"], 1, 2))
    # the feet's frames move with the feet's bodies: the angular rows are the body Jacobians' of the same file (jacobian rows 1, 2: the feet)
    assert same_bits(z["contact_jacobian"].reshape(T, 2, 6, 39)[:, :, 3:6], z["jacobian"][:, 1:3, 3:6])
    # the contact-space inertia against the files' own M and J_c (the bits the kernel factored), inverted in float64: within 4 d of lambda,
    # which also pays for the chain and for forming M and J_c
    M, J = z["mass_matrix"].astype(np.float64), z["contact_jacobian"].astype(np.float64)
    A = J @ np.linalg.solve(M, np.swapaxes(J, 1, 2))
    d = CR.measured(1, 2)
    err = np.abs(np.linalg.inv(A) - z["contact_lambda"].astype(np.float64)).max()
    print("the player's contact_lambda against the files' own M and J_c: %.2e, %.3f of 4 d" % (err, err / (CR.FACTOR * d["lambda"])))
    assert err <= CR.FACTOR * d["lambda"]
