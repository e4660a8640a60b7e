"""The walk learner's rollout kernels (dwp_rollout_pre / _post, dwp_gae, dwp_policy: include/dyros_ppo.h, csrc/dw_ppo.hip) through the C ABI at
their row and launch edges, against the float64 restatement tests/ppo_rollout_truth.py with the bounds derived there (tests/test_ppo_rollout_truth.py
holds that restatement to the consumer's own functions and shows that its checks reject eight injected faults).  Every output is allocated with
NaN-filled guard rows and compared as a whole: bit for bit where a kernel copies, within the bound where it computes, untouched elsewhere.

A line `ppo-rollout-edges ...` per case reports the worst error of each stage as a fraction of its bound (pytest -s shows them; DESIGN.md
section 10 has the table)."""
import itertools

import numpy as np
import pytest
import torch

import ppo_rollout_truth as T
from isaacgymdyros_amd import _lib
from isaacgymdyros_amd import ppo_update as PU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PPO = T.consumer()
NS, HS = (4, 252, 255, 256, 260, 1024, 1028), (1, 3)          # (255: odd, so N * num_obs is no multiple of 4 for an odd num_obs -- refused)
NOBS = (13, 16, 48, 52, 487, 488, 512)
LAYOUTS = ("step", "env", "half")
POLICY_NS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4097)
GAE_NS, GAE_HS = (1, 255, 256, 257, 513), (1, 2, 128)
# the forms of dwp_rollout_post: time_outs given or NULL, g_obs distinct or == new_obs, terms NULL or 1 / 15 / 64 of more columns
POST_FORMS = [dict(time_outs=to, same=same, nterms=nt) for to, same, nt in itertools.product((True, False), (False, True), (15, 0, 1, 64))]


@pytest.fixture(scope="module")
def api():
    return PU.declare(_lib.load()[0])


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def back(t, like):
    a = t.cpu().numpy()
    return a.view(np.uint16) if like.dtype == np.uint16 else a


def row1(t):
    return t.data_ptr() + t.stride(0) * t.element_size()


def report(what, case, worst):
    print("ppo-rollout-edges %s %s %s" % (what, case, " ".join("%s=%.3g" % kv for kv in sorted(worst.items()))))


def merge(worst, res):
    for k, v in res.items():
        worst[k] = max(worst.get(k, 0.0), v)


def call_pre(api, inp, before, nobs=None):
    d = {k: dev(v) for k, v in before.items()}
    t = {k: dev(inp[k]) for k in ("mu", "value", "noise", "obs", "dones", "logstd")}
    n = torch.tensor([inp["n"]], dtype=torch.int64, device=DEV)
    layout, H = inp["layout"], inp["H"]
    rc = api["rollout_pre"](t["mu"].data_ptr(), t["value"].data_ptr(), t["noise"].data_ptr(), t["obs"].data_ptr(), t["dones"].data_ptr(), t["logstd"].data_ptr(),
                            n.data_ptr(), inp["N"], inp["nobs"] if nobs is None else nobs, row1(d["mb_obs"]), row1(d["mb_act"]), row1(d["mb_mu"]), row1(d["mb_nlp"]),
                            row1(d["mb_val"]), row1(d["mb_done"]), row1(d["act"]), 0 if layout == "step" else H, int(layout == "half"), H, stream())
    torch.cuda.synchronize()
    assert int(n.item()) == inp["n"] and all(np.array_equal(T.bits(back(t[k], inp[k])), T.bits(inp[k])) for k in t)          # (the inputs are only read)
    return rc, {k: back(v, before[k]) for k, v in d.items()}


def call_post(api, inp, before, nobs=None):
    d = {k: dev(v) for k, v in before.items()}
    t = {k: dev(inp[k]) for k in ("rew", "value", "done", "new_obs")}
    to = dev(inp["time_outs"]) if inp["time_outs"] is not None else None
    st = dev(inp["stacked"]) if inp["stacked"] is not None else None
    n = torch.tensor([inp["n"]], dtype=torch.int64, device=DEV)
    new_obs = row1(d["new_obs"]) if inp["same"] else t["new_obs"].data_ptr()
    rc = api["rollout_post"](t["rew"].data_ptr(), t["value"].data_ptr(), None if to is None else to.data_ptr(), None if st is None else st.data_ptr(), inp["ncols"],
                             t["done"].data_ptr(), new_obs, n.data_ptr(), inp["N"], inp["nobs"] if nobs is None else nobs, inp["scale"], inp["gamma"],
                             row1(d["mb_rew"]), row1(d["terms"]) if "terms" in d else None, inp["nterms"], row1(d["g_dones"]),
                             new_obs if inp["same"] else row1(d["g_obs"]), inp["H"], stream())
    torch.cuda.synchronize()
    assert all(np.array_equal(T.bits(back(t[k], inp[k])), T.bits(inp[k])) for k in t)
    return rc, {k: back(v, before[k]) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ dwp_rollout_pre
@pytest.mark.parametrize("nobs", NOBS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rollout_pre_at_row_and_launch_edges(api, layout, nobs):
    """Every step of a rollout of H rows into the same guarded buffers, at every N: the step's row is right, everything else is as it was."""
    for N in NS:
        worst = {}
        for H in HS:
            rng = np.random.default_rng(1000 * N + 10 * nobs + H)
            bufs = T.alloc_pre(N, H, nobs, layout)
            for n in range(H):
                inp = T.pre_inputs(rng, N, H, nobs, n, layout)
                rc, after = call_pre(api, inp, bufs)
                if (N * nobs) % 4:
                    assert rc == -1 and all(T.exact(after[k], bufs[k]) == 0.0 for k in bufs), (N, H, n)
                    continue
                assert rc == 0, api["last_error"]()
                res = T.check_pre(inp, bufs, after)
                assert T.failures(res) == [], (N, H, n, res)
                merge(worst, res)
                bufs = after
        report("pre", "%s nobs=%d N=%d" % (layout, nobs, N), {k: worst[k] for k in ("mb_act", "mb_nlp") if k in worst})


@pytest.mark.parametrize("layout", LAYOUTS)
def test_row_counter_outside_the_rows_records_nothing_and_still_acts(api, layout):
    for N, nobs, H in ((260, 16, 3), (1028, 487, 3), (256, 13, 1)):
        for n in (-1, H, H + 5):
            rng = np.random.default_rng(N + nobs + n)
            inp, bufs = T.pre_inputs(rng, N, H, nobs, n, layout), T.alloc_pre(N, H, nobs, layout)
            rc, after = call_pre(api, inp, bufs)
            assert rc == 0, api["last_error"]()
            res = T.check_pre(inp, bufs, after)
            assert T.failures(res) == [] and res["mb_obs"] == 0.0 and res["mb_act_rest"] == 0.0, (N, nobs, n, res)
            pin = T.post_inputs(rng, N, H, nobs, n)
            pb = T.alloc_post(pin, rng)
            rc, pa = call_post(api, pin, pb)
            assert rc == 0, api["last_error"]()
            res = T.check_post(pin, pb, pa)
            assert T.failures(res) == [] and res["terms"] == 0.0 and res["mb_rew_rest"] == 0.0, (N, nobs, n, res)


# ------------------------------------------------------------------------------------------------ dwp_rollout_post
@pytest.mark.parametrize("nobs", NOBS)
def test_rollout_post_at_row_and_launch_edges(api, nobs):
    forms = itertools.cycle(POST_FORMS[NOBS.index(nobs):] + POST_FORMS[:NOBS.index(nobs)])
    for N in NS:
        worst = {}
        for H in HS:
            rng = np.random.default_rng(2000 * N + 10 * nobs + H)
            for n in range(H):
                form = next(forms)
                inp = T.post_inputs(rng, N, H, nobs, n, **form)
                bufs = T.alloc_post(inp, rng)
                rc, after = call_post(api, inp, bufs)
                if (N * nobs) % 4:
                    assert rc == -1 and all(T.exact(after[k], bufs[k]) == 0.0 for k in bufs), (N, H, n)
                    continue
                assert rc == 0, api["last_error"]()
                res = T.check_post(inp, bufs, after)
                assert T.failures(res) == [], (N, H, n, form, res)
                merge(worst, res)
        report("post", "nobs=%d N=%d" % (nobs, N), {k: worst[k] for k in ("mb_rew", "terms") if k in worst})


@pytest.mark.parametrize("N,nobs", [(260, 16), (1028, 487), (1024, 13), (1024, 2), (1024, 1), (260, 3)])
def test_rollout_post_every_form(api, N, nobs):
    """num_obs below 4 (dwp_rollout_post takes any from 1 on): the observation copy has fewer 16-byte pieces than there are envs, and the grid is the envs'."""
    worst = {}
    for i, form in enumerate(POST_FORMS):
        rng = np.random.default_rng(N + i)
        inp = T.post_inputs(rng, N, 3, nobs, i % 3, **form)
        bufs = T.alloc_post(inp, rng)
        rc, after = call_post(api, inp, bufs)
        assert rc == 0, api["last_error"]()
        res = T.check_post(inp, bufs, after)
        assert T.failures(res) == [], (form, res)
        merge(worst, res)
    report("post-forms", "nobs=%d N=%d" % (nobs, N), {k: worst[k] for k in ("mb_rew", "terms")})


def test_rollout_calls_that_are_refused(api):
    """N * num_obs not a multiple of 4 (the kernels move 16-byte pieces), fewer observation words than actions, an fp16 row longer than its 512
    words, a rollout_post without observation words: -1 with a message, and nothing is launched."""
    rng = np.random.default_rng(9)
    for N, nobs, layout, arg, msg in ((6, 13, "step", None, "multiple of 4"), (3, 487, "env", None, "multiple of 4"), (5, 13, "half", None, "multiple of 4"),
                                      (8, 16, "step", 12, "bad argument"), (8, 520, "env", None, None), (8, 520, "half", None, "bad argument")):
        inp, bufs = T.pre_inputs(rng, N, 2, nobs, 0, layout), T.alloc_pre(N, 2, min(nobs, T.INP) if layout == "half" else nobs, layout)
        rc, after = call_pre(api, inp, bufs, nobs=arg)
        if msg is None:          # (a row longer than 512 words is fine in fp32)
            assert rc == 0 and T.failures(T.check_pre(inp, bufs, after)) == []
            continue
        assert rc == -1 and msg in api["last_error"]().decode(), (N, nobs, layout, api["last_error"]())
        assert all(T.exact(after[k], bufs[k]) == 0.0 for k in bufs)
    for N, nobs, arg, msg in ((6, 13, None, "multiple of 4"), (8, 16, 0, "bad argument"), (8, 16, -4, "bad argument")):
        for same in (False, True):
            inp = T.post_inputs(rng, N, 2, nobs, 0, same=same)
            bufs = T.alloc_post(inp, rng)
            rc, after = call_post(api, inp, bufs, nobs=arg)
            assert rc == -1 and msg in api["last_error"]().decode(), (N, nobs, arg, api["last_error"]())
            assert all(T.exact(after[k], bufs[k]) == 0.0 for k in bufs)
    for kw in (dict(nterms=15, ncols=14), dict(nterms=T.TERMS_MAX + 1, ncols=T.TERMS_MAX + 2)):          # (fewer columns than terms; more terms than the kernel reduces)
        inp = T.post_inputs(rng, 8, 2, 16, 0, **kw)
        bufs = T.alloc_post(inp, rng)
        rc, after = call_post(api, inp, bufs)
        assert rc == -1 and all(T.exact(after[k], bufs[k]) == 0.0 for k in bufs), kw


# ------------------------------------------------------------------------------------------------ dwp_gae
@pytest.mark.parametrize("pattern", T.DONE_PATTERNS)
def test_gae_at_workgroup_edges(api, pattern):
    worst = {}
    for N in GAE_NS:
        for H in GAE_HS:
            inp = T.gae_inputs(np.random.default_rng(N + H), N, H, pattern)
            bufs = T.alloc_gae(N, H)
            t = {k: dev(inp[k]) for k in ("fdones", "last_values", "mb_fdones", "mb_values", "mb_rewards")}
            advs = dev(bufs["advs"])
            rc = api["gae"](t["fdones"].data_ptr(), t["last_values"].data_ptr(), t["mb_fdones"].data_ptr(), t["mb_values"].data_ptr(), t["mb_rewards"].data_ptr(),
                            inp["gamma"], inp["tau"], H, N, row1(advs), stream())
            assert rc == 0, api["last_error"]()
            torch.cuda.synchronize()
            truth = T.gae_truth(inp["fdones"], inp["last_values"], inp["mb_fdones"], inp["mb_values"], inp["mb_rewards"], inp["gamma"], inp["tau"])
            res = T.check_gae(inp, bufs, {"advs": back(advs, bufs["advs"])}, truth)
            assert T.failures(res) == [], (N, H, res)
            # the reference's own fp32 loop (examples/ppo_consumer.py::discount_values) sits within the same bound
            c = lambda k: torch.from_numpy(inp[k])          # noqa: E731
            ref = PPO.discount_values(c("fdones"), c("last_values").unsqueeze(1), c("mb_fdones"), c("mb_values").unsqueeze(2), c("mb_rewards").unsqueeze(2),
                                      inp["gamma"], inp["tau"]).squeeze(2).numpy()
            res["reference_loop"] = T.ratio(ref, *truth)
            assert res["reference_loop"] <= 1.0, (N, H, res)
            merge(worst, res)
            report("gae", "%s N=%d H=%d" % (pattern, N, H), {k: res[k] for k in ("advs", "reference_loop")})
    report("gae", "%s worst" % pattern, {k: worst[k] for k in ("advs", "reference_loop")})


# ------------------------------------------------------------------------------------------------ dwp_policy
@pytest.fixture(scope="module")
def policy_case(api):
    """One learner with lively weights and dead units, 4097 observation rows (T.policy_obs), their float64 truth and bounds, a plain fp32
    evaluation on the CPU, and the kernel's outputs for all 4097 rows: computed once, read by every case."""
    net = T.policy_net(2).to(DEV)
    fused = PU.FusedPpoUpdate(net, dict(PPO.TRAIN_CFG["config"]), 32, 1, DEV)
    W = T.weights_of(net)
    assert float(fused.views["W1"][:, list(T.DEAD_UNITS)].abs().max()) == 0.0
    obs = T.policy_obs(max(POLICY_NS), 2)
    truth = T.policy_truth(W, obs)
    mu32, v32 = T._forward(W, obs, np.float32)
    case = {"fused": fused, "obs": obs, "obs_dev": dev(obs), "truth": truth, "f32": (mu32, v32)}
    case["whole"] = run_policy(api, case, max(POLICY_NS))[1]
    return case


def run_policy(api, case, N):
    f, bufs = case["fused"], T.alloc_policy(N)
    d = {k: dev(v) for k, v in bufs.items()}
    obs = case["obs_dev"][:N].clone()          # (its own allocation: nothing lies behind row N - 1 that a read past the end could take for a row)
    rc = api["policy"](obs.data_ptr(), f.p.data_ptr(), f.p32f.data_ptr(), N, row1(d["mu"]), row1(d["value"]), stream())
    assert rc == 0, api["last_error"]()
    torch.cuda.synchronize()
    return bufs, {k: back(v, bufs[k]) for k, v in d.items()}


@pytest.mark.parametrize("N", POLICY_NS)
def test_policy_rows_at_tile_edges(api, policy_case, N):
    bufs, after = run_policy(api, policy_case, N)
    res = T.check_policy(N, bufs, after, policy_case["truth"])          # both outputs within the bound; nothing past row N, nothing before row 0
    assert T.failures(res) == [], (N, res)
    # row r of N rows is row r of 4097 rows, bit for bit (a row's result does not depend on its tile's other rows, nor on the rows re-read past the end)
    for k in ("mu", "value"):
        assert T.exact(after[k][1:1 + N], policy_case["whole"][k][1:1 + N]) == 0.0, (N, k)
    # with lively weights the absolute-value forward S is about 2000 times the output and the derived bound about 0.7 of it: next to it, both
    # outputs are held to the error a plain fp32 evaluation makes on rows of the same kind (128 times its largest over the 4097 rows, as
    # tests/test_walk_play_gpu.py holds dwp_play), the rows scaled by 1e3 and the others apart
    mu64, v64, _bmu, _bv = policy_case["truth"]
    mu32, v32 = policy_case["f32"]
    big = np.zeros(max(POLICY_NS), bool)
    big[T.policy_big_rows(max(POLICY_NS))] = True
    for name, rows in (("_big", big), ("", ~big)):
        if not rows[:N].any():
            continue
        for k, t64, t32 in (("mu", mu64, mu32), ("value", v64, v32)):
            e_hip = np.abs(after[k][1:1 + N][rows[:N]].astype(np.float64) - t64[:N][rows[:N]]).max()
            e_32 = np.abs(t32[rows].astype(np.float64) - t64[rows]).max()
            res[k + name + "_vs_fp32"] = e_hip / (128 * e_32 + 1e-6 * max(np.abs(t64[rows]).max(), 1e-3))
    assert T.failures(res) == [], (N, res)
    report("policy", "N=%d" % N, {k: v for k, v in res.items() if not k.endswith("guards")})
