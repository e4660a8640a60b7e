#!/usr/bin/env python3
"""The device bits of dwi_solve and dwk_solve (DESIGN.md sections 27 and 28) on a fixed set of inputs.
  --record FILE: writes the inputs and every output of both entry points to an .npz.
  --check FILE:  reruns both entry points on the stored inputs and compares every output bit for bit; exit status 1 on a difference.
N = 5 envs (two workgroups, the second holds one env); dwi_solve with K = 1, 2 and 4 contacts, dwk_solve with K = 2 and 4 and env e in stance
pattern (e + s) mod 2^K (s = 0, or 2^K - 1 with vel_at_com: flight, single support and every contact on are among them); both velocity modes;
moments weighted 10 x, with f_ref, mass_scale and dof_armature.  The states are tests/dynamics_ref.seeded's (--record only reads them).
Those wrenches follow a seeded f_ref of 200 N, which no sole can deliver: feasible is 0 in every one of them.  One more dwk_solve case
therefore stands still: the initial pose at rest, no f_ref, unit weights, the envs on both feet, in flight, on the left, on the right and on
both again, where feasible is 1, 0, 0, 0, 1."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
N, SEED = 5, 2728
FEET = [{"body": "L_Foot_Link", "pos": [0.0, 0.0, -0.09]}, {"body": "R_Foot_Link", "pos": [0.0, 0.0, -0.09]}]
SETS = {1: FEET[:1], 2: FEET, 4: FEET + [{"body": "L_Wrist2_Link", "pos": [0.02, -0.01, -0.05]}, {"body": "R_Wrist2_Link", "pos": [0.02, 0.01, -0.05]}]}
W10 = [1.0, 1.0, 1.0, 10.0, 10.0, 10.0]
GRAVITY = (0.0, 0.0, -9.81)
IOUTS = (("tau_joint", 33), ("force", None), ("contact_accel", None), ("tau_full", 39))
KOUTS = IOUTS + (("base_residual", 6), ("margins", None), ("feasible", 1))
CASES = [("dwi", K, v, "") for K in (1, 2, 4) for v in (0, 1)] + [("dwk", K, v, "") for K in (2, 4) for v in (0, 1)] + [("dwk", 2, 0, "stand_")]


def stance_of(K, v):
    p = (np.arange(N) + (((1 << K) - 1) if v else 0)) % (1 << K)
    return ((p[:, None] >> np.arange(K)) & 1).astype(np.uint8)


def inputs():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dynamics_ref as DR
    root, dof, ms, arm, acc = DR.seeded(N, SEED)
    d = {"root": root, "dof": dof, "mass_scale": ms, "dof_armature": arm, "accel": acc}
    for K in SETS:
        r = np.random.default_rng(SEED + K)
        d["force_ref_K%d" % K] = (r.normal(0, 1, (N, K, 6)) * np.array([200.0] * 3 + [20.0] * 3)).reshape(N, 6 * K).astype(np.float32)
    for K in (2, 4):
        for v in (0, 1):
            d["stance_K%d_v%d" % (K, v)] = stance_of(K, v)
    from isaacgymdyros_amd.task_constants import INITIAL_DOF_POS
    d["stand_root"], d["stand_dof"] = np.zeros((N, 13), np.float32), np.zeros((N, 33, 2), np.float32)
    d["stand_root"][:, 2], d["stand_root"][:, 6], d["stand_dof"][:, :, 0] = 0.93, 1.0, np.asarray(INITIAL_DOF_POS, np.float32)
    d["stand_stance"] = stance_of(2, 1)
    return d


def outputs(d):
    """Every output of every case on the inputs d, as {"<abi>_K<K>_v<v>_<output>": array}."""
    import torch
    from isaacgymdyros_amd import _lib
    from isaacgymdyros_amd import contact_inverse_dynamics as IM
    from isaacgymdyros_amd import stance_inverse_dynamics as SM
    from isaacgymdyros_amd.model import load_model
    lib, model = _lib.load()[0], load_model()
    api = {"dwi": IM.declare(lib), "dwk": SM.declare(lib)}
    dev = {k: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for k, a in d.items()}
    stream, out = torch.cuda.current_stream().cuda_stream, {}
    for abi, K, v, tag in CASES:
        c = IM.resolve({"contacts": SETS[K], "weights": None if tag else W10}, model.body_names, model.body_moving)
        at = (lambda k: dev[k].data_ptr())
        root, dof, ms, arm, acc, fr, stance = ([at("stand_root"), at("stand_dof"), None, None, None, None, "stand_stance"] if tag else
                                               [at("root"), at("dof"), at("mass_scale"), at("dof_armature"), at("accel"), at("force_ref_K%d" % K), "stance_K%d_v%d" % (K, v)])
        if abi == "dwi":
            t, outs, st = IM.pack_table(api[abi], model, c["ids"], c["pos"], c["w"]), IOUTS, ()
        else:
            t = SM.pack_table(api[abi], model, c["ids"], c["pos"], c["w"], SM.resolve_soles("model", c["ids"], c["pos"], model), 1.0)
            outs, st = KOUTS, (at(stance),)
        table = torch.from_numpy(t.view(np.int32)).to(DEV)
        buf = {k: torch.full((N, w), 255, dtype=torch.uint8, device=DEV) if k == "feasible"
               else torch.full((N, (4 if k == "margins" else 6) * K if w is None else w), float("nan"), device=DEV) for k, w in outs}
        rc = api[abi]["solve"](N, table.data_ptr(), root, dof, ms, arm, *GRAVITY, acc, fr, *st, v, *[buf[k].data_ptr() for k, _ in outs], stream)
        torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError(api[abi]["last_error"]().decode())
        for k, _ in outs:
            out["%s_K%d_v%d_%s%s" % (abi, K, v, tag, k)] = buf[k].cpu().numpy()
    return out


def differences(path):
    """The names of the outputs whose bits differ from the file's, with the number of differing bytes."""
    with np.load(path) as z:
        stored = {k: z[k] for k in z.files}
    want = {k: a for k, a in stored.items() if k.startswith(("dwi_", "dwk_"))}
    got = outputs({k: a for k, a in stored.items() if k not in want})
    assert sorted(got) == sorted(want) and len(want) == 6 * len(IOUTS) + 5 * len(KOUTS), "the file does not hold this tool's cases"
    bad = {}
    for k, a in want.items():
        b = got[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            bad[k] = -1
        elif not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            bad[k] = int((a.view(np.uint8) != b.view(np.uint8)).sum())
    return bad


def main():
    ap = argparse.ArgumentParser()
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--record", metavar="FILE")
    g.add_argument("--check", metavar="FILE")
    a = ap.parse_args()
    if a.record:
        d = inputs()
        d.update(outputs(d))
        assert all(np.isfinite(v).all() for k, v in d.items() if v.dtype == np.float32), "an output word was not written"
        assert d["dwk_K2_v0_stand_feasible"].reshape(-1).tolist() == [1, 0, 0, 0, 1], "the standing case does not pin feasible = 1"
        np.savez_compressed(a.record, **d)
        print("recorded %d arrays, %d bytes" % (len(d), os.path.getsize(a.record)))
        return 0
    bad = differences(a.check)
    for k, n in sorted(bad.items()):
        print("%s: %s" % (k, "shape or type differs" if n < 0 else "%d bytes differ" % n))
    print("bits differ" if bad else "the same bits")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
