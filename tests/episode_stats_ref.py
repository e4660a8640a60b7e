"""A numpy restatement of the episode statistics (include/dyros_stats.h, isaacgymdyros_amd/csrc/dw_stats.h), vectorised over envs, in float32 where
the kernels are.  Used by tests/test_episode_stats.py (against the g++ build) and tests/test_episode_stats_gpu.py (against the HIP kernels and the
step's own flags)."""
from __future__ import annotations

import numpy as np

from isaacgymdyros_amd import abi
from isaacgymdyros_amd.episode_stats import K

f32 = np.float32
E = abi.K
NEVER = K["DWS_OFF_NEVER"]
LF, RF = K["DWS_LFOOT"], K["DWS_RFOOT"]


def es_int(es, off):
    return np.ascontiguousarray(es).view(np.int32)[:, off]


def over_1n(cf):
    """[n, 38] bool: |F| > 1 N, the soles excluded (synthetic cases keep away from the threshold; the GPU tests use the kernel's own bits)."""
    o = np.sqrt((cf.astype(np.float64) ** 2).sum(-1)) > 1.0
    o[:, LF] = False
    o[:, RF] = False
    return o


class StatsRef:
    def __init__(self, n, max_len, dt_policy):
        self.n, self.ml, self.dtp = n, f32(max_len), f32(dt_policy)
        self.st = np.zeros((K["DWS_ST_WORDS"], n), np.uint32)
        self.si, self.sf = self.st.view(np.int32), self.st.view(np.float32)
        self.ac = np.zeros((K["DWS_AC_WORDS"], n), np.float32)
        self.ct = np.zeros(K["DWS_CT_WORDS"], np.int64)

    def _begin(self, m, steps, root, tv0, pert, nanr):
        si, sf = self.si, self.sf
        si[K["DWS_ST_N"], m] = steps[m]
        si[K["DWS_ST_NAN"], m] = nanr[m]
        si[K["DWS_ST_NR"], m] = 0
        si[K["DWS_ST_PERT"], m] = pert[m]
        si[K["DWS_ST_OFF"], m] = np.where(pert[m] != 0, 0, NEVER)
        for k, v in (("X0", root[:, 0]), ("Y0", root[:, 1]), ("XL", root[:, 0]), ("YL", root[:, 1]), ("TV0", tv0)):
            sf[K["DWS_ST_" + k], m] = v[m]
        for k in ("VERR", "PKL", "PKR", "DTM"):
            sf[K["DWS_ST_" + k], m] = 0.0
        sf[K["DWS_ST_TAU"]:K["DWS_ST_TAU"] + 12, m] = 0.0

    def restart(self, root, es, progress, ids=None):
        m = np.zeros(self.n, bool)
        if ids is None:
            m[:] = True
        else:
            m[np.asarray(ids)] = True
        pert = (es_int(es, E["DW_ES_PERT_ON"]) != 0).astype(np.int32)
        self._begin(m, np.asarray(progress, np.int64).astype(np.int32), root, es[:, E["DW_ES_TARGET_VEL"]], pert, es_int(es, E["DW_ES_NAN_RESETS"]))

    def record(self, root, cf, es, reset, mass, over=None):
        """One step's buffers (numpy: root [n,13], cf [n,38,3], es [n,DW_ES_WORDS] float32, reset [n], mass [n]) -> cause [n] uint8.  `over`:
        [n, 38] bools to use instead of over_1n(cf)."""
        si, sf, ac, ct = self.si, self.sf, self.ac, self.ct
        g = lambda k: K["DWS_" + k]                                                  # noqa: E731
        reset = np.asarray(reset) != 0
        nr_ = ~reset
        tv0, tv1 = es[:, E["DW_ES_TARGET_VEL"]], es[:, E["DW_ES_TARGET_VEL"] + 1]
        tf0, tf1 = es[:, E["DW_ES_TARGET_FORCE"]], es[:, E["DW_ES_TARGET_FORCE"] + 1]
        tq = es[:, E["DW_ES_ACTION_TORQUE"]:E["DW_ES_ACTION_TORQUE"] + 12]
        pert = (es_int(es, E["DW_ES_PERT_ON"]) != 0).astype(np.int32)
        nanr = es_int(es, E["DW_ES_NAN_RESETS"])
        lr = es[:, E["DW_ES_LAST_RETURN"]]
        fl, fr = cf[:, LF, 2], cf[:, RF, 2]
        pkl, pkr = np.fmax(sf[g("ST_PKL")], fl), np.fmax(sf[g("ST_PKR")], fr)
        ws = mass.astype(np.float32) / f32(104.48)
        ac[g("AC_FT")] += np.abs(fl + ws * tf0)
        ac[g("AC_FT") + 1] += np.abs(fr + ws * tf1)
        tau = np.zeros(self.n, np.float32)
        for j in range(12):
            tau = tau + np.abs(tq[:, j])
        ac[g("AC_TAU")] += tau
        # |tau_t - tau_t-1| against the previous record's action_torque of the same episode (terminal step included)
        dtm = sf[g("ST_DTM")].copy()
        prev = sf[g("ST_TAU"):g("ST_TAU") + 12]
        for j in range(12):
            dtm = np.fmax(dtm, np.abs(tq[:, j] - prev[j]))
        dtm = np.where(si[g("ST_NR")] > 0, dtm, sf[g("ST_DTM")])
        sf[g("ST_DTM")] = dtm
        n_ = si[g("ST_N")] + 1
        # ---- envs that did not reset ----
        dx, dy = tv0 - root[:, 7], tv1 - root[:, 8]
        verr = np.sqrt(dx * dx + dy * dy)
        ct[g("CT_PUSHES")] += int((nr_ & (pert != 0) & (si[g("ST_PERT")] == 0)).sum())
        off = np.where(pert != 0, 0, np.where(si[g("ST_OFF")] >= NEVER, NEVER, si[g("ST_OFF")] + 1))
        m = nr_
        old = dict(off=si[g("ST_OFF")].copy(), nr=si[g("ST_NR")].copy(), nan=si[g("ST_NAN")].copy(), tv=sf[g("ST_TV0")].copy(),
                   verr=sf[g("ST_VERR")].copy(), x0=sf[g("ST_X0")].copy(), y0=sf[g("ST_Y0")].copy(), xl=sf[g("ST_XL")].copy(),
                   yl=sf[g("ST_YL")].copy(), dtm=sf[g("ST_DTM")].copy())
        sf[g("ST_TAU"):g("ST_TAU") + 12, m] = tq[m].T
        sf[g("ST_VERR"), m] = (sf[g("ST_VERR")] + verr)[m]
        si[g("ST_NR"), m] += 1
        sf[g("ST_XL"), m] = root[m, 0]
        sf[g("ST_YL"), m] = root[m, 1]
        si[g("ST_OFF"), m] = off[m]
        si[g("ST_PERT"), m] = pert[m]
        si[g("ST_N"), m] = n_[m]
        si[g("ST_NAN"), m] = nanr[m]
        sf[g("ST_PKL"), m] = pkl[m]
        sf[g("ST_PKR"), m] = pkr[m]
        # ---- envs that reset ----
        r = reset
        ov = over_1n(cf) if over is None else np.asarray(over, bool)
        cause = np.where(nanr > old["nan"], 4, np.where(ov.any(1), 2, np.where(n_.astype(np.float32) >= self.ml - f32(1), 1, 3)))
        cause = np.where(r, cause, 0).astype(np.uint8)
        ct[g("CT_EPISODES")] += int(r.sum())
        for c in range(1, 5):
            ct[g("CT_CAUSE") + c] += int((cause == c).sum())
        ct[g("CT_LEN_SUM")] += int(n_[r].sum())
        if r.any():
            ct[g("CT_LEN_MAX")] = max(int(ct[g("CT_LEN_MAX")]), int(n_[r].max()))
        hb = np.clip((n_.astype(np.float32) * f32(K["DWS_LEN_BINS"]) / self.ml).astype(np.int64), 0, K["DWS_LEN_BINS"] - 1)
        ct[g("CT_LEN_HIST"):g("CT_LEN_HIST") + K["DWS_LEN_BINS"]] += np.bincount(hb[r], minlength=K["DWS_LEN_BINS"])
        ct[g("CT_BODY"):g("CT_BODY") + ov.shape[1]] += ov[cause == 2].sum(0)
        idx = np.nonzero(r)[0]
        ac[g("AC_RET"), idx] += lr[idx]
        b = np.clip((old["tv"] / f32(0.2)).astype(np.int64), 0, 3)
        ct[g("CT_BIN_EP"):g("CT_BIN_EP") + 4] += np.bincount(b[r], minlength=4)
        rr = r & (old["nr"] > 0)
        ct[g("CT_BIN_ROOT"):g("CT_BIN_ROOT") + 4] += np.bincount(b[rr], minlength=4)
        i2 = np.nonzero(rr)[0]
        ac[g("AC_VERR") + b[i2], i2] += old["verr"][i2] / old["nr"][i2].astype(np.float32)
        ac[g("AC_DRIFT") + b[i2], i2] += np.abs(old["yl"][i2] - old["y0"][i2])
        dist = old["tv"] * (old["nr"].astype(np.float32) * self.dtp)
        rq = rr & (dist >= f32(0.05))          # (DWS_RATIO_MIN_M)
        ct[g("CT_BIN_RATIO"):g("CT_BIN_RATIO") + 4] += np.bincount(b[rq], minlength=4)
        i3 = np.nonzero(rq)[0]
        ac[g("AC_RATIO") + b[i3], i3] += (old["xl"][i3] - old["x0"][i3]) / dist[i3]
        ac[g("AC_PK"), idx] += pkl[idx]
        ac[g("AC_PK") + 1, idx] += pkr[idx]
        ct[g("CT_PK_OVER")] += int((r & (pkl > f32(1400))).sum())
        ct[g("CT_PK_OVER") + 1] += int((r & (pkr > f32(1400))).sum())
        ac[g("AC_DTM"), idx] += old["dtm"][idx]
        ct[g("CT_PUSH_FALLS")] += int((r & (cause != 1) & (old["off"] + 1 <= K["DWS_PUSH_WINDOW"])).sum())
        self._begin(r, np.zeros(self.n, np.int32), root, tv0, pert, nanr)
        # ---- once per record ----
        s0 = int(es_int(es, E["DW_ES_PERT_START"])[0])
        if s0 and ct[g("CT_GATE_AT")] == 0:
            ct[g("CT_GATE_AT")] = ct[g("CT_CALLS")] + 1
        ct[g("CT_CALLS")] += 1
        ct[g("CT_RECORDS")] += 1
        return cause

    def reset_totals(self):
        self.ac[:] = 0
        self.ct[:K["DWS_CT_WINDOW"]] = 0

    def raw(self):
        return np.concatenate([self.ct.astype(np.float64), self.ac.astype(np.float64).sum(1)])


def compare_raw(got, want, rtol=1e-6):
    """Integer counts exact, float sums to rtol (relative to the larger of the value and 1e-3)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nct = K["DWS_CT_WORDS"]
    bad = np.nonzero(got[:nct] != want[:nct])[0]
    assert bad.size == 0, {int(i): (got[i], want[i]) for i in bad}
    a, b = got[nct:], want[nct:]
    err = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
    assert (err <= rtol).all(), {int(i): (a[i], b[i]) for i in np.nonzero(err > rtol)[0]}
