"""A numpy restatement of TocabiAMPLower's episode statistics (include/dyros_amp_stats.h, isaacgymdyros_amd/csrc/dw_amp_stats.h), vectorised
over envs, in float32 where the kernels are.  Used by tests/test_amp_episode_stats.py (against the g++ build) and
tests/test_amp_episode_stats_gpu.py (against the HIP kernels and the step's own flags)."""
from __future__ import annotations

import numpy as np

from isaacgymdyros_amd.amp_episode_stats import K

f32 = np.float32
LF, RF, NB = K["DWE_LFOOT"], K["DWE_RFOOT"], K["DWE_BODIES"]
TILT = f32(3.141592 / 4.0)


def over_1(cf):
    """[n, 38] bool: a component > 1, the soles excluded."""
    o = (cf > f32(1.0)).any(-1)
    o[:, LF] = False
    o[:, RF] = False
    return o


def quat_err(q):
    """|quat_diff_rad| against the identity, float32 (dw::quat_err: the quaternion product written out, the norm of its vector part in
    torch's CPU order for three elements, asin clamped at 1)."""
    q = q.astype(f32)
    x2, y2, z2, w2 = -q[:, 0], -q[:, 1], -q[:, 2], q[:, 3]
    o, z = f32(1.0), f32(0.0)
    ww = (z + z) * (x2 + y2)
    yy = (o - z) * (w2 + z2)
    zz = (o + z) * (w2 - z2)
    xx = ww + yy + zz
    qq = f32(0.5) * (xx + (z - z) * (x2 - y2))
    x = qq - xx + (z + o) * (x2 + w2)
    y = qq - yy + (o - z) * (y2 + z2)
    zc = qq - zz + (z + z) * (w2 - x2)
    # three elements: no 8-lane block, no 4-wide chunk, a fused scalar tail (dw::norm_fn); the products are exact in float64
    b = np.zeros(len(q), f32)
    for c in (x, y, zc):
        b = (c.astype(np.float64) * c.astype(np.float64) + b.astype(np.float64)).astype(f32)
    n = np.minimum(np.sqrt(b), f32(1.0))
    return np.abs(f32(2.0) * np.arcsin(n.astype(f32)))


def quat_rotate_inverse_x(q, v):
    """Component 0 of dwa::quat_rotate_inverse, float32 in its order (the cross product's first product contracted into the subtraction)."""
    q, v = q.astype(f32), v.astype(f32)
    w = q[:, 3]
    s = f32(2.0) * (w * w) - f32(1.0)
    t = (q[:, 2] * v[:, 1]).astype(f32)
    cr = (q[:, 1].astype(np.float64) * v[:, 2].astype(np.float64) - t.astype(np.float64)).astype(f32)          # fmaf(q1, v2, -(q2 v1))
    dot = (q[:, 0] * v[:, 0] + q[:, 1] * v[:, 1]) + q[:, 2] * v[:, 2]
    a = v[:, 0] * s
    b = cr * w * f32(2.0)
    c = q[:, 0] * dot * f32(2.0)
    return a - b + c


def cause_mask(root, cf, rbp, progress, max_len, term_h, eet, over=None):
    """The step's termination test, one bit per term (the issue's rules; float32)."""
    p = np.asarray(progress, np.int64)
    m = np.where(p.astype(f32) >= f32(max_len) - f32(1.0), K["DWE_C_TIME"], 0)
    if eet:
        ov = over_1(cf) if over is None else over
        gate = p > 1
        with np.errstate(invalid="ignore"):
            m = m | np.where(gate & ov.any(1), K["DWE_C_CONTACT"], 0)
            m = m | np.where(gate & (root[:, 2] < f32(term_h)), K["DWE_C_LOW"], 0)
            m = m | np.where(gate & ((rbp[:, LF, 2] > f32(0.5)) | (rbp[:, RF, 2] > f32(0.5))), K["DWE_C_FLY"], 0)
            m = m | np.where(gate & (quat_err(root[:, 3:7]) > TILT), K["DWE_C_TILT"], 0)
    return m.astype(np.uint8)


class AmpStatsRef:
    def __init__(self, n, max_len, term_h, eet, cmd_lo, cmd_hi):
        self.n, self.ml, self.th, self.eet, self.lo, self.hi = n, f32(max_len), f32(term_h), bool(eet), f32(cmd_lo), f32(cmd_hi)
        self.st = np.zeros((K["DWE_ST_WORDS"], n), np.uint32)
        self.si, self.sf = self.st.view(np.int32), self.st.view(np.float32)
        self.ac = np.zeros((K["DWE_AC_WORDS"], n), np.float32)
        self.ct = np.zeros(K["DWE_CT_WORDS"], np.int64)
        self.restart()

    def restart(self, ids=None):
        if ids is None:
            self.si[K["DWE_ST_N"], :] = -1
        else:
            self.si[K["DWE_ST_N"], np.asarray(ids)] = -1

    def record(self, root, cf, rbp, cmd, rew, rv, reset, progress, mass):
        """One step's buffers (numpy float32: root [n,13], cf / rbp [n,38,3], cmd [n,3], rew [n], rv [n,9], mass [n]; reset, progress [n]) -> the
        cause masks [n] uint8."""
        si, sf, ac, ct = self.si, self.sf, self.ac, self.ct
        g = lambda k: K["DWE_" + k]                                                  # noqa: E731
        ar = np.arange(self.n)
        reset = np.asarray(reset) != 0
        p = np.asarray(progress, np.int64).astype(np.int32)
        mass = np.asarray(mass, f32).reshape(self.n)
        ov = over_1(cf)
        mask = cause_mask(root, cf, rbp, p, self.ml, self.th, self.eet, ov)
        n0, closed = si[g("ST_N")].copy(), si[g("ST_CLOSED")] != 0
        nxt = p == si[g("ST_PREV")] + 1
        unreset = closed & (n0 >= 0) & nxt                                    # 1.
        ct[g("CT_UNRESET")] += int(unreset.sum())
        live = ~unreset
        new = live & (closed | (n0 < 0) | ~nxt)                               # 2.
        ct[g("CT_DISCARDED")] += int((new & (n0 >= 0) & ~closed).sum())
        si[g("ST_N"), new] = 0
        si[g("ST_CLOSED"), new] = 0
        for w in ("ST_RET", "ST_PKL", "ST_PKR"):
            sf[g(w), new] = 0.0
        si[g("ST_PREV")] = p
        si[g("ST_N"), live] += 1                                              # 3.
        fin = np.isfinite(root).all(1)
        ct[g("CT_NONFINITE")] += int((live & ~fin).sum())
        sm = live & fin
        ct[g("CT_SAMPLES")] += int(sm.sum())
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            sf[g("ST_RET"), sm] = (sf[g("ST_RET")] + rew)[sm]
            for k in range(9):
                ac[g("AC_REW") + k, sm] = (ac[g("AC_REW") + k] + rv[:, k])[sm]
            lvx = quat_rotate_inverse_x(root[:, 3:7], root[:, 7:10])
            u = (cmd[:, 0] - self.lo) / (self.hi - self.lo) * f32(K["DWE_CMD_BINS"])
            b = np.where(~(u >= 0), 0, np.where(u >= K["DWE_CMD_BINS"], K["DWE_CMD_BINS"] - 1, np.nan_to_num(u).astype(np.int64).clip(0, 3)))
            ev = np.abs(cmd[:, 0] - lvx)
            i = ar[sm]
            ac[g("AC_VERR") + b[i], i] += ev[i]
            ac[g("AC_VCNT") + b[i], i] += f32(1.0)
            ac[g("AC_YAW"), sm] = (ac[g("AC_YAW")] + np.abs(cmd[:, 2] - root[:, 12]))[sm]
            w = f32(9.81) * mass
            sf[g("ST_PKL"), sm] = np.fmax(sf[g("ST_PKL")], cf[:, LF, 2] / w)[sm]
            sf[g("ST_PKR"), sm] = np.fmax(sf[g("ST_PKR")], cf[:, RF, 2] / w)[sm]
            thr = f32(1.4 * 9.81) * mass
            ct[g("CT_SOLE_OVER")] += int((sm & (cf[:, LF, 2] > thr)).sum())
            ct[g("CT_SOLE_OVER") + 1] += int((sm & (cf[:, RF, 2] > thr)).sum())
        r = live & reset                                                      # 4.
        si[g("ST_CLOSED"), r] = 1
        ct[g("CT_EPISODES")] += int(r.sum())
        ct[g("CT_MASK"):g("CT_MASK") + K["DWE_MASKS"]] += np.bincount(mask[r], minlength=K["DWE_MASKS"])
        ct[g("CT_LEN_SUM")] += int(p[r].sum())
        if r.any():
            ct[g("CT_LEN_MAX")] = max(int(ct[g("CT_LEN_MAX")]), int(p[r].max()))
        hb = np.clip((p.astype(f32) * f32(K["DWE_LEN_BINS"]) / self.ml).astype(np.int64), 0, K["DWE_LEN_BINS"] - 1)
        ct[g("CT_LEN_HIST"):g("CT_LEN_HIST") + K["DWE_LEN_BINS"]] += np.bincount(hb[r], minlength=K["DWE_LEN_BINS"])
        ct[g("CT_BODY"):g("CT_BODY") + NB] += ov[r & ((mask & K["DWE_C_CONTACT"]) != 0)].sum(0)
        ac[g("AC_RET"), r] += sf[g("ST_RET"), r]
        ac[g("AC_PK"), r] += sf[g("ST_PKL"), r]
        ac[g("AC_PK") + 1, r] += sf[g("ST_PKR"), r]
        ct[g("CT_CALLS")] += 1
        ct[g("CT_RECORDS")] += 1
        return mask

    def reset_totals(self):
        self.ac[:] = 0
        self.ct[:K["DWE_CT_WINDOW"]] = 0

    def raw(self):
        return np.concatenate([self.ct.astype(np.float64), self.ac.astype(np.float64).sum(1)])


def compare_raw(got, want, rtol=1e-6):
    """Integer counts exact, float sums to rtol (relative to the larger of the value and 1e-3)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nct = K["DWE_CT_WORDS"]
    bad = np.nonzero(got[:nct] != want[:nct])[0]
    assert bad.size == 0, {int(i): (got[i], want[i]) for i in bad}
    a, b = got[nct:], want[nct:]
    err = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
    assert (err <= rtol).all(), {int(i): (a[i], b[i]) for i in np.nonzero(err > rtol)[0]}
