"""numpy restatements of the episode-return meter (include/dyros_meter.h): MeterRef in float32 in the documented summation order (what the
g++ build and the HIP kernel must give bit for bit), step64() in float64 (what the sums would be without rounding), and Synth, the rewards
and dones the tests feed them."""
import numpy as np

from isaacgymdyros_amd import cbind

K = cbind.constants("dyros_meter.h", "dwm_")
GROUP, WAVE, HEAD, CMAX = K["DWM_GROUP"], 64, K["DWM_WORK_HEAD"], K["DWM_COLS_MAX"]
F = np.float32


def groups(n):
    return (n + GROUP - 1) // GROUP


def work_words(n, cols):
    return HEAD + groups(n) * (cols + 3)


def tree_depth():
    """float additions on the longest path from one env's term to its workgroup's partial sum: 6 butterfly levels and 3 wavefront adds"""
    return 6 + 3


def group_sums(x):
    """x [G * GROUP] float32 -> [G]: the xor butterfly inside every wavefront, then ((w0 + w1) + w2) + w3."""
    t = x.reshape(-1, GROUP // WAVE, WAVE).copy()
    h = WAVE // 2
    while h >= 1:
        t = t[..., :h] + t[..., h:2 * h]          # (lane l meets lane l ^ h: for l < h that is l + h)
        h //= 2
    w = t[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


class MeterRef:
    def __init__(self, n, cols, max_size):
        self.n, self.cols, self.max_size = n, cols, max_size
        self.cur = np.zeros((cols + 1, n), F)
        self.ms = np.zeros(K["DWM_MS_WORDS"], np.uint32)
        self.work = np.zeros(work_words(n, cols), np.uint32)

    # views of ms
    def _f(self):
        return self.ms.view(F)

    def record(self, rew, stacked, done):
        n, C = self.n, self.cols
        inc = np.ones((C + 1, n), F)
        inc[0] = rew
        if C > 1:
            inc[1:C] = stacked[:, :C - 1].T
        with np.errstate(all="ignore"):
            v = self.cur + inc
        dn = done != 0
        fin = np.isfinite(v[:C]).all(axis=0)
        in_d = dn & fin
        self.cur = np.where(dn[None, :], F(0), v).astype(F)
        g = groups(n)
        pad = np.zeros((C + 1, g * GROUP), F)
        pad[:, :n] = np.where(in_d[None, :], v, F(0))
        rows = np.zeros((g, C + 3), np.uint32)
        with np.errstate(all="ignore"):
            for c in range(C + 1):
                rows[:, c] = group_sums(pad[c]).view(np.uint32)
        ind = np.zeros(g * GROUP, bool); ind[:n] = in_d
        bad = np.zeros(g * GROUP, bool); bad[:n] = dn & ~fin
        rows[:, C + 1] = ind.reshape(g, GROUP).sum(1)
        rows[:, C + 2] = bad.reshape(g, GROUP).sum(1)
        self.work[HEAD:] = rows.reshape(-1)
        # the finishing workgroup
        acc, dacc = np.zeros(C + 1, F), np.zeros(C + 1, np.float64)
        with np.errstate(all="ignore"):
            for b in range(g):
                x = rows[b, :C + 1].view(F)
                acc = acc + x
                dacc = dacc + x.astype(np.float64)
        k, nbad = int(rows[:, C + 1].sum()), int(rows[:, C + 2].sum())
        f = self._f()
        cs = int(self.ms[K["DWM_MS_CURRENT_SIZE"]])
        if k > 0:
            size = min(k, self.max_size)
            old = min(self.max_size - size, cs)
            at = list(range(K["DWM_MS_MEAN"], K["DWM_MS_MEAN"] + C)) + [K["DWM_MS_MEAN_LEN"]]
            with np.errstate(all="ignore"):
                new_mean = acc / F(k)
                f[at] = (f[at] * F(old) + new_mean * F(size)) / F(old + size)
            self.ms[K["DWM_MS_CURRENT_SIZE"]] = old + size
            d = self.ms.view(np.float64)
            d[K["DWM_MS_SUM_RET"] // 2] += dacc[0]
            d[K["DWM_MS_SUM_LEN"] // 2] += dacc[C]
            self.ms.view(np.uint64)[K["DWM_MS_GAMES"] // 2] += np.uint64(k)
        if nbad:
            self.ms.view(np.uint64)[K["DWM_MS_DISCARDED"] // 2] += np.uint64(nbad)
        self.work[0] = 0
        return k

    def clear(self):
        self.ms[:] = 0
        self.work[:HEAD] = 0


def unpack(ms, cols):
    """The fields of an ms array (numpy uint32 [DWM_MS_WORDS])."""
    f = ms.view(F)
    return {"current_size": int(ms[K["DWM_MS_CURRENT_SIZE"]]), "mean": f[K["DWM_MS_MEAN"]:K["DWM_MS_MEAN"] + cols].copy(),
            "mean_len": float(f[K["DWM_MS_MEAN_LEN"]]), "games": int(ms.view(np.uint64)[K["DWM_MS_GAMES"] // 2]),
            "discarded": int(ms.view(np.uint64)[K["DWM_MS_DISCARDED"] // 2]), "sum_ret": float(ms.view(np.float64)[K["DWM_MS_SUM_RET"] // 2]),
            "sum_len": float(ms.view(np.float64)[K["DWM_MS_SUM_LEN"] // 2])}


def step64(cur_before, rew, stacked, done, cols, max_size, mean_before, size_before):
    """One record in float64 from the float32 state before it: (k, means [C + 1] float64, mean |x| per column over D).  The per-env sums
    cur + inc are taken in float32, as stored (they are the meter's inputs x); everything after is float64."""
    n = rew.shape[0]
    inc = np.ones((cols + 1, n), F)
    inc[0] = rew
    if cols > 1:
        inc[1:cols] = stacked[:, :cols - 1].T
    with np.errstate(all="ignore"):
        v = cur_before + inc
    in_d = (done != 0) & np.isfinite(v[:cols]).all(axis=0)
    k = int(in_d.sum())
    if k == 0:
        return 0, np.asarray(mean_before, np.float64), np.zeros(cols + 1)
    x = v[:, in_d].astype(np.float64)
    new_mean = x.sum(axis=1) / k
    size = min(k, max_size)
    old = min(max_size - size, size_before)
    return k, (np.asarray(mean_before, np.float64) * old + new_mean * size) / (old + size), np.abs(x).mean(axis=1)


class Synth:
    """Rewards of mixed sign, term columns of mixed sign and scale, dones with probability p."""

    def __init__(self, n, seed, p=0.02):
        self.n, self.p, self.rng = n, p, np.random.default_rng(seed)
        self.scale = (10.0 ** self.rng.uniform(-2, 1, 15)).astype(F) * np.where(self.rng.random(15) < 0.5, -1, 1).astype(F)

    def step(self, force=None):
        r = self.rng
        rew = r.normal(0.3, 1.0, self.n).astype(F)
        stacked = (r.normal(0.2, 1.0, (self.n, 15)).astype(F) * self.scale[None, :]).astype(F)
        if force is None:
            done = (r.random(self.n) < self.p).astype(np.int64)
        else:
            done = np.full(self.n, 1 if force else 0, np.int64)
        done[done != 0] = r.integers(1, 5, int((done != 0).sum()))          # (any non-zero value is done)
        return rew, np.ascontiguousarray(stacked), done
