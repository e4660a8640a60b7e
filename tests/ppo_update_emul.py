"""A CPU stand-in for isaacgymdyros_amd.ppo_update.FusedPpoUpdate with the buffers and state words tests/test_ppo_edges_gpu.py reads: the
same update in torch on the CPU -- fp16 operands, fp32 sums, one rounding per stage (two in the library-GEMM form's layers), partial weight
gradients per slab of dwp_wgrad, Adam and the scaler from tests/ppo_update_truth.py.  It lets the GPU tests' checking code run without a
GPU (tests/test_ppo_update_truth.py: it must pass this update and reject the same update with a fault put in), and shows which samples come
near the clip boundary over a case's four updates.  `fault`: None, or one of FAULTS."""
import math

import torch

import ppo_update_truth as T

FAULTS = ("dropped_k_block", "empty_slab_not_cleared", "bucket_not_cleared", "dz1_not_masked", "actor_stepped_twice")
LAYOUT = (("W1", (2, T.HID, T.INP)), ("W2", (2, T.HID, T.HID)), ("W3", (2, T.OUTP, T.HID)), ("b1", (2, T.HID)), ("b2", (2, T.HID)), ("b3", (2, T.OUTP)))


class EmulatedUpdate:
    def __init__(self, net, cfg, B, batch, scale, lrs, mfma=True, fault=None):
        self.B, self.mfma, self.rowmajor, self.batch, self.net, self.cfg, self.lrs, self.fault = B, bool(mfma) and B % 32 == 0, True, batch, net, cfg, lrs, fault
        self.K = T.K
        self.p, self.m, self.v = torch.zeros(T.NP), torch.zeros(T.NP), torch.zeros(T.NP)
        self.views, self._gshape, o = {}, {}, 0
        for name, shape in LAYOUT:
            n = math.prod(shape)
            self.views[name] = self.p[o:o + n].view(shape)
            if name[0] == "W":
                self._gshape[name] = (o, n, shape)
            o += n
        with torch.no_grad():
            for k, (tr, hd, rows) in enumerate(((net.actor_mlp, net.mu, T.ACT), (net.critic_mlp, net.value, 1))):
                self.views["W1"][k, :, :T.IN], self.views["b1"][k], self.views["W2"][k], self.views["b2"][k] = tr[0].weight, tr[0].bias, tr[2].weight, tr[2].bias
                self.views["W3"][k, :rows], self.views["b3"][k, :rows] = hd.weight, hd.bias
        self.p16 = self.p.half()
        self.state = torch.zeros(T.K["DWP_S_WORDS"])
        self.state[T.K["DWP_S_SCALE"]] = scale
        self.pbuf = torch.zeros(T.PBUF_BUCKETS, 2, T.K["DWP_PBUF_WORDS"])
        self.g32, self.g16, self.gb = torch.zeros(T.WG_SLABS, T.NWT), torch.zeros(T.NWT).half(), torch.zeros(T.NB1 + T.NB2 + T.NB3)
        self.L = None

    @property
    def views16(self):
        d, o = {}, 0
        for name, shape in LAYOUT:
            n = math.prod(shape)
            d[name] = self.p16[o:o + n].view(shape)
            o += n
        return d

    @property
    def gviews(self):
        g = self.g16 if not self.mfma else self.g32.sum(0)
        return {name: g[o:o + n].view(shape) for name, (o, n, shape) in self._gshape.items()}

    def logged(self):
        return self.state[T.K["DWP_S_OUT"]:T.K["DWP_S_OUT"] + 8]

    def update(self):
        K, B, c = T.K, self.B, self.cfg
        st = self.state
        mb, scale = int(st[K["DWP_S_MB"]]), float(st[K["DWP_S_SCALE"]])
        obs, act, nlp_old, mu_old, adv, ret = (t[mb * B:(mb + 1) * B] for t in self.batch)
        W = {k: v.float() for k, v in self.views16.items()}

        def layer(a, w, b):          # (the library-GEMM form rounds the bare product first)
            y = a @ w.transpose(1, 2)
            return ((y if self.mfma else y.half().float()) + b.unsqueeze(1)).half()
        self.x16 = torch.zeros(B, T.INP).half()
        self.x16[:, :T.IN] = obs.half()
        x = self.x16.float()
        self.h1 = torch.relu(layer(x, W["W1"], W["b1"]))
        self.h2 = torch.relu(layer(self.h1.float(), W["W2"], W["b2"]))
        self.out = layer(self.h2.float(), W["W3"], W["b3"])
        self.L = L = T.loss(self.out, act, nlp_old, mu_old, adv, ret, self.net.sigma, scale, c["e_clip"], c["critic_coef"])
        self.dout = T.dout_of(L).half()
        self.dh2 = (self.dout.float() @ W["W3"]).half() * (self.h2 > 0)
        self.dh1 = (self.dh2.float() @ W["W2"]).half()
        if self.fault != "dz1_not_masked":
            self.dh1 = self.dh1 * (self.h1 > 0)
        x2 = x.unsqueeze(0).expand(2, B, T.INP)
        table = T.wgrad_slabs(B // 32) if self.mfma else None
        if self.fault == "dropped_k_block":
            table = [(a, b - 1) if b > a else (a, b) for a, b in table]
        for name, dz, a in (("W1", self.dh1, x2), ("W2", self.dh2, self.h1.float()), ("W3", self.dout, self.h2.float())):
            o, n, _ = self._gshape[name]
            if self.mfma:
                for i, r in enumerate(T.slab_rows(B, table)):
                    self.g32[i, o:o + n] = (dz[:, r].float().transpose(1, 2) @ a[:, r]).reshape(-1)
                    if self.fault == "empty_slab_not_cleared" and r.stop == r.start:
                        self.g32[i, o + 5] = 1e-3
            else:
                self.g16[o:o + n] = (dz.float().transpose(1, 2) @ a).half().reshape(-1)
        self.gb = torch.cat([d.float().sum(1).reshape(-1) for d in (self.dh1, self.dh2, self.dout)])
        g = torch.cat([self.g32.sum(0) if self.mfma else self.g16.float(), self.gb])
        steps = [int(st[K["DWP_S_STEP"]]), int(st[K["DWP_S_STEP"] + 1])]
        R = T.clip_adam(g, scale, self.p, self.m, self.v, steps, self.lrs, c["grad_norm"])
        self.p.copy_(R["p"].float())
        self.m, self.v, self.p16 = R["m"].float(), R["v"].float(), self.p.half()
        if not self.mfma:
            self.gb = torch.zeros_like(self.gb)          # (dwp_finish clears it)
        if self.fault == "bucket_not_cleared":
            self.pbuf[7, 1, 300] = 1e-6
        o = K["DWP_S_OUT"]
        st[o:o + 5] = torch.tensor([float(L[k]) for k in ("a_loss", "c_loss", "b_loss", "clip_frac", "kl")])
        st[o + 5], st[o + 6], st[o + 7] = R["norm"], scale, float(any(R["found"]))
        new_scale, growth = T.scaler_update(scale, int(st[K["DWP_S_GROWTH"]]), any(R["found"]))
        st[K["DWP_S_SCALE"]], st[K["DWP_S_GROWTH"]] = new_scale, growth
        st[K["DWP_S_STEP"]], st[K["DWP_S_STEP"] + 1] = R["steps"][0] + (self.fault == "actor_stepped_twice"), R["steps"][1]
        st[K["DWP_S_MB"]] = (mb + 1) % T.NMB
