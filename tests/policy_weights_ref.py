"""Float64 statement of the sample-weighted policy update -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

One sentence defines it: a sample of weight w behaves as w copies of itself.  Every mean over the batch of
``oracle.refupdate.PolicyGraph`` and of ``tests/ppo_lag_ref.Surrogate`` becomes sum(w x) / sum(w); nothing else changes
(entropy has no per-sample part).  ``trust_weights`` restates the formula and the order of ``cmbpo_buffer_trust_weights``.
"""
import numpy as np
import torch

from oracle import refupdate

import ppo_lag_ref as ref

F64 = torch.float64
EPS = refupdate.EPS


class WeightedPolicyGraph(refupdate.PolicyGraph):
    def __init__(self, obs_dim, act_dim, batch, weights, dtype=F64, **kw):
        super().__init__(obs_dim, act_dim, batch, dtype=dtype, **kw)
        self.w = torch.as_tensor(np.asarray(weights, np.float64), dtype=dtype)
        self.W = self.w.sum()

    def _wmean(self, x):
        return (self.w * x).sum() / self.W

    def d_kl(self, p):
        mu, ls = self._mu(p)
        var0, var1 = torch.exp(2 * ls), torch.exp(2 * self.b["log_std_old"])
        pre = 0.5 * (((self.b["mu_old"] - mu) ** 2 + var0) / (var1 + EPS) - 1) + self.b["log_std_old"] - ls
        return self._wmean(pre.sum(dim=1))

    def surr(self, p):
        ratio = torch.exp(self.logp(p) - self.b["logp_old"])
        return self._wmean(ratio * self.b["adv"]), self._wmean(ratio * self.b["cadv"])

    def cur_cret_avg(self):
        return self._wmean(self.b["cost"]) * self.T

    def fisher_vp(self, flat, v, damping=0.1):
        p = self._param(flat)
        vv = torch.as_tensor(np.asarray(v), dtype=self.dtype)
        mu, ls = self._mu(p)
        var1 = torch.exp(2 * self.b["log_std_old"]) + EPS
        _, jv = torch.autograd.functional.jvp(lambda q: self._mu(q)[0], (p.detach(),), (vv,))
        out, = torch.autograd.grad(mu, p, grad_outputs=self.w[:, None] * jv / var1 / self.W)
        coef = (self.w[:, None] * (2 * torch.exp(2 * ls.detach()) / var1)).sum(dim=0) / self.W
        out = out.clone()
        out[-self.A:] += coef * vv[-self.A:]
        return (out + damping * vv).numpy()


class WeightedSurrogate(ref.Surrogate):
    """``Surrogate`` on a WeightedPolicyGraph: weighted means, and the eight loss sums as the kernels define them
    ({sum w, sum w obj, sum w ratio cadv, sum w kl, sum w cost, sum w [clipped away], sum w ratio adv, 0})."""

    def pi_loss(self, p, penalty):
        ratio, obj, _ = self.terms(p)
        o = self.g._wmean(obj) + self.g.ent_reg * self.g.ent(p)
        if self.objective_penalized:
            o = (o - penalty * self.g._wmean(ratio * self.g.b["cadv"])) / (1 + penalty)
        return -o

    def sums(self, flat):
        with torch.no_grad():
            p = torch.as_tensor(np.asarray(flat, np.float64), dtype=F64)
            b, w = self.g.b, self.g.w
            ratio, obj, active = self.terms(p)
            W = float(self.g.W)
            return np.array([W, float((w * obj).sum()), float((w * ratio * b["cadv"]).sum()), float(self.g.d_kl(p)) * W,
                             float((w * b["cost"]).sum()), float((w * (~active)).sum()), float((w * ratio * b["adv"]).sum()),
                             0.0])


def replicate(batch, counts):
    """The batch with row i repeated counts[i] times (0: dropped), rows in order."""
    idx = np.repeat(np.arange(len(counts)), np.asarray(counts, np.int64))
    return {k: np.asarray(v)[idx] for k, v in batch.items()}, idx


def trust_weights(cumvar, lens, ref_var):
    """cumvar [T, B] float64, lens [B]: the weights in the order of ModelBuffer.get() -- branch-major, time-minor, entries
    t < lens[b] only -- as float32 stores of the float64 quotient ref_var / (ref_var + cumvar)."""
    out = []
    for b, L in enumerate(np.asarray(lens)):
        out.append((np.float64(ref_var) / (np.float64(ref_var) + np.asarray(cumvar, np.float64)[:L, b])).astype(np.float32))
    return np.concatenate(out) if out else np.zeros(0, np.float32)
