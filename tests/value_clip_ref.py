"""Restatement of the clipped / sample-weighted value loss of the reference's deterministic ensembles
(``_nll_loss(inc_var_loss=False, weights=, oldpred_v=)``, models/pens/pe.py:866-868,881-905,917) in torch autograd --
TEST INFRASTRUCTURE, the checker of tests/test_value_clip_*.py.  TensorFlow cannot run here, so, as for all of training
(oracle/reftrain.py), the restatement is the reference; its analytic cross-checks are tests/test_value_clip_cpu.py.

With t' the scaled target, m the raw network output, w the sample weight (1 without weights):

    old'    = (old_pred - mu) / sigma           with the output scaler on (the same transform as the targets), else old_pred
    old_var = mean over ALL members, rows, outputs of 0.5 (old' - t')^2
    c       = sqrt(2) sqrt(kl old_var)
    m_c     = old' + clamp(m - old', -c, c)
    loss_e  = mean_b w mean_d 0.5 (m_c - t')^2                      (the mean divides by the batch, not by sum w)

One deliberate deviation from the reference's text: pe.py:879 scales the targets and :890-893 then subtract them from the
UNSCALED old predictions; here both sides of every difference are in the scaled unit.  With the scaler off the two agree.
"""
import numpy as np
import torch

from oracle.reftrain import AdamTF, forward_raw, scale_targets


def clip_range(old_s, t_s, kl):
    """c of one step (a 0-d tensor of the inputs' dtype): pe.py:890-893."""
    old_var = (0.5 * (old_s - t_s) ** 2).mean()
    root2 = torch.sqrt(torch.tensor(2.0, dtype=old_s.dtype))
    return root2 * torch.sqrt(torch.tensor(kl, dtype=old_s.dtype) * old_var)


def clipped_mean(m, old_s, c):
    return old_s + torch.clamp(m - old_s, -c, c)


def value_losses(o, t_s, w=None, old_s=None, kl=None):
    """Per-member losses [E] of raw outputs o [E,B,D] against scaled targets; w [E,B]; old_s [E,B,D] scaled."""
    m = o if old_s is None else clipped_mean(o, old_s, clip_range(old_s, t_s, kl).detach())
    per_row = (0.5 * (m - t_s) ** 2).mean(dim=-1)
    if w is not None:
        per_row = w * per_row
    return per_row.mean(dim=-1)


def closed_form_delta(o, t_s, w=None, old_s=None, kl=None):
    """d(sum_e loss_e) / d o: w (m_c - t') / (B D) inside the clip range (boundary included, tf.clip_by_value), 0 outside."""
    B, D = o.shape[1], o.shape[2]
    if old_s is None:
        d = o - t_s
    else:
        c = clip_range(old_s, t_s, kl)
        dm = o - old_s
        d = torch.where((dm >= -c) & (dm <= c), clipped_mean(o, old_s, c) - t_s, torch.zeros_like(o))
    if w is not None:
        d = w[..., None] * d
    return d / (B * D)


def boundary_margin(o, old_s, c):
    """| |m - old'| / c - 1 | per element: how far (in units of c) an element is from switching sides."""
    return (torch.abs(o - old_s) / c - 1.0).abs()


class ValueTrainer:
    """One optimisation state of a deterministic ensemble under the clipped / weighted loss; the interface of
    oracle.reftrain.EnsembleTrainer with the extra feeds."""

    def __init__(self, ws, bs, decays, lr=1e-3, dtype=torch.float32):
        self.dtype = dtype
        self.ws = [torch.tensor(np.asarray(w), dtype=dtype) for w in ws]
        self.bs = [torch.tensor(np.asarray(b), dtype=dtype).reshape(w.shape[0], 1, w.shape[2]) for b, w in zip(bs, ws)]
        self.decays = decays
        self.opt = AdamTF(self.ws + self.bs, lr=lr)
        self.scaler_in = self.scaler_out = None

    def set_scalers(self, scaler_in, scaler_out):
        t = lambda a: torch.tensor(np.asarray(a), dtype=self.dtype).reshape(-1)
        self.scaler_in = None if scaler_in is None else (t(scaler_in[0]), t(scaler_in[1]))
        self.scaler_out = None if scaler_out is None else (t(scaler_out[0]), t(scaler_out[1]))

    def _t(self, a):
        return None if a is None else torch.as_tensor(np.asarray(a), dtype=self.dtype)

    def outputs(self, x, ws=None, bs=None):
        return forward_raw(self._t(x), self.ws if ws is None else ws, self.bs if bs is None else bs, self.scaler_in)

    def scaled(self, t):
        return scale_targets(self._t(t), self.scaler_out)

    def train_loss(self, ps, x, t, w=None, old=None, kl=None):
        n = len(self.ws)
        o = self.outputs(x, ps[:n], ps[n:])
        loss = value_losses(o, self.scaled(t), self._t(w), None if old is None else self.scaled(old), kl).sum()
        for p, d in zip(ps[:n], self.decays):
            loss = loss + d * 0.5 * (p ** 2).sum()
        return loss

    def grads(self, x, t, w=None, old=None, kl=None):
        ps = [p.clone().requires_grad_(True) for p in self.ws + self.bs]
        loss = self.train_loss(ps, x, t, w, old, kl)
        return float(loss.detach()), torch.autograd.grad(loss, ps)

    def step(self, x, t, w=None, old=None, kl=None):
        loss, gs = self.grads(x, t, w, old, kl)
        new = self.opt.step(self.ws + self.bs, list(gs))
        n = len(self.ws)
        self.ws, self.bs = new[:n], new[n:]
        return loss

    def losses(self, x, t, w=None):
        """`self.loss`: weighted, never clipped."""
        with torch.no_grad():
            return value_losses(self.outputs(x), self.scaled(t), self._t(w)).numpy()

    def clip_state(self, x, t, old, kl):
        """(c, clipped share, smallest boundary margin) of one batch on the current weights."""
        with torch.no_grad():
            o, ts, os_ = self.outputs(x), self.scaled(t), self.scaled(old)
            c = clip_range(os_, ts, kl)
            share = float((torch.abs(o - os_) > c).double().mean())
            return float(c), share, float(boundary_margin(o, os_, c).min())
