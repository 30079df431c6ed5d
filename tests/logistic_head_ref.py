"""Float64 torch restatement of the probabilistic losses with logistic columns (the definition stands in
include/cmbpo_hip.h at cmbpo_trainer_set_column_kinds) -- TEST INFRASTRUCTURE, built on oracle/reftrain.py's forward_raw /
scale_targets, in the manner of tests/column_weights_ref.py.

For a logistic column d the raw mean output z is a logit and the raw float32 target gives y = (t > 0.5f) (a NaN target is 0);
neither passes through the output scaler.  The element's data term is w l, l = softplus(z) - y z; its log-variance output has no
data term ('MSPE' keeps the unweighted regulariser on it, 'NLL' nothing); 'MSPE''s ratio runs over the Gaussian columns only.
Gaussian columns keep column_weights_ref's formulas term for term."""
import numpy as np
import torch

import column_weights_ref as cw_ref
from oracle import reftrain

F64 = torch.float64


def kinds_mask(kinds, D):
    """bool tensor [D], True on logistic columns (None: none)."""
    k = np.zeros(D, bool) if kinds is None else np.asarray(kinds).astype(bool).reshape(D)
    return torch.as_tensor(k)


def labels(t_raw):
    """y of the targets' shape, float64: the comparison runs on float32 values and is written positively, as in the kernels."""
    t32 = np.asarray(t_raw, np.float32)
    return torch.as_tensor((t32 > np.float32(0.5)).astype(np.float64), dtype=F64)


def bernoulli_nll(z, y):
    """l = max(z, 0) - y z + log1p(exp(-|z|))."""
    return torch.clamp(z, min=0.0) - y * z + torch.log1p(torch.exp(-torch.abs(z)))


def sigmoid(z):
    ez = torch.exp(-torch.abs(z))
    return torch.where(z >= 0, 1.0 / (1.0 + ez), ez / (1.0 + ez))


def mspe_ratio(o, ts, w, km):
    D = o.shape[-1] // 2
    g = (~km).to(o.dtype)
    mse = (o[..., :D] - ts) ** 2
    var = torch.exp(o[..., D:])
    return (0.05 * (g * w * mse).sum() / (g * w * (var - mse) ** 2).sum()).detach()


def mspe_losses(o, ts, w, y, km):
    D = o.shape[-1] // 2
    mean, lv = o[..., :D], o[..., D:]
    mse = (mean - ts) ** 2
    var_logit = (torch.exp(lv) - mse.detach()) ** 2
    ratio = mspe_ratio(o.detach(), ts, w, km)
    data = torch.where(km, w * bernoulli_nll(mean, y), w * mse + ratio * w * var_logit)
    return data.mean(dim=(-1, -2)) + 0.05 * (lv ** 2).mean()


def nll_losses(o, ts, w, y, km):
    D = o.shape[-1] // 2
    mean, lv = o[..., :D], o[..., D:]
    gauss = w * 0.5 * torch.exp(-lv) * (mean - ts) ** 2 + w * 0.5 * lv
    return torch.where(km, w * bernoulli_nll(mean, y), gauss).mean(dim=(-1, -2))


def self_losses(o, ts, w, y, km):
    """`self.loss`: mean over (row, column) of 0.5 w (m - t')^2 on Gaussian columns and w l on logistic ones."""
    D = o.shape[-1] // 2
    mean = o[..., :D]
    return torch.where(km, w * bernoulli_nll(mean, y), 0.5 * w * (mean - ts) ** 2).mean(dim=(-1, -2))


def output_deltas(o, ts, w, y, km, loss_type):
    """The closed forms of the header: d(sum_e total_e) / d(raw output) [E, B, 2 D]."""
    D = o.shape[-1] // 2
    B = o.shape[1]
    mean, lv = o[..., :D], o[..., D:]
    diff = mean - ts
    bd = float(B * D)
    dz = w * (sigmoid(mean) - y) / bd
    if loss_type == "NLL":
        iv = torch.exp(-lv)
        dm = torch.where(km, dz, w * iv * diff / bd)
        dl = torch.where(km, torch.zeros_like(lv), w * (0.5 - 0.5 * iv * diff ** 2) / bd)
        return torch.cat((dm, dl), dim=-1)
    ratio = mspe_ratio(o, ts, w, km)
    var = torch.exp(lv)
    dm = torch.where(km, dz, 2.0 * w * diff / bd)
    dl = torch.where(km, 0.1 * lv / bd, (2.0 * ratio * w * (var - diff ** 2) * var + 0.1 * lv) / bd)
    return torch.cat((dm, dl), dim=-1)


class LogisticTrainer(reftrain.EnsembleTrainer):
    """reftrain.EnsembleTrainer (Adam, decays, scalers) in float64 with column kinds and, optionally, §3s's weights."""

    def __init__(self, ws, bs, loss_type, decays, lr=1e-3, kinds=None, col_weight=None, pos_weight=None):
        super().__init__(ws, bs, loss_type=loss_type, decays=decays, lr=lr, dtype=F64)
        self.kinds, self.col_weight, self.pos_weight = kinds, col_weight, pos_weight

    def _forward(self, ws, bs, x, t):
        o = reftrain.forward_raw(torch.as_tensor(np.asarray(x), dtype=F64), ws, bs, self.scaler_in)
        ts = reftrain.scale_targets(torch.as_tensor(np.asarray(t), dtype=F64), self.scaler_out)
        D = ts.shape[-1]
        return o, ts, cw_ref.element_weights(t, self.col_weight, self.pos_weight), labels(t), kinds_mask(self.kinds, D)

    def train_losses(self, ws, bs, x, t):
        """With no logistic column the model IS the one without kinds: the expressions of column_weights_ref (weights attached)
        or of reftrain (none) are evaluated as they stand there, so that the results agree to the last bit."""
        o, ts, w, y, km = self._forward(ws, bs, x, t)
        if not bool(km.any()):
            if self.col_weight is None and self.pos_weight is None:
                return {"MSPE": reftrain.mspe_losses, "NLL": reftrain.nll_losses}[self.loss_type](o, ts)
            return {"MSPE": cw_ref.mspe_losses, "NLL": cw_ref.nll_losses}[self.loss_type](o, ts, w)
        return {"MSPE": mspe_losses, "NLL": nll_losses}[self.loss_type](o, ts, w, y, km)

    def grads(self, x, t):
        ps = [p.clone().requires_grad_(True) for p in self.ws + self.bs]
        n = len(self.ws)
        loss = self.train_losses(ps[:n], ps[n:], x, t).sum()
        for p, d in zip(ps[:n], self.decays):
            loss = loss + d * 0.5 * (p ** 2).sum()
        return float(loss.detach()), torch.autograd.grad(loss, ps)

    def losses(self, x, t):
        with torch.no_grad():
            o, ts, w, y, km = self._forward(self.ws, self.bs, x, t)
            if not bool(km.any()):
                if self.col_weight is None and self.pos_weight is None:
                    return reftrain.holdout_losses(o, ts, True).numpy()
                return cw_ref.self_losses(o, ts, w).numpy()
            return self_losses(o, ts, w, y, km).numpy()


class LogisticTrainer32(LogisticTrainer):
    """LogisticTrainer evaluated at float32: the yardstick of tests/ens_train_f64_ref.py's bound for the cases with kinds."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dtype = torch.float32
        self.ws = [w.to(torch.float32) for w in self.ws]
        self.bs = [b.to(torch.float32) for b in self.bs]

    def _forward(self, ws, bs, x, t):
        o = reftrain.forward_raw(torch.as_tensor(np.asarray(x), dtype=torch.float32), ws, bs, self.scaler_in)
        ts = reftrain.scale_targets(torch.as_tensor(np.asarray(t), dtype=torch.float32), self.scaler_out)
        D = ts.shape[-1]
        w = cw_ref.element_weights(t, self.col_weight, self.pos_weight).to(torch.float32)
        return o, ts, w, labels(t).to(torch.float32), kinds_mask(self.kinds, D)
