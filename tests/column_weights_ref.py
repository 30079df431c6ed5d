"""Float64 torch restatement of the column- and class-weighted probabilistic losses (the definition stands in
include/cmbpo_hip.h at cmbpo_trainer_set_column_weights) -- TEST INFRASTRUCTURE, built on oracle/reftrain.py's forward_raw /
scale_targets.

    w[e][b][d] = col_weight[d] * (t_raw[e][b][d] > 0.5f ? pos_weight[d] : 1)

on the RAW float32 target (a NaN target takes the plain weight); every mean over (row, column) of a data term becomes the mean of
w times the term, the divisor stays B D, the log-variance regulariser stays unweighted."""
import numpy as np
import torch

from oracle import reftrain

F64 = torch.float64


def element_weights(t_raw, col_weight=None, pos_weight=None):
    """w of the targets' shape, float64.  The comparison runs on float32 values, as in the kernels."""
    t32 = np.asarray(t_raw, np.float32)
    D = t32.shape[-1]
    cw = np.ones(D, np.float32) if col_weight is None else np.asarray(col_weight, np.float32).reshape(D)
    pw = np.ones(D, np.float32) if pos_weight is None else np.asarray(pos_weight, np.float32).reshape(D)
    w = np.where(t32 > np.float32(0.5), pw.astype(np.float64), 1.0) * cw.astype(np.float64)
    return torch.as_tensor(w, dtype=F64)


def mspe_ratio(o, ts, w):
    D = o.shape[-1] // 2
    mse = (o[..., :D] - ts) ** 2
    var = torch.exp(o[..., D:])
    return (0.05 * (w * mse).sum() / (w * (var - mse) ** 2).sum()).detach()


def mspe_losses(o, ts, w):
    D = o.shape[-1] // 2
    mean, lv = o[..., :D], o[..., D:]
    mse = (mean - ts) ** 2
    var_logit = (torch.exp(lv) - mse.detach()) ** 2
    ratio = mspe_ratio(o.detach(), ts, w)
    return (w * mse).mean(dim=(-1, -2)) + ratio * (w * var_logit).mean(dim=(-1, -2)) + 0.05 * (lv ** 2).mean()


def nll_losses(o, ts, w):
    D = o.shape[-1] // 2
    mean, lv = o[..., :D], o[..., D:]
    return (w * 0.5 * torch.exp(-lv) * (mean - ts) ** 2).mean(dim=(-1, -2)) + (w * 0.5 * lv).mean(dim=(-1, -2))


def self_losses(o, ts, w):
    """`self.loss` with weights attached: 0.5 mean(w (m - t)^2) per member."""
    D = o.shape[-1] // 2
    return (0.5 * w * (o[..., :D] - ts) ** 2).mean(dim=(-1, -2))


def output_deltas(o, ts, w, loss_type):
    """The closed forms of the header: d(sum_e total_e) / d(raw output) [E, B, 2 D]."""
    D = o.shape[-1] // 2
    E, B = o.shape[0], o.shape[1]
    mean, lv = o[..., :D], o[..., D:]
    diff = mean - ts
    bd = float(B * D)
    if loss_type == "NLL":
        iv = torch.exp(-lv)
        return torch.cat((w * iv * diff / bd, w * (0.5 - 0.5 * iv * diff ** 2) / bd), dim=-1)
    ratio = mspe_ratio(o, ts, w)
    var = torch.exp(lv)
    # the regulariser 0.05 mean_all(lv^2) is a scalar added to EVERY member's total: E times in the sum, 1 / (E B D) each
    return torch.cat((2.0 * w * diff / bd, (2.0 * ratio * w * (var - diff ** 2) * var + 0.1 * lv) / bd), dim=-1)


class WeightedTrainer(reftrain.EnsembleTrainer):
    """reftrain.EnsembleTrainer (Adam, decays, scalers) in float64 with the weighted losses."""

    def __init__(self, ws, bs, loss_type, decays, lr=1e-3, col_weight=None, pos_weight=None):
        super().__init__(ws, bs, loss_type=loss_type, decays=decays, lr=lr, dtype=F64)
        self.col_weight, self.pos_weight = col_weight, pos_weight

    def _forward(self, ws, bs, x, t):
        o = reftrain.forward_raw(torch.as_tensor(np.asarray(x), dtype=F64), ws, bs, self.scaler_in)
        ts = reftrain.scale_targets(torch.as_tensor(np.asarray(t), dtype=F64), self.scaler_out)
        return o, ts, element_weights(t, self.col_weight, self.pos_weight)

    def grads(self, x, t):
        ps = [p.clone().requires_grad_(True) for p in self.ws + self.bs]
        n = len(self.ws)
        o, ts, w = self._forward(ps[:n], ps[n:], x, t)
        loss = {"MSPE": mspe_losses, "NLL": nll_losses}[self.loss_type](o, ts, w).sum()
        for p, d in zip(ps[:n], self.decays):
            loss = loss + d * 0.5 * (p ** 2).sum()
        return float(loss.detach()), torch.autograd.grad(loss, ps)

    def losses(self, x, t):
        with torch.no_grad():
            o, ts, w = self._forward(self.ws, self.bs, x, t)
            return self_losses(o, ts, w).numpy()
