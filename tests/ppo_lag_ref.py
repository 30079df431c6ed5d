"""Float64 statement of the first-order penalised update (PPO-Lagrangian) -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

On top of ``oracle.refupdate.PolicyGraph`` (its ``logp``, ``d_kl`` and ``ent`` are what the objective needs), torch-CPU
autograd in float64.  Semantics (safety-starter-agents' PPO-Lagrangian, the family the reference's Agent declares):

    ratio     = exp(logp - logp_old)
    min_adv   = adv > 0 ? (1 + clip) adv : (1 - clip) adv
    surr_adv  = mean(clipped_adv ? min(ratio adv, min_adv) : ratio adv)
    surr_cost = mean(ratio cadv)
    objective = surr_adv + ent_reg entropy;  penalised: (objective - penalty surr_cost) / (1 + penalty)
    pi_loss   = -objective

One update = penalty step (learn_penalty), then up to ``pi_iters`` iterations, numbered from 1: iteration i measures the KL
of the parameters it finds; above kl_margin * target_kl it stops WITHOUT stepping (StopIter = i), otherwise it takes one
TF-Adam step along grad pi_loss.
"""
import numpy as np
import torch

from oracle import refupdate

F64 = torch.float64


def make_graph(D, A, batch, hidden=128, ent_reg=0.0, max_path_length=1):
    return refupdate.PolicyGraph(D, A, batch, ent_reg=ent_reg, max_path_length=max_path_length, dtype=F64, hidden=hidden)


def softplus(x):
    return float(np.log1p(np.exp(-abs(x))) + max(x, 0.0))


def sigmoid(x):
    return float(1.0 / (1.0 + np.exp(-x)))


class Surrogate:
    def __init__(self, graph, clip_ratio=0.2, clipped_adv=True, objective_penalized=True):
        self.g, self.clip = graph, float(clip_ratio)
        self.clipped_adv, self.objective_penalized = clipped_adv, objective_penalized

    def terms(self, p):
        """ratio, per-sample objective term, active mask (first argument of the minimum wins a tie, as in tf.minimum)"""
        b = self.g.b
        ratio = torch.exp(self.g.logp(p) - b["logp_old"])
        ra = ratio * b["adv"]
        min_adv = torch.where(b["adv"] > 0, (1 + self.clip) * b["adv"], (1 - self.clip) * b["adv"])
        active = (ra <= min_adv) if self.clipped_adv else torch.ones_like(ra, dtype=torch.bool)
        return ratio, torch.where(active, ra, min_adv), active

    def pi_loss(self, p, penalty):
        ratio, obj, _ = self.terms(p)
        o = obj.mean() + self.g.ent_reg * self.g.ent(p)
        if self.objective_penalized:
            o = (o - penalty * (ratio * self.g.b["cadv"]).mean()) / (1 + penalty)
        return -o

    def grad(self, flat, penalty):
        p = torch.tensor(np.asarray(flat, np.float64), dtype=F64, requires_grad=True)
        g, = torch.autograd.grad(self.pi_loss(p, penalty), p)
        return g.numpy()

    def sums(self, flat):
        """The eight loss sums of a pass: n, sum objective term, sum ratio cadv, sum kl, sum cost, clip count, sum ratio adv, 0"""
        with torch.no_grad():
            p = torch.as_tensor(np.asarray(flat, np.float64), dtype=F64)
            b = self.g.b
            ratio, obj, active = self.terms(p)
            n = ratio.shape[0]
            return np.array([n, float(obj.sum()), float((ratio * b["cadv"]).sum()), float(self.g.d_kl(p)) * n,
                             float(b["cost"].sum()), float((~active).sum()), float((ratio * b["adv"]).sum()), 0.0])

    def ratio(self, flat):
        with torch.no_grad():
            return self.terms(torch.as_tensor(np.asarray(flat, np.float64), dtype=F64))[0].numpy()


def adam_step(theta, m, v, t, g, lr, b1=0.9, b2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer, float64; returns (theta, m, v, t) after the step"""
    t = t + 1
    lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    m = m + (g - m) * (1 - b1)
    v = v + (g * g - v) * (1 - b2)
    return theta - lr_t * m / (np.sqrt(v) + eps), m, v, t


def penalty_step(pen, cur_cost, cost_lim, lr, penalty_param_loss=True):
    """pen = dict(param, m, v, t); penalty_loss = -param (cur_cost - cost_lim) or -softplus(param) (...); one Adam step"""
    x = pen["param"]
    g = -(cur_cost - cost_lim) * (1.0 if penalty_param_loss else sigmoid(x))
    x, m, v, t = adam_step(x, pen["m"], pen["v"], pen["t"], g, lr)
    return dict(param=float(x), m=float(m), v=float(v), t=t)


def penalty_first_step_closed_form(param, cur_cost, cost_lim, lr, penalty_param_loss=True, b2=0.999, eps=1e-8):
    """From zero moments Adam's first step is lr g / (|g| + eps / sqrt(1 - b2))"""
    g = -(cur_cost - cost_lim) * (1.0 if penalty_param_loss else sigmoid(param))
    return param - lr * g / (abs(g) + eps / np.sqrt(1 - b2))


def run_loop(sur, theta, m, v, t, penalty, pi_lr, iters, kl_lim):
    """The gated iterations.  Returns dict(theta, m, v, t, stop (0: none), steps, kls [k] = KL measured at iteration k + 1,
    sums_first, clip_last)"""
    theta = np.asarray(theta, np.float64).copy()
    kls, stop, steps, sums_first, clip_last = [], 0, 0, None, 0.0
    for it in range(1, iters + 1):
        s = sur.sums(theta)
        if it == 1:
            sums_first = s
        kls.append(s[3] / s[0])
        clip_last = s[5]
        if not kls[-1] <= kl_lim:
            stop = it
            break
        theta, m, v, t = adam_step(theta, m, v, t, sur.grad(theta, penalty), pi_lr)
        steps += 1
    return dict(theta=theta, m=m, v=v, t=t, stop=stop, steps=steps, kls=np.array(kls), sums_first=sums_first,
                clip_last=clip_last)


class RefAgent:
    """PPOLagAgent in float64: state persists across updates"""

    def __init__(self, P, penalty_init=1.0, penalty_lr=5e-2, penalty_param_loss=True, learn_penalty=True, pi_lr=3e-4,
                 pi_iters=80, clip_ratio=0.2, kl_margin=1.2, clipped_adv=True, objective_penalized=True, max_path_length=1):
        self.pen = dict(param=float(np.log(max(np.exp(penalty_init) - 1, 1e-8))), m=0.0, v=0.0, t=0)
        self.m, self.v, self.t = np.zeros(P), np.zeros(P), 0
        self.kw = dict(clip_ratio=clip_ratio, clipped_adv=clipped_adv, objective_penalized=objective_penalized)
        self.penalty_lr, self.penalty_param_loss, self.learn_penalty = penalty_lr, penalty_param_loss, learn_penalty
        self.pi_lr, self.pi_iters, self.kl_margin, self.T = pi_lr, pi_iters, kl_margin, max_path_length

    def update_pi(self, graph, theta, target_kl, cost_lim):
        sur = Surrogate(graph, **self.kw)
        before = softplus(self.pen["param"])
        if self.learn_penalty:
            cur_cost = float(graph.b["cost"].mean()) * self.T
            self.pen = penalty_step(self.pen, cur_cost, cost_lim, self.penalty_lr, self.penalty_param_loss)
        penalty = softplus(self.pen["param"])
        r = run_loop(sur, theta, self.m, self.v, self.t, penalty, self.pi_lr, self.pi_iters, self.kl_margin * target_kl)
        self.m, self.v, self.t = r["m"], r["v"], r["t"]
        post = sur.sums(r["theta"])
        n = post[0]
        return dict(params=r["theta"], Penalty=penalty, PenaltyDelta=penalty - before,
                    StopIter=r["stop"] if r["stop"] else self.pi_iters, ClipFrac=r["clip_last"] / n, kls=r["kls"],
                    kl_lim=self.kl_margin * target_kl,
                    post=dict(KL=post[3] / n, SurrAdv=post[6] / n, SurrCost=post[2] / n))
