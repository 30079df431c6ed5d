"""Float64 yardstick for the ensemble training step (csrc/ens_train.hip) -- TEST INFRASTRUCTURE shared by
tests/test_ens_train_f64_cpu.py, tests/test_ens_train_f64_gpu.py and tools/probe_ens_train_f64.py.

The float32 parameters, inputs, scalers and hyper-parameters count as exact.  The training graph of oracle/reftrain.py
(tests/column_weights_ref.py for column-weighted cases) is evaluated twice on them: at float64, the ground truth, and at
float32, the yardstick.  The error of a gradient tensor is

    err[member] = max |g - g64| / max(max |g64|, tiny)          over that member's slice, biases alike,

`e32` of a (case, tensor) is the float32 reference's err, the largest over the members, and the bound a HIP gradient (read as
10 x the first Adam moment after step 1 of a fresh trainer) has to meet is

    MARGIN * max(e32, FLOOR),        FLOOR = 6e-7: five float32 roundings of the tensor's scale (tests/test_f16_range_gpu.py).

`self.loss` is held to the same expression, relative to the loss.

MARGIN is a measurement (tools/probe_ens_train_f64.py on the MI355X, profiles/r16/ens_train_f64.json): the worst
err_hip / max(e32, FLOOR) over the plain cases (CASES_A, CASES_C) is MEASURED_WORST_RATIO = 2.52 (per path: fused step 1.44,
fp32 kernels 1.29 at 128, 0.83 at 256, 1.72 at 512, f16 chain behind the fp32 forward 2.52, f16 chain and forward 1.02, small
batches on a 2048-row trainer 1.32; the range cases of CASES_B reach 3.17), MARGIN = 8 is twice that rounded up to a power of
two.  The factor two is for scatter between seeds and members.  The denominator is always the reference: MARGIN is never
derived from the kernels' output alone.  tests/test_ens_train_f64_cpu.py holds the condition that keeps MARGIN meaningful
whatever was measured: on every 512-wide case the bound on dW0 and dW1 stays below one eighth of what a backward pass errs by
once its matrix operands are cut to ONE f16 piece (a lost low piece or cross term); that leaves room up to 16.
"""
import collections

import numpy as np
import torch

from oracle import reftrain

import column_weights_ref

FLOOR = 6e-7
MEASURED_WORST_RATIO = 2.52      # dW2 of 2x20-512-1-MSE-b1 (f16 backward chain behind the fp32 forward): 1.51e-6 against e32 5.2e-7
MARGIN = 8.0                     # 2 x 2.52 = 5.04, rounded up to a power of two
TENSORS = ("dW0", "dW1", "dW2", "db0", "db1", "db2")
N_ROWS, N_HOLD = 300, 157
LR, DECAY = 1e-3, 1e-4           # decays 2.5e-5 / 5e-5 / 1e-4 (models/pens/pe_factory.py:50-60)

Case = collections.namedtuple("Case", "E I H D loss batch paths fused weighted mutation max_batch")


def case(E, I, H, D, loss, batch, paths, fused=False, weighted=False, mutation=None, max_batch=None):
    return Case(E, I, H, D, loss, batch, paths, fused, weighted, mutation, max_batch)


def case_id(c):
    s = "%dx%d-%d-%d-%s-b%d" % (c.E, c.I, c.H, c.D, c.loss, c.batch)
    for flag, text in ((c.weighted, "colw"), (c.mutation, c.mutation), (c.max_batch, "max%s" % c.max_batch)):
        if flag:
            s += "-" + text
    return s


# A: every kernel path at its smallest shapes.  `paths` is cmbpo_trainer_f16_paths (bit 0 the f16 backward chain, bit 1 the f16
# training forward), `fused` whether fused_mse_step_kernel runs (H == 128, 'MSE', O <= 32, in_pad <= 64).  in_pad = I rounded up
# to 8, OPk = raw outputs (D, or 2 D for the probabilistic heads) rounded up to 8.
CASES_A = [
    # fused step: in_pad 8 / 32 / 40 / 64 (both N_IT instances and their borders), 1, 2 and 8 outputs, one and three members
    case(1, 5, 128, 1, "MSE", 1, 0, True),
    case(3, 5, 128, 2, "MSE", 31, 0, True),
    case(3, 32, 128, 1, "MSE", 33, 0, True),
    case(1, 32, 128, 8, "MSE", 63, 0, True),
    case(3, 33, 128, 2, "MSE", 65, 0, True),
    case(1, 33, 128, 8, "MSE", 97, 0, True),
    case(3, 64, 128, 8, "MSE", 33, 0, True),
    case(1, 64, 128, 1, "MSE", 65, 0, True),
    # general fp32 kernels: in_pad 72 is too wide to fuse; the probabilistic losses; the 256-wide net
    case(2, 65, 128, 1, "MSE", 1, 0),
    case(2, 65, 128, 1, "MSE", 63, 0),
    case(2, 11, 128, 4, "MSPE", 31, 0),
    case(2, 11, 128, 4, "NLL", 97, 0),
    case(2, 20, 256, 6, "MSPE", 33, 0),
    # f16 backward chain + f16 training forward: in_pad 8 / 24 / 40 / 64, OPk 8 / 24 / 40 / 56 / 64 (k-slabs are 16 wide)
    case(2, 5, 512, 4, "MSPE", 1, 3),
    case(2, 20, 512, 11, "NLL", 63, 3),
    case(2, 37, 512, 20, "MSPE", 65, 3),
    case(2, 64, 512, 28, "NLL", 65, 3),
    case(2, 37, 512, 32, "MSPE", 63, 3),
    case(7, 37, 512, 32, "NLL", 33, 3),
    case(2, 5, 512, 32, "NLL", 97, 3),
    case(2, 64, 512, 4, "MSPE", 31, 3),
    case(2, 20, 512, 20, "NLL", 1, 3),
    # f16 backward chain behind the fp32 training forward: a deterministic head; in_pad 72
    case(2, 20, 512, 1, "MSE", 1, 1),
    case(2, 20, 512, 1, "MSE", 65, 1),
    case(2, 70, 512, 1, "MSPE", 63, 1),
    # fp32 kernels at 512: OPk 72 (the first width past the f16 images) and 80
    case(2, 20, 512, 33, "MSPE", 63, 0),
    case(2, 20, 512, 40, "MSPE", 65, 0),
    case(2, 20, 512, 33, "MSPE", 1, 0),
    # column and class weights, the "both" mode of tests/test_column_weights_gpu.py
    case(2, 37, 512, 32, "MSPE", 65, 3, weighted=True),
    case(2, 20, 512, 11, "NLL", 63, 3, weighted=True),
    case(2, 11, 128, 4, "MSPE", 33, 0, weighted=True),
]

# B: ranges inside one batch (the lifts of the two-piece f16 operands), on the f16 kernels and on the fused step
MUTATIONS = ("x_row_1e3", "target_1e3_sigma", "x_row_zero", "w2_entry_1e3", "w1_member_1e-2")
CASES_B = [case(2, 37, 512, 30, "MSPE", 65, 3, mutation=m) for m in MUTATIONS] + \
          [case(3, 33, 128, 2, "MSE", 65, 0, True, mutation=m) for m in MUTATIONS]

# C: a small batch on a trainer created for 2048 rows, after a 2048-row step filled every partial-gradient slot
C_SHAPES = [(3, 29, 128, 1, "MSE", 0, True), (2, 11, 128, 4, "MSPE", 0, False), (2, 37, 512, 30, "MSPE", 3, False)]
CASES_C = [case(E, I, H, D, loss, b, paths, fused, max_batch=2048) for (E, I, H, D, loss, paths, fused) in C_SHAPES for b in (1, 17, 33)]

# D: Adam element by element
CASES_D = [case(E, I, H, D, loss, 33, paths, fused) for (E, I, H, D, loss, paths, fused) in C_SHAPES]


def _truncated_normal(rng, shape):
    """PE.init_weights' draw (two-sigma rejection, tf.truncated_normal_initializer)."""
    w = rng.standard_normal(shape)
    bad = np.abs(w) > 2.0
    while bad.any():
        w[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(w) > 2.0
    return w


class _Weighted32(column_weights_ref.WeightedTrainer):
    """column_weights_ref.WeightedTrainer evaluated at float32: the yardstick of the column-weighted cases."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dtype = torch.float32
        self.ws = [w.to(torch.float32) for w in self.ws]
        self.bs = [b.to(torch.float32) for b in self.bs]

    def _forward(self, ws, bs, x, t):
        o = reftrain.forward_raw(torch.as_tensor(np.asarray(x), dtype=torch.float32), ws, bs, self.scaler_in)
        ts = reftrain.scale_targets(torch.as_tensor(np.asarray(t), dtype=torch.float32), self.scaler_out)
        return o, ts, column_weights_ref.element_weights(t, self.col_weight, self.pos_weight).to(torch.float32)


class Reference:
    """Parameters, data, scalers and index lists of one case, with the float64 and the float32 trainer on them."""

    def figures(self):
        """Gradients and both `self.loss` evaluations at float64 and float32, and the float32 reference's own errors."""
        if self._fig is None:
            f = {}
            xb, tb = self.x[self.idx], self.t[self.idx]
            E = self.case.E
            xh, th = np.tile(self.x[self.hold][None], (E, 1, 1)), np.tile(self.t[self.hold][None], (E, 1, 1))
            for tag, r in (("64", self.r64), ("32", self.r32)):
                f["g" + tag] = [g.numpy().astype(np.float64) for g in r.grads(xb, tb)[1]]
                f["hold" + tag] = r.losses(xh, th).astype(np.float64)
                f["boot" + tag] = r.losses(xb, tb).astype(np.float64)
            f["e32"] = [float(e.max()) for e in tensor_errors(f["g32"], f["g64"])]
            f["e32_hold"] = float(loss_errors(f["hold32"], f["hold64"]).max())
            f["e32_boot"] = float(loss_errors(f["boot32"], f["boot64"]).max())
            self._fig = f
        return self._fig

    def bound(self, e32, margin=None):
        return (MARGIN if margin is None else margin) * max(e32, FLOOR)


def reference(E, I, H, D, loss, batch=33, seed=None, weighted=False, mutation=None, n=N_ROWS, lr=LR, decay=DECAY, **case_kw):
    """Parameters and data drawn as `_make` of tests/test_ens_train_gpu.py draws them (truncated-normal weights, a livelier
    output layer, non-zero biases, inputs of unequal scale, tanh targets, scalers fitted to the data), index lists for a
    bootstrap batch [E, batch] and a shared holdout list, and the trainers: reftrain.EnsembleTrainer at float64 beside the same
    at float32, column_weights_ref.WeightedTrainer for column-weighted cases."""
    c = case(E, I, H, D, loss, batch, case_kw.pop("paths", None), case_kw.pop("fused", None), weighted, mutation,
             case_kw.pop("max_batch", None))
    assert not case_kw, case_kw
    rng = np.random.RandomState(E * 1000 + I + 7 * D + batch if seed is None else seed)
    O = D if loss == "MSE" else 2 * D
    ws = [(_truncated_normal(rng, (E, k, m)) / (2.0 * np.sqrt(k))).astype(np.float32) for k, m in ((I, H), (H, H), (H, O))]
    bs = [(0.1 * rng.standard_normal((E, 1, w.shape[2]))).astype(np.float32) for w in ws]
    ws[2] = (ws[2] * 3).astype(np.float32)
    x = (rng.standard_normal((n, I)) * (1 + rng.rand(I)) + rng.standard_normal(I)).astype(np.float32)
    wtrue = rng.standard_normal((I, D)) / np.sqrt(I)
    t = (np.tanh(x @ wtrue) + 0.1 * rng.standard_normal((n, D))).astype(np.float32)
    cw = pw = None
    if weighted:
        # the last two target columns Bernoulli (rates 0.1 and 0.3), one column without a data term, two class weights
        for col, rate in ((D - 2, 0.1), (D - 1, 0.3)):
            z = x @ wtrue[:, col] + rng.standard_normal(n)
            t[:, col] = (z > np.quantile(z, 1.0 - rate)).astype(np.float32)
        cw = rng.uniform(0.5, 4.0, D).astype(np.float32)
        cw[1] = 0.0
        pw = np.ones(D, np.float32)
        pw[-2:] = (7.0, 3.0)
    sc_in = (x.mean(0, keepdims=True), x.var(0, keepdims=True))
    sc_out = (t.mean(0, keepdims=True), t.var(0, keepdims=True))
    idx = rng.randint(0, n, size=(E, batch)).astype(np.int32)
    hold = rng.permutation(n)[:N_HOLD].astype(np.int32)
    if mutation is not None:
        row = int(idx[0, min(5, batch - 1)])
        idx[:, min(5, batch - 1)] = row          # every member's batch holds the row, so does the holdout list
        hold[3] = row
        if mutation == "x_row_1e3":              # sets the member-wide lift of x in the weight-gradient GEMM
            x[row] *= np.float32(1e3)
            if loss != "MSE":
                # the row's raw outputs are in the hundreds: a log-variance head of the usual size overflows float32's exp in
                # the reference itself (NaN gradients); its weights a hundredth keep the row's log-variances within +-20
                ws[2][:, :, D:] *= np.float32(1e-2)
        elif mutation == "target_1e3_sigma":     # its d3 sets the lifts of d3, d2 and d1
            t[row] += (1e3 * np.sqrt(sc_out[1][0])).astype(np.float32)
        elif mutation == "x_row_zero":
            x[row] = 0.0
        elif mutation == "w2_entry_1e3":         # moves the bound on |d2| ten binades away from the data
            ws[2][:, 7, 0] = np.float32(1e3) * np.abs(ws[2]).max()
        elif mutation == "w1_member_1e-2":       # per-member weight lifts
            ws[1][1] *= np.float32(1e-2)
        else:
            raise ValueError(mutation)
    for a in [x, t, idx, hold] + ws + bs:
        a.setflags(write=False)
    r = Reference()
    r.case, r.ws, r.bs, r.x, r.t, r.sc_in, r.sc_out, r.idx, r.hold = c, ws, bs, x, t, sc_in, sc_out, idx, hold
    r.lr, r.decay, r.decays, r.cw, r.pw, r._fig = lr, decay, (decay / 4.0, decay / 2.0, decay), cw, pw, None
    if weighted:
        r.r64 = column_weights_ref.WeightedTrainer(ws, bs, loss, r.decays, lr=lr, col_weight=cw, pos_weight=pw)
        r.r32 = _Weighted32(ws, bs, loss, r.decays, lr=lr, col_weight=cw, pos_weight=pw)
    else:
        r.r64 = reftrain.EnsembleTrainer(ws, bs, loss_type=loss, decays=r.decays, lr=lr, dtype=torch.float64)
        r.r32 = reftrain.EnsembleTrainer(ws, bs, loss_type=loss, decays=r.decays, lr=lr, dtype=torch.float32)
    for t_ in (r.r64, r.r32):
        t_.set_scalers(sc_in, sc_out)
    return r


_REFS = {}


def reference_of(c):
    """The case's reference, built once and shared (its arrays are read-only)."""
    if c not in _REFS:
        _REFS[c] = reference(c.E, c.I, c.H, c.D, c.loss, batch=c.batch, weighted=c.weighted, mutation=c.mutation, paths=c.paths,
                             fused=c.fused, max_batch=c.max_batch)
    return _REFS[c]


def tensor_errors(got, ref64, tiny=1e-300):
    """Per tensor an array [E]: max |got - ref64| / max(max |ref64|, tiny) over the member's slice."""
    out = []
    for g, r in zip(got, ref64):
        r = np.asarray(r, np.float64)
        d = np.abs(np.asarray(g, np.float64).reshape(r.shape) - r).reshape(r.shape[0], -1).max(axis=1)
        out.append(d / np.maximum(np.abs(r).reshape(r.shape[0], -1).max(axis=1), tiny))
    return out


def loss_errors(got, ref64, tiny=1e-300):
    ref64 = np.asarray(ref64, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref64) / np.maximum(np.abs(ref64), tiny)


# ---------------------------------------------------------------------------------------------------------------------------
# The device side (imported by the GPU test and the probe only)
# ---------------------------------------------------------------------------------------------------------------------------
def make_pe(ref, max_batch=None):
    """(PE, trainer) holding the case's parameters; asserts the kernels the case is meant for."""
    from cmbpo_amd.pens import PE
    c = ref.case
    pe = PE(c.I, c.D, name="T", hidden_dims=(c.H, c.H), num_networks=c.E, num_elites=max(1, c.E - 2), loss=c.loss,
            use_scaler_in=True, use_scaler_out=True, device="cuda:0", lr=ref.lr, decay=ref.decay, col_weight=ref.cw,
            pos_weight=ref.pw)
    pe.set_weights(ref.ws, ref.bs, ref.sc_in, ref.sc_out)
    tr = pe._ensure_trainer(max_batch or c.max_batch or c.batch)
    assert tr.f16_paths == c.paths, (case_id(c), tr.f16_paths)
    assert tr.fused == bool(c.fused), (case_id(c), tr.fused)
    return pe, tr


def _dev(a):
    return torch.tensor(np.asarray(a)).cuda()      # (a copy: the shared arrays are read-only)


def gradient_of_first_step(tr, scale=10.0):
    """The gradient a fresh trainer's first step saw: the first Adam moment over 1 - beta1."""
    mw, mb = tr.get_moments(0)
    return [scale * a.astype(np.float64) for a in mw + mb]


def gpu_losses(ref, tr):
    """`self.loss` on the shared holdout list (idx_stride 0) and on the per-member bootstrap rows."""
    xd, td = _dev(ref.x), _dev(ref.t)
    hold = tr.losses(xd, td, _dev(ref.hold), 0, ref.hold.shape[0]).cpu().numpy()
    boot = tr.losses(xd, td, _dev(ref.idx), ref.case.batch, ref.case.batch).cpu().numpy()
    return hold, boot


def gpu_step(ref, tr, idx=None):
    idx = ref.idx if idx is None else idx
    idx_d = _dev(idx)
    tr.step(_dev(ref.x), _dev(ref.t), idx_d.data_ptr(), idx.shape[1], idx.shape[1])
    torch.cuda.synchronize()


def gpu_first_step_errors(ref):
    """A/B: {tensor: err[E]} of a fresh trainer's first step, and the two loss errors [E], against float64."""
    fig = ref.figures()
    pe, tr = make_pe(ref)
    hold, boot = gpu_losses(ref, tr)
    gpu_step(ref, tr)
    assert tr.steps_done == 1
    errs = dict(zip(TENSORS, tensor_errors(gradient_of_first_step(tr), fig["g64"])))
    return errs, loss_errors(hold, fig["hold64"]), loss_errors(boot, fig["boot64"])


def gpu_small_batch_errors(ref):
    """C: one step at max_batch rows (every partial-gradient slot written), the initial parameters and a zeroed optimizer again,
    one step at the case's batch: {tensor: err[E]} of that step against float64 on its rows."""
    c = ref.case
    fig = ref.figures()
    pe, tr = make_pe(ref)
    big = np.random.RandomState(c.batch).randint(0, ref.x.shape[0], size=(c.E, c.max_batch)).astype(np.int32)
    gpu_step(ref, tr, big)
    pe.set_weights(ref.ws, ref.bs, ref.sc_in, ref.sc_out)
    tr.reset_optimizer()
    assert pe._trainer is tr and tr.max_batch == c.max_batch and tr.steps_done == 0      # cmbpo_trainer_reset_optimizer zeroes the count
    gpu_step(ref, tr)
    assert tr.steps_done == 1
    return dict(zip(TENSORS, tensor_errors(gradient_of_first_step(tr), fig["g64"])))


B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))      # the trainer's float32 hyper-parameters, taken as exact


def gpu_adam(ref):
    """D: a fresh trainer's step gives g = 10 m; a second trainer starts the same step from moments (m0, v0) and 7 steps done.
    Returns per parameter tensor (W0 W1 W2 b0 b1 b2) the float32 inputs and the trainer's m, v, w, and the PE."""
    c = ref.case
    _, t1 = make_pe(ref)
    gpu_step(ref, t1)
    g = [a.astype(np.float32) * np.float32(10.0) for a in sum(t1.get_moments(0), [])]
    pe, t2 = make_pe(ref)
    rng = np.random.RandomState(c.E + c.I)
    m0, v0 = [], []
    for a in g:
        s = float(np.sqrt(np.mean(a.astype(np.float64) ** 2)))
        m0.append((s * rng.uniform(-2.0, 2.0, a.shape)).astype(np.float32))
        v0.append((s * s * rng.uniform(0.5, 2.0, a.shape)).astype(np.float32))
    t2.set_moments(0, m0[:3], m0[3:], 7)
    t2.set_moments(1, v0[:3], v0[3:], 7)
    gpu_step(ref, t2)
    got = dict(m=sum(t2.get_moments(0), []), v=sum(t2.get_moments(1), []), w=sum(t2.get_weights(), []), steps_done=t2.steps_done)
    return dict(g=g, m0=m0, v0=v0, w0=list(ref.ws) + list(ref.bs), got=got, pe=pe, lr=float(np.float32(ref.lr)))


def adam_float64(g, m0, v0, w0, lr, steps_before=7):
    """tf.train.AdamOptimizer's step in float64 on float32 inputs; `g` already contains the layer's decay."""
    g, m0, v0, w0 = (np.asarray(a, np.float64).reshape(np.shape(w0)) for a in (g, m0, v0, w0))
    t = steps_before + 1
    m1 = m0 + (g - m0) * (1.0 - B1)
    v1 = v0 + (g * g - v0) * (1.0 - B2)
    lr_t = lr * np.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)
    return m1, v1, w0 - lr_t * m1 / (np.sqrt(v1) + 1e-8), lr_t


def adam_errors(d):
    """Per parameter tensor the largest element-wise error of m, v and w, relative to max(|m0|, |g|), max(v0, g^2) and
    |W0| + lr_t."""
    out = []
    for k in range(6):
        m1, v1, w1, lr_t = adam_float64(d["g"][k], d["m0"][k], d["v0"][k], d["w0"][k], d["lr"])
        g, m0, v0, w0 = (np.asarray(d[n][k], np.float64).reshape(m1.shape) for n in ("g", "m0", "v0", "w0"))
        got = {n: np.asarray(d["got"][n][k], np.float64).reshape(m1.shape) for n in ("m", "v", "w")}
        out.append(dict(m=float((np.abs(got["m"] - m1) / np.maximum(np.abs(m0), np.abs(g))).max()),
                        v=float((np.abs(got["v"] - v1) / np.maximum(v0, g * g)).max()),
                        w=float((np.abs(got["w"] - w1) / (np.abs(w0) + lr_t)).max())))
    return out


def forward_errors(pe, x):
    """D, last step: the prediction kernels' packed and f16 images followed the masters.  Returns (err_hip, err32) per (member,
    row), each max over the outputs of |out - f64| / the (member, row)'s output scale: the prediction of the PE against
    test_f16_range_gpu.f64_forward of the trainer's own weights, and a float32 numpy evaluation of the same against it."""
    from test_f16_range_gpu import f64_forward
    ws, bs = pe.get_weights()
    sc_in = (pe.scaler_in.cached_mu, pe.scaler_in.cached_var)
    sc_out = (pe.scaler_out.cached_mu, pe.scaler_out.cached_var)
    if pe.is_probabilistic:
        ref_mean, _ = f64_forward(x, ws, bs, sc_in, sc_out)
        mean, _ = pe.predict_ensemble(x)
    else:
        # a deterministic head: f64_forward splits its last layer in two halves, so run it on the head doubled
        ref_mean, _ = f64_forward(x, ws[:2] + [np.concatenate([ws[2], ws[2]], 2)], bs[:2] + [np.concatenate([bs[2], bs[2]], 2)],
                                  sc_in, sc_out)
        ref_mean = ref_mean.mean(axis=0, keepdims=True)
        mean = pe.predict(x)[None]                 # the mean over the members, through the output scaler
    # the same network in float32 numpy: the yardstick of the floor-and-twice rule
    f32 = np.float32
    sig_in = np.maximum(np.sqrt(sc_in[1].astype(f32)), f32(1e-2)).reshape(1, -1)
    sig_out = np.maximum(np.sqrt(sc_out[1].astype(f32)), f32(1e-2)).reshape(1, 1, -1)
    h = (x.astype(f32) - sc_in[0].astype(f32).reshape(1, -1)) / sig_in
    h = np.einsum("ij,ajk->aik", h, ws[0]) + bs[0].reshape(ws[0].shape[0], 1, -1)
    h = h / (f32(1) + np.exp(-h))
    h = np.matmul(h, ws[1]) + bs[1].reshape(ws[1].shape[0], 1, -1)
    h = h / (f32(1) + np.exp(-h))
    o = np.matmul(h, ws[2]) + bs[2].reshape(ws[2].shape[0], 1, -1)
    m32 = sig_out * o[..., :pe.out_dim] + sc_out[0].astype(f32).reshape(1, 1, -1)
    if not pe.is_probabilistic:
        m32 = m32.mean(axis=0, keepdims=True)
    assert m32.dtype == f32
    scale = np.maximum(np.abs(ref_mean).max(axis=2), 1e-30)
    return np.abs(mean.astype(np.float64) - ref_mean).max(axis=2) / scale, np.abs(m32.astype(np.float64) - ref_mean).max(axis=2) / scale
