"""Float64 yardstick for the policy-update kernels (csrc/policy_update.hip, csrc/pi_kernel_f16.h) -- TEST INFRASTRUCTURE shared
by tests/test_pi_f64_cpu.py, tests/test_pi_f64_gpu.py and tools/probe_pi_f64.py.

The float32 parameters and batch count as exact.  The existing graphs (oracle/refupdate.PolicyGraph, tests/ppo_lag_ref.Surrogate,
tests/policy_weights_ref.WeightedPolicyGraph / WeightedSurrogate) are evaluated twice on them: at float64, the ground truth, and
at float32, the yardstick.  The kernels compute the Fisher form of the product, so `fisher_vp` is its reference at any theta.

A flat vector (gradient, Fisher-vector product) is cut into its seven blocks W0, b0, W1, b1, W2, b2, log_std, and per block

    err = max |x - x64| / S,        S = max(max |x64| over the block, 2^-10 max |x64| over the whole vector).

2^-10 is how far below its matrix's lift an operand may sit before its second f16 piece leaves the f16 range (header of
pi_kernel_f16.h): a block smaller than that against the rest of its vector is measured against the vector.  `e32` is the float32
reference's err, and the bound a HIP result has to meet on block k is

    MARGIN * max(e32[k], mean of e32 over the vector's seven blocks, FLOOR),        FLOOR = 6e-7 (tests/test_f16_range_gpu.py).

The mean is there because one block's float32 error is a maximum over few rounding patterns (with A = 1 a block is one number).
The loss sums are held to the same expression -- the mean being that of the launch's gradient blocks -- with the KL sum relative
to max(|ref|, 1e-7 n) and the surrogate sums (sum ratio adv, sum ratio cadv, the clipped objective) relative to the SUM OF THEIR
TERMS' MAGNITUDES, sum |w ratio adv|.  Relative to the sum's own magnitude they were first measured at up to 9.7 x (plain cases),
25.6 x (weighted) and 18.7 x (range cases) the float32 reference's error ON BOTH MATRIX PATHS alike: adv and cadv have zero mean,
the sum cancels ten- to fifty-fold, and err / e32 is then the quotient of two single draws of the same amplified rounding noise.
The yardstick was off, not the kernels: a term's rounding error scales with the term, so the terms' magnitudes are the scale.
The count, the cost sum and the clip count stay exact or at rtol 1e-6.

MARGIN is a measurement (tools/probe_pi_f64.py on the MI355X, profiles/r17/pi_f64.json): twice the worst
err_hip / max(e32, mean e32, FLOOR) over the plain cases (CASES_A, CASES_A2, CASES_C) of the f16 path, rounded up to a power of
two; the factor two is for scatter between seeds.  Measured worst ratios at hidden 128, f16 path / fp32-MFMA path: gradients 4.07 /
4.01, products (recomputed and saved alike) 2.41 / 2.86, loss sums 2.01 / 1.62, two tiles per workgroup 1.71 / 0.91, a small
batch after a large one 2.90 / 2.77; hidden 256 (one kernel on both paths) 4.31: MARGIN = 16.  Held to it: the range cases reach
13.7 / 9.4 (products of the 1e3 x observation row, where the float32 reference itself errs by 3e-6; every other mutation stays
below 6.7), sample weights 6.6 / 4.6, the first-order gradient 6.6 / 4.6 and its sums 4.2 / 2.8.  The denominator is always
the reference: MARGIN is never derived from the kernels' output alone.  The range cases (CASES_B) and the weighted / first-order
cases are held to the same MARGIN; the CG solve (CASES_D) has CG_MARGIN, formed the same way from its own ratio (whole vector,
relative to its maximum, against refupdate.cg on the float32 operator).  tests/test_pi_f64_cpu.py holds the condition that keeps MARGIN meaningful whatever was measured: the
bound stays below a quarter of what a float64 evaluation errs by once W1 or W0 is cut to ONE lifted f16 piece.

Cases (batches from tests/golden/worlds.make_update_batch, seeds zlib.crc32 of the case id; parameters `p` 0.03 N(0,1) off
theta_old for gradients, eval and the first-order gradient; the products at theta_old AND at p, each once before any loss_grad
(the recomputing kernel) and once after it (the saved-activation kernel), for a dense direction, a direction with only the log_std
block set and one with dW0 = db0 = 0):
  A   smallest shapes at every border at hidden 128: D in 1 .. 64 (8-wide in_pad groups, half-filled 16-wide k-slabs, the n_it
      switch at 32 / 33), A in 1 .. 32, n in 1 .. 97 (tiles are 32 samples; both n_it instances with a ragged and a full last
      tile); two shapes at hidden 256 (fp32 MFMAs on either path) as a control;
  A2  n = 64 CU + 33 at hidden 128, 32 CU + 33 at hidden 256: the persistent workgroups walk two tiles;
  B   ranges the lifts have to cover, one mutation each (MUTATIONS below).  Mutated observations and parameters are made
      consistent again (mu_old, act and logp_old re-derived at theta_old), so that ratio stays near 1 and the mutated row keeps
      its say in the gradient.  Changed sizes: none of the ten was made smaller; with `w2_entry_1e3` the parameters `p` sit
      3e-4 N(0,1) off theta_old instead of 0.03, because at 0.03 the mean of one action moves by ~1e3 x 0.1 x 0.1 standard
      deviations, every ratio underflows and float32 and float64 alike return a zero gradient (nothing to compare);
  C   batches of 1, 17 and 33 rows bound on a handle that just ran A2 (every partial-vector slot and the saved-activation
      block hold the large batch's data);
  W / PPO  three A shapes and one B mutation with fractional sample weights, and through ppo_grad with `clipped_adv` on and off at
      penalty 0 and 7.5 (rows whose float64 ratio lies within 1e-3 of a clip edge dropped, at most 2 %, as in
      tests/test_ppo_lag_gpu.py);
  D   cg_dev, ten iterations, damping 0.1.
"""
import collections
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(HERE, "golden"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import refupdate  # noqa: E402

import policy_weights_ref as wref  # noqa: E402
import ppo_lag_ref  # noqa: E402

FLOOR = 6e-7
# the b0 block of flat_g of 33x17-n2t-h256 (fp32 MFMAs on either path): 4.38e-6 against 1.02e-6; hidden 128: 4.07 (W1 block, 8x32-n32)
MEASURED_WORST_RATIO = 4.31
MARGIN = 16.0                    # 2 x 4.31 = 8.62, rounded up to a power of two
CG_MEASURED_WORST_RATIO = 0.108  # 29x8-n1037: 5.0e-7 against the float32 operator's 4.6e-6 (the device's dot products are float64)
CG_MARGIN = 0.25                 # 2 x 0.108 = 0.217, rounded up to a power of two

BLOCKS = ("W0", "b0", "W1", "b1", "W2", "b2", "log_std")
KEYS = ("obs", "act", "adv", "cadv", "logp_old", "cost", "mu_old", "log_std_old")
T, SHIFT, CLIP, DAMPING, CG_ITERS = 35, 0.03, 0.2, 0.1, 10
DIRECTIONS = ("dense", "log_std_only", "no_layer0")
PPO_COMBOS = [(clipped, penalty) for clipped in (True, False) for penalty in (0.0, 7.5)]
TWO_TILES = "2t"          # n = 64 CU + 33 (hidden 128) / 32 CU + 33 (hidden 256), resolved on the device

Case = collections.namedtuple("Case", "D A n hidden mutation weighted ppo after_big")


def case(D, A, n, hidden=128, mutation=None, weighted=False, ppo=False, after_big=False):
    return Case(D, A, n, hidden, mutation, weighted, ppo, after_big)


def case_id(c):
    s = "%dx%d-n%s-h%d" % (c.D, c.A, c.n, c.hidden)
    for flag, text in ((c.mutation, c.mutation), (c.weighted, "wfrac"), (c.ppo, "ppo"), (c.after_big, "after2t")):
        if flag:
            s += "-" + text
    return s


CASES_A = [case(*t) for t in (
    # n_it = 1 (D <= 32); (8, 32, 32) and (31, 9, 32) end on a full tile
    (1, 1, 1), (1, 8, 33), (8, 7, 31), (8, 32, 32), (9, 9, 33), (9, 1, 97), (16, 16, 63), (16, 8, 65), (17, 17, 65), (17, 7, 1),
    (31, 31, 97), (31, 9, 32), (32, 32, 33), (32, 16, 63),
    # n_it = 2; (33, 17, 32) and (64, 1, 32) end on a full tile
    (33, 1, 31), (33, 17, 32), (33, 8, 97), (48, 9, 65), (48, 31, 1), (49, 7, 33), (49, 16, 63), (64, 32, 65), (64, 1, 32),
    (64, 17, 97))] + [case(17, 9, 33, 256), case(49, 17, 65, 256)]
SINGLE_TILE_A = [CASES_A[2], CASES_A[11], CASES_A[15]]      # the probe's one-piece sanity check runs on these

CASES_A2 = [case(33, 17, TWO_TILES, 128), case(33, 17, TWO_TILES, 256)]

MUTATIONS = ("obs_row_1e3", "obs_feature_3e4", "obs_row_zero", "adv_outlier_1e4", "adv_zero_tile", "log_std_old_spread",
             "w2_entry_1e3", "w1_1e-2", "wide_direction", "weights_tile")
CASES_B = [case(D, A, n, mutation=m) for (D, A, n) in ((37, 8, 65), (33, 17, 97)) for m in MUTATIONS]

CASES_C = [case(33, 17, n, hidden, after_big=True) for hidden in (128, 256) for n in (1, 17, 33)]

PPO_SHAPES = [case(9, 9, 33), case(32, 16, 63), case(64, 17, 97), case(37, 8, 65, mutation="adv_outlier_1e4")]
CASES_PPO = [c._replace(ppo=True, weighted=w) for w in (False, True) for c in PPO_SHAPES]
CASES_W = [c for c in CASES_PPO if c.weighted]

CASES_D = [case(29, 8, 1037), case(33, 17, TWO_TILES)]

PLAIN = CASES_A + CASES_A2 + CASES_C


def cu_count():
    """Compute units of device 0 (the MI355X has 256; without a device that figure is assumed)."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def rows(c):
    if c.n == TWO_TILES:
        return (64 if c.hidden == 128 else 32) * cu_count() + 33
    return int(c.n)


def one_piece(w):
    """A matrix cut to ONE lifted f16 piece: what a two-piece operand is once its second piece or a cross term is lost."""
    w = np.asarray(w, np.float64)
    lift = 2.0 ** (13.0 - np.floor(np.log2(np.abs(w).max())))
    return (w * lift).astype(np.float16).astype(np.float64) / lift


def cut_block(flat, D, A, hidden, block):
    """`flat` as float64 with one block (index into BLOCKS) replaced by its one-piece rounding."""
    out = np.array(flat, np.float64)
    parts = refupdate.split_params(out, D, A, hidden)       # views
    parts[block][...] = one_piece(parts[block])
    return out


class _At32:
    """The float32 evaluation of a Surrogate (its `grad`, `sums` and `ratio` are written for float64): the yardstick of the
    first-order cases.  `sums` is the weighted form; with no weights it is the plain one (w = 1)."""

    def grad(self, flat, penalty):
        p = torch.tensor(np.asarray(flat, np.float32), dtype=torch.float32, requires_grad=True)
        g, = torch.autograd.grad(self.pi_loss(p, penalty), p)
        return g.numpy()

    def sums(self, flat):
        with torch.no_grad():
            p = torch.as_tensor(np.asarray(flat, np.float32), dtype=torch.float32)
            b = self.g.b
            ratio, obj, active = self.terms(p)
            w = getattr(self.g, "w", None)
            w = torch.ones_like(ratio) if w is None else w
            W = float(w.sum())
            return np.array([W, float((w * obj).sum()), float((w * ratio * b["cadv"]).sum()), float(self.g.d_kl(p)) * W,
                             float((w * b["cost"]).sum()), float((w * (~active)).sum()), float((w * ratio * b["adv"]).sum()), 0.0])


class _Surrogate32(_At32, ppo_lag_ref.Surrogate):
    pass


class _WeightedSurrogate32(_At32, wref.WeightedSurrogate):
    pass


def _refresh_old(params, batch, D, A, hidden):
    """mu_old, act (same noise) and logp_old of the batch at `params`, as make_update_batch derives them."""
    zero = {**batch, "logp_old": np.zeros(batch["obs"].shape[0])}
    with torch.no_grad():
        mu = refupdate.PolicyGraph(D, A, zero, hidden=hidden)._mu(torch.as_tensor(params))[0].numpy().astype(np.float32)
    batch["act"] = (mu + (batch["act"] - batch["mu_old"])).astype(np.float32)
    batch["mu_old"] = mu
    with torch.no_grad():
        g = refupdate.PolicyGraph(D, A, {**batch, "logp_old": np.zeros(mu.shape[0])}, hidden=hidden)
        batch["logp_old"] = g.logp(torch.as_tensor(params)).numpy().astype(np.float32)


def block_errors(x, x64, D, A, hidden):
    """Per block of the flat vector: max |x - x64| / max(max |x64| over the block, 2^-10 max |x64| over the vector)."""
    x, x64 = np.asarray(x, np.float64).reshape(-1), np.asarray(x64, np.float64).reshape(-1)
    whole = float(np.abs(x64).max())
    out = []
    for bx, br in zip(refupdate.split_params(x, D, A, hidden), refupdate.split_params(x64, D, A, hidden)):
        s = max(float(np.abs(br).max()), 2.0 ** -10 * whole, 1e-300)
        out.append(float(np.abs(bx - br).max()) / s)
    return np.array(out)


def yardstick(e32):
    """max(e32[k], mean e32, FLOOR) per block."""
    e32 = np.asarray(e32, np.float64)
    return np.maximum(np.maximum(e32, e32.mean()), FLOOR)


def scalar_error(x, x64, scale):
    return abs(float(x) - float(x64)) / max(float(scale), 1e-300)


def sum_yardstick(e32, *block_e32):
    """max(e32 of the sum, mean e32 over the blocks of the launch's vector(s), FLOOR): a sum is ONE number, so its float32 error
    is one rounding pattern -- the reason the blocks have the mean term."""
    return max(float(e32), float(np.mean(np.concatenate([np.asarray(b, np.float64) for b in block_e32]))), FLOOR)


class Reference:
    """Parameters, batch, directions and weights of one case, with the float64 and the float32 graph on them; every reference
    figure is computed once (`figures`, `ppo_figures`, `cg_figures`) and shared, the arrays are read-only."""

    def __init__(self, c):
        from worlds import make_update_batch
        self.case = c
        D, A, H, n = c.D, c.A, c.hidden, rows(c)
        rng = np.random.default_rng(zlib.crc32(case_id(c._replace(n=n)).encode()))
        theta, batch = make_update_batch(rng, n, D, A, H, 0.3, 1.0, T)
        noise = rng.standard_normal(theta.shape)
        dirs = {"dense": rng.standard_normal(theta.shape).astype(np.float32)}
        dirs["log_std_only"] = np.zeros_like(dirs["dense"])
        dirs["log_std_only"][-A:] = rng.standard_normal(A)
        dirs["no_layer0"] = rng.standard_normal(theta.shape).astype(np.float32)
        dirs["no_layer0"][:D * H + H] = 0.0
        weights, shift, m = None, SHIFT, c.mutation
        row, tile = min(5, n - 1), slice(32, 64)        # the mutated sample (tile 0) and the mutated tile (tile 1)
        w0, b0, w1, b1, w2, b2, ls = refupdate.split_params(theta, D, A, H)      # views
        if m == "obs_row_1e3":
            batch["obs"][row] *= np.float32(1e3)
        elif m == "obs_feature_3e4":
            batch["obs"][row, D // 2] = np.float32(3e4)
        elif m == "obs_row_zero":
            batch["obs"][row] = 0.0
        elif m == "adv_outlier_1e4":            # sets the tile-maximum lift of the cotangent
            batch["adv"][row] *= np.float32(1e4)
            batch["cadv"][row] *= np.float32(1e4)
        elif m == "adv_zero_tile":              # the lift of zero
            batch["adv"][tile] = 0.0
            batch["cadv"][tile] = 0.0
        elif m == "log_std_old_spread":         # 1 / var_old of the Fisher cotangent spans e^8 inside a tile
            batch["log_std_old"] = np.tile(rng.choice(np.array([-3.0, 0.0, 1.0], np.float32), size=(n, 1)), (1, A))
        elif m == "w2_entry_1e3":               # moves the bound max |cot| A max |W2| ten binades away from the data
            w2[7, 0] *= np.float32(1e3)
            shift = SHIFT * 1e-2
        elif m == "w1_1e-2":
            w1 *= np.float32(1e-2)
        elif m == "wide_direction":
            dirs["dense"] = (dirs["dense"] * 10.0 ** rng.uniform(-4, 3, size=theta.shape)).astype(np.float32)
        elif m == "weights_tile":
            weights = np.ones(n, np.float32)
            weights[tile] = 0.0
            weights[row] = 1e3
        elif m is not None:
            raise ValueError(m)
        if m in ("obs_row_1e3", "obs_feature_3e4", "obs_row_zero", "w2_entry_1e3", "w1_1e-2"):
            _refresh_old(theta, batch, D, A, H)
        p = (theta + shift * noise).astype(np.float32)
        if c.weighted:
            weights = np.exp(rng.uniform(np.log(1 / 64), np.log(64), n)).astype(np.float32)     # log-uniform in [1/64, 64]
            weights[::7] = 0.0
        self.dropped = 0
        if c.ppo:
            ratio = ppo_lag_ref.Surrogate(ppo_lag_ref.make_graph(D, A, batch, hidden=H), CLIP).ratio(p)
            keep = (np.abs(ratio - (1 - CLIP)) > 1e-3) & (np.abs(ratio - (1 + CLIP)) > 1e-3)
            self.dropped = int((~keep).sum())
            assert self.dropped <= 0.02 * n, "clip-edge filter removed %d of %d rows" % (self.dropped, n)
            batch = {k: np.ascontiguousarray(v[keep]) for k, v in batch.items()}
            weights = None if weights is None else np.ascontiguousarray(weights[keep])
        self.n = batch["obs"].shape[0]
        self.theta, self.p, self.batch, self.dirs, self.weights = theta, p, batch, dirs, weights
        for a in [theta, p] + list(batch.values()) + list(dirs.values()) + ([] if weights is None else [weights]):
            a.setflags(write=False)
        kw = dict(max_path_length=T, hidden=H)
        if weights is None:
            self.g64 = refupdate.PolicyGraph(D, A, batch, dtype=torch.float64, **kw)
            self.g32 = refupdate.PolicyGraph(D, A, batch, dtype=torch.float32, **kw)
            self.s64, self.s32 = ppo_lag_ref.Surrogate, _Surrogate32
        else:
            self.g64 = wref.WeightedPolicyGraph(D, A, batch, weights, dtype=torch.float64, **kw)
            self.g32 = wref.WeightedPolicyGraph(D, A, batch, weights, dtype=torch.float32, **kw)
            self.s64, self.s32 = wref.WeightedSurrogate, _WeightedSurrogate32
        self.norm = float(self.n) if weights is None else float(np.sum(weights.astype(np.float64)))
        self._fig = self._ppo = self._cg = None

    def errors(self, x, x64):
        return block_errors(x, x64, self.case.D, self.case.A, self.case.hidden)

    def theta_of(self, at):
        return self.theta if at == "old" else self.p

    def figures(self):
        """{"g", "b", ("fvp", at, direction)}: (x64, e32 per block); {"lo", "sc", "ev_kl", "ev_lo", "ev_sc"}: (ref64, e32, scale),
        every one a mean over the batch; the scale of a surrogate is the mean of its terms' magnitudes, of the KL max(|ref|, 1e-7)."""
        if self._fig is None:
            f = {}
            r64, r32 = self.g64.grads(self.p), self.g32.grads(self.p)
            for k, name in enumerate(("g", "b")):
                x64 = np.asarray(r64[k], np.float64)
                f[name] = (x64, self.errors(r32[k], x64))
            with torch.no_grad():
                ratio = torch.exp(self.g64.logp(torch.as_tensor(self.p, dtype=torch.float64)) - self.g64.b["logp_old"]).numpy()
            w = (np.ones(self.n) if self.weights is None else self.weights.astype(np.float64)) / self.norm
            s_lo = float(np.sum(np.abs(w * ratio * self.batch["adv"])))
            s_sc = float(np.sum(np.abs(w * ratio * self.batch["cadv"])))
            f["lo"] = (r64[2], scalar_error(r32[2], r64[2], s_lo), s_lo)
            f["sc"] = (r64[3], scalar_error(r32[3], r64[3], s_sc), s_sc)
            e64, e32 = self.g64.evals(self.p), self.g32.evals(self.p)
            s_kl = max(abs(e64[0]), 1e-7)
            f["ev_kl"] = (e64[0], scalar_error(e32[0], e64[0], s_kl), s_kl)
            f["ev_lo"] = (e64[1], scalar_error(e32[1], e64[1], s_lo), s_lo)
            f["ev_sc"] = (e64[2], scalar_error(e32[2], e64[2], s_sc), s_sc)
            for at in ("old", "off"):
                for d in DIRECTIONS:
                    x64 = np.asarray(self.g64.fisher_vp(self.theta_of(at), self.dirs[d], 0.0), np.float64)
                    f[("fvp", at, d)] = (x64, self.errors(self.g32.fisher_vp(self.theta_of(at), self.dirs[d], 0.0), x64))
            f["cost_sum"] = float(np.sum((1.0 if self.weights is None else self.weights.astype(np.float64)) *
                                         self.batch["cost"].astype(np.float64)))
            self._fig = f
        return self._fig

    def ppo_figures(self):
        """{(clipped, penalty): dict(g=(x64, e32 per block), sums64, sums32, scales)} at `p`; `scales` [8]: the sum of the terms'
        magnitudes for the sums [1], [2], [6], max(|ref|, 1e-7 n) for the KL sum [3]."""
        if self._ppo is None:
            f = {}
            for clipped, penalty in PPO_COMBOS:
                s64 = self.s64(self.g64, CLIP, clipped_adv=clipped, objective_penalized=True)
                s32 = self.s32(self.g32, CLIP, clipped_adv=clipped, objective_penalized=True)
                x64 = np.asarray(s64.grad(self.p, penalty), np.float64)
                sums64 = s64.sums(self.p)
                with torch.no_grad():
                    ratio, obj, _ = s64.terms(torch.as_tensor(self.p, dtype=torch.float64))
                w = np.ones(self.n) if self.weights is None else self.weights.astype(np.float64)
                scales = np.zeros(8)
                scales[1] = np.sum(np.abs(w * obj.numpy()))
                scales[2] = np.sum(np.abs(w * ratio.numpy() * self.batch["cadv"]))
                scales[6] = np.sum(np.abs(w * ratio.numpy() * self.batch["adv"]))
                scales[3] = max(abs(sums64[3]), 1e-7 * sums64[0])
                f[(clipped, penalty)] = dict(g=(x64, self.errors(s32.grad(self.p, penalty), x64)), sums64=sums64,
                                             sums32=s32.sums(self.p), scales=scales)
            self._ppo = f
        return self._ppo

    def cg_figures(self):
        """b, refupdate.cg on the float64 operator at theta_old, and the float32 operator's error over the whole vector."""
        if self._cg is None:
            b = np.random.default_rng(zlib.crc32(b"cg" + case_id(self.case).encode())).standard_normal(self.theta.shape)
            b = b.astype(np.float32)
            x64 = refupdate.cg(lambda v: self.g64.fisher_vp(self.theta, v, DAMPING), b.astype(np.float64), CG_ITERS)
            x32 = refupdate.cg(lambda v: self.g32.fisher_vp(self.theta, v, DAMPING), b.copy(), CG_ITERS)
            assert x32.dtype == np.float32
            self._cg = dict(b=b, x64=x64, e32=whole_error(x32, x64))
        return self._cg


def whole_error(x, x64):
    x64 = np.asarray(x64, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / max(float(np.abs(x64).max()), 1e-300))


_REFS = {}


def reference_of(c):
    """The case's reference, built once and shared."""
    key = c._replace(n=rows(c), after_big=False) if c.after_big else c._replace(n=rows(c))
    if key not in _REFS:
        _REFS[key] = Reference(key)
    return _REFS[key]


def big_case_of(c):
    """The two-tile case a CASES_C case runs first on its handle."""
    return case(c.D, c.A, TWO_TILES, c.hidden)


def scalar_checks(ref, sums, which):
    """[(name, err, yardstick)] of the loss sums a plain launch returns (`which`: 'g', 'b' or 'ev') against float64, as means over
    the batch, after asserting what stays exact: the count (rtol 1e-6 of the weights' sum) and the cost sum (rtol 1e-6).  The
    yardstick's mean term is over the blocks of the launch's gradient (of both gradients for the eval launch)."""
    fig = ref.figures()
    W = float(sums[0])
    if ref.weights is None:
        assert W == ref.n, (W, ref.n)
    else:
        np.testing.assert_allclose(W, ref.norm, rtol=1e-6)
    np.testing.assert_allclose(sums[4], fig["cost_sum"], rtol=1e-6, atol=1e-12)
    blocks = [fig["g"][1], fig["b"][1]] if which == "ev" else [fig[which][1]]
    got = (("ev_kl", sums[3] / W), ("ev_lo", -sums[1] / W), ("ev_sc", sums[2] / W)) if which == "ev" else \
        (("lo", -sums[1] / W), ("sc", sums[2] / W))
    return [(name, scalar_error(x, fig[name][0], fig[name][2]), sum_yardstick(fig[name][1], *blocks)) for name, x in got]


def ppo_scalar_checks(ref, sums, combo):
    """The same for the eight sums of ppo_grad: [1] objective, [2] ratio cadv, [6] ratio adv, [3] KL; the count, the cost sum and
    the clip count (weighted: rtol 1e-6) asserted here."""
    f = ref.ppo_figures()[combo]
    s64, s32, scales = f["sums64"], f["sums32"], f["scales"]
    if ref.weights is None:
        assert sums[0] == ref.n == s64[0] and sums[5] == s64[5], (sums, s64)
    else:
        np.testing.assert_allclose(sums[0], s64[0], rtol=1e-6)
        np.testing.assert_allclose(sums[5], s64[5], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(sums[4], s64[4], rtol=1e-6, atol=1e-12)
    assert sums[7] == 0
    return [(name, scalar_error(sums[k], s64[k], scales[k]), sum_yardstick(scalar_error(s32[k], s64[k], scales[k]), f["g"][1]))
            for k, name in ((1, "obj"), (2, "ratio_cadv"), (6, "ratio_adv"), (3, "kl"))]


# ---------------------------------------------------------------------------------------------------------------------------
# The device side (imported by the GPU test and the probe only)
# ---------------------------------------------------------------------------------------------------------------------------
def make_ops(ref, params=None):
    from cmbpo_amd.cpo_update import PolicyOps
    ops = PolicyOps(ref.case.D, ref.case.A, ref.case.hidden, device="cuda:0")
    ops.set_params(ref.p if params is None else params)
    return ops


def bind(ops, ref):
    ops.bind(*[np.array(ref.batch[k]) for k in KEYS], weights=None if ref.weights is None else np.array(ref.weights))


def _uses(ops):
    from cmbpo_amd import _lib
    return _lib.lib().cmbpo_pi_saved_activation_uses(ops._h)


def last_grid(ops):
    from cmbpo_amd import _lib
    return _lib.lib().cmbpo_pi_last_grid(ops._h)


def gpu_modes(ops, ref, theta=None, p=None):
    """Every plain fetch on the bound batch: {("fvp", at, direction, "recomputed" | "saved"): vector, "g", "b": vectors, "sg",
    "sb", "ev": sums}.  At theta_old and at p the three products run before any loss_grad (nothing saved since set_params: the
    recomputing kernel) and after it (the saved-activation kernel); the use of the saved activations is asserted."""
    out = {}
    for at, params in (("old", ref.theta if theta is None else theta), ("off", ref.p if p is None else p)):
        ops.set_params(np.array(params))
        before = _uses(ops)
        for d in DIRECTIONS:
            out[("fvp", at, d, "recomputed")] = ops.fvp(np.array(ref.dirs[d]))
        assert _uses(ops) == before, "a product before loss_grad read saved activations"
        out["g"], out["sg"] = ops.loss_grad(0)
        if at == "off":
            out["b"], out["sb"] = ops.loss_grad(1)
        out["grid"] = last_grid(ops)
        for d in DIRECTIONS:
            out[("fvp", at, d, "saved")] = ops.fvp(np.array(ref.dirs[d]))
        assert _uses(ops) == before + len(DIRECTIONS), "the products after loss_grad did not read the saved activations"
    out["ev"] = ops.evals()
    return out


def mode_records(ref, got):
    """[(mode, name, err, yard)] of gpu_modes' result against float64: one record per (vector, block) and per loss sum; `yard` is
    max(e32, mean e32, FLOOR).  Asserts what stays exact."""
    fig, rec = ref.figures(), []
    for name in ("g", "b"):
        x64, e32 = fig[name]
        for blk, e, y in zip(BLOCKS, ref.errors(got[name], x64), yardstick(e32)):
            rec.append(("grad", "%s/%s" % (name, blk), float(e), float(y)))
    for key in [k for k in got if isinstance(k, tuple)]:
        _, at, d, inst = key
        x64, e32 = fig[("fvp", at, d)]
        for blk, e, y in zip(BLOCKS, ref.errors(got[key], x64), yardstick(e32)):
            rec.append(("fvp_" + inst, "fvp@%s/%s/%s" % (at, d, blk), float(e), float(y)))
    for which, s in (("g", got["sg"]), ("b", got["sb"]), ("ev", got["ev"])):
        for name, e, y in scalar_checks(ref, s, which):
            rec.append(("eval" if which == "ev" else "grad", "sums_%s/%s" % (which, name), e, y))
    return rec


def set_penalty(ops, penalty):
    """the three derived slots of the state block, directly (penalty 0 has no finite penalty_param)"""
    from cmbpo_amd import _lib
    ops.ppo_state[_lib.PPO_ST_PENALTY:_lib.PPO_ST_CC + 1] = torch.tensor(
        [penalty, 1.0 / (1.0 + penalty), penalty / (1.0 + penalty)], dtype=torch.float64, device=ops.device)


def gpu_ppo(ops, ref):
    out = {}
    ops.set_params(np.array(ref.p))
    for clipped, penalty in PPO_COMBOS:
        set_penalty(ops, penalty)
        out[(clipped, penalty)] = ops.ppo_grad(ops.ppo_cfg(clip_ratio=CLIP, clipped_adv=clipped, objective_penalized=True))
    return out


def ppo_records(ref, got):
    rec = []
    for combo, (g, s) in got.items():
        tag = "clip%d_pen%g" % combo
        x64, e32 = ref.ppo_figures()[combo]["g"]
        for blk, e, y in zip(BLOCKS, ref.errors(g, x64), yardstick(e32)):
            rec.append(("ppo", "%s/%s" % (tag, blk), float(e), float(y)))
        for name, e, y in ppo_scalar_checks(ref, s, combo):
            rec.append(("ppo", "%s/sums/%s" % (tag, name), e, y))
    return rec


def gpu_cg(ops, ref):
    fig = ref.cg_figures()
    ops.set_params(np.array(ref.theta))
    b = torch.from_numpy(np.array(fig["b"])).cuda()
    x = torch.zeros_like(b)
    ops.cg_dev(b, x, DAMPING, iters=CG_ITERS)
    return x.cpu().numpy()
