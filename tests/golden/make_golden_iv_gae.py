"""Generate golden G17: inverse-variance-weighted GAE, recorded from the REFERENCE's own weighted branch of
discount_cumsum(x, discount, lam, weights=..., axis=-1) (utilities/utils.py:189-208) and from its ModelBuffer /
ModelSampler with that branch switched on.

Usage (build container only, like make_golden.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_iv_gae.py

The reference's ModelBuffer calls discount_cumsum without weights (buffers/modelbuffer.py:168,177), although it keeps the
per-step epistemic variance in dyn_error_buf for exactly this.  To plug the weights in, the name `discount_cumsum` inside
the reference's buffers.modelbuffer module is replaced by a wrapper that adds weights=, and ModelBuffer.finish_path_multiple
is wrapped only to note which rows are being finished: their weights are
    w[b, u] = 1 / (iv_eps + cumsum_u(float64(dyn_error_buf[b, :ptr]))).
No method body of the reference is copied.

Writes data only, every file at most 520 KB:
  (a) g17_iv_cumsum.npz -- direct calls: L in {1, 2, 3, 7, 34}, 16 rows each, (gamma, lam) in {(0.99, 0.95), (0.97, 0.5)},
      x float32 and float64, variances 10^U(-12, 2) with some exact zeros, iv_eps in {1e-8, 1e-2}; beside them the
      lambda tables: lfilter([1], [1, -lam]) on a unit impulse (the reference's lam_vec) and Python's lam ** L.
  (b) g17_iv_buffer.npz -- the patched ModelBuffer driven through store_multiple / finish_path_multiple / get at B = 37,
      T = 6 with a ragged schedule: finishes before any store, mid-way with float32 and float64-zero bootstraps, at the end.
  (c) g17_trace_iv_{ant_term,hcs_sched}.npz -- make_golden.run_sampler_trace under the patch (iv_eps = 1e-8).  Asserted
      before a trace is written: its row counts per step are those of the unpatched run, and at least 25 % of its adv and
      of its cadv samples differ from the unpatched run's by more than ten times the tolerance of the replays.
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the stubs behind which the reference imports; puts the reference on sys.path)

MAX_BYTES = 520 * 1024
CUMSUM_L = (1, 2, 3, 7, 34)
CUMSUM_ROWS = 16
CUMSUM_GL = ((0.99, 0.95), (0.97, 0.5))
CUMSUM_EPS = (1e-8, 1e-2)
TABLE_T = 34
TRACE_EPS = 1e-8
TRACE_TOL = dict(adv=5e-3, cadv=2e-3)        # test_rollout_sampler_gpu.TOL
TRACE_MIN_CHANGED = 0.25

TRACES = {
    "g17_trace_iv_ant_term": dict(seed=7, task="AntSafe-v2", B=96, T=8, hidden=128, dkl_lim=float("inf"), budget=None,
                                  mode="uncertainty", q_boost=2.5),
    "g17_trace_iv_hcs_sched": dict(seed=8, task="HalfCheetahSafe-v2", B=64, T=9, hidden=128, dkl_lim=float("inf"),
                                   budget=None, mode="schedule"),
}


def variances(rng, shape):
    """float32 variances spread over 1e-12 .. 1e2, about one in eight exactly zero."""
    v = (10.0 ** rng.uniform(-12, 2, shape)).astype(np.float32)
    v[rng.random(shape) < 0.125] = 0.0
    return v


def iv_weights(var32, iv_eps):
    return 1.0 / (iv_eps + np.cumsum(var32.astype(np.float64), axis=-1))


class IvPatch:
    """Switches the reference's ModelBuffer to the weighted branch of its own discount_cumsum."""

    def __init__(self, iv_eps):
        import buffers.modelbuffer as mb
        self.mb, self.iv_eps, self.weights = mb, iv_eps, None
        self.orig_dc, self.orig_fin = mb.discount_cumsum, mb.ModelBuffer.finish_path_multiple
        patch = self

        def dc(x, discount, lam, weights=None, axis=0):
            return patch.orig_dc(x, discount, lam, weights=patch.weights, axis=axis)

        def fin(buf, term_mask, last_val=0, last_cval=0):
            tm = np.asarray(term_mask, dtype=bool)
            if tm.any() and buf.ptr > 0:
                rows = np.flatnonzero(buf.alive_paths)[tm]
                patch.weights = iv_weights(buf.dyn_error_buf[rows, :buf.ptr], patch.iv_eps)
            return patch.orig_fin(buf, term_mask, last_val, last_cval)

        mb.discount_cumsum, mb.ModelBuffer.finish_path_multiple = dc, fin

    def close(self):
        self.mb.discount_cumsum, self.mb.ModelBuffer.finish_path_multiple = self.orig_dc, self.orig_fin


def save(out, name, data):
    blob = io.BytesIO()
    np.savez_compressed(blob, **data)
    assert blob.getbuffer().nbytes <= MAX_BYTES, (name, blob.getbuffer().nbytes)
    with open(os.path.join(out, name + ".npz"), "wb") as f:
        f.write(blob.getvalue())
    print(name, "bytes", blob.getbuffer().nbytes)


def gen_cumsum(out):
    import scipy.signal
    from utilities.utils import discount_cumsum
    rng = np.random.default_rng(1700)
    data = dict(Ls=np.array(CUMSUM_L), gl=np.array(CUMSUM_GL), eps=np.array(CUMSUM_EPS), table_T=TABLE_T)
    for L in CUMSUM_L:
        var = variances(rng, (CUMSUM_ROWS, L))
        x64 = rng.standard_normal((CUMSUM_ROWS, L))
        x32 = rng.standard_normal((CUMSUM_ROWS, L)).astype(np.float32)
        data.update({f"L{L}_var": var, f"L{L}_x32": x32, f"L{L}_x64": x64})
        for gi, (g, l) in enumerate(CUMSUM_GL):
            for ei, eps in enumerate(CUMSUM_EPS):
                w = iv_weights(var, eps)
                for tag, x in (("32", x32), ("64", x64)):
                    with np.errstate(all="ignore"):
                        y = discount_cumsum(x.copy(), g, l, weights=w.copy(), axis=-1)
                    assert y.dtype == np.float64 and y.shape == x.shape
                    data[f"L{L}_g{gi}_e{ei}_y{tag}"] = y
    for gi, (g, l) in enumerate(CUMSUM_GL):
        seed = np.zeros(TABLE_T)
        seed[0] = 1
        data[f"lam_vec_g{gi}"] = scipy.signal.lfilter([1], [1, float(-l)], seed)      # utilities/utils.py:195-197
        data[f"lam_pow_g{gi}"] = np.array([l ** k for k in range(TABLE_T + 1)], np.float64)   # :192
    save(out, "g17_iv_cumsum", data)


def gen_buffer(out):
    from buffers.modelbuffer import ModelBuffer
    rng = np.random.default_rng(1717)
    B, T, D, A = 37, 6, 5, 2
    iv_eps = 1e-8
    patch = IvPatch(iv_eps)
    try:
        buf = ModelBuffer(batch_size=B, obs_dim=D, act_dim=A, max_path_length=T)
        buf.initialize({"mu": [A], "log_std": [A]}, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
        names = ("rew", "val", "cost", "cval", "logp")
        step = {k: np.zeros((T, B), np.float32) for k in names + ("dyn_error",)}
        step["obs"], step["act"] = np.zeros((T, B, D), np.float32), np.zeros((T, B, A), np.float32)
        step["mu"], step["log_std"] = np.zeros((T, B, A), np.float32), np.zeros((T, B, A), np.float32)
        # finish events, by branch slot: after step ev_step (-1: before any store)
        ev_step, ev_mask, ev_zero, ev_lv, ev_lcv = [], [], [], [], []
        alive = np.ones(B, bool)

        def finish(t, slots, zero):
            idx = np.flatnonzero(alive)
            tm = np.isin(idx, slots)
            n = int(tm.sum())
            lv = np.zeros(n) if zero else rng.standard_normal(n).astype(np.float32)
            lcv = rng.standard_normal(n).astype(np.float32)
            buf.finish_path_multiple(tm, lv, lcv)
            m, a, c = np.zeros(B, bool), np.zeros(B, np.float32), np.zeros(B, np.float32)
            m[idx[tm]], a[idx[tm]], c[idx[tm]] = True, lv, lcv
            ev_step.append(t); ev_mask.append(m); ev_zero.append(zero); ev_lv.append(a); ev_lcv.append(c)
            alive[idx[tm]] = False

        finish(-1, [1, 5, 36], False)
        for t in range(T):
            idx = np.flatnonzero(alive)
            n = len(idx)
            v = {k: rng.standard_normal(n).astype(np.float32) for k in names}
            v["dyn_error"] = variances(rng, n)
            v["obs"] = rng.standard_normal((n, D)).astype(np.float32)
            for k in ("act", "mu", "log_std"):
                v[k] = rng.standard_normal((n, A)).astype(np.float32)
            buf.store_multiple(v["obs"], v["act"], v["obs"], v["rew"], v["val"], v["cost"], v["cval"], v["dyn_error"], v["logp"],
                               {"mu": v["mu"], "log_std": v["log_std"]}, np.zeros(n, bool))
            for k in v:
                step[k][t, idx] = v[k]
            if t < T - 1:
                tm = rng.random(n) < 0.25
                if tm.any():
                    finish(t, idx[tm], t % 2 == 1)
            assert (buf.alive_paths == alive).all()
        finish(T - 1, np.flatnonzero(alive), False)
        with np.errstate(all="ignore"):
            res, diag = buf.get()
    finally:
        patch.close()
    data = dict(B=B, T=T, D=D, A=A, iv_eps=iv_eps, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5,
                ev_step=np.array(ev_step), ev_mask=np.array(ev_mask), ev_zero=np.array(ev_zero), ev_lv=np.array(ev_lv),
                ev_lcv=np.array(ev_lcv), poolm_batch_size=diag["poolm_batch_size"])
    data.update({"step_" + k: v for k, v in step.items()})
    for k, v in zip(["obs", "act", "adv", "cadv", "ret", "cret", "logp", "val", "cval", "cost", "log_std", "mu"], res):
        data["get_" + k] = v
    assert np.isfinite(data["get_adv"]).all() and np.isfinite(data["get_cret"]).all()
    print("buffer: events", len(ev_step), "zero-boot events", int(np.sum(ev_zero)), "samples", int(diag["poolm_batch_size"]))
    save(out, "g17_iv_buffer", data)


def gen_traces(out):
    for name, cfg in TRACES.items():
        plain = mg.run_sampler_trace(**cfg)
        patch = IvPatch(TRACE_EPS)
        try:
            data = mg.run_sampler_trace(**cfg)
        finally:
            patch.close()
        assert data["n_rows"].tolist() == plain["n_rows"].tolist(), (name, data["n_rows"], plain["n_rows"])
        np.testing.assert_array_equal(data["alive"], plain["alive"])
        np.testing.assert_array_equal(data["get_obs"], plain["get_obs"])
        changed = {}
        for k, tol in TRACE_TOL.items():
            a, b = data["get_" + k], plain["get_" + k]
            assert np.isfinite(a).all(), (name, k)
            changed[k] = float(np.mean(np.abs(a - b) > 10 * (tol + tol * np.abs(b))))
            assert changed[k] >= TRACE_MIN_CHANGED, (name, k, changed[k])
        data["iv_eps"] = TRACE_EPS
        data["changed_adv"], data["changed_cadv"] = changed["adv"], changed["cadv"]
        print(name, "rows/step", data["n_rows"].tolist(), "samples", int(data["poolm_batch_size"]),
              "changed adv %.3f cadv %.3f" % (changed["adv"], changed["cadv"]))
        save(out, name, data)


if __name__ == "__main__":
    mg.install_stubs()
    gen_cumsum(HERE)
    gen_buffer(HERE)
    gen_traces(HERE)
