"""Is the ensemble training step of another build of the library (the parent commit's libcmbpo_hip.so) the step of this tree,
bit for bit?  For every configuration, under both libraries: the same seeded weights and batches, two steps, one `losses` call
on a shared holdout list; the weights, the biases and both Adam moments are compared bit for bit, `self.loss` to one float32 ulp
(its float64 atomics may reorder, which is far below a float32 ulp before the final rounding).  The configurations are the
tests' own smallest shapes, so every path is hit:
  the SHAPES of tests/test_column_weights_gpu.py, each plain, with column and class weights ("both") and with the logistic
  columns tests/test_logistic_head_gpu.py gives the same shape;
  the FIRST_STEP_CASES of tests/test_value_clip_gpu.py, each plain, weighted, clipped, and weighted plus clipped.
One line per configuration and mode; exit status 1 on any mismatch.
    python tools/probe_train_parity.py [out.json] --other-lib PATH"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib
from probe_column_weights import library, other_library

import test_column_weights_gpu as tcw
import test_logistic_head_gpu as tlh
import test_value_clip_gpu as tvc

STEPS = 2


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()


def state_and_loss(pe, batch, x, t, idxs, hold, **extras):
    """STEPS steps, then `self.loss` on the holdout rows: ([W, b, m, v tensors], losses[E])."""
    tr = pe._ensure_trainer(batch)
    xd, td = dev(x), dev(t)
    for idx in [dev(i) for i in idxs]:
        tr.step(xd, td, idx.data_ptr(), batch, batch, **extras)
    loss_extras = {"weights": extras["weights"]} if extras.get("weights") is not None else {}
    losses = tr.losses(xd, td, dev(hold), 0, hold.shape[0], **loss_extras).cpu().numpy()
    state = [a for k in (tr.get_weights(), tr.get_moments(0), tr.get_moments(1)) for part in k for a in part]
    pe._trainer.__del__()
    pe.mlp.__del__()
    return state, losses


def dynamics(i, how):
    """Shape i of the column-weight tests: (name, make) with make() -> (state, losses) under the current library."""
    E, I, H, D, loss, batch, _ = tcw.SHAPES[i]
    cols = tlh.SHAPES[i][7] if how == "logistic" else ()

    def make():
        _, pe, _, x, t, _, _ = tlh._make(E, I, H, D, loss, 300, seed=23, cols=cols, mode="both" if how == "weighted" else None)
        rng = np.random.RandomState(5)
        idxs = [rng.randint(0, x.shape[0], size=(E, batch)).astype(np.int32) for _ in range(STEPS)]
        return state_and_loss(pe, batch, x, t, idxs, rng.permutation(x.shape[0])[:157].astype(np.int32))
    return "%s %s" % (tcw._ID(tcw.SHAPES[i]), how), make


def value(case, how):
    """A first-step case of the value-clip tests; the old predictions are the targets plus noise of the targets' own size."""
    E, I, H, D, batch = case
    use_w, use_old = how in ("weighted", "weighted+clipped"), how in ("clipped", "weighted+clipped")

    def make():
        rng = np.random.RandomState(1000 * E + I + H)
        N = E * batch
        ws, bs, x, t, sc_in, sc_out = tvc._weights_and_data(rng, E, I, H, D, N)
        w = tvc._sample_weights(rng, N)
        old = (t + np.sqrt(sc_out[1]) * rng.standard_normal(t.shape)).astype(np.float32)
        idxs = [rng.randint(0, N, size=(E, batch)).astype(np.int32) for _ in range(STEPS)]
        pe = tvc._make_pe(E, I, H, D, ws, bs, sc_in, sc_out, clip_loss=True, weighted=True)
        return state_and_loss(pe, batch, x, t, idxs, rng.permutation(N)[:min(157, N)].astype(np.int32),
                              weights=dev(w) if use_w else None, old_pred=dev(old) if use_old else None, kl_cliprange=0.1)
    return "MSE %dx%d-%d-%d-b%d %s" % (E, I, H, D, batch, how), make


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--other-lib", required=True)
    args = ap.parse_args()
    libs = {"here": _lib.lib(), "other": other_library(args.other_lib)}
    configs = [dynamics(i, how) for i in range(len(tcw.SHAPES)) for how in ("plain", "weighted", "logistic")]
    configs += [value(c, how) for c in tvc.FIRST_STEP_CASES for how in ("plain", "weighted", "clipped", "weighted+clipped")]
    rows, bad = [], 0
    for name, make in configs:
        got = {}
        for which, handle in libs.items():
            with library(handle):
                got[which] = make()
        (s_here, l_here), (s_other, l_other) = got["here"], got["other"]
        same = len(s_here) == len(s_other) and all(np.array_equal(a, b) for a, b in zip(s_here, s_other))
        moved = any(float(np.abs(a).max()) > 0 for a in s_here[6:12])       # (the first moments are not all zero)
        ulps = int(np.abs(l_here.view(np.int32).astype(np.int64) - l_other.view(np.int32).astype(np.int64)).max())
        ok = same and moved and ulps <= 1 and bool(np.isfinite(l_here).all())
        bad += not ok
        rows.append(dict(config=name, state_bit_identical=bool(same), gradients_nonzero=bool(moved), self_loss_ulps=ulps, ok=bool(ok)))
        print("%-48s weights, biases, Adam moments: %s; self.loss: %d ulp%s" % (
            name, "bit-identical" if same else "DIFFERENT", ulps, "" if ok else "   <-- MISMATCH"))
    res = dict(command="python tools/probe_train_parity.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0),
               steps=STEPS, rows=rows, mismatches=bad)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
