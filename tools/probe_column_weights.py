"""What column / class weights cost in the training step, and what the class weight buys in the trainer.
  --step     the dynamics ensemble's training step, 7 x (37 -> 512 -> 512 -> 64), batch 2048, 'MSPE' and 'NLL': HIP events around
             one cmbpo_trainer_epoch of STEPS steps, the configurations taken in turn (alternating rounds in alternating order,
             the first DROP thrown away, three trainers per configuration taken in turn):
             (a) here: the step with column and class weights attached against the plain step;
             (b) with --other-lib PATH (the parent commit's libcmbpo_hip.so): the plain step there against the plain step here
                 -- a step without weights must not pay for them; the yardstick is the other library's own (max - min) / median.
                 Both trainers start from the same weights and see the same batches: their weights afterwards are compared
                 bit for bit.  A second set of plain trainers of this tree is timed with them: what it differs by from the
                 first is what two sets of buffers differ by, whatever the code.
             (c) with --other-lib too: the weighted step there (other_weighted) against the weighted step here, judged and
                 compared bit for bit in the same way.
  --trainer  recall and false-alarm rate of the termination head at h = 1 after two epochs on the box point mass of
             tests/test_term_head_cmbpo_gpu.py, seeds 0 / 1 / 2, with m_term_pos_weight 1 and 'balanced', REPEATS times each.
    python tools/probe_column_weights.py [out.json] [--step] [--trainer] [--other-lib PATH]"""
import argparse
import contextlib
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib

DROP, INST = 2, 3


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def alternate(fns, rounds):
    """{name: [figure per round]}: the configurations in turn, every other round in reverse order (whoever runs first after the
    host's wait pays for it), DROP rounds thrown away."""
    got = {k: [] for k in fns}
    for rnd in range(DROP + rounds):
        for k, fn in (list(fns.items())[::-1] if rnd & 1 else fns.items()):
            x = fn()
            if rnd >= DROP:
                got[k].append(x)
    return got


@contextlib.contextmanager
def library(handle):
    """Every call of the package goes through _lib.lib(): objects made under a handle are used under it."""
    before, _lib._lib = _lib._lib, handle
    try:
        yield
    finally:
        _lib._lib = before


def other_library(path):
    """Another build of the library (the parent commit's libcmbpo_hip.so), bound like this tree's."""
    other = C.CDLL(os.path.abspath(path))
    for name, (r, a) in _lib.SIGNATURES.items():
        if hasattr(other, name):
            fn = getattr(other, name)
            fn.restype, fn.argtypes = r, a
    return other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--other-lib")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=4, help="--trainer: runs per (seed, weight)")
    ap.add_argument("--steps", type=int, default=400)      # 0.1 s per timed window
    args = ap.parse_args()
    res = dict(command="python tools/probe_column_weights.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0))

    if args.step:
        from cmbpo_amd.pens import PE
        E, I, H, D, B = 7, 37, 512, 32, 2048
        here = _lib.lib()
        libs = {"here": here}
        if args.other_lib:
            libs["other"] = other_library(args.other_lib)
        n = B * args.steps
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn(n, I, device="cuda", generator=g)
        t = torch.randn(n, D, device="cuda", generator=g)
        t[:, -2] = (torch.rand(n, device="cuda", generator=g) < 0.1).float()
        t[:, -1] = (torch.rand(n, device="cuda", generator=g) < 0.3).float()
        idx = torch.randint(0, n, (E, n), dtype=torch.int32, device="cuda", generator=g)
        cw = np.random.RandomState(1).uniform(0.5, 4.0, D).astype(np.float32)
        step, keep = {}, []
        for loss in ("MSPE", "NLL"):
            made = {}

            def make(lib_name, weighted):
                # INST trainers per configuration, taken in turn: two trainers of the same library differ by a few per cent (their
                # buffers lie elsewhere), more than one trainer differs from itself between rounds
                inst = []
                for _ in range(INST):
                    with library(libs[lib_name]):
                        pe = PE(I, D, hidden_dims=(H, H), num_networks=E, num_elites=5, loss=loss, use_scaler_in=True, use_scaler_out=True,
                                device="cuda:0", lr=1e-3, decay=1e-6, col_weight=cw if weighted else None,
                                pos_weight={-2: 7.0, -1: 3.0} if weighted else None)
                        pe.init_weights(np.random.RandomState(2))
                        inst.append((pe, pe._ensure_trainer(B)))
                    keep.append((lib_name, pe))
                made[(lib_name, weighted)] = inst[0][0]
                calls = [0]

                def run():
                    tr = inst[calls[0] % INST][1]
                    calls[0] += 1
                    with library(libs[lib_name]):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        tr.epoch(x, t, idx, B)
                        e1.record()
                        e1.synchronize()
                    return e0.elapsed_time(e1) * 1e3 / args.steps
                return run
            # here_plain_again: a second set of trainers of the same code, the yardstick for what a set's placement alone does
            fns = {"here_plain": make("here", False), "here_weighted": make("here", True), "here_plain_again": make("here", False)}
            if args.other_lib:
                fns = {"other_plain": make("other", False), "other_weighted": make("other", True), **fns}
            us = alternate(fns, args.rounds)
            k = dict(us_per_step=us, weighted_over_plain=statistics.median(us["here_weighted"]) / statistics.median(us["here_plain"]),
                     here_spread=spread(us["here_plain"]),
                     second_set_over_first_same_code=statistics.median(us["here_plain_again"]) / statistics.median(us["here_plain"]))
            with library(here):
                assert made[("here", False)]._trainer.f16_paths == made[("here", True)]._trainer.f16_paths == 3
            if args.other_lib:
                with library(here):
                    mine = made[("here", False)].get_weights()
                with library(libs["other"]):
                    theirs = made[("other", False)].get_weights()
                same = all(np.array_equal(a, b) for a, b in zip(mine[0] + mine[1], theirs[0] + theirs[1]))
                sp = spread(us["other_plain"])
                ratio = statistics.median(us["here_plain"]) / statistics.median(us["other_plain"])
                k.update(weights_bit_identical_to_other_lib_after_all_rounds=bool(same), other_spread=sp,
                         median_ratio_here_over_other=ratio, within_other_spread=bool(abs(ratio - 1.0) <= sp))
                print("%s (b) plain step here / other: %.4f (other's own spread %.4f) -> %s; weights bit-identical: %s"
                      % (loss, ratio, sp, "within" if k["within_other_spread"] else "OUTSIDE", same))
                # (c) the same for the weighted step of the two libraries
                with library(here):
                    mine = made[("here", True)].get_weights()
                with library(libs["other"]):
                    theirs = made[("other", True)].get_weights()
                same = all(np.array_equal(a, b) for a, b in zip(mine[0] + mine[1], theirs[0] + theirs[1]))
                sp = spread(us["other_weighted"])
                ratio = statistics.median(us["here_weighted"]) / statistics.median(us["other_weighted"])
                k["other_weighted"] = dict(weights_bit_identical_to_other_lib_after_all_rounds=bool(same), other_spread=sp,
                                      median_ratio_here_over_other=ratio, within_other_spread=bool(abs(ratio - 1.0) <= sp))
                print("%s (c) weighted step here / other: %.4f (other's own spread %.4f) -> %s; weights bit-identical: %s"
                      % (loss, ratio, sp, "within" if k["other_weighted"]["within_other_spread"] else "OUTSIDE", same))
            print("%s     a second set of plain trainers of this tree / the first: %.4f" % (loss, k["second_set_over_first_same_code"]))
            print("%s (a) weighted step / plain step, here: %.4f (%.1f us / %.1f us)"
                  % (loss, k["weighted_over_plain"], statistics.median(us["here_weighted"]), statistics.median(us["here_plain"])))
            step[loss] = k
        for lib_name, pe in keep:       # every handle goes back to the library that made it
            with library(libs[lib_name]):
                pe._trainer.__del__()
                pe.mlp.__del__()
        res["step"] = dict(E=E, I=I, H=H, D=D, batch=B, steps_per_epoch_call=args.steps, rounds=args.rounds, dropped_rounds=DROP,
                           trainers_per_configuration=INST, **step)

    if args.trainer:
        from test_column_weights_cmbpo_gpu import column_weight_keys
        from test_term_head_cmbpo_gpu import head_figures, run_box_loop
        runs = []
        for repeat in range(args.repeats):       # (the loop is not bitwise repeatable: the repeats show by how much)
            for seed in (0, 1, 2):
                for weight in (1.0, 'balanced'):
                    t0 = time.perf_counter()
                    with column_weight_keys(m_term_pos_weight=weight):
                        algo, seen, diags = run_box_loop(True, seed=seed)
                    recall, false_alarm, pos, neg = head_figures(algo)
                    runs.append(dict(repeat=repeat, seed=seed, m_term_pos_weight=weight,
                                     term_pos_weight_logged=diags[-1].get('model/term_pos_weight'), recall_h1=float(recall),
                                     false_alarm_h1=float(false_alarm), real_terminations=pos, real_continuations=neg,
                                     target_share=seen["term_share"][-1], seconds=time.perf_counter() - t0))
                    print(runs[-1])
        gains = [[runs[6 * r + 2 * s + 1]["recall_h1"] - runs[6 * r + 2 * s]["recall_h1"] for s in range(3)] for r in range(args.repeats)]
        alarms = [[runs[6 * r + 2 * s + 1]["false_alarm_h1"] for s in range(3)] for r in range(args.repeats)]
        res["trainer"] = dict(runs=runs, recall_gain_h1=gains, smallest_recall_gain_h1_per_seed=[min(g[s] for g in gains) for s in range(3)],
                              largest_false_alarm_h1_per_seed=[max(a[s] for a in alarms) for s in range(3)],
                              gain_positive_on_all_seeds=bool(min(min(g) for g in gains) > 0))
        print("recall gain at h = 1, seeds 0 / 1 / 2, per repeat:", gains)

    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
