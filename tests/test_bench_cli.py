"""bench.py's command line: a plain run measures the headline rollout only (--full adds the sub-measurements), and
--dump-outputs writes a fixed, seeded sample of the last timed step's get() list as float32 / float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import importlib
    return importlib.import_module("bench")


def _fake_get_list(n, D=29, A=8, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    dims = [D, A, 0, 0, 0, 0, 0, 0, 0, 0, A, A]
    return [torch.randn((n, d) if d else (n,), generator=g) for d in dims]


def test_full_is_off_by_default_and_steps_must_be_positive():
    bench = _bench()
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full is True
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_is_a_fixed_sample_of_the_get_list(tmp_path):
    bench = _bench()
    n = 200000
    res = _fake_get_list(n)
    bench.dump_outputs(str(tmp_path / "a"), n, res)
    bench.dump_outputs(str(tmp_path / "b"), n, res)
    names = list(bench.OUTPUT_NAMES) + ["sample_index", "samples_added"]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in names)
    total = 0
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert idx.dtype == np.float64 and len(idx) == bench.DUMP_ROWS
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    rows = idx.astype(np.int64)
    for k, name in enumerate(names):
        x = np.load(tmp_path / "a" / (name + ".npy"))
        assert x.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(x, np.load(tmp_path / "b" / (name + ".npy")))       # same arguments, same files
        if k < len(res):
            np.testing.assert_array_equal(x, res[k].numpy()[rows])
        total += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "samples_added.npy")[0] == n


def test_dump_outputs_stays_under_the_size_cap_for_wide_tasks_and_keeps_small_phases_whole(tmp_path):
    bench = _bench()
    n = 400000
    bench.dump_outputs(str(tmp_path / "wide"), n, _fake_get_list(n, D=376, A=17))
    total = sum(os.path.getsize(tmp_path / "wide" / f) for f in os.listdir(tmp_path / "wide"))
    assert total <= 64 << 20
    res = _fake_get_list(1000)
    bench.dump_outputs(str(tmp_path / "small"), 1000, res)
    np.testing.assert_array_equal(np.load(tmp_path / "small" / "obs.npy"), res[0].numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "small" / "sample_index.npy"), np.arange(1000))


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_full_adds_the_rest(tmp_path):
    """A small plain run: the result line's headline fields, no sub-measurements, the dump; then --full (without the
    update / training / sub-configs / CPU baseline parts) adds the events phase's roofline and get() entries."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    common = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--branches", "3000", "--maxroll", "6"]

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + extra, capture_output=True,
                           text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])

    out = run(["--dump-outputs", str(tmp_path / "d")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"]["samples_per_step"] == 3000 * 5
    assert not {"roofline", "gae_get", "cpo_update", "ensemble_train", "configs", "cpu_baseline"} & set(out)
    obs = np.load(tmp_path / "d" / "obs.npy")
    assert obs.dtype == np.float32 and obs.shape == (3000 * 5, 29) and np.isfinite(obs).all()
    assert np.load(tmp_path / "d" / "samples_added.npy")[0] == 3000 * 5

    full = run(["--full", "--no-extras"])
    assert full["roofline"] is not None and full["gae_get"] is not None
