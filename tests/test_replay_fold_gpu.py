"""GPU: the one fold kernel behind the five `*_finish` entries of the model replay.

For each table the partials are filled through the single-step entries on made-up prediction arrays (no model), the table's
`*_finish` entry is called, and `sums` / `counts` are held byte for byte against a NumPy fold of the downloaded `part_sum` /
`part_cnt` in slot order -- a Python loop `s = s + p[:, k]` in float64 / int64, the order that makes a table's bits.  Shapes:
H = 2 with horizon 1 never stepped (it must come out as the fold of its zero partials: zeros); B = 129 windows, three slots, the
last with one row; obs_dim = 29, where the calibration table has 180 + 122 = 302 > 256 entries, a second trip of the entry loop;
two reliability columns of 15 bins; the vote table, which has no sums; the particle table at S = 2, B = 65, obs_dim = 29 (three
slots) and at S = 64, B = 3, obs_dim = 3 (18 + 262 entries)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
F32, U8 = np.float32, np.uint8
H = 2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _fold(part, dtype):
    p = part.cpu().numpy()
    assert p.dtype == dtype and p.ndim == 3 and p.shape[0] == H
    s = np.zeros((H, p.shape[2]), dtype)
    for k in range(p.shape[1]):
        s = s + p[:, k]
    return s


def _check(arrays, where, n_part, n_sums, n_counts):
    """arrays: a dict with part_cnt / counts and, for n_sums > 0, part_sum / sums."""
    pairs = [("part_cnt", "counts", np.int64, n_counts)] + ([("part_sum", "sums", np.float64, n_sums)] if n_sums else [])
    for part, table, dtype, n in pairs:
        assert tuple(arrays[part].shape) == (H, n_part, n), (where, part, tuple(arrays[part].shape))
        want, got = _fold(arrays[part], dtype), arrays[table].cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype, (where, table)
        np.testing.assert_array_equal(got.view(U8), want.view(U8), err_msg=f"{where}: {table}")
        assert got[0].any(), f"{where}: {table} of the stepped horizon is empty"
        assert not got[1].view(U8).any(), f"{where}: {table} of the horizon that was never stepped"
        arrays[table].fill_(1)          # (so that the zeros above were written by the fold)


def _recording(rng, B, D):
    return dict(next_obs=rng.standard_normal((H, B, D)).astype(F32), rew=rng.standard_normal((H, B)).astype(F32),
                cost=(rng.random((H, B)) < 0.4).astype(F32), term=(rng.random((H, B)) < 0.2).astype(U8))


def _predictions(rng, rec0, R, D, reps):
    """One step's prediction arrays for R rows: the recording of horizon 0 (each window `reps` times) plus noise."""
    return dict(next_obs=(np.repeat(rec0, reps, axis=0) + rng.standard_normal((R, D)) * 0.3).astype(F32),
                rew=rng.standard_normal(R).astype(F32), cost=rng.random(R).astype(F32), term=(rng.random(R) < 0.2).astype(U8),
                ep_var_mean=rng.random(R).astype(F32), dkl_path=rng.random(R).astype(F32))


def test_fold_of_the_plain_calibration_reliability_and_vote_tables(hip_lib):
    _need_gpu()
    from cmbpo_amd import _lib
    from cmbpo_amd.replay import ReplayBuffers
    rng = np.random.default_rng(30)
    B, D, A, E = 129, 29, 2, 3
    O = D + 1
    rec = _recording(rng, B, D)
    rb = ReplayBuffers(rng.standard_normal((B, D)).astype(F32), np.zeros((H, B, A), F32), rec["next_obs"], rec["rew"], rec["cost"],
                       rec["term"], mode="one_step", ensemble=E, out_dim=O, device=DEV, calibration=True, votes=dict(),
                       reliability=dict(columns=[dict(name="a", col=D, target="cost"), dict(name="b", col=D - 1, target="term")], bins=15))
    assert rb.n_part == 3
    rb.set_elite(rng.integers(0, E, (H, B)).astype(np.int32))
    pred = _predictions(rng, rec["next_obs"][0], B, D, 1)
    pred["next_obs"][5, 3] = np.nan                 # one row for n_nonfinite
    for k, v in pred.items():
        rb.step_outputs()[k].copy_(torch.from_numpy(v))
    rb.t["mean"].copy_(torch.from_numpy((rng.standard_normal((E, B, O)) * 0.3).astype(F32)))
    rb.t["var"].copy_(torch.from_numpy(np.exp(rng.uniform(-6.0, 2.0, (E, B, O))).astype(F32)))
    rb.v["done_votes"].copy_(torch.from_numpy(rng.integers(0, E + 1, B).astype(U8)))
    rb.v["cost_votes"].copy_(torch.from_numpy(rng.integers(0, E + 1, B).astype(U8)))
    rb.calibrate(0)
    rb.reliab(0)
    rb.votes(0)
    rb.compare(0)                                   # (last: it clears `alive`)
    for _ in range(2):                              # the second pass: the tables start from ones, the fold overwrites them
        rb.finish()
        rb.calib_finish()
        rb.reliab_finish()
        rb.votes_finish()
        torch.cuda.synchronize()
        _check(rb.t, "plain", 3, D + _lib.REPLAY_SCALAR_SUMS, _lib.REPLAY_COUNTS)
        _check(rb.c, "calibration", 3, 6 * O, 4 * O + 2)
        _check(rb.r, "reliability", 3, 2 * 2 * (2 * 15 + 2), 2 * 2 * 2 * 15 + 2 * 2)
        _check(rb.v, "votes", 3, 0, _lib.REPLAY_VOTE_COUNTS)


@pytest.mark.parametrize("S,B,D", [(2, 65, 29), (64, 3, 3)])
def test_fold_of_the_particle_table(hip_lib, S, B, D):
    _need_gpu()
    from cmbpo_amd.replay import ParticleBuffers
    rng = np.random.default_rng(31 + S)
    R = B * S
    rec = _recording(rng, B, D)
    pb = ParticleBuffers(S, rng.standard_normal((B, D)).astype(F32), np.zeros((H, B, 2), F32), rec["next_obs"], rec["rew"], rec["cost"],
                         rec["term"], mode="one_step", device=DEV)
    assert pb.n_part == 3
    for k, v in _predictions(rng, rec["next_obs"][0], R, D, S).items():
        pb.step_outputs()[k].copy_(torch.from_numpy(v))
    pb.particles(0)
    for _ in range(2):
        pb.finish()
        torch.cuda.synchronize()
        _check(pb.t, "particles S = %d" % S, 3, 4 * (D + 1) + 2, (D + 1) * (S + 1) + 2)
