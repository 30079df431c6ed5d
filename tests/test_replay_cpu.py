"""CPU: open-loop model validation without a device -- the NumPy specification tests/replay_ref.py on cases small
enough to verify by eye, the result table's means, CPOBuffer.windows on archives of toy paths, and the C-ABI of the four
cmbpo_replay_* entry points (exports, header against binding, argument refusals before any HIP call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import replay_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------
# 1. the specification, by eye
# ------------------------------------------------------------------------------------------------------------------
def _hand_case(nan_row=None):
    """3 windows x 3 steps x 2 columns.  The model adds 1 to every column; the world adds 1 and, to column 0, 0.5 more.
    Window 0 has one real step; window 1's recording ends with a terminal at h = 1; the model predicts a termination for
    window 2 at h = 1."""
    obs0 = np.array([[0.0, 10.0], [1.0, 11.0], [2.0, 12.0]], np.float32)
    H, B = 3, 3
    real_next = np.zeros((H, B, 2), np.float32)
    x = obs0.copy()
    for h in range(H):
        x = x + np.float32(1.0)
        x[:, 0] += np.float32(0.5)
        real_next[h] = x
    rec = dict(next_obs=real_next,
               rew=np.array([[1.0, 1.0, 1.0], [1.0, 3.0, 1.0], [1.0, 1.0, 1.0]], np.float32),
               cost=np.array([[0.0, 1.0, 1.0], [0.0, 0.0, 2.0], [0.0, 0.0, 0.0]], np.float32),
               term=np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.uint8))
    p_cost = np.array([[0.0, 0.6, 0.4], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], np.float32)
    p_term = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 0]], np.uint8)

    def step(h, cur):
        nxt = cur + np.float32(1.0)
        rew = np.ones(B, np.float32)
        if nan_row is not None and h == nan_row[0]:
            nxt = nxt.copy()
            if nan_row[2] == "obs":
                nxt[nan_row[1], 1] = np.nan
            elif nan_row[2] == "rew":
                rew[nan_row[1]] = np.inf
        return dict(next_obs=nxt, rew=rew, cost=p_cost[h].copy(), term=p_term[h].copy(),
                    ep_var_mean=np.full(B, 0.5, np.float32), dkl_path=np.full(B, 0.25, np.float32))

    return obs0, rec, np.array([1, 3, 3], np.int32), step


def test_spec_open_loop_by_eye():
    obs0, rec, lengths, step = _hand_case()
    tab, cur, alive = ref.replay(step, obs0, rec, lengths, ref.OPEN_LOOP)
    # h = 0: all three; window 0 ends by its length.  h = 1: windows 1 and 2; one ends by the recorded terminal, the other by
    # the predicted one.  h = 2: nobody.
    np.testing.assert_array_equal(tab["n"], [3, 2, 0])
    np.testing.assert_array_equal(tab["n_nonfinite"], [0, 0, 0])
    assert not alive.any()
    # the model's own output is fed back: it misses 0.5 in column 0 at h = 0 and 1.0 at h = 1, nothing in column 1
    np.testing.assert_array_equal(tab["se_obs"], [[3 * 0.25, 0.0], [2 * 1.0, 0.0], [0.0, 0.0]])
    np.testing.assert_array_equal(tab["se_rew"], [0.0, 4.0, 0.0])                 # window 1 at h = 1: 1 against 3
    e =np.float32(0.6) - np.float32(1.0), np.float32(0.4) - np.float32(1.0)
    np.testing.assert_array_equal(tab["se_cost"], [float(e[0]) ** 2 + float(e[1]) ** 2, 1.0, 0.0])
    np.testing.assert_array_equal(tab["sum_ep_var"], [1.5, 1.0, 0.0])
    np.testing.assert_array_equal(tab["sum_dkl"], [0.75, 0.5, 0.0])
    # [real, predicted]: h = 0 one quiet step, one hit (0.6 > 0.5), one miss (0.4); h = 1 one quiet, one hit
    np.testing.assert_array_equal(tab["cost_cm"], [[[1, 0], [1, 1]], [[1, 0], [0, 1]], [[0, 0], [0, 0]]])
    np.testing.assert_array_equal(tab["term_cm"], [[[3, 0], [0, 0]], [[0, 1], [1, 0]], [[0, 0], [0, 0]]])
    # frozen where they died: window 0 never moved, windows 1 and 2 hold the h = 0 prediction
    np.testing.assert_array_equal(cur, [[0.0, 10.0], [2.0, 12.0], [3.0, 13.0]])
    m = ref.means(tab)
    np.testing.assert_array_equal(m["mse_obs"][:2], [[0.25, 0.0], [1.0, 0.0]])
    assert np.isnan(m["mse_obs"][2]).all() and np.isnan(m["mse_rew"][2]) and np.isnan(m["ep_var_mean"][2])


def test_spec_one_step_by_eye():
    obs0, rec, lengths, step = _hand_case()
    tab, cur, alive = ref.replay(step, obs0, rec, lengths, ref.ONE_STEP)
    # the predicted termination of window 2 at h = 1 is counted and does not end it
    np.testing.assert_array_equal(tab["n"], [3, 2, 1])
    np.testing.assert_array_equal(tab["term_cm"], [[[3, 0], [0, 0]], [[0, 1], [1, 0]], [[1, 0], [0, 0]]])
    # teacher-forced: every step starts from the real observation, the error does not compound
    np.testing.assert_array_equal(tab["se_obs"], [[0.75, 0.0], [0.5, 0.0], [0.25, 0.0]])
    np.testing.assert_array_equal(alive, [False, False, False])                    # h + 1 == len ends window 2 after h = 2
    np.testing.assert_array_equal(cur, [[0.0, 10.0], rec["next_obs"][0, 1], rec["next_obs"][1, 2]])


@pytest.mark.parametrize("where", ["obs", "rew"])
@pytest.mark.parametrize("mode", [ref.OPEN_LOOP, ref.ONE_STEP])
def test_spec_nonfinite_row_counts_once_and_nowhere_else(mode, where):
    obs0, rec, lengths, step = _hand_case(nan_row=(0, 1, where))
    tab, cur, alive = ref.replay(step, obs0, rec, lengths, mode)
    clean = ref.replay(_hand_case()[3], obs0, rec, lengths, mode)[0]
    np.testing.assert_array_equal(tab["n_nonfinite"], [1, 0, 0])
    np.testing.assert_array_equal(tab["n"], clean["n"] - [1, 1, 0])              # window 1 is gone from h = 0 on
    for k, v in tab.items():
        assert np.isfinite(v).all(), k
    np.testing.assert_array_equal(tab["se_obs"][0], [2 * 0.25, 0.0])
    np.testing.assert_array_equal(tab["cost_cm"][0], [[1, 0], [1, 0]])            # window 1's hit is not counted
    np.testing.assert_array_equal(cur[1], obs0[1])                                  # and its state never moved


def test_table_means_and_empty_horizons():
    from cmbpo_amd import replay
    D = 3
    sums = np.zeros((2, D + 4))
    counts = np.zeros((2, 10), np.int64)
    sums[0] = [2.0, 4.0, 6.0, 8.0, 10.0, 1.0, 3.0]
    counts[0] = [2, 1, 1, 0, 0, 1, 2, 0, 0, 0]
    t = replay.table(sums, counts, D)
    np.testing.assert_array_equal(t["n"], [2, 0])
    np.testing.assert_array_equal(t["n_nonfinite"], [1, 0])
    np.testing.assert_array_equal(t["mse_obs"][0], [1.0, 2.0, 3.0])
    assert (t["mse_rew"][0], t["mse_cost"][0], t["ep_var_mean"][0], t["dkl_mean"][0]) == (4.0, 5.0, 0.5, 1.5)
    np.testing.assert_array_equal(t["cost_cm"][0], [[1, 0], [0, 1]])
    np.testing.assert_array_equal(t["term_cm"][0], [[2, 0], [0, 0]])
    for k in ("mse_obs", "mse_rew", "mse_cost", "ep_var_mean", "dkl_mean"):
        assert np.isnan(t[k][1]).all(), k
    assert not t["cost_cm"][1].any() and not t["term_cm"][1].any()
    for k in ("se_obs", "se_rew", "se_cost", "sum_ep_var", "sum_dkl"):
        assert k in t


# ------------------------------------------------------------------------------------------------------------------
# 2. CPOBuffer.windows
# ------------------------------------------------------------------------------------------------------------------
PATHS = (1, 4, 9)


def host_only_buffer(size, archive_size, D=3, A=2):
    """A CPOBuffer whose two device steps (the GAE of finish_path, the advantage normalisation of get) are left out: the
    advantage columns stay zero, every column windows() reads is what the real buffer archives.  The GPU suite runs the same
    checks through the real store / finish_path / get."""
    import toyworld
    from cmbpo_amd.cpobuffer import CPOBuffer

    class HostOnly(CPOBuffer):
        def finish_path(self, last_val=0, last_cval=0):
            self.path_start_idx, self.path_finished = self.ptr, True

        def get(self):
            self.dump_to_archive()
            self.reset_buffers()

    buf = HostOnly(size, archive_size, toyworld.Space(D), toyworld.Space(A), device="cpu")
    buf.initialize({"mu": [A], "log_std": [A]})
    return buf


def fill_paths(buf, lengths, epoch, tag, terminal_last=True, D=3, A=2):
    """Store one path per entry of `lengths`: consecutive steps share an observation (next_obs[i] is obs[i + 1]); the last
    step of a path is a terminal, or (terminal_last False) a time-out whose successor starts somewhere else."""
    for p, L in enumerate(lengths):
        x = np.full(D, 100.0 * tag + 10.0 * p, np.float32)
        for s in range(L):
            nxt = x + np.float32(1.0)
            buf.store(x, np.full(A, s, np.float32), nxt, float(s), 0.0, float(s % 2), 0.0, 0.0,
                      {"mu": np.zeros(A, np.float32), "log_std": np.zeros(A, np.float32)},
                      bool(terminal_last and s == L - 1), epoch)
            x = nxt
        buf.finish_path()
    buf.get()


def check_windows(buf, H, n, epochs, rng_seed, path_of):
    """The properties every window must have; path_of[i] = id of the path archive slot i belongs to."""
    start, length, w = buf.windows(H, n, epochs=epochs, rng=np.random.default_rng(rng_seed))
    a = buf.arch_dict
    assert start.shape == (n,) and length.shape == (n,) and w["lengths"] is length
    assert w["actions"].shape[:2] == (H, n) and w["next_obs"].shape == (H, n, a["observations"].shape[1])
    assert w["rewards"].shape == w["costs"].shape == w["terminals"].shape == (H, n)
    for j in range(n):
        s, L = int(start[j]), int(length[j])
        ids = path_of[s:s + L]
        assert 1 <= L <= H and (ids == ids[0]).all()                       # no window crosses a path end
        assert not a["terminals"][s:s + L - 1].any()                       # ... or a terminal
        remaining = int((path_of[s:] == path_of[s]).cumprod().sum())
        assert L == min(H, remaining)
        np.testing.assert_array_equal(w["obs0"][j], a["observations"][s])
        for h in range(H):
            i = s + min(h, L - 1)                                          # behind the length: the last real step again
            np.testing.assert_array_equal(w["next_obs"][h, j], a["next_observations"][i])
            np.testing.assert_array_equal(w["actions"][h, j], a["actions"][i])
            assert w["rewards"][h, j] == a["rewards"][i] and w["costs"][h, j] == a["costs"][i]
            assert w["terminals"][h, j] == a["terminals"][i]
        if epochs is not None:
            assert a["epochs"][s] in epochs
    return start, length


@pytest.mark.parametrize("terminal_last", [True, False], ids=["terminals", "timeouts"])
def test_windows_respect_paths_lengths_epochs_and_rng(terminal_last):
    buf = host_only_buffer(32, 200)
    fill_paths(buf, PATHS, epoch=0, tag=0, terminal_last=terminal_last)
    fill_paths(buf, PATHS[::-1], epoch=1, tag=1, terminal_last=terminal_last)
    assert buf.arch_size == 28
    path_of = np.repeat(np.arange(6), PATHS + PATHS[::-1])
    cont = buf.path_continues()
    np.testing.assert_array_equal(cont, np.r_[path_of[1:] == path_of[:-1], False])
    for H in (1, 3, 5, 12):
        start, length = check_windows(buf, H, 400, None, 3, path_of)      # (a one-step path is missed once in 10^6 such draws)
        assert len(np.unique(path_of[start])) == 6                         # every path is drawn from, the short ones too
        assert (length < H).any() or H == 1                                # ... and kept with their length
    start, _ = check_windows(buf, 5, 40, [1], 4, path_of)
    assert (start >= 14).all()
    start, _ = check_windows(buf, 5, 40, [0], 4, path_of)
    assert (start < 14).all()
    # the same generator state gives the same windows; NumPy's global stream is not touched
    state = np.random.get_state()[1].copy()
    a = buf.windows(4, 16, rng=np.random.default_rng(9))
    b = buf.windows(4, 16, rng=np.random.default_rng(9))
    buf.windows(4, 16)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    for k in a[2]:
        np.testing.assert_array_equal(a[2][k], b[2][k], err_msg=k)
    np.testing.assert_array_equal(np.random.get_state()[1], state)
    with pytest.raises(ValueError, match="windows"):
        buf.windows(4, 8, epochs=[7])
    with pytest.raises(ValueError, match="windows"):
        buf.windows(0, 8)


def test_windows_never_join_newest_and_oldest_samples_of_a_wrapped_archive():
    import warnings
    buf = host_only_buffer(16, 40)
    # one long path per epoch, cut by the epoch's end and CONTINUED in the next (finish_all_paths(reset_path=False)): the
    # observations chain across the slabs, so only the pointer test separates the newest sample from the oldest behind it
    x = np.zeros(3, np.float32)
    for epoch in range(4):
        for s in range(12):
            nxt = x + np.float32(1.0)
            buf.store(x, np.zeros(2, np.float32), nxt, 0.0, 0.0, 0.0, 0.0, 0.0,
                      {"mu": np.zeros(2, np.float32), "log_std": np.zeros(2, np.float32)}, False, epoch)
            x = nxt
        buf.finish_path()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            buf.get()
        if epoch == 2:                                                      # three slabs in a row: one path of 36 steps
            np.testing.assert_array_equal(buf.path_continues(), np.r_[np.ones(35, bool), False])
    assert buf.archive_full and buf.archive_ptr == 12 and buf.arch_size == 36
    # slots 0..11 now hold steps 36..47; the step in front of slot 12 is step 11's slot, rewritten: make the chain hold there
    # bit for bit, as a path that happens to return to an old state would
    buf.arch_dict["next_observations"][11] = buf.arch_dict["observations"][12]
    cont = buf.path_continues()
    assert not cont[11] and cont[:11].all() and cont[12:35].all() and not cont[35]
    start, length, _ = buf.windows(30, 600, rng=np.random.default_rng(0))
    assert ((start + length <= 12) | (start >= 12)).all() and (start < 12).any() and (start >= 12).any()
    assert length.max() == 24


# ------------------------------------------------------------------------------------------------------------------
# 3. the C-ABI
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def _header():
    text = open(os.path.join(ROOT, "include", "cmbpo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


NAMES = ("cmbpo_replay_parts", "cmbpo_replay_compare", "cmbpo_replay_finish", "cmbpo_replay_run")


def test_library_exports_the_four_symbols(lib):
    from cmbpo_amd import _lib
    assert lib.cmbpo_version() == 6            # the parent's 5 plus one: one bump, not two
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    for B, want in ((-3, 0), (0, 0), (1, 1), (63, 1), (64, 1), (65, 2), (257, 5), (4099, 65)):
        assert lib.cmbpo_replay_parts(B) == want


def test_header_signatures_and_struct_image_agree():
    from cmbpo_amd import _lib
    text = _header()
    m = re.search(r"typedef struct cmbpo_replay \{(.*?)\} cmbpo_replay_t;", text, flags=re.S)
    assert m, "cmbpo_replay_t is not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = "pointer" if "*" in decl else "int32"
        assert kind == "pointer" or decl.startswith("int32_t"), decl
        names = re.sub(r"^(const\s+)?(float|double|int32_t|int64_t|uint8_t)", "", decl)
        fields += [(n.strip().lstrip("*").strip(), kind) for n in names.split(",")]
    image = [(n, "pointer" if t is C.c_void_p else "int32" if t is C.c_int32 else "?") for n, t in _lib.ReplayStruct._fields_]
    assert image == fields
    assert [n for n, _ in fields[:6]] == ["B", "H", "obs_dim", "act_dim", "mode", "reserved"] and len(fields) == 26
    S = _lib.ReplayStruct
    assert C.sizeof(S) == 184 and S.act.offset == 24 and S.cur_obs.offset == 72 and S.p_next_obs.offset == 88
    assert S.mean.offset == 136 and S.part_sum.offset == 152 and S.counts.offset == 176
    rp = C.POINTER(S)
    sig = _lib.SIGNATURES
    assert sig["cmbpo_replay_parts"] == (C.c_int, [C.c_int])
    assert sig["cmbpo_replay_compare"] == (C.c_int, [rp, C.c_int, C.c_void_p])
    assert sig["cmbpo_replay_finish"] == (C.c_int, [rp, C.c_void_p])
    assert sig["cmbpo_replay_run"] == (C.c_int, [rp, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p])
    assert re.search(r"int cmbpo_replay_parts\(int n_rows\);", text)
    assert re.search(r"int cmbpo_replay_compare\(const cmbpo_replay_t \*rp, int h, void \*stream\);", text)
    assert re.search(r"int cmbpo_replay_finish\(const cmbpo_replay_t \*rp, void \*stream\);", text)
    assert re.search(r"int cmbpo_replay_run\(const cmbpo_replay_t \*rp, cmbpo_mlp_t \*model, int task, int ensemble,\s*"
                     r"const int32_t \*d_elite,\s*void \*stream\);", text)
    assert (_lib.REPLAY_OPEN_LOOP, _lib.REPLAY_ONE_STEP, _lib.REPLAY_SCALAR_SUMS, _lib.REPLAY_COUNTS) == (0, 1, 4, 10)
    for name, val in (("OPEN_LOOP", 0), ("ONE_STEP", 1), ("SCALAR_SUMS", 4), ("COUNTS", 10)):
        assert re.search(r"#define CMBPO_REPLAY_%s %d\b" % (name, val), text)


COMPARE_ARRAYS = ("next_obs", "rew", "cost", "term", "len", "cur_obs", "alive", "p_next_obs", "p_rew", "p_term", "p_cost",
                  "p_dkl_path", "p_ep_var_mean", "part_sum", "part_cnt")
FINISH_ARRAYS = ("part_sum", "part_cnt", "sums", "counts")


def _image(**kw):
    """A descriptor whose every array points at host memory that is never read: each call below fails a check first."""
    from cmbpo_amd import _lib
    host = (C.c_double * 8)()
    rs = _lib.ReplayStruct()
    rs._keep = host
    rs.B, rs.H, rs.obs_dim, rs.act_dim, rs.mode = 5, 3, 11, 3, 0
    for n, t in _lib.ReplayStruct._fields_:
        if t is C.c_void_p:
            setattr(rs, n, C.cast(host, C.c_void_p).value)
    for k, v in kw.items():
        setattr(rs, k, v)
    return rs


def test_every_entry_refuses_bad_arguments_without_a_gpu(lib):
    fake = C.cast((C.c_double * 8)(), C.c_void_p)          # stands for a handle / an index array that is never reached

    def calls(rs):
        return (("cmbpo_replay_compare", lambda: lib.cmbpo_replay_compare(C.byref(rs), 0, None)),
                ("cmbpo_replay_finish", lambda: lib.cmbpo_replay_finish(C.byref(rs), None)),
                ("cmbpo_replay_run", lambda: lib.cmbpo_replay_run(C.byref(rs), fake, 0, 7, fake, None)))

    def refused(name, call, *words):
        assert call() == -1, name
        msg = lib.cmbpo_last_error()
        assert name.encode() in msg, msg
        for w in words:
            assert w in msg, msg

    for bad, word in ((dict(B=0), b"B 0"), (dict(B=-4), b"B -4"), (dict(H=0), b"H 0"), (dict(H=-1), b"H -1"),
                      (dict(mode=2), b"unknown mode 2"), (dict(mode=-1), b"unknown mode"), (dict(obs_dim=0), b"bad dims"),
                      (dict(obs_dim=513), b"bad dims"), (dict(act_dim=-1), b"bad dims"), (dict(reserved=1), b"reserved")):
        for name, call in calls(_image(**bad)):
            refused(name, call, word)
    assert lib.cmbpo_replay_compare(None, 0, None) == -1 and b"cmbpo_replay_compare" in lib.cmbpo_last_error()
    assert lib.cmbpo_replay_finish(None, None) == -1 and b"cmbpo_replay_finish" in lib.cmbpo_last_error()
    assert lib.cmbpo_replay_run(None, fake, 0, 7, fake, None) == -1 and b"cmbpo_replay_run" in lib.cmbpo_last_error()
    for k in COMPARE_ARRAYS:
        rs = _image(**{k: None})
        refused("cmbpo_replay_compare", lambda: lib.cmbpo_replay_compare(C.byref(rs), 0, None), b"NULL")
        refused("cmbpo_replay_run", lambda: lib.cmbpo_replay_run(C.byref(rs), fake, 0, 7, fake, None), b"NULL")
    for k in FINISH_ARRAYS:
        rs = _image(**{k: None})
        refused("cmbpo_replay_finish", lambda: lib.cmbpo_replay_finish(C.byref(rs), None), b"NULL")
        refused("cmbpo_replay_run", lambda: lib.cmbpo_replay_run(C.byref(rs), fake, 0, 7, fake, None), b"NULL")
    rs = _image()
    for h in (-1, 3, 4, 1 << 20):
        refused("cmbpo_replay_compare", lambda: lib.cmbpo_replay_compare(C.byref(rs), h, None), b"outside [0, 3)")
    # cmbpo_replay_run alone: the handle, the member indices, the arrays only it uses
    refused("cmbpo_replay_run", lambda: lib.cmbpo_replay_run(C.byref(rs), None, 0, 7, fake, None), b"model")
    refused("cmbpo_replay_run", lambda: lib.cmbpo_replay_run(C.byref(rs), fake, 0, 7, None, None), b"d_elite")
    for k in ("act", "mean", "var"):
        rk = _image(**{k: None})
        refused("cmbpo_replay_run", lambda: lib.cmbpo_replay_run(C.byref(rk), fake, 0, 7, fake, None), b"NULL")
