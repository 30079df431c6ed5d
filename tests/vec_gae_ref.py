"""NumPy restatements and bounds for the vector-algebra and GAE kernels (csrc/vec_ops.hip, csrc/gae_segments.hip) -- TEST
INFRASTRUCTURE shared by tests/test_vec_gae_cpu.py, tests/test_gae_segments_gpu.py, tests/test_vec_ops_gpu.py and
tools/probe_vec_gae.py.  No GPU and no torch are needed to import it.

Every input is a float32 value and counts as exact.  Each operation has a float64 restatement, the ground truth, and --
where the kernel rounds in between -- an emulation that takes the kernel's roundings one by one (the library is built with
-ffp-contract=off, so a product and the sum it feeds are rounded separately).  The inputs of every GPU case are generated
HERE (`gae_case`, `norm_input`, `vec_input`, `dots_case`, `cg_step_case`), so that tests/test_vec_gae_cpu.py can show on
exactly those inputs that each bound rejects a wrong kernel.

BOUNDS.  u = 2^-24 (unit roundoff of float32).  A bound counts the float32 roundings between the exact inputs and the output
and doubles the count.

gae_segments   bit-exact (assert_array_equal).  The kernel rounds every operation on its own (_rn intrinsics): the delta in
               float32 with gamma cast to float32 (r + g32 v' - v: 3 roundings), or in float64 with the double gamma where the
               path's mask bit is set; the state y = d + (gamma lam) y in float64, gamma lam being ONE float64 product;
               adv = float32(y), ret = float32(adv + val).  NumPy rounds the same operations the same way.
adv            |out - out64| <= u (8 |out64| + 2 |mean64| / (std64 + 1e-8)).  On |out|: x - mean32 (1), float32(std) (1),
               + 1e-8f (1), the division (1): 4, doubled 8.  The float32 squares of the variance (mpi_tools.py:86 squares in
               float32 too) move std by at most 1.5 u relative (x - mean32 rounded: 2 u on the square, the square: u, halved by
               the root) and sit in the slack.  On the mean: its cast to float32 (1), doubled 2, divided by the denominator.
cadv           |out - out64| <= u (2 |out64| + |cmean64|).  norm_apply subtracts the float64 mean in float64 and rounds once:
               1 rounding of at most u |out64|, doubled 2.  The |cmean64| term is what a cast of the mean to float32 ahead of
               the subtraction would cost (at most u |cmean64|, felt in full by an entry at the mean).  The kernel made that
               cast until these tests measured it at 0.806 of the bound (n = 256, 1e4 + N(0,1)): sound, but with no slack
               left, so the subtraction was moved to float64; the bound stands as it was set and the term is now headroom.
stats          |mean - mean64| <= n 2^-52 mean|x| (float64 sums in another order: n additions of 2^-53 relative each, doubled);
               std to rtol 4 u (1 + |mean64| / std64): 1.5 u from the float32 squares, doubled and rounded up to 4, and the
               mean's cast, which moves the sum of squares by n (u mean)^2, under u |mean| / std relative for |mean| / std < 1 / u.
lincomb        |out - (a x + b y)| <= 3 u (|a x| + |b y|), a and b the float32 values the ABI takes: the two products and the
               sum, each at most u of |a x| + |b y|.  A contracted FMA has one rounding fewer and is covered.
               With y = NULL the result is the single product float32(a x), compared bit for bit.
dots           |s - s64| <= P 2^-52 sum |x_i y_i|: the products of float32 values are exact in float64, P additions of 2^-53
               relative each, doubled.  s64 is math.fsum, exact.
cg_step        against `cg_step64(emulate=True)`: alpha and beta within 2 ulp(float32) (the float64 dot products differ in
               order only, so their float32 casts differ by at most 1 ulp, and the division adds one); x, r, p entries
               within 8 u (|x| + |alpha p|), 8 u (|r| + |alpha z|), 8 u (|r_new| + |beta p|): 2 ulp of alpha are 4 u |alpha p|,
               the product's and the sum's rounding may each fall the other way (2 u each on their magnitudes).  alpha is
               not an output: the single-step cases plant x_j = 0, p_j = 1 at j = P // 2 (P >= 3), where x_j leaves the
               kernel as alpha itself.  beta is float32(scal[0] after) / float32(scal[0] before), both outputs.
               scal[0] is float32(r.r) within 1 ulp -- taken on the r the device returned, so the reduction alone is measured --
               and scal[1] is untouched.
adam           the bound of tests/test_ppo_lag_gpu.py::test_adam_step_matches_float64_tf_adam, 1e-5 lr + 2 ulp(theta) on the
               parameter's change per step, restated in `adam_bound`.

MEASURED, not derived: ten device CG steps on a dense SPD operator against float64 CG.  err = max |x - x64| / max |x64|, e32 the
same for oracle/refupdate.cg run in float32 on the same operator, bound CG_STEP_MARGIN * max(e32, 6e-7).  CG_STEP_MARGIN is
twice the worst err / max(e32, 6e-7) measured on the MI355X over CG_DENSE_SIZES, rounded up to a power of two -- the rule
pi_f64_ref.CG_MARGIN was formed by; the denominator is the float32 reference, never the kernel.  Figures: see the constants
below and profiles/r22/vec_gae.json (tools/probe_vec_gae.py).

WHAT THE BOUNDS REJECT (tests/test_vec_gae_cpu.py, on the GPU cases' inputs; DEFECTS below).  Each defect is applied to the
emulation only and has to leave its bound by a factor of 4 on at least one case, the undamaged emulation staying below half:
  1 wave_dropped     dot products without the elements i % 1024 >= 960;
  2 tail_dropped     dot products without the ragged tail i >= 1024 (P // 1024);
  3 gl_float32       gamma lam rounded to float32 in the GAE state;
  4 delta_float32    the delta of a mask-bit path computed in float32;
  5 one_pass_var     the variance from E[x^2] - mean^2 in float32;
  6 cadv_adv_mean    cadv centred with the adv mean.
For the bit-exact GAE a bound of zero has no multiples: there "4 x" is read as at least four differing elements.
Measured (clean emulation, worst over the cases): dots 0.018, cg step 0 (it is its own reference), GAE 0 elements, adv 0.43,
std 0.085, cadv 0.495 (one rounding against twice its size); the defects: dots 4.5e15, alpha 1.6e21, beta 8.4e6 (tail; the
dropped wave 5.5e11, 2.2e6, 3.8e6), GAE 571 .. 3400 elements, adv 3.2e11 and std 718 (one-pass variance at the far-off mean),
cadv 1.1e9.  No input had to be changed.
"""
import math
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
EPS = 1e-8
KT = 1024                      # threads of the one workgroup that reduces (vec_ops.hip)
FLOOR = 6e-7                   # the float32 yardstick's floor (pi_f64_ref.FLOOR)

# ten cmbpo_cg_step on the dense operator: worst err / max(e32, FLOOR) measured on the MI355X (tools/probe_vec_gae.py)
CG_STEP_MEASURED_WORST_RATIO = 0.321  # P = 63: 1.93e-7 against max(e32 = 1.72e-7, 6e-7); the other sizes 0.157 .. 0.307
CG_STEP_MARGIN = 1.0                   # 2 x 0.321 = 0.642, rounded up to a power of two

DEFECTS = ("wave_dropped", "tail_dropped", "gl_float32", "delta_float32", "one_pass_var", "cadv_adv_mean")

RECORDS = {}                   # name -> worst error as a fraction of its bound, filled by the GPU tests (read by the probe)


def record(name, frac):
    frac = float(frac)
    RECORDS[name] = max(RECORDS.get(name, 0.0), frac)
    return frac


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def ulps(a, b):
    """|a - b| in units of the float32 spacing at b (arrays or scalars)."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    sp = np.spacing(np.abs(b).astype(F32)).astype(F64)
    return np.abs(a - b) / sp


def family(rng, n, fam):
    """The input families of the GPU cases, as float32."""
    z = rng.standard_normal(n)
    if fam == "n01":
        x = z
    elif fam == "n01+3":
        x = 3.0 + z
    elif fam == "n01+1e4":
        x = 1e4 + z
    elif fam == "spread6":                  # magnitudes 1e-6 .. 1e3
        x = np.sign(z) * 10.0 ** rng.uniform(-6, 3, n)
    elif fam == "spread4":                  # magnitudes 1e-4 .. 1e3
        x = np.sign(z) * 10.0 ** rng.uniform(-4, 3, n)
    elif fam == "const":
        x = np.full(n, 2.5 if rng.integers(2) else -0.75)
    elif fam == "zeros":
        x = np.zeros(n)
    else:
        raise ValueError(fam)
    return x.astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# cmbpo_gae_segments
# ---------------------------------------------------------------------------------------------------------------------------
GAE_PARAMS = ((0.99, 0.95, 0.97, 0.5), (1.0, 1.0, 1.0, 1.0), (0.0, 0.3, 0.99, 0.0))
GAE_LENGTHS = (0, 1, 2, 7, 64, 1000)
GAE_FIRST, GAE_SPARE = 5, 9             # offs[0] and the spare rows behind offs[n_paths]
# (n_paths, variant): a single path cannot be empty and 1000 rows long at once, so n_paths = 1 comes twice
GAE_LAYOUTS = ((1, "long"), (1, "empty"), (63, ""), (64, ""), (65, "nullmask"), (130, ""))
SENTINEL = -777.25


def gae_case(n_paths, variant=""):
    """dict(offs int32 [n_paths + 1], rew, val, cost, cval float32 [N], last_val, last_cval float32 [n_paths], mask uint8
    [n_paths] or None).  Lengths from GAE_LENGTHS; an empty segment first, last and in the middle; a 1000-row path in the first
    workgroup and, beyond 64 paths, one in the second; masks 0 .. 3 mixed, the long paths carrying 3 and 1."""
    rng = _rng("gae", n_paths, variant)
    if n_paths == 1:
        lens = np.array([0 if variant == "empty" else 1000])
        mask = np.array([1 if variant == "empty" else 3], np.uint8)
    else:
        lens = rng.choice(np.array(GAE_LENGTHS[:-1]), size=n_paths, p=[0.1, 0.25, 0.25, 0.25, 0.15])
        mask = rng.integers(0, 4, n_paths).astype(np.uint8)
        lens[[0, n_paths // 2, n_paths - 1]] = 0
        lens[1], mask[1] = 1000, 3
        lens[2:8] = GAE_LENGTHS
        mask[2:8] = (0, 1, 2, 3, 1, 2)
        if n_paths > 70:
            lens[70], mask[70] = 1000, 1
        assert set(lens) == set(GAE_LENGTHS)
    offs = (GAE_FIRST + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)
    N = int(offs[-1]) + GAE_SPARE
    c = dict(n_paths=n_paths, offs=offs, N=N,
             rew=family(rng, N, "n01"), val=(3.0 * rng.standard_normal(N)).astype(F32),
             cost=np.abs(rng.standard_normal(N)).astype(F32), cval=(2.0 + rng.standard_normal(N)).astype(F32),
             last_val=family(rng, n_paths, "n01"), last_cval=family(rng, n_paths, "n01"),
             mask=None if variant == "nullmask" else mask)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def gae_segments(offs, rew, val, cost, cval, last_val, last_cval, mask, gamma, lam, cgamma, clam, fill=SENTINEL, defect=None):
    """(adv, ret, cadv, cret), float32 [N], `fill` outside [offs[0], offs[-1]): the per-path recurrence of
    buffers/cpobuffer.py:179-207 and discount_cumsum, every operation rounded on its own as the kernel does.  All paths
    advance together, one row per pass, from their last row backwards."""
    offs = np.asarray(offs, np.int64)
    n_paths = len(offs) - 1
    mask = np.zeros(n_paths, np.uint8) if mask is None else np.asarray(mask, np.uint8)
    if defect == "delta_float32":
        mask = np.zeros(n_paths, np.uint8)
    lo, hi = offs[:-1], offs[1:]
    out = [np.full(len(rew), fill, F32) for _ in range(4)]
    streams = ((rew, val, last_val, 1, gamma, lam, out[0], out[1]), (cost, cval, last_cval, 2, cgamma, clam, out[2], out[3]))
    for x, v, last, bit, g, l, adv, ret in streams:
        x, v = np.asarray(x, F32), np.asarray(v, F32)
        g, l = float(g), float(l)
        g32 = F32(g)
        gl = g * l                                   # one float64 product
        if defect == "gl_float32":
            gl = float(F32(gl))
        wide = (mask & bit) != 0
        y = np.zeros(n_paths, F64)
        vnext = np.asarray(last, F32).copy()
        for k in range(int((hi - lo).max()) if n_paths else 0):
            act = np.nonzero(hi - lo > k)[0]
            t = hi[act] - 1 - k
            xt, vt, vn = x[t], v[t], vnext[act]
            d32 = ((xt + g32 * vn) - vt).astype(F64)                        # float32: three roundings
            d64 = (xt.astype(F64) + g * vn.astype(F64)) - vt.astype(F64)    # float64 where the mask bit is set
            d = np.where(wide[act], d64, d32)
            y[act] = d + gl * y[act]
            a = y[act].astype(F32)
            adv[t] = a
            ret[t] = a + vt
            vnext[act] = vt
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# cmbpo_adv_normalize
# ---------------------------------------------------------------------------------------------------------------------------
NORM_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 131072, 131073, 300001)
NORM_FAMILIES = ("n01", "n01+3", "n01+1e4", "spread6", "const", "zeros")
NORM_CASES = [(n, f) for n in NORM_SIZES for f in NORM_FAMILIES if n <= 1000 or f in NORM_FAMILIES[:2]]


def norm_input(n, fam):
    rng = _rng("norm", n, fam)
    adv, cadv = family(rng, n, fam), family(rng, n, fam)
    adv.setflags(write=False)
    cadv.setflags(write=False)
    return adv, cadv


def adv_normalize64(adv, cadv, emulate=False, defect=None):
    """dict(adv, cadv, mean, std, cmean): float64 mean, population std, (adv - mean) / (std + 1e-8), cadv - cmean.  With
    `emulate` the kernel's order: float64 sums, the adv mean cast to float32, (x - mean32)^2 in float32 summed in float64, a
    float32 denominator; cadv minus the float64 mean, rounded once; outputs float32."""
    a, c = np.asarray(adv, F32), np.asarray(cadv, F32)
    n = a.size
    mean = float(np.sum(a, dtype=F64)) / n
    cmean = float(np.sum(c, dtype=F64)) / n
    if not emulate:
        a64, c64 = a.astype(F64), c.astype(F64)
        std = float(np.sqrt(np.mean((a64 - mean) ** 2)))
        return dict(adv=(a64 - mean) / (std + EPS), cadv=c64 - cmean, mean=mean, std=std, cmean=cmean)
    m32 = F32(mean)
    d = a - m32
    if defect == "one_pass_var":
        ex2 = F32(float(np.sum(a * a, dtype=F64)) / n)
        std = float(np.sqrt(max(float(ex2 - m32 * m32), 0.0)))
    else:
        std = float(np.sqrt(float(np.sum(d * d, dtype=F64)) / n))
    den = F32(std) + F32(EPS)
    assert den.dtype == F32
    centre = mean if defect == "cadv_adv_mean" else cmean
    return dict(adv=d / den, cadv=(c.astype(F64) - centre).astype(F32), mean=mean, std=std, cmean=cmean)


def bound_adv(ref):
    return U * (8.0 * np.abs(ref["adv"]) + 2.0 * abs(ref["mean"]) / (ref["std"] + EPS))


def bound_cadv(ref):
    return U * (2.0 * np.abs(ref["cadv"]) + abs(ref["cmean"]))


def bound_mean(x):
    x = np.asarray(x, F64)
    return x.size * 2.0 ** -52 * float(np.mean(np.abs(x)))


def rtol_std(ref):
    return 4.0 * U * (1.0 + abs(ref["mean"]) / ref["std"])


def frac(err, bound):
    """worst err / bound over the entries; an entry with bound 0 has to be exact (and counts as 0 or inf)."""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def norm_fractions(got, ref):
    """{quantity: worst error as a fraction of its bound} of a normalisation result `got` (dict as adv_normalize64's) against the
    float64 `ref`.  A zero std (constant input) admits no relative bound: there std has to be exactly zero."""
    f = dict(adv=frac(np.abs(np.asarray(got["adv"], F64) - ref["adv"]), bound_adv(ref)),
             cadv=frac(np.abs(np.asarray(got["cadv"], F64) - ref["cadv"]), bound_cadv(ref)))
    if ref["std"] > 0:
        f["std"] = frac(abs(got["std"] - ref["std"]), rtol_std(ref) * ref["std"])
    else:
        f["std"] = 0.0 if got["std"] == 0 else np.inf
    return f


# ---------------------------------------------------------------------------------------------------------------------------
# vec_ops: lincomb, dots, cg
# ---------------------------------------------------------------------------------------------------------------------------
VEC_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 17154, 65536, 65537, 200003)
VEC_BIG = VEC_SIZES[-3:]                # lincomb and adam only: the 64 x 1024 cap and the stride beyond it
VEC_SMALL = VEC_SIZES[:-3]
VEC_FAMILIES = ("n01", "spread4")
LINCOMB_A, LINCOMB_B = float(F32(0.37)), float(F32(-1.73))
ADAM_SIZES = (1, 255, 256, 257, 65537)
CG_DENSE_SIZES = (63, 64, 65, 1023, 1025, 2049)
CG_INV_N, CG_DAMPING, CG_ITERS, CG_N = 1.0 / 777.0, float(F32(0.1)), 10, 777.0


def vec_input(P, fam, tag):
    x = family(_rng("vec", P, fam, tag), P, fam)
    x.setflags(write=False)
    return x


def lincomb64(a, x, b=0.0, y=None):
    """(a x + b y in float64, |a x| + |b y|); a and b are the float32 values the ABI takes."""
    a, b = float(F32(a)), float(F32(b))
    ax = a * np.asarray(x, F32).astype(F64)
    by = 0.0 * ax if y is None else b * np.asarray(y, F32).astype(F64)
    return ax + by, np.abs(ax) + np.abs(by)


def lincomb_emul(a, x, b=0.0, y=None):
    v = F32(a) * np.asarray(x, F32)
    return v if y is None else v + F32(b) * np.asarray(y, F32)


def bound_lincomb(scale):
    return 3.0 * U * scale


def dots64(x, y):
    """(x . y, sum |x_i y_i|): the products of float32 values are exact in float64 and math.fsum adds them exactly."""
    t = np.asarray(x, F32).astype(F64) * np.asarray(y, F32).astype(F64)
    return math.fsum(t), math.fsum(np.abs(t))


def bound_dot(P, sabs):
    return P * 2.0 ** -52 * sabs


def dot_emul(x, y, defect=None):
    """The float64 dot product in block_sum_all's order: thread t adds i = t, t + 1024, ... in turn; a wave folds its 64 lanes
    by halves (__shfl_down 32, 16, ... 1); the 16 wave sums are added in turn."""
    t = np.asarray(x, F32).astype(F64) * np.asarray(y, F32).astype(F64)
    P = t.size
    i = np.arange(P)
    if defect == "wave_dropped":
        t = np.where(i % KT >= KT - 64, 0.0, t)
    elif defect == "tail_dropped":
        t = np.where(i >= KT * (P // KT), 0.0, t)
    rows = -(-P // KT)
    t = np.concatenate([t, np.zeros(rows * KT - P)]).reshape(rows, KT)
    acc = np.zeros(KT)
    for row in t:
        acc = acc + row
    w = acc.reshape(KT // 64, 64)
    o = 32
    while o:
        w = w[:, :o] + w[:, o:2 * o]
        o >>= 1
    s = 0.0
    for v in w[:, 0]:
        s += float(v)
    return s


DOT_SCALES = (1.0, 1.0, 1e6, 1e-6, 1e3, 1e-3, 1.0, 1e5)
DOT_PAIRS = ((0, 0), (0, 1), (2, 2), (3, 3), (2, 3), (4, 5), (5, 5), (6, 7))     # the first n of them form a launch of n
DOT_COUNTS = (1, 3, 8)


def dots_case(P, fam):
    """Eight vectors of very different magnitude; DOT_PAIRS indexes them (a pair (k, k) is one pointer twice)."""
    vs = [(F32(s) * vec_input(P, fam, "dots%d" % k)).astype(F32) for k, s in enumerate(DOT_SCALES)]
    for v in vs:
        v.setflags(write=False)
    return vs


def cg_step_case(P, fam):
    """dict(hp_sum, x, r, p float32 [P], rr float32(r.r)): random vectors, hp_sum of magnitude 777 so that hp_sum / n and
    damping p both count; for P >= 3 entry j = P // 2 has x_j = 0, p_j = 1 (x_j leaves the step as alpha itself)."""
    x, r, p = (vec_input(P, fam, "cg" + k).copy() for k in "xrp")
    hp = (F32(CG_N) * vec_input(P, fam, "cgh")).astype(F32)
    if P >= 3:
        x[P // 2], p[P // 2] = 0.0, 1.0
    rr = F32(dots64(r, r)[0])
    c = dict(P=P, hp_sum=hp, x=x, r=r, p=p, rr=rr)
    for v in (hp, x, r, p):
        v.setflags(write=False)
    return c


def cg_step64(hp_sum, inv_n, damping, x, r, p, rr, emulate=False, dot=None):
    """One iteration of utilities/trust_region.py:37-44.  Returns dict(x, r, p, rr, alpha, beta, z).  In float64 on the
    float32-exact inputs; with `emulate` the kernel's roundings: inv_n cast to float32, z, alpha, beta and the element updates
    in float32 (products and sums rounded separately), the dot products in float64 (`dot`, default dot_emul) cast to float32."""
    if not emulate:
        hp, x, r, p = (np.asarray(v, F64) for v in (hp_sum, x, r, p))
        z = hp * float(inv_n) + float(damping) * p
        alpha = float(rr) / (float(np.dot(p, z)) + EPS)
        x = x + alpha * p
        r = r - alpha * z
        rr_new = float(np.dot(r, r))
        beta = rr_new / float(rr)
        return dict(x=x, r=r, p=r + beta * p, rr=rr_new, alpha=alpha, beta=beta, z=z)
    dot = dot_emul if dot is None else dot
    hp, x, r, p = (np.asarray(v, F32) for v in (hp_sum, x, r, p))
    z = hp * F32(inv_n) + F32(damping) * p
    rr_old = F32(rr)
    alpha = rr_old / (F32(dot(p, z)) + F32(EPS))
    x = x + alpha * p
    r = r - alpha * z
    rr_new = F32(dot(r, r))
    beta = rr_new / rr_old
    p_new = r + beta * p
    assert z.dtype == x.dtype == r.dtype == p_new.dtype == F32 and type(alpha) is F32 and type(beta) is F32
    return dict(x=x, r=r, p=p_new, rr=rr_new, alpha=alpha, beta=beta, z=z)


def cg_step_fractions(got, c, emu=None):
    """{quantity: worst error as a fraction of its bound} of one step's result `got` (dict x, r, p, rr, and alpha where it is
    known) on the case `c` against the undamaged emulation."""
    emu = cg_step64(c["hp_sum"], CG_INV_N, CG_DAMPING, c["x"], c["r"], c["p"], c["rr"], emulate=True) if emu is None else emu
    a, b = abs(float(emu["alpha"])), abs(float(emu["beta"]))
    x0, r0, p0, z = (np.abs(np.asarray(v, F64)) for v in (c["x"], c["r"], c["p"], emu["z"]))
    rn = np.abs(emu["r"].astype(F64))
    f = dict(x=frac(np.abs(np.asarray(got["x"], F64) - emu["x"]), 8 * U * (x0 + a * p0)),
             r=frac(np.abs(np.asarray(got["r"], F64) - emu["r"]), 8 * U * (r0 + a * z)),
             p=frac(np.abs(np.asarray(got["p"], F64) - emu["p"]), 8 * U * (rn + b * p0)))
    beta = F32(got["rr"]) / F32(c["rr"])
    f["beta"] = float(ulps(beta, emu["beta"])) / 2.0
    if got.get("alpha") is not None:
        f["alpha"] = float(ulps(got["alpha"], emu["alpha"])) / 2.0
    # the reduction alone: float32(r.r) of the r that came back
    f["rr"] = float(ulps(got["rr"], F32(dots64(got["r"], got["r"])[0])))
    return f


class DenseOperator:
    """A = damping I + G G^T / k with G float32-exact, k = P: eigenvalues of the Gram part in [0, 4].  `hp_sum(p)` is what the
    Fisher-vector product kernel would hand to cmbpo_cg_step: N (G G^T / k) p, computed in float64 and rounded to float32."""

    def __init__(self, P):
        rng = _rng("dense", P)
        self.P = P
        self.G = rng.standard_normal((P, P)).astype(F32)
        self.G64 = self.G.astype(F64)
        self.b = family(rng, P, "n01")
        self.b.setflags(write=False)
        self._fig = None

    def gram64(self, v):
        return self.G64 @ (self.G64.T @ np.asarray(v, F64)) / self.P

    def hp_sum(self, p):
        return (CG_N * self.gram64(p)).astype(F32)

    def A64(self, v):
        return self.gram64(v) + CG_DAMPING * np.asarray(v, F64)

    def A32(self, v):
        v = np.asarray(v, F32)
        out = self.G @ (self.G.T @ v) / F32(self.P) + F32(CG_DAMPING) * v
        assert out.dtype == F32
        return out

    def figures(self):
        """dict(x64, e32): refupdate.cg on the float64 operator, and the float32 run's error relative to max |x64|."""
        if self._fig is None:
            from oracle import refupdate
            x64 = refupdate.cg(self.A64, self.b.astype(F64), CG_ITERS)
            x32 = refupdate.cg(self.A32, self.b.copy(), CG_ITERS)
            assert x32.dtype == F32 and x64.dtype == F64
            self._fig = dict(x64=x64, e32=whole_error(x32, x64))
        return self._fig


_DENSE = {}


def dense_operator(P):
    if P not in _DENSE:
        _DENSE[P] = DenseOperator(P)
    return _DENSE[P]


def whole_error(x, x64):
    x64 = np.asarray(x64, F64)
    return float(np.abs(np.asarray(x, F64) - x64).max() / max(float(np.abs(x64).max()), 1e-300))


# ---------------------------------------------------------------------------------------------------------------------------
# cmbpo_vec_adam_step
# ---------------------------------------------------------------------------------------------------------------------------
def adam_bound(lr, theta):
    """the bound of test_ppo_lag_gpu.py::test_adam_step_matches_float64_tf_adam on one step's change of theta"""
    return 1e-5 * lr + 2 * np.spacing(np.abs(theta).astype(F32)).astype(F64)
