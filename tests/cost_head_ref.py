"""NumPy specification of the logistic learned-cost head (include/cmbpo_hip.h at cmbpo_cost_head_t), in float32
operation for operation, plus a float64 sigma to measure the float32 one against.

    zs_e     = fl32(z_e - logit_shift)                 (logit_shift == 0: z_e bit for bit, no subtraction)
    p_e      = sigma32(zs_e)
    cost     = p_elite                                  without disagreement, or kappa_cost == 0
    cost_var = np.var(p_e over ALL members) in the order s = ((p_0 + p_1) + ...), m = s / E, q = sum (p_e - m)^2, var = q / E
    cost     = clip1(fl32(p_elite + fl32(kappa_cost * sqrt(cost_var))))       if kappa_cost > 0

sigma32 here calls NumPy's float32 exp, whose last bit need not be the device's expf's: the GPU tests therefore take the members'
probabilities from the device itself and hold everything DOWNSTREAM of them against `downstream` bit for bit, and hold the
probabilities against `sigma64` within the bound derived in `sigma_bound`."""
import numpy as np

f32 = np.float32
KIND_MAGNITUDE, KIND_LOGISTIC = 0, 1


def cost_column(obs_dim):
    return int(obs_dim) + 1


def sigma64(z):
    """sigma in float64, the branch that never overflows on each side of 0; +inf -> 1, -inf -> 0, NaN -> NaN."""
    z = np.asarray(z, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(z))
        return np.where(np.isnan(z), np.nan, np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))


def sigma32(zs):
    """1 / (1 + exp(-zs)) for zs >= 0, exp(zs) / (1 + exp(zs)) otherwise (a NaN takes that branch and stays one): float32
    throughout, every operation rounded on its own."""
    zs = np.asarray(zs, f32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        pos = f32(1) / (f32(1) + np.exp(-zs, dtype=f32))
        e = np.exp(zs, dtype=f32)
        neg = e / (f32(1) + e)
    return np.where(zs >= 0, pos, neg).astype(f32)


def shift(z, logit_shift):
    z = np.asarray(z, f32)
    return z if f32(logit_shift) == 0 else (z - f32(logit_shift)).astype(f32)


def clip1(c):
    """c > 1 ? 1 : c -- a positive test, so a NaN passes."""
    c = np.asarray(c, f32)
    return np.where(c > 1, f32(1), c).astype(f32)


def member_var(p):
    """np.var over axis 0 in the kernel's order of operations; p: [E, n] float32."""
    p = np.asarray(p, f32)
    E = p.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros(p.shape[1], f32)
        for e in range(E):
            s = (s + p[e]).astype(f32)
        m = (s / f32(E)).astype(f32)
        q = np.zeros(p.shape[1], f32)
        for e in range(E):
            d = (p[e] - m).astype(f32)
            q = (q + (d * d).astype(f32)).astype(f32)
        return (q / f32(E)).astype(f32)


def downstream(p, inds, kappa_cost=None):
    """(cost, cost_var) from the members' probabilities p [E, n] and the elite per row.  kappa_cost None: no disagreement (the
    variance is not measured: None); 0: measured, the elite's probability bit for bit whatever the others hold."""
    p = np.asarray(p, f32)
    inds = np.asarray(inds)
    p_el = p[inds, np.arange(p.shape[1])]
    if kappa_cost is None:
        return p_el, None
    var = member_var(p)
    if not f32(kappa_cost) > 0:
        return p_el, var
    with np.errstate(invalid="ignore", over="ignore"):
        pess = (p_el + (f32(kappa_cost) * np.sqrt(var, dtype=f32)).astype(f32)).astype(f32)
    return clip1(pess), var


def cost_head(mean, inds, obs_dim, logit_shift=0.0, kappa_cost=None, rows=None):
    """The whole block on mean [E, B, out]: (cost, cost_var or None, cost_logit) for the listed rows (None: all)."""
    mean = np.asarray(mean, f32)
    rows = np.arange(mean.shape[1]) if rows is None else np.asarray(rows)
    z = mean[:, rows, cost_column(obs_dim)]
    el = np.asarray(inds)[rows]
    cost, var = downstream(sigma32(shift(z, logit_shift)), el, kappa_cost)
    return cost, var, z[el, np.arange(len(rows))]


# |sigma32(z) - sigma(z)| <= SIGMA_ULPS * 2^-23 * sigma(z).  expf is documented at 1 ulp (ROCm's OCML, and the CUDA tables it
# follows): e~ = e (1 + d1), |d1| <= 2^-23 (an ulp is at most 2^-23 relative).  z >= 0: 1 + e~ with e~ <= 1 has absolute error
# <= 2^-23 e from e~ and relative rounding error 2^-24, the correctly rounded division adds 2^-24: (1 + 0.5 + 0.5) 2^-23 = 2 at
# most (e / (1 + e) <= 1/2 scales the first term down).  z < 0: e~ / (1 + e~): the numerator carries d1, the denominator d1 e / (1 + e)
# <= d1 / 2 in the other direction at most, the sum's rounding 2^-24, the division's 2^-24: (1 + 0.5 + 0.5 + 0.5) 2^-23 = 2.5.
# Asserted: 4, the bound rounded up.  Where expf(zs) is subnormal (zs < -87.3) its relative error is unbounded; the tests stay at
# |z| <= 80 apart from the special values, where the results are exact (0, 1, NaN).
SIGMA_ULPS = 4.0


def sigma_bound(z):
    return SIGMA_ULPS * 2.0 ** -23 * sigma64(z)
