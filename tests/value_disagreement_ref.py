"""NumPy specification of the critics' own disagreement and of the pessimistic values made from it
(cmbpo_critic_pair_predict_var, include/cmbpo_hip.h), and the seeded critics the tests of it share.

For a row with the per-member critic values ``x[E]`` (float32, after each member's ``inverse_transform``: the bits the kernels
add up for the mean), per critic:

    mean = (((x0 + x1) + x2) + ...) / E                        what cmbpo_critic_pair_predict returns, unchanged
    var  = member_var(x)                                        tests/disagreement_ref.py: np.var over the members, float32
    v    = fl32(mean - fl32(kappa_v  * sqrt(var_v )))           where kappa_v  > 0, else mean bit for bit
    vc   = fl32(mean + fl32(kappa_vc * sqrt(var_vc)))           where kappa_vc > 0, else mean bit for bit

``member_var`` and ``penalise`` are those of the reward / cost disagreement; nothing is restated here.  E = 1 gives var = +0;
with kappa > 0 non-finite members propagate as NumPy propagates them; the variance is in output units (after the output
scaler)."""
import numpy as np

from disagreement_ref import member_var, penalise


def member_mean(x):
    """The plain entry's mean: a float32 sum that starts at +0 and takes the members in order, then one division."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    with np.errstate(all="ignore"):
        s = np.zeros(x.shape[1], np.float32)
        for e in range(x.shape[0]):
            s = (s + x[e]).astype(np.float32)
        return (s / np.float32(x.shape[0])).astype(np.float32)


def value_disagreement(xv, xvc, kappa_v=0.0, kappa_vc=0.0):
    """(v, vc, v_var, vc_var) from the member values xv[E, n], xvc[E, n] of the two critics."""
    v_var, vc_var = member_var(xv), member_var(xvc)
    return (penalise(member_mean(xv), v_var, kappa_v, -1), penalise(member_mean(xvc), vc_var, kappa_vc, +1), v_var, vc_var)


# ---- the critics of the tests ------------------------------------------------------------------------------------------
def critic_weights(seed, E, obs_dim, out_mu=None):
    """Two E-member critics ([W0, W1, W2], [b0, b1, b2], scaler_in, scaler_out each) with independent members whose values
    sit around 1 with a member spread of about 0.1 in network units: the members' output biases are 1 + 0.1 xi_e, the rest of
    the output is a few hundredths.  sigma / |mean| is then around 0.1 after the output scaler (sigma in [0.5, 2], mu about 0.1)
    and kappa * sigma is thousands of ulps of the mean.  out_mu: an output scaler (out_mu, 1) instead -- values around
    out_mu + 1 with the same spread, where a one-pass E[x^2] - E[x]^2 in float32 has no digit left."""
    from cmbpo_amd import synthetic
    rng = np.random.default_rng([seed, E, obs_dim])
    out = []
    for _ in range(2):
        ws, bs = synthetic.ensemble_weights(rng, E, obs_dim, 128, 1, bias_scale=0.1, out_scale=0.25)
        bs[2] = (1.0 + 0.1 * rng.standard_normal((E, 1, 1))).astype(np.float32)
        sc_in = synthetic.scaler(rng, obs_dim, hit_clamp=False)
        if out_mu is None:
            sc_out = synthetic.scaler(rng, 1)
        else:
            sc_out = (np.full((1, 1), out_mu, np.float32), np.ones((1, 1), np.float32))
        out.append((ws, bs, sc_in, sc_out))
    return out


def one_member(critic, e):
    """The one-member critic made of member e of `critic`, same scalers."""
    ws, bs, sc_in, sc_out = critic
    return [w[e:e + 1] for w in ws], [b[e:e + 1] for b in bs], sc_in, sc_out


def observations(seed, n, obs_dim):
    """Rows of different scale (the kernels lift every row by its own power of two)."""
    rng = np.random.default_rng([seed, n, obs_dim, 1])
    return (rng.standard_normal((n, obs_dim)) * np.exp(0.5 * rng.standard_normal((n, 1)))).astype(np.float32)


def check_non_vacuous(x, kappa, sign, relative=True):
    """The conditions under which a comparison against the specification says something, on the member values x[E, n] (E >= 2):
    sigma / |mean| in [1e-3, 1] on >= 90 % of the rows (relative=False, the out_mu = 1000 case: sigma in [1e-2, 1] instead,
    the mean is a thousand times that by construction), and with kappa > 0 the penalised value differs from the mean in bits
    on >= 90 % of the rows."""
    mean, var = member_mean(x), member_var(x)
    sig = np.sqrt(var.astype(np.float64))
    ratio = sig / np.abs(mean.astype(np.float64)) if relative else sig
    lo = 1e-3 if relative else 1e-2
    frac = float(np.mean((ratio >= lo) & (ratio <= 1.0)))
    assert frac >= 0.9, f"spread in range on {frac:.2%} of the rows only"
    if kappa > 0.0:
        moved = float(np.mean(penalise(mean, var, kappa, sign).view(np.uint32) != mean.view(np.uint32)))
        assert moved >= 0.9, f"kappa = {kappa} moves {moved:.2%} of the rows only"
