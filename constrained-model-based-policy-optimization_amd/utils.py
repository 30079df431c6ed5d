"""Object construction from the reference's experiment variant (config schema of ``configs/*.py`` merged over
``configs/baseconfig/base.py``): the registries of ``buffers/utils.py``, ``samplers/utils.py``, ``policies/utils.py``
and ``algorithms/utils.py`` and the build order of ``scripts/run.py:44-76``, with this package's classes behind them.
The variant is the RESOLVED dict (ray-tune ``sample_from`` entries already evaluated); the environment is passed in
(``get_env_from_params`` builds gym / safety-gym environments in the reference, which are out of scope here)."""
from copy import deepcopy

import numpy as np


def pos_weight_level(p, omega):
    """Where a 0/1 target column of positive rate ``p`` settles under the class weight ``omega`` (``PE(pos_weight=)``,
    ``CMBPO(m_term_pos_weight=)``): the weighted least-squares level q = omega p / (omega p + 1 - p), not p."""
    p, omega = float(p), float(omega)
    if not (0.0 <= p <= 1.0 and omega >= 0.0):
        raise ValueError("pos_weight_level: 0 <= p <= 1 and omega >= 0 expected, got %r, %r" % (p, omega))
    den = omega * p + 1.0 - p
    return omega * p / den if den > 0.0 else 0.0


def sigmoid(z):
    """sigma(z) of a logistic model column (``PE(logistic_columns=)``), float64, without overflow: 1 / (1 + exp(-z))
    for z >= 0, exp(z) / (1 + exp(z)) otherwise."""
    z = np.asarray(z, np.float64)
    ez = np.exp(-np.abs(z))
    out = np.where(z >= 0, 1.0 / (1.0 + ez), ez / (1.0 + ez))
    return out if out.ndim else float(out)


def logit(p):
    """log(p / (1 - p)) in float64 for a probability strictly inside (0, 1): the inverse of :func:`sigmoid`."""
    p = float(p)
    if not 0.0 < p < 1.0:       # (written positively: NaN is refused)
        raise ValueError("logit: a probability strictly inside (0, 1) expected, got %r" % (p,))
    return float(np.log(p / (1.0 - p)))


def logit_threshold(tau):
    """The float32 number a logistic termination head compares its logit with: sigma(z) > tau is defined as
    z > float32(log(tau / (1 - tau))) (include/cmbpo_hip.h at cmbpo_trainer_set_column_kinds)."""
    try:
        return float(np.float32(logit(tau)))
    except (TypeError, ValueError):
        raise ValueError("a logistic termination head reads term_threshold as a probability strictly inside (0, 1), "
                         "got %r" % (tau,)) from None


def term_thresholds(u, loss, check=True):
    """THE place that turns termination draws into the thresholds of ``cmbpo_fakeenv_post_term_draws`` (sampled terminations,
    DESIGN §3y): a branch whose termination column says p ends where ``column > threshold``, which happens with probability p for
    ``u`` uniform on (0, 1].  ``loss`` says how the column was trained: under ``'logistic'`` it is a logit and the threshold
    ``log(u) - log1p(-u)``, computed in float64 and rounded to float32 (u = 1 gives +inf: a probability of exactly 0 never
    ends a branch; u = 0.5 gives 0; u = 0 gives -inf); under ``'gaussian'`` it is in 0 / 1 target units and the threshold ``u``
    itself.  ``u``: a NumPy array or a torch tensor, any shape; the result is float32 of the same kind (and device).  A ``u``
    outside [0, 1] or NaN raises ``ValueError``; ``check=False`` skips that test for draws that are inside by construction
    (on a device tensor it costs a synchronisation)."""
    if loss not in ('gaussian', 'logistic'):
        raise ValueError(f"term_thresholds: loss 'gaussian' or 'logistic', got {loss!r}")
    import torch
    if not isinstance(u, torch.Tensor):
        u = np.asarray(u)
        if u.dtype.kind not in 'fiu':
            raise ValueError("term_thresholds: draws must be real numbers, got dtype %s" % (u.dtype,))
        # (written positively: a NaN is refused)
        if check and not bool(np.all((u >= 0) & (u <= 1))):
            raise ValueError("term_thresholds: draws must lie in [0, 1] (NaN is refused): they are uniform numbers, "
                             "u = 1 - rand() in (0, 1]")
        if loss == 'gaussian':
            return u.astype(np.float32)
        u64 = u.astype(np.float64)
        with np.errstate(divide='ignore'):
            return (np.log(u64) - np.log1p(-u64)).astype(np.float32)
    if not u.is_floating_point():
        raise ValueError("term_thresholds: draws must be a floating-point tensor, got %s" % (u.dtype,))
    if check and not bool(((u >= 0) & (u <= 1)).all()):
        raise ValueError("term_thresholds: draws must lie in [0, 1] (NaN is refused): they are uniform numbers, "
                         "u = 1 - rand() in (0, 1]")
    if loss == 'gaussian':
        return u.to(torch.float32)
    u64 = u.to(torch.float64)
    return (torch.log(u64) - torch.log1p(-u64)).to(torch.float32)


def get_cpobuffer(env, *args, **kwargs):
    from .cpobuffer import CPOBuffer
    return CPOBuffer(*args, observation_space=env.observation_space, action_space=env.action_space, **kwargs)


def get_cposampler(*args, **kwargs):
    from .cpo_sampler import CpoSampler
    return CpoSampler(*args, **kwargs)


def get_cpo_policy(env, session=None, *args, **kwargs):
    from .cpo_policy import CPOPolicy
    return CPOPolicy(obs_space=env.observation_space, act_space=env.action_space, session=session, *args, **kwargs)


def create_CMBPO_algorithm(variant, *args, **kwargs):
    from .cmbpo import CMBPO
    return CMBPO(*args, **kwargs)


BUFFER_FUNCTIONS = {'CPOBuffer': get_cpobuffer}
SAMPLERS_FUNCTIONS = {'CPOSampler': get_cposampler}
POLICY_FUNCTIONS = {'cpopolicy': get_cpo_policy}
ALGORITHM_CLASSES = {'CMBPO': create_CMBPO_algorithm}


def get_buffer_from_params(params, env, *args, **kwargs):
    p = params['buffer_params']
    return BUFFER_FUNCTIONS[p.get('type', 'CPOBuffer')](env, *args, **deepcopy(p.get('kwargs', {})), **kwargs)


def get_sampler_from_params(params, *args, **kwargs):
    p = params['sampler_params']
    kw = deepcopy(p.get('kwargs', {}))
    return SAMPLERS_FUNCTIONS[p.get('type', 'CPOSampler')](*deepcopy(p.get('args', ())), *args, **kw, **kwargs)


def get_policy_from_params(params, env, *args, **kwargs):
    p = params['policy_params']
    return POLICY_FUNCTIONS[p['type']](env, *args, **deepcopy(p['kwargs']), **kwargs)


def get_algorithm_from_params(variant, *args, **kwargs):
    p = variant['algorithm_params']
    kw = deepcopy(p['kwargs'])
    if hasattr(kw, 'toDict'):
        kw = kw.toDict()
    return ALGORITHM_CLASSES[p['type']](variant, *args, **kw, **kwargs)


def build_experiment(params, env, device=None):
    """scripts/run.py:44-76: buffer, sampler, policy, algorithm -- returns the algorithm (``.train()`` is the generator
    the reference's tune trainable steps).  Entries the reference fills in through ray-tune lambdas may be left out:
    the buffer size defaults to ``epoch_length``, the archive to 3e5 samples, the sampler's / policy's
    ``max_path_length`` to the environment's ``max_episode_steps`` attribute (or 1000), the task to ``params['task']``."""
    params = deepcopy(params)
    akw = params['algorithm_params']['kwargs']
    mpl = int(getattr(env, 'max_episode_steps', getattr(env, '_max_episode_steps', 1000)))
    params.setdefault('buffer_params', {})
    bkw = params['buffer_params'].setdefault('kwargs', {})
    bkw.setdefault('size', int(akw.get('epoch_length', 50000)))
    bkw.setdefault('archive_size', int(3e5))
    params.setdefault('sampler_params', {})
    skw = params['sampler_params'].setdefault('kwargs', {})
    skw.setdefault('max_path_length', mpl)
    params['policy_params']['kwargs'].setdefault('max_path_length', skw['max_path_length'])
    akw.setdefault('task', params.get('task', 'default'))
    dev = {} if device is None else {'device': device}
    buffer = get_buffer_from_params(params, env)
    sampler = get_sampler_from_params(params)
    policy = get_policy_from_params(params, env, None, **dev)
    for k in ('eval_render_mode', 'eval_n_episodes', 'eval_deterministic'):
        akw.pop(k, None)
    return get_algorithm_from_params(variant=params, env=env, policy=policy, buffer=buffer, sampler=sampler, **dev)
