"""User-defined termination and cost rules for imagined rollouts -- the counterpart of adding a function to
``TERMS_BY_TASK`` / ``COST_BY_TASK`` in the reference's ``models/statics.py:56-69``.

A rule set is a table of at most 16 clauses (``include/cmbpo_hip.h``, ``cmbpo_task_rules_t``) that the post kernel of
``FakeEnv.step`` evaluates per branch on the device.  A clause tests a slice of columns of ``next_obs``, ``obs`` or ``act``
against an interval::

    f = float32(x * scale);  f = |f| if abs
    column holds  iff  (f > lo if lo_strict else f >= lo) and (f < hi if hi_strict else f <= hi)     # never for a NaN
    clause holds  iff  all columns hold (any of them with any=True)

and has one of three roles: ``healthy`` (the branch is done if the clause does NOT hold), ``fatal`` (done if it holds),
``cost`` (the step costs 1 if it holds).  ``healthy`` and ``fatal`` differ on NaN, as ``1.0 <= z <= 2.0`` and
``not (z < 1.0 or z > 2.0)`` do in NumPy: keep whichever the function being ported did.

    from cmbpo_amd.statics import TaskRules, healthy, cost, register_task
    hopper = TaskRules([healthy(cols=slice(1, None), abs=True, hi=100.0, hi_strict=True),    # (|s[1:]| < 100).all()
                        healthy(cols=0, lo=0.7, lo_strict=True),                              # height > 0.7
                        healthy(cols=1, abs=True, hi=0.2, hi_strict=True)],                   # |angle| < 0.2
                       require_finite=True)                                                   # np.isfinite(s).all()
    register_task("Hopper-v2", hopper)           # FakeEnv(task="Hopper-v2") / CMBPO(task="Hopper-v2") now resolve it
    term_fn, cost_fn = hopper.numpy_fns()        # the same rules as NumPy functions of (obs, act, next_obs)

``TaskRules.numpy_fns()`` is bit-exact with the kernel by construction (float32 products with one rounding, the same
comparisons), and has the signature, shapes and dtypes of the reference's functions, so the pair can be put into the
reference's own tables.

**Derived quantities.**  An interval on a single column cannot say "within radius r of a point", "planar speed above v" or
"tilt below c".  A rule set may therefore declare up to 8 derived quantities, each a bias plus up to 4 terms over columns of
``next_obs``, ``obs`` or ``act``, in float32 with single roundings in exactly this order::

    g = bias
    for each term:  t = float32(x - c);  t = float32(t * t) if pow == 2;  g = float32(g + float32(w * t))

and a clause with ``src='derived'`` tests them: its ``cols`` index the derived quantities, everything else (``scale``, ``abs``,
the interval, ``any``, the role) applies to ``g`` unchanged, and a NaN ``g`` never holds::

    from cmbpo_amd.statics import TaskRules, cost, healthy, dist_sq, speed_sq, tilt
    hazards = TaskRules([cost(src='derived', cols=slice(0, 2), any=True, hi=0.25),       # inside either circle of radius 0.5
                         cost(src='derived', cols=2, lo=4.0, lo_strict=True)],           # planar speed above 2
                        derived=[dist_sq((0, 1), (1.0, -2.0)), dist_sq((0, 1), (3.0, 0.5)), speed_sq((5, 6))])
    # the rule AntSafe's static function meant (models/statics.py:17-33): height in [0.2, 1], tilt >= -0.7, finite state
    ant = TaskRules([healthy(cols=0, lo=0.2, hi=1.0), healthy(src='derived', cols=0, lo=-0.7)],
                    derived=[tilt(2, 3)], require_finite=True)

``term(col, w=, c=, pow=1)`` writes any linear combination of columns (goal minus robot).  Products of two different columns
stay out, and so does the built-in AntSafe task's precedence quirk (``a*b*c*z_rot >= -0.7``), a conjunction across clauses that
the language cannot and should not write: ``AntSafe-v2`` stays a built-in task.
"""
import ctypes as C

import numpy as np

from . import _lib

_ROLES = {"healthy": _lib.RULE_HEALTHY, "fatal": _lib.RULE_FATAL, "cost": _lib.RULE_COST}
_SRCS = {"next_obs": _lib.RULE_SRC_NEXT_OBS, "obs": _lib.RULE_SRC_OBS, "act": _lib.RULE_SRC_ACT, "derived": _lib.RULE_SRC_DERIVED}
_TERM_SRCS = ("next_obs", "obs", "act")


class Term:
    """One term ``w * (x - c) ** pow`` of a derived quantity; built by ``term``."""
    __slots__ = ("src", "col", "w", "c", "pow")

    def __init__(self, col, src='next_obs', w=1.0, c=0.0, pow=1):
        if src not in _TERM_SRCS:
            raise ValueError("term src: one of %s, got %r" % (sorted(_TERM_SRCS), src))
        if isinstance(col, (bool, float)) or int(col) != col:
            raise TypeError("term col: an integer column, got %r" % (col,))
        if pow not in (1, 2):
            raise ValueError("term pow: 1 or 2, got %r" % (pow,))
        self.src, self.col, self.pow = src, int(col), int(pow)
        with np.errstate(all="ignore"):
            self.w, self.c = np.float32(w), np.float32(c)
        if not (np.isfinite(self.w) and np.isfinite(self.c)):
            raise ValueError("term w / c: finite float32 numbers, got w=%r c=%r" % (w, c))

    def __repr__(self):
        return "Term(col=%d, src=%r, w=%r, c=%r, pow=%d)" % (self.col, self.src, float(self.w), float(self.c), self.pow)


def term(col, src='next_obs', w=1.0, c=0.0, pow=1):
    """``w * (x[col] - c) ** pow`` with ``x`` one of ``next_obs`` / ``obs`` / ``act``; ``col < 0`` counts from the end."""
    return Term(col, src=src, w=w, c=c, pow=pow)


class Derived:
    """A derived quantity ``bias + sum of terms``; built by ``derived`` or one of ``dist_sq`` / ``speed_sq`` / ``tilt``."""
    __slots__ = ("terms", "bias")

    def __init__(self, terms, bias=0.0):
        self.terms = tuple(terms)
        if not 1 <= len(self.terms) <= _lib.RULE_MAX_TERMS:
            raise ValueError("a derived quantity has 1 to %d terms, got %d" % (_lib.RULE_MAX_TERMS, len(self.terms)))
        for t in self.terms:
            if not isinstance(t, Term):
                raise TypeError("terms: built with term(), got %r" % (t,))
        with np.errstate(all="ignore"):
            self.bias = np.float32(bias)
        if not np.isfinite(self.bias):
            raise ValueError("bias: a finite float32 number, got %r" % (bias,))

    def values(self, obs, act, next_obs):
        """The float32 values of this quantity over the leading dimensions: what the kernel computes, one NumPy operation per
        rounding, in the kernel's order."""
        srcs = {"next_obs": next_obs, "obs": obs, "act": act}
        g = None
        with np.errstate(all="ignore"):
            for t in self.terms:
                x = np.asarray(srcs[t.src], dtype=np.float32)
                width = x.shape[-1]
                col = t.col + width if t.col < 0 else t.col
                if not 0 <= col < width:
                    raise ValueError("term column %d outside %s's width %d" % (t.col, t.src, width))
                if g is None:
                    g = np.full(x.shape[:-1], self.bias, dtype=np.float32)
                d = x[..., col] - t.c                  # float32 - float32: one rounding
                if t.pow == 2:
                    d = d * d
                g = g + t.w * d                        # two roundings: the product, then the sum
        return g

    def __repr__(self):
        return "Derived(%r, bias=%r)" % (list(self.terms), float(self.bias))


def derived(terms, bias=0.0):
    """``bias + sum_i w_i * (x_i - c_i) ** pow_i`` over at most 4 terms, accumulated in the order given."""
    return Derived(terms, bias=bias)


def dist_sq(cols, center, src='next_obs'):
    """Squared distance of the columns ``cols`` from the point ``center``: ``sum_i (x[cols[i]] - center[i]) ** 2``."""
    cols, center = tuple(cols), tuple(center)
    if len(cols) != len(center):
        raise ValueError("dist_sq: %d columns but %d centre coordinates" % (len(cols), len(center)))
    return Derived([Term(c, src=src, c=m, pow=2) for c, m in zip(cols, center)])


def speed_sq(cols, src='next_obs'):
    """Squared norm of the columns ``cols``: ``sum_i x[cols[i]] ** 2``."""
    return Derived([Term(c, src=src, pow=2) for c in tuple(cols)])


def tilt(q1_col, q2_col, src='next_obs'):
    """``1 - 2 (q1^2 + q2^2)``, the z component of the rotated up vector (``z_rot`` of ``models/statics.py:22``), accumulated as
    ``(1 + -2 q1^2) + -2 q2^2``."""
    return Derived([Term(q1_col, src=src, w=-2.0, pow=2), Term(q2_col, src=src, w=-2.0, pow=2)], bias=1.0)


class Clause:
    """One clause of a rule set; built by ``healthy`` / ``fatal`` / ``cost``."""
    __slots__ = ("role", "src", "col0", "n_cols", "lo", "hi", "lo_strict", "hi_strict", "abs", "scale", "any")

    def __init__(self, role, src='next_obs', cols=0, lo=-np.inf, hi=np.inf, lo_strict=False, hi_strict=False, abs=False,
                 scale=1.0, any=False):
        if role not in _ROLES:
            raise ValueError("role: one of %s, got %r" % (sorted(_ROLES), role))
        if src not in _SRCS:
            raise ValueError("src: one of %s, got %r" % (sorted(_SRCS), src))
        if isinstance(cols, slice):
            if cols.step not in (None, 1):
                raise ValueError("cols: a slice with step 1, got %r" % (cols,))
            col0 = 0 if cols.start is None else int(cols.start)
            if cols.stop is None:
                n_cols = -1
            else:
                stop = int(cols.stop)
                if (col0 < 0) != (stop < 0):
                    raise ValueError("cols: start and stop of a slice must count from the same end, got %r" % (cols,))
                n_cols = stop - col0
                if n_cols < 1:
                    raise ValueError("cols: empty slice %r" % (cols,))
        else:
            col0, n_cols = int(cols), 1
        self.role, self.src, self.col0, self.n_cols = role, src, col0, n_cols
        self.lo, self.hi = np.float32(lo), np.float32(hi)
        self.scale = np.float32(scale)
        self.lo_strict, self.hi_strict, self.abs, self.any = bool(lo_strict), bool(hi_strict), bool(abs), bool(any)

    @property
    def flags(self):
        return (_lib.RULE_ABS * self.abs | _lib.RULE_LO_STRICT * self.lo_strict | _lib.RULE_HI_STRICT * self.hi_strict
                | _lib.RULE_ANY * self.any)

    def values(self, obs, act, next_obs, derived=None):
        """The float32 values this clause compares with ``lo`` / ``hi``, ``[..., n_cols]``.  ``derived``: the derived quantities
        ``[..., n_derived]`` a clause with ``src='derived'`` reads (``TaskRules.derived_values``)."""
        if self.src == "derived" and derived is None:
            raise ValueError("a clause with src='derived' needs the derived quantities (TaskRules.derived_values)")
        x = np.asarray({"next_obs": next_obs, "obs": obs, "act": act, "derived": derived}[self.src], dtype=np.float32)
        width = x.shape[-1]
        col0 = self.col0 + width if self.col0 < 0 else self.col0
        n = width - col0 if self.n_cols == -1 else self.n_cols
        if not (0 <= col0 < width and 1 <= n <= width - col0):
            raise ValueError("clause columns (col0 %d, n_cols %d) outside %s's width %d" % (self.col0, self.n_cols, self.src, width))
        with np.errstate(all="ignore"):
            f = x[..., col0:col0 + n] * self.scale          # float32 * float32: one rounding
            if self.abs:
                f = np.abs(f)
        return f

    def holds(self, obs, act, next_obs, derived=None):
        """Boolean mask over the leading dimensions: what the kernel computes for this clause."""
        f = self.values(obs, act, next_obs, derived)
        with np.errstate(all="ignore"):
            ok = (f > self.lo if self.lo_strict else f >= self.lo) & (f < self.hi if self.hi_strict else f <= self.hi)
        return ok.any(axis=-1) if self.any else ok.all(axis=-1)

    def __repr__(self):
        return "Clause(%r, src=%r, col0=%d, n_cols=%d, lo=%r, hi=%r, flags=0x%x, scale=%r)" % (
            self.role, self.src, self.col0, self.n_cols, float(self.lo), float(self.hi), self.flags, float(self.scale))


def healthy(**kw):
    """The branch is done if this clause does not hold (``notdone = ... * clause``)."""
    return Clause("healthy", **kw)


def fatal(**kw):
    """The branch is done if this clause holds (``done = ... + clause``)."""
    return Clause("fatal", **kw)


def cost(**kw):
    """The step costs 1.0 if this clause holds."""
    return Clause("cost", **kw)


class TaskRules:
    """A set of clauses plus two flags.  ``require_finite`` adds ``np.isfinite(next_obs).all()`` to the healthy conditions;
    ``cost_on_term`` makes the cost ``min(1, done + obj)`` (``models/statics.py:51-52``) instead of ``obj``.  ``derived``: the
    derived quantities (at most 8) that clauses with ``src='derived'`` address by index."""

    def __init__(self, clauses=(), derived=(), require_finite=False, cost_on_term=False):
        if isinstance(derived, (bool, Derived)):
            raise TypeError("derived: a list of derived quantities, got %r" % (derived,))
        self.clauses = tuple(clauses)
        self.derived = tuple(derived)
        if len(self.derived) > _lib.RULE_MAX_DERIVED:
            raise ValueError("at most %d derived quantities, got %d" % (_lib.RULE_MAX_DERIVED, len(self.derived)))
        for d in self.derived:
            if not isinstance(d, Derived):
                raise TypeError("derived: built with derived() / dist_sq() / speed_sq() / tilt(), got %r" % (d,))
        if len(self.clauses) > _lib.RULE_MAX_CLAUSES:
            raise ValueError("at most %d clauses, got %d" % (_lib.RULE_MAX_CLAUSES, len(self.clauses)))
        for c in self.clauses:
            if not isinstance(c, Clause):
                raise TypeError("clauses: built with healthy() / fatal() / cost(), got %r" % (c,))
            if c.src == "derived":
                n = len(self.derived)
                col0 = c.col0 + n if c.col0 < 0 else c.col0
                cnt = n - col0 if c.n_cols == -1 else c.n_cols
                if not (0 <= col0 < n and 1 <= cnt <= n - col0):
                    raise ValueError("clause indices (col0 %d, n_cols %d) outside the %d derived quantities" % (c.col0, c.n_cols, n))
        self.require_finite, self.cost_on_term = bool(require_finite), bool(cost_on_term)
        self._task_id = None

    def struct(self):
        """The ``cmbpo_task_rules_t`` image of this rule set."""
        s = _lib.TaskRulesStruct()
        s.n_clauses, s.require_finite, s.cost_on_term = len(self.clauses), int(self.require_finite), int(self.cost_on_term)
        for i, c in enumerate(self.clauses):
            d = s.clause[i]
            d.role, d.src, d.col0, d.n_cols, d.flags = _ROLES[c.role], _SRCS[c.src], c.col0, c.n_cols, c.flags
            d.scale, d.lo, d.hi = float(c.scale), float(c.lo), float(c.hi)
        return s

    def derived_struct(self):
        """The ``cmbpo_rule_derived_table_t`` image of this set's derived quantities (all zeros without any)."""
        s = _lib.RuleDerivedTableStruct()
        s.n_derived = len(self.derived)
        for i, q in enumerate(self.derived):
            d = s.derived[i]
            d.n_terms, d.bias = len(q.terms), float(q.bias)
            for k, t in enumerate(q.terms):
                m = d.term[k]
                m.src, m.pow, m.col, m.w, m.c = _SRCS[t.src], t.pow, t.col, float(t.w), float(t.c)
        return s

    @property
    def task_id(self):
        """The rule id of this set in the native library; registered on first use (equal sets share one id)."""
        if self._task_id is None:
            out = C.c_int(-1)
            s = self.struct()
            if self.derived:
                d = self.derived_struct()
                _lib.check(_lib.lib().cmbpo_task_rules_register_ex(C.byref(s), C.byref(d), C.byref(out)), "cmbpo_task_rules_register_ex")
            else:
                _lib.check(_lib.lib().cmbpo_task_rules_register(C.byref(s), C.byref(out)), "cmbpo_task_rules_register")
            self._task_id = int(out.value)
        return self._task_id

    def derived_values(self, obs, act, next_obs):
        """The derived quantities as one float32 array ``[..., n_derived]`` (None without any)."""
        if not self.derived:
            return None
        return np.stack([q.values(obs, act, next_obs) for q in self.derived], axis=-1)

    @property
    def has_cost(self):
        return self.cost_on_term or any(c.role == "cost" for c in self.clauses)

    def done(self, obs, act, next_obs):
        next_obs = np.asarray(next_obs, dtype=np.float32)
        d = np.zeros(next_obs.shape[:-1], dtype=bool)
        if self.require_finite:
            d |= ~np.isfinite(next_obs).all(axis=-1)
        g = self.derived_values(obs, act, next_obs)
        for c in self.clauses:
            if c.role == "healthy":
                d |= ~c.holds(obs, act, next_obs, g)
            elif c.role == "fatal":
                d |= c.holds(obs, act, next_obs, g)
        return d

    def numpy_fns(self):
        """``(term_fn, cost_fn)`` with the reference's signature ``(obs, act, next_obs)``: term is bool ``[..., 1]``, cost is
        float32 ``[..., 1]``; ``cost_fn`` is None when the set has neither a cost clause nor ``cost_on_term`` (the
        reference's FakeEnv then returns ``np.zeros_like(terms)``)."""
        def term_fn(obs, act, next_obs):
            assert len(obs.shape) == len(next_obs.shape) == len(act.shape)
            return self.done(obs, act, next_obs)[..., None]

        def cost_fn(obs, act, next_obs):
            assert len(obs.shape) == len(next_obs.shape) == len(act.shape)
            obj = np.zeros(np.asarray(next_obs).shape[:-1], dtype=bool)
            g = self.derived_values(obs, act, next_obs)
            for c in self.clauses:
                if c.role == "cost":
                    obj |= c.holds(obs, act, next_obs, g)
            obj = obj.astype(np.float32)
            if self.cost_on_term:
                obj = np.minimum(self.done(obs, act, next_obs).astype(np.float32) + obj, np.float32(1.0))
            return obj[..., None]

        return term_fn, (cost_fn if self.has_cost else None)

    def __repr__(self):
        der = "derived=%r, " % (list(self.derived),) if self.derived else ""
        return "TaskRules(%r, %srequire_finite=%r, cost_on_term=%r)" % (list(self.clauses), der, self.require_finite, self.cost_on_term)


_TASKS = {}


def register_task(name, rules):
    """Make ``name`` resolvable wherever a task name is accepted (``FakeEnv(task=name)``, ``CMBPO(task=name)``).  The names
    of the built-in tasks (``_lib.TASK_IDS``) cannot be redefined."""
    if not isinstance(rules, TaskRules):
        raise TypeError("rules: a TaskRules, got %r" % (rules,))
    if name in _lib.TASK_IDS:
        raise ValueError("task %r is built in" % (name,))
    _TASKS[name] = rules
    return rules


def lookup(task):
    """``task`` (a name or a TaskRules) -> (rule id, TaskRules or None).  Unknown names are the default task, as in the
    reference (``models/fake_env.py:134-146``)."""
    if isinstance(task, TaskRules):
        return task.task_id, task
    if task in _TASKS:
        return _TASKS[task].task_id, _TASKS[task]
    return _lib.TASK_IDS.get(task, _lib.TASK_DEFAULT), None
