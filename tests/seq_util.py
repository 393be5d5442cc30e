"""Random operation sequences on ONE handle against the CPU oracle: host model, generator, adapters.

Every other comparison of a device path with the oracle takes a fresh driver, k Newton steps in one
policy and the same read-outs in the same order.  Here one driver object (and, through the handle
pool, one device handle) lives through a sequence of operations in a random order -- steps in both
call patterns, outer advances that change dt and / or rho, a new outer point, a new point between two
steps, read-outs in any order and number, and a round trip of the handle through the pool to another
user -- and after every operation that has an expectation the device is held to the model.

``SequenceModel`` is the host model.  The oracle is stateless in the point: a new ``NewtonOracle`` is a
new outer step and ``.step(x, y)`` takes the point, so the model of any call sequence is the tuple
(problem, kind, tau, x_hat, y_hat, dt, rho, x, y) and one oracle.  ``BatchModel`` is B of them plus the
frozen flags.

``sequence(seed, n_ops, adapter, B)`` is the deterministic generator.  Operations are tuples:

  single handle                                      device batch
  ("S", inertia)   step(inertia_check=inertia)       ("S",)  step_local()
  ("Y",)           step_async(); residual_norm();    ("A", dt, rho)  advance_outer
                   sync()  (bench.py's pattern)      ("E", dts, rhos, accepted)  advance_outer_each
  ("A", dt, rho)   advance_outer                     ("F", flags)  set_frozen
  ("O", vseed, far, dt, rho, start)  set_outer; vseed 0: at the point the handle holds
                                                     ("R", names)  points / masks / measures /
  ("P", vseed)     set_point, x clipped to the box                 residual_norms
  ("R", names)     point / mask / residual_norm / measures, in the order given
  ("H", kind)      close(), an interloper of kind a / b / c / d on the pooled handle, re-creation
                   from the model with start = (x, y)
  ("o", vseed, dt, rho)  regression cases only, Full and ActiveSet: pgf_set_outer through the C ABI
                   alone -- a new outer step at new hats while the device point stays

Vectors are not stored in the operation: ``op_vectors`` derives them from the problem's shape and the
operation's ``vseed``, so a sequence is a short string (``opstr``) and a regression case an explicit
list.

The tie guard: a mask is ``p < lamb lb - 1e-8 or p > lamb ub + 1e-8``; where an entry of p sits within
rounding of a threshold the device and the oracle may disagree without either being wrong.  The model
records, before every mask evaluation, the distance of p from the two thresholds relative to
max(1, max |p|); a sequence whose smallest margin is below 1e-8 (100 times the bar on the point) is
replaced by the next seed (seed + NEXT_SEED).  This is a condition on the input, not a tolerance; the
host test caps the share of replaced sequences.

The bars (none new): masks bit for bit; x and y within ``golden_util.rel_err`` 1e-10
(test_gpu_parity.TOL); diff within 1e-10 max(1, the model's diff), the residual norm within 1e-9 of the scale of
test_device_resident_newton, n_neg == m; measures within rtol 1e-11 / atol 1e-13 of ``Iterate`` at the
point the device holds, as in test_measures.test_batch_measures (that bar is tighter than the one on
the point, so it is held at the device's own point, which the same read-out holds to the model); no LU
fall-back; batch status zero.

``python tests/seq_util.py replay <adapter> <seed> [--upto k]`` runs one committed sequence on the GPU
and prints the errors of every operation.
"""

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import newton_oracle as O  # noqa: E402
from tests import golden_util as G  # noqa: E402

TOL = 1e-10  # test_gpu_parity.TOL
MARGIN_BAR = 1e-8  # tie guard: 100 x TOL
NEXT_SEED = 1000  # a replaced sequence takes seed + NEXT_SEED
DTS = (0.1, 0.5, 1.0, 10.0, 1000.0)
RHOS = (0.1, 1.0, 10.0)
POLICIES = ("Full", "Simplified", "ActiveSet")
READS = ("point", "mask", "residual_norm", "measures")
BATCH_READS = ("points", "masks", "measures", "residual_norms")
ADAPTERS = ("dense", "band", "dense_batch", "band_batch")


# ------------------------------------------------------------------ operations
def op_vectors(problem, vseed, far=False, clip=False):
    """(x, y) of an operation: 0.3 N(0, 1), or for ``far`` +-3 (1 + 0.1 U) in x -- far enough outside
    every box of the committed problems that, at a small dt, every boxed variable is active."""
    n, m = problem.num_vars, problem.num_cons
    rng = np.random.default_rng([int(vseed), 77])
    if far:
        x = np.where(rng.random(n) < 0.5, -3.0, 3.0) * (1.0 + 0.1 * rng.random(n))
    else:
        x = 0.3 * rng.standard_normal(n)
    y = 0.3 * rng.standard_normal(m)
    if clip:
        x = np.clip(x, problem.var_lb, problem.var_ub)
    return x, y


def _num(v):
    return f"{v:g}"


def opstr(ops):
    """The sequence as one short string, for messages."""
    out = []
    for op in ops:
        k = op[0]
        if k == "S":
            out.append("Si" if len(op) > 1 and op[1] else "S")
        elif k == "A":
            out.append(f"A({_num(op[1])},{_num(op[2])})")
        elif k == "O":
            out.append(f"O({op[1]}{'f' if op[2] else ''},{_num(op[3])},{_num(op[4])}{',s' if op[5] else ''})")
        elif k == "P":
            out.append(f"P({op[1]})")
        elif k == "o":
            out.append(f"o({op[1]},{_num(op[2])},{_num(op[3])})")
        elif k == "R":
            out.append("R[" + ",".join(n[:2] for n in op[1]) + "]")
        elif k == "H":
            out.append(f"H{op[1]}")
        elif k == "E":
            out.append("E(" + ",".join(f"{_num(d)}/{_num(r)}/{'+' if a else '-'}"
                                       for d, r, a in zip(op[1], op[2], op[3])) + ")")
        elif k == "F":
            out.append("F(" + "".join("1" if f else "0" for f in op[1]) + ")")
        else:
            out.append(k)
    return " ".join(out)


class Seq:
    """A sequence: the policy-independent start (tau, dt, rho, the seed of the first outer point) and
    the operations."""

    def __init__(self, tau, dt, rho, vseed, ops):
        self.tau, self.dt, self.rho, self.vseed, self.ops = tau, dt, rho, vseed, list(ops)

    def key(self):
        return (self.tau, self.dt, self.rho, self.vseed, tuple(self.ops))


def _draw(rng, keep, values, p_keep):
    return keep if rng.random() < p_keep else float(rng.choice(values))


def _draw_outer(rng, dt, rho):
    """(dt', rho') of a new outer step: both drawn anew (either may come out as it was), rho alone,
    dt alone, or neither."""
    mode = rng.random()
    other_rho = float(rng.choice([r for r in RHOS if r != rho]))
    other_dt = float(rng.choice([d for d in DTS if d != dt]))
    if mode < 0.4:
        return float(rng.choice(DTS)), float(rng.choice(RHOS))
    if mode < 0.7:
        return dt, other_rho
    if mode < 0.85:
        return other_dt, rho
    return dt, rho


def sequence(seed, n_ops=14, adapter="dense", B=0):
    """Deterministic in (seed, n_ops, adapter, B).  The first operation is a step, about half are
    steps, the last reads everything out.  A new outer step draws (dt, rho) by ``_draw_outer``: either
    can stay and rho can change alone."""
    rng = np.random.default_rng([int(seed), ADAPTERS.index(adapter), int(n_ops), int(B)])
    tau = 0.05 if rng.random() < 0.25 else None
    dt, rho = float(rng.choice(DTS[:4])), float(rng.choice(RHOS))
    vseed = int(rng.integers(1 << 20))
    batch = adapter.endswith("_batch")
    ops, steps = [], 0
    cur_dt, cur_rho = dt, rho
    kinds = "abcd" if adapter == "dense" else "ab"
    for i in range(n_ops - 1):
        if i == 0 or rng.random() < 0.5:
            if batch:
                ops.append(("S",))
            elif i > 0 and rng.random() < 0.35:
                ops.append(("Y",))
            else:
                steps += 1
                ops.append(("S", steps % 3 == 0))
            continue
        if batch:
            k = str(rng.choice(["A", "E", "F", "R"], p=[0.25, 0.35, 0.2, 0.2]))
            if k == "A":
                cur_dt, cur_rho = _draw_outer(rng, cur_dt, cur_rho)
                ops.append(("A", cur_dt, cur_rho))
            elif k == "E":
                dts = tuple(_draw(rng, cur_dt, DTS, 1 / 3) for _ in range(B))
                rhos = tuple(_draw(rng, cur_rho, RHOS, 0.5) for _ in range(B))
                ops.append(("E", dts, rhos, tuple(bool(v) for v in rng.random(B) < 0.6)))
            elif k == "F":
                ops.append(("F", tuple(bool(v) for v in rng.random(B) < 0.4)))
            else:
                names = [n for n in rng.permutation(BATCH_READS) if rng.random() < 0.6]
                ops.append(("R", tuple(str(n) for n in names) or ("points",)))
            continue
        k = str(rng.choice(["A", "O", "P", "R", "H"], p=[0.25, 0.2, 0.2, 0.2, 0.15]))
        if k == "A":
            cur_dt, cur_rho = _draw_outer(rng, cur_dt, cur_rho)
            ops.append(("A", cur_dt, cur_rho))
        elif k == "O":
            cur_dt, cur_rho = _draw_outer(rng, cur_dt, cur_rho)
            if rng.random() < 0.35:  # at the point the handle holds (vseed 0)
                ops.append(("O", 0, False, cur_dt, cur_rho, False))
            else:
                ops.append(("O", int(rng.integers(1, 1 << 20)), bool(rng.random() < 0.4), cur_dt, cur_rho,
                            bool(rng.random() < 0.5)))
        elif k == "P":
            ops.append(("P", int(rng.integers(1 << 20))))
        elif k == "R":
            names = [n for n in rng.permutation(READS) if rng.random() < 0.6]
            ops.append(("R", tuple(str(n) for n in names) or ("point",)))
        else:
            ops.append(("H", str(rng.choice(list(kinds)))))
    ops.append(("R", BATCH_READS if batch else READS))
    return Seq(tau, dt, rho, vseed, ops)


# ------------------------------------------------------------------ host model
def residual_norm_of(problem, x_hat, y_hat, dt, rho, x, y):
    pt = O.PointData(problem, x, y)
    return float(np.linalg.norm(O.unscaled_residual(dt, x_hat, y_hat, pt.x, pt.y, pt.g(rho), pt.cons,
                                                    problem.var_lb, problem.var_ub)))


def hess_scale(problem):
    """max row sum of |H|: the scale of the residual norm's rounding (test_device_resident_newton)."""
    H = abs(problem.hess_sparse())
    return float(H.sum(axis=1).max()) if H.shape[0] else 0.0


def measures_of(problem, x, y):
    from pygradflow_amd.iterate import Iterate
    from pygradflow_amd.params import Params

    it = Iterate(problem, Params(), np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    return np.array([it.stat_res, it.cons_violation, it.bound_violation,
                     float(np.max(np.abs(y))) if len(y) else 0.0])


class SequenceModel:
    """(problem, kind, tau, x_hat, y_hat, dt, rho, x, y) and one NewtonOracle.  ``apply(op)`` moves the
    state and returns what the device must show: a dict with some of diff, n_neg, x, y, mask,
    residual_norm, measures (True: to be taken at the device's point), lu."""

    def __init__(self, problem, kind, tau, x_hat, y_hat, dt, rho, start=None):
        self.problem, self.kind, self.tau = problem, kind, tau
        self.n, self.m = problem.num_vars, problem.num_cons
        self.min_margin = np.inf
        self.sizes = []  # |I| of every step
        self.rho_alone = 0  # advances that changed rho and nothing else
        self.p_between_steps = 0  # a P with a step before it and a step as the next state change
        self._stepped = self._p_pending = False
        self._outer(x_hat, y_hat, dt, rho, start)

    # -- state
    def _outer(self, x_hat, y_hat, dt, rho, start=None):
        self.x_hat, self.y_hat = np.array(x_hat, dtype=np.float64), np.array(y_hat, dtype=np.float64)
        self.dt, self.rho = float(dt), float(rho)
        if start is None:
            self.x, self.y = self.x_hat.copy(), self.y_hat.copy()
        else:
            self.x, self.y = np.array(start[0], dtype=np.float64), np.array(start[1], dtype=np.float64)
        self._new_oracle()

    def _new_oracle(self):
        if self.kind == "Simplified":  # the mask is taken here, at the outer point
            self._guard(self.x_hat, self.y_hat)
        self.oracle = O.NewtonOracle(self.problem, self.kind, self.x_hat, self.y_hat, self.dt, self.rho,
                                     self.tau)
        self.mask = None  # expected from mask() only after a step
        self._stepped = self._p_pending = False

    def _guard(self, x, y):
        pt = O.PointData(self.problem, x, y)
        p = O.projection_initial(self.dt, self.x_hat, pt.x, pt.g(self.rho), self.tau)
        lamb = 1.0 / self.dt
        lo, hi = lamb * self.problem.var_lb - O.ACTIVE_EPS, lamb * self.problem.var_ub + O.ACTIVE_EPS
        with np.errstate(invalid="ignore"):
            d = np.minimum(np.abs(p - lo), np.abs(p - hi))
        if d.size:
            self.min_margin = min(self.min_margin, float(d.min() / max(1.0, np.max(np.abs(p)))))

    def residual_norm(self):
        return residual_norm_of(self.problem, self.x_hat, self.y_hat, self.dt, self.rho, self.x, self.y)

    def _step(self):
        if self.kind != "Simplified":
            self._guard(self.x, self.y)
        xn, yn, diff = self.oracle.step(self.x, self.y)
        self.x, self.y = xn, yn
        self.mask = self.oracle.solver.record["mask"].copy()
        self.sizes.append(int(self.n - self.mask.sum()))
        if self._p_pending:
            self.p_between_steps += 1
        self._stepped, self._p_pending = True, False
        return dict(diff=float(diff), n_neg=self.m)

    def read(self, name):
        if name in ("point", "points"):
            return dict(x=self.x.copy(), y=self.y.copy())
        if name in ("mask", "masks"):
            return {} if self.mask is None else dict(mask=self.mask.copy())
        if name in ("residual_norm", "residual_norms"):
            return dict(residual_norm=self.residual_norm())
        assert name == "measures", name
        return dict(measures=True, x=self.x.copy(), y=self.y.copy())

    def apply(self, op):
        k = op[0]
        if k == "S":
            return self._step()
        if k == "Y":
            exp = self._step()
            exp["residual_norm"] = self.residual_norm()
            return exp
        if k == "A":
            if op[1] == self.dt and op[2] != self.rho:
                self.rho_alone += 1
            self._outer(self.x, self.y, op[1], op[2])
            return {}
        if k == "O":
            xh, yh = (self.x, self.y) if op[1] == 0 else op_vectors(self.problem, op[1], far=op[2])
            start = op_vectors(self.problem, op[1] + 1) if op[5] else None
            self._outer(xh, yh, op[3], op[4], start)
            return {}
        if k == "P":
            self.x, self.y = op_vectors(self.problem, op[1], clip=True)
            self._p_pending = self._stepped
            return {}
        if k == "o":
            assert self.kind != "Simplified", "its mask is taken at the outer point: set_outer"
            self._outer(*op_vectors(self.problem, op[1]), op[2], op[3], start=(self.x, self.y))
            return {}
        if k == "R":
            exp = {}
            for name in op[1]:
                exp.update(self.read(name))
            return exp
        assert k == "H", op
        self._new_oracle()  # as the constructor implies; the point stays (start = (x, y))
        return dict(lu=0)


class BatchModel:
    """B independent SequenceModels, the frozen flags and the rule of a rejected instance: back to its
    outer point before the new outer step (what ``sequential=True`` of batched.py spells out).  The
    batch starts every instance at zero with an outer step there."""

    def __init__(self, problems, kind, tau, dt, rho):
        self.models = [SequenceModel(p, kind, tau, np.zeros(p.num_vars), np.zeros(p.num_cons), dt, rho)
                       for p in problems]
        self.B = len(problems)
        self.frozen = np.zeros(self.B, dtype=bool)
        self.mask_ready = False  # a step since the last advance: masks() answers
        self.rejected_moved = 0  # rejections of an instance that had left its outer point
        self.frozen_steps = 0  # instance steps sat out

    @property
    def min_margin(self):
        return min(m.min_margin for m in self.models)

    def apply(self, op):
        k, ms = op[0], self.models
        if k == "S":
            live = ~self.frozen
            self.mask_ready = True
            self.frozen_steps += int(self.frozen.sum())
            recs = [m._step() if live[i] else None for i, m in enumerate(ms)]
            return dict(status=np.zeros(self.B, dtype=np.int32), live=live,
                        diff=np.array([r["diff"] if r else 0.0 for r in recs]),
                        n_neg=np.array([m.m for m in ms]))
        if k == "A":
            for m in ms:
                m.apply(("A", op[1], op[2]))
            self.frozen[:] = False
            self.mask_ready = False
            return {}
        if k == "E":
            for i, m in enumerate(ms):
                if not op[3][i]:
                    self.rejected_moved += int(m._stepped)
                    m.x, m.y = m.x_hat.copy(), m.y_hat.copy()
                m.apply(("A", op[1][i], op[2][i]))
            self.frozen[:] = False
            self.mask_ready = False
            return {}
        if k == "F":
            self.frozen = np.array(op[1], dtype=bool)
            return {}
        assert k == "R", op
        exp = {}
        for name in op[1]:
            rows = [m.read(name) for m in ms]
            if name == "masks":
                if self.mask_ready:
                    exp["mask"] = [r.get("mask") for r in rows]  # None: no expectation for that instance
            elif name == "residual_norms":
                exp["residual_norm"] = np.array([r["residual_norm"] for r in rows])
            else:
                if name == "measures":
                    exp["measures"] = True
                exp["x"] = np.array([r["x"] for r in rows])
                exp["y"] = np.array([r["y"] for r in rows]).reshape(self.B, -1)
        return exp


# ------------------------------------------------------------------ comparison
class SequenceFailure(AssertionError):
    pass


def _cmp_one(problem, exp, got, scale_h, errs, tag=""):
    """One instance's expectations against what the driver showed; fills ``errs`` (quantity -> error)
    and returns the first quantity that misses its bar, or None."""
    bad = None

    def note(name, err, ok):
        nonlocal bad
        errs[name + tag] = max(errs.get(name + tag, 0.0), float(err))
        if not ok and bad is None:
            bad = f"{name}{tag} (error {err:.3e})"

    if "lu" in exp:
        note("lu", got["lu"], got["lu"] == exp["lu"])
    if "n_neg" in exp:
        note("n_neg", abs(int(got["n_neg"]) - int(exp["n_neg"])), int(got["n_neg"]) == int(exp["n_neg"]))
    if "diff" in exp:
        d = abs(got["diff"] - exp["diff"])  # (scaled by the model's value: a wrong device value cannot widen it)
        note("diff", d / max(1.0, abs(exp["diff"])), d <= TOL * max(1.0, abs(exp["diff"])))
    if exp.get("mask") is not None:
        flips = int(np.count_nonzero(np.asarray(got["mask"], dtype=bool) != exp["mask"]))
        note("mask", flips, flips == 0)
    if "x" in exp:
        for nm in ("x", "y"):
            e = G.rel_err(got[nm], exp[nm])
            note(nm, e, e <= TOL)
    if "residual_norm" in exp:
        xs = exp["x"] if "x" in exp else got.get("x_for_scale")
        xmax = float(np.max(np.abs(xs))) if xs is not None and np.size(xs) else 0.0
        scale = max(1.0, exp["residual_norm"], scale_h * xmax)
        d = abs(got["residual_norm"] - exp["residual_norm"])
        note("residual_norm", d / scale, d <= 1e-9 * scale)
    if exp.get("measures"):
        want = measures_of(problem, got["x"], got["y"])
        ok = bool(np.allclose(got["measures"], want, rtol=1e-11, atol=1e-13))
        e = float(np.max(np.abs(got["measures"] - want) / (1e-13 / 1e-11 + np.abs(want))))
        note("measures", e, ok)
    return bad


def compare(case, model, exp, got, errs):
    """None, or the first quantity that misses its bar."""
    if not case.batch:
        got = dict(got)
        got.setdefault("x_for_scale", model.x)
        return _cmp_one(case.problem(0), exp, got, case.hess_scale(0), errs)
    if "status" in exp:
        if np.any(np.asarray(got["status"]) != 0):
            errs["status"] = 1.0
            return f"status {list(got['status'])}"
        errs.setdefault("status", 0.0)
    for i in range(model.B):
        e, g = {}, {}
        if "live" in exp:
            if not exp["live"][i]:
                continue
            e = dict(diff=exp["diff"][i], n_neg=exp["n_neg"][i])
            g = dict(diff=got["diff"][i], n_neg=got["n_neg"][i])
        for nm in ("x", "y", "residual_norm"):
            if nm in exp:
                e[nm], g[nm] = exp[nm][i], got[nm][i]
        if "mask" in exp and exp["mask"][i] is not None:
            e["mask"], g["mask"] = exp["mask"][i], got["mask"][i]
        if exp.get("measures"):
            e["measures"], g["measures"] = True, got["measures"][i]
        g["x_for_scale"] = model.models[i].x
        bad = _cmp_one(case.problem(i), e, g, case.hess_scale(i), errs)
        if bad:
            return f"instance {i}: {bad}"
    return None


# ------------------------------------------------------------------ adapters
class SingleAdapter:
    """open / apply(op) / close over a driver with DeviceNewton's surface.  ``backend.new(problem, kind,
    x_hat, y_hat, dt, rho, tau, start)`` creates one; ``backend.interlope(kind, case)`` is another user
    of the pooled handle."""

    def __init__(self, case, backend):
        self.case, self.backend, self.dn = case, backend, None

    def _create(self, model, start=None):
        self.dn = self.backend.new(self.case.problem(0), model.kind, model.x_hat, model.y_hat, model.dt,
                                   model.rho, model.tau, start)
        self._lu0 = self.dn.refinement_stats()[1]

    def _drop(self):
        lu = self.dn.refinement_stats()[1] - self._lu0
        self.dn.close()
        self.dn = None
        return lu

    def open(self, model):
        self._create(model)

    def _read(self, name, got, model):
        dn = self.dn
        if name == "point":
            got["x"], got["y"] = dn.point()
        elif name == "mask":
            if model.mask is not None:  # (a new outer step has dropped the mask: mask() refuses, rightly)
                got["mask"] = dn.mask()
        elif name == "residual_norm":
            got["residual_norm"] = dn.residual_norm()
        else:
            ms = dn.measures()
            got["measures"] = np.array([ms["stat_res"], ms["cons_violation"], ms["bound_violation"], ms["y_inf"]])
            got["x"], got["y"] = dn.point()

    def apply(self, op, model):
        """``model`` is the host model AFTER the operation: H re-creates the driver from it."""
        dn, k, prob = self.dn, op[0], self.case.problem(0)
        got = {}
        if k == "S":
            got["diff"], got["n_neg"] = dn.step(inertia_check=bool(op[1]))
        elif k == "Y":
            dn.step_async()
            got["residual_norm"] = dn.residual_norm()
            got["diff"], got["n_neg"] = dn.sync()
        elif k == "A":
            dn.advance_outer(op[1], op[2])
        elif k == "O":
            xh, yh = (model.x_hat, model.y_hat) if op[1] == 0 else op_vectors(prob, op[1], far=op[2])
            dn.set_outer(xh, yh, op[3], op[4], start=op_vectors(prob, op[1] + 1) if op[5] else None)
        elif k == "P":
            dn.set_point(*op_vectors(prob, op[1], clip=True))
        elif k == "o":
            self.backend.set_outer_keeping_point(dn, *op_vectors(prob, op[1]), op[2], op[3])
        elif k == "R":
            for name in op[1]:
                self._read(name, got, model)
        else:
            got["lu"] = self._drop()
            self.backend.interlope(op[1], self.case)
            self._create(model, start=(model.x, model.y))
        return got

    def close(self):
        return self._drop() if self.dn is not None else 0


class BatchAdapter:
    """The same over BatchedDeviceNewton's surface; ``backend.new_batch(case, kind, tau, dt, rho)``."""

    def __init__(self, case, backend):
        self.case, self.backend, self.bd = case, backend, None

    def open(self, model):
        m0 = model.models[0]
        self.bd = self.backend.new_batch(self.case, m0.kind, m0.tau, m0.dt, m0.rho)

    def apply(self, op, model):
        bd, k = self.bd, op[0]
        got = {}
        if k == "S":
            got["status"], got["n_neg"], got["diff"] = bd.step_local()
        elif k == "A":
            bd.advance_outer(op[1], op[2])
        elif k == "E":
            bd.advance_outer_each(np.array(op[1]), np.array(op[2]), np.array(op[3], dtype=bool))
        elif k == "F":
            bd.set_frozen(np.array(op[1], dtype=bool))
        else:
            for name in op[1]:
                if name == "points":
                    got["x"], got["y"] = bd.points()
                elif name == "masks":
                    if model.mask_ready:  # (the batch has one flag: a step since the last advance)
                        got["mask"] = bd.masks()
                elif name == "residual_norms":
                    got["residual_norm"] = bd.residual_norms_local()
                else:
                    got["measures"] = bd.measures()
                    got["x"], got["y"] = bd.points()
        return got

    def close(self):
        lu = 0
        if self.bd is not None:
            lu = self.backend.batch_lu(self.bd)
            self.bd.close()
            self.bd = None
        return lu


# ------------------------------------------------------------------ the GPU backend
class DeviceBackend:
    """DeviceNewton / BatchedDeviceNewton and the interlopers of the handle pool."""

    def new(self, problem, kind, x_hat, y_hat, dt, rho, tau, start):
        from pygradflow_amd.newton import DeviceNewton

        return DeviceNewton(problem, kind, x_hat, y_hat, dt, rho, tau, start=start)

    def new_batch(self, case, kind, tau, dt, rho):
        from pygradflow_amd.batched import BatchedDeviceNewton

        bd = BatchedDeviceNewton(case.problem, case.B, kind, dt, rho, tau=tau, **case.batch_flags)
        self._lu0 = sum(s.refinement_stats()[1] for s in bd.solvers)
        return bd

    def batch_lu(self, bd):
        return sum(s.refinement_stats()[1] for s in bd.solvers) - self._lu0

    def set_outer_keeping_point(self, dn, x_hat, y_hat, dt, rho):
        """pgf_set_outer alone.  No public call sequence of DeviceNewton reaches this state: its set_outer
        always sends a point behind pgf_set_outer, which clears what was evaluated ahead; a caller of the C
        ABI may keep the point.  Hence the handle and library taken from the driver's private members, and
        its dt, rho kept in step by hand.  (The batch has no such call: pgf_batch_advance_outer_each is its
        only way to a new outer step, and it drops the evaluation when an instance's rho changes.)"""
        from pygradflow_amd import _lib

        xh, yh = _lib.as_f64(x_hat), _lib.as_f64(y_hat)
        _lib.check(dn._lib.pgf_set_outer(dn._hd.h, _lib.dptr(xh), _lib.dptr(yh), float(dt), float(rho)),
                   dn._hd.h, "pgf_set_outer")
        dn.dt, dn.rho = float(dt), float(rho)

    def interlope(self, kind, case):
        """One step of another user of the handle's pool slot, on another problem of the same (n, m);
        checked only for raising nothing."""
        import pygradflow_amd as pgf
        from pygradflow_amd.batched import BatchedDeviceNewton

        other = case.problem(1)
        n, m = other.num_vars, other.num_cons
        x0, y0 = np.zeros(n), np.zeros(m)
        if kind == "a":
            pol = POLICIES[(POLICIES.index(case.policy) + 1) % 3]
            dn = pgf.DeviceNewton(other, pol, x0, y0, 1.0, 1.0)
            dn.step()
            dn.close()
        elif kind == "b":
            params = pgf.Params(newton_type="Full", step_solver=pgf.HipStepSolver)
            gen = pgf.newton_steps(other, params, pgf.Iterate(other, params, x0, y0), 1.0, 1.0)
            next(gen)
            gen.close()  # drops the method and with it the step solver: its handle returns to the pool
            del gen
        elif kind == "c":
            dn = pgf.DeviceNewton(other, "Full", x0, y0, 1.0, 1.0,
                                  step_solver_type=("Standard", "Extended")[case.seed % 2])
            dn.step()
            dn.close()
        else:
            assert kind == "d", kind
            bd = BatchedDeviceNewton(lambda i: case.problem(1 + i), 2, "Full", 1.0, 1.0)
            bd.step_local()
            bd.close()


# ------------------------------------------------------------------ the numpy backend (host test)
DEFECTS = {
    1: "factor kept over rho",
    2: "mask over set_outer",
    3: "stale step on set_point",
    4: "problem not restored",
    5: "rejection ignored",
}


class FakeDriver:
    """A pure-numpy driver with DeviceNewton's surface around the oracle.  It keeps the kinds of state
    the device keeps -- the factor, the ActiveSet mask, the point the next step was evaluated at, the
    vectors resident for the handle -- so that each can be left stale on purpose (``defect``)."""

    def __init__(self, pool, problem, kind, x_hat, y_hat, dt, rho, tau, start=None, defect=None):
        self.pool, self.kind, self.tau, self.defect = pool, kind, tau, defect
        self.n, self.m = problem.num_vars, problem.num_cons
        last = pool.get("qp")
        if defect == 4 and last is not None and last is not problem:
            from pygradflow_amd.problems import LinearQuadraticProblem

            problem = LinearQuadraticProblem(problem.Q, last.q, problem.A, last.b, problem.var_lb, problem.var_ub)
        else:
            pool["qp"] = problem
        self.problem = problem
        self.oracle = None
        self.set_outer(x_hat, y_hat, dt, rho, start)

    def _begin(self, x_hat, y_hat, dt, rho, keep_factor=False, keep_mask=False):
        old = self.oracle
        new = O.NewtonOracle(self.problem, self.kind, x_hat, y_hat, dt, rho, self.tau)
        if old is not None and old.solver._lu is not None:
            so, sn = old.solver, new.solver
            if keep_factor:  # the factor of a K that is stale in rho alone (the mask is the new one)
                sn._hess_rows = O.shifted_hess_rows(sn.hess, sn.lamb, sn.mask)
                sn._K = O.kkt_matrix(sn._hess_rows, sn.jac, sn.mask, sn.lamb, so.rho)
                sn._lu = O.factor_kkt(sn._K)
            if keep_mask:
                new._curr_mask = old._curr_mask
                sn.mask, sn._hess_rows, sn._K, sn._lu = so.mask, so._hess_rows, so._K, so._lu
        self.oracle = new
        self.x_hat, self.y_hat, self.dt, self.rho = np.array(x_hat), np.array(y_hat), float(dt), float(rho)

    def set_outer(self, x_hat, y_hat, dt, rho, start=None):
        self._begin(x_hat, y_hat, dt, rho, keep_mask=self.defect == 2 and self.kind == "ActiveSet")
        self.x, self.y = (np.array(x_hat), np.array(y_hat)) if start is None else (np.array(start[0]), np.array(start[1]))
        self._ahead = (self.x, self.y)

    def advance_outer(self, dt, rho):
        rho_alone = dt == self.dt and rho != self.rho
        self._begin(self.x, self.y, dt, rho,
                    keep_factor=self.defect == 1 and self.kind == "Simplified" and rho_alone)
        self._ahead = (self.x, self.y)

    def step(self, inertia_check=False):
        xn, yn, diff = self.oracle.step(*self._ahead)
        self.x, self.y = xn, yn
        self._ahead = (xn, yn)
        self._mask = self.oracle.solver.record["mask"]
        return float(diff), self.m

    def step_async(self):
        self._pending = self.step()

    def sync(self):
        return self._pending

    def set_point(self, x, y):
        self.x, self.y = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)
        if self.defect != 3:
            self._ahead = (self.x, self.y)

    def point(self):
        return self.x.copy(), self.y.copy()

    def mask(self):
        return np.array(getattr(self, "_mask", np.zeros(self.n, dtype=bool)))  # (before a step: no expectation)

    def residual_norm(self):
        return residual_norm_of(self.problem, self.x_hat, self.y_hat, self.dt, self.rho, self.x, self.y)

    def measures(self):
        v = measures_of(self.problem, self.x, self.y)
        return dict(stat_res=v[0], cons_violation=v[1], bound_violation=v[2], y_inf=v[3])

    def refinement_stats(self):
        return 0, 0, 0.0

    def close(self):
        pass


class FakeBatch:
    def __init__(self, drivers, defect):
        self.drivers, self.defect = drivers, defect
        self.frozen = np.zeros(len(drivers), dtype=bool)
        for d in drivers:
            d.advance_outer(d.dt, d.rho)
        self.solvers = drivers

    def step_local(self):
        B = len(self.drivers)
        st, nn, df = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B)
        for i, d in enumerate(self.drivers):
            if not self.frozen[i]:
                df[i], nn[i] = d.step()
        return st, nn, df

    def advance_outer(self, dt, rho):
        self.advance_outer_each([dt] * len(self.drivers), [rho] * len(self.drivers), None)

    def advance_outer_each(self, dt, rho, accepted):
        for i, d in enumerate(self.drivers):
            if accepted is not None and not accepted[i] and self.defect != 5:
                d.set_point(d.x_hat, d.y_hat)
            d.advance_outer(float(dt[i]), float(rho[i]))
        self.frozen[:] = False

    def set_frozen(self, flags):
        self.frozen = np.array(flags, dtype=bool)

    def points(self):
        return (np.array([d.x for d in self.drivers]),
                np.array([d.y for d in self.drivers]).reshape(len(self.drivers), -1))

    def masks(self):
        return np.array([getattr(d, "_mask", np.zeros(d.n, dtype=bool)) for d in self.drivers])

    def measures(self):
        return np.array([measures_of(d.problem, d.x, d.y) for d in self.drivers])

    def residual_norms_local(self):
        return np.array([d.residual_norm() for d in self.drivers])

    def close(self):
        pass


class FakeBackend:
    def __init__(self, defect=None):
        self.defect, self.pool = defect, {}

    def new(self, problem, kind, x_hat, y_hat, dt, rho, tau, start):
        return FakeDriver(self.pool, problem, kind, x_hat, y_hat, dt, rho, tau, start, self.defect)

    def new_batch(self, case, kind, tau, dt, rho):
        ds = []
        for i in range(case.B):
            p = case.problem(i)
            ds.append(FakeDriver({}, p, kind, np.zeros(p.num_vars), np.zeros(p.num_cons), dt, rho, tau,
                                 None, self.defect))
        return FakeBatch(ds, self.defect)

    def batch_lu(self, bd):
        return 0

    def set_outer_keeping_point(self, dn, x_hat, y_hat, dt, rho):
        dn.set_outer(x_hat, y_hat, dt, rho, start=(dn.x, dn.y))

    def interlope(self, kind, case):
        other = case.problem(1)
        d = FakeDriver(self.pool, other, "Full", np.zeros(other.num_vars), np.zeros(other.num_cons), 1.0, 1.0, None)
        d.step()


# ------------------------------------------------------------------ committed cases
def _other_bounds(prob, make):
    """The interloper's problem: ``make()`` (another seed) with every finite bound halved, the band
    settings of ``prob`` carried over."""
    from pygradflow_amd.problems import LinearQuadraticProblem

    o = make()
    new = LinearQuadraticProblem(o.Q, o.q, o.A, o.b, 0.5 * o.var_lb, 0.5 * o.var_ub)
    for att in ("pgf_force_band", "pgf_band_block", "pgf_band_split", "pgf_border", "pgf_border_limit"):
        if hasattr(prob, att):
            setattr(new, att, getattr(prob, att))
    return new


# (n, m, boxed_frac, box, policy): m >= 64 four times; n_I + m above 512 for the three n = 513 shapes
DENSE_SHAPES = [
    (100, 20, 0.3, 0.05, "Full"), (100, 33, 0.7, 0.01, "Simplified"), (100, 0, 0.05, 0.5, "ActiveSet"),
    (257, 64, 0.3, 0.05, "ActiveSet"), (257, 40, 0.0, 0.01, "Full"), (257, 85, 0.7, 0.05, "Simplified"),
    (300, 100, 0.05, 0.01, "Full"), (300, 56, 0.3, 0.5, "Simplified"), (300, 80, 0.7, 0.01, "ActiveSet"),
    (513, 100, 0.05, 0.05, "Full"), (513, 171, 0.0, 0.01, "Simplified"), (513, 64, 0.3, 0.01, "ActiveSet"),
]

BAND_PROBLEMS = ("sparse_ocp60", "box_qp300", "ms40_split", "ms40_nosplit", "ms30_split", "ms30_nosplit",
                 "budget300", "ocp_param30")
BATCH_BAND_PROBLEMS = ("box_qp300", "ms40_wide")


def _band_problem(name, seed):
    from pygradflow_amd import problems as P

    if name == "sparse_ocp60":
        p = P.sparse_ocp(60, seed=seed)
    elif name == "box_qp300":
        p = P.box_qp(300, seed=seed)
    elif name.startswith("ms40"):
        p = P.multistate_ocp(40, 4, 2, seed=seed)
    elif name.startswith("ms30"):
        p = P.multistate_ocp(30, 8, 4, seed=seed)
    elif name == "budget300":
        p = P.budget_box_qp(300, seed=seed)
    else:
        assert name == "ocp_param30", name
        p = P.ocp_global_parameter(30, 4, 2, 3, seed=seed)
    if name in ("budget300", "ocp_param30"):
        p.pgf_border = "auto"
    else:
        p.pgf_force_band = True
    if name.endswith("_split"):
        p.pgf_band_split = True
    elif name.endswith("_nosplit"):
        p.pgf_band_split = False
    return p


# Committed seeds are the case's index unless listed here.  Each replacement serves one mutant of
# test_seq_model_host.py, which the index's own sequence does not catch on that handle kind (re-pick them
# with that test if the generator changes):
#   mutant 1, factor kept over rho (a rho-only advance between two Simplified steps, m > 0):
#     dense 7 -> 607, band 1 -> 301 (sparse_ocp60), band 22 -> 822 (ocp_param30)
#   mutant 2, mask over set_outer (a set_outer behind an ActiveSet step after which the mask is the same):
#     dense 2 -> 902, dense 3 -> 903, band 11 -> 111 (ms40_nosplit), band 20 -> 620 (budget300)
SEEDS = {"dense": {2: 902, 3: 903, 7: 607}, "band": {1: 301, 11: 111, 20: 620, 22: 822}}


class Case:
    """One committed sequence: adapter, problem, policy, seed.  (adapter, seed) names it."""

    def __init__(self, adapter, name, policy, seed, make, B=0, batch_flags=None, ops=None, start=None):
        self.adapter, self.name, self.policy, self.seed = adapter, name, policy, seed
        self.batch, self.B, self.batch_flags = adapter.endswith("_batch"), B, dict(batch_flags or {})
        self._make, self._problems, self._scales = make, {}, {}
        self._fixed = None if ops is None else Seq(*start, ops)
        self._resolved = None

    @property
    def id(self):
        return f"{self.adapter}-{self.name}-{self.policy}-s{self.seed}"

    def problem(self, i):
        """single: 0 the problem, 1 (and 2) the interlopers'; batch: instance i."""
        if i not in self._problems:
            self._problems[i] = self._make(i)
        return self._problems[i]

    def hess_scale(self, i):
        if i not in self._scales:
            self._scales[i] = hess_scale(self.problem(i))
        return self._scales[i]

    def model(self, seq):
        if self.batch:
            return BatchModel([self.problem(i) for i in range(self.B)], self.policy, seq.tau, seq.dt, seq.rho)
        p = self.problem(0)
        xh, yh = op_vectors(p, seq.vseed)
        return SequenceModel(p, self.policy, seq.tau, xh, yh, seq.dt, seq.rho)

    def host_run(self, seq):
        """The model alone over the sequence; returns it (margins, sizes, counters)."""
        model = self.model(seq)
        for op in seq.ops:
            model.apply(op)
        return model

    def resolved(self):
        """(sequence, seed used, replaced): the seed's sequence, or -- tie guard -- the next one's."""
        if self._resolved is None:
            if self._fixed is not None:
                self._resolved = (self._fixed, self.seed, False)
            else:
                seed = self.seed
                for _ in range(4):
                    seq = sequence(seed, adapter=self.adapter, B=self.B)
                    if self.host_run(seq).min_margin >= MARGIN_BAR:
                        break
                    seed += NEXT_SEED
                else:
                    raise AssertionError(f"{self.id}: four seeds in a row with a tie")
                self._resolved = (seq, seed, seed != self.seed)
        return self._resolved


def _dense_case(i, ops=None, start=None, name=None, seed=None):
    from pygradflow_amd import problems as P

    n, m, frac, box, pol = DENSE_SHAPES[i]

    def make(k):
        if k == 0:
            return P.dense_qp(n, m, seed=500 + i, boxed_frac=frac, box=box)
        return P.dense_qp(n, m, seed=600 + 10 * i + k, boxed_frac=0.3 if frac != 0.3 else 0.05, box=2.0 * box)

    return Case("dense", name or f"n{n}m{m}", pol, SEEDS["dense"].get(i, i) if seed is None else seed, make,
                ops=ops, start=start)


def _band_case(j, pol_i, ops=None, start=None, name=None, seed=None):
    pname = BAND_PROBLEMS[j]

    def make(k):
        if k == 0:
            return _band_problem(pname, 40 + j)
        return _other_bounds(make(0), lambda: _band_problem(pname, 80 + j + k))

    idx = 3 * j + pol_i
    return Case("band", name or pname, POLICIES[pol_i], SEEDS["band"].get(idx, idx) if seed is None else seed, make,
                ops=ops, start=start)


def committed(adapter):
    """The committed cases of an adapter (regression cases with explicit operations included)."""
    from pygradflow_amd import problems as P

    if adapter == "dense":
        return [_dense_case(i) for i in range(len(DENSE_SHAPES))] + REGRESSIONS.get("dense", [])
    if adapter == "band":
        return [_band_case(j, k) for j in range(len(BAND_PROBLEMS)) for k in range(3)] + REGRESSIONS.get("band", [])
    if adapter == "dense_batch":
        return [Case("dense_batch", "n200m56", pol, 2 * k + r,
                     lambda i: P.dense_qp(200, 56, seed=10 + i, boxed_frac=0.1 * i, box=0.02), B=5)
                for k, pol in enumerate(POLICIES) for r in range(2)]
    assert adapter == "band_batch", adapter
    out = []
    for j, pname in enumerate(BATCH_BAND_PROBLEMS):
        for k, pol in enumerate(POLICIES):
            for r in range(2):
                if pname == "box_qp300":
                    make, flags = (lambda i: _band_problem("box_qp300", 20 + i)), {}
                else:
                    make, flags = (lambda i: _band_problem("ms40", 30 + i)), dict(wide_band=True)
                out.append(Case("band_batch", pname, pol, 6 * j + 2 * k + r, make, B=4, batch_flags=flags))
    return out


# Named regression sequences (explicit operations, not seeds): adapter -> [Case].
#
# set_outer_keeps_rho_stale_eval: pgf_set_outer with a new rho left eval_fresh set, so a step behind
# it used g = grad f + J'(rho c + y) of the OLD rho wherever g, c had been evaluated at the device
# point before -- ahead of the host's wait by the dense step, by residual_norm() on the banded handle.
# pgf_qp_advance_outer had the line; DeviceNewton.set_outer hid the gap by sending a point behind every
# pgf_set_outer.  Found by reading, while modelling what each operation invalidates.
REGRESSIONS = {
    "dense": [_dense_case(0, ops=[("S", False), ("o", 5, 1.0, 10.0), ("S", False), ("R", READS)],
                          start=(None, 1.0, 1.0, 3), name="set_outer_keeps_rho_stale_eval", seed=9001)],
    "band": [_band_case(0, 0, ops=[("S", False), ("R", ("residual_norm",)), ("o", 5, 1.0, 10.0), ("S", False),
                                   ("R", READS)],
                        start=(None, 1.0, 1.0, 3), name="set_outer_keeps_rho_stale_eval", seed=9001)],
}


# ------------------------------------------------------------------ runner
def run_sequence(case, backend, upto=None, report=None):
    """The case's sequence on ``backend`` against the model.  Raises SequenceFailure naming the adapter,
    the seed, the operations, the first failing one and the quantity; returns quantity -> worst error.
    ``report(i, op, errs)`` sees every operation's errors."""
    seq, seed, _ = case.resolved()
    model = case.model(seq)
    ad = (BatchAdapter if case.batch else SingleAdapter)(case, backend)
    worst = {}
    ops = seq.ops if upto is None else seq.ops[:upto]

    def fail(i, what):
        raise SequenceFailure(f"{case.id} (adapter {case.adapter}, seed {seed}, tau {seq.tau}, dt {seq.dt:g}, "
                              f"rho {seq.rho:g}): ops [{opstr(seq.ops)}]: first failing op {i} "
                              f"[{opstr(ops[i:i + 1]) if i < len(ops) else 'close'}]: {what}")

    ad.open(model)
    try:
        for i, op in enumerate(ops):
            exp = model.apply(op)
            try:
                got = ad.apply(op, model)
            except SequenceFailure:
                raise
            except Exception as e:  # the driver raised: part of the finding, with its place
                fail(i, f"raised {type(e).__name__}: {e}")
            errs = {}
            bad = compare(case, model, exp, got, errs)
            for k, v in errs.items():
                worst[k] = max(worst.get(k, 0.0), v)
            if report is not None:
                report(i, op, errs)
            if bad:
                fail(i, bad)
        lu = ad.close()
        if lu:
            fail(len(ops), f"{lu} LU fall-backs")
    finally:
        ad.close()
    return worst


def _replay(argv):
    import argparse

    ap = argparse.ArgumentParser(prog="seq_util.py replay")
    ap.add_argument("adapter", choices=ADAPTERS)
    ap.add_argument("seed", type=int)
    ap.add_argument("--upto", type=int, default=None)
    args = ap.parse_args(argv)
    cases = [c for c in committed(args.adapter) if c.seed == args.seed]
    if not cases:
        sys.exit(f"no committed {args.adapter} sequence with seed {args.seed}")
    case = cases[0]
    seq, seed, replaced = case.resolved()
    print(f"{case.id}: seed {seed}{' (replaced)' if replaced else ''} tau {seq.tau} dt {seq.dt:g} rho {seq.rho:g}")
    print("ops:", opstr(seq.ops))

    def report(i, op, errs):
        print(f"  {i:2d} {opstr([op]):28s} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()), flush=True)

    try:
        run_sequence(case, DeviceBackend(), upto=args.upto, report=report)
    except SequenceFailure as e:
        print("FAILED:", e)
        sys.exit(1)
    print("ok")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "replay":
        _replay(sys.argv[2:])
    else:
        sys.exit("usage: python tests/seq_util.py replay <adapter> <seed> [--upto k]")
