"""Numpy restatement of the Fixer for the tests (TEST INFRASTRUCTURE ONLY):
mpisppy/extensions/fixer.py:114-128 (_update_fix_counts), 131-223 (iter0), 226-304 (iterk),
with the two departures of mpisppy_amd/extensions/fixer.py (lags per nonant; the variation
test per node entry).

``rule`` is the decision for arrays of entries.  ``FixerOraclePH`` is oracle.ph.OraclePH with
the rule between convergence_diff and solve_loop (the place of miditer, phbase.py:919-926)
and with the fixed columns eliminated from every solve, as oracle/wheel.py::xhat_objective
does (the dense IPM needs lb < ub); a subproblem none of whose free columns has a quadratic
term goes to the HiGHS LP (the IPM fails on fully fixed farmer subproblems at 70 scenarios).
"""
import functools

import numpy as np

from oracle.lpqp import solve_lp_highs, solve_qp_ipm
from oracle.ph import OraclePH


def rule(iter0, xb, xsq, th, nb, lb, ub, l, u, boundtol, count, fixval):
    """One miditer for arrays of entries (any common shape; th / nb / lb / ub broadcast;
    lags < 0 are None).  Returns (count, fixval, newly fixed mask, arrived mask): new arrays.
    An entry whose fixval is not NaN, or with l == u, is skipped and its counter kept."""
    xb, xsq, l, u = (np.asarray(a, dtype=np.float64) for a in (xb, xsq, l, u))
    shape = np.broadcast(xb, l, count).shape
    th, nb, lb, ub = (np.broadcast_to(np.asarray(a), shape) for a in (th, nb, lb, ub))
    xb, xsq, l, u = (np.broadcast_to(a, shape) for a in (xb, xsq, l, u))
    count = np.array(np.broadcast_to(count, shape), dtype=np.int64)
    fixval = np.array(np.broadcast_to(fixval, shape), dtype=np.float64)
    skip = ~np.isnan(fixval) | (l == u)
    diff = xb * xb - xsq
    t2 = th.astype(np.float64) * th.astype(np.float64)
    with np.errstate(invalid="ignore"):
        near_l = xb - l < boundtol
        near_u = u - xb < boundtol
        if iter0:
            conv = ~((-diff > t2) | (diff > t2))                        # fixer.py:169
            b_nb = conv & (nb >= 0)                                     # :175
            b_lb = conv & ~b_nb & (lb >= 0) & near_l                    # :180
            b_ub = conv & ~b_nb & ~b_lb & (ub >= 0) & near_u            # :185
        else:
            hit = (-diff < t2) & (diff < t2)                            # fixer.py:124
            count = np.where(skip, count, np.where(hit, count + 1, 0))
            pos = count > 0                                             # :260
            b_nb = pos & (nb >= 0) & (nb <= count)                      # :263
            b_lb = pos & ~b_nb & (lb >= 0) & (lb < count) & near_l      # :268
            b_ub = pos & ~b_nb & ~b_lb & (ub >= 0) & (ub < count) & near_u   # :274
    val = np.where(b_nb, xb, np.where(b_lb, l, u))
    new = (b_nb | b_lb | b_ub) & ~skip
    fixval = np.where(new, np.minimum(np.maximum(val, l), u), fixval)
    arrived = skip if iter0 else np.zeros(shape, dtype=bool)
    return count, fixval, new, arrived


def margins(xb, xsq, th, free):
    """| |diff| - th² | / th² of the free entries with a threshold: how far each counter
    decision is from flipping."""
    diff = np.abs(xb * xb - xsq)
    t2 = np.broadcast_to(np.asarray(th, dtype=np.float64) ** 2, diff.shape)
    ok = free & (t2 > 0)
    return np.abs(diff[ok] - t2[ok]) / t2[ok]


def oracle_keys(o):
    """key[s, j] = node index * nlen_max + offset, node names (first seen), nlen_max."""
    names, S = [], len(o.scens)
    for sl in o.node_slices:
        for (ndn, a, b) in sl:
            if ndn not in names:
                names.append(ndn)
    nl = max(b - a for sl in o.node_slices for (_, a, b) in sl)
    key = np.zeros((S, o.nn), dtype=np.int64)
    for s, sl in enumerate(o.node_slices):
        for (ndn, a, b) in sl:
            key[s, a:b] = names.index(ndn) * nl + np.arange(b - a)
    return key, names, nl


class FixerOraclePH(OraclePH):
    """OraclePH stepped with the Fixer.  ``iter0`` / ``iterk``: (th, nb, lb, ub) per nonant
    ([nn] arrays, lags < 0 = None) or None (no tuples: nothing is done)."""

    def __init__(self, scens, default_rho, iter0, iterk, boundtol, **kw):
        super().__init__(scens, default_rho, **kw)
        self.fix_iter0, self.fix_iterk, self.boundtol = iter0, iterk, float(boundtol)
        S = len(scens)
        self.count = np.zeros((S, self.nn), dtype=np.int64)
        self.fixval = np.full((S, self.nn), np.nan)
        self.key, self.node_names, self.nlen_max = oracle_keys(self)
        self.nkeys = len(self.node_names) * self.nlen_max
        self.l = np.array([np.asarray(a[3])[idx] for a, idx in zip(self.arr, self.nonant_idx)])
        self.u = np.array([np.asarray(a[4])[idx] for a, idx in zip(self.arr, self.nonant_idx)])
        self.totals = np.zeros(3, dtype=np.int64)
        self.log = []

    # -- the solve with the fixed columns eliminated (oracle/wheel.py::xhat_objective)
    def _solve_one(self, k):
        fv = self.fixval[k]
        if np.isnan(fv).all():
            return super()._solve_one(k)
        A, rl, ru, lb, ub, c, q = self.arr[k]
        idx = np.asarray(self.nonant_idx[k])
        c, q = c.copy(), q.copy()
        const = 0.0
        if self.W_on:
            c[idx] += self.W[k]
        if self.prox_on:
            c[idx] -= self.rho[k] * self.xbar[k]
            q[idx] += self.rho[k]
            const = 0.5 * float(np.sum(self.rho[k] * self.xbar[k] ** 2))
        xf = np.full(len(c), np.nan)
        xf[idx] = fv
        fx = ~np.isnan(xf)
        fr = ~fx
        shift = A[:, fx] @ xf[fx]
        const += float(c[fx] @ xf[fx] + 0.5 * np.sum(q[fx] * xf[fx] ** 2))
        rl, ru = rl - shift, ru - shift
        live = np.any(A[:, fr] != 0.0, axis=1)
        tol = 1e-9 * (1.0 + np.abs(shift[~live]))
        if np.any(rl[~live] > tol) or np.any(ru[~live] < -tol):
            raise RuntimeError(f"oracle: fixed values infeasible for {self.scens[k].name}")
        if not np.any(q[fr]):
            x, obj, st = solve_lp_highs(A[live][:, fr], rl[live], ru[live], lb[fr], ub[fr], c[fr])
        else:
            x, obj, st = solve_qp_ipm(A[live][:, fr], rl[live], ru[live], lb[fr], ub[fr], c[fr], q[fr])
        if st != 0:
            raise RuntimeError(f"oracle solve failed for {self.scens[k].name}: status {st}")
        full = xf.copy()
        full[fr] = x
        self.x[k] = full[idx]
        self.obj[k] = obj + const
        self.outer[k] = obj + const

    # -- node x̄ / E[x²] as [S, nn] (every scenario reads its node's entry)
    def _xb_xsq(self):
        xb = np.zeros((len(self.scens), self.nn))
        xsq = np.zeros_like(xb)
        for s, sl in enumerate(self.node_slices):
            for (ndn, a, b) in sl:
                xb[s, a:b] = self.node_xbar[ndn]
                xsq[s, a:b] = self.node_xsqbar[ndn]
        return xb, xsq

    def miditer(self, ph_iter):
        iter0 = ph_iter == 1
        t = self.fix_iter0 if iter0 else self.fix_iterk
        if t is None:
            return None
        th, nb, lb, ub = t
        xb, xsq = self._xb_xsq()
        free = np.isnan(self.fixval) & (self.l != self.u)
        mg = margins(xb, xsq, th, free)
        self.count, self.fixval, new, arrived = rule(iter0, xb, xsq, th, nb, lb, ub, self.l, self.u,
                                                     self.boundtol, self.count, self.fixval)
        nfix = np.bincount(self.key[new], minlength=self.nkeys)
        nloc = np.bincount(self.key.ravel(), minlength=self.nkeys)
        self.totals += [int(new.sum()), int(arrived.sum()), int(((nfix > 0) & (nfix < nloc)).sum())]
        rec = {"iter": ph_iter, "nfix": nfix, "new": new, "margin": float(mg.min()) if mg.size else np.inf}
        self.log.append(rec)
        return rec

    def run(self, iters):
        """``iters`` PH iterations in the loop order of phbase.py:909-957; per iteration
        {conv, xbar, W} in ``hist``."""
        self.hist = []
        for it in range(1, iters + 1):
            self.compute_xbar()
            self.update_W()
            conv = self.convergence_diff()
            self.miditer(it)
            self.hist.append({"iter": it, "conv": conv, "xbar": self.xbar.copy(), "W": self.W.copy()})
            self.solve_loop()
        return self.hist

    def node_xbar_flat(self):
        out = np.zeros(self.nkeys)
        out[self.key] = self.xbar
        return out


AIR_KW = {"start_seed": 1134}      # aircond with the model's own default parameters (aircond.py:19-35)

# the three trajectories: th, nb (iterk tuples of every nonant; the iter0 tuples carry the
# threshold and no lag), PH iterations, and the fixing observed with the reference's rule:
# {PH iteration: entries newly fixed}
CASES = {
    "farmer3": {"th": 10.0, "nb": 3, "iters": 12, "S": 3, "fixed": {5: 3, 11: 6}},
    "farmer70": {"th": 10.0, "nb": 3, "iters": 10, "S": 70, "fixed": {6: 70, 7: 70, 8: 70}},
    "aircond32": {"th": 5.0, "nb": 2, "iters": 6, "S": 6, "bf": [3, 2], "fixed": {3: 22, 4: 2}},
}
BOUNDTOL = 1e-2


def tuples(case, nn):
    """(iter0, iterk) per-nonant arrays of a case."""
    c = CASES[case]
    none = np.full(nn, -1, dtype=np.int32)
    th = np.full(nn, c["th"])
    return (th, none, none, none), (th, np.full(nn, c["nb"], dtype=np.int32), none, none)


def scenarios(case):
    c = CASES[case]
    names = [f"scen{i}" for i in range(c["S"])]
    if case.startswith("farmer"):
        from oracle.models import farmer_scenario
        return [farmer_scenario(n, 1, num_scens=c["S"]) for n in names]
    from oracle.models import aircond_scenario
    return [aircond_scenario(n, c["bf"], **AIR_KW) for n in names]


@functools.lru_cache(maxsize=None)
def trajectory(case):
    """The case's stepped oracle after its iterations, computed once per session and shared
    (read-only) by the tests."""
    scens = scenarios(case)
    nn = len(scens[0].nonant_indices())
    i0, ik = tuples(case, nn)
    o = FixerOraclePH(scens, 1.0, i0, ik, BOUNDTOL, solver="ipm")
    o.trivial = o.iter0()
    o.run(CASES[case]["iters"])
    return o
