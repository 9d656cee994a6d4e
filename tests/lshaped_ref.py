"""The L-shaped method in numpy: a restatement of the algorithm of DESIGN.md 3.19 (after
mpisppy/opt/lshaped.py:477-666) over oracle.models scenarios, the reference of
tests/test_lshaped.py and tests/test_gpu_lshaped.py.  Written from reading those lines; it
holds none of their text.

All scenarios are two-stage minimisations.  The master is

    min sum_g eta_g   over x in R^nn, eta in R^G
    xlb <= x <= xub,  rl <= R x <= ru,  eta >= etalb,  eta_g - a.x >= b for every cut (g, a, b)

where eta_g models sum_{s in g} p_s f_s(x), f_s the whole objective of scenario s with its
nonants fixed at x.  Subproblems and master are solved by HiGHS (scipy.optimize.linprog,
highs-ds); the subgradient is the reduced cost of the fixed columns, read from the bound
marginals.
"""
import numpy as np
from scipy.optimize import linprog

_OPTS = {"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10}


def _bounds(lb, ub):
    return [(None if not np.isfinite(lo) else lo, None if not np.isfinite(hi) else hi) for lo, hi in zip(lb, ub)]


def lp_highs(A, rl, ru, lb, ub, c):
    """min c.x, rl <= A x <= ru, lb <= x <= ub.  Returns (x, obj, reduced costs) or raises."""
    A = np.asarray(A, float)
    eq = np.isfinite(rl) & np.isfinite(ru) & (rl == ru)
    up = (~eq) & np.isfinite(ru)
    lo = (~eq) & np.isfinite(rl)
    A_ub = np.vstack([A[up], -A[lo]])
    b_ub = np.concatenate([ru[up], -rl[lo]])
    res = linprog(c, A_ub=A_ub if len(b_ub) else None, b_ub=b_ub if len(b_ub) else None,
                  A_eq=A[eq] if eq.any() else None, b_eq=rl[eq] if eq.any() else None,
                  bounds=_bounds(lb, ub), method="highs-ds", options=_OPTS)
    if res.status != 0:
        raise RuntimeError(f"LP failed: status {res.status} ({res.message})")
    return res.x, float(res.fun), np.asarray(res.lower.marginals) + np.asarray(res.upper.marginals)


def group_of(s, G, S_total):
    """The cut group of the scenario with global index s."""
    return s * G // S_total


def default_groups(S_total):
    return S_total if S_total <= 32 else 32


def first_stage(arrs, idx):
    """The master's own constraints from the scenarios' arrays (A, rl, ru, lb, ub, c, q) and the
    nonant columns idx: rows of which every column is a nonant and whose coefficients and
    sides are bitwise equal in all scenarios, as dense (R [n_rows, nn], rl, ru); the nonant
    bounds, the tightest over the scenarios."""
    A0, rl0, ru0 = arrs[0][0], arrs[0][1], arrs[0][2]
    idx = np.asarray(idx)
    other = np.setdiff1d(np.arange(A0.shape[1]), idx)
    rows = []
    for i in range(A0.shape[0]):
        if not np.any(A0[i, idx]) or any(np.any(a[0][i, other]) for a in arrs):
            continue
        same = all(a[0][i].tobytes() == A0[i].tobytes() and a[1][i].tobytes() == rl0[i].tobytes()
                   and a[2][i].tobytes() == ru0[i].tobytes() for a in arrs)
        if same:
            rows.append(i)
    R = A0[rows][:, idx] if rows else np.zeros((0, len(idx)))
    xlb = np.max([a[3][idx] for a in arrs], axis=0)
    xub = np.min([a[4][idx] for a in arrs], axis=0)
    return R, rl0[rows], ru0[rows], xlb, xub


def solve_master(nn, G, cuts, R, rl, ru, xlb, xub, etalb):
    """The master by HiGHS.  cuts: list of (g, a, b).  Returns (x, eta, objective, status) with
    scipy's status (0 optimal, 2 infeasible)."""
    N = nn + G
    rows = [np.concatenate([R[i], np.zeros(G)]) for i in range(len(rl))]
    lo = list(rl)
    hi = list(ru)
    for g, a, b in cuts:
        h = np.zeros(N)
        h[:nn] = -np.asarray(a)
        h[nn + g] = 1.0
        rows.append(h)
        lo.append(b)
        hi.append(np.inf)
    A = np.array(rows) if rows else np.zeros((0, N))
    lo, hi = np.array(lo, float), np.array(hi, float)
    eq = np.isfinite(lo) & np.isfinite(hi) & (lo == hi)
    up = (~eq) & np.isfinite(hi)
    lw = (~eq) & np.isfinite(lo)
    A_ub = np.vstack([A[up], -A[lw]])
    b_ub = np.concatenate([hi[up], -lo[lw]])
    c = np.concatenate([np.zeros(nn), np.ones(G)])
    lb = np.concatenate([xlb, etalb])
    ub = np.concatenate([xub, np.full(G, np.inf)])
    res = linprog(c, A_ub=A_ub if len(b_ub) else None, b_ub=b_ub if len(b_ub) else None,
                  A_eq=A[eq] if eq.any() else None, b_eq=lo[eq] if eq.any() else None,
                  bounds=_bounds(lb, ub), method="highs-ds", options=_OPTS)
    if res.status != 0:
        return None, None, None, res.status
    return res.x[:nn], res.x[nn:], float(res.fun), 0


def master_violation(z, nn, G, cuts, R, rl, ru, xlb, xub, etalb):
    """The largest scaled violation of the master's constraints at z = (x, eta): each row's
    violation over max(1, |its side|)."""
    x, eta = z[:nn], z[nn:]
    v = 0.0
    for val, lo, hi in [(x, xlb, xub), (eta, etalb, np.full(G, np.inf))] + ([(R @ x, rl, ru)] if len(rl) else []):
        with np.errstate(invalid="ignore"):
            v = max(v, float(np.max(np.where(np.isfinite(lo), (lo - val) / np.maximum(1, np.abs(lo)), 0.0), initial=0.0)))
            v = max(v, float(np.max(np.where(np.isfinite(hi), (val - hi) / np.maximum(1, np.abs(hi)), 0.0), initial=0.0)))
    for g, a, b in cuts:
        v = max(v, (b - (eta[g] - np.dot(a, x))) / max(1.0, abs(b)))
    return v


class LShapedRef:
    """scens: oracle.models scenarios (two-stage, q = 0).  ``G``: cut groups (None: one per
    scenario up to 32, else 32).  After ``run()``: ``bounds`` (the outer bound of every
    master), ``cuts`` [(g, a, b)], ``masters`` (the cut count at every master solve), ``xhat``,
    ``Qsum`` (the expected cost at the last candidate), ``iters``."""

    def __init__(self, scens, G=None, tol=1e-8, max_iter=30, valid_eta_lb=None):
        self.scens = scens
        self.S = len(scens)
        self.arr = [s.arrays() for s in scens]
        self.idx = np.array(scens[0].nonant_indices())
        self.nn = len(self.idx)
        if len(scens[0].nodes) != 1:
            raise RuntimeError("two-stage problems only")
        for a in self.arr:
            assert not np.any(a[6]), "LPs only"
        self.prob = np.array([s.prob for s in scens], float)
        self.G = default_groups(self.S) if G is None else int(G)
        self.grp = np.array([group_of(s, self.G, self.S) for s in range(self.S)])
        self.tol, self.max_iter = float(tol), int(max_iter)
        self.R, self.rl, self.ru, self.xlb, self.xub = first_stage(self.arr, self.idx)
        self.valid_eta_lb = valid_eta_lb
        self.cuts, self.bounds, self.masters = [], [], []
        self.iters = 0

    def sub(self, s, x):
        """Scenario s with its nonants fixed at x (clipped to its bounds): (obj, d, x used)."""
        A, rl, ru, lb, ub, c, _ = self.arr[s]
        lb, ub = lb.copy(), ub.copy()
        xc = np.minimum(np.maximum(x, lb[self.idx]), ub[self.idx])
        lb[self.idx] = xc
        ub[self.idx] = xc
        _, obj, rc = lp_highs(A, rl, ru, lb, ub, c)
        return obj, rc[self.idx], xc

    def expected_cost(self, x):
        return float(sum(self.prob[s] * self.sub(s, x)[0] for s in range(self.S)))

    def group_cuts(self, x):
        """(a [G, nn], b [G], Q [G]) at the candidate x."""
        a = np.zeros((self.G, self.nn))
        b = np.zeros(self.G)
        Q = np.zeros(self.G)
        for s in range(self.S):
            obj, d, xc = self.sub(s, x)
            g, p = self.grp[s], self.prob[s]
            a[g] += p * d
            b[g] += p * (obj - d @ xc)
            Q[g] += p * obj
        return a, b, Q

    def wait_and_see(self):
        xs = np.zeros((self.S, self.nn))
        objs = np.zeros(self.S)
        for s in range(self.S):
            A, rl, ru, lb, ub, c, _ = self.arr[s]
            x, obj, _ = lp_highs(A, rl, ru, lb, ub, c)
            xs[s], objs[s] = x[self.idx], obj
        return xs, objs

    def run(self):
        xs, objs = self.wait_and_see()
        if self.valid_eta_lb is not None:
            lbs = np.array([self.valid_eta_lb[s] for s in range(self.S)], float)
        else:
            lbs = objs
        self.etalb = np.array([np.sum((self.prob * lbs)[self.grp == g]) for g in range(self.G)])
        self.trivial_bound = float(self.prob @ objs)
        x = self.prob @ xs / self.prob.sum()
        eta = self.etalb.copy()
        self.bounds.append(float(self.etalb.sum()))
        for it in range(1, self.max_iter + 1):
            self.iters = it
            a, b, Q = self.group_cuts(x)
            self.xhat, self.Qsum = x.copy(), float(Q.sum())
            added = 0
            for g in range(self.G):
                if Q[g] - eta[g] > self.tol * max(1.0, abs(Q[g])):
                    self.cuts.append((g, a[g].copy(), float(b[g])))
                    added += 1
            if added == 0:
                return True
            self.masters.append(len(self.cuts))
            x, eta, obj, st = solve_master(self.nn, self.G, self.cuts, self.R, self.rl, self.ru, self.xlb, self.xub,
                                           self.etalb)
            if st != 0:
                raise RuntimeError(f"master failed: status {st}")
            self.bounds.append(obj)
        return False


def ef_optimum(scens):
    """The extensive form by HiGHS: one copy of the nonants, every scenario's other columns.
    Returns (objective, x of the nonants)."""
    arr = [s.arrays() for s in scens]
    idx = np.array(scens[0].nonant_indices())
    nn = len(idx)
    n = arr[0][0].shape[1]
    other = np.setdiff1d(np.arange(n), idx)
    no = len(other)
    S = len(scens)
    ncol = nn + S * no
    rows, lo, hi = [], [], []
    c = np.zeros(ncol)
    lb = np.full(ncol, -np.inf)
    ub = np.full(ncol, np.inf)
    for s, (A, rl, ru, l, u, cc, _) in enumerate(arr):
        p = scens[s].prob
        blk = np.zeros((A.shape[0], ncol))
        blk[:, :nn] = A[:, idx]
        blk[:, nn + s * no: nn + (s + 1) * no] = A[:, other]
        rows.append(blk)
        lo.append(rl)
        hi.append(ru)
        c[:nn] += p * cc[idx]
        c[nn + s * no: nn + (s + 1) * no] = p * cc[other]
        lb[:nn] = np.maximum(lb[:nn], l[idx])
        ub[:nn] = np.minimum(ub[:nn], u[idx])
        lb[nn + s * no: nn + (s + 1) * no] = l[other]
        ub[nn + s * no: nn + (s + 1) * no] = u[other]
    x, obj, _ = lp_highs(np.vstack(rows), np.concatenate(lo), np.concatenate(hi), lb, ub, c)
    return obj, x[:nn]
