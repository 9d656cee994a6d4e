"""The CONDITIONED multistage extensive form two ways (TEST INFRASTRUCTURE ONLY):
z entries held at values.  tests/ef_tree_ref.py extended, not edited: HiGHS on the assembled
extensive form with lb = ub = value on the held columns, and the numpy restatement of the tree
interior point with the held entries taken out of z.

The restatement solves the same problem in the free entries only: a held entry has dz = 0, no duals,
no complementarity and no part in the test (phgpu_eft_fix), which is the interior point on the
problem whose rows have T_held v moved into their activities.  So ``CondTreeEFRef`` is TreeEFRef
with z cut down to the free entries and the row activities w shifted by T_held v: the primal
residual, its scaling by the rows' own sides, every other residual and the step lengths are then
those of the device's iteration.  (The start of a ONE-sided row's activity is not invariant under
that shift -- lo + max(1, 0.1 |lo|) -- so on such rows the iterates are close, not equal; aircond has
none.)
"""
import numpy as np
import scipy.sparse as sp
from scipy.optimize import linprog

import ef_ref as E
import ef_tree_ref as R
from oracle.lpqp import solve_qp_highs


# ------------------------------------------------------------------ HiGHS
def cond_optimum(b, zfix, lay=None, scen=None):
    """HiGHS on the extensive form over the scenarios ``scen`` (default: all; their probabilities
    divided by their sum, so a subtree's own objective) with lb = ub = zfix on the held z columns:
    (ok, objective, z [Ztot]).  ok: HiGHS found it feasible and bounded.  z columns off the
    scenarios' paths are shut at 0."""
    lay = lay or R.Layout(b)
    ss = np.arange(b.S) if scen is None else np.asarray(scen, dtype=np.int64)
    zfix = np.asarray(zfix, dtype=np.float64)
    p = b.prob[ss] / b.prob[ss].sum()
    nc = np.asarray(b.nonant_col, dtype=np.int64)
    oth = np.setdiff1d(np.arange(b.n), nc)
    no, Z, m, S = len(oth), lay.Ztot, b.m, len(ss)
    N = Z + S * no
    M = sp.lil_matrix((S * m, N))
    cc, qq = np.zeros(N), np.zeros(N)
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    lo[:Z], hi[:Z] = 0.0, 0.0
    zlb, zub, _, _ = R.z_data(b, lay)
    for i, s in enumerate(ss):
        A = b.dense_A(s)
        zi = lay.zidx[s]
        cols = slice(Z + i * no, Z + (i + 1) * no)
        M[i * m:(i + 1) * m, zi] = A[:, nc]
        M[i * m:(i + 1) * m, cols] = A[:, oth]
        np.add.at(cc, zi, p[i] * b.c[s, nc])
        np.add.at(qq, zi, p[i] * b.q[s, nc])
        lo[zi], hi[zi] = zlb[zi], zub[zi]
        cc[cols], qq[cols] = p[i] * b.c[s, oth], p[i] * b.q[s, oth]
        lo[cols], hi[cols] = b.lb[s, oth], b.ub[s, oth]
    on = np.zeros(Z, dtype=bool)
    on[np.unique(lay.zidx[ss])] = True
    held = ~np.isnan(zfix) & on
    if np.any(zfix[held] < lo[:Z][held]) or np.any(zfix[held] > hi[:Z][held]):
        return False, np.nan, None
    lo[:Z][held] = hi[:Z][held] = zfix[held]
    const = float(p @ b.obj_const[ss]) if getattr(b, "obj_const", None) is not None else 0.0
    rl, ru = b.rl[ss].ravel(), b.ru[ss].ravel()
    if np.any(qq):
        x, obj, st = solve_qp_highs(M.toarray(), rl, ru, lo, hi, cc, qq)
        return st == 0, obj + const, (x[:Z] if st == 0 else None)
    M = M.tocsr()
    fl, fu = np.isfinite(rl), np.isfinite(ru)
    eq = fl & fu & (rl == ru)
    Aub = sp.vstack([M[fu & ~eq], -M[fl & ~eq]])
    bub = np.concatenate([ru[fu & ~eq], -rl[fl & ~eq]])
    res = linprog(cc, A_ub=Aub if Aub.shape[0] else None, b_ub=bub if Aub.shape[0] else None,
                  A_eq=M[eq] if eq.any() else None, b_eq=rl[eq] if eq.any() else None,
                  bounds=list(zip(np.where(np.isfinite(lo), lo, None), np.where(np.isfinite(hi), hi, None))), method="highs")
    if res.status != 0:
        return False, np.nan, None
    return True, float(res.fun) + const, res.x[:Z]


# ------------------------------------------------------------------ the interior point with held entries
class CondTreeEFRef(R.TreeEFRef):
    """TreeEFRef on the free entries of z (module docstring).  ``zfix`` [Ztot]: NaN = free.  With
    every entry held, z keeps one inert entry (no column, no bounds, diagonal 1) so that the dense
    Schur system is never empty; it stays 0."""

    def __init__(self, b, zfix, tol=1e-8, max_iter=100):
        super().__init__(b, tol=tol, max_iter=max_iter)
        self.zfix = zfix = np.asarray(zfix, dtype=np.float64)
        self.held = held = ~np.isnan(zfix)
        free = ~held
        zb = self.z
        assert np.all(zfix[held] >= zb.lo[held]) and np.all(zfix[held] <= zb.hi[held])
        off = self.T[:, :, held] @ zfix[held]
        w = E._Box(self.w.lo - off, self.w.hi - off, self.p[:, None] * np.ones_like(off))
        w.v = np.where(self.eq, self.rl - off, w.v)
        self.w = w
        self.y = w.zl - w.zu
        if free.any():
            self.T = self.T[:, :, free]
            self.cz, self.qz = self.cz[free], self.qz[free]
            self.z = E._Box(zb.lo[free], zb.hi[free], 1.0 + np.abs(self.cz))
        else:
            self.T = np.zeros((self.S, self.m, 1))
            self.cz, self.qz = np.zeros(1), np.ones(1)
            self.z = E._Box(np.array([-np.inf]), np.array([np.inf]), np.ones(1))
        self.ncomp = max(1, self.x.count() + self.w.count() + self.z.count())

    def z_full(self):
        z = self.zfix.copy()
        if (~self.held).any():
            z[~self.held] = self.z.v
        return z

    def _full(self):
        xf = np.zeros((self.S, self.n))
        xf[:, self.oth] = self.x.v
        xf[:, self.idx] = self.z_full()[self.lay.zidx]
        return xf

    def node_systems(self):
        raise NotImplementedError("the per-node systems are checked on given matrices (test_ef_cond.py)")


# ------------------------------------------------------------------ the certificate on the free entries
def cond_kkt(b, x, y, zfix):
    """tests/ef_tree_ref.py's tree_kkt with the held entries' stationarity left out: a held z has a
    multiplier of either sign (that of lb = ub = value).  Everything else is tree_kkt's."""
    lay = R.Layout(b)
    zfix = np.asarray(zfix, dtype=np.float64)
    held = ~np.isnan(zfix)
    A, rl, ru, lb, ub, c, q, p, idx = E.batch_data(b)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    k = R.tree_kkt(b, x, y)
    if not held.any():
        return k
    # dres again, with the held entries' reduced costs zeroed: tree_kkt's formulas on z
    oth = np.setdiff1d(np.arange(A.shape[2]), idx)
    ax = np.einsum("smj,sj->sm", A, x)

    def wrong(r, v, lo, hi):
        with np.errstate(invalid="ignore"):
            dl = np.where(np.isfinite(lo), np.minimum(1.0, np.abs(v - lo) / (1 + np.abs(v))), 1.0)
            du = np.where(np.isfinite(hi), np.minimum(1.0, np.abs(hi - v) / (1 + np.abs(v))), 1.0)
        return float(np.max(np.maximum(r, 0.0) * dl + np.maximum(-r, 0.0) * du, initial=0.0))

    zlb, zub, _, _ = R.z_data(b, lay)
    r = c + q * x - np.einsum("smj,sm->sj", A, y)
    rz, zv = np.zeros(lay.Ztot), np.zeros(lay.Ztot)
    for kk in range(b.nn):
        np.add.at(rz, lay.zidx[:, kk], p * r[:, idx[kk]])
        zv[lay.zidx[:, kk]] = x[:, idx[kk]]
    rz[held] = 0.0
    scale = 1.0 + float(np.abs(c).max())
    k["dres"] = max(wrong(r[:, oth], x[:, oth], lb[:, oth], ub[:, oth]), wrong(rz, zv, zlb, zub), wrong(y, ax, rl, ru)) / scale
    return k


# ------------------------------------------------------------------ fixings and the shared cases
def zfix_of(lay, names, cache):
    """{node name: values (NaN = free)} -> zfix [Ztot]."""
    z = np.full(lay.Ztot, np.nan)
    names = list(names)
    for nd, v in cache.items():
        n = names.index(nd)
        z[lay.zoff[n]:lay.zoff[n + 1]] = v
    return z


_CASES = {}


def cond_case(key, b, zfix):
    """{"ok", "obj", "z", "ref", "zfix", "lay"} of batch ``b`` with ``zfix`` held, once per ``key``.
    ok: HiGHS found the conditioned problem feasible and bounded AND the restatement converged."""
    if key not in _CASES:
        lay = R.Layout(b)
        ok, obj, z = cond_optimum(b, zfix, lay)
        ref, conv = None, False
        if ok:
            ref = CondTreeEFRef(b, zfix)
            conv = ref.run()
        _CASES[key] = {"ok": bool(ok and conv), "obj": obj, "z": z, "ref": ref, "zfix": np.asarray(zfix, dtype=np.float64), "lay": lay}
    return _CASES[key]
