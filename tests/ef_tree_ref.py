"""The extensive form of a MULTISTAGE problem two ways (TEST INFRASTRUCTURE ONLY): by HiGHS on the
assembled extensive form, and by a numpy restatement of the tree interior point of DESIGN.md 3.23
(csrc/ph_ef_tree.inc) with a dense Ztot x Ztot Schur system.  Written from DESIGN.md 3.21 / 3.23; it
holds no text of the reference.

The problem is tests/ef_ref.py's with x_s[N_d] = z_{node_of[s, d]} for every depth d: one column
per (non-leaf node, offset), every scenario's other columns, costs p_s c_s.
"""
import numpy as np
import scipy.sparse as sp
from scipy.optimize import linprog

import ef_ref as E
from oracle.lpqp import solve_qp_highs


class Layout:
    """The non-leaf nodes of a ScenarioBatch as the engine numbers them: per node its depth, parent
    and first z index; per scenario the z index of each of its nn path nonants."""

    def __init__(self, b):
        self.D, self.nn, self.S = b.depth, b.nn, b.S
        self.nlens = np.asarray(b.nlens(), dtype=np.int64)
        self.P = np.concatenate([[0], np.cumsum(self.nlens)])
        Nn = len(b.node_names)
        self.depth, self.parent = np.zeros(Nn, dtype=np.int64), np.full(Nn, -1, dtype=np.int64)
        for d in range(self.D):
            self.depth[b.node_of[:, d]] = d
            if d:
                self.parent[b.node_of[:, d]] = b.node_of[:, d - 1]
        self.zoff = np.concatenate([[0], np.cumsum(self.nlens[self.depth])])
        self.Ztot = int(self.zoff[-1])
        self.node_of = np.asarray(b.node_of, dtype=np.int64)
        self.zidx = np.zeros((b.S, b.nn), dtype=np.int64)
        for k in range(b.nn):
            d = int(b.nonant_depth[k])
            self.zidx[:, k] = self.zoff[self.node_of[:, d]] + (k - self.P[d])
        self.Nn = Nn

    def path(self, n):
        """z indices of node n's path (ROOT's entries first)."""
        out = []
        while n >= 0:
            out = list(range(self.zoff[n], self.zoff[n + 1])) + out
            n = self.parent[n]
        return np.array(out, dtype=np.int64)

    def scenarios(self, n):
        return np.flatnonzero(self.node_of[:, self.depth[n]] == n)

    def children(self, n):
        return np.flatnonzero(self.parent == n)


def z_data(b, lay):
    """(zlb, zub, cz, qz) [Ztot]: per node the tightest bounds and the probability-weighted sums."""
    nc = np.asarray(b.nonant_col, dtype=np.int64)
    zlb, zub, cz, qz = np.full(lay.Ztot, -np.inf), np.full(lay.Ztot, np.inf), np.zeros(lay.Ztot), np.zeros(lay.Ztot)
    for k in range(b.nn):
        np.maximum.at(zlb, lay.zidx[:, k], b.lb[:, nc[k]])
        np.minimum.at(zub, lay.zidx[:, k], b.ub[:, nc[k]])
        np.add.at(cz, lay.zidx[:, k], b.prob * b.c[:, nc[k]])
        np.add.at(qz, lay.zidx[:, k], b.prob * b.q[:, nc[k]])
    return zlb, zub, cz, qz


# ------------------------------------------------------------------ HiGHS
def ef_tree_optimum(b, lay=None):
    """The multistage extensive form by HiGHS (LP: scipy's linprog(method="highs"); any q > 0:
    HiGHS's QP solver): (objective, z [Ztot]).  The matrix is the dense assembly column for column,
    kept in sparse storage."""
    lay = lay or Layout(b)
    A = np.array([b.dense_A(s) for s in range(b.S)])
    S, m, n = A.shape
    nc = np.asarray(b.nonant_col, dtype=np.int64)
    oth = np.setdiff1d(np.arange(n), nc)
    no, Z = len(oth), lay.Ztot
    N = Z + S * no
    M = sp.lil_matrix((S * m, N))
    zlb, zub, cz, qz = z_data(b, lay)
    cc, qq = np.zeros(N), np.zeros(N)
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    cc[:Z], qq[:Z], lo[:Z], hi[:Z] = cz, qz, zlb, zub
    for s in range(S):
        cols = slice(Z + s * no, Z + (s + 1) * no)
        M[s * m:(s + 1) * m, lay.zidx[s]] = A[s][:, nc]
        M[s * m:(s + 1) * m, cols] = A[s][:, oth]
        cc[cols], qq[cols] = b.prob[s] * b.c[s, oth], b.prob[s] * b.q[s, oth]
        lo[cols], hi[cols] = b.lb[s, oth], b.ub[s, oth]
    const = float(b.prob @ b.obj_const) if getattr(b, "obj_const", None) is not None else 0.0
    rl, ru = b.rl.ravel(), b.ru.ravel()
    if np.any(qq):
        x, obj, st = solve_qp_highs(M.toarray(), rl, ru, lo, hi, cc, qq)
        if st != 0:
            raise RuntimeError(f"HiGHS failed on the extensive form: status {st}")
        return obj + const, x[:Z]
    M = M.tocsr()
    fl, fu = np.isfinite(rl), np.isfinite(ru)
    eq = fl & fu & (rl == ru)
    Aub = sp.vstack([M[fu & ~eq], -M[fl & ~eq]])
    bub = np.concatenate([ru[fu & ~eq], -rl[fl & ~eq]])
    res = linprog(cc, A_ub=Aub if Aub.shape[0] else None, b_ub=bub if Aub.shape[0] else None,
                  A_eq=M[eq] if eq.any() else None, b_eq=rl[eq] if eq.any() else None,
                  bounds=list(zip(np.where(np.isfinite(lo), lo, None), np.where(np.isfinite(hi), hi, None))), method="highs")
    if res.status != 0:
        raise RuntimeError(f"HiGHS failed on the extensive form: {res.message}")
    return float(res.fun) + const, res.x[:Z]


# ------------------------------------------------------------------ the interior point, dense in z
class TreeEFRef(E.EFRef):
    """tests/ef_ref.py's EFRef with z the Ztot values of the tree: T_s scatters the scenario's
    nonant columns to its path's entries of z, so C is the dense Ztot x Ztot matrix whose block
    (n, a) is non-zero only where a is n or an ancestor of n.  Every update is EFRef's."""

    def __init__(self, b, tol=1e-8, max_iter=100):
        data = E.batch_data(b)
        super().__init__(data=data, tol=tol, max_iter=max_iter)
        self.lay = lay = Layout(b)
        A = data[0]
        T = np.zeros((self.S, self.m, lay.Ztot))
        for s in range(self.S):
            T[s][:, lay.zidx[s]] = A[s][:, self.idx]
        self.T = T
        zlb, zub, self.cz, self.qz = z_data(b, lay)
        self.z = E._Box(zlb, zub, 1.0 + np.abs(self.cz))
        self.ncomp = max(1, self.x.count() + self.w.count() + self.z.count())
        self.const = float(b.prob @ b.obj_const) if getattr(b, "obj_const", None) is not None else 0.0

    def _full(self):
        xf = np.zeros((self.S, self.n))
        xf[:, self.oth] = self.x.v
        xf[:, self.idx] = self.z.v[self.lay.zidx]
        return xf

    def objective(self):
        xf = self._full()
        return float(self.p @ np.sum(self.c_full * xf + 0.5 * self.q_full * xf * xf, axis=1))

    def solution(self):
        return self._full(), self.y / self.p[:, None]

    def node_systems(self):
        """The first predictor's per-node systems as the elimination forms them, bottom-up in numpy:
        {node: (A_n [P_d, P_d], b_n [P_d])} in path order, as summed from the node's scenarios or its
        children's Schur complements, before its own Dz^-1 and -r_z are added."""
        lay = self.lay
        Cs, rt = self.first_terms
        out, up = {}, {}
        for n in range(lay.Nn - 1, -1, -1):
            path = lay.path(n)
            Pd = len(path)
            if lay.depth[n] == lay.D - 1:
                ss = lay.scenarios(n)
                A = np.zeros((Pd, Pd))
                bb = np.zeros(Pd)
                for s in ss:                      # (index order, as the segmented sum adds)
                    A += Cs[s][np.ix_(path, path)]
                    bb += rt[s][path]
            else:
                A, bb = np.zeros((Pd, Pd)), np.zeros(Pd)
                for c in lay.children(n):
                    A += up[c][0]
                    bb += up[c][1]
            out[n] = (A.copy(), bb.copy())
            nl = int(lay.nlens[lay.depth[n]])
            own = path[Pd - nl:]
            A = A.copy()
            dd = np.diag(A)[Pd - nl:] + self.qz[own] + self.theta0[own]
            A[np.arange(Pd - nl, Pd), np.arange(Pd - nl, Pd)] = dd + self.REG * dd
            bb = bb.copy()
            bb[Pd - nl:] -= self.rz0[own]
            A11, A12, A22 = A[:Pd - nl, :Pd - nl], A[:Pd - nl, Pd - nl:], A[Pd - nl:, Pd - nl:]
            up[n] = (A11 - A12 @ np.linalg.solve(A22, A12.T), bb[:Pd - nl] - A12 @ np.linalg.solve(A22, bb[Pd - nl:]))
        return out


# ------------------------------------------------------------------ the certificate on a tree
def tree_kkt(b, x, y):
    """tests/ef_ref.py's ef_kkt with z per node: pres has the spread of each nonant column WITHIN a
    node, and the stationarity of a nonant is that of sum_s p_s r_s over the node's scenarios
    against z's bounds there.  Everything else, and both scalings, are ef_kkt's."""
    A, rl, ru, lb, ub, c, q, p, idx = E.batch_data(b)
    lay = Layout(b)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    oth = np.setdiff1d(np.arange(A.shape[2]), idx)
    ax = np.einsum("smj,sj->sm", A, x)

    def viol(v, lo, hi):
        with np.errstate(invalid="ignore"):
            a = np.where(np.isfinite(lo), (lo - v) / (1 + np.abs(lo)), 0.0)
            bb = np.where(np.isfinite(hi), (v - hi) / (1 + np.abs(hi)), 0.0)
        return float(max(a.max(initial=0.0), bb.max(initial=0.0), 0.0))

    def wrong(r, v, lo, hi):
        with np.errstate(invalid="ignore"):
            dl = np.where(np.isfinite(lo), np.minimum(1.0, np.abs(v - lo) / (1 + np.abs(v))), 1.0)
            du = np.where(np.isfinite(hi), np.minimum(1.0, np.abs(hi - v) / (1 + np.abs(v))), 1.0)
        return float(np.max(np.maximum(r, 0.0) * dl + np.maximum(-r, 0.0) * du, initial=0.0))

    zlb, zub, _, _ = z_data(b, lay)
    r = c + q * x - np.einsum("smj,sm->sj", A, y)
    rz, zhi, zlo = np.zeros(lay.Ztot), np.full(lay.Ztot, -np.inf), np.full(lay.Ztot, np.inf)
    for k in range(b.nn):
        np.add.at(rz, lay.zidx[:, k], p * r[:, idx[k]])
        np.maximum.at(zhi, lay.zidx[:, k], x[:, idx[k]])
        np.minimum.at(zlo, lay.zidx[:, k], x[:, idx[k]])
    pres = max(viol(ax, rl, ru), viol(x, lb, ub), float((zhi - zlo).max()))
    scale = 1.0 + float(np.abs(c).max())
    dres = max(wrong(r[:, oth], x[:, oth], lb[:, oth], ub[:, oth]), wrong(rz, zhi, zlb, zub), wrong(y, ax, rl, ru)) / scale
    return {"pres": pres, "dres": dres, "obj": float(p @ np.sum(c * x + 0.5 * q * x * x, axis=1))}


# ------------------------------------------------------------------ the shapes the tests share
SOLVER = "mi355x_pdhg"


def aircond_opt(cls, bfs, quad=0.0, names=None, **options):
    """``cls`` (ExtensiveForm, SchurComplement) on aircond over the tree ``bfs``, start_seed 0."""
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    bfs = list(bfs)
    o = {"solver": SOLVER, "toc": False}
    o.update(options)
    kw = {"branching_factors": bfs, "start_seed": 0}
    if quad:
        kw["QuadShortCoeff"] = quad
    return cls(o, names or aircond.scenario_names_creator(int(np.prod(bfs))), aircond.scenario_creator,
               all_nodenames=create_nodenames_from_branching_factors(bfs), scenario_creator_kwargs=kw)


_CASES = {}


def case(bfs, quad=0.0):
    """(batch, the restatement after its run, whether it converged, HiGHS's (objective, z)): once."""
    from mpisppy_amd.opt.ef import ExtensiveForm
    key = (tuple(bfs), quad)
    if key not in _CASES:
        b = aircond_opt(ExtensiveForm, bfs, quad).batch
        ref = TreeEFRef(b)
        ok = ref.run()
        _CASES[key] = (b, ref, ok, ef_tree_optimum(b, ref.lay))
    return _CASES[key]


def synthetic_batch(seed=3):
    """A ScenarioBatch with nlens = [3, 1, 2] over a 2,3,2 tree (12 scenarios, 9 non-leaf nodes, Ztot
    17): six nonant columns and three others, five rows that each touch another column; every column
    boxed and every row ranged (one of them an equality, one one-sided) around a known feasible
    point, so the problem is feasible and bounded by construction."""
    from mpisppy_amd.batch import ScenarioBatch
    rng = np.random.default_rng(seed)
    bfs, nlens = [2, 3, 2], [3, 1, 2]
    S, D, nn, n, m = 12, 3, 6, 9, 5
    names = [f"scen{i}" for i in range(S)]
    node_names = ["ROOT"] + [f"ROOT_{i}" for i in range(2)] + [f"ROOT_{i}_{j}" for i in range(2) for j in range(3)]
    node_of = np.array([[0, 1 + s // 6, 3 + s // 2] for s in range(S)], dtype=np.int32)
    nonant_col = [0, 1, 2, 3, 4, 5]
    nonant_depth, nonant_off = [0, 0, 0, 1, 2, 2], [0, 1, 2, 0, 0, 1]
    mask = rng.random((m, n)) < 0.6
    mask[:, 6 + np.arange(m) % 3] = True                       # every row touches a column that is no nonant
    mask[np.arange(nn) % m, np.arange(nn)] = True              # every nonant column is in a row
    rows, cols = np.nonzero(mask)
    row_ptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    A = rng.uniform(0.5, 2.0, (S, len(cols))) * rng.choice([-1.0, 1.0], len(cols))
    zoff = np.concatenate([[0], np.cumsum(np.array(nlens)[[0, 1, 1, 2, 2, 2, 2, 2, 2]])])
    z0 = rng.uniform(-3.0, 3.0, zoff[-1])
    zlo, zhi = z0 - rng.uniform(0.5, 2.0, len(z0)), z0 + rng.uniform(0.5, 2.0, len(z0))
    x0, lb, ub = rng.uniform(-3.0, 3.0, (S, n)), np.zeros((S, n)), np.zeros((S, n))
    for k in range(nn):
        zi = zoff[node_of[:, nonant_depth[k]]] + nonant_off[k]
        x0[:, k], lb[:, k], ub[:, k] = z0[zi], zlo[zi], zhi[zi]
    lb[:, nn:], ub[:, nn:] = x0[:, nn:] - rng.uniform(0.5, 2.0, (S, n - nn)), x0[:, nn:] + rng.uniform(0.5, 2.0, (S, n - nn))
    act = np.zeros((S, m))
    np.add.at(act, (slice(None), rows), A * x0[:, cols])
    rl, ru = act - rng.uniform(0.5, 1.0, (S, m)), act + rng.uniform(0.5, 1.0, (S, m))
    rl[:, 1] = ru[:, 1] = act[:, 1]                            # an equality
    ru[:, 2] = np.inf                                          # one-sided
    c = rng.uniform(-2.0, 2.0, (S, n))
    prob = rng.uniform(0.5, 1.5, S)
    prob /= prob.sum()
    pc = np.ones((S, D))
    return ScenarioBatch(names, row_ptr, cols.astype(np.int32), A, c, lb, ub, rl, ru, np.zeros((S, n)), np.zeros(S), nonant_col,
                         nonant_depth, nonant_off, node_of, node_names, prob, pc, 1, [f"x[{j}]" for j in range(n)],
                         [f"x[{j}]" for j in range(nn)])


def synthetic_opt(**options):
    """ExtensiveForm on ``synthetic_batch`` (through a batch_creator: no per-scenario models)."""
    from mpisppy_amd.opt.ef import ExtensiveForm
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    o = {"solver": SOLVER, "toc": False, "batch_creator": lambda names, **kw: synthetic_batch()}
    o.update(options)
    return ExtensiveForm(o, [f"scen{i}" for i in range(12)], None,
                         all_nodenames=create_nodenames_from_branching_factors([2, 3, 2]))


def synthetic_case():
    """(ExtensiveForm, batch, the restatement after its run, whether it converged, HiGHS's answer): once."""
    if "synthetic" not in _CASES:
        ef = synthetic_opt()
        ref = TreeEFRef(ef.batch)
        ok = ref.run()
        _CASES["synthetic"] = (ef, ef.batch, ref, ok, ef_tree_optimum(ef.batch, ref.lay))
    return _CASES["synthetic"]
