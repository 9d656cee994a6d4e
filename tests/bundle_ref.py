"""PH with bundles on the CPU (TEST INFRASTRUCTURE ONLY).

A bundle is the extensive form of a contiguous slice of a rank's scenarios with the probabilities
p_s / p_B (reference spbase.py:219-253, spopt.py:805-836).  ``BundlePH`` is ``oracle.ph.OraclePH``
with ``solve_loop`` solving each bundle instead of each scenario, two ways:

  * ``mode="exact"``: the explicit bundle LP / QP (one copy of the nonants, every scenario's other
    columns) through ``oracle.lpqp``;
  * ``mode="efref"``: ``ef_ref.EFRef``, the numpy restatement of the device's interior point, on the
    bundle's scenarios with ``c[N] += W - rho xbar`` and ``q[N] += rho``.

Every scenario of a bundle gets the bundle's nonants and the bundle's objective, so x̄, W, conv,
Ebound and Eobjective of OraclePH work unchanged (sum_s p_s obj_B over a bundle is p_B obj_B).
"""
import numpy as np

from oracle.lpqp import solve_lp_highs, solve_qp_ipm
from oracle.ph import OraclePH, rank_slices

import ef_ref


def bundle_slices(rank_slice, bundles_per_rank):
    """The reference's slicing of one rank's scenarios (spbase.py:236-246)."""
    n = len(rank_slice)
    if n < bundles_per_rank:
        raise RuntimeError("Not enough scenarios to satisfy the bundles_per_rank requirement")
    avg = n / bundles_per_rank
    return [[rank_slice[j] for j in range(int(i * avg), int((i + 1) * avg))] for i in range(bundles_per_rank)]


def names_in_bundles(names, n_proc, bundles_per_rank):
    """{rank: {bundle: [scenario names]}} as SPBase._assign_bundles builds it."""
    return {r: {b: [names[k] for k in sl] for b, sl in enumerate(bundle_slices(rs, bundles_per_rank))}
            for r, rs in enumerate(rank_slices(len(names), n_proc))}


def explicit_bundle(A, rl, ru, lb, ub, c, q, p, idx):
    """The bundle as one problem: (M, rl, ru, lo, hi, cc, qq) over [z | x_1 others | x_2 others ...]."""
    S, m, n = A.shape
    nn = len(idx)
    oth = np.setdiff1d(np.arange(n), idx)
    no = len(oth)
    N = nn + S * no
    M = np.zeros((S * m, N))
    cc, qq = np.zeros(N), np.zeros(N)
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    for s in range(S):
        cols = slice(nn + s * no, nn + (s + 1) * no)
        M[s * m:(s + 1) * m, :nn] = A[s][:, idx]
        M[s * m:(s + 1) * m, cols] = A[s][:, oth]
        cc[:nn] += p[s] * c[s, idx]
        qq[:nn] += p[s] * q[s, idx]
        cc[cols], qq[cols] = p[s] * c[s, oth], p[s] * q[s, oth]
        lo[:nn], hi[:nn] = np.maximum(lo[:nn], lb[s, idx]), np.minimum(hi[:nn], ub[s, idx])
        lo[cols], hi[cols] = lb[s, oth], ub[s, oth]
    return M, rl.ravel(), ru.ravel(), lo, hi, cc, qq


class BundlePH(OraclePH):
    def __init__(self, scens, default_rho, bundles_per_rank, n_proc=1, mode="exact", tol=1e-10, max_iter=100):
        super().__init__(scens, default_rho, n_proc=n_proc)
        self.bundles = [b for sl in self.slices for b in bundle_slices(sl, bundles_per_rank)]
        self.mode, self.tol, self.max_iter = mode, tol, max_iter
        self.data = ef_ref.stack(scens)
        self.ipm_iters = []          # per solve_loop: the bundles' interior-point iterations (efref)
        self.failures = 0            # bundles that did not pass the test (efref)
        self.refs = []               # the last solve_loop's EFRef objects (efref)

    def bundle_data(self, b):
        """``ef_ref.stack``'s tuple of bundle ``b`` with the PH terms of the current state; and the
        prox term's constant."""
        A, rl, ru, lb, ub, c, q, p, idx = self.data
        ks = np.asarray(self.bundles[b])
        c, q = c[ks].copy(), q[ks].copy()
        pc = p[ks] / p[ks].sum()
        const = 0.0
        if self.W_on:
            c[:, idx] += self.W[ks]
        if self.prox_on:
            c[:, idx] -= self.rho[ks] * self.xbar[ks]
            q[:, idx] += self.rho[ks]
            const = float(pc @ (0.5 * self.rho[ks] * self.xbar[ks] ** 2).sum(axis=1))
        return (A[ks], rl[ks], ru[ks], lb[ks], ub[ks], c, q, pc, idx), const

    def solve_bundle_exact(self, b):
        data, const = self.bundle_data(b)
        M, rl, ru, lo, hi, cc, qq = explicit_bundle(*data)
        if np.any(qq):
            x, obj, st = solve_qp_ipm(M, rl, ru, lo, hi, cc, qq)
        else:
            x, obj, st = solve_lp_highs(M, rl, ru, lo, hi, cc)
        if st != 0:
            raise RuntimeError(f"oracle solve failed for bundle {b}: status {st}")
        return x[:self.nn], obj + const

    def solve_bundle_efref(self, b):
        data, const = self.bundle_data(b)
        ref = ef_ref.EFRef(data=data, tol=self.tol, max_iter=self.max_iter)
        ok = ref.run()
        self.failures += 0 if ok else 1
        self.refs.append(ref)
        return ref.z.v.copy(), ref.obj + const, ref.it

    def solve_loop(self):
        its = []
        self.refs = []
        for b, ks in enumerate(self.bundles):
            if self.mode == "exact":
                z, obj = self.solve_bundle_exact(b)
            else:
                z, obj, it = self.solve_bundle_efref(b)
                its.append(it)
            self.x[ks] = z
            self.obj[ks] = obj
            self.outer[ks] = obj
        if its:
            self.ipm_iters.append(its)


_RUNS = {}


def farmer_run(S, cm, bundles_per_rank, iters, mode="exact", n_proc=1, rho=1.0, tol=1e-10):
    """A BundlePH run on farmer (Iter0, then ``iters`` PH iterations), computed once and shared;
    the caller must not change it."""
    from oracle.models import farmer_scenario
    key = (S, cm, bundles_per_rank, iters, mode, n_proc, rho, tol)
    if key not in _RUNS:
        sc = [farmer_scenario(f"scen{i}", cm, num_scens=S) for i in range(S)]
        ph = BundlePH(sc, rho, bundles_per_rank, n_proc=n_proc, mode=mode, tol=tol)
        ph.iter0()
        ph.iterk_loop(iters, -1.0)
        _RUNS[key] = ph
    return _RUNS[key]
