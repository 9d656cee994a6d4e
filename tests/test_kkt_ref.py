"""The KKT certificate of tests/kkt_ref.py can fail (CPU): exact solutions with their own
multipliers pass at 1e-9, and a sign flip, a 0.1 % scaling or a one-row shift of the row duals
is rejected at the 1e-5 the GPU tests hold the kernels to (test_gpu_kkt.py).

LP solutions and marginals come from scipy's HiGHS, with the row split of
oracle/lpqp.solve_lp_highs; QP solutions from the oracle's solve_qp_ipm, their multipliers
from a sign-constrained least-squares fit on the active set, as oracle/lpqp.kkt_certify does.
"""
import numpy as np
import pytest
from scipy.optimize import linprog, lsq_linear

from kkt_ref import certify_batch, feasible_fixing, kkt_certificate
from test_gpu_parity import _random_lp_batch

ACCEPT = 1e-9
REJECT = 1e-5


def _highs_xy(A, rl, ru, lb, ub, c):
    """x and the row duals y (positive = lower bound active) of one LP from HiGHS: equality
    rows from eqlin, <= rows as they come, >= rows negated."""
    eq = np.isfinite(rl) & np.isfinite(ru) & (rl == ru)
    ub_rows = (~eq) & np.isfinite(ru)
    lb_rows = (~eq) & np.isfinite(rl)
    A_ub = np.vstack([A[ub_rows], -A[lb_rows]])
    b_ub = np.concatenate([ru[ub_rows], -rl[lb_rows]])
    bounds = [(None if not np.isfinite(l) else l, None if not np.isfinite(u) else u) for l, u in zip(lb, ub)]
    res = linprog(c, A_ub=A_ub if len(b_ub) else None, b_ub=b_ub if len(b_ub) else None,
                  A_eq=A[eq] if eq.any() else None, b_eq=rl[eq] if eq.any() else None, bounds=bounds,
                  method="highs-ds", options={"primal_feasibility_tolerance": 1e-10,
                                              "dual_feasibility_tolerance": 1e-10})
    assert res.status == 0, res.message
    y = np.zeros(A.shape[0])
    if eq.any():
        y[eq] = res.eqlin.marginals
    if len(b_ub):
        mg = np.asarray(res.ineqlin.marginals)
        nu = int(ub_rows.sum())
        y[ub_rows] += mg[:nu]
        y[lb_rows] -= mg[nu:]
    return res.x, y, float(res.fun)


def _fit_y(A, rl, ru, lb, ub, c, q, x, act_tol=1e-7):
    """Row duals of a QP solution x: the sign-constrained least-squares fit of
    q x + c = A'y + (reduced costs of the active column bounds) on the active set."""
    m, n = A.shape
    ax = A @ x
    tol_r, tol_x = act_tol * (1.0 + np.abs(ax)), act_tol * (1.0 + np.abs(x))
    at_rl = np.isfinite(rl) & (ax - rl <= tol_r)
    at_ru = np.isfinite(ru) & (ru - ax <= tol_r)
    at_lb = np.isfinite(lb) & (x - lb <= tol_x)
    at_ub = np.isfinite(ub) & (ub - x <= tol_x)
    cols, lo, hi, rows = [], [], [], []
    for i in range(m):
        if at_rl[i] or at_ru[i]:
            cols.append(A[i])
            rows.append(i)
            lo.append(0.0 if not at_ru[i] else -np.inf)
            hi.append(0.0 if not at_rl[i] else np.inf)
    for j in range(n):
        if at_lb[j] or at_ub[j]:
            e = np.zeros(n)
            e[j] = 1.0
            cols.append(e)
            lo.append(0.0 if not at_ub[j] else -np.inf)
            hi.append(0.0 if not at_lb[j] else np.inf)
    y = np.zeros(m)
    if cols:
        sol = lsq_linear(np.array(cols).T, q * x + c, bounds=(np.array(lo), np.array(hi)), method="bvls", tol=1e-14)
        y[rows] = sol.x[:len(rows)]
    return y


LP_BATCHES = [(67, 9, 6, 0.5, 67), (97, 11, 7, 0.35, 2), (41, 30, 20, 0.2, 5)]
QP_BATCHES = [(67, 9, 6, 0.5, 67), (97, 11, 7, 0.35, 2)]
_CACHE = {}


def _lp_solutions(key):
    if ("lp", key) not in _CACHE:
        S, n, m, dens, seed = key
        b = _random_lp_batch(S, n, m, dens, seed=seed)
        xy = [_highs_xy(b.dense_A(s), b.rl[s], b.ru[s], b.lb[s], b.ub[s], b.c[s]) for s in range(S)]
        _CACHE["lp", key] = (b, np.array([v[0] for v in xy]), np.array([v[1] for v in xy]),
                             np.array([v[2] for v in xy]))
    return _CACHE["lp", key]


def _qp_solutions(key, ph=None, xfix=None):
    """(batch, x, y, obj, ph) of a with_q batch from the oracle's IPM on the effective problem
    (``ph``: dict of W, rho, xbar [S, 2]; ``xfix`` [S, 2])."""
    from oracle.lpqp import solve_qp_ipm
    tag = ("qp", key, ph is not None, xfix is not None)
    if tag not in _CACHE:
        S, n, m, dens, seed = key
        b = _random_lp_batch(S, n, m, dens, seed=seed, with_q=True)
        nc = np.asarray(b.nonant_col)
        X, Y, O = [], [], []
        for s in range(S):
            c, q, lb, ub, k = b.c[s].copy(), b.q[s].copy(), b.lb[s].copy(), b.ub[s].copy(), 0.0
            if ph is not None:
                c[nc] += ph["W"][s] - ph["rho"][s] * ph["xbar"][s]
                q[nc] += ph["rho"][s]
                k = 0.5 * float(np.sum(ph["rho"][s] * ph["xbar"][s] ** 2))
            if xfix is not None:
                for t, j in enumerate(nc):
                    if not np.isnan(xfix[s, t]):
                        lb[j] = ub[j] = min(max(xfix[s, t], lb[j]), ub[j])
            A = b.dense_A(s)
            # the oracle's IPM needs an interior: fixed columns are substituted out
            fx = lb == ub
            shift = A[:, fx] @ lb[fx]
            xf, ob, rc = solve_qp_ipm(A[:, ~fx], b.rl[s] - shift, b.ru[s] - shift, lb[~fx], ub[~fx], c[~fx], q[~fx])
            assert rc == 0
            x = lb.copy()
            x[~fx] = xf
            ob += float(c[fx] @ lb[fx] + 0.5 * np.sum(q[fx] * lb[fx] ** 2))
            X.append(x)
            Y.append(_fit_y(A, b.rl[s], b.ru[s], lb, ub, c, q, x))
            O.append(ob + k)
        _CACHE[tag] = (b, np.array(X), np.array(Y), np.array(O))
    return _CACHE[tag]


def _accept(cert, what):
    for k in ("pres", "dres", "gap", "obj_err", "bound_err", "xres"):
        w = np.abs(cert[k])
        assert w.max() <= ACCEPT, (what, k, float(w.max()), int(w.argmax()))


def _reject(b, x, y, what, qp=False, **kw):
    """-y, 1.001 y and a one-row shift of y are each rejected, max(dres, |gap|) > 1e-5, in every
    scenario that has a nonzero dual.  On a QP the gap is flat to first order in y wherever the
    columns a row touches are strictly convex, so 1.001 y moves it by 1e-8..3e-4 only (measured
    on these batches); there the stationarity residual ``xres`` joins the score of that one
    mutation and must exceed 1e-5 in the scenarios whose duals reach 1e-2 (xres is 0.001 |A'y| /
    q~ relative to 1 + |x|: a dual of 1e-6 cannot show at 1e-5 and does not matter at it)."""
    live = np.nonzero(np.abs(y).max(1) > 1e-9)[0]
    assert len(live) > b.S // 2, (what, len(live))
    for name, ym in (("-y", -y), ("1.001 y", 1.001 * y), ("roll", np.roll(y, 1, axis=1))):
        idx = live
        if qp and name == "1.001 y":
            idx = np.nonzero(np.abs(y).max(1) > 1e-2)[0]
            assert len(idx) > b.S // 2, (what, len(idx))
        cert = certify_batch(b, x, ym, scenarios=idx, **kw)
        score = np.maximum(cert["dres"], np.abs(cert["gap"]))
        if qp and name == "1.001 y":
            score = np.maximum(score, cert["xres"])
        assert score.min() > REJECT, (what, name, float(score.min()), int(idx[score.argmin()]))


@pytest.mark.parametrize("key", LP_BATCHES)
def test_lp_solutions_with_highs_marginals_are_accepted(key):
    b, x, y, obj = _lp_solutions(key)
    # obj and bound of an exact solve are both the optimum
    _accept(certify_batch(b, x, y, obj, obj), key)


@pytest.mark.parametrize("key", LP_BATCHES)
def test_lp_mutated_duals_are_rejected(key):
    b, x, y, obj = _lp_solutions(key)
    _reject(b, x, y, key)


@pytest.mark.parametrize("key", QP_BATCHES)
def test_qp_solutions_are_accepted_and_mutations_rejected(key):
    b, x, y, obj = _qp_solutions(key)
    _accept(certify_batch(b, x, y, obj, obj), key)
    _reject(b, x, y, key, qp=True)


def _ph_state(S):
    rng = np.random.default_rng(11)
    return {"W": rng.normal(size=(S, 2)), "rho": np.ones((S, 2)), "xbar": rng.uniform(0.0, 3.0, size=(S, 2))}


def test_ph_augmented_qp():
    """W, rho = 1 and xbar on the two nonants: the certificate's effective problem is the one
    the oracle solved (c~, q~ and the prox constant k)."""
    key = QP_BATCHES[0]
    ph = _ph_state(key[0])
    b, x, y, obj = _qp_solutions(key, ph=ph)
    kw = dict(W=ph["W"], rho=ph["rho"], xbar=ph["xbar"], W_on=1, prox_on=1)
    _accept(certify_batch(b, x, y, obj, obj, **kw), "ph")
    _reject(b, x, y, "ph", qp=True, **kw)
    # the same outputs against the problem without the PH terms do not certify
    plain = certify_batch(b, x, y, obj, obj)
    assert np.median(np.maximum(np.abs(plain["gap"]), plain["obj_err"])) > REJECT


def test_fixed_nonants_with_a_nan_and_a_clipped_entry():
    """Nonant 0 fixed inside its bounds (NaN in every fifth scenario: the model bounds stay),
    nonant 1 fixed outside its bounds where that clips back to a feasible value
    (kkt_ref.feasible_fixing, between the plain and the PH-augmented optimum)."""
    key = QP_BATCHES[0]
    _, xa, _, _ = _qp_solutions(key)
    b, xb, _, _ = _qp_solutions(key, ph=_ph_state(key[0]))
    xfix, clipped = feasible_fixing(b, xa, xb, nan_every=5)
    assert clipped.any() and np.isnan(xfix[::5, 0]).all()
    j = b.nonant_col[1]
    assert np.all((xfix[clipped, 1] < b.lb[clipped, j]) | (xfix[clipped, 1] > b.ub[clipped, j]))
    b, x, y, obj = _qp_solutions(key, xfix=xfix)
    fixed = ~np.isnan(xfix[:, 0])
    assert np.abs(x[fixed, 0] - xfix[fixed, 0]).max() <= 1e-12
    assert np.abs(x[:, 1] - np.clip(xfix[:, 1], b.lb[:, j], b.ub[:, j])).max() <= 1e-12
    free = certify_batch(b, x, y, obj, obj)                 # the unfixed problem: x is not optimal for it
    _accept(certify_batch(b, x, y, obj, obj, xfix=xfix), "fixed")
    _reject(b, x, y, "fixed", qp=True, xfix=xfix)
    assert np.abs(free["gap"]).max() > REJECT


def test_certificate_names_each_failure():
    """One hand-made LP: min x0 + x1, x0 + x1 >= 1, 0 <= x0 <= 2, x1 >= 0; x = (1, 0), y = 1."""
    A = np.array([[1.0, 1.0]])
    args = (A, np.array([1.0]), np.array([np.inf]), np.zeros(2), np.array([2.0, np.inf]), np.ones(2), np.zeros(2), 3.0)
    good = kkt_certificate(*args, x=np.array([1.0, 0.0]), y=np.array([1.0]), obj=4.0, bound=4.0)
    assert all(abs(float(good[k])) <= 1e-15 for k in ("pres", "dres", "gap", "obj_err", "bound_err"))
    assert float(good["f"]) == 4.0 and float(good["D"]) == 4.0
    infeas = kkt_certificate(*args, x=np.array([0.5, 0.0]), y=np.array([1.0]))
    assert abs(float(infeas["pres"]) - 0.25) <= 1e-15           # 0.5 below rl = 1: 0.5 / (1 + 1)
    wrong_side = kkt_certificate(*args, x=np.array([1.0, 0.0]), y=np.array([-1.0]))
    assert abs(float(wrong_side["dres"]) - 0.5) <= 1e-15        # y- = 1 on ru = +inf, 1 + max|c| = 2
    over = kkt_certificate(*args, x=np.array([1.0, 0.0]), y=np.array([1.5]))
    assert abs(float(over["dres"]) - 0.25) <= 1e-15             # g = -0.5 on x1 with ub = +inf
    assert abs(float(over["D"]) - (3.0 + 1.5 - 0.5 * 2.0)) <= 1e-15   # x1's component dropped
    off = kkt_certificate(*args, x=np.array([1.0, 0.0]), y=np.array([1.0]), obj=4.1, bound=3.9)
    assert abs(float(off["obj_err"]) - 0.02) <= 1e-12 and abs(float(off["bound_err"]) - 0.02) <= 1e-12
