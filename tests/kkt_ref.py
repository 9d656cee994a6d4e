"""KKT certificate of one scenario's solve outputs (TEST INFRASTRUCTURE ONLY; numpy in
``np.longdouble``, no solver).

phgpu_solve returns x, y, obj and bound per scenario (include/phgpu.h).  The certificate
recomputes, from the problem as the batch holds it and from x and y alone, everything that
weak duality needs to say "x and y are optimal together", so it needs no second solver and
no unique solution (degenerate LPs, where duals are not unique, certify like any other).

The effective problem of a solve (phgpu_set_ph_state, phgpu_fix_nonants) is

    min  c~'x + 1/2 sum q~ x^2 + k     s.t.  rl <= A x <= ru,  lb <= x <= ub

with, on the nonant columns,  c~ = c + W_on W - prox_on rho xbar,  q~ = q + prox_on rho,
k = obj_const + prox_on sum rho/2 xbar^2,  and a fixed nonant's lb = ub = clip(xfix, lb, ub)
(a NaN entry of xfix leaves the model bounds).

Row duals follow the library's convention: y_i > 0 prices the lower side rl_i, y_i < 0 the
upper side ru_i, in the caller's unscaled row space; g = c~ - A'y is the Lagrangian's linear
term in x.

The projection rule of D (the same in every solve path: row_dual_term / col_dual_term of
csrc/phgpu.hip for the PDHG paths, the KKT test of the jit_ipm*.hip.in kernels for the
interior points): a multiplier component that points at an infinite side contributes
nothing to the bound -- y+ on a row with rl = -inf, y- on a row with ru = +inf, g+ on a
column with lb = -inf and q~ = 0, g- on a column with ub = +inf and q~ = 0 -- and is
reported in ``dres`` instead.
"""
import numpy as np

LD = np.longdouble


def _ld(a):
    return np.asarray(a, dtype=LD)


def effective_problem(c, q, lb, ub, obj_const, nonant_col=None, W=None, rho=None, xbar=None,
                      W_on=0, prox_on=0, xfix=None):
    """(c~, q~, lb, ub, k) of one scenario in longdouble.  W, rho, xbar, xfix: [nn] over the
    nonant columns ``nonant_col`` (None: absent)."""
    ct, qt, lo, hi = _ld(c).copy(), _ld(q).copy(), _ld(lb).copy(), _ld(ub).copy()
    k = LD(obj_const)
    if nonant_col is not None and len(nonant_col):
        nc = np.asarray(nonant_col, dtype=np.int64)
        if W_on and W is not None:
            ct[nc] += _ld(W)
        if prox_on and rho is not None:
            r, xb = _ld(rho), _ld(xbar)
            ct[nc] -= r * xb
            qt[nc] += r
            k = k + np.sum(LD(0.5) * r * xb * xb)
        if xfix is not None:
            xf = _ld(xfix)
            fixed = ~np.isnan(xf)
            v = np.minimum(np.maximum(np.where(fixed, xf, LD(0)), lo[nc]), hi[nc])
            lo[nc] = np.where(fixed, v, lo[nc])
            hi[nc] = np.where(fixed, v, hi[nc])
    return ct, qt, lo, hi, k


def _fin_times(v, bnd):
    """v * bnd where bnd is finite, 0 elsewhere (no inf * 0)."""
    fin = np.isfinite(bnd)
    return np.where(fin, v * np.where(fin, bnd, LD(0)), LD(0))


def kkt_certificate(A, rl, ru, lb, ub, c, q, obj_const, x, y, obj=None, bound=None, nonant_col=None,
                    W=None, rho=None, xbar=None, W_on=0, prox_on=0, xfix=None):
    """The certificate of one scenario: a dict of

      pres       largest violation of a row range or column bound by x, each divided by
                 1 + |the bound it violates|
      dres       largest multiplier component pointing at a side that cannot carry it (y+ with
                 rl = -inf, y- with ru = +inf; with r = g + q~ x: r+ with lb = -inf and q~ = 0,
                 r- with ub = +inf and q~ = 0), divided by 1 + max|c~|
      f          the effective objective recomputed at x
      D          the Lagrangian bound recomputed from y, wrong-side components dropped:
                 k + sum_i (y+ rl - y- ru) + sum_j min over [lb, ub] of g_j x + 1/2 q~_j x^2
                 (the clipped stationary point for q~_j > 0, the bound g_j points at for q~_j = 0)
      gap        (f - D) / (1 + |f|): weak duality gives D <= optimum <= f up to pres and dres,
                 so a small gap certifies x and y together
      xres       on the columns with q~_j > 0, where y determines x: the largest
                 |x_j - clip(-g_j / q~_j, lb_j, ub_j)| / (1 + |x_j|).  The gap is flat to first
                 order in y on such columns (the Lagrangian bound is smooth there: 1.001 y moves
                 it by ~1e-6 |y|^2 |A|^2 / q~), so this residual is what sees a small error of y
                 on a strictly convex column; 0 for an LP
      obj_err    |obj - f| / (1 + |f|)      (NaN when obj is None)
      bound_err  |bound - D| / (1 + |D|)    (NaN when bound is None)
    """
    A = _ld(A)
    rl, ru, x, y = _ld(rl), _ld(ru), _ld(x), _ld(y)
    ct, qt, lo, hi, k = effective_problem(c, q, lb, ub, obj_const, nonant_col, W, rho, xbar, W_on, prox_on, xfix)
    zero = LD(0)
    # primal residual
    ax = A @ x
    viol = [zero]
    for v, bnd, sign in ((ax, rl, -1), (ax, ru, 1), (x, lo, -1), (x, hi, 1)):
        fin = np.isfinite(bnd)
        d = np.where(fin, sign * (v - np.where(fin, bnd, zero)), zero)
        viol.append(np.max(np.maximum(d, zero) / (1 + np.abs(np.where(fin, bnd, zero))), initial=zero))
    pres = max(viol)
    # dual residual
    yp, ym = np.maximum(y, zero), np.maximum(-y, zero)
    g = ct - A.T @ y
    r = g + qt * x
    lin = qt == 0
    wrong = [zero,
             np.max(np.where(np.isneginf(rl), yp, zero), initial=zero),
             np.max(np.where(np.isposinf(ru), ym, zero), initial=zero),
             np.max(np.where(lin & np.isneginf(lo), np.maximum(r, zero), zero), initial=zero),
             np.max(np.where(lin & np.isposinf(hi), np.maximum(-r, zero), zero), initial=zero)]
    dres = max(wrong) / (1 + np.max(np.abs(ct), initial=zero))
    # objective at x and the Lagrangian bound from y
    f = k + np.sum(ct * x + LD(0.5) * qt * x * x)
    D = k + np.sum(_fin_times(yp, rl)) - np.sum(_fin_times(ym, ru))
    qs = np.where(lin, LD(1), qt)
    xm = np.minimum(np.maximum(-g / qs, lo), hi)        # the clipped stationary point (q~ > 0)
    quad = g * xm + LD(0.5) * qt * xm * xm
    flat = _fin_times(np.maximum(g, zero), lo) - _fin_times(np.maximum(-g, zero), hi)
    D = D + np.sum(np.where(lin, flat, quad))
    xres = np.max(np.where(lin, zero, np.abs(x - xm) / (1 + np.abs(x))), initial=zero)
    out = {"pres": pres, "dres": dres, "f": f, "D": D, "gap": (f - D) / (1 + abs(f)), "xres": xres,
           "obj_err": LD("nan"), "bound_err": LD("nan")}
    if obj is not None:
        out["obj_err"] = abs(LD(obj) - f) / (1 + abs(f))
    if bound is not None:
        out["bound_err"] = abs(LD(bound) - D) / (1 + abs(D))
    return out


KEYS = ("pres", "dres", "gap", "obj_err", "bound_err", "xres", "f", "D")


def certify_batch(b, x, y, obj=None, bound=None, W=None, rho=None, xbar=None, W_on=0, prox_on=0, xfix=None,
                  scenarios=None, A=None):
    """kkt_certificate over the scenarios of a ScenarioBatch ``b`` and an engine's host arrays
    (``PHEngine.host``: x [S, n], y [S, m], obj / bound [S]; W, rho, xbar, xfix [S, nn] or
    None; ``A``: the scenarios' dense matrices if the caller keeps them, else b.dense_A(s)).
    Returns {name: float64 array over the scenarios} for the names in ``KEYS``."""
    idx = range(b.S) if scenarios is None else scenarios
    rows = []
    pick = lambda a, s: None if a is None else a[s]  # noqa: E731
    for s in idx:
        r = kkt_certificate(b.dense_A(s) if A is None else A[s], b.rl[s], b.ru[s], b.lb[s], b.ub[s], b.c[s], b.q[s],
                            b.obj_const[s], x[s], y[s][:b.m], pick(obj, s), pick(bound, s), b.nonant_col,
                            pick(W, s), pick(rho, s), pick(xbar, s), W_on, prox_on, pick(xfix, s))
        rows.append([float(r[k]) for k in KEYS])
    a = np.array(rows, dtype=np.float64).reshape(-1, len(KEYS))
    return {k: a[:, i] for i, k in enumerate(KEYS)}


def feasible_fixing(b, xa, xb, nan_every=0):
    """A nonant fixing [S, nn] (phgpu_fix_nonants) that keeps every scenario feasible, from two
    feasible points xa, xb [S, n] of the same scenarios (two solves with different objectives):
    the nonants of their midpoint z, which is feasible because the feasible set is convex.
    Nonant 0 is fixed at z (inside its bounds).  The last nonant is fixed outside its bounds, at
    lb - 1 or ub + 1, in the scenarios where z sits on that bound -- the value clips back to z --
    and at z elsewhere; the second return value marks those scenarios.  ``nan_every`` > 0 leaves
    nonant 0 of every nan_every-th scenario NaN (not fixed)."""
    nc = np.asarray(b.nonant_col, dtype=np.int64)
    z = 0.5 * (np.asarray(xa) + np.asarray(xb))
    xfix = z[:, nc].copy()
    j = nc[-1]
    at_lb = z[:, j] == b.lb[:, j]
    at_ub = (z[:, j] == b.ub[:, j]) & ~at_lb
    xfix[at_lb, -1] = b.lb[at_lb, j] - 1.0
    xfix[at_ub, -1] = b.ub[at_ub, j] + 1.0
    if nan_every:
        xfix[::nan_every, 0] = np.nan
    return xfix, at_lb | at_ub


def worst(cert):
    """{name: worst value over the scenarios} of the six residuals (|gap| for the gap)."""
    return {k: float(np.max(np.abs(cert[k]))) for k in KEYS[:6]}
