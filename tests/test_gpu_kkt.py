"""Every solve path's x, y, obj and bound under the KKT certificate of tests/kkt_ref.py.

phgpu_solve's row duals ``y`` (positive = lower bound active, the caller's unscaled row space)
are written by about ten separate pieces of code -- k_solve, solve_reg.inc in scenario order and
in record mode (k_from_records), solve_wg.inc, solve_stream.inc, jit_kernel.hip.in, the five
interior-point epilogues and the path-5 fallback over path 6's fail list -- and ``bound`` is
formed from the kernels' internal duals before any of that output code runs.  One case per
y-writing code: a cold solve, a warm PH solve (W, rho = 1, x̄ bound: the paths' PH plumbing) and
two solves with fixed nonants (phgpu_fix_nonants: one value inside the bounds, one outside that
clips, one run with NaN entries), each certified against the effective problem in longdouble;
then the bounds are restored and the first solve's objectives must return.  x and y are filled
with NaN before every solve, so a row or column a kernel does not write fails the certificate.

Thresholds are the project's own (north_star): pres <= 1e-6; dres, |gap|, obj_err and bound_err
<= OBJ_REL = 1e-5.  test_kkt_ref.py shows that a 0.1 % error of y exceeds them on an LP.  On the
QP batches (q >= 0.05: x unique) x is also held to the oracle's, |x - x_oracle| <= 1e-5 (1 +
|x_oracle|).  xres, the distance of x from the x that y implies on strictly convex columns, is
printed and not asserted: the kernels stop on the gap, which holds x on a column of curvature q
only to sqrt(2 gap (1 + |f|) / q), and no tolerance of the project bounds it further.
Every case prints its worst residuals; DESIGN.md section 4 has the measured table.
"""
import contextlib
import os

import numpy as np
import pytest

from kkt_ref import certify_batch, worst
from test_gpu_parity import GOLD, OBJ_REL, _random_lp_batch
from test_gpu_wg import _long_row_col_batch
from test_gpu_ipm_wave import arrow_batch
from test_gpu_config4 import KW as AIRCOND_KW

pytestmark = pytest.mark.gpu

PRES_TOL = 1e-6
X_REL = 1e-5
TOL = {"pres": PRES_TOL, "dres": OBJ_REL, "gap": OBJ_REL, "obj_err": OBJ_REL, "bound_err": OBJ_REL}
ENV_KEYS = ("PHGPU_REG_REC", "PHGPU_WPS", "PHGPU_IPM", "PHGPU_IPM_LANES", "PHGPU_IPM_LDS", "PHGPU_IPM_WAVE",
            "PHGPU_IPM_BLK", "PHGPU_IPM_MAXIT", "PHGPU_LANES", "PHGPU_JIT")


@contextlib.contextmanager
def _env(env):
    """The case's environment: the variables that pick a kernel are cleared, the case's set,
    and all of them restored afterwards."""
    keep = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------- batches (built once)
_BATCH = {}


def _batch(kind, *a):
    key = (kind,) + a
    if key not in _BATCH:
        from mpisppy_amd.examples import aircond, farmer
        if kind == "rand":
            S, n, m, dens, seed, wq = a
            b = _random_lp_batch(S, n, m, dens, seed=seed, with_q=wq)
        elif kind == "longrc":
            S, wq = a
            b = _long_row_col_batch(S, seed=S, with_q=wq)
        elif kind == "arrow":
            S, blocks, wq, free_row, shapes = a
            b = arrow_batch(S, blocks, seed=blocks + S, with_q=wq, shapes=shapes)
            if free_row:
                # a block row free in every scenario: the subtree kernel's INACT rows (y = 0)
                b.rl[:, 1] = -np.inf
                b.ru[:, 1] = np.inf
        elif kind == "farmer":
            S, cm = a
            b = farmer.batch_creator(farmer.scenario_names_creator(S), crops_multiplier=cm, num_scens=S)
        elif kind == "aircond432":
            g = GOLD["aircond432_rho1"]
            b = aircond.batch_creator(g["names"], branching_factors=g["branching_factors"], **g["kwargs"])
        else:
            bf = list(a)
            b = aircond.batch_creator(aircond.scenario_names_creator(int(np.prod(bf))), branching_factors=bf,
                                      **AIRCOND_KW)
        qp = kind in ("rand", "longrc", "arrow") and bool(b.q.any())
        if qp:
            b.q[:] = np.maximum(b.q, 0.05)     # x unique and well conditioned
        _BATCH[key] = {"b": b, "qp": qp, "A": [b.dense_A(s) for s in range(b.S)], "x_oracle": None}
    return _BATCH[key]


def _oracle_x(ent):
    """The oracle's x of a QP batch (computed once, shared by the cases on that batch)."""
    if ent["x_oracle"] is None:
        from oracle.lpqp import solve_qp_ipm
        b, xs = ent["b"], []
        for s in range(b.S):
            x, _, rc = solve_qp_ipm(ent["A"][s], b.rl[s], b.ru[s], b.lb[s], b.ub[s], b.c[s], b.q[s])
            assert rc == 0, s
            xs.append(x)
        ent["x_oracle"] = np.array(xs)
        ent["x_oracle"].setflags(write=False)
    return ent["x_oracle"]


def _interior_point(A, rl, ru, lb, ub, at_lb=None):
    """(x, t): the point of largest margin t <= 1 to every inequality row side and column bound
    (equality rows hold exactly; column ``at_lb``, if given, sits on its lower bound), or
    (None, 0) if there is none.  One small LP (scipy HiGHS)."""
    from scipy.optimize import linprog
    m, n = A.shape
    eq = rl == ru
    rows, rhs = [], []
    for i in np.nonzero(~eq)[0]:
        if np.isfinite(rl[i]):
            rows.append(np.append(-A[i], 1.0))
            rhs.append(-rl[i])
        if np.isfinite(ru[i]):
            rows.append(np.append(A[i], 1.0))
            rhs.append(ru[i])
    for j in range(n):
        if j == at_lb:
            continue
        e = np.zeros(n + 1)
        e[n] = 1.0
        if np.isfinite(lb[j]):
            e[j] = -1.0
            rows.append(e.copy())
            rhs.append(-lb[j])
        if np.isfinite(ub[j]):
            e[j] = 1.0
            rows.append(e.copy())
            rhs.append(ub[j])
    Aeq = [np.append(A[i], 0.0) for i in np.nonzero(eq)[0]]
    beq = list(rl[eq])
    if at_lb is not None:
        e = np.zeros(n + 1)
        e[at_lb] = 1.0
        Aeq.append(e)
        beq.append(lb[at_lb])
    cost = np.zeros(n + 1)
    cost[n] = -1.0
    res = linprog(cost, A_ub=np.array(rows), b_ub=np.array(rhs), A_eq=np.array(Aeq) if Aeq else None,
                  b_eq=np.array(beq) if Aeq else None, bounds=[(None, None)] * n + [(0.0, 1.0)], method="highs")
    if res.status != 0:
        return None, 0.0
    return res.x[:n], float(res.x[n])


MARGIN = 1e-3


def _fixing(ent):
    """A nonant fixing [S, nn] (phgpu_fix_nonants) whose completion is strictly feasible: the
    nonants of a point with margin >= 1e-3 to every inequality and bound, so that the fixed
    problem stays well posed at the solvers' 1e-9 feasibility.  (The nonants of a solve's own x
    are feasible to 1e-9 only: fixed there, a scenario whose other columns sit on their bounds
    is infeasible by that much, and a first-order solve then stalls a hair above its gap
    tolerance.)  Nonant 0 lies inside its bounds.  The last nonant is fixed one below its lower
    bound -- the value clips to the bound -- in the scenarios that keep the margin with that
    column on its bound, inside its bounds in the others; the second return value marks them."""
    if "xfix" not in ent:
        b = ent["b"]
        j = int(b.nonant_col[-1])
        xfix = np.empty((b.S, b.nn))
        clip = np.zeros(b.S, dtype=bool)
        for s in range(b.S):
            x, t = (None, 0.0)
            if np.isfinite(b.lb[s, j]):
                x, t = _interior_point(ent["A"][s], b.rl[s], b.ru[s], b.lb[s], b.ub[s], at_lb=j)
            clip[s] = t >= MARGIN
            if not clip[s]:
                x, t = _interior_point(ent["A"][s], b.rl[s], b.ru[s], b.lb[s], b.ub[s])
                assert t >= MARGIN, (s, t)
            xfix[s] = x[b.nonant_col]
            if clip[s]:
                xfix[s, -1] = b.lb[s, j] - 1.0
        xfix.setflags(write=False)
        ent["xfix"], ent["clip"] = xfix, clip
    return ent["xfix"], ent["clip"]


# ---------------------------------------------------------------- which kernel ran
def _only_pdhg(e):
    ii = e.ipm_info()
    assert ii["compiled"] == 0, ii


def _ran_global(e, it, fixed=False):
    info = e.kernel_info()
    _only_pdhg(e)
    assert info["rec"] == -1 and info["jit_wpe"] == 0, info


def _ran_reg(rec):
    def check(e, it, fixed=False):
        info = e.kernel_info()
        _only_pdhg(e)
        assert info["instance"] >= 0 and info["rec"] == rec and info["jit_wpe"] == 0, info
    return check


def _ran_wg(wps):
    def check(e, it, fixed=False):
        info = e.kernel_info()
        _only_pdhg(e)
        assert info["wg_instance"] >= 0 and info["wps"] == wps and info["rec"] == -1 and info["jit_wpe"] == 0, info
    return check


def _ran_stream(e, it, fixed=False):
    assert e.kernel_info()["path"] == 4 and e.stream_info()["path4"] == 1, (e.kernel_info(), e.stream_info())


def _ran_jit(e, it, fixed=False):
    info = e.kernel_info()
    _only_pdhg(e)
    assert info["jit_wpe"] >= 1 and info["rec"] == -1, info


def _ran_ipm(kernel, lanes=None, lds=None):
    def check(e, it, fixed=False):
        ii = e.ipm_info()
        assert ii["compiled"] == 1 and int(ii["kernel"]) == kernel, ii
        if lanes is not None:
            assert int(ii["lanes"]) == lanes, ii
        else:
            assert ii["lanes"] >= 64, ii
        if lds is not None:
            assert int(ii["lds_slacks"]) == lds, ii
        # interior-point iterations: nothing went to the fallback.  With fixed nonants path 6 may
        # hand a scenario it does not finish to its PDHG fallback (certified like the others)
        late = int((it > 80).sum())
        assert late == 0 or (fixed and late <= max(1, it.size // 50)), (late, it.max())
    return check


def _ran_fallback(e, it, fixed=False):
    ii = e.ipm_info()
    assert ii["compiled"] == 1 and int(ii["kernel"]) in (1, 2), ii
    assert it.min() > 2, it.min()                # PDHG iteration counts: every scenario's outputs are the fallback's


# ---------------------------------------------------------------- the cases
RAND96 = ("rand", 67, 9, 6, 0.5, 67, False)
RAND96Q = ("rand", 130, 9, 6, 0.5, 130, True)
FARMER1 = ("farmer", 256, 1)


def _case(cid, batch, check, kernel=0, env=None, shared=None, eps=None):
    opts = {"kernel": kernel}
    if eps is not None:
        opts["eps_rel"] = eps
    return pytest.param(batch, check, opts, env or {}, shared, id=cid)


def _ipm_cases():
    out = []
    for lanes, kern in ((1, 1), (4, 2), (8, 2)):
        env = {"PHGPU_IPM_LANES": str(lanes)}
        for nm, bt, eps in (("lp", RAND96, None), ("qp", RAND96Q, None), ("farmer", FARMER1, 1e-10)):
            out.append(_case(f"6-lanes{lanes}-{nm}", bt, _ran_ipm(kern, lanes), kernel=6, env=env, eps=eps))
    return out


CASES = [
    _case("1-global-lp", RAND96, _ran_global, kernel=1),
    _case("1-global-qp", RAND96Q, _ran_global, kernel=1),
    _case("2-reg-order-qp", ("rand", 97, 11, 7, 0.35, 2, True), _ran_reg(0), kernel=2, env={"PHGPU_REG_REC": "0"}),
    _case("2-reg-order-lp", ("rand", 300, 11, 7, 0.35, 3, False), _ran_reg(0), kernel=2, env={"PHGPU_REG_REC": "0"}),
    _case("2-reg-records-qp", ("rand", 97, 11, 7, 0.35, 2, True), _ran_reg(1), kernel=2, env={"PHGPU_REG_REC": "1"}),
    _case("2-reg-records-lp", ("rand", 300, 11, 7, 0.35, 3, False), _ran_reg(1), kernel=2,
          env={"PHGPU_REG_REC": "1"}),
    _case("3-wg-wps1-qp", ("longrc", 67, True), _ran_wg(1), kernel=3, env={"PHGPU_WPS": "1"}),
    _case("3-wg-wps4-lp", ("longrc", 40, False), _ran_wg(4), kernel=3, env={"PHGPU_WPS": "4"}),
    _case("4-stream-aircond432", ("aircond432",), _ran_stream, shared=True),
    _case("5-jit-qp", RAND96Q, _ran_jit, kernel=5),
    *_ipm_cases(),
    _case("6-lane1-aircond-lds", ("aircond", 8, 8, 8), _ran_ipm(1, 1, lds=1), env={"PHGPU_IPM_LANES": "1"}),
    _case("6-lane1-aircond-regs", ("aircond", 8, 8, 8), _ran_ipm(1, 1, lds=0),
          env={"PHGPU_IPM_LANES": "1", "PHGPU_IPM_LDS": "0"}),
    _case("6-subtree-farmer-cm10", ("farmer", 64, 10), _ran_ipm(4, 64), eps=1e-10),
    _case("6-subtree-arrow", ("arrow", 24, 15, False, True, "two"), _ran_ipm(4), env={"PHGPU_IPM_WAVE": "1"}),
    _case("6-workgroup-arrow-qp", ("arrow", 40, 30, True, False, "random"), _ran_ipm(3),
          env={"PHGPU_IPM_WAVE": "1", "PHGPU_IPM_BLK": "0"}),
    _case("6-fallback-lp", RAND96, _ran_fallback, kernel=6, env={"PHGPU_IPM_MAXIT": "2"}),
]


def _solve_and_certify(e, ent, opts, warm, what, **prob):
    """One solve into NaN-filled x / y, certified: returns (outputs, worst residuals)."""
    from mpisppy_amd import _lib
    e.x.fill_(float("nan"))
    e.y.fill_(float("nan"))
    e.solve(_lib.default_options(**opts), warm=warm)
    out = {k: e.host(k).copy() for k in ("x", "y", "obj", "bound", "status", "iters")}
    assert (out["status"] == _lib.OPTIMAL).all(), (what, out["status"], out["iters"])
    cert = certify_batch(ent["b"], out["x"], out["y"], out["obj"], out["bound"], A=ent["A"], **prob)
    w = worst(cert)
    print(f"KKT {what}: " + " ".join(f"{k}={v:.1e}" for k, v in w.items()), flush=True)
    return out, cert, w


def _assert_certified(cert, w, what):
    for k, tol in TOL.items():
        assert w[k] <= tol, (what, k, w[k], int(np.nanargmax(np.abs(cert[k]))))


@pytest.mark.parametrize("batch,check,opts,env,shared", CASES)
def test_solve_outputs_are_kkt_certified(gpu, request, batch, check, opts, env, shared):
    import torch
    from mpisppy_amd.engine import PHEngine
    cid = request.node.callspec.id
    ent = _batch(*batch)
    b = ent["b"]
    with _env(env):
        e = PHEngine(b, device="cuda:0", shared=shared)
        e.want_duals = True
        try:
            # 1. the cold solve of the model itself
            o0, cert, w = _solve_and_certify(e, ent, opts, False, f"{cid} cold")
            check(e, o0["iters"])
            _assert_certified(cert, w, f"{cid} cold")
            if ent["qp"]:
                xo = _oracle_x(ent)
                err = np.abs(o0["x"] - xo) / (1.0 + np.abs(xo))
                print(f"KKT {cid} cold: x_vs_oracle={err.max():.1e}", flush=True)
                assert err.max() <= X_REL, (cid, err.max(), np.unravel_index(err.argmax(), err.shape))
            # 2. a warm PH solve: W, rho = 1 and x̄ bound
            rng = np.random.default_rng(1)
            W = rng.normal(size=(b.S, b.nn))
            xb = rng.uniform(0.0, 3.0, size=(b.S, b.nn))
            rho = np.ones((b.S, b.nn))
            ph = dict(W=W, rho=rho, xbar=xb, W_on=1, prox_on=1)
            e.set_rho(1.0)
            e.set_W(W)
            e.set_xbar(xb)
            e.set_terms(1, 1)
            o1, cert, w = _solve_and_certify(e, ent, opts, True, f"{cid} ph", **ph)
            check(e, o1["iters"])
            _assert_certified(cert, w, f"{cid} ph")
            # 3. fixed nonants: every nonant fixed without the PH terms (an xhat evaluation), then
            #    with nonant 0 of every third scenario NaN (left free) and the PH terms
            for nan_every, terms in ((0, 0), (3, 1)):
                xfix, clipped = _fixing(ent)
                # (farmer keeps no margin with an acreage on its bound: that crop's sales are
                # then forced to zero, so its batches get no clipping value)
                assert clipped.any() or batch[0] == "farmer", cid
                if nan_every:
                    xfix = xfix.copy()
                    xfix[::nan_every, 0] = np.nan
                e.set_terms(terms, terms)
                e.fix_nonants(torch.as_tensor(np.ascontiguousarray(xfix.T), device=e.device))
                what = f"{cid} fixed{'+nan+ph' if nan_every else ''}"
                print(f"KKT {what}: {int(clipped.sum())} of {b.S} scenarios clip", flush=True)
                o2, cert, w = _solve_and_certify(e, ent, opts, True, what, xfix=xfix, **(ph if terms else {}))
                check(e, o2["iters"], fixed=True)
                _assert_certified(cert, w, what)
                j = b.nonant_col[-1]
                want = np.clip(xfix[:, -1], b.lb[:, j], b.ub[:, j])
                assert np.abs(o2["x"][:, j] - want).max() <= 1e-7 * (1.0 + np.abs(want).max()), what
            # 4. the model bounds again: the first solve's objectives return
            e.fix_nonants(None)
            e.set_terms(0, 0)
            o3, cert, w = _solve_and_certify(e, ent, opts, False, f"{cid} restored")
            _assert_certified(cert, w, f"{cid} restored")
            assert np.all(np.abs(o3["obj"] - o0["obj"]) <= OBJ_REL * (1.0 + np.abs(o0["obj"]))), cid
        finally:
            e.close()
