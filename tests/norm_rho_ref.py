"""Numpy restatement of NormRhoUpdater and the two convergers for the tests (TEST
INFRASTRUCTURE ONLY): mpisppy/extensions/norm_rho_updater.py:50-143,
mpisppy/convergers/norm_rho_converger.py:23-46, primal_dual_converger.py:44-124.

``Stepped`` steps an oracle (oracle.ph.OraclePH or oracle.farmer_vec.FarmerVecPH, which both
take per-scenario rho) by hand in the loop order of phbase.py:909-957: x̄, W, conv, miditer
(the rule), converger, solve.  Every (node, nonant) of the tree is one key; a scenario's
nonant j maps to key[s, j].
"""
import functools
import math

import numpy as np

# norm_rho_updater.py:12-20
DEFAULTS = {"convergence_tolerance": 1e-4, "rho_decrease_multiplier": 2.0, "rho_increase_multiplier": 2.0,
            "primal_dual_difference_factor": 100.0, "iterations_converged_before_decrease": 0,
            "rho_converged_decrease_multiplier": 1.1, "rho_update_stop_iterations": None, "verbose": False}

NONE, INC, DEC, CONV = 0, 1, 2, 3


def actions(p, d, tol, f, allow_decrease):
    """norm_rho_updater.py:134-143 for arrays of residuals: the action each entry takes."""
    p, d = np.asarray(p, dtype=np.float64), np.asarray(d, dtype=np.float64)
    inc = (p > f * d) & (p > tol)
    dec = ~inc & (d > f * p) & (d > tol)
    conv = ~inc & ~dec & (p < tol) & (d < tol)
    a = np.where(inc, INC, np.where(dec, DEC if allow_decrease else NONE, np.where(conv, CONV, NONE)))
    return a.astype(np.int64)


def apply_actions(rho, act, opts):
    """rho after the actions (rho *= increase, /= decrease, /= converged decrease)."""
    out = np.array(rho, dtype=np.float64, copy=True)
    out[act == INC] = out[act == INC] * opts["rho_increase_multiplier"]
    out[act == DEC] = out[act == DEC] / opts["rho_decrease_multiplier"]
    out[act == CONV] = out[act == CONV] / opts["rho_converged_decrease_multiplier"]
    return out


def perturbation_safe(p, d, rho_last, tol, f, allow_decrease):
    """True where the action does not change when p is replaced by p +- (1e-3 p + 1e-5) and d
    by d +- (1e-3 d + 1e-5 rho), in all four sign combinations: no decision of the
    trajectory sits on a threshold."""
    base = actions(p, d, tol, f, allow_decrease)
    ok = np.ones(base.shape, dtype=bool)
    for sp in (-1.0, 1.0):
        for sd in (-1.0, 1.0):
            pp = p + sp * (1e-3 * p + 1e-5)
            dd = d + sd * (1e-3 * d + 1e-5 * rho_last)
            ok &= actions(pp, dd, tol, f, allow_decrease) == base
    return ok


class Stepped:
    """An oracle stepped by hand with the rho rule between Update_W and the solve."""

    def __init__(self, oracle, key, prob, opts=None):
        self.o = oracle
        self.key = np.asarray(key)                  # [S, nn] -> (node, nonant) key
        self.prob = np.asarray(prob, dtype=np.float64)
        self.nkeys = int(self.key.max()) + 1
        self.opts = dict(DEFAULTS, **(opts or {}))
        self.prev_avg = None                        # NormRhoUpdater._prev_avg
        self.pd_prev = np.zeros(self.nkeys)         # PrimalDualConverger.prev_xbars (x̄ = 0 at Iter0)
        self.log = []

    # -- the oracle's loop pieces
    def iter0(self):
        return self.o.iter0()

    def _xbar_W_conv(self):
        o = self.o
        o.compute_xbar()
        if hasattr(o, "update_W"):
            o.update_W()
            return o.convergence_diff()
        o.W += o.rho * (o.x - o.xbar)                                   # phbase.py:293-318
        return np.abs(o.x - o.xbar).sum() / (o.S * o.K)               # phbase.py:321-343

    def _solve(self):
        o = self.o
        if hasattr(o, "solve_loop"):
            o.solve_loop()
        else:
            from oracle.farmer_vec import prox
            o.x, o.obj = prox(o.bp, o.sl, o.f0, o.W, o.xbar, o.rho, o.total)

    # -- per-key sums
    def _by_key(self, v):
        out = np.zeros(self.nkeys)
        np.add.at(out, self.key, v)
        return out

    def node_xbar(self):
        out = np.zeros(self.nkeys)
        out[self.key] = self.o.xbar                 # the same value for every scenario of a key
        return out

    def rho_last(self):
        out = np.zeros(self.nkeys)
        for s in range(self.key.shape[0]):          # scenario order: the last one wins
            out[self.key[s]] = self.o.rho[s]
        return out

    def primal_resid(self):                         # norm_rho_updater.py:55-96
        return self._by_key(self.prob[:, None] * np.abs(self.o.x - self.o.xbar))

    # -- norm_rho_updater.py:112-143
    def miditer(self, ph_iter):
        opts = self.opts
        stop = opts["rho_update_stop_iterations"]
        if stop is not None and ph_iter > stop:
            return None
        xb = self.node_xbar()
        if self.prev_avg is None:
            self.prev_avg = xb
            return None
        p = self.primal_resid()
        rl = self.rho_last()
        d = rl * np.abs(xb - self.prev_avg)          # norm_rho_updater.py:98-104
        self.prev_avg = xb
        allow = ph_iter >= opts["iterations_converged_before_decrease"]
        act = actions(p, d, opts["convergence_tolerance"], opts["primal_dual_difference_factor"], allow)
        self.o.rho[...] = apply_actions(self.o.rho, act[self.key], opts)
        rec = {"iter": ph_iter, "p": p, "d": d, "rho_last": rl, "act": act, "allow": allow,
               "counts": np.bincount(act[self.key].ravel(), minlength=4)}
        self.log.append(rec)
        return rec

    # -- primal_dual_converger.py:58-124 (pcoef: the x̄ weights, [S, nn])
    def primal_dual(self, pcoef):
        primal = float((pcoef * np.abs(self.o.x - self.o.xbar)).sum())
        xb = self.node_xbar()
        dual = float((self._by_key(self.o.rho) * np.abs(xb - self.pd_prev)).sum())
        self.pd_prev = xb
        return primal, dual

    # -- norm_rho_converger.py:23-46
    def log_rho_norm(self):
        return math.log(float((self.prob[:, None] * self.o.rho).sum()))

    def run(self, iters, updater=True, pcoef=None, pd_tol=None):
        """``iters`` PH iterations (or up to the primal-dual converger's break); returns the
        per-iteration records {conv, gaps, log_rho_norm}."""
        hist = []
        for it in range(1, iters + 1):
            conv = self._xbar_W_conv()
            if updater:
                self.miditer(it)
            h = {"iter": it, "conv": conv, "log_rho_norm": self.log_rho_norm()}
            if pcoef is not None:
                h["primal"], h["dual"] = self.primal_dual(pcoef)
            hist.append(h)
            if pd_tol is not None and max(h["primal"], h["dual"]) <= pd_tol:
                break
            self._solve()
        self.hist = hist
        return hist


def _oracle_keys(o):
    """key[s, j], node names and nlen_max of an OraclePH's tree (node order: first seen)."""
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


AIR_BF = [4, 3, 2]
AIR_KW = dict(Capacity=200, QuadShortCoeff=0.3, BeginInventory=50, mu_dev=0, sigma_dev=40, start_seed=0)

CASES = {
    "farmer3": {"factor": 2.0, "iters": 12},
    "farmer1000": {"factor": 2.0, "iters": 10},
    "aircond432": {"factor": 10.0, "iters": 8},
}


def make(case, opts=None):
    """A fresh Stepped oracle of a case (rho0 = 1) with the case's difference factor."""
    from oracle.ph import OraclePH
    o2 = dict({"primal_dual_difference_factor": CASES[case]["factor"]}, **(opts or {}))
    if case == "farmer3":
        from oracle.models import farmer_scenario, farmer_yields
        names = ["scen0", "scen1", "scen2"]
        scens = [farmer_scenario(n, 1, num_scens=3) for n in names]
        crops_sorted = sorted(farmer_yields("scen0", 1)[0])
        o = OraclePH(scens, 1.0, solver="farmer",
                     farmer_info=(crops_sorted, [farmer_yields(n, 1)[1] for n in names], 1))
    elif case == "farmer1000":
        from oracle.farmer_vec import FarmerVecPH
        o = FarmerVecPH([f"scen{i}" for i in range(1000)], 1, rho=1.0, num_scens=1000)
        st = Stepped(o, np.tile(np.arange(3), (1000, 1)), o.prob, o2)
        st.node_names, st.nlen_max = ["ROOT"], 3
        st.pcoef = np.tile(o.prob[:, None], (1, 3))
        return st
    elif case == "aircond432":
        from oracle.models import aircond_scenario
        o = OraclePH([aircond_scenario(f"scen{i}", AIR_BF, **AIR_KW) for i in range(24)], 1.0)
    else:
        raise KeyError(case)
    key, names, nl = _oracle_keys(o)
    st = Stepped(o, key, [s.prob for s in o.scens], o2)
    st.node_names, st.nlen_max = names, nl
    st.pcoef = np.array([[pc for (_, a, b), pc in zip(o.node_slices[s], o.prob_coeff[s]) for _ in range(b - a)]
                         for s in range(len(o.scens))])
    return st


@functools.lru_cache(maxsize=None)
def trajectory(case):
    """The case's stepped oracle after its iterations, computed once per session and shared
    (read-only) by the tests: the Stepped object with ``log`` (rule records), ``hist``
    (conv, gaps, rho norm per iteration) and ``trivial_bound``."""
    st = make(case)
    st.trivial_bound = st.iter0()
    st.run(CASES[case]["iters"], updater=True, pcoef=st.pcoef)
    return st


# PrimalDualConverger on farmer3 with the updater on (factor 2): the tolerance, and the
# iteration at which max(primal, dual) first drops to it on the oracle's trajectory
PD_TOL = 40.0
PD_BREAK = 4
