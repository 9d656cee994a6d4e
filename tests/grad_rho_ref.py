"""Numpy restatement of the gradient / cost-proportional rho tools for the tests (TEST
INFRASTRUCTURE ONLY): mpisppy/utils/find_rho.py:78-203, utils/gradient.py:65-81,
utils/wtracker.py:134-157, extensions/gradient_extension.py:60-95 and
extensions/mult_rho_updater.py:78-100.

Arrays are [S, nn] (scenario, nonant) as the oracles hold them.  ``GradStepped`` steps an
oracle of tests/norm_rho_ref.py by hand in the loop order of phbase.py:909-957 with the rule of
gradient_extension.py:80-95 between Update_W and the solve.
"""
import csv
import functools

import numpy as np

import norm_rho_ref as N

# the farmer's planting costs per acre in nonant order (CORN, SUGAR_BEETS, WHEAT): the true
# derivative of the objective with respect to DevotedAcreage, negated as gradient.py:79 does
FARMER_COST = np.array([-230.0, -260.0, -150.0])


# ---------------------------------------------------------------- find_rho.py
def w_denom(x, xbar):
    """find_rho.py:78-95, every scenario's row."""
    return np.abs(x - xbar)


def prox_denom(x, xbar):
    """find_rho.py:98-115."""
    return 2 * np.square(x - xbar)


def grad_denom(x, xbar, pcoef, rel_bound=1e3):
    """find_rho.py:118-147: sum_s prob_coeff |x - x̄| per nonant, bounded below."""
    g = (pcoef * np.abs(x - xbar)).sum(axis=0)
    return np.maximum(np.ones(len(g)) / rel_bound, g)


def order_stat(rho_list, alpha):
    """find_rho.py:150-168."""
    assert 0 <= alpha <= 1
    rho_mean, rho_min, rho_max = np.mean(rho_list), np.min(rho_list), np.max(rho_list)
    if alpha == 0.5:
        return rho_mean
    if alpha < 0.5:
        return rho_min + alpha * 2 * (rho_mean - rho_min)
    return (2 * rho_mean - rho_max) + alpha * 2 * (rho_max - rho_mean)


def ratios(cost, x, xbar, gden=None):
    """|cost / denom| of find_rho.py:185-200, [S, nn].  Scenario-dependent mode: np.max over the
    PAIR of arrays (w_denom, prox_denom) at :189 is one scalar per scenario."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if gden is not None:
            return np.abs(np.divide(cost, gden[None, :]))
        d = np.array([np.max((w_denom(x[s], xbar[s]), prox_denom(x[s], xbar[s]))) for s in range(x.shape[0])])
        return np.abs(np.divide(cost, d[:, None]))


def planes(r):
    """What phgpu_rho_ratio_stats reduces the ratios to: sum, max(-r), max(r) per nonant."""
    return np.stack([r.sum(axis=0), (-r).max(axis=0), r.max(axis=0)])


def compute_rho(cost, x, xbar, alpha, gden=None):
    """find_rho.py:170-203: one rho per nonant."""
    r = ratios(cost, x, xbar, gden)
    return np.array([order_stat(r[:, k], alpha) for k in range(r.shape[1])])


# ---------------------------------------------------------------- gradient.py / wtracker.py
def grad_cost(c, q, xn):
    """gradient.py:65-81 for f = c.x + 1/2 x.diag(q).x on the nonant columns."""
    return -(c + q * xn)


def w_diff(W, W_prev):
    """wtracker.py:141-157 with one rank."""
    return np.abs(W - W_prev).sum() / W.size


def gate_ratio(prev, cur):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs((np.float64(prev) - np.float64(cur)) / np.float64(prev))


def gate_open(prev, cur, thr=0.05):
    """gradient_extension.py:65-68 (NaN and inf compare False)."""
    return bool(gate_ratio(prev, cur) <= thr)


# ---------------------------------------------------------------- the csv formats
def read_cost_csv(path):
    """{(scenario, variable): cost} of a grad cost / What csv."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.reader(f):
            if row and not row[0].startswith("#"):
                out[(row[0], row[1])] = float(row[2])
    return out


def read_rho_csv(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.reader(f):
            if row and not row[0].startswith("#"):
                out[row[0]] = float(row[1])
    return out


# ---------------------------------------------------------------- mult_rho_updater.py:78-100
class MultRho:
    def __init__(self, rho0, tol=1e-4, start=None, stop=None):
        self.rho = np.array(rho0, dtype=np.float64, copy=True)
        self.tol, self.start, self.stop = tol, start, stop
        self.first_rho = None
        self.best = float("inf")
        self.acted = []

    def miditer(self, it, conv):
        if (self.stop is not None and it > self.stop) or (self.start is not None and it < self.start):
            return
        if conv < self.best:
            self.best = conv
        else:
            return
        if self.first_rho is None:
            if conv is None or conv == self.tol:
                return
            self.first_c = conv
            self.first_rho = self.rho.copy()
        elif conv != 0:
            self.rho[...] = self.first_rho * self.first_c / conv
            self.acted.append(it)


# ---------------------------------------------------------------- gradient_extension.py:74-95
class GradStepped:
    """A stepped oracle with the gradient rho rule between Update_W and the solve."""

    def __init__(self, st, cost, alpha, thr=0.05, gden_pcoef=None):
        self.st, self.o = st, st.o
        self.cost = np.broadcast_to(np.asarray(cost, dtype=np.float64), self.o.rho.shape)
        self.alpha, self.thr = alpha, thr
        self.pcoef = gden_pcoef                       # not None: the scenario-independent denominator
        self.log = []

    def iter0(self):
        tb = self.st.iter0()
        self.W_prev = self.o.W.copy()
        self.wd = [w_diff(self.o.W, self.W_prev)]     # post_iter0: 0
        return tb

    def run(self, iters, convthresh=-1.0, mult=None):
        o = self.o
        for it in range(1, iters + 1):
            conv = self.st._xbar_W_conv()
            rec = {"iter": it, "conv": conv, "x": o.x.copy(), "xbar": o.xbar.copy(), "W": o.W.copy()}
            if mult is not None:
                mult.rho = o.rho
                mult.miditer(it, conv)
            else:
                self.wd.append(w_diff(o.W, self.W_prev))
                self.W_prev = o.W.copy()
                rec["w_diff"] = self.wd[-1]
                rec["ratio"] = float(gate_ratio(self.wd[-2], self.wd[-1]))
                rec["applied"] = gate_open(self.wd[-2], self.wd[-1], self.thr)
                if rec["applied"]:
                    gden = None if self.pcoef is None else grad_denom(o.x, o.xbar, self.pcoef)
                    o.rho[...] = compute_rho(self.cost, o.x, o.xbar, self.alpha, gden)[None, :]
            rec["rho"] = o.rho.copy()
            self.log.append(rec)
            if conv < convthresh:
                break
            self.st._solve()
        return self.log

    def applied_iterations(self):
        return {r["iter"] for r in self.log if r.get("applied")}


def perturbation_tolerance(rec, cost, alpha, seed=0, patterns=16, dx=1e-5):
    """Twice the largest relative change of the oracle's rho at a rewrite when its x moves by
    +-dx (the project's bar on x) in ``patterns`` random sign patterns: how far a rho computed
    from an x within that bar may be from the oracle's."""
    rng = np.random.default_rng(seed)
    x, xbar = rec["x"], rec["xbar"]
    cost = np.broadcast_to(np.asarray(cost, dtype=np.float64), x.shape)
    base = compute_rho(cost, x, xbar, alpha)
    worst = 0.0
    for _ in range(patterns):
        sg = rng.choice([-1.0, 1.0], size=x.shape)
        worst = max(worst, float(np.abs(compute_rho(cost, x + dx * sg, xbar, alpha) / base - 1).max()))
    return 2 * worst


CASES = {
    "farmer3": {"alpha": 0.4, "iters": 15, "thresh": -1.0, "applied": {4, 11}},
    "farmer1000": {"alpha": 0.5, "iters": 30, "thresh": 1e-3, "applied": {11, 20}},
    # the two-rank case, 96 + 97 scenarios (its next gate ratio under 0.05 is 0.039 at 16)
    "farmer193": {"alpha": 0.5, "iters": 12, "thresh": -1.0, "applied": {8}},
}


def make(case):
    """A fresh stepped oracle of a farmer case (rho0 = 1); sizes tests/norm_rho_ref.py does not
    name are built the way it builds farmer1000."""
    if case in N.CASES:
        return N.make(case)
    from oracle.farmer_vec import FarmerVecPH
    S = int(case[len("farmer"):])
    o = FarmerVecPH([f"scen{i}" for i in range(S)], 1, rho=1.0, num_scens=S)
    st = N.Stepped(o, np.tile(np.arange(3), (S, 1)), o.prob)
    st.node_names, st.nlen_max = ["ROOT"], 3
    st.pcoef = np.tile(o.prob[:, None], (1, 3))
    return st


@functools.lru_cache(maxsize=None)
def trajectory(case):
    """The case's stepped oracle after its run, computed once per session and shared
    (read-only): the GradStepped with ``log`` and ``trivial_bound``."""
    c = CASES[case]
    g = GradStepped(make(case), FARMER_COST, c["alpha"])
    g.trivial_bound = g.iter0()
    g.run(c["iters"], c["thresh"])
    return g
