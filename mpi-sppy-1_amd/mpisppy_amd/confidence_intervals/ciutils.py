"""Utilities of the confidence-interval package (mirrors mpisppy/confidence_intervals/ciutils.py;
DESIGN.md 3.20): the Mak-Morton-Wood gap estimators G and s of [bm2011] section 2 at a candidate
x̂, the xhat files, and a Student-t quantile.  Two-stage problems, and multistage ones
(``EF_mstage``) through ``sample_tree.py``: one free tree extensive form, one conditioned extensive
form per interior stage and the same two batched evaluations.

The reference computes one estimator at a time: an extensive-form solve for the sample problem's
optimum x*, then two Xhat_Eval passes and a host loop over the scenarios (ciutils.py:335-415).
Here ``gap_estimators_batched`` is the hot path: ONE Xhat_Eval over the scenarios of all batches,
one batched solve with every scenario fixed at x̂, one with every scenario fixed at the x* of its
own batch (a [nn, S] table for ``engine.fix_nonants``), and one ``engine.gap_moments`` call
(phgpu_gap_moments) whose host read is the only synchronisation.  ``gap_estimators`` is that
function with one batch.

DEPARTURES from the reference.  x* comes from ``LShapedMethod`` on the batch's scenarios (the
reference solves the extensive form through the amalgamator); ``xstar_solver`` takes a caller's
own, and ``ef_xstar_solver`` makes one that does solve the extensive form (opt/ef.py).  The merged engine holds the probabilities the scenario creator gives each batch (1 / n), so
they sum to the number of batches: every moment is divided by its segment's sum of probabilities,
and no result depends on their common scale.  A scenario that is not solved to optimality in
either solve raises (an estimator over a subset of its sample is not the estimator); the
reference would carry on with whatever the solver left.  ``EF_mstage`` on a model module without
``sample_tree_scen_creator`` raises NotImplementedError naming it (the reference: RuntimeError, from
SampleSubtree's constructor), before ``sample_options`` is looked at.
"""
import importlib
import math
import os
import time

import numpy as np

from .. import global_toc
from ..comm import Comm
from ..sputils import extract_num, number_of_nodes, create_nodenames_from_branching_factors

MINIMIZE, MAXIMIZE = 1, -1          # pyo.minimize, pyo.maximize


# ------------------------------------------------------------------ cfg and module access
class CfgView:
    """A cfg (any object with the reference's option names as attributes, or a mapping) with
    ephemeral overrides: attribute access, ``get``, ``in`` and ``[]``, which is what the model
    modules' ``kw_creator`` and this package read.  Stands in for the reference's ``cfg()`` copy
    followed by ``quick_assign``."""

    def __init__(self, base=None, **over):
        object.__setattr__(self, "_base", base)
        object.__setattr__(self, "_over", dict(over))

    def _lookup(self, name):
        if name in self._over:
            return True, self._over[name]
        b = self._base
        if b is None:
            return False, None
        if isinstance(b, dict):
            return (True, b[name]) if name in b else (False, None)
        if isinstance(b, CfgView):
            return b._lookup(name)
        if hasattr(b, name):
            return True, getattr(b, name)
        try:
            return (True, b[name]) if name in b else (False, None)
        except TypeError:
            return False, None

    def get(self, name, default=None):
        found, v = self._lookup(name)
        return v if found and v is not None else default

    def __contains__(self, name):
        return self._lookup(name)[0]

    def __getitem__(self, name):
        found, v = self._lookup(name)
        if not found:
            raise KeyError(name)
        return v

    def __getattr__(self, name):
        found, v = self._lookup(name)
        if not found:
            raise AttributeError(name)
        return v

    def __setattr__(self, name, value):
        self._over[name] = value

    __setitem__ = __setattr__

    def quick_assign(self, name, domain, value):
        self._over[name] = value

    def __call__(self):
        return CfgView(self)


def model_module(mname):
    """``mname``: a module object or a dotted name."""
    return importlib.import_module(mname) if isinstance(mname, str) else mname


def check_module(m):
    """What amalgamator.check_module_ama asks of a model module."""
    missing = [fct for fct in ("scenario_names_creator", "scenario_creator", "kw_creator", "scenario_denouement")
               if not hasattr(m, fct)]
    if missing:
        raise RuntimeError(f"Module {getattr(m, '__name__', m)} not complete for from_module (missing: {missing})")


# ------------------------------------------------------------------ sample trees (ciutils.py:25-133)
def _prime_factors(n):
    """{prime: multiplicity} of n >= 1, the primes ascending."""
    if n < 1:
        raise ValueError(f"_prime_factors require positive input ({n})")
    out, p = {}, 2
    while p * p <= n:
        while n % p == 0:
            out[p] = out.get(p, 0) + 1
            n //= p
        p += 1 if p == 2 else 2
    if n > 1:
        out[n] = out.get(n, 0) + 1
    return out


def branching_factors_from_numscens(numscens, num_stages):
    """Branching factors of a balanced sample tree with about ``numscens`` leaves: the prime factors
    of the first of numscens, numscens + 1, ... that has at least num_stages - 1 of them, dealt
    round-robin to the stages (ciutils.py:54-84).  None for two stages."""
    if num_stages == 2:
        return None
    k = num_stages - 1
    for i in range(2 ** k):
        pf = _prime_factors(numscens + i) if numscens + i >= 1 else {}
        if sum(pf.values()) >= k:
            facts = [f for f, mult in pf.items() for _ in range(mult)]
            return [int(np.prod(facts[j::k])) for j in range(k)]
    raise RuntimeError("branching_factors_from_numscens is not working correctly.")


def scalable_branching_factors(numscens, ref_branching_factors):
    """Branching factors of a tree with at least ``numscens`` leaves shaped like
    ``ref_branching_factors``, the first stages rounded up first: 233 with [5, 3, 2] gives [10, 6, 4]
    (ciutils.py:86-123)."""
    k = len(ref_branching_factors)
    if numscens < 2 ** k:
        return [2] * k
    mult = (numscens / np.prod(ref_branching_factors)) ** (1 / k)
    new = np.maximum(np.floor(np.array(ref_branching_factors) * mult), 1.0)
    i = 0
    while np.prod(new) < numscens:
        if i == k:
            raise RuntimeError("scalable branching_factors is failing")
        new[i] += 1
        i += 1
    return [int(v) for v in new]


def is_sorted(nodelist):
    """ciutils.py:125-133: a scenario's node list runs ROOT, its child, ... one node per stage."""
    parent = None
    for t, node in enumerate(nodelist):
        if t + 1 != node.stage or node.parent_name != parent:
            raise RuntimeError(f"The node list is not well-constructed: the stage {node.stage} node {node.name} (parent "
                               f"{node.parent_name}) is element {t + 1} of the list, after {parent}")
        parent = node.name


# ------------------------------------------------------------------ xhat files (ciutils.py:135-164)
def _two_stage_only(num_stages):
    if num_stages != 2:
        raise RuntimeError("Only 2-stage is suported to write/read xhat to a file")


def writetxt_xhat(xhat, path="xhat.txt", num_stages=2):
    _two_stage_only(num_stages)
    np.savetxt(path, xhat["ROOT"])


def readtxt_xhat(path="xhat.txt", num_stages=2, delete_file=False):
    _two_stage_only(num_stages)
    xhat = {"ROOT": np.loadtxt(path)}
    if delete_file and Comm().Get_rank() == 0:
        os.remove(path)
    return xhat


def write_xhat(xhat, path="xhat.npy", num_stages=2):
    _two_stage_only(num_stages)
    np.save(path, xhat["ROOT"])


def read_xhat(path="xhat.npy", num_stages=2, delete_file=False):
    _two_stage_only(num_stages)
    xhat = {"ROOT": np.load(path)}
    if delete_file and Comm().Get_rank() == 0:
        os.remove(path)
    return xhat


# ------------------------------------------------------------------ ciutils.py:185-205
def correcting_numeric(G, cfg, relative_error=True, threshold=1e-4, objfct=None):
    """A gap estimate of the wrong sign that is numerically small (below ``threshold``, times
    |objfct| when ``relative_error``) becomes 0; a large one is returned with a warning."""
    sense = CfgView(cfg).get("pyo_opt_sense", MINIMIZE)
    assert sense == MINIMIZE or sense == MAXIMIZE
    if objfct is None:
        raise RuntimeError("We need a value of the objective function to remove numerically small G")
    crit = threshold * abs(objfct) if relative_error else threshold
    if (sense == MINIMIZE and G <= -crit) or (sense == MAXIMIZE and G >= crit):
        print(f"WARNING: The gap estimator is the wrong sign: {G}")
        return G
    return max(0, G) if sense == MINIMIZE else min(0, G)


# ------------------------------------------------------------------ Student-t quantile
def _betacf(a, b, x):
    """The continued fraction of the incomplete beta function (modified Lentz)."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 2000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        de = d * c
        h *= de
        if abs(de - 1.0) <= 3e-16:
            break
    return h


def _betai(a, b, x, xc):
    """Regularised incomplete beta I_x(a, b); ``xc`` = 1 - x, given by the caller so that neither
    end loses digits."""
    if x <= 0.0:
        return 0.0
    if xc <= 0.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log(xc))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, xc) / b


def _t_sf(t, df):
    """P(T > t) for t >= 0."""
    den = df + t * t
    return 0.5 * _betai(0.5 * df, 0.5, df / den, t * t / den)


def t_ppf(q, df):
    """The quantile of Student's t with ``df`` degrees of freedom (scipy.stats.t.ppf without
    scipy): the upper tail 0.5 I_{df/(df+t^2)}(df/2, 1/2) by its continued fraction, inverted by
    a Newton iteration kept inside a bracket."""
    q, df = float(q), float(df)
    if not 0.0 < q < 1.0 or df <= 0.0:
        raise ValueError(f"t_ppf needs 0 < q < 1 and df > 0 (got {q}, {df})")
    if q == 0.5:
        return 0.0
    if q < 0.5:
        return -t_ppf(1.0 - q, df)
    target = 1.0 - q
    lo, hi = 0.0, 1.0
    while _t_sf(hi, df) > target:
        lo, hi = hi, 2.0 * hi
    logc = math.lgamma(0.5 * (df + 1.0)) - math.lgamma(0.5 * df) - 0.5 * math.log(df * math.pi)
    t = 0.5 * (lo + hi)
    for _ in range(200):
        f = _t_sf(t, df) - target
        if f > 0.0:
            lo = t
        else:
            hi = t
        pdf = math.exp(logc - 0.5 * (df + 1.0) * math.log1p(t * t / df))
        tn = t + f / pdf
        if not lo < tn < hi:
            tn = 0.5 * (lo + hi)
        if abs(tn - t) <= 4e-16 * abs(tn):
            return tn
        t = tn
    return t


# ------------------------------------------------------------------ x* of a sample problem
class _Solo(Comm):
    """A one-rank communicator inside a larger world: the x* runs are shared out over the ranks,
    each run on one rank."""

    def __init__(self):
        self.group, self.rank, self.size = None, 0, 1


def _split_solver_options(cfg, solver_options):
    """(L-shaped tol, options of the batched solves) from the caller's solver options, else the
    cfg's ``EF_solver_options``."""
    so = solver_options if solver_options is not None else CfgView(cfg).get("EF_solver_options")
    so = {k: v for k, v in (so or {}).items() if v is not None}
    tol = float(so.pop("tol", 1e-8))
    return tol, so


XSTAR_GAP = 1e-6    # certified relative gap at which a stalled L-shaped run's candidate is taken as x*


def lshaped_xstar(m, scenario_names, scenario_creator_kwargs, solver_name, tol=1e-8, sp_options=None,
                  device=None, max_iter=None, accept_gap=XSTAR_GAP, report=None):
    """The optimum of the sample problem over ``scenario_names`` by the L-shaped method on one
    rank: one eta per scenario up to 32 scenarios, 32 cut groups above that.  Raises when the run
    stops at its iteration limit without converging.  When the master LP cannot be solved any
    further (its interior point stalls on the nearly parallel cuts of the last iterations, DESIGN.md
    3.20), the last candidate is x* if its CERTIFIED relative gap -- its expected cost over the
    sample against the last solved master's outer bound -- is at most ``accept_gap`` (0: never);
    ``report`` (a list) then receives that gap.  Host [nn]."""
    from ..opt.lshaped import LShapedMethod
    opts = {"root_solver": solver_name, "sp_solver": solver_name, "solver_name": solver_name, "tol": tol,
            "max_iter": int(max_iter or 200), "toc": False, "verbose": False, "device": device,
            "sp_solver_options": dict(sp_options or {}), "root_solver_options": {}}
    if hasattr(m, "batch_creator"):
        opts["batch_creator"] = m.batch_creator
    ls = LShapedMethod(opts, scenario_names, m.scenario_creator, scenario_creator_kwargs=scenario_creator_kwargs,
                       mpicomm=_Solo())
    try:
        try:
            ls.lshaped_algorithm()
        except RuntimeError as err:
            if "master was not solved" not in str(err) or not ls.history:
                raise
            q, b = ls.Eobj_at_xhat, ls._LShaped_bound
            gap = ls.batch.sense * (q - b) / max(1.0, abs(q))
            if not gap <= accept_gap:
                raise RuntimeError(f"the L-shaped run for x* over {scenario_names[0]}..{scenario_names[-1]} stalled "
                                   f"with a certified relative gap of {gap:.2e} (accepted: {accept_gap:.1e})") from err
            if report is not None:
                report.append(float(gap))
            return np.array(ls.current_xhat(), dtype=np.float64)
        if not ls.first_stage_solution_available:
            raise RuntimeError(f"the L-shaped run for x* over {scenario_names[0]}..{scenario_names[-1]} stopped at "
                               f"max_iter = {ls.max_iter} without converging (tol {tol})")
        return np.array(ls.current_xhat(), dtype=np.float64)
    finally:
        if ls.engine is not None:
            ls.engine.close()


def ef_xstar_solver(mname, solver_name=None, tol=1e-8, max_iter=100, device=None):
    """A ready-made ``xstar_solver`` for ``gap_estimators`` / ``gap_estimators_batched``: the optimum
    of each sample problem from ``ExtensiveForm`` (opt/ef.py: one interior point on the sample's
    extensive form, LPs and diagonal QPs, no cut groups and no master rounds) instead of the L-shaped method,
    which stays the default.  ``mname``: the model module or its name.  Returns the callable
    (scenario_names, scenario_creator_kwargs) -> x* [ROOT's nonants] (on a multistage model, whose
    kwargs hold ``branching_factors``, the extensive form is that of the whole tree); a solve that does not reach ``tol``
    within ``max_iter`` iterations raises."""
    from ..opt.ef import ExtensiveForm
    from ..spopt import SOLVER_NAMES
    from ..sputils import create_nodenames_from_branching_factors
    m = model_module(mname) if isinstance(mname, str) else mname

    def solve(scenario_names, scenario_creator_kwargs):
        opts = {"solver": solver_name or SOLVER_NAMES[0], "tol": tol, "max_iter": max_iter, "toc": False,
                "device": device}
        if hasattr(m, "batch_creator"):
            opts["batch_creator"] = m.batch_creator
        bfs = (scenario_creator_kwargs or {}).get("branching_factors")     # a multistage model names its tree by them
        nodenames = create_nodenames_from_branching_factors(list(bfs)) if bfs is not None and len(bfs) > 1 else None
        ef = ExtensiveForm(opts, scenario_names, m.scenario_creator, scenario_creator_kwargs=scenario_creator_kwargs,
                           all_nodenames=nodenames)
        try:
            res = ef.solve_extensive_form()
            if res.solver.termination_condition != "optimal":
                raise RuntimeError(f"the extensive form over {scenario_names[0]}..{scenario_names[-1]} was not solved "
                                   f"to tol {tol} in {max_iter} iterations")
            return np.array(ef.root_nonants(), dtype=np.float64)
        finally:
            if ef.engine is not None:
                ef.engine.close()
    return solve


# ------------------------------------------------------------------ the estimators
def gap_estimators_batched(xhat_one, mname, num_batches, batch_size, start, ArRP=1, cfg=None,
                           scenario_denouement=None, solver_name=None, solver_options=None, verbose=False,
                           mpicomm=None, xstar_solver=None, scenario_names=None, info=None):
    """G and s of ``num_batches`` batches of ``batch_size`` scenarios (scenario numbers from
    ``start``, or ``scenario_names``) at the candidate ``xhat_one`` ({"ROOT": values}): arrays
    G [num_batches], s [num_batches] and the advanced seed, from two batched solves and one host
    read whatever ``num_batches`` is (module docstring).  ``ArRP`` > 1 pools each batch's
    estimators from ArRP sub-batches, each with its own x*, as ciutils.py:285-313 does.
    ``xstar_solver``: a callable (scenario_names, scenario_creator_kwargs) -> x* [nn]; None: the
    L-shaped method.  ``info``: a dict that receives "solves" (the batched solves of the merged
    Xhat_Eval), "xstar_certified_gaps" (``lshaped_xstar``'s certificates, if a run of this rank needed
    one) and, when it holds ``time_phases`` = True, "seconds" spent in "xstar", "solves" and "moments"
    (each phase then ends with a device synchronisation)."""
    import torch
    from ..utils.xhat_eval import Xhat_Eval
    m = model_module(mname)
    check_module(m)
    B, n, ArRP = int(num_batches), int(batch_size), int(ArRP)
    if B < 1 or n < 1:
        raise RuntimeError(f"gap_estimators_batched needs num_batches >= 1 and batch_size >= 1 (got {B}, {n})")
    if n % ArRP != 0:
        raise RuntimeWarning(f"You put as an input a number of scenarios which is not a mutliple of {ArRP}.")
    names = list(scenario_names) if scenario_names is not None else m.scenario_names_creator(B * n, start=start)
    if len(names) != B * n:
        raise RuntimeError(f"{len(names)} scenario names for {B} batches of {n}")
    lcfg = CfgView(cfg, num_scens=n, _mpisppy_probability=1 / n)
    kw = m.kw_creator(lcfg)
    comm = mpicomm if mpicomm is not None else Comm()
    if solver_name is None:
        solver_name = lcfg.get("EF_solver_name", lcfg.get("solver_name"))
    tol, sp_options = _split_solver_options(lcfg, solver_options)
    device = lcfg.get("device")
    sub, nseg = n // ArRP, B * ArRP
    tick = time.perf_counter()
    timing = info.setdefault("seconds", {}) if info is not None and info.get("time_phases") else None

    def lap(key):
        nonlocal tick
        if timing is not None:
            torch.cuda.synchronize()
            timing[key] = timing.get(key, 0.0) + time.perf_counter() - tick
        tick = time.perf_counter()

    # x* of every segment: the runs are shared out over the ranks, each on one rank, so the
    # values do not depend on the number of ranks
    stalled = []
    if xstar_solver is None:
        def xstar_solver(seg_names, seg_kw):
            return lshaped_xstar(m, seg_names, seg_kw, solver_name, tol=tol, sp_options=sp_options, device=device,
                                 max_iter=lcfg.get("lshaped_max_iter"),
                                 accept_gap=lcfg.get("xstar_gap", XSTAR_GAP), report=stalled)
    mine = {j: np.asarray(xstar_solver(names[j * sub:(j + 1) * sub], kw), dtype=np.float64)
            for j in range(comm.Get_rank(), nseg, comm.Get_size())}
    xstars = {}
    for part in comm.allgather_object(mine):
        xstars.update(part)
    if info is not None:
        info["xstar_certified_gaps"] = stalled      # (this rank's runs that ended on the certificate)
    lap("xstar")

    ev = Xhat_Eval({"solver_name": solver_name, "toc": False, "verbose": False, "device": device,
                    "solver_options": sp_options,
                    **({"batch_creator": m.batch_creator} if hasattr(m, "batch_creator") else {})},
                   names, m.scenario_creator, scenario_denouement, scenario_creator_kwargs=kw, mpicomm=comm)
    try:
        ev._lazy_create_solvers()
        e = ev.engine
        if ev.multistage or ev.batch.depth != 1:
            raise NotImplementedError("multistage sampling (sample_tree.py, EF_mstage) is not served: two-stage only")
        xstar_tab = torch.from_numpy(np.stack([xstars[j] for j in range(nseg)], axis=1)).to(e.device)   # [nn, nseg]
        if tuple(xstar_tab.shape) != (e.nn, nseg):
            raise RuntimeError(f"x* has {xstar_tab.shape[0]} entries, the model {e.nn} nonants")
        ev._fix_nonants({"ROOT": np.asarray(xhat_one["ROOT"], dtype=np.float64)})
        ev.solve_loop(solver_options=sp_options)
        f_hat, st_hat = e.obj.clone(), e.status.clone()
        seg_of = (torch.arange(e.S, device=e.device) + e.scen_offset) // sub
        e.fix_nonants(xstar_tab.index_select(1, seg_of))
        ev.solve_loop(solver_options=sp_options)
        lap("solves")
        M = e.gap_moments(np.arange(nseg + 1, dtype=np.int64) * sub, f_hat, st_hat, e.obj, e.status)
        lap("moments")
        sense = ev.batch.sense
        if info is not None:
            info["solves"] = len(ev.solve_times)
    finally:
        if ev.engine is not None:
            ev.engine.close()
    bad = np.nonzero(M[:, 6] > 0)[0]
    if len(bad):
        j = int(bad[0])
        raise RuntimeError(f"batch {j // ArRP} (scenarios {names[j * sub]}..{names[(j + 1) * sub - 1]}): "
                           f"{int(M[j, 6])} scenario(s) were not solved to optimality at the candidate or at x*; "
                           f"the estimator needs its whole sample")
    est = moments_to_estimators(M, sense, lcfg)
    G = est["G"].reshape(B, ArRP).mean(axis=1)
    if ArRP > 1:
        s = np.linalg.norm(est["s"].reshape(B, ArRP), axis=1) / np.sqrt(sub)
    else:
        s = est["s"]
    if verbose and comm.Get_rank() == 0:
        for b in range(B):
            global_toc(f"G = {G[b]} s = {s[b]} for the batch {b}")
    first = extract_num(names[0]) if scenario_names is not None else int(start)
    return {"G": G, "s": s, "seed": first + B * n,
            "zhat": est["zhat"].reshape(B, ArRP).mean(axis=1), "zstar": est["zstar"].reshape(B, ArRP).mean(axis=1)}


def moments_to_estimators(M, sense, cfg):
    """Rows of ``engine.gap_moments`` -> per-segment G, s, ẑ(x̂), ẑ(x*) (ciutils.py:408-424), every
    moment divided by the segment's sum of probabilities."""
    sp = M[:, 0]
    G = sense * M[:, 2] / sp
    ssq = M[:, 3] / sp
    psq = M[:, 1] / (sp * sp)
    s = np.sqrt(np.maximum((ssq - G * G) / (1.0 - psq), 0.0))        # unbiased sample variance
    zhat, zstar = sense * M[:, 4] / sp, sense * M[:, 5] / sp
    lcfg = CfgView(cfg)
    if "pyo_opt_sense" not in lcfg:
        lcfg = CfgView(cfg, pyo_opt_sense=MINIMIZE if sense > 0 else MAXIMIZE)
    G = np.array([correcting_numeric(G[j], lcfg, objfct=zhat[j], relative_error=bool(abs(zstar[j]) > 1))
                  for j in range(len(G))], dtype=np.float64)
    return {"G": G, "s": s, "zhat": zhat, "zstar": zstar}


def gap_estimators(xhat_one, mname, solving_type="EF_2stage", scenario_names=None, sample_options=None, ArRP=1,
                   cfg=None, scenario_denouement=None, solver_name=None, solver_options=None, verbose=False,
                   mpicomm=None, xstar_solver=None, info=None):
    """ciutils.py:208-427: {"G", "s", "seed"} at ``xhat_one`` over ``scenario_names``; with ArRP > 1
    pooled from ArRP sub-samples.  ``gap_estimators_batched`` with one batch."""
    if solving_type not in ("EF_2stage", "EF_mstage"):
        raise RuntimeError("Only EF solve for the approximate problem is supported yet.")
    if solving_type == "EF_mstage":
        return _gap_estimators_mstage(xhat_one, mname, sample_options, ArRP, cfg, scenario_denouement, solver_name,
                                      solver_options, verbose, mpicomm, info)
    if not scenario_names:
        raise RuntimeError("gap_estimators needs scenario_names for a two-stage problem")
    names = list(scenario_names)
    r = gap_estimators_batched(xhat_one, mname, 1, len(names), extract_num(names[0]), ArRP=ArRP, cfg=cfg,
                               scenario_denouement=scenario_denouement, solver_name=solver_name,
                               solver_options=solver_options, verbose=verbose, mpicomm=mpicomm,
                               xstar_solver=xstar_solver, scenario_names=names, info=info)
    return {"G": float(r["G"][0]), "s": float(r["s"][0]), "seed": r["seed"]}


def _gap_estimators_mstage(xhat_one, mname, sample_options, ArRP, cfg, scenario_denouement, solver_name, solver_options,
                           verbose, mpicomm, info):
    """ciutils.py:319-427 for ``EF_mstage``: the sample tree at ``seed`` and its free extensive form
    (zn_star, xstars), ``walking_tree_xhats`` from ``xhat_one["ROOT"]`` with the seed advanced past
    the sample tree, then Xhat_Eval over the sample tree at xhats and at xstars and the moments of
    the two objective arrays in one ``engine.gap_moments`` read.  ``info`` (a dict) receives
    "iterations" {"free": n, "conditioned": [n per stage]}, "seconds" {"free", "conditioned",
    "evaluations"}, "xhats", "zn_star" and the per-scenario objective arrays "f_hat", "f_star"
    (host, the model's sense)."""
    import torch
    from ..utils.xhat_eval import Xhat_Eval
    from . import sample_tree
    m = model_module(mname)
    if not hasattr(m, "sample_tree_scen_creator"):
        raise NotImplementedError(f"EF_mstage needs a model module with sample_tree_scen_creator (sample_tree.py); "
                                  f"{getattr(m, '__name__', m)} has none")
    check_module(m)
    try:
        branching_factors = list(sample_options["branching_factors"])
        start = int(sample_options["seed"])
    except (TypeError, KeyError):
        raise RuntimeError("For multistage problems, sample_options must be a dict with branching_factors and seed "
                           "attributes.") from None
    if ArRP > 1:
        raise RuntimeError("Pooled estimators are not supported for multistage problems yet.")
    lcfg = CfgView(cfg)
    if solver_name is None:
        solver_name = lcfg.get("EF_solver_name", lcfg.get("solver_name"))
    _, sp_options = _split_solver_options(lcfg, solver_options)
    secs = {}
    tick = time.perf_counter()

    def lap(key):
        nonlocal tick
        torch.cuda.synchronize()
        secs[key] = secs.get(key, 0.0) + time.perf_counter() - tick
        tick = time.perf_counter()

    samp_tree = sample_tree.SampleSubtree(m, [], None, 1, branching_factors, start, cfg, solver_name, solver_options)
    ev = None
    try:
        samp_tree.run()
        lap("free")
        start += number_of_nodes(branching_factors)
        zn_star = samp_tree.best_outer_bound
        xstars = {nd: np.array(v, dtype=np.float64) for nd, v in samp_tree.ef.tree_nonants()}
        walk = {}
        xhats, start = sample_tree.walking_tree_xhats(m, dict(samp_tree.ef.scenarios()), xhat_one["ROOT"], branching_factors,
                                                      start, cfg, solver_name=solver_name, solver_options=solver_options,
                                                      info=walk)
        lap("conditioned")
        nodenames = create_nodenames_from_branching_factors(branching_factors) if len(branching_factors) > 1 else None
        ev = Xhat_Eval({"solver_name": solver_name, "toc": False, "verbose": False, "device": lcfg.get("device"),
                        "solver_options": sp_options}, samp_tree.scenario_names, samp_tree.scenario_creator,
                       scenario_denouement, scenario_creator_kwargs=samp_tree.kwargs, all_nodenames=nodenames, mpicomm=mpicomm)
        ev._lazy_create_solvers()
        e = ev.engine
        ev._fix_nonants(xhats)
        ev.solve_loop(solver_options=sp_options)
        f_hat, st_hat = e.obj.clone(), e.status.clone()
        ev._fix_nonants(xstars)
        ev.solve_loop(solver_options=sp_options)
        M = e.gap_moments(np.array([0, len(samp_tree.scenario_names)], dtype=np.int64), f_hat, st_hat, e.obj, e.status)
        sense = ev.batch.sense
        if info is not None:
            info["f_hat"], info["f_star"] = sense * f_hat.cpu().numpy(), sense * e.obj.cpu().numpy()
        lap("evaluations")
    finally:
        samp_tree.close()
        if ev is not None and ev.engine is not None:
            ev.engine.close()
    if M[0, 6] > 0:
        raise RuntimeError(f"{int(M[0, 6])} scenario(s) of the sample tree were not solved to optimality at the policy or at "
                           f"x*; the estimator needs its whole sample")
    est = moments_to_estimators(M, sense, lcfg)      # (G, s with 1 - sum p^2, correcting_numeric: as two-stage)
    G, s = float(est["G"][0]), float(est["s"][0])
    if info is not None:
        info.update({"iterations": {"free": samp_tree.ef.iterations, "conditioned": walk.get("iterations", [])},
                     "seconds": secs, "xhats": xhats, "zn_star": zn_star, "walk": walk})
    if verbose and (mpicomm is None or mpicomm.Get_rank() == 0):
        global_toc(f"G = {G} s = {s}")
    return {"G": G, "s": s, "seed": start}
