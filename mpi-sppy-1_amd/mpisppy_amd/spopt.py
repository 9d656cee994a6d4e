"""SPOpt: the batched solve loop and expectations (mirrors mpisppy/spopt.py).

``solve_loop`` keeps the reference's signature (spopt.py:226-233) but replaces the
per-scenario ``solve_one`` + SolverFactory plugin call (spopt.py:85-223) with ONE
``phgpu_solve`` over all local scenarios.  Solver selection is by ``solver_name``
(cfg_vanilla.py:43 -> spopt.py:844): this engine answers to ``"mi355x_pdhg"``
(aliases below).  ``iter0_solver_options`` / ``iterk_solver_options`` keys are the
fields of ``phgpu_options`` (include/phgpu.h).

Per-scenario extension hooks ``pre_solve`` / ``post_solve`` (spopt.py:146-147, 220-221)
bracket the batched solve: all local scenarios' ``pre_solve`` before the launch, all
``post_solve`` after it (solutions loaded, one ``ScenarioResults`` each).
"""
import time
import numpy as np

from . import _lib
from .spbase import SPBase
from .engine import PHEngine
from .extensions.extension import overrides

_TERMINATION = {_lib.OPTIMAL: "optimal", _lib.ITER_LIMIT: "maxIterations",
                _lib.PRIMAL_INFEASIBLE: "infeasible", _lib.DUAL_INFEASIBLE: "unbounded"}


class ScenarioResults:
    """What ``post_solve`` gets for one scenario, in the shape of the Pyomo results the
    reference passes (spopt.py:165-206): ``solver.termination_condition`` /
    ``solver.status``, ``Problem[0].Lower_bound`` / ``Upper_bound`` (the Lagrangian bound
    and the objective of the solve, swapped for a maximisation), plus the engine's own
    ``status`` code and ``iterations``."""

    class _Solver:
        def __init__(self, tc):
            self.termination_condition = tc
            self.status = "ok" if tc in ("optimal", "maxIterations") else "warning"

    class _Problem:
        def __init__(self, lo, up):
            self.Lower_bound = lo
            self.Upper_bound = up

    def __init__(self, status, obj, bound, iterations, sense=1):
        self.status = int(status)
        self.iterations = int(iterations)
        self.solver = self._Solver(_TERMINATION.get(self.status, "error"))
        lo, up = (bound, obj) if sense > 0 else (obj, bound)
        self.Problem = [self._Problem(float(lo), float(up))]
        self.solution = _SolutionSet([self] if self.status in (_lib.OPTIMAL, _lib.ITER_LIMIT) else [])


class _SolutionSet(list):
    """``results.solution`` of a Pyomo results object: indexable and callable
    (``results.solution(0)``); empty for an infeasible / unbounded solve."""

    def __call__(self, i=0):
        return self[i]


class ScenarioView:
    """The subproblem handed to ``pre_solve`` / ``post_solve`` when the scenarios were
    built by a ``batch_creator`` (no per-scenario models): its name, its index in the local
    batch and, after the solve, its x."""

    def __init__(self, opt, k, name):
        self._opt, self.index, self.name = opt, k, name
        self._name = name

    @property
    def x(self):
        return self._opt.engine.host("x")[self.index]

class Bundle:
    """A bundle as a subproblem (spopt.py:805-836): the extensive form of ``scen_list`` with the
    probabilities p_s / ``_mpisppy_probability``.  No model of it is built: it is the local
    scenarios ``first`` .. ``last`` - 1 of the batch, one segment of the device's segmented
    interior point.  After a solve: ``x`` [scenarios, n]."""

    def __init__(self, opt, name, scen_list, first, last, prob):
        self._opt, self.name, self._name = opt, name, name
        self.scen_list = list(scen_list)
        self.first, self.last = int(first), int(last)
        self._mpisppy_probability = float(prob)

    @property
    def x(self):
        return self._opt.engine.host("x")[self.first:self.last]


SOLVER_NAMES = ("mi355x_pdhg", "phgpu", "mi355x")
DEFAULT_BUNDLE_TOL = 1e-10       # 1e-8 leaves W 1.5e-4 off on farmer, 1e-12 is below what fp64 reaches
# a bundle is over when, besides, the predictor's step of its nonants is at most this times 1 + max |z|:
# the residuals bound the objective, not z; 1e-8 keeps z of farmer (up to 250 per crop)
# within 2.5e-6, a quarter of the project's 1e-5 on W and x̄
DEFAULT_BUNDLE_STEP_TOL = 1e-8
DEFAULT_BUNDLE_MAX_ITER = 100


# phgpu_options structs by their settings (built once: the PH loop solves with the same
# options every iteration)
_OPTIONS_CACHE = {}

class SPOpt(SPBase):
    def __init__(self, options, all_scenario_names, scenario_creator, scenario_denouement=None,
                 all_nodenames=None, mpicomm=None, extensions=None, extension_kwargs=None,
                 scenario_creator_kwargs=None, variable_probability=None, E1_tolerance=1e-5):
        super().__init__(options, all_scenario_names, scenario_creator, scenario_denouement,
                         all_nodenames, mpicomm, scenario_creator_kwargs, variable_probability,
                         E1_tolerance)
        self.extensions = extensions
        self.extension_kwargs = extension_kwargs
        if extensions is not None:
            self.extobject = extensions(self) if extension_kwargs is None else extensions(self, **extension_kwargs)
        self.spcomm = None
        self.engine = None
        self._fixed = False
        self._bundles = None
        if self.bundling:
            self.subproblem_creation()
        self.solve_times = []
        self.pdhg_iters = []

    # spopt.py:839-868
    def _create_solvers(self):
        sname = self.options.get("solver_name")
        if sname not in SOLVER_NAMES:
            raise RuntimeError(f"solver_name {sname!r} is not served by this engine; use one of {SOLVER_NAMES}")
        if self.engine is None:
            self.engine = PHEngine(self.batch, device=self.options.get("device"), comm=self.mpicomm,
                                   node_names=self.node_names, shared=self.options.get("shared_matrix"))
            self.engine.scen_offset = int(self._rank_slices[self.cylinder_rank][0])
            if getattr(self, "var_prob", None) is not None:
                self.engine.set_nonant_probs(self.var_prob)
            if self.options.get("ipm_tuning"):
                # a model's interior-point constants (e.g. examples/aircond.py IPM_TUNING)
                self.engine.set_ipm_tuning(self.options["ipm_tuning"])
            if self.bundling:
                self._bundle_setup()

    # spopt.py:805-836
    def subproblem_creation(self, verbose=False):
        """``local_subproblems`` keyed ``rank{r}bundle{b}``: this rank's bundles, each a contiguous
        slice of the local scenarios."""
        if self.multistage or self.batch.depth != 1:
            raise RuntimeError(f"bundles serve two-stage problems only ({len(self.all_nodenames)} tree nodes)")
        if self.options.get("shared_matrix"):
            raise NotImplementedError("bundles: a shared-matrix handle has no per-scenario matrix to factor")
        self.bundle_tol = float(self.options.get("bundle_tol", DEFAULT_BUNDLE_TOL))
        self.bundle_step_tol = float(self.options.get("bundle_step_tol", DEFAULT_BUNDLE_STEP_TOL))
        self.bundle_max_iter = int(self.options.get("bundle_max_iter", DEFAULT_BUNDLE_MAX_ITER))
        if not self.bundle_tol > 0.0 or not self.bundle_step_tol > 0.0 or self.bundle_max_iter < 0:
            raise ValueError(f"bundle_tol = {self.bundle_tol} and bundle_step_tol = {self.bundle_step_tol} must be positive "
                             f"and bundle_max_iter = {self.bundle_max_iter} non-negative")
        r = self.cylinder_rank
        self._bundles, first = {}, 0
        for b, names in self.names_in_bundles[r].items():
            if names != self.local_scenario_names[first:first + len(names)]:
                raise RuntimeError(f"bundle {b} of rank {r} is not a contiguous slice of the rank's scenarios")
            last = first + len(names)
            self._bundles[f"rank{r}bundle{b}"] = Bundle(self, f"rank{r}bundle{b}", names, first, last,
                                                        self.batch.prob[first:last].sum())
            first = last
        self.bundle_ipm_iters = []     # per solve_loop: (max, mean) interior-point iterations over the bundles

    def _bundle_data(self):
        """What phgpu_bundle_init takes, after the checks of what the segmented interior point does
        not serve (those of opt/sc.py, per bundle)."""
        from .opt.lshaped import first_stage_rows
        b = self.batch
        if b.nn > 64 or b.m > 64:
            raise NotImplementedError(f"bundles: the interior point serves nn <= 64 and m <= 64 (nn {b.nn}, m {b.m})")
        rows, _, lo, hi, _ = first_stage_rows(b)
        for i, l, u in zip(rows, lo, hi):
            if l == u:
                raise NotImplementedError(f"bundles: row {i} has only nonant columns and equal sides [{l}, {u}]: its block of "
                                          f"the scenario's normal matrix has no interior")
        nc = np.asarray(b.nonant_col, dtype=np.int64)
        oth = np.setdiff1d(np.arange(b.n), nc)
        ranged = b.rl < b.ru
        G = len(self._bundles)
        seg = np.zeros(G + 1, dtype=np.int32)
        zlb, zub, ncomp, cmax = np.zeros((G, b.nn)), np.zeros((G, b.nn)), np.zeros(G), np.zeros(G)
        for g, (name, bd) in enumerate(self._bundles.items()):
            sl = slice(bd.first, bd.last)
            seg[g + 1] = bd.last
            zlb[g], zub[g] = b.lb[sl][:, nc].max(axis=0), b.ub[sl][:, nc].min(axis=0)
            if not np.all(zlb[g] < zub[g]):
                k = int(np.nonzero(~(zlb[g] < zub[g]))[0][0])
                raise NotImplementedError(f"bundle {name}: nonant {k} has the bounds [{zlb[g, k]}, {zub[g, k]}] over its "
                                          f"scenarios: a fixed first-stage column leaves the interior point no interior")
            ncomp[g] = (np.isfinite(b.lb[sl][:, oth]).sum() + np.isfinite(b.ub[sl][:, oth]).sum()
                        + (np.isfinite(b.rl[sl]) & ranged[sl]).sum() + (np.isfinite(b.ru[sl]) & ranged[sl]).sum()
                        + np.isfinite(zlb[g]).sum() + np.isfinite(zub[g]).sum())
            cmax[g] = np.abs(b.c[sl]).max(initial=0.0)
        return seg, zlb, zub, ncomp, cmax, bool(np.any(b.q))

    def _bundle_setup(self):
        e = self.engine
        if e.shared:
            raise NotImplementedError("bundles: a shared-matrix handle has no per-scenario matrix to factor")
        data = self._bundle_data()
        e.bundle_init(*data[:5], self.bundle_tol, self.bundle_step_tol, data[5])

    def _bundle_solve(self, dtiming):
        """Every bundle's extensive form at once (engine.bundle_solve), under the engine's W_on /
        prox_on: Iter0's LPs, the PH QPs and the Lagrangian pass alike."""
        r = self.engine.bundle_solve(self.bundle_max_iter)
        self.bundle_last = r
        if dtiming or self.options.get("record_pdhg_iters", False):
            it = self.engine.iters.cpu().numpy()[[bd.first for bd in self._bundles.values()]]
            self.pdhg_iters.append((int(it.max()), float(it.mean())))
            self.bundle_ipm_iters.append(self.pdhg_iters[-1])
        if r["open"] > 0 or r["stopped"] > 0:
            self._bundle_gripe()

    def _bundle_gripe(self):
        st, it = self.engine.host("status"), self.engine.host("iters")
        for name, bd in self._bundles.items():
            if st[bd.first] != _lib.OPTIMAL:
                self.bundle_griped = getattr(self, "bundle_griped", 0) + 1     # bundle solves griped so far
                print(f"Solve of bundle {name} ended without optimality after {int(it[bd.first])} interior-point "
                      f"iterations (status {int(st[bd.first])}, bundle_tol {self.bundle_tol:g}, bundle_max_iter "
                      f"{self.bundle_max_iter}); its nonants are the last finite iterate's", flush=True)

    # options the reference's cfg_vanilla.shared_options passes to MIP/LP plugins
    # (threads, mipgap; cfg_vanilla.py:41-62) or that only drive plugin output (Tee):
    # meaningless for PDHG, accepted and ignored; any other unknown key raises
    FOREIGN_SOLVER_OPTIONS = ("threads", "mipgap", "Tee", "tee", "timelimit", "time_limit")

    @staticmethod
    def _to_phgpu_options(solver_options):
        so = {k: v for k, v in (solver_options or {}).items() if k not in SPOpt.FOREIGN_SOLVER_OPTIONS}
        key = tuple(sorted(so.items()))
        o = _OPTIONS_CACHE.get(key)
        if o is None:
            o = _OPTIONS_CACHE[key] = _lib.default_options(**so)
        return o

    # spopt.py:226-307
    def solve_loop(self, solver_options=None, use_scenarios_not_subproblems=False, dtiming=False,
                   gripe=False, disable_pyomo_signal_handling=False, tee=False, verbose=False,
                   warm_start=True, speculative=False):
        if self.extensions is not None and hasattr(self.extobject, "pre_solve_loop"):
            self.extobject.pre_solve_loop()
        ext = self.extobject if self.extensions is not None else None
        pre, post = overrides(ext, "pre_solve"), overrides(ext, "post_solve")
        if pre:
            for sp in self._subproblems():
                ext.pre_solve(sp)
        t0 = time.perf_counter()
        if self.bundling:
            if speculative:
                raise NotImplementedError("the speculative solve is not served with bundles: a bundle solve reads the "
                                          "host's record every interior-point iteration")
            self._bundle_solve(dtiming)
            gripe = False            # (_bundle_solve gripes by bundle name)
        else:
            self.engine.solve(self._to_phgpu_options(solver_options), warm=warm_start, speculative=speculative)
        if not self.bundling and (dtiming or self.options.get("record_pdhg_iters", False)):
            import torch
            torch.cuda.synchronize()
            it = self.engine.iters.cpu().numpy()
            self.pdhg_iters.append((int(it.max()), float(it.mean())))
        self.solve_times.append(time.perf_counter() - t0)
        if post:
            self._post_solve_hooks(ext)
        if self.extensions is not None and hasattr(self.extobject, "post_solve_loop"):
            self.extobject.post_solve_loop()
        if dtiming and self.cylinder_rank == 0:
            print("Batched solve time (seconds): %4.4f  PDHG iters max/mean %d/%.1f"
                  % (self.solve_times[-1], *self.pdhg_iters[-1]))
        if gripe == "deferred":
            # iterk_loop: the count is read at the next host synchronisation (the conv
            # readback of the next PH iteration, or the end of the loop), not here
            self.engine.count_not_optimal_async()
            self._gripe_pending = True
        elif gripe and self.engine.count_not_optimal() > 0:
            self._gripe_print()

    def _subproblems(self):
        """Per-scenario models when the creator built them, else ScenarioViews."""
        if self.bundling:
            return list(self._bundles.values())
        if self.local_scenarios:
            return [self.local_scenarios[nm] for nm in self.local_scenario_names]
        return [ScenarioView(self, k, nm) for k, nm in enumerate(self.local_scenario_names)]

    def _post_solve_hooks(self, ext):
        # (a speculative solve is never bracketed: PHBase._speculate is off with these hooks)
        self.load_solutions_to_models()
        st, obj, bd, it = (self.engine.host(k) for k in ("status", "obj", "bound", "iters"))
        sense = self.batch.sense
        # spopt.py:165-221: the results object with termination 'infeasible' / 'unbounded'
        # (and no solution) for a certified failure; None only where the solver raised,
        # which a batched launch does not do per scenario
        if self.bundling:
            # a bundle's objective is sum_s (p_s / p_B) of its scenarios'; status and iterations are the bundle's
            p = self.batch.prob
            for sp in self._subproblems():
                sl, k = slice(sp.first, sp.last), sp.first
                w = p[sl] / sp._mpisppy_probability
                ext.post_solve(sp, ScenarioResults(st[k], sense * float(w @ obj[sl]), sense * float(w @ bd[sl]), it[k], sense))
            return
        for k, sp in enumerate(self._subproblems()):
            ext.post_solve(sp, ScenarioResults(st[k], sense * obj[k], sense * bd[k], it[k], sense))

    def gripe_report(self):
        """The gripe of a solve_loop(gripe="deferred") (spopt.py:284-294 prints it right
        after the solves; here it comes at the next synchronisation)."""
        if getattr(self, "_gripe_pending", False):
            self._gripe_pending = False
            if self.engine.pending_not_optimal() > 0:
                self._gripe_print()

    def _gripe_print(self):
        st = self.engine.status.cpu().numpy()
        bad = np.nonzero((st != _lib.OPTIMAL) & (st != _lib.ITER_LIMIT))[0]
        for k in bad[:10]:
            print(f"Solve failed for scenario {self.batch.names[k]} (status {st[k]})")
        lim = np.nonzero(st == _lib.ITER_LIMIT)[0]
        if len(lim) and self.cylinder_rank == 0:
            print(f"WARNING: {len(lim)} scenario(s) hit the PDHG iteration limit "
                  f"(e.g. {self.batch.names[lim[0]]}); their solutions are approximate")

    # spopt.py:310-343 ("weighted, proxed" objective, phbase.py:991)
    def Eobjective(self, verbose=False):
        e = self.engine.expectations()
        return self.batch.sense * e[0]

    # spopt.py:346-391
    def Ebound(self, verbose=False, extra_sum_terms=None):
        e = self.engine.expectations()
        b = self.batch.sense * e[1]
        if extra_sum_terms is not None:
            import torch
            t = torch.tensor(list(extra_sum_terms), dtype=torch.float64, device=self.engine.device)
            self.mpicomm.allreduce_sum_(t)
            return b, t.cpu().numpy()
        return b

    # spopt.py:394-408
    def _update_E1(self):
        self.E1 = self.engine.expectations()[2]

    # spopt.py:411-439
    def feas_prob(self):
        return self.engine.expectations()[3]

    def infeas_prob(self):
        e = self.engine.expectations()
        return e[2] - e[3]

    # -- fixing the nonants (Xhat_Eval, XhatBase._try_one, and the xhat extensions of a PH object)
    def _node_table(self, cache):
        """dict node name -> values (spopt.py:557-592 cache) -> device [num_nodes, nlen_max]."""
        import torch
        e = self.engine
        tab = np.zeros((e.num_nodes, e.nlen_max))
        for g, nd in enumerate(e.node_names):
            if nd in cache and cache[nd] is not None:
                v = np.asarray(cache[nd], dtype=np.float64).reshape(-1)
                tab[g, :len(v)] = v
        return torch.from_numpy(tab).to(e.device)

    # spopt.py:557-592
    def _fix_nonants(self, cache):
        """Fix the nonants of all local scenarios: ``cache`` is {node name: values} or a
        device [num_nodes, nlen_max] tensor (global node order)."""
        import torch
        if self.bundling:
            # (a bundle solve reads the problem's own bounds and z's, set once: fixed nonants would be
            # ignored and the free bundle's objective reported as the value at the candidate)
            raise NotImplementedError("fixing the nonants (_fix_nonants: the xhat extensions and spokes, Xhat_Eval) is not "
                                      "served with bundles: a fixed column leaves a bundle's interior point no interior")
        tab = cache if torch.is_tensor(cache) else self._node_table(cache)
        self.engine.fix_nonants_by_node(tab)
        self._fixed = True

    # spopt.py:638-660
    def _restore_nonants(self):
        if self.engine is not None and self._fixed:
            self.engine.fix_nonants(None)
        self._fixed = False

    # -- values back into the LinearModels (for denouement / writers)
    def load_solutions_to_models(self):
        if not self.local_scenarios:
            return
        x = self.engine.host("x")  # [S, n]
        for s, nm in enumerate(self.local_scenario_names):
            mdl = self.local_scenarios[nm]
            for j, v in enumerate(mdl.vars):
                v._value = float(x[s, j])
