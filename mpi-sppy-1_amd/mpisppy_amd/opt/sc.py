"""SchurComplement: the extensive form by one interior point over all scenarios (mirrors
mpisppy/opt/sc.py).

Same constructor as the reference and ``solve()``.  The reference hands the scenarios' blocks to
parapint's Schur-complement interior point over MPI; here the whole method runs on the device
(phgpu_ef_*, include/phgpu.h): a lane per scenario factors its own block, the only coupling is the
nn x nn system in the ROOT nonants, and every rank solves that system from the same all-reduced
bits.  Two-stage continuous problems (LPs and diagonal QPs; a multistage tree is ``ExtensiveForm``'s,
opt/ef.py, and is refused here as the reference's sc.py has one set of linking variables),
minimisation internally; a
maximisation model is negated as everywhere else.  Per iteration, one read of pinned memory.

``options`` is a dict: ``tol`` (relative KKT tolerance, default 1e-8), ``max_iter`` (default 100),
``device``, ``solver_name`` (one of ``spopt.SOLVER_NAMES``; default the first), ``verbose``.

DEPARTURES from the reference.  ``SCOptions`` objects and a caller's linear solver are not taken
(there is no linear-solver plug-in to choose).  Refused with the reason: multistage trees
(RuntimeError), bundles (ValueError, as in the reference), a shared-matrix handle, a nonant whose
tightest bounds over the scenarios coincide, and a row whose columns are all nonants and whose
sides are equal (its block of the scenario's normal matrix has no interior) -- the last three
NotImplementedError.  After ``solve()`` the engine's x, y, obj, bound and status hold the
extensive form's solution per scenario, with the nonants bitwise equal over the scenarios.
"""
import math
import time

import numpy as np
import torch

from ..spopt import SPOpt, SOLVER_NAMES
from .lshaped import first_stage_rows

DEFAULT_TOL = 1e-8
DEFAULT_MAX_ITER = 100


class SchurComplement(SPOpt):
    # the reference's sc.py couples the blocks through ONE set of linking variables; the subclass
    # that eliminates along a scenario tree (opt/ef.py) says so here
    _serves_trees = False

    # sc.py:59-87
    def __init__(self, options, all_scenario_names, scenario_creator, scenario_creator_kwargs=None,
                 all_nodenames=None, mpicomm=None, model_name=None, suppress_warnings=False):
        options = dict(options or {})
        if options.get("bundles_per_rank", 0):
            raise ValueError("The Schur-Complement method does not support bundling")        # sc.py:76-77
        options.setdefault("solver_name", options.get("solver", SOLVER_NAMES[0]))
        options.setdefault("toc", False)
        super().__init__(options, all_scenario_names, scenario_creator, all_nodenames=all_nodenames, mpicomm=mpicomm,
                         scenario_creator_kwargs=scenario_creator_kwargs)
        self._tree = self.multistage or self.batch.depth != 1
        if self._tree and not self._serves_trees:
            raise RuntimeError("the Schur-complement interior point serves two-stage problems only "
                               f"({len(self.all_nodenames)} tree nodes)")
        if options.get("shared_matrix"):
            raise NotImplementedError("a shared-matrix handle has no per-scenario matrix to factor")
        self.model_name = model_name
        self.tol = float(options.get("tol", DEFAULT_TOL))
        self.max_iter = int(options.get("max_iter", DEFAULT_MAX_ITER))
        if not self.tol > 0.0 or self.max_iter < 0:
            raise ValueError(f"tol = {self.tol} must be positive and max_iter = {self.max_iter} non-negative")
        self.verbose = bool(options.get("verbose", False))
        self.first_stage_solution_available = False
        self.tree_solution_available = False
        self.iterations = 0
        self.history = []          # per iteration: the dict of engine.ef_read()
        self.seconds = 0.0
        self.status = None

    def _global_data(self):
        """z's bounds and objective, the count of finite bounds, max |c| and whether any q is set:
        the same on every rank."""
        b = self.batch
        nc = np.asarray(b.nonant_col, dtype=np.int64)
        oth = np.setdiff1d(np.arange(b.n), nc)
        ranged = b.rl < b.ru
        count = (np.isfinite(b.lb[:, oth]).sum() + np.isfinite(b.ub[:, oth]).sum()
                 + (np.isfinite(b.rl) & ranged).sum() + (np.isfinite(b.ru) & ranged).sum())
        sums = np.concatenate([b.prob @ b.c[:, nc], b.prob @ b.q[:, nc], [float(count)]])
        maxs = np.concatenate([b.lb[:, nc].max(axis=0), -b.ub[:, nc].min(axis=0), [np.abs(b.c).max(initial=0.0)],
                               [1.0 if np.any(b.q) else 0.0]])
        if self.n_proc > 1:
            dev = self.engine.device
            ts, tm = torch.from_numpy(sums).to(dev), torch.from_numpy(maxs).to(dev)
            self.mpicomm.allreduce_sum_(ts)
            self.mpicomm.allreduce_max_(tm)
            sums, maxs = ts.cpu().numpy(), tm.cpu().numpy()
        nn = b.nn
        zlb, zub = maxs[:nn], -maxs[nn:2 * nn]
        ncomp = sums[2 * nn] + np.isfinite(zlb).sum() + np.isfinite(zub).sum()
        return zlb, zub, sums[:nn], sums[nn:2 * nn], float(ncomp), float(maxs[2 * nn]), bool(maxs[2 * nn + 1])

    def _problem_data(self):
        """What phgpu_ef_init takes, after the checks of what the method does not serve."""
        b = self.batch
        if b.nn > 64 or b.m > 64:
            raise NotImplementedError(f"the Schur-complement interior point serves nn <= 64 and m <= 64 (nn {b.nn}, m {b.m})")
        rows, _, lo, hi, _ = first_stage_rows(b)
        for i, l, u in zip(rows, lo, hi):
            if l == u:
                raise NotImplementedError(f"row {i} has only nonant columns and equal sides [{l}, {u}]: its block of the "
                                          f"scenario's normal matrix has no interior")
        zlb, zub, cz, qz, ncomp, cmax, qp = self._global_data()
        if not np.all(zlb < zub):
            k = int(np.nonzero(~(zlb < zub))[0][0])
            raise NotImplementedError(f"nonant {k} has the bounds [{zlb[k]}, {zub[k]}] over the scenarios: a fixed "
                                      f"first-stage column leaves the interior point no interior")
        return zlb, zub, cz, qz, ncomp, cmax, qp

    def _setup(self):
        self._create_solvers()
        e = self.engine
        if e.shared:
            raise NotImplementedError("a shared-matrix handle has no per-scenario matrix to factor")
        data = self._problem_data()
        e.fix_nonants(None)
        if self._tree:
            e.eft_init(*data[0], *data[1:7], self.tol, data[7])
            zfix = self._held_z()
            if zfix is not None:
                e.eft_fix(zfix)
        else:
            e.ef_init(*data[:6], self.tol, data[6])
        self.is_qp = data[-1]

    def _held_z(self):
        """z entries to hold at values ([Ztot], NaN = free), or None (opt/ef.py fix_node_nonants)."""
        return None

    def _run(self):
        """The iterations; True when the iterate passes the test."""
        self._setup()
        e = self.engine
        iteration, schur, direction, export = ((e.eft_iteration, e.eft_schur, e.eft_direction, e.eft_export) if self._tree
                                               else (e.ef_iteration, e.ef_schur, e.ef_direction, e.ef_export))
        t0 = time.perf_counter()
        self.history, done, r = [], False, None
        for _ in range(self.max_iter):
            iteration()
            r = e.ef_read()
            self.history.append(r)
            if self.verbose and self.cylinder_rank == 0:
                print(f"EF iteration {int(r['iter']):3d}  mu {r['mu']:.3e}  primal {r['pres']:.2e}  dual {r['dres']:.2e}  "
                      f"gap {r['gap']:.2e}  objective {self.batch.sense * r['obj']:.8f}")
            done = r["done"] == 1.0
            if done or not math.isfinite(r["mu"]):
                break
        else:
            schur(0)                  # the test of the last iterate (nothing steps)
            direction(0)
            r = e.ef_read()
            self.history.append(r)
            done = r["done"] == 1.0
        export()
        torch.cuda.synchronize(e.device)
        self.seconds = time.perf_counter() - t0
        self.iterations = int(r["iter"]) if r is not None and math.isfinite(r["iter"]) else len(self.history)
        self.last = r
        self.status = "optimal" if done else "maxIterations"
        if done:
            self.load_solutions_to_models()
            self.first_stage_solution_available = True
            self.tree_solution_available = True
        return done

    # sc.py:89-104
    def solve(self):
        if not self._run():
            raise RuntimeError("Schur-Complement Interior Point algorithm did not converge")
        return self.status

    def root_nonants(self):
        """z, the ROOT nonants of the last solve (host [nlens[0]])."""
        return self.engine.ef_z.cpu().numpy()[:int(self.batch.nlens()[0])]

    def objective_value(self):
        """The extensive form's objective at the last iterate, in the model's sense."""
        return self.Eobjective()
