"""The L-shaped method on the batched engine (mirrors mpisppy/opt/lshaped.py).

Same constructor as the reference and ``lshaped_algorithm(converger=None)``.  Two-stage problems,
minimisation internally (lshaped.py:84-85); a maximisation model is negated as everywhere else.

    master:  min sum_g eta_g   over the ROOT nonants x and one eta per cut group
             nonant bounds, first-stage rows, eta >= etalb, eta_g - a.x >= b for every cut

eta_g models sum_{s in g} p_s f_s(x) with f_s the WHOLE objective of scenario s, first-stage cost
included.  Per iteration, one read of pinned memory:

    fix_nonants(x̂) -> solve (W off, prox off, duals kept) -> phgpu_lshaped_cuts -> all-reduce
    -> phgpu_lshaped_append -> phgpu_lshaped_master -> read {cuts added, E[f(x̂)], outer bound, ..}

DEPARTURES from the reference.  ``cut_groups`` aggregates the etas (the reference has one per
scenario; here that is the default up to 32 scenarios, above that 32 groups).  Without
``valid_eta_lb`` the first action is the wait-and-see solve: its dual bounds are etalb and the
probability-weighted mean of its nonants is the first candidate (first-stage feasible by
convexity); the reference solves a master without cuts instead, whose x is arbitrary.  An
infeasible subproblem raises: feasibility cuts need a Farkas ray, which the solve does not
export.  ``root_scenarios``, bundles and a shared-matrix handle raise NotImplementedError.
``relax_root`` and ``store_subproblems`` are accepted and ignored (LPs only; the subproblems live
in the batch).  A nonant whose bounds are equal over the scenarios (no interior for the master's
interior point) raises NotImplementedError.  ``max_cuts`` (this engine's own, default
``cut_groups * max_iter``, so that no cut is ever dropped) sizes the cut store; with a smaller
value a full store raises RuntimeError when a wanted cut does not fit.
"""
import time

import numpy as np
import torch

from .. import _lib
from ..spopt import SPOpt, SOLVER_NAMES

# the master's objective agrees with HiGHS to 4.2e-10 relative on the test masters (DESIGN.md
# 3.19), more than ten times below the reference's 1e-8, which therefore stands
DEFAULT_TOL = 1e-8
MAX_GROUPS = 32


def default_cut_groups(S_total):
    return S_total if S_total <= MAX_GROUPS else MAX_GROUPS


def first_stage_rows(batch):
    """The rows of the shared pattern whose columns are all nonants, from the local batch:
    (row indices, dense R [rows, nn] of local scenario 0, rl, ru of it, and per row whether
    coefficients and sides are bitwise equal in every local scenario)."""
    slot = np.full(batch.n, -1, dtype=np.int64)
    slot[batch.nonant_col] = np.arange(batch.nn)
    rows, R, lo, hi, same = [], [], [], [], []
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)  # noqa: E731
    for i in range(batch.m):
        a, b = batch.row_ptr[i], batch.row_ptr[i + 1]
        cols = batch.col_idx[a:b]
        if b == a or np.any(slot[cols] < 0):
            continue
        r = np.zeros(batch.nn)
        np.add.at(r, slot[cols], batch.A_val[0, a:b])
        rows.append(i)
        R.append(r)
        lo.append(batch.rl[0, i])
        hi.append(batch.ru[0, i])
        A, l, u = bits(batch.A_val[:, a:b]), bits(batch.rl[:, i]), bits(batch.ru[:, i])
        same.append(bool((A == A[:1]).all() and (l == l[0]).all() and (u == u[0]).all()))
    return rows, np.array(R).reshape(len(rows), batch.nn), np.array(lo), np.array(hi), same


class LShapedMethod(SPOpt):
    # lshaped.py:64-125
    def __init__(self, options, all_scenario_names, scenario_creator, scenario_denouement=None,
                 all_nodenames=None, mpicomm=None, scenario_creator_kwargs=None):
        options.setdefault("solver_name", options.get("sp_solver", SOLVER_NAMES[0]))
        super().__init__(options, all_scenario_names, scenario_creator, scenario_denouement=scenario_denouement,
                         all_nodenames=all_nodenames, mpicomm=mpicomm,
                         scenario_creator_kwargs=scenario_creator_kwargs)
        if self.multistage or self.batch.depth != 1:
            raise RuntimeError("LShaped does not currently support multiple stages")      # lshaped.py:84-85
        self.options_check()
        self.scenario_count = len(self.all_scenario_names)
        self.valid_eta_lb = options.get("valid_eta_lb")
        self.compute_eta_bound = self.valid_eta_lb is None
        G = options.get("cut_groups")
        self.cut_groups = default_cut_groups(self.scenario_count) if G is None else int(G)
        if not 1 <= self.cut_groups <= min(MAX_GROUPS, self.scenario_count):
            raise ValueError(f"cut_groups = {self.cut_groups} must be in 1..{min(MAX_GROUPS, self.scenario_count)}")
        self.tol = float(options.get("tol", DEFAULT_TOL))
        self.max_iter = int(options.get("max_iter", 30))
        self.verbose = bool(options.get("verbose", False))
        self.iter = 0
        self._LShaped_bound = None
        self.first_stage_solution_available = False
        self.tree_solution_available = False
        # per iteration: the master's outer bound, E[f(x̂)], cuts added, master iterations, seconds so far
        self.history = []
        self.timing = {"solve": 0.0, "cuts": 0.0, "master": 0.0}

    # lshaped.py:127-145 and what this engine does not serve
    def options_check(self):
        o = self.options
        for key in ("root_solver", "sp_solver"):
            if key not in o:
                raise RuntimeError(f"LShapedMethod needs the option {key!r}")
            if o[key] not in SOLVER_NAMES:
                raise RuntimeError(f"{key} {o[key]!r} is not served by this engine; use one of {SOLVER_NAMES}")
        o.setdefault("root_solver_options", {})
        o.setdefault("sp_solver_options", {})
        if o.get("root_scenarios"):
            raise NotImplementedError("root_scenarios (lshaped.py:99-101, 172-230) are not served: "
                                      "the master holds the nonants and the etas only")
        if o.get("bundles_per_rank", 0):
            raise NotImplementedError("bundles (spbase.py:184-216) are outside the batched engine")
        if o.get("shared_matrix"):
            raise NotImplementedError("a shared-matrix handle has no per-scenario matrix for the cut pass "
                                      "(lshaped.py:477-520)")
        # relax_root, store_subproblems: accepted and ignored (module docstring)

    def _global_offset(self):
        return int(self._rank_slices[self.cylinder_rank][0])

    def _master_data(self):
        """First-stage rows and nonant bounds, agreed over the ranks (every rank the same)."""
        b = self.batch
        rows, R, lo, hi, same = first_stage_rows(b)
        nc = b.nonant_col
        mine = (rows, R, lo, hi, same, b.lb[:, nc].max(axis=0), b.ub[:, nc].min(axis=0))
        every = self.mpicomm.allgather_object(mine) if self.n_proc > 1 else [mine]
        r0 = every[0]
        bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)  # noqa: E731
        keep = []
        for j in range(len(r0[0])):
            ok = all(e[4][j] and (bits(e[1][j]) == bits(r0[1][j])).all() and bits(e[2][j:j + 1])[0] == bits(r0[2][j:j + 1])[0]
                     and bits(e[3][j:j + 1])[0] == bits(r0[3][j:j + 1])[0] for e in every)
            if ok:
                keep.append(j)
        xlb = np.max([e[5] for e in every], axis=0)
        xub = np.min([e[6] for e in every], axis=0)
        return r0[1][keep].reshape(len(keep), b.nn), r0[2][keep], r0[3][keep], xlb, xub

    def _group_sums(self, per_scenario):
        """sum over the scenarios of every group of p_s v_s, over all ranks: host [G]."""
        G, S_tot, off = self.cut_groups, self.scenario_count, self._global_offset()
        grp = (np.arange(self.batch.S) + off) * G // S_tot
        loc = np.bincount(grp, weights=self.batch.prob * per_scenario, minlength=G)
        t = torch.from_numpy(loc).to(self.engine.device)
        if self.n_proc > 1:
            self.mpicomm.allreduce_sum_(t)
        return t.cpu().numpy()

    def _raise_if_infeasible(self):
        st = self.engine.status.cpu().numpy()
        bad = np.nonzero(st == _lib.PRIMAL_INFEASIBLE)[0]
        if len(bad):
            raise RuntimeError(f"subproblem {self.batch.names[bad[0]]} is infeasible at the candidate: feasibility "
                               f"cuts are not served (no relatively complete recourse)")
        n = int((st != _lib.OPTIMAL).sum())
        if n:
            raise RuntimeError(f"{n} subproblem(s) were not solved to optimality (first: "
                               f"{self.batch.names[np.nonzero(st != _lib.OPTIMAL)[0][0]]}, status "
                               f"{st[np.nonzero(st != _lib.OPTIMAL)[0][0]]})")

    def _setup(self):
        self._create_solvers()
        e = self.engine
        if e.shared:
            raise NotImplementedError("a shared-matrix handle has no per-scenario matrix for the cut pass "
                                      "(lshaped.py:477-520)")
        e.set_terms(0, 0)
        e.want_duals = True
        self._sp_opts = self._to_phgpu_options(self.options.get("sp_solver_options"))
        self._root_opts = self._to_phgpu_options(self.options.get("root_solver_options"))
        # the wait-and-see solve: etalb and the first candidate (module docstring)
        e.fix_nonants(None)
        e.solve(self._sp_opts, warm=False)
        self._raise_if_infeasible()
        e.compute_xbar()
        x0 = np.array(e.node_xbar()["ROOT"][: self.batch.nn], dtype=np.float64)
        bound = e.bound.cpu().numpy()
        self.trivial_bound = self.batch.sense * float(self._group_sums(bound).sum())
        if self.valid_eta_lb is not None:
            lbs = np.array([self.valid_eta_lb[nm] for nm in self.batch.names], dtype=np.float64)
        else:
            lbs = bound
        self.etalb = self._group_sums(lbs)
        R, rl, ru, xlb, xub = self._master_data()
        self.master_rows = (R, rl, ru, xlb, xub)
        if not np.all(xlb < xub):
            k = int(np.nonzero(~(xlb < xub))[0][0])
            raise NotImplementedError(f"nonant {k} has the bounds [{xlb[k]}, {xub[k]}] over the scenarios: a fixed "
                                      f"first-stage column leaves the master's interior point no interior")
        max_cuts = int(self.options.get("max_cuts", self.cut_groups * self.max_iter))
        e.lshaped_init(self.cut_groups, max_cuts, self._global_offset(), self.scenario_count, R, rl, ru, xlb, xub,
                       self.etalb)
        e.ls_xhat.copy_(torch.from_numpy(x0).to(e.device)[:, None].expand(-1, e.S))
        self._cand = torch.empty_like(e.ls_xhat)

    def current_xhat(self):
        """The candidate the last cuts were made at (host [nn])."""
        return self._cand[:, 0].cpu().numpy()

    def nonants_dev(self):
        """The newest candidate for every local scenario (device [nn, S]): what the hub sends."""
        return self.engine.ls_xhat

    # lshaped.py:523-666
    def lshaped_algorithm(self, converger=None):
        if converger:
            converger = converger(self, self.cylinder_rank, self.n_proc)
        self._setup()
        e = self.engine
        sense = self.batch.sense
        self._LShaped_bound = sense * float(self.etalb.sum())
        t_start = time.perf_counter()
        timed = bool(self.options.get("time_phases", False))

        def mark(key, t0):
            if timed:
                torch.cuda.synchronize(e.device)
                self.timing[key] += time.perf_counter() - t0
            return time.perf_counter()

        if self.spcomm:
            self.spcomm.sync(send_nonants=True)
            if self.spcomm.is_converged():
                return None
        res = None
        for self.iter in range(self.max_iter):
            t0 = time.perf_counter()
            self._cand.copy_(e.ls_xhat)
            e.fix_nonants(self._cand)
            e.solve(self._sp_opts, warm=True)
            t0 = mark("solve", t0)
            e.lshaped_cuts()
            e.lshaped_append(self.tol)
            t0 = mark("cuts", t0)
            e.lshaped_master(self._root_opts)
            res = dict(e.lshaped_read())
            mark("master", t0)
            if res["not_optimal"] > 0:
                self._raise_if_infeasible()
            self.Eobj_at_xhat = sense * res["Q"]
            added = int(res["added"])
            self.history.append((sense * res["bound"], self.Eobj_at_xhat, added, int(res["iters"]),
                                 time.perf_counter() - t_start))
            if self.verbose and self.cylinder_rank == 0:
                print(f"Current Iteration: {self.iter + 1} Time Elapsed: {time.perf_counter() - t_start:7.2f} "
                      f"Cuts Added: {added} Expected Cost: {self.Eobj_at_xhat:.4f} Current Objective: "
                      f"{self._LShaped_bound:.4f}")
            if int(res["wanted"]) > added:
                raise RuntimeError(f"the cut store is full ({int(res['held'])} cuts, option max_cuts): "
                                   f"{int(res['wanted']) - added} cut(s) were dropped at iteration {self.iter + 1}")
            if added == 0:
                # no group's eta is cut off: the candidate is optimal for the master (lshaped.py:640-651)
                self.first_stage_solution_available = True
                self.tree_solution_available = True
                if self.verbose and self.cylinder_rank == 0:
                    print(f"Converged in {self.iter + 1} iterations.")
                break
            if self.spcomm:
                self.spcomm.sync(send_nonants=False)
                if self.spcomm.is_converged():
                    break
            if int(res["status"]) == _lib.PRIMAL_INFEASIBLE:
                raise RuntimeError("the L-shaped master is infeasible: the first-stage rows and bounds contradict")
            if int(res["status"]) != _lib.OPTIMAL:
                raise RuntimeError(f"the L-shaped master was not solved (status {int(res['status'])} after "
                                   f"{int(res['iters'])} iterations; residuals {res['pres']:.1e} {res['dres']:.1e} "
                                   f"{res['gap']:.1e})")
            self._LShaped_bound = sense * res["bound"]
            if self.spcomm:
                self.spcomm.sync(send_nonants=True)
                if self.spcomm.is_converged():
                    break
            if converger:
                converger.convergence_value()
                if converger.is_converged():
                    break
        else:
            if self.verbose and self.cylinder_rank == 0:
                print("WARNING MAX ITERATION LIMIT REACHED !!! ")
        return res
