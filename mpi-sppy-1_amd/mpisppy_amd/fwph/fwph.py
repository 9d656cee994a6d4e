"""FWPH: Frank-Wolfe progressive hedging (Boland et al., Algorithms 2 and 3) on the batched
engine (mirrors mpisppy/fwph/fwph.py:53-303, 519-547, 596-667, 806-876).

Same constructor and options as the reference; ``fw_prep() -> best_bound`` and
``fwph_main() -> (iterations, weight_dict, xbars_dict)``.  Per outer iteration:

  for t in 0 .. FW_iter_limit - 1:                       SDM, fwph.py:210-303, all scenarios
      phgpu_fwph_direction   What = W + rho (src - x̄)
      phgpu_solve            the "MIP": one batched LP solve, What on, prox off
      phgpu_fwph_column      Gamma, the new column, the QP over the columns, the break test
      stop when the pinned active count is 0
  bound = sum_s p_s dual_bound_s                         :154-159
  diff  = sum_s p_s |xq - x̄|^2 (old x̄)                  _conv_diff, :528-547
  x̄ from the QP points; stop if diff < convthresh; W += rho (xq - x̄)

x̄ and W come from the QP points, never from the LP solutions (_swap_nonant_vars, :134).
The reference's second Pyomo model and QP solver call per scenario and inner iteration
(:284-289) are one device pass (csrc/ph_fwph.inc).  Departures: a full
column store replaces its least-weighted column; a scenario whose LP is not OPTIMAL adds no
column, and an outer iteration one of whose t = 0 LPs (the ones its bound is made of) was not
OPTIMAL reports no bound, where the reference raises (:510-517).
"""
import contextlib
import time

import numpy as np

from .. import _lib
from ..phbase import PHBase


class FWPH(PHBase):
    SERVES_BUNDLES = False     # (PHBase serves bundles; the column store is per scenario)

    # fwph.py:55-82
    def __init__(self, PH_options, FW_options, all_scenario_names, scenario_creator, scenario_denouement=None,
                 all_nodenames=None, mpicomm=None, scenario_creator_kwargs=None, ph_converger=None,
                 rho_setter=None):
        super().__init__(PH_options, all_scenario_names, scenario_creator, scenario_denouement,
                         all_nodenames=all_nodenames, mpicomm=mpicomm,
                         scenario_creator_kwargs=scenario_creator_kwargs, extensions=None,
                         extension_kwargs=None, ph_converger=ph_converger, rho_setter=rho_setter)
        self._init(FW_options)

    # fwph.py:84-89
    def _init(self, FW_options):
        self.FW_options = FW_options
        self._options_checks_fw()
        self.vb = bool(self.FW_options.get("FW_verbose", True))
        if np.any(self.batch.q != 0.0):
            # the columns carry c.x only: _extract_objective's quadratic part (fwph.py:587-593)
            # needs the leaf variables of every column (the QP's y, :723), which are not kept
            raise NotImplementedError("FWPH on this engine needs a linear objective (q = 0): its columns hold "
                                      "the nonants and c.x, not the leaf variables (fwph.py:587-593, 723)")
        self._local_bound = None
        self.fw_gamma_warnings = 0
        self.fw_inner_iters = []

    # fwph.py:816-876
    def _options_checks_fw(self):
        reqd = ["FW_iter_limit", "FW_weight", "FW_conv_thresh", "solver_name"]
        losers = [o for o in reqd if o not in self.FW_options]
        if losers:
            raise RuntimeError("FW_options is missing the following key(s): " + ", ".join(losers))
        if self.FW_options.get("point_creator") is not None:
            raise NotImplementedError("FWPH initial points (point_creator, fwph.py:96-109) are outside the "
                                      "batched engine: the store starts from Iter0's solution")
        if self.FW_options["FW_iter_limit"] == 1:
            raise RuntimeError("FW_iter_limit set to 1. To ensure convergence, provide initial points, or "
                               "increase FW_iter_limit")
        for k in ("linearize_binary_proximal_terms", "linearize_proximal_terms"):
            if self.options.get(k):
                print(f"Warning: {k} cannot be used with the FWPH algorithm. Ignoring...")
                self.options[k] = False
        self.FW_options.setdefault("time_limit", np.inf)
        mc = int(self.FW_options.setdefault("FW_max_columns", 32))
        if not 2 <= mc <= 64:
            raise RuntimeError(f"FW_max_columns = {mc} is not in [2, 64]")
        # accepted; the QP is the library's own (no solver to configure)
        self.FW_options.setdefault("qp_solver_options", {})

    # the LP solves' options: the PH object's, with mip_solver_options merged in (fwph.py:116-117)
    def _lp_options(self, base):
        o = dict(base or {})
        o.update(self.FW_options.get("mip_solver_options") or {})
        return o

    # fwph.py:91-140
    def fw_prep(self):
        self.t0 = getattr(self, "t0", time.time())
        self.PH_Prep(attach_duals=True, attach_prox=False)
        self._output_header()
        self.iter0_solver_options = self._lp_options(self.iter0_solver_options)
        self._iter0_eps_default = self._iter0_eps_default and "eps_rel" not in (self.FW_options.get("mip_solver_options") or {})
        self.iterk_solver_options = self._lp_options(self.iterk_solver_options)
        self.current_solver_options = self.iter0_solver_options
        converger, self.ph_converger = self.ph_converger, None      # made below, after the store exists
        trivial_bound = self.Iter0()
        self.ph_converger = converger
        self._output(0, trivial_bound, trivial_bound, np.nan, time.time() - self.t0)
        best_bound = trivial_bound
        e = self.engine
        # the first column is Iter0's solution, a = (1) (_initialize_QP_var_values, :773-791)
        e.fwph_init(self.FW_options["FW_max_columns"])
        e.fwph_load(e.nonant_x_dev()[None], e.obj[None])
        self._fw_prm = _lib.FwphParams(float(self.FW_options["FW_conv_thresh"]),
                                       float(self.FW_options.get("stop_check_tol", 1e-4)))
        # lines 2 and 3 of Algorithm 3 (:120-121): x̄ and W from the columns
        e.fwph_xbar_step(update_W=True)
        e.fwph_bind(False)
        if self.ph_converger is not None:
            with self._qp_points_as_x():
                self.convobject = self.ph_converger(self)
        return best_bound

    @contextlib.contextmanager
    def _qp_points_as_x(self):
        """_swap_nonant_vars (fwph.py:134): whoever reads the nonants sees the QP points."""
        e = self.engine
        e.x, e.fw_xqx = e.fw_xqx, e.x
        try:
            yield
        finally:
            e.x, e.fw_xqx = e.fw_xqx, e.x

    # SDM for every local scenario (fwph.py:210-303); returns the inner iterations launched
    def _sdm_all(self):
        e = self.engine
        alpha = float(self.FW_options["FW_weight"])
        tmax = int(self.FW_options["FW_iter_limit"])
        opts = self.current_solver_options
        neg = nopt = nopt0 = 0
        t = 0
        e.fwph_bind(True)
        while t < tmax:
            e.fwph_direction(t == 0, alpha)
            self.solve_loop(solver_options=opts, dtiming=False, gripe=False, verbose=False, warm_start=True)
            e.fwph_column(self._fw_prm, t == 0)
            t += 1
            active, n, o = e.fwph_counts()
            neg += n
            nopt += o
            if t == 1:
                nopt0 = o
            if self.n_proc > 1:
                # every rank launches the same number of solves (they hold collectives)
                active = int(max(self.mpicomm.allgather_object(active)))
            if active == 0:
                break
        e.fwph_bind(False)
        return t, neg, nopt, nopt0

    def _outer_iteration(self):
        """One outer iteration up to x̄ (fwph.py:153-187): (bound or None, diff, inner
        iterations).  W is not yet updated."""
        e = self.engine
        inner, neg, nopt, nopt0 = self._sdm_all()
        self.fw_inner_iters.append(inner)
        if self.n_proc > 1:
            neg, nopt, nopt0 = (int(sum(v)) for v in zip(*self.mpicomm.allgather_object((neg, nopt, nopt0))))
        if neg > 0:
            self.fw_gamma_warnings += 1
            if self.cylinder_rank == 0:
                print(f"Warning (fwph): convergence quantity Gamma^t < -stop_check_tol in {neg} "
                      f"scenario pass(es) (should be non-negative)\n"
                      f"Try decreasing the LP tolerance and re-solving")
        # Only fully certified LPs give a bound (the rule of LagrangianOuterBound.lagrangian; the
        # reference raises, _check_solve :510-517).  The bound is made of the t = 0 LPs alone
        # (dual_bound, :258-262), so it is withheld when one of THOSE was not OPTIMAL; a later LP
        # that was not costs its scenario a column, not the iteration its bound.
        self.fw_not_optimal = (nopt, nopt0)
        if nopt > 0 and self.cylinder_rank == 0 and (self.vb or nopt0 > 0):
            print(f"WARNING (fwph): {nopt} LP solve(s) of outer iteration {self._PHIter + 1} were not OPTIMAL and add "
                  f"no column" + (f"; {nopt0} of them at t = 0: the iteration reports no bound" if nopt0 else ""),
                  flush=True)
        bound = None if nopt0 > 0 else self.batch.sense * e.fwph_bound()
        self._local_bound = bound
        diff = float(e.fwph_diff().item())        # the old x̄ (_conv_diff before Compute_Xbar, :186-187)
        return bound, diff, inner

    def _is_timed_out(self):
        out = (time.time() - self.t0) > self.FW_options["time_limit"] if self.cylinder_rank == 0 else None
        return bool(self.mpicomm.bcast_object(out, root=0))

    def _better(self, best, bound):
        if bound is None:
            return best
        return max(best, bound) if self.is_minimizing else min(best, bound)

    def fw_step(self, itr, best_bound):
        """Outer iteration ``itr`` (0-based) in full: (best_bound, stop)."""
        self._PHIter = itr
        e = self.engine
        bound, diff, _ = self._outer_iteration()
        best_bound = self._better(best_bound, bound)
        shown = np.nan if bound is None else bound
        if self.spcomm is not None and self.spcomm.is_converged():
            self._output(itr + 1, shown, best_bound, np.nan, time.time() - self.t0)
            return best_bound, True
        if self.ph_converger is not None:
            e.fwph_xbar_step(update_W=False)
            with self._qp_points_as_x():
                diff = self.convobject.convergence_value() if hasattr(self.convobject, "convergence_value") \
                    else np.nan
                stop = self.convobject.is_converged()
        else:
            stop = diff < self.options["convthresh"]
            if stop:
                e.fwph_xbar_step(update_W=False)
        self._output(itr + 1, shown, best_bound, diff, time.time() - self.t0)
        self.fw_last_diff = diff
        if stop:
            if self.cylinder_rank == 0 and self.vb:
                print("FWPH converged to user-specified criteria" if self.ph_converger is not None
                      else "PH converged based on standard criteria")
            return best_bound, True
        # Update_W (:198) with the new x̄ (one launch does both without a converger)
        e.fwph_xbar_step(update_W=True)
        if self._is_timed_out():
            if self.cylinder_rank == 0 and self.vb:
                print("Timeout.")
            return best_bound, True
        return best_bound, False

    # fwph.py:142-208
    def fwph_main(self):
        self.t0 = time.time()
        best_bound = self.fw_prep()
        if self.spcomm is not None and self.spcomm.is_converged():
            return None, None, None
        itr = -1
        for itr in range(self.options["PHIterLimit"]):
            best_bound, stop = self.fw_step(itr, best_bound)
            if stop:
                break
            if self.spcomm is not None:
                self.spcomm.sync()
        self.best_bound = best_bound
        return itr + 1, self._gather_weight_dict(), self._get_xbars()

    # fwph.py:596-621: per rank {scenario name: {nonant name: W}}, gathered on rank 0
    def _gather_weight_dict(self):
        W = self.W_array()
        names = self.batch.nonant_names or [f"nonant[{k}]" for k in range(self.batch.nn)]
        local = {sn: {names[k]: float(W[s, k]) for k in range(self.batch.nn)}
                 for s, sn in enumerate(self.local_scenario_names)}
        out = self.mpicomm.gather_object(local, root=0)
        return out if self.cylinder_rank == 0 else None

    # fwph.py:637-666: {nonant name: x̄} of the first local scenario, rank 0 only
    def _get_xbars(self):
        if self.cylinder_rank != 0:
            return None
        xb = self.engine.host("xbar")
        names = self.batch.nonant_names or [f"nonant[{k}]" for k in range(self.batch.nn)]
        return {names[k]: float(xb[0, k]) for k in range(self.batch.nn)}

    # fwph.py:878-897
    def _output(self, itr, bound, best_bound, diff, secs):
        if self.cylinder_rank == 0 and self.vb:
            print(f"{itr:3d} {bound:12.4f} {best_bound:12.4f} {diff:12.4e} {secs:11.1f}s")
        if self.cylinder_rank == 0 and "save_file" in self.FW_options:
            with open(self.FW_options["save_file"], "a") as f:
                f.write(f"{itr:d},{bound:.16f},{best_bound:.16f},{diff:.16f},{secs:.16f}\n")

    def _output_header(self):
        if self.cylinder_rank == 0 and self.vb:
            print("itr {:>12s} {:>12s} {:>12s} {:>12s}".format("bound", "best bound", "conv. diff", "time"))
        if self.cylinder_rank == 0 and "save_file" in self.FW_options:
            with open(self.FW_options["save_file"], "a") as f:
                f.write("itr,bound,best bound,conv diff,time\n")
