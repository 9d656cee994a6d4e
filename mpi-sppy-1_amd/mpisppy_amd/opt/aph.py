"""APH: asynchronous projective hedging on the batched engine (mirrors mpisppy/opt/aph.py).

Same constructor and options as the reference and ``APH_main(spcomm=None, finalize=True) ->
(conv, Eobj, trivial_bound)``.  Per iteration, in the order of aph.py:734-814:

  phgpu_aph_reduce       Update_y (:151-181) and the sums of x̄, E[x²] and ȳ  + all-reduce
  phgpu_aph_norms        x̄, u = x - x̄, phi_s, tau, phi and the norms (:254-310)  + all-reduce
  phgpu_aph_update       theta, W += theta u, z (:453-496), the post-step phi (:756)
  Compute_Convergence    (:499-518) from the iteration's one read of pinned memory
  spoke sync, converger, miditer
  phgpu_select_smallest  the dispatch list (:602-632): the dispatch_frac share of the local
                         scenarios with the smallest (-max(last_iter, shelf_life - 1), phi)
  phgpu_solve_list       their subproblems (a full dispatch is an ordinary phgpu_solve)
  enditer
  phgpu_aph_mark         the dispatch record (:646) and the lagged W and z (:529-550)

W and x̄ are the engine's tensors, which spokes and extensions read; z is bound as the solves'
prox centre.

DEPARTURES from the reference.  Its two reductions are asynchronous (a listener thread per
rank, ``async_frac_needed``, ``async_sleep_secs``); here there is one process per GPU and no
listener thread: both reductions are synchronous all-reduces, which is what the reference
computes with async_frac_needed = 1.  The two options are accepted and ignored.  Bundles are
outside the batched engine, as for PH.  The first sort key is kept as the reference writes it:
once iterations pass shelf_life - 1 it prefers the scenarios dispatched most recently.
"""
import math
import time

from .. import global_toc
from ..phbase import PHBase


def dispatch_count(n_local, dispatch_frac):
    """Subproblems a rank dispatches per iteration (aph.py:638): Python's round (to even), at
    least one."""
    return max(1, round(n_local * dispatch_frac))


class APH(PHBase):
    SERVES_BUNDLES = False     # (PHBase serves bundles; APH's dispatch and list solve do not)

    # aph.py:69-123
    def __init__(self, options, all_scenario_names, scenario_creator, scenario_denouement=None,
                 all_nodenames=None, mpicomm=None, scenario_creator_kwargs=None, extensions=None,
                 extension_kwargs=None, ph_converger=None, rho_setter=None, variable_probability=None):
        super().__init__(options, all_scenario_names, scenario_creator, scenario_denouement,
                         all_nodenames=all_nodenames, mpicomm=mpicomm,
                         scenario_creator_kwargs=scenario_creator_kwargs, extensions=extensions,
                         extension_kwargs=extension_kwargs, ph_converger=ph_converger, rho_setter=rho_setter,
                         variable_probability=variable_probability)
        self._aph_options_check()
        self.global_tau = self.global_phi = 0.0
        self.global_pusqnorm = self.global_pvsqnorm = 0.0
        self.global_pwsqnorm = self.global_pzsqnorm = 0.0
        self.local_pwsqnorm = self.local_pzsqnorm = 0.0
        self.theta = 0.0
        self.conv = None
        self.aph_history = []       # per iteration: tau, phi, theta, conv and the post-step sum of phi
        self.dispatch_counts = []

    def _aph_options_check(self):
        o = self.options
        self.use_lag = bool(o.get("APHuse_lag", False))
        self.APHgamma = o.get("APHgamma", 1)
        if not self.APHgamma > 0:
            raise RuntimeError(f"APHgamma = {self.APHgamma} must be positive")
        self.nu = o.get("APHnu", 1)
        if not 0 < self.nu < 2:
            raise RuntimeError(f"APHnu = {self.nu} must be in (0, 2)")
        self.shelf_life = int(o.get("shelf_life", 99))
        self.round_robin_dispatch = bool(o.get("round_robin_dispatch", False))
        frac = o.get("dispatch_frac", 1)
        if not 0 < frac <= 1:
            raise RuntimeError(f"dispatch_frac = {frac} must be in (0, 1]")
        # accepted and ignored: the reductions are synchronous (module docstring)
        o.setdefault("async_frac_needed", 1)
        o.setdefault("async_sleep_secs", 0.01)

    # aph.py:499-518
    def Compute_Convergence(self, verbose=False):
        punorm, pwnorm = math.sqrt(self.global_pusqnorm), math.sqrt(self.global_pwsqnorm)
        pvnorm, pznorm = math.sqrt(self.global_pvsqnorm), math.sqrt(self.global_pzsqnorm)
        if pwnorm > 0 and pznorm > 0:
            self.conv = punorm / pwnorm + pvnorm / pznorm

    # aph.py:671-681
    def _print_conv_detail(self):
        print("Convergence Metric=", self.conv)
        punorm, pwnorm = math.sqrt(self.global_pusqnorm), math.sqrt(self.global_pwsqnorm)
        pvnorm, pznorm = math.sqrt(self.global_pvsqnorm), math.sqrt(self.global_pzsqnorm)
        print(f"   punorm={punorm} pwnorm={pwnorm} pvnorm={pvnorm} pznorm={pznorm}")
        if pwnorm > 0 and pznorm > 0:
            print(f"    scaled U term={punorm / pwnorm}; scaled V term={pvnorm / pznorm}")
        else:
            print("    ! convergence metric cannot be computed due to zero-divide")

    # aph.py:685-700 (the scalars; the per-scenario table stays on the device)
    def display_details(self, msg):
        print(f"*** cylinder rank {self.cylinder_rank} display details: {msg}")
        print(f"zero-based iteration number {self._PHIter}")
        self._print_conv_detail()
        print(f"phi={self.global_phi}, nu={self.nu}, tau={self.global_tau} so theta={self.theta}")

    # Update_y .. Update_theta_zw and the iteration's one read (aph.py:744-756)
    def _projective_step(self, first, mask):
        e = self.engine
        e.aph_reduce(first, mask)
        e.aph_norms(self.APHgamma)
        e.aph_update(first, self.nu, self.APHgamma)
        (pw, pz, theta, phisum), red = e.aph_scalars()
        self.global_tau, self.global_phi = float(red[0]), float(red[1])
        self.global_pusqnorm, self.global_pvsqnorm = float(red[2]), float(red[3])
        # the second reduction carried the previous update's local W and z norms; this rank's
        # new ones replace its own share (aph.py:469-496)
        self.global_pwsqnorm = float(red[4]) + (pw - self.local_pwsqnorm)
        self.global_pzsqnorm = float(red[5]) + (pz - self.local_pzsqnorm)
        self.local_pwsqnorm, self.local_pzsqnorm = pw, pz
        self.theta = theta
        self.phisum = phisum

    # APH_solve_loop (aph.py:554-668): the dispatch and its solves
    def APH_solve_loop(self, solver_options=None, dtiming=False, gripe=False, verbose=False, dispatch_frac=1):
        e = self.engine
        S = e.S
        scnt = dispatch_count(S, dispatch_frac)
        self.dispatch_counts.append(scnt)
        if scnt >= S:
            # a full dispatch is the ordinary solve of every local scenario
            e.aph_mask.fill_(1)
            self.solve_loop(solver_options=solver_options, dtiming=dtiming, gripe=gripe, verbose=verbose)
        else:
            k2 = e.aph_last_phi if self.round_robin_dispatch else e.aph_phi
            e.select_smallest(e.aph_k1, k2, scnt)
            t0 = time.perf_counter()
            rc = e.solve_list(e.aph_list, scnt, self._to_phgpu_options(solver_options))
            if rc:
                raise RuntimeError("APH with dispatch_frac < 1 needs the list solve, which a shared-matrix "
                                   "handle (path 4) does not have yet; use dispatch_frac = 1")
            self.solve_times.append(time.perf_counter() - t0)
            if gripe == "deferred":
                e.count_not_optimal_async()     # read at the next iteration's wait (gripe_report)
                self._gripe_pending = True
            elif gripe and e.count_not_optimal() > 0:
                self._gripe_print()
        return scnt

    # aph.py:704-817
    def APH_iterk(self, spcomm):
        verbose = self.options["verbose"]
        have_extensions = self.extensions is not None
        have_converger = self.ph_converger is not None
        dprogress = self.options["display_progress"]
        dtiming = self.options["display_timing"]
        ddetail = bool(self.options.get("display_convergence_detail"))
        self.dispatch_frac = self.options.get("dispatch_frac", 1)   # on the object: extensions may change it
        e = self.engine
        self.conv = None
        mask = None     # the bottom of the loop is at its top: the first pass sees everything dispatched
        for self._PHIter in range(1, int(self.options["PHIterLimit"]) + 1):
            t0 = time.perf_counter()
            if dprogress:
                global_toc(f"\nInitiating APH Iteration {self._PHIter}\n", self.cylinder_rank == 0)
            first = self._PHIter == 1
            self._projective_step(first, mask)
            if dprogress or verbose:
                self.gripe_report()                    # the previous iteration's solves (a second wait)
            self.Compute_Convergence()
            self.aph_history.append({"iter": self._PHIter, "tau": self.global_tau, "phi": self.global_phi,
                                     "theta": self.theta, "conv": self.conv, "phisum": self.phisum})
            if spcomm is not None:
                spcomm.sync_with_spokes()
                if spcomm.is_converged():
                    break
            if have_converger and self.convobject.is_converged():
                global_toc("User-supplied converger determined termination criterion reached",
                           self.cylinder_rank == 0)
                break
            if ddetail and self.cylinder_rank == 0:
                self.display_details("pre-solve loop (everything is updated from prev iter)")
            if have_extensions and hasattr(self.extobject, "miditer"):
                self.extobject.miditer()
            # the first pass dispatches everything, to get a decent W for everyone (:785-800)
            frac = 1 if first else self.dispatch_frac
            self.APH_solve_loop(solver_options=self.current_solver_options, dtiming=dtiming, gripe="deferred",
                                verbose=verbose, dispatch_frac=frac)
            if have_extensions and hasattr(self.extobject, "enditer"):
                self.extobject.enditer()
            # the dispatch record and, after the solves as in the reference, the lagged W and z
            e.aph_mark(self._PHIter, self.shelf_life, self.round_robin_dispatch)
            mask = e.aph_mask
            self.iter_times.append(time.perf_counter() - t0)
            if dprogress and self.cylinder_rank == 0:
                print("")
                print("After APH Iteration", self._PHIter)
                if not ddetail:
                    self._print_conv_detail()
                print("Iteration time: %6.2f" % (time.perf_counter() - t0))
                print("Elapsed time:   %6.2f" % (time.perf_counter() - self.start_time))
        self.gripe_report()

    # aph.py:820-922
    def APH_main(self, spcomm=None, finalize=True):
        """PH_Prep -> Iter0 -> APH_iterk -> post_loops; returns (conv, Eobj, trivial_bound).
        Eobj is the expected weighted objective with the proximal term (None when finalize is
        False); the trivial bound is computed after iter 0."""
        if spcomm is None:
            spcomm = self.spcomm
        self.PH_Prep()
        trivial_bound = self.Iter0()
        e = self.engine
        e.aph_init(use_lag=self.use_lag)
        e.aph_bind(True)
        self._aph_ran = False
        try:
            self.APH_iterk(spcomm)
            self._aph_ran = self._PHIter >= 1 and bool(self.dispatch_counts)
            Eobj = self.post_loops(self.extensions) if finalize else None
        finally:
            e.aph_bind(False)
        return self.conv, Eobj, trivial_bound

    def Eobjective(self, verbose=False):
        """E of the scenarios' objective expressions as they stand (spopt.py:310-343): f(x) +
        W.x + sum rho / 2 (x - z)^2 at every scenario's current x with the W and z the
        expression holds now -- the current ones, or under lag the copies of its last dispatch
        (made after that solve) -- which for a scenario not solved since they moved is not its
        solver's objective value."""
        e = self.engine
        if not getattr(self, "_aph_ran", False) or e.nn == 0:
            return self.batch.sense * e.expectations()[0]
        nn = e.nn
        Wu, zu = e._aph_use()
        xn, rho = e.nonant_x_dev()[:nn], e.rho[:nn]
        f = (e.c * e.x).sum(0) + 0.5 * (e.q * e.x * e.x).sum(0) + e.obj_const
        f = f + (Wu[:nn] * xn + 0.5 * rho * (xn - zu[:nn]) ** 2).sum(0)
        tot = (e.prob * f).sum().reshape(1)
        self.mpicomm.allreduce_sum_(tot)
        return self.batch.sense * float(tot.item())
