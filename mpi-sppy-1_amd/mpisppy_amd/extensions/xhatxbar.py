"""XhatXbar: x̄ itself as the xhat candidate (mirrors mpisppy/extensions/xhatxbar.py:12-133).

The reference computes x̄ (phbase._Compute_Xbar, :83), sets every nonant Var to its node's
x̄ and fixes it (:38-55; integers rounded -- this engine has continuous nonants only), solves
every scenario and takes E[objective] if none is infeasible (:87-103).  Here x̄ of the given
nonant values is one device reduction over all local scenarios and one all-reduce
(engine.nonant_stats, plane 0), the fix is one kernel (fix_nonants_by_node) and the solves
one batched launch.  For continuous LP/QP x̄ is a convex combination of feasible first
stages; a multistage tree is served node by node (the reference does not restrict it).

Works on an Xhat_Eval (the spoke, cylinders/xhatxbar_bounder.py) and as a PH extension
(``post_everything``, :125-133).
"""
from .extension import Extension
from .xhatbase import XhatBase


class XhatXbar(XhatBase):
    def __init__(self, spo):
        super().__init__(spo)
        self.options = spo.options["xhat_xbar_options"]
        self.solver_options = self.options.get("xhat_solver_options")
        self.keep_solution = bool(self.options.get("keep_solution", True))
        self.verbose = spo.options.get("verbose", False)

    # xhatxbar.py:59-110
    def xhat_tryit(self, verbose=False, restore_nonants=True, nonant_cache=None):
        """Fix every nonant at its node's x̄ of ``nonant_cache`` (device [nn, S_local]; default:
        the nonants of the last solve), solve, and return E[objective] -- or None if some
        scenario is not accepted (infeas_prob() > 1e-12, as XhatBase._try_one)."""
        def _vb(msg):
            if verbose and self.cylinder_rank == 0:
                print("  xhat_xbar: " + msg)

        e = self.opt.engine
        if nonant_cache is None:
            nonant_cache = e.nonant_x_dev()
        _vb("   Solver options=" + str(self.solver_options))
        xbar = e.nonant_stats(nonant_cache)[0].clone()
        self.opt._fix_nonants(xbar)
        self.opt.solve_loop(solver_options=self.solver_options, verbose=verbose)
        if self.opt.infeas_prob() > 1e-12:
            self.opt._restore_nonants()
            _vb("Infeasible")
            return None
        obj = self.opt.Eobjective(verbose=verbose)
        self.last_table = xbar
        if restore_nonants:
            self.opt._restore_nonants()
        _vb("Feasible, returning " + str(obj))
        return obj

    # the loop hooks the reference defines as no-ops: the base class's own, so the PH loop
    # sees nothing to call and keeps its speculative solve
    miditer = Extension.miditer
    enditer = Extension.enditer

    # xhatxbar.py:125-133
    def post_everything(self):
        restore_nonants = not self.keep_solution
        self.opt.disable_W_and_prox()
        self.opt.Compute_Xbar()
        obj = self.xhat_tryit(verbose=self.verbose, restore_nonants=restore_nonants)
        self.opt.reenable_W_and_prox()
        self._xhat_xbar_obj_final = obj
