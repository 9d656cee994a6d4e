"""PrimalDualConverger: stop when max(primal gap, dual gap) <= tol (mirrors
mpisppy/convergers/primal_dual_converger.py:9-137).

  primal gap = sum_s sum_k pcoef |x - x̄|                (plane 1 of engine.residuals)
  dual gap   = sum_s sum_k rho[k, s] |x̄ - x̄_prev|      (plane 2 times the node x̄ change)

The reference's tracker (pandas / matplotlib, ``tracking``) is not carried over.
"""
from .converger import Converger


class PrimalDualConverger(Converger):
    # primal_dual_converger.py:16-42
    def __init__(self, ph):
        super().__init__(ph)
        self.options = ph.options.get("primal_dual_converger_options", {})
        self._verbose = self.options.get("verbose", False)
        self._ph = ph
        self.convergence_threshold = self.options.get("tol", 1)
        self.tracking = self.options.get("tracking", False)
        if self.tracking:
            raise NotImplementedError("PrimalDualConverger: tracking (the reference's pandas / matplotlib "
                                      "tracker) is not available; set tracking to False")
        self.prev_xbars = self._get_xbars()
        self._rank = self._ph.cylinder_rank

    # primal_dual_converger.py:44-56 (the node x̄ as one host vector)
    def _get_xbars(self):
        return self._ph.engine.node_xbar_flat().copy()

    # primal_dual_converger.py:58-85
    def _compute_primal_convergence(self):
        return self._ph.engine.primal_gap()

    # primal_dual_converger.py:87-110
    def _compute_dual_residual(self):
        return self._ph.engine.dual_gap(self.prev_xbars)

    # primal_dual_converger.py:112-137
    def is_converged(self):
        self._ph.engine.residuals()
        primal_gap = self._compute_primal_convergence()
        dual_gap = self._compute_dual_residual()
        self.prev_xbars = self._get_xbars()
        self.primal_gap, self.dual_gap = primal_gap, dual_gap
        ret_val = max(primal_gap, dual_gap) <= self.convergence_threshold
        if self._verbose and self._rank == 0:
            print(f"primal gap = {round(primal_gap, 5)}, dual gap = {round(dual_gap, 5)}")
            if ret_val:
                print("Dual convergence check passed")
            else:
                print("Dual convergence check failed "
                      f"(requires primal + dual gaps) <= {self.convergence_threshold}")
        return ret_val
