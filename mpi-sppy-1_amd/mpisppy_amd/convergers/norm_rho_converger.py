"""NormRhoConverger: stop when log(sum_s prob_s sum_k rho[k, s]) drops below convthresh
(mirrors mpisppy/convergers/norm_rho_converger.py:12-56).  The sum is plane 3 of
engine.residuals (phgpu_ph_residuals), summed over the ranks there.
"""
import math

from .converger import Converger


class NormRhoConverger(Converger):
    # norm_rho_converger.py:14-21
    def __init__(self, ph):
        super().__init__(ph)
        opts = ph.options.get("norm_rho_converger_options") or {}
        self._verbose = bool(opts.get("verbose", False))
        self.ph = ph

    # norm_rho_converger.py:23-29
    def _compute_rho_norm(self, ph):
        ph.engine.residuals()
        return ph.engine.rho_norm()

    # norm_rho_converger.py:31-56
    def is_converged(self):
        # this never does anything unless the norm rho updater is also used
        if not getattr(self.ph, "_mpisppy_norm_rho_update_inuse", False):
            raise RuntimeError("NormRhoConverger can only be used if NormRhoUpdater is")
        log_rho_norm = math.log(self._compute_rho_norm(self.ph))
        ret_val = log_rho_norm < self.ph.options["convthresh"]
        self.conv = log_rho_norm
        if self._verbose and self.ph.cylinder_rank == 0:
            print(f"log(|rho|) = {log_rho_norm}")
            if ret_val:
                print("Norm rho convergence check passed")
            else:
                print("Adaptive rho convergence check failed "
                      f"(requires log(|rho|) < {self.ph.options['convthresh']}")
                print("Continuing PH with updated rho")
        return ret_val
