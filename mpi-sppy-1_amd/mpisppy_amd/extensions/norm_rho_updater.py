"""NormRhoUpdater: adaptive rho from the primal and dual residual norms, on the device
(mirrors mpisppy/extensions/norm_rho_updater.py:12-164).

The reference loops over scenarios and nonants on the host; here the residual sums are one
device pass (engine.residuals -> phgpu_ph_residuals), the ranks' sums one all-reduce, and
the rule one kernel over every local (nonant, scenario) (engine.norm_rho_update ->
phgpu_norm_rho_update).  Nothing is read back unless ``verbose`` asks for the table.
"""
import numpy as np

from .. import _lib
from .extension import Extension

# norm_rho_updater.py:12-20
_norm_rho_defaults = {
    "convergence_tolerance": 1e-4,
    "rho_decrease_multiplier": 2.0,
    "rho_increase_multiplier": 2.0,
    "primal_dual_difference_factor": 100.0,
    "iterations_converged_before_decrease": 0,
    "rho_converged_decrease_multiplier": 1.1,
    "rho_update_stop_iterations": None,
    "verbose": False,
}

# norm_rho_updater.py:22-31
_attr_to_option_name_map = {
    "_tol": "convergence_tolerance",
    "_rho_decrease": "rho_decrease_multiplier",
    "_rho_increase": "rho_increase_multiplier",
    "_primal_dual_difference_factor": "primal_dual_difference_factor",
    "_required_converged_before_decrease": "iterations_converged_before_decrease",
    "_rho_converged_residual_decrease": "rho_converged_decrease_multiplier",
    "_stop_iter_rho_update": "rho_update_stop_iterations",
    "_verbose": "verbose",
}

_ACTIONS = (None, "Increasing", "Decreasing", "Converged, Decreasing")


class NormRhoUpdater(Extension):
    # norm_rho_updater.py:35-43
    def __init__(self, ph):
        super().__init__(ph)
        self.ph = ph
        self.norm_rho_options = ph.options["norm_rho_options"] if "norm_rho_options" in ph.options else dict()
        self._set_options()
        self._have_prev_avg = False
        self.ph._mpisppy_norm_rho_update_inuse = True  # allow NormRhoConverger
        # miditer only enqueues device work unless the table is printed (it reads rho back)
        self.miditer_on_device = not self._verbose

    # norm_rho_updater.py:45-48
    def _set_options(self):
        options = self.norm_rho_options
        for attr_name, opt_name in _attr_to_option_name_map.items():
            setattr(self, attr_name, options[opt_name] if opt_name in options else _norm_rho_defaults[opt_name])

    # the constants of norm_rho_updater.py:134-143 for phgpu_norm_rho_update
    def _params(self, ph_iter):
        return _lib.NormRhoParams(tol=float(self._tol), inc=float(self._rho_increase),
                                  dec=float(self._rho_decrease),
                                  conv_dec=float(self._rho_converged_residual_decrease),
                                  f=float(self._primal_dual_difference_factor),
                                  allow_decrease=1 if ph_iter >= self._required_converged_before_decrease else 0)

    # norm_rho_updater.py:112-158
    def miditer(self):
        ph = self.ph
        ph_iter = ph._PHIter
        if self._stop_iter_rho_update is not None and (ph_iter > self._stop_iter_rho_update):
            return
        e = ph.engine
        if not self._have_prev_avg:
            e.xbar_snapshot()
            self._have_prev_avg = True
            return
        e.residuals()
        params = self._params(ph_iter)
        if self._verbose and ph.cylinder_rank == 0:
            before = self._table_inputs(e)
        e.norm_rho_update(params)
        if self._verbose and ph.cylinder_rank == 0:
            self._print_table(e, params, *before)

    # the inputs of the table's residual columns, read before the update renews the snapshot
    def _table_inputs(self, e):
        half = e.num_nodes * e.nlen_max
        p = e.residual_planes()[0]
        d = e.rho_last.cpu().numpy() * np.abs(e.node_buf[:half].cpu().numpy() - e._xbar_prev.cpu().numpy())
        return p, d

    # norm_rho_updater.py:144-157: the first local scenario's rows, on cylinder rank 0
    def _print_table(self, e, params, p, d):
        b = e.batch
        rho0 = e.rho[:, 0].cpu().numpy()
        node0 = e.node_of[:, 0].cpu().numpy()
        first = True
        for k in range(b.nn):
            o = int(node0[b.nonant_depth[k]]) * e.nlen_max + int(b.nonant_off[k])
            pr, dr = float(p[o]), float(d[o])
            if pr > params.f * dr and pr > params.tol:
                action = 1
            elif dr > params.f * pr and dr > params.tol:
                action = 2 if params.allow_decrease else 0
            elif pr < params.tol and dr < params.tol:
                action = 3
            else:
                action = 0
            if not action:
                continue
            if first:
                first = False
                print("Updating rho values:\n%21s %40s %16s %16s %16s"
                      % ("Action", "Variable", "Primal Residual", "Dual Residual", "New Rho"))
            name = b.nonant_names[k] if getattr(b, "nonant_names", None) else f"nonant[{k}]"
            print("%21s %40s %16g %16g %16g" % (_ACTIONS[action], name, pr, dr, rho0[k]))
