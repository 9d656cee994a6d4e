"""MultRhoUpdater: rho held at a constant multiple of 1 / conv, updated only when the
convergence metric reaches a new best (mirrors mpisppy/extensions/mult_rho_updater.py:14-106).

The decision needs the loop's conv on the host, so this is a plain host ``miditer`` (the PH
loop runs it after the convergence readback, without its speculative solve); the rescale
itself is one device operation on the [nn, S] rho array.  The reference keeps the first rho of
one arbitrary scenario per (node, nonant) and writes it to all (:59-69); here every scenario
keeps its own first rho, which is the same thing whenever rho does not depend on the scenario.
"""
import torch

from .extension import Extension

# mult_rho_updater.py:15-19
_mult_rho_defaults = {
    "convergence_tolerance": 1e-4,
    "rho_update_stop_iteration": None,
    "rho_update_start_iteration": None,
    "verbose": False,
}

# mult_rho_updater.py:21-26
_attr_to_option_name_map = {
    "_tol": "convergence_tolerance",
    "_stop_iter": "rho_update_stop_iteration",
    "_start_iter": "rho_update_start_iteration",
    "_verbose": "verbose",
}


class MultRhoUpdater(Extension):
    # mult_rho_updater.py:31-39
    def __init__(self, ph):
        super().__init__(ph)
        self.ph = ph
        self.mult_rho_options = ph.options["mult_rho_options"] if "mult_rho_options" in ph.options else dict()
        self._set_options()
        self._first_rho = None
        self.best_conv = float("inf")
        self.acted = []               # the PH iterations at which rho was rescaled

    # mult_rho_updater.py:42-46
    def _conv(self):
        if self.ph.convobject is not None:
            return self.ph.convobject.conv
        return self.ph.conv

    # mult_rho_updater.py:49-52
    def _set_options(self):
        options = self.mult_rho_options
        for attr_name, opt_name in _attr_to_option_name_map.items():
            setattr(self, attr_name, options[opt_name] if opt_name in options else _mult_rho_defaults[opt_name])

    # mult_rho_updater.py:55-69
    def _attach_rho_ratio_data(self, ph, conv):
        if conv is None or conv == self._tol:
            return
        self.first_c = conv
        self._first_rho = ph.engine.rho.clone()

    # mult_rho_updater.py:78-100
    def miditer(self):
        ph = self.ph
        ph_iter = ph._PHIter
        if (self._stop_iter is not None and ph_iter > self._stop_iter) \
                or (self._start_iter is not None and ph_iter < self._start_iter):
            return
        conv = self._conv()
        if conv < self.best_conv:
            self.best_conv = conv
        else:
            return   # only do something if we have a new best
        if self._first_rho is None:
            self._attach_rho_ratio_data(ph, conv)  # rho / conv
        elif conv != 0:
            e = ph.engine
            e._flush_step()
            torch.mul(self._first_rho, self.first_c / conv, out=e.rho)
            self.acted.append(ph_iter)
            if self._verbose and ph.cylinder_rank == 0:
                print(f"MultRhoUpdater iter={ph_iter}; the first scenario's last nonant now has rho "
                      f"{float(e.rho[max(e.nn - 1, 0), 0])}")
