"""Gradient_extension: PH with the gradient-based (cost-proportional) rho, on the device
(mirrors mpisppy/extensions/gradient_extension.py:18-108).

Options: ``ph.options["gradient_extension_options"]``, a dict (or ``{"cfg": obj}`` as the
reference) with ``order_stat``, ``rho_relative_bound``, ``xhat`` / ``xhatpath``,
``indep_denom`` (default False: compute_rho()'s scenario-dependent denominators),
``dual_update_threshold`` (default 0.05, hard-coded at gradient_extension.py:68) and
``verbose``.

The hooks keep the reference's order: post_iter0 takes the first W_diff; miditer takes W_diff,
at PH iteration 1 the gradient cost, and rewrites rho when the dual metric moved by at most the
threshold since the previous iteration.  Without ``verbose`` miditer only enqueues device work
(the gate is evaluated by phgpu_rho_from_stats), so the PH loop keeps its speculative solve.
The reference passes cost and rho through temporary csv files and a rho setter; here they stay
on the device, and there are no files.  ``rho_update_iterations()`` tells afterwards at which
PH iterations rho was rewritten.
"""
import torch

from .. import global_toc
from ..utils import find_rho, gradient
from ..utils.wtracker import WTracker
from .extension import Extension


class Gradient_extension(Extension):
    def __init__(self, opt, comm=None):
        super().__init__(opt)
        self.cylinder_rank = opt.cylinder_rank
        o = opt.options.get("gradient_extension_options") or {}
        self.cfg = o["cfg"] if isinstance(o, dict) and "cfg" in o else o
        get = gradient.cfg_get
        self._thr = float(get(o, "dual_update_threshold", get(self.cfg, "dual_update_threshold", 0.05)))
        self._indep = bool(get(o, "indep_denom", get(self.cfg, "indep_denom", False)))
        self._verbose = bool(get(o, "verbose", get(self.cfg, "verbose", False)))
        self.grad_object = gradient.Find_Grad(opt, self.cfg)
        self.rho_object = None
        self.wt = WTracker(opt)
        self._applied = None          # device int32[iterations]: 1 where rho was rewritten
        # miditer only enqueues device work unless it prints (printing reads rho back)
        self.miditer_on_device = not self._verbose

    # gradient_extension.py:47-52
    def _display_rho_values(self):
        e = self.opt.engine
        if self.cylinder_rank == 0 and e.S:
            print(self.opt.local_scenario_names[0], "rho values: ", e.rho[:e.nn, 0].cpu().tolist())

    def _slot(self, it):
        n = int(self.opt.options["PHIterLimit"]) + 2
        if self._applied is None:
            self._applied = torch.zeros(max(n, it + 1), dtype=torch.int32, device=self.opt.engine.device)
        if it >= self._applied.numel():
            self._applied = torch.cat([self._applied, torch.zeros(it + 1, dtype=torch.int32,
                                                                   device=self._applied.device)])
        return self._applied[it:it + 1]

    # gradient_extension.py:74-78
    def post_iter0(self):
        global_toc("Using gradient-based rho setter", self.cylinder_rank == 0 and self.opt.options.get("toc", True))
        self.wt.W_diff_device()
        self.opt.engine.total_scenarios()     # its one read back happens here, not in the loop
        if self._verbose:
            self._display_rho_values()

    # gradient_extension.py:80-95
    def miditer(self):
        opt = self.opt
        gate = self.wt.W_diff_device()
        if opt._PHIter == 1:
            self.grad_object.find_grad_cost()
            self.rho_object = find_rho.Find_Rho(opt, self.cfg, cost=self.grad_object.cost, refresh_xbar=False)
        if self.rho_object is None:      # the loop did not start at iteration 1: no cost yet
            return
        slot = self._slot(opt._PHIter)
        self.rho_object.apply(self._indep, gate=gate, thr=self._thr, applied=slot)
        if self._verbose and int(slot.item()):
            self._display_rho_values()

    # gradient_extension.py:101-108 removes the temporary files: there are none here
    def post_everything(self):
        pass

    def rho_update_iterations(self):
        """The PH iterations at which rho was rewritten so far (one read back)."""
        if self._applied is None:
            return []
        return [int(i) for i in torch.nonzero(self._applied).flatten().cpu().tolist()]
