"""L-shaped inner bound spoke (mirrors mpisppy/cylinders/lshaped_bounder.py:14-98).

Every time the L-shaped hub's candidate x̂ arrives, the spoke puts it into its scenarios' nonants,
fixes them there, solves and offers E[objective] as an inner bound
(``calculate_incumbent(fix_nonants=True)``, :61-64).  The reference's ``main`` is a loop on its own
ranks; with this project's scheduling (cylinders/spoke.py) ``main`` is its set-up part and
``do_work`` one pass of the loop body, which ``Spoke.run_remote`` drives on the spoke's own ranks.
"""
import torch

from .spoke import InnerBoundNonantSpoke
from ..utils.xhat_eval import Xhat_Eval


class XhatLShapedInnerBound(InnerBoundNonantSpoke):
    converger_spoke_char = "X"

    # :18-40
    def xhatlshaped_prep(self):
        if self.opt.options.get("bundles_per_rank", 0):
            raise RuntimeError("xhat spokes cannot have bundles (yet)")
        if not isinstance(self.opt, Xhat_Eval):
            raise RuntimeError("XhatLShapedInnerBound must be used with Xhat_Eval.")
        self.verbose = self.opt.options.get("verbose", False)
        self.opt._lazy_create_solvers()
        self.opt._update_E1()
        if abs(1 - self.opt.E1) > self.opt.E1_tolerance:
            raise ValueError(f"Total probability of scenarios was {self.opt.E1} "
                             f"(E1_tolerance is {self.opt.E1_tolerance})")
        e = self.opt.engine
        self._cols = torch.as_tensor(self.opt.batch.nonant_col, dtype=torch.long, device=e.device)

    # :42-48 (set-up part of main)
    def main(self):
        self.xhatlshaped_prep()

    # :50-77 (loop body)
    def do_work(self):
        if self.get_serial_number() == 0 or not self.new_nonants:
            return
        e = self.opt.engine
        # the hub's values into the nonants (:56-59), then fixed there and solved
        e.x.index_copy_(0, self._cols, self.localnonants[: len(self._cols)])
        self.opt._restore_nonants()
        innerbound = self.opt.calculate_incumbent(fix_nonants=True, verbose=self.verbose)
        if self.update_if_improving(innerbound):
            self.best_xhat = {"ROOT": self.localnonants[: len(self._cols), 0].cpu().numpy()}
