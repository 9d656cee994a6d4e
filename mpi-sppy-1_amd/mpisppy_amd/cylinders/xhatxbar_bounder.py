"""x̄ inner bound spoke (mirrors mpisppy/cylinders/xhatxbar_bounder.py:31-108).

Every time the hub's nonants arrive, the spoke fixes every scenario's nonants at the x̄ of
those values, solves and offers E[objective] as an inner bound (:96-104).  The x̄ comes from
the delivered nonants by one device reduction (extensions/xhatxbar.py), so the spoke needs
no xbars Params of its own (the reference's _attach_xbars, :19-27).
"""
from .spoke import InnerBoundNonantSpoke
from ..extensions.xhatxbar import XhatXbar
from ..utils.xhat_eval import Xhat_Eval


class XhatXbarInnerBound(InnerBoundNonantSpoke):
    converger_spoke_char = "B"

    # :35-74
    def ib_prep(self):
        if self.opt.options.get("bundles_per_rank", 0):
            raise RuntimeError("xhat spokes cannot have bundles (yet)")
        if not isinstance(self.opt, Xhat_Eval):
            raise RuntimeError("XhatXbarInnerBound must be used with Xhat_Eval.")
        self.verbose = self.opt.options["verbose"]
        xhatter = XhatXbar(self.opt)
        xhatter.pre_iter0()
        self.opt._lazy_create_solvers()
        self.opt._update_E1()
        if abs(1 - self.opt.E1) > self.opt.E1_tolerance:
            raise ValueError(f"Total probability of scenarios was {self.opt.E1} "
                             f"(E1_tolerance is {self.opt.E1_tolerance})")
        xhatter.post_iter0()
        return xhatter

    # :76-85 (set-up part of main)
    def main(self):
        self.xhatter = self.ib_prep()

    # :96-104 (loop body)
    def do_work(self):
        if self.get_serial_number() == 0 or not self.new_nonants:
            return
        innerbound = self.xhatter.xhat_tryit(verbose=self.verbose, restore_nonants=False,
                                             nonant_cache=self.localnonants)
        if self.update_if_improving(innerbound):
            self.best_xhat = {nd: v for nd, v in zip(self.opt.engine.node_names,
                                                     self.xhatter.last_table.cpu().numpy())}
