"""Frank-Wolfe outer bound spoke (mirrors mpisppy/cylinders/fwph_spoke.py:5-34).

A bounds-only spoke: it takes nothing from the hub (Hub.initialize_spoke_indices puts it in
``bounds_only_indices``) and runs its own dual ascent, FWPH, next to it.  The reference's
``main`` is ``opt.fwph_main()``, whose loop calls the spoke's ``sync`` once per outer
iteration; with this project's scheduling (cylinders/spoke.py) ``main`` is ``fw_prep`` and the
first bound, ``do_work`` one outer iteration followed by what ``sync`` does there, and
``finalize`` the reference's.  On its own ranks ``Spoke.run_remote`` drives the same two.
"""
from .spoke import OuterBoundSpoke


class FrankWolfeOuterBound(OuterBoundSpoke):
    converger_spoke_char = "F"

    # fwph_spoke.py:9-10 with fwph.py:142-150
    def main(self):
        opt = self.opt
        self._best = opt.fw_prep()
        self._itr = 0
        self._done = False
        if getattr(opt, "trivial_bound_converged", True):
            opt._local_bound = self._best
            self.bound = self._best

    # fwph_spoke.py:12-13
    def is_converged(self):
        return self._killed if self._remote else self.got_kill_signal()

    # fwph_spoke.py:15-23
    def sync(self):
        if getattr(self.opt, "_local_bound", None) is None:
            return
        self.bound = self.opt._local_bound

    # one pass of fwph_main's loop body (fwph.py:152-203)
    def do_work(self):
        opt = self.opt
        if self._done or self._itr >= opt.options["PHIterLimit"]:
            return
        self._best, self._done = opt.fw_step(self._itr, self._best)
        self._itr += 1
        self.sync()

    # fwph_spoke.py:25-34
    def finalize(self):
        if getattr(self.opt, "_local_bound", None) is None:
            self.final_bound = self.bound
            return self.final_bound
        self.bound = self.opt._local_bound
        self.final_bound = self.opt._local_bound
        return self.final_bound
