"""Slam heuristics (mirrors mpisppy/cylinders/slam_heuristic.py:24-125; two-stage only).

The candidate is the column-wise maximum (SlamMaxHeuristic) or minimum (SlamMinHeuristic) of
the hub's nonants over all scenarios: numpy_op over the local scenarios (:57-67), then an
Allreduce with mpi.MAX / mpi.MIN (:84).  Here both come from engine.nonant_stats -- plane 3 is
the maximum, plane 2 the negated minimum, reduced over the ranks by one MAX all-reduce.  The
candidate is fixed in every scenario (:92-99) and evaluated by
``calculate_incumbent(fix_nonants=False)`` (:101); no rounding (continuous nonants).
"""
from .spoke import InnerBoundNonantSpoke
from ..utils.xhat_eval import Xhat_Eval


class _SlamHeuristic(InnerBoundNonantSpoke):
    converger_spoke_char = "S"

    def candidate(self, planes):
        """Device [num_nodes, nlen_max] candidate from the planes of engine.nonant_stats."""
        raise NotImplementedError

    # :38-55
    def slam_heur_prep(self):
        if self.opt.multistage:
            raise RuntimeError(f"The {self.__class__.__name__} only supports "
                               "two-stage models at this time.")
        if not isinstance(self.opt, Xhat_Eval):
            raise RuntimeError(f"{self.__class__.__name__} must be used with Xhat_Eval.")
        self.verbose = self.opt.options["verbose"]
        self.opt._lazy_create_solvers()
        self.opt._update_E1()

    # :69-70 (set-up part of main)
    def main(self):
        self.slam_heur_prep()

    # :78-103 (loop body)
    def do_work(self):
        if self.get_serial_number() == 0 or not self.new_nonants:
            return
        cand = self.candidate(self.opt.engine.nonant_stats(self.localnonants)).clone()
        self.opt._fix_nonants(cand)
        obj = self.opt.calculate_incumbent(fix_nonants=False)
        if self.update_if_improving(obj):
            self.best_xhat = {nd: v for nd, v in zip(self.opt.engine.node_names, cand.cpu().numpy())}


class SlamMaxHeuristic(_SlamHeuristic):
    def candidate(self, planes):
        return planes[3]


class SlamMinHeuristic(_SlamHeuristic):
    def candidate(self, planes):
        return -planes[2]
