"""XhatClosest: the scenario closest to x̄ as the xhat candidate (mirrors
mpisppy/extensions/xhatclosest.py:10-112; two-stage only, :91-93).

The reference sums, per local scenario, the truncated z-scores min(3, |x - x̄| / stdev) of the
nonants with positive variance x̄² - x̄ x̄ (:37-45), keeps the first scenario with the smallest
sum (:46-51), agrees on the winner over the ranks (MIN of the distance, then MAX of the rank
among those attaining it, :53-65), broadcasts its name and tries it (:75-83).  Here the
distances and the local winner are one kernel (engine.closest_scenario), the agreement its
MAX all-reduces, and the try is XhatBase._try_one's batched fixed-nonant solve.
"""
from .extension import Extension
from .xhatbase import XhatBase


class XhatClosest(XhatBase):
    def __init__(self, ph):
        super().__init__(ph)
        self.options = ph.options["xhat_closest_options"]
        self.solver_options = self.options.get("xhat_solver_options")
        self.keep_solution = bool(self.options.get("keep_solution", True))
        self.verbose = ph.options.get("verbose", False)

    # xhatclosest.py:23-89
    def xhat_closest_to_xbar(self, verbose=False, restore_nonants=True, nonant_cache=None, xbar_node=None,
                             xsqbar_node=None):
        """(objective or None, {"ROOT": scenario name}).  ``nonant_cache``: device [nn, S_local]
        (default: the nonants of the last solve).  ``xbar_node`` / ``xsqbar_node``: device
        [nlen_max]; by default the x̄ / x̄² in a PH object's node_buf (the reference's xbars /
        xsqbars Params), and for an object without them those of ``nonant_cache`` itself."""
        def _vb(msg):
            if verbose and self.cylinder_rank == 0:
                print("(rank0) xhat_looper: " + msg)

        e = self.opt.engine
        if nonant_cache is None:
            nonant_cache = e.nonant_x_dev()
        if xbar_node is None:
            if hasattr(self.opt, "Compute_Xbar"):
                e._flush_xbar()
                half = e.num_nodes * e.nlen_max
                xbar_node, xsqbar_node = e.node_buf[:half], e.node_buf[half:]
            else:
                planes = e.nonant_stats(nonant_cache)
                xbar_node, xsqbar_node = planes[0, 0], planes[1, 0]
        _, rank, li = e.closest_scenario(nonant_cache, xbar_node, xsqbar_node)
        sname = self.opt.all_scenario_names[self._slices[rank][li]]
        self.closest_name = sname
        _vb("Trying scenario " + sname)
        _vb("   Solver options=" + str(self.solver_options))
        snamedict = {"ROOT": sname}
        obj = self._try_one(snamedict, solver_options=self.solver_options, verbose=False,
                            restore_nonants=restore_nonants, nonant_cache=nonant_cache)
        _vb("    Infeasible" if obj is None else "    Feasible, returning " + str(obj))
        return obj, snamedict

    # xhatclosest.py:91-93
    def pre_iter0(self):
        if self.opt.multistage:
            raise RuntimeError("xhatclosest not done for multi-stage")

    # the loop hooks the reference defines as no-ops: the base class's own, so the PH loop
    # sees nothing to call and keeps its speculative solve
    miditer = Extension.miditer
    enditer = Extension.enditer

    # xhatclosest.py:105-112
    def post_everything(self):
        restore_nonants = not self.keep_solution
        self.opt.disable_W_and_prox()
        obj, srcsname = self.xhat_closest_to_xbar(verbose=self.verbose, restore_nonants=restore_nonants)
        self.opt.reenable_W_and_prox()
        self._final_xhat_closest_obj = obj
        self._final_xhat_closest_name = srcsname["ROOT"]
