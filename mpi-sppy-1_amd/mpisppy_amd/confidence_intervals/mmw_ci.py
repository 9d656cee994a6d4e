"""The Mak-Morton-Wood confidence interval on the optimality gap of a candidate (mirrors
mpisppy/confidence_intervals/mmw_ci.py:31-185).  ``run`` is ONE ``ciutils.gap_estimators_batched``
call: the reference's loop over the batches (mmw_ci.py:144-166) becomes two batched solves over
num_batches * batch_size scenarios.  With ``EF_mstage`` (a multistage model) the batches run in
sequence, each a ``ciutils.gap_estimators(solving_type="EF_mstage")`` call on a sample tree of about
``batch_size`` leaves that takes the seed the previous one returned (mmw_ci.py:144-166).

DEPARTURE.  ``EF_mstage`` with a model module that has no ``sample_tree_scen_creator`` raises
NotImplementedError naming it, at construction (the reference: RuntimeError, at the first batch)."""
import numpy as np

from . import ciutils


def remove_None(d):
    return {} if d is None else {k: v for k, v in d.items() if v is not None}


class MMWConfidenceIntervals:
    """``refmodel``: a model module or its dotted name; ``cfg``: the options (``EF_2stage`` or
    ``EF_mstage`` True, ``EF_solver_name``, optionally ``EF_solver_options``, and what the module's
    ``kw_creator`` reads; ``EF_mstage`` needs ``branching_factors``, whose length gives the number of
    stages); ``xhat_one``: {"ROOT": candidate}; ``num_batches`` batches of ``batch_size`` scenarios
    numbered from ``start``."""

    def __init__(self, refmodel, cfg, xhat_one, num_batches, batch_size=None, start=None, verbose=True,
                 mpicomm=None):
        self.refmodel = ciutils.model_module(refmodel)
        self.refmodelname = refmodel
        self.cfg = ciutils.CfgView(cfg)
        self.xhat_one = xhat_one
        self.num_batches = num_batches
        self.batch_size = batch_size
        self.verbose = verbose
        self.mpicomm = mpicomm
        self.xstar_solver = None        # a caller's own x* (ciutils.gap_estimators_batched); None: L-shaped
        if start is None:
            raise RuntimeError("Start must be specified")
        self.start = start
        if self.cfg.get("EF_2stage", False):
            self.type, self.multistage, self.numstages = "EF_2stage", False, 2
        elif self.cfg.get("EF_mstage", False):
            if not hasattr(self.refmodel, "sample_tree_scen_creator"):
                raise NotImplementedError(f"EF_mstage needs a model module with sample_tree_scen_creator (sample_tree.py); "
                                          f"{getattr(self.refmodel, '__name__', refmodel)} has none")
            if "branching_factors" not in self.cfg:
                raise RuntimeError("EF_mstage needs branching_factors in cfg")
            self.type, self.multistage = "EF_mstage", True
            self.numstages = len(self.cfg["branching_factors"]) + 1
        else:
            raise RuntimeError("Only EF is currently supported; cfg should have an attribute 'EF-2stage' or "
                               "'EF-mstage' set to True")
        complete = True
        for fct in ("scenario_names_creator", "scenario_creator", "kw_creator"):
            if not hasattr(self.refmodel, fct):
                print(f"Module {refmodel} is missing {fct}")
                complete = False
        if not complete:
            raise RuntimeError(f"Module {refmodel} not complete for MMW")
        if "EF_solver_name" not in self.cfg:
            raise RuntimeError("EF_solver_name not in Argument list for MMW")

    def run(self, confidence_level=0.95, info=None):
        batch_size = self.batch_size if self.batch_size is not None else self.cfg.get("num_scens")
        if not batch_size:
            raise RuntimeError("batch size can't be zero for two stage problems")
        if self.multistage:
            return self._run_mstage(batch_size, confidence_level, info)
        est = ciutils.gap_estimators_batched(
            self.xhat_one, self.refmodel, self.num_batches, batch_size, self.start, ArRP=1, cfg=self.cfg,
            scenario_denouement=getattr(self.refmodel, "scenario_denouement", None),
            solver_name=self.cfg["EF_solver_name"], solver_options=remove_None(self.cfg.get("EF_solver_options")),
            verbose=self.verbose, mpicomm=self.mpicomm, xstar_solver=self.xstar_solver, info=info)
        return self._interval(np.array(est["G"], dtype=np.float64), confidence_level)

    def _run_mstage(self, batch_size, confidence_level, info):
        """mmw_ci.py:144-166 with ``EF_mstage``: one sample tree per batch, the seed handed on."""
        bfs = ciutils.branching_factors_from_numscens(batch_size, self.numstages)
        seed, G = self.start, []
        if info is not None:
            info["batches"] = []
        for _ in range(self.num_batches):
            one = {} if info is not None else None
            est = ciutils.gap_estimators(self.xhat_one, self.refmodel, solving_type=self.type,
                                         sample_options={"branching_factors": bfs, "seed": seed}, cfg=self.cfg,
                                         scenario_denouement=getattr(self.refmodel, "scenario_denouement", None),
                                         solver_name=self.cfg["EF_solver_name"],
                                         solver_options=remove_None(self.cfg.get("EF_solver_options")),
                                         verbose=self.verbose, mpicomm=self.mpicomm, info=one)
            seed = est["seed"]
            G.append(est["G"])
            if info is not None:
                info["batches"].append({"G": est["G"], "s": est["s"], "seed": seed, **one})
        return self._interval(np.array(G, dtype=np.float64), confidence_level)

    def _interval(self, G, confidence_level):
        s_g = np.std(G)                                  # ddof 0, as mmw_ci.py:168
        Gbar = np.mean(G)
        t_g = ciutils.t_ppf(confidence_level, self.num_batches - 1)
        epsilon_g = t_g * s_g / np.sqrt(self.num_batches)
        self.result = {"gap_inner_bound": Gbar + epsilon_g, "gap_outer_bound": 0, "Gbar": Gbar, "std": s_g,
                       "Glist": G}
        return self.result
