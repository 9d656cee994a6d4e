"""Sampling for multistage problems (mirrors mpisppy/confidence_intervals/sample_tree.py; DESIGN.md
3.24): ``SampleSubtree`` solves the extensive form of a sampled subtree whose ancestors' nonants are
fixed at a policy's values, ``walking_tree_xhats`` finds such a policy for every non-leaf node of a
sample tree.

The reference walks the tree node by node: one subtree extensive form after another on the host,
each waiting for its parent's.  All subtrees that start at the same stage are independent, and with
their fixed ancestors they have together the shape of the sample tree itself; only the data below
the stage differ per node.  So ``walking_tree_xhats`` solves a stage at once: ONE tree extensive form
over the model's ``sample_forest_batch_creator`` batch with every node above the stage held
(``ExtensiveForm.fix_node_nonants``, phgpu_eft_fix).  A D-stage tree takes D - 2 such solves whatever
its node count.

DEPARTURES.  The amalgamator is not restated: ``SampleSubtree`` carries what ``gap_estimators`` reads
off the reference's ``ama`` (``scenario_creator``, ``kwargs``, ``scenario_names``,
``best_outer_bound``) itself.  Its scenario names are the reference's (``seed`` .. ``seed`` +
numscens - 1) put in TREE order, i.e. sorted by scenario number modulo numscens, which is where the
model's demand sampler places them in the subtree; the extensive form needs every node's scenarios
contiguous.  ``mname`` may be the module itself.  An extensive form that does not reach its tolerance
raises RuntimeError.
"""
import time

import numpy as np

from ..sputils import extract_num, number_of_nodes, create_nodenames_from_branching_factors
from . import ciutils


class SampleSubtree:
    """sample_tree.py:18-158.  A scenario tree whose scenarios share the nodes of ``root_scen`` up to
    ``starting_stage`` t and are sampled below it (``branching_factors[t - 1:]``, ``seed``); the
    nonants of stages 1 .. t - 1 are fixed at ``xhats`` (one list of values per stage).  ``run()``
    solves its extensive form -- stage 1: the free tree extensive form; t > 1: the conditioned one
    -- and leaves ``xhat_at_stage`` (the stage-t node's nonants), ``EF_Obj`` and ``ef``."""

    def __init__(self, mname, xhats, root_scen, starting_stage, branching_factors, seed, cfg, solver_name=None,
                 solver_options=None):
        self.refmodel = ciutils.model_module(mname)
        for attr in ("sample_tree_scen_creator", "kw_creator", "scenario_names_creator"):
            if not hasattr(self.refmodel, attr):
                raise RuntimeError(f"The construction of a sample subtree failed because the reference model has no {attr} "
                                   f"function.")
        self.xhats = xhats
        self.root_scen = root_scen
        self.stage = int(starting_stage)
        self.sampling_branching_factors = list(branching_factors[self.stage - 1:])
        self.original_branching_factors = list(branching_factors)
        self.numscens = int(np.prod(self.sampling_branching_factors))
        self.seed = int(seed)
        self.solver_name = solver_name
        self.solver_options = solver_options
        self.fixed_nodes = ["ROOT" + "_0" * i for i in range(self.stage - 1)]
        over = {"num_scens": self.numscens, "EF_solver_name": solver_name}
        if "start_seed" not in ciutils.CfgView(cfg):
            over["start_seed"] = self.seed
        self.cfg = ciutils.CfgView(cfg, **over)
        if "branching_factors" not in self.cfg:
            raise RuntimeError("branching_factors is not in cfg")
        self.kwargs = self.refmodel.kw_creator(self.cfg)
        names = self.refmodel.scenario_names_creator(self.numscens, start=self.seed)
        self.scenario_names = sorted(names, key=lambda nm: extract_num(nm) % self.numscens)
        self.scenario_creator = self._sample_creator
        self.ef = self.EF_Obj = self.best_outer_bound = self.xhat_at_stage = None

    # sample_tree.py:79-112 (the fixing is the extensive form's, in run())
    def _sample_creator(self, sname, **scenario_creator_kwargs):
        kw = {k: v for k, v in scenario_creator_kwargs.items() if k != "seed"}     # (the seed is this object's)
        return self.refmodel.sample_tree_scen_creator(sname, given_scenario=self.root_scen, stage=self.stage,
                                                      sample_branching_factors=self.sampling_branching_factors,
                                                      seed=self.seed, **kw)

    def run(self):
        from ..opt.ef import ExtensiveForm
        from ..spopt import SOLVER_NAMES
        bfs = [1] * (self.stage - 1) + self.sampling_branching_factors
        nodenames = create_nodenames_from_branching_factors(bfs) if len(bfs) > 1 else None
        opts = {"solver": self.solver_name or SOLVER_NAMES[0], "toc": False, "device": self.cfg.get("device")}
        ef = ExtensiveForm(opts, self.scenario_names, self.scenario_creator, scenario_creator_kwargs=self.kwargs,
                           all_nodenames=nodenames)
        self.ef = ef
        if self.fixed_nodes:
            nlens = ef.batch.nlens()
            for k, nd in enumerate(self.fixed_nodes):
                if len(self.xhats[k]) != nlens[k]:
                    raise RuntimeError(f"xhats does not have the right size for stage {k + 1}, xhats has {len(self.xhats[k])} "
                                       f"nonant variables, but should have {nlens[k]} of them")
            ef.fix_node_nonants({nd: self.xhats[k] for k, nd in enumerate(self.fixed_nodes)})
        res = ef.solve_extensive_form(solver_options=self.solver_options)
        if res.solver.termination_condition != "optimal":
            raise RuntimeError(f"the extensive form of the sample subtree at stage {self.stage} (seed {self.seed}) was not "
                               f"solved to tol {ef.tol} in {ef.max_iter} iterations ({_where(ef)})")
        self.EF_Obj = self.best_outer_bound = ef.get_objective_value()
        pseudo_root = "ROOT" + "_0" * (self.stage - 1)
        self.xhat_at_stage = np.array(dict(ef.tree_nonants())[pseudo_root], dtype=np.float64)

    def close(self):
        if self.ef is not None and self.ef.engine is not None:
            self.ef.engine.close()


def _where(ef):
    """where an extensive form that did not converge stopped: its last iterate with a finite mu"""
    fin = [r for r in ef.history if np.isfinite(r["mu"])]
    if not fin:
        return "no iterate with a finite mu"
    r = fin[-1]
    end = "" if len(fin) == len(ef.history) else "; mu is not finite after it"
    return (f"iteration {int(r['iter'])}: primal {r['pres']:.1e} dual {r['dres']:.1e} gap {r['gap']:.1e} mu {r['mu']:.1e}"
            f"{end}")


def _feasible_solution(mname, scenario, xhat_one, branching_factors, seed, cfg, solver_name=None, solver_options=None):
    """sample_tree.py:161-184: non-anticipative feasible policies for the later stages of ONE
    scenario, stage by stage: ({node name: values}, the advanced seed)."""
    assert solver_name is not None
    if xhat_one is None:
        raise RuntimeError("Xhat_one can't be None for now")
    ciutils.is_sorted(scenario._mpisppy_node_list)
    nodenames = [node.name for node in scenario._mpisppy_node_list]
    xhats = [xhat_one]
    for t in range(2, len(branching_factors) + 1):          # (none for the final stage)
        subtree = SampleSubtree(mname, xhats, scenario, t, branching_factors, seed, cfg, solver_name, solver_options)
        try:
            subtree.run()
        finally:
            subtree.close()
        xhats.append(subtree.xhat_at_stage)
        seed += number_of_nodes(branching_factors[t - 1:])
    return {ndn: xhat for ndn, xhat in zip(nodenames, xhats)}, seed


def walk_seeds(local_scenarios, branching_factors, seed):
    """The seed the reference's walk (sample_tree.py:234-251) gives each node below ROOT, which needs
    no solve: scenario by scenario, a node met for the first time takes the current seed, which
    then advances by ``number_of_nodes(branching_factors[stage - 1:])``.  ({node name: seed}, the
    seed after the walk)."""
    seeds = {}
    for s in local_scenarios.values():
        ciutils.is_sorted(s._mpisppy_node_list)
        for node in s._mpisppy_node_list:
            if node.name != "ROOT" and node.name not in seeds:
                seeds[node.name] = seed
                seed += number_of_nodes(branching_factors[node.stage - 1:])
    return seeds, seed


def _balanced_in_tree_order(local_scenarios, branching_factors):
    """Whether the scenarios are the whole balanced tree over ``branching_factors`` in tree order."""
    bfs = list(branching_factors)
    scens = list(local_scenarios.values())
    if len(scens) != int(np.prod(bfs)):
        return False
    for i, s in enumerate(scens):
        if len(s._mpisppy_node_list) != len(bfs):
            return False
        name, rest = "ROOT", int(np.prod(bfs))
        for d, node in enumerate(s._mpisppy_node_list):
            if d:
                rest //= bfs[d - 1]
                name += f"_{(i // rest) % bfs[d - 1]}"
            if node.name != name:
                return False
    return True


def walking_tree_xhats(mname, local_scenarios, xhat_one, branching_factors, seed, cfg, solver_name=None,
                       solver_options=None, info=None, batched=True):
    """sample_tree.py:186-253: a feasible non-anticipative policy for every non-leaf node of the
    scenario tree ``local_scenarios`` ({name: scenario}) that starts from ``xhat_one`` at ROOT:
    ({node name: values}, the advanced seed).

    Every node's seed comes first, from the reference's own walk (``walk_seeds``).  The BATCHED walk
    then solves, for each stage t = 2 .. D - 1 in turn, all nodes of the stage in one conditioned
    extensive form with the stages before t held at the values found so far.  It needs a full
    BALANCED tree over ``branching_factors`` with the scenarios in tree order, a model module with
    ``sample_forest_batch_creator`` and scenarios that carry their ``demands``; any other scenario set
    (the reference allows unbalanced trees) falls back to one ``SampleSubtree`` per node, in the
    reference's order (``batched=False`` asks for that walk on any tree: the baseline of
    tools/mmw_ci.py).  A single scenario is ``_feasible_solution``'s, as in the reference.  ``info``
    (a dict) receives "batched", "iterations" (per conditioned solve), "seconds" and, from the batched
    walk, "node_objectives" {stage: [(node, its subtree's objective)]}."""
    assert xhat_one is not None, "Xhat_one can't be None for now"
    m = ciutils.model_module(mname)
    info = info if info is not None else {}
    info.update({"batched": False, "iterations": [], "seconds": [], "node_objectives": {}})
    xhats = {"ROOT": np.array(xhat_one, dtype=np.float64)}
    if len(local_scenarios) == 1:
        scen = list(local_scenarios.values())[0]
        return _feasible_solution(m, scen, xhats["ROOT"], branching_factors, seed, cfg, solver_name=solver_name,
                                  solver_options=solver_options)
    bfs = list(branching_factors)
    seeds, end_seed = walk_seeds(local_scenarios, bfs, seed)
    scens = list(local_scenarios.values())
    if (batched and hasattr(m, "sample_forest_batch_creator") and _balanced_in_tree_order(local_scenarios, bfs)
            and all(hasattr(s, "demands") for s in scens)):
        info["batched"] = True
        _batched_walk(m, scens, xhats, bfs, seeds, cfg, solver_name, solver_options, info)
        return xhats, end_seed
    for s in scens:                                      # the reference's walk, one subtree at a time
        scen_xhats = []
        for node in s._mpisppy_node_list:
            if node.name not in xhats:
                subtree = SampleSubtree(m, scen_xhats, s, node.stage, bfs, seeds[node.name], cfg, solver_name, solver_options)
                t0 = time.perf_counter()
                try:
                    subtree.run()
                    info["iterations"].append(subtree.ef.iterations)
                finally:
                    subtree.close()
                info["seconds"].append(time.perf_counter() - t0)
                xhats[node.name] = subtree.xhat_at_stage
            scen_xhats.append(xhats[node.name])
    return xhats, end_seed


def _batched_walk(m, scens, xhats, bfs, seeds, cfg, solver_name, solver_options, info):
    """One conditioned tree extensive form per stage 2 .. D - 1 (module docstring); fills ``xhats``."""
    from ..opt.ef import ExtensiveForm
    from ..spopt import SOLVER_NAMES
    lcfg = ciutils.CfgView(cfg)
    kwargs = dict(m.kw_creator(lcfg))
    kwargs["branching_factors"] = bfs               # (the sample tree's, not the cfg's)
    nodenames = create_nodenames_from_branching_factors(bfs)
    demands = [s.demands for s in scens]
    for t in range(2, len(bfs) + 1):
        stage_nodes = [nd for nd in nodenames if nd.count("_") == t - 1]
        batch = m.sample_forest_batch_creator(demands, t, [seeds[nd] for nd in stage_nodes], **kwargs)
        opts = {"solver": solver_name or SOLVER_NAMES[0], "toc": False, "device": lcfg.get("device"),
                "batch_creator": lambda names, _b=batch, **kw: _b}
        t0 = time.perf_counter()
        ef = ExtensiveForm(opts, list(batch.names), None, all_nodenames=nodenames)
        try:
            ef.fix_node_nonants({nd: v for nd, v in xhats.items() if nd.count("_") < t - 1})
            res = ef.solve_extensive_form(solver_options=solver_options)
            if res.solver.termination_condition != "optimal":
                raise RuntimeError(f"the conditioned extensive form of stage {t} ({len(stage_nodes)} subtrees) was not solved "
                                   f"to tol {ef.tol} in {ef.max_iter} iterations ({_where(ef)})")
            for nd, v in ef.tree_nonants():
                if nd.count("_") == t - 1:
                    xhats[nd] = np.array(v, dtype=np.float64)
            info["node_objectives"][t] = ef.node_objectives(t - 1)
            info["iterations"].append(ef.iterations)
        finally:
            if ef.engine is not None:
                ef.engine.close()
        info["seconds"].append(time.perf_counter() - t0)
