"""Multistage sampling without a GPU (confidence_intervals/sample_tree.py): the seeds
of the walk against a transcription of the reference's loop, aircond's sample-tree scenario creator
and its vectorised forest form, and the branching-factor utilities."""
import types

import numpy as np
import pytest

from mpisppy_amd.batch import batch_from_models
from mpisppy_amd.confidence_intervals import ciutils, sample_tree
from mpisppy_amd.examples import aircond
from mpisppy_amd.sputils import number_of_nodes

BFS = [[3, 2], [2, 2, 2], [2, 3, 2]]


def _tree(bfs, seed=0):
    names = aircond.scenario_names_creator(int(np.prod(bfs)))
    kw = {"branching_factors": list(bfs), "start_seed": seed}
    return {nm: aircond.scenario_creator(nm, **kw) for nm in names}, kw


# ------------------------------------------------------------------ the seeds of the walk
def _reference_walk(local_scenarios, branching_factors, seed):
    """sample_tree.py:234-251 with the solve left out: which seed each SampleSubtree is built with."""
    xhats, used = {"ROOT": None}, {}
    for k, s in local_scenarios.items():
        for node in s._mpisppy_node_list:
            if node.name in xhats:
                pass
            else:
                used[node.name] = seed
                seed += number_of_nodes(branching_factors[(node.stage - 1):])
                xhats[node.name] = None
    return used, seed


@pytest.mark.parametrize("bfs", BFS)
def test_walk_seeds_are_the_reference_walks(bfs):
    scens, _ = _tree(bfs)
    start = 1000
    seeds, end = sample_tree.walk_seeds(scens, bfs, start)
    want, want_end = _reference_walk(scens, bfs, start)
    assert seeds == want and end == want_end
    nonleaf_below_root = [nd.name for s in scens.values() for nd in s._mpisppy_node_list[1:]]
    assert set(seeds) == set(nonleaf_below_root)
    total = sum(number_of_nodes(bfs[nd.count("_"):]) for nd in seeds)
    assert end == start + total
    assert sample_tree._balanced_in_tree_order(scens, bfs)
    rev = dict(reversed(list(scens.items())))
    assert not sample_tree._balanced_in_tree_order(rev, bfs)
    assert not sample_tree._balanced_in_tree_order(dict(list(scens.items())[:-1]), bfs)


def test_number_of_nodes():
    assert number_of_nodes([2]) == 2 and number_of_nodes([3, 2]) == 9 and number_of_nodes([2, 2, 2]) == 14


# ------------------------------------------------------------------ sample_tree_scen_creator
def test_sample_tree_scen_creator_stage_one_is_the_scenario_creator():
    bfs, seed = [3, 2], 77
    kw = {"branching_factors": bfs, "start_seed": 5}
    for nm in aircond.scenario_names_creator(6, start=seed):
        a = aircond.sample_tree_scen_creator(nm, 1, bfs, seed, **kw)
        b = aircond.scenario_creator(nm, branching_factors=bfs, start_seed=seed)
        assert a.demands == b.demands
        assert [n.name for n in a._mpisppy_node_list] == [n.name for n in b._mpisppy_node_list]
        assert [n.cond_prob for n in a._mpisppy_node_list] == [1.0, 1.0 / 3]
        assert a._mpisppy_probability == 1.0 / 6


@pytest.mark.parametrize("bfs,stage", [([3, 2], 2), ([2, 2, 2], 2), ([2, 2, 2], 3)])
def test_sample_tree_scen_creator_keeps_the_past_and_samples_the_future(bfs, stage):
    scens, kw = _tree(bfs)
    given = list(scens.values())[-1]
    seed, sub = 300, bfs[stage - 1:]
    root_name = "ROOT" + "_0" * (stage - 1)
    for nm in aircond.scenario_names_creator(int(np.prod(sub)), start=seed):
        mdl = aircond.sample_tree_scen_creator(nm, stage, sub, seed, given_scenario=given, **kw)
        fut, nodenames = aircond.demands_creator(nm, sub, root_name=root_name, **{**aircond.PARMS, "start_seed": seed})
        assert mdl.demands[:stage] == given.demands[:stage]
        assert mdl.demands[stage:] == fut[1:] and len(mdl.demands) == len(bfs) + 1
        assert fut[0] == aircond.PARMS["starting_d"]             # (the walk restarts there, as in the reference)
        names = [n.name for n in mdl._mpisppy_node_list]
        want = ["ROOT" + "_0" * i for i in range(stage)]
        for d in nodenames[1:-1]:
            want.append(want[-1] + "_" + d)
        assert names == want and len(names) == len(bfs)
        assert [n.cond_prob for n in mdl._mpisppy_node_list] == [1.0] * stage + [1.0 / f for f in sub[:-1]]
        assert [n.stage for n in mdl._mpisppy_node_list] == list(range(1, len(bfs) + 1))
        assert mdl._mpisppy_probability == 1.0 / np.prod(sub)
        ciutils.is_sorted(mdl._mpisppy_node_list)
    with pytest.raises(RuntimeError, match="given_scenario"):
        aircond.sample_tree_scen_creator("scen0", stage, sub, seed, **kw)


def test_kw_creator_and_denouement():
    kw = aircond.kw_creator({"branching_factors": [3, 2], "start_seed": 9, "Capacity": None})
    assert kw["branching_factors"] == [3, 2] and kw["start_seed"] == 9 and kw["Capacity"] == aircond.PARMS["Capacity"]
    assert set(kw) == set(aircond.PARMS) | {"branching_factors"}
    ns = types.SimpleNamespace(branching_factors=[2, 2], sigma_dev=10.0)
    assert aircond.kw_creator(ns)["sigma_dev"] == 10.0
    assert aircond.kw_creator(ns, {"sigma_dev": 3.0})["sigma_dev"] == 3.0
    assert aircond.kw_creator(ns, {"kwargs": {"a": 1}}) == {"a": 1}
    assert aircond.scenario_denouement(0, "scen0", None) is None


# ------------------------------------------------------------------ the forest of one stage
@pytest.mark.parametrize("bfs,stage", [([3, 2], 2), ([2, 2, 2], 3), ([2, 2, 2], 2)])
def test_sample_forest_batch_equals_the_single_models(bfs, stage):
    """Array for array the batch of the individual sample_tree_scen_creator models; the nodes and
    probabilities are the sample tree's (a subtree's own are these over its node's)."""
    scens, kw = _tree(bfs)
    models = list(scens.values())
    S, sub = len(models), int(np.prod(bfs[stage - 1:]))
    seeds = [500 + 13 * j for j in range(S // sub)]                  # (13: the names wrap around inside a subtree)
    fb = aircond.sample_forest_batch_creator([m.demands for m in models], stage, seeds, **kw)
    single = []
    for j, seed in enumerate(seeds):
        nums = sorted(range(seed, seed + sub), key=lambda k: k % sub)
        assert fb.names[j * sub:(j + 1) * sub] == [f"scen{k}" for k in nums]
        single += [aircond.sample_tree_scen_creator(f"scen{k}", stage, bfs[stage - 1:], seed, given_scenario=models[j * sub], **kw)
                   for k in nums]
    bb = batch_from_models(fb.names, single)
    for k in ("row_ptr", "col_idx", "A_val", "c", "q", "lb", "ub", "rl", "ru", "obj_const", "nonant_col", "nonant_depth",
              "nonant_off"):
        assert np.array_equal(np.asarray(getattr(fb, k)), np.asarray(getattr(bb, k))), k
    assert np.array_equal(fb.demands, np.array([m.demands for m in single]))
    tree = aircond.batch_creator(list(scens), **kw)
    assert np.array_equal(fb.node_of, tree.node_of) and list(fb.node_names) == list(tree.node_names)
    assert np.array_equal(fb.prob, tree.prob) and np.array_equal(fb.prob_coeff, tree.prob_coeff)
    assert np.allclose(fb.prob * (S // sub), bb.prob, rtol=1e-15)
    with pytest.raises(RuntimeError, match="no subtrees to sample"):
        aircond.sample_forest_batch_creator([m.demands for m in models], 1, seeds, **kw)
    with pytest.raises(RuntimeError, match="seeds for"):
        aircond.sample_forest_batch_creator([m.demands for m in models], stage, seeds[:-1], **kw)


# ------------------------------------------------------------------ branching factors
def test_branching_factor_utilities():
    assert ciutils.scalable_branching_factors(233, [5, 3, 2]) == [10, 6, 4]          # the reference's own example
    assert ciutils.scalable_branching_factors(7, [5, 3, 2]) == [2, 2, 2]             # numscens < 2 ** (stages - 1)
    assert ciutils.scalable_branching_factors(30, [5, 3, 2]) == [5, 3, 2]
    assert ciutils.branching_factors_from_numscens(100, 2) is None
    assert ciutils.branching_factors_from_numscens(6, 3) == [2, 3]
    assert ciutils.branching_factors_from_numscens(8, 4) == [2, 2, 2]
    assert ciutils.branching_factors_from_numscens(7, 4) == [2, 2, 2]                # 7 is prime: 8 is the first that splits
    assert ciutils.branching_factors_from_numscens(24, 3) == [4, 6]                  # 2 2 2 3 dealt round-robin
    for n, st in [(6, 3), (30, 3), (97, 4), (1000, 4)]:
        bf = ciutils.branching_factors_from_numscens(n, st)
        assert len(bf) == st - 1 and n <= int(np.prod(bf)) < n + 2 ** (st - 1) and min(bf) >= 2


# ------------------------------------------------------------------ what SampleSubtree asks of a module
def test_sample_subtree_construction():
    cfg = {"branching_factors": [2, 2, 2], "EF_mstage": True}
    t = sample_tree.SampleSubtree(aircond, [], None, 1, [2, 3, 2], 40, cfg, solver_name="mi355x_pdhg")
    assert t.numscens == 12 and t.sampling_branching_factors == [2, 3, 2] and t.fixed_nodes == []
    assert sorted(t.scenario_names) == sorted(aircond.scenario_names_creator(12, start=40))
    assert [int(nm[4:]) % 12 for nm in t.scenario_names] == list(range(12))          # tree order
    assert t.kwargs["start_seed"] == 40 and t.scenario_creator == t._sample_creator
    mdl = t.scenario_creator(t.scenario_names[0], **t.kwargs)
    assert mdl.demands == aircond.scenario_creator(t.scenario_names[0], branching_factors=[2, 3, 2], start_seed=40).demands
    t3 = sample_tree.SampleSubtree(aircond, [[1.0, 2.0], [3.0, 4.0]], mdl, 3, [2, 3, 2], 90, cfg, solver_name="mi355x_pdhg")
    assert t3.fixed_nodes == ["ROOT", "ROOT_0"] and t3.numscens == 2 and t3.sampling_branching_factors == [2]
    with pytest.raises(RuntimeError, match="no sample_tree_scen_creator function"):
        from mpisppy_amd.examples import farmer
        sample_tree.SampleSubtree(farmer, [], None, 1, [2, 2], 0, cfg)
    with pytest.raises(RuntimeError, match="branching_factors is not in cfg"):
        sample_tree.SampleSubtree(aircond, [], None, 1, [2, 2], 0, {})
    with pytest.raises(RuntimeError, match="sample_options must be a dict"):
        ciutils.gap_estimators({"ROOT": [1.0, 2.0]}, aircond, solving_type="EF_mstage", cfg=cfg)
