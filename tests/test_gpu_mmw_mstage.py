"""The multistage MMW gap estimators on the device (ciutils.gap_estimators with EF_mstage,
sample_tree.walking_tree_xhats, MMWConfidenceIntervals) on aircond sample trees
[3, 2] and [2, 2, 2]: the policy of every non-leaf node, the seeds, every subtree's objective against
HiGHS on that subtree alone, a subtree solved alone by SampleSubtree against the forest's value for
it, and G and s against host values."""
import numpy as np
import pytest

import ef_cond_ref as C
import ef_tree_ref as R

pytestmark = pytest.mark.gpu

REL = 1e-5
SEED, XHAT_SEED = 100, 4000
TREES = [(3, 2), (2, 2, 2)]
_EST = {}


def _cfg(bfs):
    return {"branching_factors": list(bfs), "EF_mstage": True, "EF_solver_name": R.SOLVER, "device": "cuda:0"}


def _sample_tree(bfs, seed):
    """The sample tree at ``seed`` on the host: ({name: model} in tree order, its batch)."""
    from mpisppy_amd.batch import batch_from_models
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    S = int(np.prod(bfs))
    names = sorted(aircond.scenario_names_creator(S, start=seed), key=lambda nm: int(nm[4:]) % S)
    kw = aircond.kw_creator(_cfg(bfs))
    scens = {nm: aircond.sample_tree_scen_creator(nm, 1, list(bfs), seed, **kw) for nm in names}
    nonleaf = [nd for nd in create_nodenames_from_branching_factors(list(bfs)) if nd.count("_") < len(bfs)]
    return scens, batch_from_models(names, list(scens.values()), node_names=nonleaf), kw


def _estimate(bfs):
    """One gap estimate per tree, shared by the tests: (xhat_one, the estimators, info)."""
    from mpisppy_amd.confidence_intervals import ciutils
    from mpisppy_amd.examples import aircond
    if bfs not in _EST:
        S = int(np.prod(bfs))
        xhat_one = ciutils.ef_xstar_solver(aircond, solver_name=R.SOLVER, device="cuda:0")(
            aircond.scenario_names_creator(S), {"branching_factors": list(bfs), "start_seed": XHAT_SEED})
        info = {}
        est = ciutils.gap_estimators({"ROOT": xhat_one}, aircond, solving_type="EF_mstage",
                                     sample_options={"branching_factors": list(bfs), "seed": SEED}, cfg=_cfg(bfs),
                                     solver_name=R.SOLVER, info=info)
        _EST[bfs] = (xhat_one, est, info)
    return _EST[bfs]


@pytest.mark.parametrize("bfs", TREES)
def test_policy_seeds_and_subtree_objectives(gpu, bfs):
    from mpisppy_amd.confidence_intervals import sample_tree
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.sputils import number_of_nodes
    xhat_one, est, info = _estimate(bfs)
    xhats, walk = info["xhats"], info["walk"]
    scens, b, kw = _sample_tree(bfs, SEED)
    assert walk["batched"] and len(walk["iterations"]) == len(bfs) - 1
    assert set(xhats) == set(b.node_names)                                        # every non-leaf node
    assert np.array_equal(np.asarray(xhats["ROOT"]).view(np.int64), xhat_one.view(np.int64))
    seeds, end = sample_tree.walk_seeds(scens, list(bfs), SEED + number_of_nodes(list(bfs)))
    assert est["seed"] == end
    # every stage-2 subtree: the forest's value for it against HiGHS on that subtree alone
    models = list(scens.values())
    stage2 = [nd for nd in b.node_names if nd.count("_") == 1]
    fb = aircond.sample_forest_batch_creator([m.demands for m in models], 2, [seeds[nd] for nd in stage2],
                                             **{**kw, "branching_factors": list(bfs)})
    lay = R.Layout(fb)
    zfix = C.zfix_of(lay, fb.node_names, {"ROOT": xhat_one})
    got = dict(walk["node_objectives"][2])
    for nd in stage2:
        ok, want, _ = C.cond_optimum(fb, zfix, lay, scen=lay.scenarios(list(fb.node_names).index(nd)))
        print(f"{bfs} subtree {nd} (seed {seeds[nd]}): forest {got[nd]:.8f} HiGHS alone {want:.8f}")
        assert ok and abs(got[nd] - want) <= REL * abs(want)


def test_a_stage_three_subtree_alone_gives_the_forests_value(gpu):
    from mpisppy_amd.confidence_intervals import sample_tree
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.sputils import number_of_nodes
    bfs = (2, 2, 2)
    xhat_one, est, info = _estimate(bfs)
    xhats, walk = info["xhats"], info["walk"]
    scens, b, _ = _sample_tree(bfs, SEED)
    seeds, _ = sample_tree.walk_seeds(scens, list(bfs), SEED + number_of_nodes(list(bfs)))
    nd = "ROOT_1_0"
    root_scen = next(m for m in scens.values() if m._mpisppy_node_list[2].name == nd)
    sub = sample_tree.SampleSubtree(aircond, [xhat_one, xhats["ROOT_1"]], root_scen, 3, list(bfs), seeds[nd], _cfg(bfs),
                                    solver_name=R.SOLVER)
    try:
        sub.run()
        want = dict(walk["node_objectives"][3])[nd]
        print(f"stage-3 subtree {nd} alone: EF_Obj {sub.EF_Obj:.8f}, the forest's {want:.8f}; policy {sub.xhat_at_stage} "
              f"forest {xhats[nd]}")
        assert abs(sub.EF_Obj - want) <= REL * abs(want)
        held = dict(sub.ef.tree_nonants())
        assert np.array_equal(held["ROOT"], xhat_one) and np.array_equal(held["ROOT_0"], xhats["ROOT_1"])
    finally:
        sub.close()


@pytest.mark.parametrize("bfs", TREES)
def test_G_and_s_against_host_values(gpu, bfs):
    """G: the mean objective with every nonant fixed at the device's policy, scenario by scenario by
    HiGHS, minus HiGHS's optimum of the sample tree; two objectives, each good to REL.  s: the
    reference's formula on the device's own per-scenario objectives (the optimum's per-scenario
    objectives are not unique, so none from HiGHS)."""
    xhat_one, est, info = _estimate(bfs)
    scens, b, _ = _sample_tree(bfs, SEED)
    lay = R.Layout(b)
    zn_star, _ = R.ef_tree_optimum(b, lay)
    zfix = C.zfix_of(lay, b.node_names, info["xhats"])
    assert not np.any(np.isnan(zfix))
    zhat = 0.0
    for s in range(b.S):
        ok, f, _ = C.cond_optimum(b, zfix, lay, scen=[s])
        assert ok
        zhat += b.prob[s] * f
    G_host = zhat - zn_star
    print(f"{bfs}: G {est['G']:.8f} host {G_host:.8f} (zn_star {zn_star:.6f}, device {info['zn_star']:.6f}); s {est['s']:.8f}; "
          f"iterations {info['iterations']}; seconds {info['seconds']}")
    assert abs(info["zn_star"] - zn_star) <= REL * abs(zn_star)
    assert abs(est["G"] - G_host) <= 2 * REL * abs(zn_star)
    assert est["G"] >= -2 * REL * abs(zn_star)
    gaps = info["f_hat"] - info["f_star"]
    p = b.prob
    Gd, ssq = float(gaps @ p), float((gaps ** 2) @ p)
    s_host = np.sqrt((ssq - Gd ** 2) / (1.0 - float(p @ p)))
    assert abs(est["s"] - s_host) <= 1e-10 * abs(s_host)


def test_mmw_interval_runs_the_batches_in_sequence(gpu):
    from mpisppy_amd.confidence_intervals import ciutils, mmw_ci
    from mpisppy_amd.examples import aircond
    bfs = (3, 2)
    xhat_one, _, _ = _estimate(bfs)
    cfg = _cfg(bfs)
    mmw = mmw_ci.MMWConfidenceIntervals(aircond, cfg, {"ROOT": xhat_one}, 3, batch_size=6, start=SEED, verbose=False)
    assert mmw.type == "EF_mstage" and mmw.multistage and mmw.numstages == 3
    info = {}
    r = mmw.run(info=info)
    assert set(r) == {"gap_inner_bound", "gap_outer_bound", "Gbar", "std", "Glist"} and len(r["Glist"]) == 3
    sbf = ciutils.branching_factors_from_numscens(6, 3)
    assert sbf == [2, 3]
    seed = SEED
    for i in range(3):
        est = ciutils.gap_estimators({"ROOT": xhat_one}, aircond, solving_type="EF_mstage",
                                     sample_options={"branching_factors": sbf, "seed": seed}, cfg=cfg, solver_name=R.SOLVER)
        assert np.array_equal(np.float64(est["G"]).view(np.int64), np.float64(r["Glist"][i]).view(np.int64)), i
        assert info["batches"][i]["seed"] == est["seed"] and info["batches"][i]["s"] == est["s"]
        seed = est["seed"]
    assert r["Gbar"] == np.mean(r["Glist"]) and r["gap_inner_bound"] >= r["Gbar"]


def test_the_walk_one_subtree_at_a_time_and_for_one_scenario(gpu):
    """What a scenario set that is no balanced tree in tree order gets: the reference's walk, one
    SampleSubtree per node (asked for on a balanced tree, and by itself on the same scenarios out of
    tree order): the nodes and the seed of the batched walk; and the reference's special case of a
    single scenario."""
    from mpisppy_amd.confidence_intervals import sample_tree
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.sputils import number_of_nodes
    bfs = (2, 2, 2)
    xhat_one, est, info = _estimate(bfs)
    scens, b, _ = _sample_tree(bfs, SEED)
    start = SEED + number_of_nodes(list(bfs))
    walk = {}
    xh, end = sample_tree.walking_tree_xhats(aircond, scens, xhat_one, list(bfs), start, _cfg(bfs), solver_name=R.SOLVER,
                                             info=walk, batched=False)
    assert not walk["batched"] and len(walk["iterations"]) == 6 and end == est["seed"]
    assert set(xh) == set(info["xhats"]) and np.array_equal(xh["ROOT"], xhat_one)
    rev = dict(reversed(list(scens.items())))                # not in tree order: the fallback by itself
    walk2 = {}
    xr, end2 = sample_tree.walking_tree_xhats(aircond, rev, xhat_one, list(bfs), start, _cfg(bfs), solver_name=R.SOLVER, info=walk2)
    assert not walk2["batched"] and set(xr) == set(xh) and end2 == end
    one = dict(list(scens.items())[5:6])
    x1, end1 = sample_tree.walking_tree_xhats(aircond, one, xhat_one, list(bfs), start, _cfg(bfs), solver_name=R.SOLVER)
    assert list(x1) == ["ROOT", "ROOT_1", "ROOT_1_0"] and np.array_equal(x1["ROOT"], xhat_one)
    assert end1 == start + number_of_nodes([2, 2]) + number_of_nodes([2])
