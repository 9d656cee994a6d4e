"""The L-shaped method without a GPU: the numpy restatement (tests/lshaped_ref.py) against the
extensive form, its bounds and cuts, and the option checks of mpisppy_amd.opt.lshaped."""
import numpy as np
import pytest

import lshaped_ref as R
from oracle.models import farmer_scenario

_RUNS = {}


def _run(S, G=None):
    if (S, G) not in _RUNS:
        scens = [farmer_scenario(f"scen{i}", 1, num_scens=S) for i in range(S)]
        ref = R.LShapedRef(scens, G=G, tol=1e-12)
        done = ref.run()
        _RUNS[(S, G)] = (ref, done, R.ef_optimum(scens))
    return _RUNS[(S, G)]


@pytest.mark.parametrize("S,G", [(3, None), (12, None), (30, None), (30, 8), (3, 1)])
def test_restatement_reaches_the_ef_optimum(S, G):
    ref, done, (ef_obj, _) = _run(S, G)
    print(f"farmer S={S} G={ref.G}: {ref.iters} iterations, bound {ref.bounds[-1]:.8f}, EF {ef_obj:.8f}")
    assert done
    assert abs(ref.bounds[-1] - ef_obj) <= 1e-9 * abs(ef_obj)
    assert abs(ref.Qsum - ef_obj) <= 1e-9 * abs(ef_obj)
    assert ref.iters <= (8 if G is None else 20)


@pytest.mark.parametrize("S,G", [(3, None), (12, None), (30, 8)])
def test_outer_bound_is_monotone_and_below_the_optimum(S, G):
    ref, _, (ef_obj, _) = _run(S, G)
    b = np.array(ref.bounds)
    assert np.all(np.diff(b) >= -1e-9 * np.abs(b[:-1]))
    assert np.all(b <= ef_obj + 1e-9 * abs(ef_obj))
    assert abs(b[0] - ref.trivial_bound) <= 1e-12 * abs(ref.trivial_bound)      # etalb: the wait-and-see bound


@pytest.mark.parametrize("S,G", [(3, None), (12, 4)])
def test_every_cut_supports_the_expected_cost_from_below(S, G):
    """eta_g >= a.x + b holds for the true group cost at 20 random first-stage feasible x."""
    ref, _, _ = _run(S, G)
    rng = np.random.default_rng(3)
    nn = ref.nn
    for _ in range(20):
        x = rng.dirichlet(np.ones(nn + 1))[:nn] * 500.0          # x >= 0, sum x <= 500
        assert np.all(ref.R @ x <= ref.ru + 1e-9) and np.all(x >= ref.xlb) and np.all(x <= ref.xub)
        _, _, Q = ref.group_cuts(x)
        for g, a, b in ref.cuts:
            val = a @ x + b
            assert val <= Q[g] + 1e-7 * max(1.0, abs(Q[g])), (g, val, Q[g])


def test_groups_partition_the_scenarios():
    for S, G in [(3, 3), (130, 32), (130, 1), (65536, 32), (33, 32)]:
        g = np.array([R.group_of(s, G, S) for s in range(S)])
        assert g.min() == 0 and g.max() == G - 1 and np.all(np.diff(g) >= 0)
        # the closed form of the device's group ranges
        lo = [(k * S + G - 1) // G for k in range(G + 1)]
        assert all(np.all(g[lo[k]:lo[k + 1]] == k) for k in range(G)) and lo[G] == S
    assert R.default_groups(32) == 32 and R.default_groups(33) == 32 and R.default_groups(3) == 3


# ------------------------------------------------------------------ the product's option checks
def _method(all_nodenames=None, **o):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.lshaped import LShapedMethod
    options = {"root_solver": "mi355x_pdhg", "sp_solver": "mi355x_pdhg", "toc": False}
    options.update(o)
    return LShapedMethod(options, farmer.scenario_names_creator(3), farmer.scenario_creator,
                         scenario_creator_kwargs={"num_scens": 3}, all_nodenames=all_nodenames)


def test_option_checks():
    m = _method()
    assert m.cut_groups == 3 and m.max_iter == 30 and m.tol == 1e-8 and m._LShaped_bound is None
    assert not m.first_stage_solution_available and not m.tree_solution_available
    assert _method(relax_root=True, store_subproblems=True, cut_groups=1).cut_groups == 1    # accepted and ignored
    with pytest.raises(RuntimeError, match="multiple stages"):
        _method(all_nodenames=["ROOT", "ROOT_0", "ROOT_1"])
    with pytest.raises(NotImplementedError, match="bundles"):
        _method(bundles_per_rank=1)
    with pytest.raises(NotImplementedError, match="root_scenarios"):
        _method(root_scenarios=["scen0"])
    with pytest.raises(NotImplementedError, match="shared-matrix"):
        _method(shared_matrix=True)
    with pytest.raises(RuntimeError, match="gurobi"):
        _method(sp_solver="gurobi")
    with pytest.raises(RuntimeError, match="cplex"):
        _method(root_solver="cplex")
    with pytest.raises(ValueError, match="cut_groups"):
        _method(cut_groups=4)


def test_first_stage_rows_of_the_farmer_batch():
    """The acreage row: all its columns are nonants and it is the same in every scenario."""
    from mpisppy_amd.opt.lshaped import first_stage_rows
    m = _method()
    rows, Rr, lo, hi, same = first_stage_rows(m.batch)
    assert len(rows) == 1 and same == [True]
    assert np.array_equal(Rr, np.ones((1, 3))) and hi[0] == 500.0 and lo[0] == -np.inf
    Rm, rl, ru, xlb, xub = m._master_data()
    assert np.array_equal(Rm, Rr) and np.all(xlb == 0.0) and np.all(xub == 500.0)
    # a row that differs in one scenario is not a first-stage row
    a, b = m.batch.row_ptr[rows[0]], m.batch.row_ptr[rows[0] + 1]
    m.batch.A_val[1, a] = 2.0
    assert first_stage_rows(m.batch)[4] == [False] and m._master_data()[0].shape == (0, 3)
