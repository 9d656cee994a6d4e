"""The conditioned multistage extensive form on the device (phgpu_eft_fix,
ExtensiveForm.fix_node_nonants): solves with held nonants against HiGHS with lb = ub
on the held columns, the certificate on the free entries and the restatement's iteration count
(tests/ef_cond_ref.py); the held values bit for bit; every subtree's own objective; the bits of a
solve that holds nothing; what the entry refuses."""
import numpy as np
import pytest

import ef_cond_ref as C
import ef_tree_ref as R

pytestmark = pytest.mark.gpu

REL = 1e-5                 # the project's standing tolerances (tests/test_gpu_ef_tree.py)
PRES, DRES = 1e-6, 1e-5
DEV = {"device": "cuda:0"}
NAN = float("nan")


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _ef(bfs, quad=0.0):
    from mpisppy_amd.opt.ef import ExtensiveForm
    return R.aircond_opt(ExtensiveForm, bfs, quad, **DEV)


def _values(depth, i):
    """(RegularProd, OvertimeProd) held at node i of a depth: inside the bounds, not optimal, different
    between siblings (aircond has complete recourse: any such value is feasible)."""
    return [[150.0, 20.0], [120.0 + 10.0 * i, 5.0 * i], [100.0 + 7.0 * i, 3.0 * i]][depth]


def _cache(b, depths):
    lay = R.Layout(b)
    first = {d: int(np.flatnonzero(lay.depth == d)[0]) for d in depths}
    return {b.node_names[n]: _values(int(lay.depth[n]), n - first[int(lay.depth[n])]) for n in range(lay.Nn)
            if int(lay.depth[n]) in depths}


def _solve_and_check(ef, key, cache):
    """Hold ``cache``, solve, and check what every conditioned solve has to show; returns the case."""
    b = ef.batch
    lay = R.Layout(b)
    zfix = C.zfix_of(lay, b.node_names, cache)
    case = C.cond_case(key, b, zfix)
    assert case["ok"], "HiGHS finds the conditioned problem infeasible, or the restatement did not converge"
    ef.fix_node_nonants(cache)
    res = ef.solve_extensive_form()
    e = ef.engine
    x, y = e.host("x"), e.host("y")[:, :b.m]
    got, obj, ref = ef.get_objective_value(), case["obj"], case["ref"]
    k = C.cond_kkt(b, x, y, zfix)
    z = e.ef_z.cpu().numpy()
    held = ~np.isnan(zfix)
    print(f"{key}: {int(held.sum())} of {lay.Ztot} held, {ef.iterations} iterations (restatement {ref.it}) in {ef.seconds:.3f} s, "
          f"objective {got:.8f} HiGHS {obj:.8f} rel {abs(got - obj) / abs(obj):.1e}, certificate {k['pres']:.1e} {k['dres']:.1e}")
    assert res.solver.termination_condition == "optimal" and ef.status == "optimal"
    assert np.all(e.status.cpu().numpy() == 0)
    assert abs(got - obj) <= REL * abs(obj)
    assert k["pres"] <= PRES and k["dres"] <= DRES
    assert ef.iterations <= 2 * ref.it
    assert np.array_equal(z[held].view(np.int64), zfix[held].view(np.int64))              # ef_z: the held bits
    assert np.array_equal(x[:, b.nonant_col].view(np.int64), z[lay.zidx].view(np.int64))  # and every scenario's columns
    tn = dict(ef.tree_nonants())
    for nd, v in cache.items():
        v = np.asarray(v, dtype=np.float64)
        assert np.array_equal(tn[nd][~np.isnan(v)].view(np.int64), v[~np.isnan(v)].view(np.int64)), nd
    by = {}
    for nd, _, v in ef.nonants():
        by.setdefault(nd, []).append(v)
    assert all(np.array_equal(np.array(by[nd]), tn[nd]) for nd in tn)
    return case


def test_root_held_at_the_optimum_gives_the_unconditioned_optimum(gpu):
    b, ref, ok, (obj, zh) = R.case((2, 2))
    assert ok
    ef = _ef((2, 2))
    try:
        case = _solve_and_check(ef, "aircond22/root=opt", {"ROOT": zh[:2]})
        assert abs(case["obj"] - obj) <= 1e-7 * abs(obj)                        # (HiGHS against itself)
        assert abs(ef.get_objective_value() - obj) <= REL * abs(obj)
    finally:
        ef.engine.close()


@pytest.mark.parametrize("what,root", [("interior", [150.0, 20.0]), ("on a bound", [150.0, 0.0])])
def test_root_held_and_every_subtrees_own_objective(gpu, what, root):
    ef = _ef((2, 2))
    try:
        b = ef.batch
        case = _solve_and_check(ef, f"aircond22/root {what}", {"ROOT": root})
        lay = case["lay"]
        objs = ef.node_objectives(1)
        assert [nd for nd, _ in objs] == ["ROOT_0", "ROOT_1"]
        for nd, v in objs:
            n = list(b.node_names).index(nd)
            ok, want, _ = C.cond_optimum(b, case["zfix"], lay, scen=lay.scenarios(n))
            print(f"  subtree {nd}: {v:.8f} HiGHS alone {want:.8f}")
            assert ok and abs(v - want) <= REL * abs(want)
        (r, v0), = ef.node_objectives(0)
        assert r == "ROOT" and abs(v0 - ef.get_objective_value()) <= 1e-12 * abs(v0)
        assert abs(sum(v for _, v in objs) / 2 - v0) <= 1e-12 * abs(v0)
    finally:
        ef.engine.close()


@pytest.mark.parametrize("depths", [(0,), (0, 1), (0, 1, 2)])
def test_whole_depths_held_on_a_four_stage_tree(gpu, depths):
    """aircond 3,2,2: depth 0; depths 0 and 1 (the forest of stage 3); everything, where the problem is
    12 separate scenario LPs and the objective is Xhat_Eval's at the same cache, an independent path."""
    ef = _ef((3, 2, 2))
    try:
        cache = _cache(ef.batch, depths)
        _solve_and_check(ef, f"aircond322/depths {depths}", cache)
        if depths == (0, 1, 2):
            from mpisppy_amd.examples import aircond
            from mpisppy_amd.sputils import create_nodenames_from_branching_factors
            from mpisppy_amd.utils.xhat_eval import Xhat_Eval
            ev = Xhat_Eval({"solver_name": R.SOLVER, "toc": False, **DEV}, aircond.scenario_names_creator(12),
                           aircond.scenario_creator, scenario_creator_kwargs={"branching_factors": [3, 2, 2], "start_seed": 0},
                           all_nodenames=create_nodenames_from_branching_factors([3, 2, 2]))
            try:
                want = ev.evaluate(cache)
            finally:
                ev.engine.close()
            print(f"  everything held: {ef.get_objective_value():.8f} Xhat_Eval {want:.8f}")
            assert want is not None and abs(ef.get_objective_value() - want) <= REL * abs(want)
    finally:
        ef.engine.close()


def test_single_entries_held_within_a_node_and_between_siblings(gpu):
    ef = _ef((3, 2, 2))
    try:
        _solve_and_check(ef, "aircond322/partial", {"ROOT": [NAN, 20.0], "ROOT_1": [130.0, NAN]})
    finally:
        ef.engine.close()


def test_root_held_on_a_qp(gpu):
    """QuadShortCoeff 0.3: one common step length for the primal and the dual side."""
    ef = _ef((3, 2), 0.3)
    try:
        _solve_and_check(ef, "aircond32q/root", {"ROOT": [150.0, 20.0]})
        assert ef.is_qp
    finally:
        ef.engine.close()


def test_holding_nothing_leaves_the_bits_and_two_conditioned_solves_agree(gpu):
    ef = _ef((4, 3, 2))
    try:
        ef.solve_extensive_form()
        z0, x0, it0 = _bits(ef.engine.ef_z).copy(), _bits(ef.engine.x).copy(), ef.iterations
        Ztot = ef.engine.eft_ztot
        ef._held_z = lambda: np.full(Ztot, NAN)                   # phgpu_eft_fix is called, with every entry free
        calls = []
        fix = ef.engine.eft_fix
        ef.engine.eft_fix = lambda z: (calls.append(1), fix(z))[1]
        ef.solve_extensive_form()
        assert calls == [1]
        assert np.array_equal(z0, _bits(ef.engine.ef_z)) and np.array_equal(x0, _bits(ef.engine.x)) and it0 == ef.iterations
        del ef._held_z
        ef.fix_node_nonants(_cache(ef.batch, (0, 1)))
        ef.solve_extensive_form()
        z1, x1, it1 = _bits(ef.engine.ef_z).copy(), _bits(ef.engine.x).copy(), ef.iterations
        assert ef.status == "optimal" and not np.array_equal(z1, z0)
        ef.solve_extensive_form()
        assert np.array_equal(z1, _bits(ef.engine.ef_z)) and np.array_equal(x1, _bits(ef.engine.x)) and it1 == ef.iterations
        ef.free_node_nonants()
        ef.solve_extensive_form()
        assert np.array_equal(z0, _bits(ef.engine.ef_z)) and it0 == ef.iterations
    finally:
        ef.engine.close()


def test_what_eft_fix_refuses(gpu):
    ef = _ef((2, 2))
    try:
        ef.fix_node_nonants({"ROOT_1": [NAN, -1.0]})
        with pytest.raises(RuntimeError, match="node 2 entry 1: the value -1 is outside its bounds"):
            ef.solve_extensive_form()
        ef.free_node_nonants()
        ef._setup()
        e = ef.engine
        z = np.full(e.eft_ztot, NAN)
        z[0] = 10.0
        e.eft_fix(z)
        with pytest.raises(RuntimeError, match="called twice"):
            e.eft_fix(z)
        ef._setup()
        e.eft_schur(0)
        with pytest.raises(RuntimeError, match="an iteration has begun"):
            e.eft_fix(z)
    finally:
        ef.engine.close()
