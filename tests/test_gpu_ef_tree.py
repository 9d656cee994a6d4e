"""ExtensiveForm on multistage trees on the device (mpisppy_amd.opt.ef, csrc/ph_ef_tree.inc;
DESIGN.md 3.23): the solves against HiGHS on the assembled extensive form and the certificate of
tests/ef_tree_ref.py, the first pass's per-node systems against the numpy restatement, the fixed
order of the sums, and the class's surface on a tree."""
import numpy as np
import pytest

import ef_tree_ref as R

pytestmark = pytest.mark.gpu

REL = 1e-5                 # the project's standing relative tolerance
PRES, DRES = 1e-6, 1e-5    # the certificate's thresholds of tests/test_gpu_ef.py
DEV = {"device": "cuda:0"}
# (branching factors, QuadShortCoeff): the smallest tree (3 non-leaf nodes); 17 nodes of depth 3, a
# middle level that both receives and gives; two 128-lane blocks, the deepest node of scenarios
# 120-129 across their boundary; a QP (one common step length); and segments of 256 scenarios, at
# which the segmented sum switches from a thread to a block per (value, segment)
SHAPES = [((2, 2), 0.0), ((4, 3, 2), 0.0), ((3, 5, 10), 0.0), ((3, 2), 0.3), ((2, 256), 0.0)]


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _ef(bfs, quad=0.0):
    from mpisppy_amd.opt.ef import ExtensiveForm
    return R.aircond_opt(ExtensiveForm, bfs, quad, **DEV)


def _check_solution(ef, b, lay, obj, zh, ref_it, what):
    """What every solved shape has to show: status, objective, certificate, the nonants' bits."""
    e = ef.engine
    x, y = e.host("x"), e.host("y")[:, :b.m]
    got = ef.get_objective_value()
    k = R.tree_kkt(b, x, y)
    z = e.ef_z.cpu().numpy()
    print(f"{what}: {ef.iterations} iterations (restatement {ref_it}) in {ef.seconds:.3f} s, objective {got:.8f} HiGHS {obj:.8f} "
          f"rel {abs(got - obj) / abs(obj):.1e}, certificate {k['pres']:.1e} {k['dres']:.1e}")
    assert ef.status == "optimal" and ef.first_stage_solution_available and ef.tree_solution_available
    assert np.all(e.status.cpu().numpy() == 0) and np.all(e.iters.cpu().numpy() == ef.iterations)
    assert abs(got - obj) <= REL * abs(obj)
    assert k["pres"] <= PRES and k["dres"] <= DRES
    assert ef.iterations <= 2 * ref_it
    # nonant columns: the node's bits in every scenario under it ...
    assert np.array_equal(x[:, b.nonant_col].view(np.int64), z[lay.zidx].view(np.int64))
    # ... and not a sibling's where HiGHS's own values differ
    for n in range(1, lay.Nn):
        for s in range(n + 1, lay.Nn):
            if lay.parent[s] != lay.parent[n]:
                continue
            a, c = slice(lay.zoff[n], lay.zoff[n + 1]), slice(lay.zoff[s], lay.zoff[s + 1])
            differ = np.abs(zh[a] - zh[c]) > 1e-6 * (1.0 + np.abs(zh[a]))
            assert np.all(z[a][differ] != z[c][differ]), (n, s)
    return z


@pytest.mark.parametrize("bfs,quad", SHAPES)
def test_aircond_trees_against_highs_and_the_certificate(gpu, bfs, quad):
    b, ref, ok, (obj, zh) = R.case(bfs, quad)
    assert ok
    ef = _ef(bfs, quad)
    try:
        res = ef.solve_extensive_form()
        assert res.solver.termination_condition == "optimal"
        assert ef.is_qp == bool(quad)
        _check_solution(ef, ef.batch, ref.lay, obj, zh, ref.it, f"aircond {bfs} quad={quad}")
    finally:
        ef.engine.close()


def _node_systems(ef, ref):
    """the first pass's per-node matrices and right-hand sides against the restatement's"""
    ef._setup()
    e = ef.engine
    A, bb = e.eft_schur(0, inspect=True)
    A, bb = A.cpu().numpy(), bb.cpu().numpy()
    worst = 0.0
    for n, (An, bn) in ref.node_systems().items():
        Pd = len(bn)
        worst = max(worst, np.abs(np.tril(A[n, :Pd, :Pd]) - np.tril(An)).max() / np.abs(An).max(),
                    np.abs(bb[n, :Pd] - bn).max() / max(1.0, np.abs(bn).max()))
    return worst


def test_synthetic_tree_with_offsets_that_differ_by_depth(gpu):
    """nlens = [3, 1, 2] over a 2,3,2 tree (tests/ef_tree_ref.py synthetic_batch): the first pass's
    per-node systems to 1e-10 relative, then the solve against HiGHS."""
    _, b, ref, ok, (obj, zh) = R.synthetic_case()
    assert ok
    ef = R.synthetic_opt(**DEV)
    try:
        worst = _node_systems(ef, ref)
        print(f"synthetic: per-node systems worst relative error {worst:.1e}")
        assert worst <= 1e-10
        res = ef.solve_extensive_form()
        assert res.solver.termination_condition == "optimal"
        _check_solution(ef, ef.batch, ref.lay, obj, zh, ref.it, "synthetic 2,3,2")
    finally:
        ef.engine.close()


def test_two_solves_give_the_same_bits_and_the_surface_on_a_tree(gpu, tmp_path):
    """aircond 4,3,2 twice in one process: bitwise the same z (fixed order, no atomics); nonants()
    over the 17 non-leaf nodes; get_root_solution ROOT's two."""
    b, ref, ok, (obj, zh) = R.case((4, 3, 2))
    ef = _ef((4, 3, 2))
    try:
        worst = _node_systems(ef, ref)
        assert worst <= 1e-10, worst
        ef.solve_extensive_form()
        z1, x1, it1 = _bits(ef.engine.ef_z).copy(), _bits(ef.engine.x).copy(), ef.iterations
        ef.solve_extensive_form()
        assert np.array_equal(z1, _bits(ef.engine.ef_z)) and np.array_equal(x1, _bits(ef.engine.x)) and it1 == ef.iterations
        z = ef.engine.ef_z.cpu().numpy()
        got = list(ef.nonants())
        assert len(got) == 17 * 2
        assert [nd for nd, _, _ in got[::2]] == list(ef.batch.node_names) and got[0][0] == "ROOT" and got[-1][0] == "ROOT_3_2"
        assert np.array_equal(np.array([v for _, _, v in got]), z)
        names = ef.batch.nonant_names
        assert [nm for _, nm, _ in got[:2]] == names[:2] and [nm for _, nm, _ in got[2:4]] == names[2:4]
        assert [nm for _, nm, _ in got[-2:]] == names[4:6]
        root = ef.get_root_solution()
        assert list(root) == names[:2] and np.array_equal(np.array(list(root.values())), z[:2])
        ef.nonants_to_csv(str(tmp_path / "nonants.csv"))
        assert len(open(tmp_path / "nonants.csv").read().splitlines()) == 1 + 34
        for nm, mdl in ef.scenarios():                                             # load_solutions_to_models
            s = ef.local_scenario_names.index(nm)
            assert mdl.find_var(names[0]).value == z[0] and mdl.find_var(names[4]).value == z[ref.lay.zidx[s, 4]]
    finally:
        ef.engine.close()


def test_ef_xstar_solver_on_a_multistage_model(gpu):
    """ciutils.ef_xstar_solver on aircond 3,2: ROOT's nonants of the tree's extensive form.  The LP's
    nonants need not be unique, so x is not compared with HiGHS's: an ExtensiveForm built here with
    the solver's arguments has to reach the HiGHS optimum's objective, and the solver, which runs
    the same deterministic solve, has to return that solve's ROOT nonants bit for bit."""
    from mpisppy_amd.confidence_intervals import ciutils
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.opt.ef import ExtensiveForm
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    b, ref, ok, (obj, zh) = R.case((3, 2))
    names, kw = aircond.scenario_names_creator(6), {"branching_factors": [3, 2], "start_seed": 0}
    x = ciutils.ef_xstar_solver(aircond, solver_name=R.SOLVER, device="cuda:0")(names, kw)
    ef = ExtensiveForm({"solver": R.SOLVER, "tol": 1e-8, "max_iter": 100, "toc": False, "device": "cuda:0",
                        "batch_creator": aircond.batch_creator}, names, aircond.scenario_creator,
                       scenario_creator_kwargs=kw, all_nodenames=create_nodenames_from_branching_factors([3, 2]))
    try:
        assert ef.solve_extensive_form().solver.termination_condition == "optimal"
        assert len(ef.batch.node_names) == 4
        assert abs(ef.get_objective_value() - obj) <= REL * abs(obj)
        assert x.shape == (2,) and np.array_equal(x.view(np.int64), ef.root_nonants().view(np.int64))
    finally:
        ef.engine.close()
