"""ExtensiveForm and SchurComplement on the device (mpisppy_amd.opt.ef / opt.sc, csrc/ph_ef.inc;
DESIGN.md 3.21): the Schur pass against numpy, the solves against HiGHS, the certificate of
tests/ef_ref.py and the numpy restatement."""
import json
import os
import socket

import numpy as np
import pytest
import torch

import ef_ref as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REL = 1e-5                 # the project's standing relative tolerance
PRES, DRES = 1e-6, 1e-5    # the certificate's thresholds in tests/test_gpu_kkt.py (path 6)
SOLVER = "mi355x_pdhg"


def _creator(quad):
    from mpisppy_amd.examples import farmer
    if not quad:
        return farmer.scenario_creator

    def with_quad(name, **kw):
        m = farmer.scenario_creator(name, **kw)
        m.quad = [quad] * len(m.quad)
        return m
    return with_quad


def _opt(cls, S=3, cm=1, sense=1, quad=0.0, **o):
    from mpisppy_amd.examples import farmer
    kw = {} if "mpicomm" not in o else {"mpicomm": o.pop("mpicomm")}
    options = {"solver": SOLVER, "toc": False, "device": "cuda:0"}
    options.update(o)
    return cls(options, farmer.scenario_names_creator(S), _creator(quad),
               scenario_creator_kwargs={"num_scens": S, "crops_multiplier": cm, "sense": sense}, **kw)


def _sc(**kw):
    from mpisppy_amd.opt.sc import SchurComplement
    return _opt(SchurComplement, **kw)


def _ef(**kw):
    from mpisppy_amd.opt.ef import ExtensiveForm
    return _opt(ExtensiveForm, **kw)


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _solved(S, cm, quad=0.0):
    """A SchurComplement solve of farmer(S, cm) checked the way tests 2, 3 and 5 share: the
    certificate on the batch's own arrays, the nonants bitwise equal over the scenarios, a second
    solve with the same bits, the iteration count against the restatement's.  Returns (opt, z)."""
    sc, data, ref, ok, (obj, zh) = E.farmer_case(S, cm, quad)
    assert ok
    opt = _sc(S=S, cm=cm, quad=quad)
    assert opt.solve() == "optimal"
    e, b = opt.engine, opt.batch
    x, y = e.host("x"), e.host("y")[:, :b.m]
    z = opt.root_nonants()
    got = opt.objective_value()
    k = E.ef_kkt(None, x, y, E.batch_data(b))
    print(f"farmer S={S} cm={cm} quad={quad}: {opt.iterations} iterations (restatement {ref.it}) in {opt.seconds:.3f} s, "
          f"objective {got:.8f} HiGHS {obj:.8f} rel {abs(got - obj) / abs(obj):.1e}, |z - HiGHS| {np.abs(z - zh).max():.1e}, "
          f"|z - restatement| {np.abs(z - ref.z.v).max():.1e}, certificate {k['pres']:.1e} {k['dres']:.1e}")
    assert opt.first_stage_solution_available and opt.tree_solution_available
    assert abs(got - obj) <= REL * abs(obj)
    assert k["pres"] <= PRES and k["dres"] <= DRES
    assert opt.iterations <= 2 * ref.it                                            # test 9
    nx = e.nonant_x_dev()
    assert np.array_equal(_bits(nx), _bits(nx[:, :1].expand(-1, e.S).contiguous()))     # bitwise equal over the scenarios
    assert np.array_equal(_bits(nx[:, 0]), _bits(e.ef_z))
    assert np.all(e.status.cpu().numpy() == 0) and np.all(e.iters.cpu().numpy() == opt.iterations)
    first = (_bits(e.x).copy(), _bits(e.y).copy(), opt.iterations)
    opt.solve()
    assert np.array_equal(first[0], _bits(e.x)) and np.array_equal(first[1], _bits(e.y)) and first[2] == opt.iterations
    return opt, z, zh


# ------------------------------------------------------------------ 1: the reference's own test
def test_farmer_three_scenarios_through_both_classes(gpu, tmp_path):
    """mpisppy/tests/test_sc.py:30-38: every scenario plants (CORN 80, SUGAR_BEETS 250, WHEAT 170)."""
    sc, data, ref, ok, _ = E.farmer_case(3, 1)
    want = {"DevotedAcreage[CORN0]": 80.0, "DevotedAcreage[SUGAR_BEETS0]": 250.0, "DevotedAcreage[WHEAT0]": 170.0}
    opt = _sc()
    try:
        assert opt.solve() == "optimal"
        sol = opt.gather_var_values_to_rank0()
        for s in ("scen0", "scen1", "scen2"):
            for nm, v in want.items():
                assert round(abs(sol[s, nm] - v), 5) == 0, (s, nm, sol[s, nm])          # assertAlmostEqual(places=5)
        assert abs(opt.objective_value() + 108390.0) <= REL * 108390.0
        assert opt.iterations <= 2 * ref.it                                        # test 9
        opt.report_var_values_at_rank0(header="farmer, 3 scenarios")
    finally:
        opt.engine.close()
    ef = _ef()
    try:
        res = ef.solve_extensive_form()
        assert res.solver.termination_condition == "optimal" and len(res.solution) == 1
        assert ef.first_stage_solution_available and ef.tree_solution_available
        assert abs(ef.get_objective_value() + 108390.0) <= REL * 108390.0
        root = ef.get_root_solution()
        assert set(root) == set(want)
        for nm, v in want.items():
            assert round(abs(root[nm] - v), 5) == 0
        assert [(nd, nm) for nd, nm, _ in ef.nonants()] == [("ROOT", nm) for nm in root]
        ef.nonants_to_csv(str(tmp_path / "nonants.csv"))
        assert len(open(tmp_path / "nonants.csv").read().splitlines()) == 4
        for _, mdl in ef.scenarios():                                              # load_solutions_to_models
            assert round(abs(mdl.find_var("DevotedAcreage[CORN0]").value - 80.0), 5) == 0
    finally:
        ef.engine.close()


# ------------------------------------------------------------------ 2, 3: three waves, nn = 6; nn = 9
@pytest.mark.parametrize("S,cm", [(130, 2), (67, 3)])
def test_farmer_lp_against_highs_and_the_certificate(gpu, S, cm):
    opt, _, _ = _solved(S, cm)
    opt.engine.close()


# ------------------------------------------------------------------ 4: the Schur pass alone
def test_schur_pass_matches_numpy(gpu):
    """At the starting iterate of S = 130, cm = 2: sum_s T' N_s^-1 T and sum_s T' N_s^-1 g_s against
    numpy on the batch's own arrays, within 1e-12 of the sum of |terms| (fp64 sums of 130 terms;
    the lanes' LDL' of the well-conditioned starting N_s against LAPACK's LU measured 2e-4 of that bound on the
    host); the same bits twice."""
    opt = _sc(S=130, cm=2)
    try:
        opt._setup()
        e, b = opt.engine, opt.batch
        assert b.nn == 6 and e.S == 130
        ref = E.EFRef(data=E.batch_data(b))
        ref.step()
        Cs, rt = ref.first_terms
        tri = np.tril_indices(b.nn)
        want = np.concatenate([Cs.sum(axis=0)[tri], rt.sum(axis=0)])
        mag = np.concatenate([np.abs(Cs).sum(axis=0)[tri], np.abs(rt).sum(axis=0)])
        e.ef_schur(0)
        got = e.ef_sum.cpu().numpy().copy()
        e.ef_schur(0)
        assert np.array_equal(got.view(np.int64), _bits(e.ef_sum))
        n = len(want)
        err = np.abs(got[:n] - want)
        print(f"Schur pass: worst error / bound = {np.max(err / (1e-12 * mag)):.3g}")
        assert np.all(err <= 1e-12 * mag), (int(np.argmax(err / mag)), err.max())
    finally:
        opt.engine.close()


# ------------------------------------------------------------------ 5: a QP
def test_farmer_qp(gpu):
    """quad = 0.01 on every column.  The restatement's z is 3.95e-2 from HiGHS's on the CPU (HiGHS's
    QP solver stops early: its objective is 6.1e-3 ABOVE the restatement's feasible one, DESIGN.md
    7.9), so the bound against HiGHS is that error times ten; against the restatement, whose
    certificate passes, z is held to 1e-5."""
    opt, z, zh = _solved(130, 2, quad=0.01)
    try:
        ref = E.farmer_case(130, 2, 0.01)[2]
        assert opt.is_qp
        assert np.abs(z - zh).max() <= 10 * 3.95e-2
        assert np.abs(z - ref.z.v).max() <= 1e-5
    finally:
        opt.engine.close()


# ------------------------------------------------------------------ 6: a maximisation
def test_a_maximisation_farmer(gpu):
    ef = _ef(sense=-1)
    try:
        res = ef.solve_extensive_form()
        assert res.solver.termination_condition == "optimal" and not ef.is_minimizing
        assert abs(ef.get_objective_value() - 108390.0) <= REL * 108390.0
    finally:
        ef.engine.close()


def test_ef_xstar_solver_gives_the_sample_optimum(gpu):
    """ciutils.ef_xstar_solver: the callable gap_estimators takes as xstar_solver=, on farmer's three
    scenarios (through the model's batch_creator, so without per-scenario models)."""
    from mpisppy_amd.confidence_intervals.ciutils import ef_xstar_solver
    from mpisppy_amd.examples import farmer
    solve = ef_xstar_solver(farmer, solver_name=SOLVER, device="cuda:0")
    x = solve(farmer.scenario_names_creator(3), {"num_scens": 3})
    assert x.shape == (3,) and np.abs(np.sort(x) - [80.0, 170.0, 250.0]).max() <= 1e-5
    with pytest.raises(RuntimeError, match="was not solved"):
        short = ef_xstar_solver(farmer, solver_name=SOLVER, device="cuda:0", max_iter=2)
        short(farmer.scenario_names_creator(3), {"num_scens": 3})


# ------------------------------------------------------------------ 8: the iteration limit
def test_iteration_limit(gpu):
    opt = _sc(max_iter=2)
    try:
        with pytest.raises(RuntimeError, match="Schur-Complement Interior Point algorithm did not converge"):
            opt.solve()
        assert opt.iterations == 2 and not opt.first_stage_solution_available
    finally:
        opt.engine.close()
    ef = _ef()
    try:
        res = ef.solve_extensive_form(solver_options={"max_iter": 2})
        assert res.solver.termination_condition == "maxIterations"
        assert not ef.first_stage_solution_available and not ef.tree_solution_available
        assert np.all(ef.engine.status.cpu().numpy() == 1)
    finally:
        ef.engine.close()


# ------------------------------------------------------------------ 7: two gloo ranks on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(HERE)
    for p in (HERE, os.path.join(root, "mpi-sppy-1_amd"), root):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mpisppy_amd.comm import Comm
        opt = _sc(S=130, cm=2, mpicomm=Comm())
        opt.solve()
        out = {"obj": opt.objective_value(), "iters": opt.iterations, "n": opt.batch.S,
               "z_bits": _bits(opt.engine.ef_z).tolist()}
        opt.engine.close()
        with open(os.path.join(out_dir, f"ef_r{rank}.json"), "w") as f:
            json.dump(out, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_give_the_one_rank_solution(gpu, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"ef_r{k}.json")) for k in range(2)]
    assert r[0]["n"] == r[1]["n"] == 65
    assert r[0]["z_bits"] == r[1]["z_bits"]                           # every rank solved the same system
    z2 = np.array(r[0]["z_bits"], dtype=np.int64).view(np.float64)
    one = _sc(S=130, cm=2)
    try:
        one.solve()
        z1 = one.root_nonants()
        print(f"two ranks: |z - one rank| {np.abs(z2 - z1).max():.1e}, iterations {r[0]['iters']} / {one.iterations}")
        assert np.abs(z2 - z1).max() <= 1e-9 * np.abs(z1).max()             # relative, as vectors (entries may be 0)
        assert r[0]["obj"] == r[1]["obj"]
    finally:
        one.engine.close()
