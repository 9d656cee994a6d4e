"""The L-shaped method on the device (mpisppy_amd.opt.lshaped, csrc/ph_lshaped.inc): the cut pass
against numpy, the master against HiGHS on the same masters, and the method end to end against
the extensive form and the numpy restatement (tests/lshaped_ref.py)."""
import json
import os
import socket

import numpy as np
import pytest
import torch

import lshaped_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REL = 1e-5          # the project's standing relative tolerance
FEAS = 1e-7         # scaled feasibility of the master's solution
SOLVER = "mi355x_pdhg"
MEASURED = {}       # name -> relative difference of the master's objective to HiGHS (printed)


def _opt(S=3, cm=1, sense=1, mpicomm=None, **o):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.lshaped import LShapedMethod
    options = {"root_solver": SOLVER, "sp_solver": SOLVER, "toc": False, "device": "cuda:0", "tol": 1e-6}
    options.update(o)
    return LShapedMethod(options, farmer.scenario_names_creator(S), farmer.scenario_creator,
                         scenario_creator_kwargs={"num_scens": S, "crops_multiplier": cm, "sense": sense},
                         mpicomm=mpicomm)


_REF = {}


def _ref(S, cm, G):
    """The restatement's run and the EF optimum of farmer(S, cm), computed once."""
    key = (S, cm, G)
    if key not in _REF:
        from oracle.models import farmer_scenario
        scens = [farmer_scenario(f"scen{i}", cm, num_scens=S) for i in range(S)]
        ref = R.LShapedRef(scens, G=G, tol=1e-6)
        assert ref.run()
        if (S, cm) not in _REF:
            _REF[(S, cm)] = R.ef_optimum(scens)
        _REF[key] = ref
    return _REF[key], _REF[(S, cm)]


# ------------------------------------------------------------------ the cut pass alone
def _numpy_cuts(b, x, y, obj, status, G, S_total, off=0):
    """a_g, b_g, Q_g, the count and the sums of |terms| from the batch's own arrays."""
    nn = b.nn
    a, bb, Q = np.zeros((G, nn)), np.zeros(G), np.zeros(G)
    mag = np.zeros((G, nn + 2))
    bad = 0
    for s in range(b.S):
        if status[s] != 0:
            bad += 1
            continue
        g = (s + off) * G // S_total
        A = b.dense_A(s)
        col = b.nonant_col
        terms = -(A[:, col] * y[s][:, None])
        d = b.c[s, col] + b.q[s, col] * x[s, col] + terms.sum(axis=0)
        p = b.prob[s]
        a[g] += p * d
        bb[g] += p * (obj[s] - d @ x[s, col])
        Q[g] += p * obj[s]
        dm = np.abs(b.c[s, col]) + np.abs(b.q[s, col] * x[s, col]) + np.abs(terms).sum(axis=0)
        mag[g, :nn] += p * dm
        mag[g, nn] += p * (abs(obj[s]) + dm @ np.abs(x[s, col]))
        mag[g, nn + 1] += p * abs(obj[s])
    return a, bb, Q, bad, mag


def test_cut_pass_matches_numpy(gpu):
    """Farmer, 130 scenarios (three waves, the last ragged), nn = 6: G = 32 (unequal groups) and
    G = 1, from a fixed solve and from constructed duals; a status that is not OPTIMAL is counted
    and leaves the sums; the same bits twice.  Bound: 1e-12 of the sum of |terms| (fp64 sums of at
    most 130 terms of at most 10 products).  More than 32 groups are refused by
    phgpu_lshaped_init, so G = 130 is asserted to be that error."""
    from mpisppy_amd import _lib
    opt = _opt(S=130, cm=2, cut_groups=32)
    try:
        opt._setup()
        e, b = opt.engine, opt.batch
        assert b.nn == 6 and e.S == 130
        e.fix_nonants(e.ls_xhat)
        e.solve(opt._sp_opts, warm=True)
        rng = np.random.default_rng(7)
        R_, rl, ru, xlb, xub = opt.master_rows
        for G in (32, 1):
            if G != 32:
                e.lshaped_init(G, 4, 0, 130, R_, rl, ru, xlb, xub, np.zeros(G))
            for kind in ("solve", "random"):
                if kind == "random":
                    e.y.copy_(torch.from_numpy(rng.normal(size=(b.m, b.S)) * 50.0).to(e.device))
                    e.status[5] = 1
                    e.status[129] = 2
                x, y, obj, st = e.host("x"), e.host("y"), e.host("obj"), e.host("status")
                e.lshaped_cuts()
                got = e.ls_cutbuf.cpu().numpy().copy()
                e.lshaped_cuts()
                assert np.array_equal(got, e.ls_cutbuf.cpu().numpy())          # the same bits twice
                a, bb, Q, bad, mag = _numpy_cuts(b, x, y, obj, st, G, 130)
                want = np.concatenate([np.concatenate([a, bb[:, None], Q[:, None]], axis=1).ravel(), [bad]])
                tol = np.concatenate([1e-12 * mag.ravel(), [0.0]])
                err = np.abs(got - want)
                print(f"cut pass G={G} {kind}: worst error / bound = {np.max(err[:-1] / np.maximum(tol[:-1], 1e-300)):.3f}, "
                      f"not optimal {got[-1]:.0f}")
                assert np.all(err <= tol), (G, kind, np.argmax(err - tol), err.max())
                assert got[-1] == (2 if kind == "random" else 0)
            e.status.zero_()
        with pytest.raises(_lib.PhgpuError, match="G 130"):
            e.lshaped_init(130, 4, 0, 130, R_, rl, ru, xlb, xub, np.zeros(130))
    finally:
        opt.engine.close()


# ------------------------------------------------------------------ the master alone
def _masters():
    """name -> (nn, G, cuts, R, rl, ru, xlb, xub, etalb, max_cuts); all with nn = 3."""
    ref, _ = _ref(3, 1, 3)
    rng = np.random.default_rng(11)
    nn = 3
    base = (ref.R, ref.rl, ref.ru, ref.xlb, ref.xub, ref.etalb)
    out = {"farmer_two_per_group": (nn, 3, ref.cuts[:ref.masters[1]]) + base + (None,),
           "farmer_converged": (nn, 3, list(ref.cuts)) + base + (None,)}
    G = 2
    xlb, xub, etalb = np.zeros(nn), np.full(nn, 10.0), np.full(G, -100.0)
    Z, e = np.zeros((0, nn)), np.zeros(0)

    def rc(n, span=0.0):
        return [(i % G, rng.uniform(-1, 1, nn) * 10 ** rng.uniform(0, span), float(rng.uniform(-5, 5))) for i in range(n)]
    cuts = rc(8)
    out["repeated_cut"] = (nn, G, cuts + [cuts[0]] * 4, Z, e, e, xlb, xub, etalb, None)
    out["equality_row"] = (nn, G, cuts, np.ones((1, nn)), np.array([7.0]), np.array([7.0]), xlb, xub, etalb, None)
    fl, fu = xlb.copy(), xub.copy()
    fl[1], fu[1] = -np.inf, np.inf
    out["free_column"] = (nn, G, cuts, Z, e, e, fl, fu, etalb, None)
    out["coefficients_1_to_1e5"] = (nn, G, rc(12, 5.0), Z, e, e, xlb, xub, etalb, None)
    out["full_store"] = (nn, G, cuts, Z, e, e, xlb, xub, etalb, len(cuts))
    return out


@pytest.fixture(scope="module")
def master_engine(gpu):
    opt = _opt(S=3)
    opt._setup()
    yield opt.engine
    opt.engine.close()


def _device_master(e, nn, G, cuts, Rr, rl, ru, xlb, xub, etalb, max_cuts):
    e.lshaped_init(G, max_cuts or max(len(cuts), 1) + 3, 0, 3, Rr, rl, ru, xlb, xub, etalb)
    e.lshaped_load([c[0] for c in cuts], np.array([c[1] for c in cuts]).reshape(len(cuts), nn), [c[2] for c in cuts])
    e.ls_xhat.zero_()
    e.lshaped_master()
    info = dict(e.lshaped_read())
    z = np.concatenate([e.ls_xhat[:nn, 0].cpu().numpy(), e.ls_eta.cpu().numpy()])
    assert torch.equal(e.ls_xhat[:nn], e.ls_xhat[:nn, :1].expand(-1, e.S))      # broadcast to every scenario
    return z, info


@pytest.mark.parametrize("name", ["farmer_two_per_group", "farmer_converged", "repeated_cut", "equality_row",
                                  "free_column", "coefficients_1_to_1e5", "full_store"])
def test_master_matches_highs(master_engine, name):
    nn, G, cuts, Rr, rl, ru, xlb, xub, etalb, mc = _masters()[name]
    x, eta, obj, st = R.solve_master(nn, G, cuts, Rr, rl, ru, xlb, xub, etalb)
    assert st == 0
    z, info = _device_master(master_engine, nn, G, cuts, Rr, rl, ru, xlb, xub, etalb, mc)
    rel = abs(info["bound"] - obj) / max(1.0, abs(obj))
    viol = R.master_violation(z, nn, G, cuts, Rr, rl, ru, xlb, xub, etalb)
    MEASURED[name] = rel
    print(f"master {name}: HiGHS {obj:.10f} device {info['bound']:.10f} rel {rel:.2e} violation {viol:.1e} "
          f"status {info['status']:.0f} iterations {info['iters']:.0f} residuals {info['pres']:.1e} {info['dres']:.1e} "
          f"{info['gap']:.1e}")
    assert info["status"] == 0 and info["iters"] <= 200
    assert rel <= REL
    assert viol <= FEAS
    assert abs(z[nn:].sum() - info["bound"]) <= 1e-12 * max(1.0, abs(info["bound"]))
    if mc is not None:
        g, a, b = master_engine.lshaped_export()
        assert len(g) == mc and np.array_equal(a, np.array([c[1] for c in cuts])) and list(g) == [c[0] for c in cuts]


def test_master_reports_contradictory_rows_infeasible(master_engine):
    """x0 + x1 + x2 <= 1 and >= 2: PRIMAL_INFEASIBLE within the iteration cap, as HiGHS says."""
    nn, G, cuts, _, _, _, xlb, xub, etalb, _ = _masters()["repeated_cut"]
    Rr, rl, ru = np.ones((2, nn)), np.array([-np.inf, 2.0]), np.array([1.0, np.inf])
    assert R.solve_master(nn, G, cuts, Rr, rl, ru, xlb, xub, etalb)[3] == 2
    _, info = _device_master(master_engine, nn, G, cuts, Rr, rl, ru, xlb, xub, etalb, None)
    print(f"contradictory rows: status {info['status']:.0f} after {info['iters']:.0f} iterations")
    assert info["status"] == 2 and info["iters"] <= 200


def test_init_limits(master_engine):
    from mpisppy_amd import _lib
    e = master_engine
    z = np.zeros(3)
    with pytest.raises(_lib.PhgpuError, match="G 33"):
        e.lshaped_init(33, 4, 0, 3, np.zeros((0, 3)), [], [], z, z + 1, np.zeros(33))
    with pytest.raises(_lib.PhgpuError, match="n_rows 65"):
        e.lshaped_init(1, 4, 0, 3, np.zeros((65, 3)), np.zeros(65), np.ones(65), z, z + 1, np.zeros(1))


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("S,cm,G", [(3, 1, 3), (3, 1, 1), (30, 1, 8), (130, 1, None), (12, 2, None)])
def test_lshaped_reaches_the_ef_optimum(gpu, S, cm, G):
    ref, (ef_obj, ef_x) = _ref(S, cm, G)
    opt = _opt(S=S, cm=cm, **({} if G is None else {"cut_groups": G}))
    try:
        res = opt.lshaped_algorithm()
        its = opt.iter + 1
        bounds = np.array([h[0] for h in opt.history])
        print(f"farmer S={S} cm={cm} G={opt.cut_groups}: {its} iterations (restatement {ref.iters}), master "
              f"iterations {[h[3] for h in opt.history]}, bound {opt._LShaped_bound:.6f}, E[f] {opt.Eobj_at_xhat:.6f}, "
              f"EF {ef_obj:.6f}")
        assert res["added"] == 0 and opt.first_stage_solution_available          # ended because no cut was added
        assert opt.cut_groups == ref.G
        assert abs(opt._LShaped_bound - ef_obj) <= REL * abs(ef_obj)
        assert abs(opt.Eobj_at_xhat - ef_obj) <= REL * abs(ef_obj)
        # the outer bound of every master but the last (whose candidate was not needed)
        # the series the method publishes: sum etalb, then every master's bound but the last one's
        # (whose candidate was not needed)
        inc = np.concatenate([[opt.batch.sense * opt.etalb.sum()], bounds[:-1]])
        assert np.all(np.diff(inc) >= -1e-9 * np.abs(inc[:-1]))
        assert its <= 3 * ref.iters
        if np.abs(ref.xhat - ef_x).max() <= 1e-7 * max(1.0, np.abs(ef_x).max()):   # the EF optimum is unique
            x = opt.current_xhat()
            assert np.all(np.abs(x - ef_x) <= REL * np.maximum(1.0, np.abs(ef_x))), (x, ef_x)
    finally:
        opt.engine.close()


def test_a_full_store_raises_instead_of_reporting_convergence(gpu):
    """max_cuts = 4 with three groups: the second iteration wants three cuts and one fits."""
    opt = _opt(S=3, max_cuts=4)
    try:
        with pytest.raises(RuntimeError, match="cut store is full"):
            opt.lshaped_algorithm()
        assert not opt.first_stage_solution_available and opt.iter == 1
        assert len(opt.engine.lshaped_export()[0]) == 4
    finally:
        opt.engine.close()


def test_a_maximisation_farmer(gpu):
    _, (ef_obj, _) = _ref(3, 1, 3)
    opt = _opt(S=3, sense=-1)
    try:
        opt.lshaped_algorithm()
        assert not opt.is_minimizing
        assert abs(opt._LShaped_bound + ef_obj) <= REL * abs(ef_obj)
        assert abs(opt.Eobj_at_xhat + ef_obj) <= REL * abs(ef_obj)
        assert opt._LShaped_bound >= opt.Eobj_at_xhat - REL * abs(ef_obj)          # an upper bound of the maximum
    finally:
        opt.engine.close()


def test_an_infeasible_subproblem_raises(gpu):
    """Scenario 0 may buy no corn: feasible on its own (it plants enough), infeasible at the first
    candidate, whose corn acreage is below its feed requirement."""
    opt = _opt(S=3)
    try:
        j = opt.batch.var_names.index("QuantityPurchased[CORN0]")
        opt.batch.ub[0, j] = 0.0
        with pytest.raises(RuntimeError, match="scen0 is infeasible"):
            opt.lshaped_algorithm()
    finally:
        if opt.engine is not None:
            opt.engine.close()


# ------------------------------------------------------------------ two gloo ranks on one GPU
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
        opt = _opt(S=12, mpicomm=Comm())
        opt.lshaped_algorithm()
        out = {"bound": opt._LShaped_bound, "Q": opt.Eobj_at_xhat, "iters": opt.iter + 1, "n": opt.batch.S,
               "xhat_bits": opt.engine.ls_xhat[:, 0].cpu().numpy().view(np.int64).tolist()}
        opt.engine.close()
        with open(os.path.join(out_dir, f"ls_r{rank}.json"), "w") as f:
            json.dump(out, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_give_the_one_rank_bound(gpu, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"ls_r{k}.json")) for k in range(2)]
    assert r[0]["n"] == r[1]["n"] == 6
    assert r[0]["xhat_bits"] == r[1]["xhat_bits"]                     # every rank solved the same master
    one = _opt(S=12)
    try:
        one.lshaped_algorithm()
        assert abs(r[0]["bound"] - one._LShaped_bound) <= 1e-9 * abs(one._LShaped_bound)
        assert r[0]["bound"] == r[1]["bound"]
    finally:
        one.engine.close()


# ------------------------------------------------------------------ a wheel
def test_wheel_with_the_lshaped_hub(gpu):
    """LShapedHub + XhatLShapedInnerBound on farmer, 3 scenarios: ends on its gap, inner >= outer."""
    from types import SimpleNamespace
    from mpisppy_amd.cylinders.hub import LShapedHub
    from mpisppy_amd.cylinders.lshaped_bounder import XhatLShapedInnerBound
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.spin_the_wheel import WheelSpinner
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    _, (ef_obj, _) = _ref(3, 1, 3)
    names = farmer.scenario_names_creator(3)
    cfg = SimpleNamespace(solver_name=SOLVER, max_iterations=30, rel_gap=1e-4, device="cuda:0", toc=False)
    kw = {"num_scens": 3}
    hub = vanilla.lshaped_hub(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
    spokes = [vanilla.xhatlshaped_spoke(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)]
    ws = WheelSpinner(hub, spokes)
    ws.spin(placement="colocated")
    h = ws.spcomm
    try:
        assert isinstance(h, LShapedHub) and isinstance(ws.spokes[0], XhatLShapedInnerBound)
        assert h.innerbound_spoke_chars == {1: "X"}
        abs_gap, rel_gap = h.compute_gaps()
        assert rel_gap <= 1e-4 and h.opt.iter + 1 < 30                            # ended on its gap
        assert ws.BestInnerBound >= ws.BestOuterBound - 1e-9 * abs(ef_obj)
        assert ws.BestOuterBound <= ef_obj + REL * abs(ef_obj) and ws.BestInnerBound >= ef_obj - REL * abs(ef_obj)
    finally:
        for s in ws.spokes:
            s.opt.engine.close()
        h.opt.engine.close()
