"""PH with bundles on the device (bundles_per_rank; csrc/ph_ef.inc's segmented kernels, entries
phgpu_bundle_*) against exact solves of every bundle's extensive form
(tests/bundle_ref.py), the reference's own fixtures, ExtensiveForm, and numpy for the reduction."""
import csv
import json
import os
import socket

import numpy as np
import pytest
import torch

import bundle_ref as B

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ABS = 1e-5                 # W and x̄: the project's tolerance (BASELINE.json)
BOUND_REL = 1e-8
SOLVER = "mi355x_pdhg"


def _ph(S, cm=1, bpr=0, iters=10, creator=None, **o):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.ph import PH
    kw = {k: o.pop(k) for k in ("mpicomm", "extensions") if k in o}
    opts = {"solver_name": SOLVER, "PHIterLimit": iters, "defaultPHrho": 1.0, "convthresh": -1.0, "verbose": False,
            "display_progress": False, "toc": False, "device": "cuda:0"}
    if bpr:
        opts["bundles_per_rank"] = bpr
    opts.update(o)
    return PH(opts, farmer.scenario_names_creator(S), creator or farmer.scenario_creator,
              scenario_creator_kwargs={"num_scens": S, "crops_multiplier": cm}, **kw)


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.int64)


def _check_solve(ph):
    """After a bundled solve: every status OPTIMAL, the nonants bitwise equal within each bundle.
    Returns the bundles' interior-point iteration counts."""
    e = ph.engine
    st, it = e.status.cpu().numpy(), e.iters.cpu().numpy()
    assert np.all(st == 0), st
    nx = _bits(e.nonant_x_dev())                # [nn, S]
    counts = []
    for bd in ph.local_subproblems.values():
        assert np.array_equal(nx[:, bd.first:bd.last], np.broadcast_to(nx[:, bd.first:bd.first + 1], (e.nn, bd.last - bd.first)))
        assert np.all(it[bd.first:bd.last] == it[bd.first])
        counts.append(int(it[bd.first]))
    return counts


def _trajectory(ph, iters):
    """Iter0 and ``iters`` PH iterations step by step: (trivial bound, [W], [x̄ of ROOT], [conv], all the
    bundles' iteration counts)."""
    ph.PH_Prep()
    tb = ph.Iter0()
    counts = _check_solve(ph)
    Ws, xbars, convs = [], [], []
    for _ in range(iters):
        ph.Compute_Xbar()
        ph.Update_W()
        convs.append(ph.convergence_diff())
        Ws.append(ph.W_array().copy())
        xbars.append(ph.xbar_by_node()["ROOT"][:ph.batch.nn].copy())
        ph.solve_loop(solver_options=ph.current_solver_options)
        counts += _check_solve(ph)
    return tb, Ws, xbars, convs, counts


def _against_oracle(S, cm, bpr, iters):
    ora = B.farmer_run(S, cm, bpr, iters, "exact")
    ph = _ph(S, cm, bpr, iters)
    try:
        tb, Ws, xbars, convs, counts = _trajectory(ph, iters)
    finally:
        ph.engine.close()
    rel = abs(tb - ora.trivial_bound) / abs(ora.trivial_bound)
    dW = max((np.abs(W - h["W"]).max() for W, h in zip(Ws, ora.history)), default=0.0)
    dx = max((np.abs(x - h["xbar"][0]).max() for x, h in zip(xbars, ora.history)), default=0.0)
    print(f"farmer S={S} cm={cm} bundles={bpr}: trivial bound {tb:.6f} oracle {ora.trivial_bound:.6f} ({rel:.1e}); over {iters} "
          f"iterations max |dW| {dW:.2e} max |dxbar| {dx:.2e}; interior-point iterations {min(counts)}..{max(counts)}")
    assert rel <= BOUND_REL
    return dW, dx, counts


# ------------------------------------------------------------------ 1: trajectory, unequal segments
def test_trajectory_unequal_segments(gpu):
    """Farmer S = 10, cm = 1, 3 bundles (3, 3, 4), rho = 1, 10 iterations.

    With the residual test alone (bundle_tol 1e-10) the device measured max |dW| 7.71e-5 and max
    |dx̄| 5.01e-5, all from one solve (the third bundle after PH iteration 1, a nearly degenerate
    vertex: gap binding, z 1.3e-4 off).  A bundle now also has to bring the predictor's step of z
    under bundle_step_tol: with it the device measures 3.35e-6 / 1.99e-6, 14 to 20
    interior-point iterations (the host build of the kernels 3.4e-6 / 2.0e-6 on the engine's model)."""
    dW, dx, counts = _against_oracle(10, 1, 3, 10)
    assert dW <= ABS and dx <= ABS
    assert len(set(counts)) >= 2                # bundles ended at different iterations: per-segment termination ran


# ------------------------------------------------------------------ 2: a segment crossing a wave and a block
def test_segments_cross_a_wave_and_a_block(gpu):
    """S = 130 in 7 bundles of 18 and 19: more than one block of 128 lanes; bundles straddle lanes 64 and 128."""
    ph = _ph(130, 1, 7, 2)
    seg = [(b.first, b.last) for b in ph.local_subproblems.values()]
    assert sorted({b - a for a, b in seg}) == [18, 19]
    assert any(a < 64 < b for a, b in seg) and any(a < 128 < b for a, b in seg)
    dW, dx, counts = _against_oracle(130, 1, 7, 2)
    assert dW <= ABS and dx <= ABS


# ------------------------------------------------------------------ 3: the segmented reduction alone
def test_segmented_reduction_matches_numpy_and_repeats(gpu):
    ph = _ph(130, 1, 7, 1)
    try:
        ph.PH_Prep()
        ph._create_solvers()
        e = ph.engine
        runs = []
        for _ in range(2):
            e.bundle_start()
            rsum, rmax, terms = e.bundle_schur(0, inspect=True)
            torch.cuda.synchronize()
            runs.append((rsum.cpu().numpy(), rmax.cpu().numpy(), terms.cpu().numpy()))
        rsum, rmax, terms = runs[0]
        nsum = e.bundle_nsum0
        assert rsum.shape == (7, nsum) and terms.shape == (nsum + 2, 130) and np.any(rsum != 0.0)
        worst = 0.0
        for g, bd in enumerate(ph.local_subproblems.values()):
            t = terms[:, bd.first:bd.last]
            ref_s, ref_m = t[:nsum].sum(axis=1), t[nsum:].max(axis=1)
            err = np.abs(rsum[g] - ref_s) / np.maximum(np.abs(ref_s), 1e-300)
            err[ref_s == rsum[g]] = 0.0
            worst = max(worst, err.max())
            assert np.all(err <= 1e-10), (g, err.max())
            assert np.array_equal(rmax[g], ref_m)
        print(f"segmented reduction: worst relative difference from numpy {worst:.1e}")
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a.view(np.int64), b.view(np.int64))      # the same bits on every run
    finally:
        ph.engine.close()


# ------------------------------------------------------------------ 4: the two ends
def test_one_bundle_is_the_extensive_form(gpu):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.ef import ExtensiveForm
    S = 10
    ef = ExtensiveForm({"solver": SOLVER, "toc": False, "device": "cuda:0"}, farmer.scenario_names_creator(S),
                       farmer.scenario_creator, scenario_creator_kwargs={"num_scens": S})
    try:
        ef.solve_extensive_form(solver_options={"tol": 1e-10})
        z, obj = ef.root_nonants().copy(), ef.get_objective_value()
    finally:
        ef.engine.close()
    ph = _ph(S, 1, 1, 1)
    try:
        ph.PH_Prep()
        tb = ph.Iter0()
        x0 = ph.nonants_array().copy()
        ph.Compute_Xbar()
        ph.Update_W()
        conv = ph.convergence_diff()
    finally:
        ph.engine.close()
    print(f"one bundle: |nonants - EF z| {np.abs(x0 - z).max():.1e}, trivial bound {tb:.8f} EF {obj:.8f}, conv {conv:.1e}")
    assert np.abs(x0 - z).max() <= 1e-8
    assert abs(tb - obj) <= BOUND_REL * abs(obj)
    assert conv < 1e-10


def test_a_bundle_per_scenario_is_plain_ph(gpu):
    """bundles_per_rank = S on farmer (3 scenarios), rho = 1, 5 iterations: the reference's own W and x̄ files."""
    ph = _ph(3, 1, 3, 5)
    try:
        ph.ph_main()
        W, xbar = ph.W_array(), ph.xbar_by_node()["ROOT"]
        names, vnames = ph.local_scenario_names, list(ph.batch.nonant_names)
    finally:
        ph.engine.close()
    with open(os.path.join(HERE, "golden", "ref_w_file.csv")) as f:
        ref_w = {(r[0], r[1]): float(r[2]) for r in csv.reader(f)}
    with open(os.path.join(HERE, "golden", "ref_xbar_file.csv")) as f:
        ref_x = {r[0]: float(r[1]) for r in csv.reader(f)}
    dW = max(abs(W[s, k] - ref_w[nm, vn]) for s, nm in enumerate(names) for k, vn in enumerate(vnames))
    dx = max(abs(xbar[k] - ref_x[vn]) for k, vn in enumerate(vnames))
    print(f"a bundle per scenario: |W - reference| {dW:.1e} |xbar - reference| {dx:.1e}")
    assert dW <= ABS and dx <= ABS


# ------------------------------------------------------------------ 5: cm = 2 (a non-unique Iter0 LP: bounds only)
def test_cm2_trivial_bound(gpu):
    _against_oracle(12, 2, 4, 0)


# ------------------------------------------------------------------ 6: the Lagrangian pass
def test_lagrangian_pass(gpu):
    """W of the oracle's iteration 5, W on, prox off: Ebound against the exact LP of every bundle."""
    src = B.farmer_run(10, 1, 3, 10, "exact")
    W = src.history[4]["W"]
    ora = B.BundlePH(src.scens, 1.0, 3)
    ora.W, ora.W_on, ora.prox_on = W.copy(), 1, 0
    ora.solve_loop()
    want = ora.Ebound()
    ph = _ph(10, 1, 3, 1)
    try:
        ph.PH_Prep(attach_prox=False)
        ph._create_solvers()
        ph.engine.set_W(W)
        ph.engine.set_terms(1, 0)
        ph.solve_loop(solver_options=ph.current_solver_options, gripe=True)
        _check_solve(ph)
        got = ph.Ebound()
    finally:
        ph.engine.close()
    print(f"Lagrangian pass: Ebound {got:.6f} exact {want:.6f} ({abs(got - want) / abs(want):.1e})")
    assert abs(got - want) <= BOUND_REL * abs(want)


# ------------------------------------------------------------------ 7: two ranks
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
        ph = _ph(12, 1, 2, 3, mpicomm=Comm())
        tb, Ws, xbars, convs, counts = _trajectory(ph, 3)
        out = {"tb": tb, "xbar": xbars[-1].tolist(), "names": ph.names_in_bundles[rank], "n": ph.batch.S}
        ph.engine.close()
        with open(os.path.join(out_dir, f"bundle_r{rank}.json"), "w") as f:
            json.dump(out, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_give_the_one_rank_trajectory(gpu, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"bundle_r{k}.json")) for k in range(2)]
    assert r[0]["n"] == r[1]["n"] == 6 and r[0]["xbar"] == r[1]["xbar"]
    one = _ph(12, 1, 4, 3)
    try:
        # the same bundles: rank r's two are the one-rank run's 2r and 2r + 1
        both = [r[k]["names"][str(b)] for k in range(2) for b in range(2)]
        assert both == [one.names_in_bundles[0][b] for b in range(4)]
        tb, Ws, xbars, convs, counts = _trajectory(one, 3)
    finally:
        one.engine.close()
    d = np.abs(np.array(r[0]["xbar"]) - xbars[-1]).max()
    print(f"two ranks x two bundles against one rank x four: |dxbar| {d:.1e}, trivial bound {r[0]['tb']:.8f} / {tb:.8f}")
    assert d <= 1e-9
    assert abs(r[0]["tb"] - tb) <= 1e-12 * abs(tb)


# ------------------------------------------------------------------ 8: refusals
def test_refusals(gpu, capsys):
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.extensions.fixer import Fixer
    from mpisppy_amd.opt.ph import PH
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    with pytest.raises(NotImplementedError, match="Fixer is not served with bundles"):
        _ph(6, 1, 2, 2, extensions=Fixer, fixeroptions={"boundtol": 0.01, "id_fix_list_fct": None})
    bfs = [2, 2]
    with pytest.raises(RuntimeError, match="bundles serve two-stage problems only"):
        PH({"solver_name": SOLVER, "PHIterLimit": 1, "defaultPHrho": 1.0, "convthresh": 1e-8, "verbose": False,
            "display_progress": False, "toc": False, "device": "cuda:0", "bundles_per_rank": 2},
           aircond.scenario_names_creator(4), aircond.scenario_creator,
           all_nodenames=create_nodenames_from_branching_factors(bfs),
           scenario_creator_kwargs={"branching_factors": bfs, "start_seed": 1134})
    with pytest.raises(NotImplementedError, match="shared-matrix handle"):
        _ph(6, 1, 2, 2, shared_matrix=True)
    # the library's own refusal of a shared-matrix handle (every scenario given scenario 0's matrix)
    from mpisppy_amd import _lib
    from mpisppy_amd.engine import PHEngine
    ph = _ph(6, 1, 0, 1)
    ph.batch.A_val[:] = ph.batch.A_val[0]
    eng = PHEngine(ph.batch, device="cuda:0", shared=True)
    try:
        with pytest.raises(_lib.PhgpuError, match="shared-matrix handle is not served"):
            eng.bundle_init([0, 3, 6], np.zeros((2, 3)), np.full((2, 3), 500.0), [10.0, 10.0], [1.0, 1.0], 1e-10, 1e-8, 0)
    finally:
        eng.close()
    # the iteration limit: no bundle passes in 3 iterations
    ph = _ph(10, 1, 3, 1, bundle_max_iter=3)
    try:
        ph.PH_Prep()
        capsys.readouterr()
        ph.Iter0()
        out = capsys.readouterr().out
        st, it = ph.engine.status.cpu().numpy(), ph.engine.iters.cpu().numpy()
        assert np.all(st == 1) and np.all(it == 3)
        for name in ("rank0bundle0", "rank0bundle1", "rank0bundle2"):
            assert f"Solve of bundle {name} ended without optimality" in out
        assert not ph.trivial_bound_converged
        ph.Compute_Xbar()
        ph.Update_W()
        xbar = ph.xbar_by_node()["ROOT"]
        assert np.all(np.isfinite(xbar)) and np.all(np.isfinite(ph.W_array())) and np.all(np.isfinite(ph.nonants_array()))
    finally:
        ph.engine.close()
