"""NormRhoUpdater and the convergers on the device (phgpu_ph_residuals /
phgpu_norm_rho_update, include/phgpu.h) against the numpy restatement of
mpisppy/extensions/norm_rho_updater.py and mpisppy/convergers/ in tests/norm_rho_ref.py.

* the four residual planes and rho_last against numpy sums over the engine's own arrays
  (rtol 1e-13 / atol 1e-12 as tests/test_gpu_readback.py; garbage in the outputs beforehand);
* the update kernel on constructed residuals: the four actions, exact ties, allow_decrease;
* PH with NormRhoUpdater against the stepped oracle on the three cases whose trajectories
  keep clear of every threshold (tests/test_norm_rho.py asserts that on the CPU): rho at rtol
  1e-13 (a wrong decision is a factor 2 or 1.1), W / x̄ / conv at 1e-5, the trivial bound at
  1e-5 relative (the tolerances of tests/test_variable_probability.py);
* two gloo ranks on one GPU; the speculative solve on and off; the two convergers.
"""
import json
import os
import socket

import numpy as np
import pytest
import torch

import norm_rho_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OBJ_REL = 1e-5
ABS = 1e-5


# ------------------------------------------------------------------ the kernels alone
def _engine(model, S, bf=None):
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.examples import aircond, farmer
    if model == "farmer":
        b = farmer.batch_creator(farmer.scenario_names_creator(S), crops_multiplier=1, num_scens=S)
    else:
        b = aircond.batch_creator(aircond.scenario_names_creator(S), branching_factors=bf, **R.AIR_KW)
    # "aircond_shared": a PHGPU_SHARED_MATRIX handle (aircond's matrix is the same in every scenario)
    return PHEngine(b, device="cuda:0", shared=True if model == "aircond_shared" else None)


def _keys(e):
    """[nn, S] index of (node, offset) of every local (nonant, scenario) in a plane."""
    b = e.batch
    node_of = e.node_of.cpu().numpy().reshape(-1, e.S)
    return np.stack([node_of[int(b.nonant_depth[k])] * e.nlen_max + int(b.nonant_off[k]) for k in range(e.nn)])


def _expected_residuals(e, pvar=None):
    b = e.batch
    key = _keys(e)
    half = e.num_nodes * e.nlen_max
    x = e.x.cpu().numpy()[np.asarray(b.nonant_col)]
    xbar, rho = e.xbar.cpu().numpy()[:e.nn], e.rho.cpu().numpy()[:e.nn]
    prob = e.prob.cpu().numpy()
    pc = e.prob_coeff.cpu().numpy().reshape(-1, e.S)[np.asarray(b.nonant_depth)] if pvar is None else pvar.T
    ad = np.abs(x - xbar)
    planes = np.zeros((4, half))
    for j, v in enumerate((prob * ad, pc * ad, rho, prob * rho)):
        np.add.at(planes[j], key, v)
    last = np.zeros(half)
    for s in range(e.S):                          # scenario order: the last one of a node wins
        last[key[:, s]] = rho[:, s]
    return planes, last


def _random_state(e, seed, pow2_rho=False):
    rng = np.random.default_rng(seed)
    e.x.copy_(torch.as_tensor(rng.normal(0.0, 50.0, (e.n, e.S)), device=e.device))
    e.set_xbar(rng.normal(0.0, 50.0, (e.S, e.nn)))
    e.set_rho(2.0 ** rng.integers(-2, 3, (e.S, e.nn)) if pow2_rho else rng.uniform(0.1, 10.0, (e.S, e.nn)))
    return rng


@pytest.mark.parametrize("model,S,bf", [("farmer", 1000, None),       # two-stage, ragged last wave
                                        ("aircond", 128, [2, 64]),    # nodes aligned to waves
                                        ("aircond", 24, [4, 3, 2]),   # waves span several nodes
                                        ("aircond_shared", 24, [4, 3, 2])])
def test_residual_planes_against_numpy(gpu, model, S, bf):
    from mpisppy_amd import _lib
    e = _engine(model, S, bf)
    assert e.shared == (model == "aircond_shared")
    ws0 = e.workspace_bytes()
    rng = _random_state(e, 11)
    e._resid_bufs()
    for pvar in (None, "vp"):
        if pvar is not None:                      # plane 1 follows pvar, plane 0 does not
            vp = rng.random((e.S, e.nn))
            vp[e.S // 2] = 0.0
            e.set_nonant_probs(vp)
            pvar = vp
        ref, last = _expected_residuals(e, pvar)
        for _ in range(2):
            e.resid.fill_(1e30)                   # stale data must not survive
            e.rho_last.fill_(1e30)
            e.residuals()
            got = e.residual_planes()
            for j in range(4):
                np.testing.assert_allclose(got[j], ref[j], rtol=1e-13, atol=1e-12, err_msg=f"plane {j}")
            assert np.array_equal(e.rho_last.cpu().numpy(), last)
        if pvar is not None:
            plain, _ = _expected_residuals(e, None)
            assert np.abs(ref[1] - plain[1]).max() > 1e-3        # the weights do change plane 1
    assert e.calls["ph_residuals"] == 4 and e.calls["allreduce_resid"] == 0
    # its partials are workspace of its own, allocated at the first call
    assert e.workspace_bytes() == ws0 + ((e.S + 63) // 64) * e.nn * (4 * 8 + 4)
    # the update on this shape (several blocks per nonant on farmer 1,000): the decisions from
    # the device's own plane 0, so none of them depends on the last bits of a sum
    half = e.num_nodes * e.nlen_max
    key = _keys(e)
    e.node_buf[:half].copy_(torch.as_tensor(rng.normal(0.0, 1.0, half), device=e.device))
    e.xbar_snapshot()
    prev = e.node_buf[:half].cpu().numpy().copy()
    e.node_buf[:half].copy_(torch.as_tensor(prev + rng.normal(0.0, 1.0, half), device=e.device))
    tol, f = 10.0, 2.0
    d = e.rho_last.cpu().numpy() * np.abs(e.node_buf[:half].cpu().numpy() - prev)
    act = R.actions(e.residual_planes()[0], d, tol, f, True)
    rho0 = e.rho.cpu().numpy()[:e.nn].copy()
    e.norm_rho_update(_lib.NormRhoParams(tol=tol, inc=2.0, dec=2.0, conv_dec=1.1, f=f, allow_decrease=1))
    np.testing.assert_allclose(e.rho.cpu().numpy()[:e.nn], R.apply_actions(rho0, act[key], R.DEFAULTS), rtol=1e-14,
                               atol=0)
    assert e.norm_rho_counts().tolist() == np.bincount(act[key].ravel(), minlength=4).tolist()
    e.close()


def test_update_kernel_on_constructed_residuals(gpu):
    """aircond 4-3-2: per (node, nonant) one of seven situations -- increase, decrease,
    converged decrease, the exact ties p = f d, p = tol, d = tol, and neither -- with rho
    different between the scenarios of a node, so that d carries the last scenario's rho."""
    from mpisppy_amd import _lib
    e = _engine("aircond", 24, [4, 3, 2])
    _random_state(e, 5, pow2_rho=True)
    e.residuals()
    _, last = _expected_residuals(e)
    assert np.array_equal(e.rho_last.cpu().numpy(), last)
    key = _keys(e)
    half = e.num_nodes * e.nlen_max
    tol, f = 0.5, 2.0
    P = np.array([4.0, 1.0, 0.25, 2.0, 0.5, 0.25, 1.0])
    D = np.array([1.0, 4.0, 0.25, 1.0, 0.25, 0.5, 1.0])
    want_kind = np.array([R.INC, R.DEC, R.CONV, R.NONE, R.NONE, R.NONE, R.NONE])
    kind = np.arange(half) % 7
    p, d = P[kind], D[kind]
    reached = last > 0
    delta = np.where(reached, d / np.where(reached, last, 1.0), 0.0)     # exact: rho is a power of two
    assert np.array_equal(last * delta, np.where(reached, d, 0.0))
    rho0 = e.rho.cpu().numpy()[:e.nn].copy()
    # the first scenario's rho differs from the last one's at some node: the quirk matters
    first = np.zeros(half)
    for s in range(e.S - 1, -1, -1):
        first[key[:, s]] = rho0[:, s]
    assert (first != last).any()
    e.xbar_snapshot()
    for allow in (1, 0):
        e.rho[:e.nn].copy_(torch.as_tensor(rho0, device=e.device))
        e.resid[:half].copy_(torch.as_tensor(p, device=e.device))
        e.node_buf[:half].copy_(torch.as_tensor(delta, device=e.device))
        e._xbar_prev.zero_()
        prm = _lib.NormRhoParams(tol=tol, inc=2.0, dec=2.0, conv_dec=1.1, f=f, allow_decrease=allow)
        e.norm_rho_update(prm)
        act = R.actions(p, last * delta, tol, f, bool(allow))
        want = np.where((want_kind[kind] == R.DEC) & (allow == 0), R.NONE, want_kind[kind])
        assert np.array_equal(act[reached], want[reached])
        ref = R.apply_actions(rho0, act[key], R.DEFAULTS)
        np.testing.assert_allclose(e.rho.cpu().numpy()[:e.nn], ref, rtol=1e-14, atol=0)
        counts = np.bincount(act[key].ravel(), minlength=4)
        assert e.norm_rho_counts().tolist() == counts.tolist()
        assert (counts[[R.NONE, R.INC, R.CONV]] > 0).all() and (counts[R.DEC] > 0) == bool(allow)
        # the snapshot was renewed with the node x̄ the update used
        assert np.array_equal(e._xbar_prev.cpu().numpy(), delta)
    e.close()


# ------------------------------------------------------------------ PH against the stepped oracle
def _ph(case, iters, thresh=-1.0, updater=True, converger=None, spec=True, mpicomm=None, **extra):
    from mpisppy_amd.extensions.norm_rho_updater import NormRhoUpdater
    from mpisppy_amd.opt.ph import PH
    opts = {"solver_name": "mi355x_pdhg", "PHIterLimit": iters, "defaultPHrho": 1.0, "convthresh": thresh,
            "verbose": False, "display_progress": False, "toc": False, "device": "cuda:0",
            "speculative_solve": spec, "fused_ph_loop": False,
            "norm_rho_options": {"primal_dual_difference_factor": R.CASES[case]["factor"]}}
    opts.update(extra)
    ext = NormRhoUpdater if updater else None
    if case.startswith("farmer"):
        from mpisppy_amd.examples import farmer
        S = int(case[6:])
        opts["batch_creator"] = farmer.batch_creator
        return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator, extensions=ext,
                  ph_converger=converger, mpicomm=mpicomm,
                  scenario_creator_kwargs={"crops_multiplier": 1, "num_scens": S})
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    opts["batch_creator"] = aircond.batch_creator
    return PH(opts, aircond.scenario_names_creator(24), aircond.scenario_creator, extensions=ext,
              ph_converger=converger, mpicomm=mpicomm,
              scenario_creator_kwargs=dict(R.AIR_KW, branching_factors=R.AIR_BF),
              all_nodenames=create_nodenames_from_branching_factors(R.AIR_BF))


def _state(ph):
    e = ph.engine
    return {"rho": e.host("rho")[:, :e.nn].copy(), "W": ph.W_array().copy(), "xbar": e.host("xbar")[:, :e.nn].copy(),
            "conv": ph.conv, "iter": ph._PHIter, "calls": dict(e.calls)}


def _assert_matches_oracle(ph, st, tb, case):
    o = st.o
    iters = R.CASES[case]["iters"]
    e = ph.engine
    rho = e.host("rho")[:, :e.nn]
    print(case, "max |rho - oracle| / oracle", np.abs(rho / o.rho - 1).max(), "max |W - oracle|",
          np.abs(ph.W_array() - o.W).max(), "conv", ph.conv, st.hist[-1]["conv"])
    np.testing.assert_allclose(rho, o.rho, rtol=1e-13, atol=0)
    assert np.abs(ph.W_array() - o.W).max() <= ABS
    nx = ph.xbar_by_node()
    want = st.node_xbar()
    for g, nd in enumerate(st.node_names):
        v = want[g * st.nlen_max:(g + 1) * st.nlen_max]
        assert np.abs(nx[nd][:len(v)] - v).max() <= ABS, nd
    assert abs(ph.conv - st.hist[-1]["conv"]) <= ABS
    assert abs(tb - st.trivial_bound) <= OBJ_REL * abs(st.trivial_bound)
    c = e.calls
    assert c["ph_residuals"] == iters - 1 and c["norm_rho_update"] == iters - 1, c
    assert e.norm_rho_counts().tolist() == st.log[-1]["counts"].tolist()


@pytest.mark.parametrize("case", ["farmer3", "farmer3_pdhg", "farmer1000", "aircond432"])
def test_ph_with_updater_matches_the_stepped_oracle(gpu, case, request):
    pdhg = case.endswith("_pdhg")
    if pdhg:                                   # every solve path picks up the changed rho
        request.getfixturevalue("register_path")
        case = case[:-5]
    st = R.trajectory(case)
    ph = _ph(case, R.CASES[case]["iters"])
    conv, _, tb = ph.ph_main(finalize=False)
    path = ph.engine.kernel_info()["path"]
    assert path != 6 if pdhg else (path == 6 or not case.startswith("farmer")), ph.engine.kernel_info()
    _assert_matches_oracle(ph, st, tb, case)
    ph.engine.close()


def test_verbose_table_reads_rho_back_and_leaves_the_loop_plain(gpu, capsys):
    """norm_rho_options['verbose']: the reference's table for the first local scenario; the
    only path that reads rho back, so the speculative solve is off; same rho as without it."""
    st = R.trajectory("farmer3")
    ph = _ph("farmer3", R.CASES["farmer3"]["iters"],
             norm_rho_options={"primal_dual_difference_factor": 2.0, "verbose": True})
    ph.ph_main(finalize=False)
    assert not ph._speculate(True) and ph.engine.calls["solve_deferred"] == 0
    np.testing.assert_allclose(ph.engine.host("rho")[:, :3], st.o.rho, rtol=1e-13, atol=0)
    out = capsys.readouterr().out
    rows = [ln for ln in out.splitlines() if ln.strip().startswith(("Increasing", "Decreasing", "Converged"))]
    assert out.count("Updating rho values:") == sum(1 for r in st.log if r["act"].any())
    assert len(rows) == sum(int((r["act"] != 0).sum()) for r in st.log)       # one row per nonant that acted
    ph.engine.close()


# ------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


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
        ph = _ph("aircond432", R.CASES["aircond432"]["iters"], mpicomm=Comm())
        conv, _, tb = ph.ph_main(finalize=False)
        s = _state(ph)
        res = {"rho": s["rho"].tolist(), "W": s["W"].tolist(), "conv": conv, "tb": tb, "calls": s["calls"],
               "names": list(ph.local_scenario_names), "spec": bool(ph._speculate(True)),
               "counts": ph.engine.norm_rho_counts().tolist()}
        ph.engine.close()
        with open(os.path.join(out_dir, f"nr_r{rank}.json"), "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_match_the_single_process_oracle(gpu, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"nr_r{k}.json")) for k in range(2)]
    st = R.trajectory("aircond432")
    iters = R.CASES["aircond432"]["iters"]
    assert r[0]["names"] + r[1]["names"] == [f"scen{i}" for i in range(24)]
    lo = 0
    for k in range(2):
        n = len(r[k]["names"])
        np.testing.assert_allclose(np.array(r[k]["rho"]), st.o.rho[lo:lo + n], rtol=1e-13, atol=0)
        assert np.abs(np.array(r[k]["W"]) - st.o.W[lo:lo + n]).max() <= ABS
        assert abs(r[k]["conv"] - st.hist[-1]["conv"]) <= ABS
        c = r[k]["calls"]
        assert r[k]["spec"] and c["solve_deferred"] == iters and c["ph_step_defer"] == 0, c
        assert c["ph_residuals"] == iters - 1 and c["allreduce_resid"] == iters - 1, c
        lo += n
    ar = [{k: v for k, v in r[j]["calls"].items() if k.startswith("allreduce")} for j in range(2)]
    assert ar[0] == ar[1], ar
    local = [np.bincount(st.log[-1]["act"][st.key[a:b]].ravel(), minlength=4).tolist() for a, b in ((0, 12), (12, 24))]
    assert [r[0]["counts"], r[1]["counts"]] == local


# ------------------------------------------------------------------ speculation
@pytest.mark.parametrize("case", ["farmer3", "aircond432"])
def test_speculative_solve_stays_on_and_invisible_with_the_updater(gpu, case):
    iters = R.CASES[case]["iters"]
    out = {}
    for spec in (True, False):
        ph = _ph(case, iters, spec=spec)
        ph.ph_main(finalize=False)
        assert ph._speculate(True) == spec and ph._miditer_early(True)
        out[spec] = _state(ph)
        ph.engine.close()
    a, b = out[True], out[False]
    assert a["iter"] == b["iter"] == iters and a["conv"] == b["conv"], (a["conv"], b["conv"])
    for k in ("rho", "W", "xbar"):
        assert np.array_equal(a[k], b[k]), (case, k, np.abs(a[k] - b[k]).max())
    # speculative solves ran, and no step was deferred into a solve launch
    assert a["calls"]["solve_deferred"] == iters and b["calls"]["solve_deferred"] == 0
    assert a["calls"]["ph_step_defer"] == 0 and b["calls"]["ph_step_defer"] == 0
    assert a["calls"]["norm_rho_update"] == b["calls"]["norm_rho_update"] == iters - 1


# ------------------------------------------------------------------ convergers
def test_primal_dual_converger_breaks_where_the_restatement_does(gpu):
    from mpisppy_amd.convergers.primal_dual_converger import PrimalDualConverger
    st = R.trajectory("farmer3")
    ph = _ph("farmer3", 12, converger=PrimalDualConverger, primal_dual_converger_options={"tol": R.PD_TOL})
    ph.ph_main(finalize=False)
    assert not ph._speculate(True)                 # a converger reads the host every iteration
    h = st.hist[R.PD_BREAK - 1]
    c = ph.convobject
    print("gaps", c.primal_gap, c.dual_gap, "oracle", h["primal"], h["dual"])
    assert ph.converged and ph._PHIter == R.PD_BREAK
    assert abs(c.primal_gap - h["primal"]) <= 1e-5 * max(1.0, abs(h["primal"]))
    assert abs(c.dual_gap - h["dual"]) <= 1e-5 * max(1.0, abs(h["dual"]))
    ph.engine.close()


def test_norm_rho_converger_value(gpu):
    from mpisppy_amd.convergers.norm_rho_converger import NormRhoConverger
    st = R.trajectory("farmer3")
    iters = 6
    ph = _ph("farmer3", iters, converger=NormRhoConverger)
    ph.ph_main(finalize=False)
    assert not ph.converged and ph._PHIter == iters
    assert abs(ph.convobject.conv - st.hist[iters - 1]["log_rho_norm"]) <= 1e-12
    ph.engine.close()
    plain = _ph("farmer3", 2, updater=False, converger=NormRhoConverger)
    with pytest.raises(RuntimeError, match="NormRhoConverger can only be used if NormRhoUpdater is"):
        plain.ph_main(finalize=False)
    plain.engine.close()
