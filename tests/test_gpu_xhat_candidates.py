"""The xhat candidates that are functions of all scenarios, on the device
(phgpu_nonant_stats / phgpu_nonant_closest, include/phgpu.h) against the numpy restatement of
mpisppy/extensions/xhatxbar.py, xhatclosest.py and cylinders/slam_heuristic.py in
tests/xhat_cand_ref.py.

* the four planes: max / -min bitwise, the two sums within 1e-12 x sum |terms| of an fsum
  restatement (the fp64 bound for at most 258 terms, 258 x 2^-53 ~ 3e-14 of that, leaves a
  margin of about 30), on two-stage and multistage trees, with variable probabilities, and
  against phgpu_ph_reduce's node_buf for the nonants of a solved x;
* dist / best: 1e-9 relative on columns whose standard deviation is at least 3 % of |mean|
  (cancellation in var then costs under 1e-12 relative), the cap at 3, an exactly constant
  column skipped, exact ties to the lowest index, -3 on a multistage handle;
* XhatXbar, XhatClosest, the slam heuristics and XhatXbarInnerBound on farmer 30 from the
  oracle hub's nonants at PH iterations 1, 2, 3 and 5 against oracle.wheel.xhat_objective
  (1e-5 relative, the project's objective tolerance); XhatXbar on aircond 4-3-2;
* a farmer wheel with the new spokes, one of them on its own rank; the post_everything form
  on a PH object; two gloo ranks on one GPU.
"""
import json
import os
import socket

import numpy as np
import pytest
import torch

import xhat_cand_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OBJ_REL = 1e-5
SUM_REL = 1e-12            # of sum |terms| (see above)
FARMER_EF_OBJ = -108390.0  # farmer 3 scenarios EF optimum (test_sc.py:30-38)
AIR_KW = dict(Capacity=200, QuadShortCoeff=0.3, BeginInventory=50, mu_dev=0, sigma_dev=40, start_seed=0)


# ------------------------------------------------------------------ the kernels alone
def _engine(model, S, bf=None):
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.examples import aircond, farmer
    if model == "farmer":
        b = farmer.batch_creator(farmer.scenario_names_creator(S), crops_multiplier=1, num_scens=S)
    else:
        b = aircond.batch_creator(aircond.scenario_names_creator(S), branching_factors=bf, **AIR_KW)
    return PHEngine(b, device="cuda:0")


def _key_pcoef(e, pvar=None):
    b = e.batch
    key = R.keys(e.node_of.cpu().numpy().reshape(-1, e.S), b.nonant_depth, b.nonant_off, e.nlen_max)
    pc = e.prob_coeff.cpu().numpy().reshape(-1, e.S)[np.asarray(b.nonant_depth)] if pvar is None else pvar.T
    return key, pc


def _dev(e, a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=e.device)


def _assert_planes(got, ref, mag):
    got = np.asarray(got).reshape(4, -1)
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    for j in (0, 1):
        err = np.abs(got[j] - ref[j])
        print(f"plane {j}: max err / sum|terms| = {np.max(err / np.maximum(mag[j], 1e-300)):.3e}")
        assert (err <= SUM_REL * mag[j]).all(), (j, err.max())


@pytest.mark.parametrize("model,S,bf,vp", [("farmer", 1, None, False), ("farmer", 64, None, False),
                                           ("farmer", 65, None, True), ("farmer", 257, None, False),
                                           ("aircond", 24, [4, 3, 2], False),     # waves span several nodes
                                           ("aircond", 258, [3, 86], True)])      # node boundaries cut waves
def test_planes_against_the_restatement(gpu, model, S, bf, vp):
    e = _engine(model, S, bf)
    assert e.S == S and (model != "farmer" or e.nn == 3)
    half = e.num_nodes * e.nlen_max
    rng = np.random.default_rng(S)
    ws0 = e.workspace_bytes()
    pvar = None
    if vp:
        pvar = rng.random((e.S, e.nn))
        pvar[e.S // 2] = 0.0
        e.set_nonant_probs(pvar)
    key, pc = _key_pcoef(e, pvar)
    for trial in range(2):
        v = rng.normal(20.0, 50.0, (e.nn, e.S))
        ref, mag = R.planes(v, key, pc, half)
        if trial:
            e.nstats.fill_(1e30)                  # stale data must not survive
        got = e.nonant_stats(_dev(e, v)).cpu().numpy()
        assert got.shape == (4, e.num_nodes, e.nlen_max)
        _assert_planes(got, ref, mag)
    if vp:                                        # the weights do change the sums
        plain, _ = R.planes(v, key, _key_pcoef(e)[1], half)
        assert np.abs(plain[0] - ref[0]).max() > 1e-3
    reached = np.zeros(half, dtype=bool)
    reached[np.unique(key)] = True
    assert (ref[0][~reached] == 0).all() and np.isneginf(ref[2][~reached]).all()
    assert e.calls["nonant_stats"] == 2 and e.calls["allreduce_stats_sum"] == 0
    # its partials are workspace of its own, allocated at the first call
    assert e.workspace_bytes() == ws0 + ((e.S + 63) // 64) * e.nn * (4 * 8 + 4)
    e.close()


@pytest.mark.parametrize("model,S,bf", [("farmer", 65, None), ("aircond", 24, [4, 3, 2])])
def test_sums_against_ph_reduce(gpu, model, S, bf):
    """With v the nonant rows of a solved x, planes 0-1 are phgpu_ph_reduce's node_buf."""
    e = _engine(model, S, bf)
    e.solve(warm=False)
    v = e.nonant_x_dev()
    key, pc = _key_pcoef(e)
    half = e.num_nodes * e.nlen_max
    _, mag = R.planes(v.cpu().numpy(), key, pc, half)
    nb = e.compute_xbar().cpu().numpy().reshape(2, half)
    got = e.nonant_stats(v).cpu().numpy().reshape(4, half)
    assert np.abs(nb[0]).max() > 1.0
    for j in (0, 1):
        assert (np.abs(got[j] - nb[j]) <= SUM_REL * mag[j]).all(), (j, np.abs(got[j] - nb[j]).max())
    e.close()


def _spread(rng, nn, S):
    """[nn, S] with per-column standard deviation 10 % of |mean| (>= 3 %)."""
    mean = np.array([100.0, 250.0, 170.0])[:nn]
    return mean[:, None] * (1.0 + 0.1 * rng.standard_normal((nn, S)))


@pytest.mark.parametrize("S", [1, 64, 65, 257, 1000])
def test_dist_and_best(gpu, S):
    e = _engine("farmer", S)
    rng = np.random.default_rng(100 + S)
    v = _spread(rng, e.nn, S)
    if S > 8:
        v[:, 5] = v.mean(1) * 2.0                 # one scenario > 3 sigma out in every column
    key, pc = _key_pcoef(e)
    ref, _ = R.planes(v, key, pc, e.nn)
    dist = R.distances(v, ref[0], ref[1])
    dmin, win = R.local_winner(dist)
    got = e.closest_scenario(_dev(e, v), _dev(e, ref[0]), _dev(e, ref[1]))
    gd = e.closest_dist.cpu().numpy()
    if S == 1:
        assert got == (0.0, 0, 0) and gd[0] == 0.0
    else:
        print(f"S={S}: max rel err of dist {np.max(np.abs(gd - dist) / dist):.3e}; winner {win}")
        np.testing.assert_allclose(gd, dist, rtol=1e-9, atol=0)
        srt = np.sort(dist)
        assert srt[1] - srt[0] > 1e-7 * srt[0]     # the winner does not hang on the last bits
        assert got[1:] == (0, win) and abs(got[0] - dmin) <= 1e-9 * dmin
        assert got[0] == gd[win]
    if S > 8:
        assert dist[5] == 3.0 * e.nn and gd[5] == 3.0 * e.nn      # the cap
    e.close()


def test_constant_column_is_skipped(gpu):
    """S = 64, p = 1/64, one column constant at 3.0: x̄ = 3 and x̄² = 9 exactly (sums of 64
    equal dyadic terms), so var is exactly 0 with or without FMA contraction and the strict
    test skips the column."""
    S = 64
    e = _engine("farmer", S)
    rng = np.random.default_rng(7)
    v = _spread(rng, e.nn, S)
    v[1] = 3.0
    pl = e.nonant_stats(_dev(e, v)).clone()
    assert pl[0, 0, 1].item() == 3.0 and pl[1, 0, 1].item() == 9.0
    xb, xs = pl[0, 0].cpu().numpy(), pl[1, 0].cpu().numpy()
    d, r, i = e.closest_scenario(_dev(e, v), pl[0, 0], pl[1, 0])
    gd = e.closest_dist.cpu().numpy()
    two = R.distances(v[[0, 2]], xb[[0, 2]], xs[[0, 2]])           # the restatement without the column
    np.testing.assert_allclose(gd, two, rtol=1e-9, atol=0)
    assert np.array_equal(R.distances(v, xb, xs), two)
    # had the column counted, every distance would differ: make its variance positive
    xs2 = xs.copy()
    xs2[1] = 9.0 + 1e-6
    e.closest_scenario(_dev(e, v), _dev(e, xb), _dev(e, xs2))
    assert np.array_equal(e.closest_dist.cpu().numpy(), gd)        # |3 - 3| / sd = 0: still nothing added
    v2 = v.copy()
    v2[1, 10] = 3.5
    e.closest_scenario(_dev(e, v2), _dev(e, xb), _dev(e, xs2))
    assert abs(e.closest_dist.cpu().numpy()[10] - (gd[10] + 3.0)) <= 1e-12      # capped at 3
    assert (r, i) == (0, R.local_winner(two)[1]) and d == gd[i]
    e.close()


@pytest.mark.parametrize("S,a,b", [(64, 7, 40), (257, 3, 256), (1000, 300, 700)])
def test_exact_ties_go_to_the_lowest_index(gpu, S, a, b):
    """Two identical scenarios (bitwise equal distances; in one wave, in two blocks) nearest
    to the given x̄: the lower index wins, as the reference's strict < scan."""
    e = _engine("farmer", S)
    rng = np.random.default_rng(S)
    v = _spread(rng, e.nn, S)
    v[:, b] = v[:, a]
    xb = v[:, a] * (1.0 + 1e-3)
    xs = xb * xb + (0.1 * xb) ** 2
    dist = R.distances(v, xb, xs)
    assert dist[a] == dist[b] == dist.min() and (dist == dist.min()).sum() == 2
    d, r, i = e.closest_scenario(_dev(e, v), _dev(e, xb), _dev(e, xs))
    gd = e.closest_dist.cpu().numpy()
    assert gd[a] == gd[b] == gd.min()
    assert (r, i) == (0, a) and d == gd[a]
    e.close()


def test_closest_refuses_a_multistage_handle(gpu):
    from mpisppy_amd import _lib
    e = _engine("aircond", 24, [4, 3, 2])
    v = torch.zeros(e.nn, e.S, dtype=torch.float64, device=e.device)
    z = torch.zeros(e.nlen_max, dtype=torch.float64, device=e.device)
    best = torch.full((2,), 7.0, dtype=torch.float64, device=e.device)
    rc = e.lib.phgpu_nonant_closest(e.h, v.data_ptr(), z.data_ptr(), z.data_ptr(), None, best.data_ptr(), None)
    assert rc == -3 and "two-stage" in _lib.last_error()
    torch.cuda.synchronize()
    assert best.cpu().tolist() == [7.0, 7.0]                      # nothing launched
    with pytest.raises(_lib.PhgpuError):
        e.closest_scenario(v, z, z)
    e.close()


# ------------------------------------------------------------------ the classes on farmer 30
def _farmer_xhat_eval(S=R.FARMER_S, mpicomm=None, **extra):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    opts = {"solver_name": "mi355x_pdhg", "verbose": False, "toc": False, "device": "cuda:0",
            "iterk_solver_options": {}, "xhat_xbar_options": {"xhat_solver_options": {}},
            "xhat_closest_options": {"xhat_solver_options": {}}}
    opts.update(extra)
    return Xhat_Eval(opts, farmer.scenario_names_creator(S), farmer.scenario_creator, mpicomm=mpicomm,
                     scenario_creator_kwargs={"num_scens": S})


def _close(a, b):
    return a is not None and b is not None and abs(a - b) <= OBJ_REL * abs(b)


def _spoke_pass(sp, wid, v):
    """One delivery of the hub's nonants and one pass of the spoke's loop body; the bound it
    wrote, or None."""
    sp.best_inner_bound = float("inf")
    before = sp.local_write_id
    sp._deliver(wid, v)
    assert not sp.got_kill_signal() and sp.new_nonants
    sp.do_work()
    return sp.bound if sp.local_write_id > before else None


def test_classes_on_farmer30_from_the_hubs_nonants(gpu):
    from mpisppy_amd.cylinders.slam_heuristic import SlamMaxHeuristic, SlamMinHeuristic
    from mpisppy_amd.cylinders.xhatxbar_bounder import XhatXbarInnerBound
    from mpisppy_amd.extensions.xhatclosest import XhatClosest
    from mpisppy_amd.extensions.xhatxbar import XhatXbar
    traj = R.farmer_trajectory()
    xe = _farmer_xhat_eval()
    xe._lazy_create_solvers()
    e = xe.engine
    xbar, closest = XhatXbar(xe), XhatClosest(xe)
    closest.pre_iter0()
    spokes = {c: c(_farmer_xhat_eval()) for c in (SlamMinHeuristic, SlamMaxHeuristic, XhatXbarInnerBound)}
    for sp in spokes.values():
        sp.main()
    for wid, it in enumerate(R.FARMER_ITERS, start=1):
        r = traj[it]
        v = _dev(e, r["v"])
        obj = xbar.xhat_tryit(nonant_cache=v)
        cobj, cname = closest.xhat_closest_to_xbar(nonant_cache=v)
        smin = _spoke_pass(spokes[SlamMinHeuristic], wid, v)
        smax = _spoke_pass(spokes[SlamMaxHeuristic], wid, v)
        sxb = _spoke_pass(spokes[XhatXbarInnerBound], wid, v)
        print(f"iter {it}: xbar {obj} / {r['xbar_obj']}; slam-min {smin} / {r['slammin_obj']}; slam-max {smax}; "
              f"closest {cname} {cobj} / scen{r['winner']} {r['closest_obj']}")
        assert _close(obj, r["xbar_obj"]) and _close(sxb, r["xbar_obj"])
        np.testing.assert_allclose(xbar.last_table.cpu().numpy()[0], r["planes"][0], rtol=1e-13)
        assert not xe._fixed                                       # restore_nonants=True put the bounds back
        assert _close(smin, r["slammin_obj"])
        assert smax is None
        assert cname == {"ROOT": f"scen{r['winner']}"} and _close(cobj, r["closest_obj"])
    sp = spokes[XhatXbarInnerBound]
    np.testing.assert_allclose(sp.best_xhat["ROOT"], traj[R.FARMER_ITERS[-1]]["planes"][0], rtol=1e-13)
    assert spokes[SlamMaxHeuristic].best_xhat is None
    for o in [xe] + [s.opt for s in spokes.values()]:
        o.engine.close()


def test_xhatxbar_on_aircond432_uses_per_node_xbar(gpu):
    from oracle.models import aircond_scenario, create_nodenames_from_branching_factors
    from oracle.wheel import xhat_objective
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.extensions.xhatxbar import XhatXbar
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    bf = [4, 3, 2]
    names = aircond.scenario_names_creator(24)
    opts = {"solver_name": "mi355x_pdhg", "verbose": False, "toc": False, "device": "cuda:0",
            "xhat_xbar_options": {"xhat_solver_options": {}}}
    xe = Xhat_Eval(opts, names, aircond.scenario_creator, all_nodenames=create_nodenames_from_branching_factors(bf),
                   scenario_creator_kwargs=dict(AIR_KW, branching_factors=bf))
    xe._lazy_create_solvers()
    xe.solve_loop(warm_start=False)                                # the Iter0 LPs' nonants as the hub's
    e = xe.engine
    cache = e.nonant_x_dev().clone()
    key, pc = _key_pcoef(e)
    ref, _ = R.planes(cache.cpu().numpy(), key, pc, e.num_nodes * e.nlen_max)
    x = XhatXbar(xe)
    obj = x.xhat_tryit(nonant_cache=cache)
    tab = x.last_table.cpu().numpy()
    np.testing.assert_allclose(tab.reshape(-1), ref[0], rtol=1e-12, atol=1e-12)
    assert len({tuple(row) for row in tab}) > 4                    # the nodes' x̄ do differ
    scens = [aircond_scenario(n, bf, **AIR_KW) for n in names]
    oobj = xhat_objective(scens, {nd: tab[g] for g, nd in enumerate(e.node_names)})
    print("aircond 4-3-2 xbar objective", obj, "oracle", oobj)
    assert _close(obj, oobj)
    e.close()


# ------------------------------------------------------------------ the wheel
def _cfg(**kw):
    from types import SimpleNamespace
    d = dict(solver_name="mi355x_pdhg", default_rho=1.0, max_iterations=200, rel_gap=1e-4,
             intra_hub_conv_thresh=1e-10, device="cuda:0", toc=False)
    d.update(kw)
    return SimpleNamespace(**d)


def _wheel(cfg, which):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.spin_the_wheel import WheelSpinner
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    names = farmer.scenario_names_creator(3)
    kw = {"num_scens": 3}
    hub = vanilla.ph_hub(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
    spokes = [getattr(vanilla, w + "_spoke")(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
              for w in which]
    return WheelSpinner(hub, spokes)


def test_wheel_with_the_new_spokes(gpu):
    base = _wheel(_cfg(), ["lagrangian", "xhatshuffle"])
    base.spin()
    ws = _wheel(_cfg(), ["lagrangian", "xhatshuffle", "xhatxbar", "slammin"])
    ws.spin()
    it, it0 = ws.spcomm.opt._PHIter, base.spcomm.opt._PHIter
    print(f"with the new spokes: {it} PH iterations, inner {ws.BestInnerBound}, outer {ws.BestOuterBound}; "
          f"without: {it0}, inner {base.BestInnerBound}; x̄ spoke {ws.spokes[2].bound}, slam-min {ws.spokes[3].bound}")
    assert 1 <= it < 200                                           # terminated on the gap
    assert ws.spcomm.innerbound_spoke_chars[3] == "B" and ws.spcomm.innerbound_spoke_chars[4] == "S"
    assert ws.BestOuterBound <= ws.BestInnerBound + OBJ_REL * abs(ws.BestInnerBound)
    assert ws.BestInnerBound <= base.BestInnerBound + OBJ_REL * abs(base.BestInnerBound)
    assert abs(ws.BestInnerBound - FARMER_EF_OBJ) <= 1e-4 * abs(FARMER_EF_OBJ)
    for sp in ws.spokes[2:]:                                       # both offered valid inner bounds
        assert np.isfinite(sp.bound) and sp.bound >= FARMER_EF_OBJ - OBJ_REL * abs(FARMER_EF_OBJ)
        assert sp.best_xhat is not None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    import sys
    root = os.path.dirname(HERE)
    for p in (HERE, os.path.join(root, "mpi-sppy-1_amd"), root):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _wheel_worker(rank, world, port, out_dir):
    dist = _init(rank, world, port)
    try:
        ws = _wheel(_cfg(max_iterations=20000, intra_hub_conv_thresh=-1.0), ["lagrangian", "xhatshuffle", "xhatxbar"])
        ws.spin()
        sp = ws.spokes[0] if ws.strata_rank > 0 else None
        res = {"inner": ws.BestInnerBound, "outer": ws.BestOuterBound, "cyl": ws.strata_rank,
               "placement": ws.placement, "cls": type(sp).__name__ if sp else "hub",
               "bound": float(getattr(sp, "bound", float("nan"))) if sp else None,
               "remote": bool(sp._remote) if sp else None,
               "served": int(sp.remote_write_id) if sp else None}
        with open(os.path.join(out_dir, f"w{rank}.json"), "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_xhatxbar_spoke_on_its_own_rank(gpu, tmp_path):
    """Hub, Lagrangian, xhatshuffle and xhatxbar on one rank each (gloo, one GPU): the x̄ spoke
    runs through Spoke.run_remote and its bound is a valid inner bound."""
    import torch.multiprocessing as mp
    mp.spawn(_wheel_worker, args=(4, _free_port(), str(tmp_path)), nprocs=4, join=True)
    r = [json.load(open(tmp_path / f"w{k}.json")) for k in range(4)]
    assert [x["placement"] for x in r] == ["ranks"] * 4 and [x["cyl"] for x in r] == [0, 1, 2, 3]
    assert r[3]["cls"] == "XhatXbarInnerBound" and r[3]["remote"] and r[3]["served"] >= 1
    ib, ob = r[0]["inner"], r[0]["outer"]
    print("x̄ spoke on its own rank: bound", r[3]["bound"], "after", r[3]["served"], "deliveries; wheel", ib, ob)
    assert all(x["inner"] == ib and x["outer"] == ob for x in r)
    assert np.isfinite(r[3]["bound"]) and r[3]["bound"] >= FARMER_EF_OBJ - OBJ_REL * abs(FARMER_EF_OBJ)
    assert ib <= r[3]["bound"] + 1e-9 * abs(ib)                   # the hub counted it
    assert ob <= ib + OBJ_REL * abs(ib) and abs(ib - FARMER_EF_OBJ) <= 1e-4 * abs(FARMER_EF_OBJ)


# ------------------------------------------------------------------ the post_everything form
def _farmer_ph(ext, iters=5, **extra):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.ph import PH
    S = R.FARMER_S
    opts = {"solver_name": "mi355x_pdhg", "PHIterLimit": iters, "defaultPHrho": 1.0, "convthresh": -1.0,
            "verbose": False, "display_progress": False, "toc": False, "device": "cuda:0",
            "xhat_xbar_options": {"xhat_solver_options": {}, "keep_solution": False},
            "xhat_closest_options": {"xhat_solver_options": {}, "keep_solution": False}}
    opts.update(extra)
    return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator, extensions=ext,
              scenario_creator_kwargs={"num_scens": S})


@pytest.mark.parametrize("which", ["xbar", "closest"])
def test_post_everything_on_a_ph_object(gpu, which):
    """XhatXbar / XhatClosest as PH extensions: post_everything gives the restatement's
    objective, and afterwards W and prox are on again and the nonants free, so the next
    solve is the untouched run's (objective 1e-5 relative; x within 1e-5 of its scale, the
    solves' own accuracy: they start from different warm starts)."""
    from mpisppy_amd.extensions.xhatclosest import XhatClosest
    from mpisppy_amd.extensions.xhatxbar import XhatXbar
    traj = R.farmer_trajectory()
    ph = _farmer_ph(XhatXbar if which == "xbar" else XhatClosest)
    _, eobj, _ = ph.ph_main()
    ext = ph.extobject
    if which == "xbar":
        want = traj[5]["xbar_obj"]
        got = ext._xhat_xbar_obj_final
    else:
        want = traj["post"]["closest_obj"]
        got = ext._final_xhat_closest_obj
        assert ext._final_xhat_closest_name == f"scen{traj['post']['winner']}"
    print(which, "post_everything objective", got, "restatement", want)
    assert _close(got, want) and _close(eobj, want)               # post_loops' Eobjective is the xhat solve's
    e = ph.engine
    assert e.W_on == 1 and e.prox_on == 1 and e.xfix is None and not ph._fixed
    ph.solve_loop(solver_options=ph.current_solver_options)
    plain = _farmer_ph(None)
    plain.ph_main()
    plain.solve_loop(solver_options=plain.current_solver_options)
    a, b = ph.nonants_array(), plain.nonants_array()
    assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), np.abs(a - b).max()
    assert _close(ph.Eobjective(), plain.Eobjective())
    assert np.array_equal(ph.W_array(), plain.W_array())          # the extension touched neither W nor x̄
    e.close()
    plain.engine.close()


# ------------------------------------------------------------------ two ranks
def _ranks_worker(rank, world, port, out_dir):
    dist = _init(rank, world, port)
    try:
        from mpisppy_amd.comm import Comm
        from mpisppy_amd.cylinders.slam_heuristic import SlamMinHeuristic
        from mpisppy_amd.extensions.xhatxbar import XhatXbar

        class Solo(Comm):                      # a one-rank communicator inside the two-rank world
            def __init__(self):
                self.group, self.rank, self.size = None, 0, 1

        it = 5
        r = R.farmer_trajectory()[it]
        S = R.FARMER_S
        res = {}

        def run(xe, v):
            xe._lazy_create_solvers()
            e = xe.engine
            vd = _dev(e, v)
            out = {"planes": e.nonant_stats(vd).cpu().numpy().reshape(4, -1).tolist(),
                   "xbar": XhatXbar(xe).xhat_tryit(nonant_cache=vd)}
            sp = SlamMinHeuristic(xe)
            sp.main()
            out["slammin"] = _spoke_pass(sp, 1, vd)
            out["calls"] = dict(e.calls)
            return out, e

        xe = _farmer_xhat_eval(mpicomm=Comm())
        lo, hi = (0, S // 2) if rank == 0 else (S // 2, S)
        assert xe.local_scenario_names == [f"scen{i}" for i in range(lo, hi)]
        res["two"], e = run(xe, r["v"][:, lo:hi])
        # the closest scenario: the plain case, then identical winners on both ranks
        pl = r["planes"]
        res["closest"] = list(e.closest_scenario(_dev(e, r["v"][:, lo:hi]), _dev(e, pl[0]), _dev(e, pl[1])))
        v = r["v"][:, lo:hi].copy()
        v[:, 2 + 2 * rank] = r["v"][:, 7]      # scenario 7's values at local index 2 (rank 0) and 4 (rank 1)
        xb = r["v"][:, 7] * (1.0 + 1e-3)
        res["tie"] = list(e.closest_scenario(_dev(e, v), _dev(e, xb), _dev(e, xb * xb + (0.1 * xb) ** 2)))
        res["tie_local"] = float(e.closest_dist.cpu().numpy()[2 + 2 * rank])
        res["calls"] = dict(e.calls)
        e.close()
        if rank == 0:
            res["one"], e1 = run(_farmer_xhat_eval(mpicomm=Solo()), r["v"])
            e1.close()
        with open(os.path.join(out_dir, f"x{rank}.json"), "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_match_one(gpu, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_ranks_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"x{k}.json")) for k in range(2)]
    ref = R.farmer_trajectory()[5]
    one = r[0]["one"]
    _assert_planes(one["planes"], ref["planes"], ref["mag"])
    for k in range(2):
        two = r[k]["two"]
        _assert_planes(two["planes"], ref["planes"], ref["mag"])  # the reduced planes on every rank
        got, want = np.array(two["planes"]), np.array(one["planes"])
        assert np.array_equal(got[2:], want[2:])
        assert (np.abs(got[:2] - want[:2]) <= 2 * SUM_REL * ref["mag"]).all()
        assert _close(two["xbar"], one["xbar"]) and _close(two["slammin"], one["slammin"])
        assert _close(two["xbar"], ref["xbar_obj"]) and _close(two["slammin"], ref["slammin_obj"])
        c = r[k]["calls"]
        assert c["nonant_stats"] == c["allreduce_stats_sum"] == c["allreduce_stats_max"] == 3, c
        # the plain case: the restatement's winner, as (rank, local index)
        w = ref["winner"]
        assert r[k]["closest"][1:] == [w // 15, w % 15] and abs(r[k]["closest"][0] - ref["dmin"]) <= 1e-9 * ref["dmin"]
        # identical winning scenarios on both ranks: the highest rank, its local index
        assert r[k]["tie"][1:] == [1, 4], r[k]["tie"]
    assert r[0]["tie_local"] == r[1]["tie_local"] == r[0]["tie"][0] == r[1]["tie"][0]
    assert one["calls"]["allreduce_stats_sum"] == 0
