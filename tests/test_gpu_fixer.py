"""The Fixer on the device (phgpu_fixer_step, include/phgpu.h; mpisppy_amd/extensions/fixer.py)
against the numpy restatement of mpisppy/extensions/fixer.py in tests/fixer_ref.py.

* the kernel alone on constructed states whose every comparison is exact in fp64 (dyadic x̄,
  th and boundtol powers of two, E[x²] = x̄² - d with d a multiple of th² / 2): counters,
  nfix, totals and the NaN pattern equal, fixed values bit-equal;
* PH with the Fixer against the stepped oracle on the three trajectories whose decisions keep
  10 % clear of the threshold (tests/test_fixer.py asserts that on the CPU): the fixing
  iterations and nfix exactly; fixval, x̄ and W at 1e-5 absolute, the trivial bound at 1e-5
  relative (the tolerances of tests/test_gpu_norm_rho.py);
* fix_nonants with a Fixer state, two gloo ranks on one GPU, and model bounds that differ
  between the scenarios of a node (the "Variation in fixing" error).
"""
import json
import os
import socket

import numpy as np
import pytest
import torch

import fixer_ref as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OBJ_REL = 1e-5
ABS = 1e-5
NAN = float("nan")


# ------------------------------------------------------------------ the kernel alone
def _engine(model, S, bf=None):
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.examples import aircond, farmer
    if model == "farmer":
        b = farmer.batch_creator(farmer.scenario_names_creator(S), crops_multiplier=1, num_scens=S)
    else:
        b = aircond.batch_creator(aircond.scenario_names_creator(S), branching_factors=bf, **F.AIR_KW)
    return PHEngine(b, device="cuda:0", shared=True if model == "aircond_shared" else None)


def _keys(e):
    """[nn, S] index of (node, offset) of every local (nonant, scenario) in node_buf."""
    b = e.batch
    node_of = e.node_of.cpu().numpy().reshape(-1, e.S)
    return np.stack([node_of[int(b.nonant_depth[k])] * e.nlen_max + int(b.nonant_off[k]) for k in range(e.nn)])


BT = 0.125          # boundtol: a power of two


def _constructed_state(e, rng):
    """x̄ / E[x²] per node entry, thresholds and lags per nonant, counters and earlier fixings
    per entry: every comparison of the rule is exact with or without a fused multiply-add."""
    key = _keys(e)
    half = e.num_nodes * e.nlen_max
    cols = np.asarray(e.batch.nonant_col)
    l = e.lb.cpu().numpy()[cols]
    u = e.ub.cpu().numpy()[cols]
    th = np.array([2.0 ** ((k % 3) - 1) for k in range(e.nn)])
    if e.nn > 3:
        th[-1] = 0.0                                 # a nonant without a tuple
    xb, xsq = np.zeros(half), np.zeros(half)
    place = [lambda lo, hi: lo + 0.5 * BT, lambda lo, hi: lo + BT, lambda lo, hi: lo + 2 * BT,
             lambda lo, hi: hi - 0.5 * BT, lambda lo, hi: hi - BT, lambda lo, hi: hi - 2 * BT,
             lambda lo, hi: lo + 64.0, lambda lo, hi: hi + 1.0, lambda lo, hi: lo - 1.0]
    dmul = [0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0]
    seen = set()
    for k in range(e.nn):
        for s in range(e.S):
            o = int(key[k, s])
            if o in seen:
                continue
            seen.add(o)
            i = len(seen)
            xb[o] = place[i % len(place)](l[k, s], u[k, s])
            d = dmul[(i // 2) % len(dmul)] * th[k] * th[k]
            xsq[o] = xb[o] * xb[o] - d
            assert xsq[o] + d == xb[o] * xb[o]        # nothing was rounded away
    lags = rng.integers(-1, 4, (3, e.nn)).astype(np.int32)
    count = rng.integers(0, 5, (e.nn, e.S)).astype(np.int32)
    pre = np.where(rng.random((e.nn, e.S)) < 0.1, 3.0, NAN)
    return key, l, u, th, lags, xb, xsq, count, pre


@pytest.mark.parametrize("iter0", [1, 0])
@pytest.mark.parametrize("model,S,bf", [("farmer", 130, None),            # three waves, the last ragged
                                        ("aircond", 24, [4, 3, 2]),       # waves span nodes
                                        ("aircond_shared", 24, [4, 3, 2])])
def test_kernel_against_the_restatement(gpu, model, S, bf, iter0):
    from mpisppy_amd import _lib
    e = _engine(model, S, bf)
    assert e.shared == (model == "aircond_shared")
    rng = np.random.default_rng(7)
    key, l, u, th, lags, xb, xsq, count, pre = _constructed_state(e, rng)
    half = e.num_nodes * e.nlen_max
    e._fixer_bufs()
    assert e.fixer_nloc.cpu().numpy().tolist() == np.bincount(key.ravel(), minlength=half).tolist()
    e.fixer_count[:e.nn].copy_(torch.as_tensor(count, device=e.device))
    e.fixer_fixval[:e.nn].copy_(torch.as_tensor(pre, device=e.device))
    e.fix_nonants(None)                              # the earlier fixings' bounds (fixer_fixval)
    e.node_buf.copy_(torch.as_tensor(np.concatenate([xb, xsq]), device=e.device))
    args = (e.fixer_arg(th, torch.float64),) + tuple(e.fixer_arg(torch.as_tensor(a), torch.int32) for a in lags)
    prm = _lib.FixerParams(boundtol=BT, iter0=iter0)
    ws0 = e.workspace_bytes()
    rc, rf = count.astype(np.int64), pre.copy()
    totals = np.zeros(3, dtype=np.int64)
    nloc = np.bincount(key.ravel(), minlength=half)
    fixed_any = 0
    for call in range(2):
        e.fixer_nfix.fill_(12345)                    # stale data must not survive
        e.fixer_step(prm, *args)
        rc, rf, new, arrived = F.rule(bool(iter0), xb[key], xsq[key], th[:, None], lags[0][:, None],
                                      lags[1][:, None], lags[2][:, None], l, u, BT, rc, rf)
        nfix = np.bincount(key[new], minlength=half)
        totals += [int(new.sum()), int(arrived.sum()), int(((nfix > 0) & (nfix < nloc)).sum())]
        fixed_any += int(new.sum())
        assert np.array_equal(e.fixer_count.cpu().numpy()[:e.nn], rc), call
        assert e.fixer_nfix.cpu().numpy().tolist() == nfix.tolist(), call
        got = e.fixer_fixval.cpu().numpy()[:e.nn]
        assert np.array_equal(np.isnan(got), np.isnan(rf)), call
        assert np.array_equal(got.view(np.int64)[~np.isnan(rf)], rf.view(np.int64)[~np.isnan(rf)]), call
        assert list(e.fixer_totals_host()) == totals.tolist(), call
    assert fixed_any > 0 and totals[2] > 0 and (totals[1] > 0) == bool(iter0)
    assert e.calls["fixer_step"] == 2 and not any(v for k, v in e.calls.items() if k.startswith("allreduce"))
    # its workspace (two int32 per node entry) came with the first call
    assert e.workspace_bytes() == ws0 + 2 * 4 * half
    e.close()


@pytest.mark.parametrize("model", ["aircond", "aircond_shared"])
def test_the_next_solve_sees_the_fixings(gpu, model):
    """Every nonant fixed at its node's x̄ by one iter0 call (nb lag 0), on a per-scenario and on
    a shared-matrix handle (whose working bounds live in its column records): the next solve
    returns the nonants at those values.  (Aircond with small productions is feasible for any
    demand: the inventory is free.)"""
    from mpisppy_amd import _lib
    e = _engine(model, 24, [4, 3, 2])
    key = _keys(e)
    half = e.num_nodes * e.nlen_max
    xb = 32.0 + 8.0 * (np.arange(half) % 5)
    e.node_buf.copy_(torch.as_tensor(np.concatenate([xb, xb * xb]), device=e.device))
    none = torch.full((e.nn,), -1, dtype=torch.int32)
    e.fixer_step(_lib.FixerParams(boundtol=BT, iter0=1), e.fixer_arg(np.ones(e.nn), torch.float64),
                 e.fixer_arg(torch.zeros(e.nn, dtype=torch.int32), torch.int32), e.fixer_arg(none, torch.int32),
                 e.fixer_arg(none, torch.int32))
    assert list(e.fixer_totals_host()) == [e.nn * e.S, 0, 0]
    assert np.array_equal(e.fixer_fixval.cpu().numpy()[:e.nn], xb[key])
    e.solve(_lib.default_options(), warm=False)
    assert (e.host("status") == _lib.OPTIMAL).all()
    x = e.nonant_x_dev().cpu().numpy()
    assert np.abs(x - xb[key]).max() <= 1e-9 * 64.0
    e.close()


# ------------------------------------------------------------------ PH against the stepped oracle
def _recording_fixer():
    from mpisppy_amd.extensions.fixer import Fixer

    class RecordingFixer(Fixer):
        """The Fixer, keeping a device copy of nfix after every miditer (no read back)."""

        def miditer(self):
            super().miditer()
            e = self.ph.engine
            self.trace = getattr(self, "trace", []) + [(self.ph._PHIter, e.fixer_nfix.clone(),
                                                        e.calls["fixer_totals_host"])]
    return RecordingFixer


def _ph(case, iters=None, spec=True, mpicomm=None, ext=None, **extra):
    from mpisppy_amd.extensions.fixer import uniform_fix_list_fct
    from mpisppy_amd.opt.ph import PH
    c = F.CASES[case]
    opts = {"solver_name": "mi355x_pdhg", "PHIterLimit": iters or c["iters"], "defaultPHrho": 1.0, "convthresh": -1.0,
            "verbose": False, "display_progress": False, "toc": False, "device": "cuda:0",
            "speculative_solve": spec, "fused_ph_loop": False,
            "fixeroptions": {"verbose": False, "boundtol": F.BOUNDTOL}}
    opts.update(extra)
    ext = ext or _recording_fixer()
    S = c["S"]
    if case == "farmer3":
        # per-scenario models: the tuples come from id_fix_list_fct, keyed by id(var)
        from mpisppy_amd.examples import farmer
        opts["fixeroptions"]["id_fix_list_fct"] = uniform_fix_list_fct(c["th"], nb=c["nb"])
        return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator, extensions=ext, mpicomm=mpicomm,
                  scenario_creator_kwargs={"crops_multiplier": 1, "num_scens": S})
    nn = 3 if case.startswith("farmer") else 2 * len(c["bf"])
    i0, ik = F.tuples(case, nn)
    opts["fixeroptions"]["fix_arrays"] = {"iter0": dict(zip(("th", "nb", "lb", "ub"), i0)),
                                         "iterk": dict(zip(("th", "nb", "lb", "ub"), ik))}
    if case.startswith("farmer"):
        from mpisppy_amd.examples import farmer
        opts["batch_creator"] = farmer.batch_creator
        return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator, extensions=ext, mpicomm=mpicomm,
                  scenario_creator_kwargs={"crops_multiplier": 1, "num_scens": S})
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    opts["batch_creator"] = aircond.batch_creator
    return PH(opts, aircond.scenario_names_creator(S), aircond.scenario_creator, extensions=ext, mpicomm=mpicomm,
              scenario_creator_kwargs=dict(F.AIR_KW, branching_factors=c["bf"]),
              all_nodenames=create_nodenames_from_branching_factors(c["bf"]))


def _fixing(ph):
    """{PH iteration: entries newly fixed} and the per-iteration nfix of a finished run."""
    tr = ph.extobject.trace
    nfix = {it: nf.cpu().numpy() for it, nf, _ in tr}
    return {it: int(nf.sum()) for it, nf in nfix.items() if nf.sum()}, nfix


def _node_perm(ph, o):
    """node_buf index of every oracle key (the engine numbers the nodes in its own order)."""
    e = ph.engine
    g = {nd: i for i, nd in enumerate(e.node_names)}
    return np.array([g[o.node_names[k // o.nlen_max]] * e.nlen_max + k % o.nlen_max for k in range(o.nkeys)])


@pytest.mark.parametrize("spec", [True, False])
@pytest.mark.parametrize("case", list(F.CASES))
def test_ph_with_fixer_matches_the_stepped_oracle(gpu, case, spec):
    o = F.trajectory(case)
    ph = _ph(case, spec=spec)
    conv, _, tb = ph.ph_main(finalize=False)
    e = ph.engine
    fx = ph.extobject
    assert fx.miditer_on_device and ph._speculate(True) == spec and ph._miditer_early(True)
    assert e.calls["solve_deferred"] == (F.CASES[case]["iters"] if spec else 0) and e.calls["ph_loop"] == 0
    assert e.calls["fixer_step"] == F.CASES[case]["iters"]
    # nothing was read back while the loop ran
    assert e.calls["fixer_totals_host"] == 0 and all(n == 0 for _, _, n in fx.trace)
    got, nfix = _fixing(ph)
    assert got == F.CASES[case]["fixed"], got
    perm = _node_perm(ph, o)
    for r in o.log:
        assert nfix[r["iter"]][perm].tolist() == r["nfix"].tolist(), r["iter"]
    fv = e.fixer_fixval.cpu().numpy()[:e.nn].T
    x = ph.nonants_array()
    W = ph.W_array()
    xbar = e.host("xbar")[:, :e.nn]
    h = o.hist[-1]
    fixed = ~np.isnan(o.fixval)
    print(case, "spec", spec, "max |fixval - oracle|", np.abs(fv[fixed] - o.fixval[fixed]).max(), "max |W - oracle|",
          np.abs(W - h["W"]).max(), "max |xbar - oracle|", np.abs(xbar - h["xbar"]).max(), "conv", conv,
          "max |x - fixval|", np.abs(x[fixed] - fv[fixed]).max(), "tb rel", abs(tb - o.trivial) / abs(o.trivial))
    assert np.array_equal(np.isnan(fv), np.isnan(o.fixval))
    assert np.abs(fv[fixed] - o.fixval[fixed]).max() <= ABS
    assert np.abs(xbar - h["xbar"]).max() <= ABS
    assert np.abs(W - h["W"]).max() <= ABS
    assert abs(tb - o.trivial) <= OBJ_REL * abs(o.trivial)
    assert np.abs(x[fixed] - fv[fixed]).max() <= 1e-9 and conv < 1e-9
    ph.post_loops(ph.extensions)                      # post_everything: the one read back
    assert e.calls["fixer_totals_host"] == 1
    S = F.CASES[case]["S"]
    assert fx.fixed_so_far == sum(got.values()) / S and fx.fixed_prior_iter0 == 0
    e.close()


def test_progress_line_reads_the_totals_and_leaves_the_loop_plain(gpu, capsys):
    """display_progress: the reference's line after every miditer, from fixer_totals_host; the
    speculative solve is then off, and the fixing is the same."""
    ph = _ph("farmer3", display_progress=True)
    ph.ph_main(finalize=False)
    assert not ph.extobject.miditer_on_device and not ph._speculate(True) and ph.engine.calls["solve_deferred"] == 0
    assert _fixing(ph)[0] == F.CASES["farmer3"]["fixed"]
    out = capsys.readouterr().out
    assert out.count("(rank0) Unique vars fixed so far - ") == 12
    assert "(rank0) Unique vars fixed so far - 1 (0 prior to iteration 0)" in out
    assert "(rank0) Unique vars fixed so far - 3 (0 prior to iteration 0)" in out
    ph.engine.close()


# ------------------------------------------------------------------ fix_nonants with a Fixer state
def test_fix_nonants_keeps_what_the_fixer_fixed(gpu):
    """farmer 70 once its first nonant is fixed (PH iteration 6): fix_nonants(xhat) fixes
    everything at xhat, fix_nonants(None) gives the fixed nonant back its Fixer value and
    frees the others, and NaN rows of an xfix keep the Fixer's value."""
    ph = _ph("farmer70", iters=6)
    ph.ph_main(finalize=False)
    e = ph.engine
    fv = e.fixer_fixval.cpu().numpy()[:e.nn]
    held = ~np.isnan(fv)
    assert held.all(axis=1).sum() == 1 and held.sum() == 70           # one whole nonant row
    k = int(np.flatnonzero(held.all(axis=1))[0])
    free = [j for j in range(e.nn) if j != k]
    opts = ph._to_phgpu_options(ph.current_solver_options)
    # the third of the acreage to every crop: feasible for every scenario
    xhat = torch.full((e.nn, e.S), 500.0 / 3.0, dtype=torch.float64, device=e.device)
    e.fix_nonants(xhat)
    e.solve(opts)
    assert np.abs(e.nonant_x_dev().cpu().numpy() - 500.0 / 3.0).max() <= 1e-9 * 500.0
    e.fix_nonants(None)
    e.solve(opts)
    x = e.nonant_x_dev().cpu().numpy()
    assert np.abs(x[k] - fv[k]).max() <= 1e-9 * 500.0
    assert all(np.ptp(x[j]) > 1e-3 for j in free), [np.ptp(x[j]) for j in free]     # free again
    part = torch.full((e.nn, e.S), NAN, dtype=torch.float64, device=e.device)
    part[free[0]] = 100.0
    e.fix_nonants(part)
    e.solve(opts)
    x = e.nonant_x_dev().cpu().numpy()
    assert np.abs(x[k] - fv[k]).max() <= 1e-9 * 500.0 and np.abs(x[free[0]] - 100.0).max() <= 1e-9 * 500.0
    # (the acreage row binds, so the third crop is the same everywhere here: whether a row is
    # free shows with an xfix of NaN only, which must act as fix_nonants(None))
    e.fix_nonants(torch.full((e.nn, e.S), NAN, dtype=torch.float64, device=e.device))
    e.solve(opts)
    x = e.nonant_x_dev().cpu().numpy()
    assert np.abs(x[k] - fv[k]).max() <= 1e-9 * 500.0
    assert all(np.ptp(x[j]) > 1e-3 for j in free), [np.ptp(x[j]) for j in free]
    e.fix_nonants(None)
    assert e.xfix is None
    e.close()


# ------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _device_noop():
    from mpisppy_amd.extensions.extension import Extension

    class DeviceNoop(Extension):
        """A miditer that does nothing, in the Fixer's place in the loop."""
        miditer_on_device = True

        def miditer(self):
            pass
    return DeviceNoop


def _run_farmer70(mpicomm=None, noop=False):
    ph = _ph("farmer70", mpicomm=mpicomm, ext=_device_noop() if noop else None)
    ph.ph_main(finalize=False)
    e = ph.engine
    res = {"calls": dict(e.calls), "names": list(ph.local_scenario_names), "spec": bool(ph._speculate(True))}
    if not noop:
        res["fixing"] = {str(k): v for k, v in _fixing(ph)[0].items()}
        res["fixval"] = np.nan_to_num(e.fixer_fixval.cpu().numpy()[:e.nn].T, nan=-1.0).tolist()
        ph.post_loops(ph.extensions)
        res["fixed_so_far"] = ph.extobject.fixed_so_far
    e.close()
    return res


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
        res = {"fixer": _run_farmer70(Comm()), "noop": _run_farmer70(Comm(), noop=True)}
        with open(os.path.join(out_dir, f"fx_r{rank}.json"), "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_fix_what_one_rank_fixes(gpu, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"fx_r{k}.json")) for k in range(2)]
    one = _run_farmer70()
    assert r[0]["fixer"]["names"] + r[1]["fixer"]["names"] == one["names"] and len(r[0]["fixer"]["names"]) == 35
    # the same PH iterations, each rank fixing its 35 scenarios of the nonant
    assert one["fixing"] == {str(k): v for k, v in F.CASES["farmer70"]["fixed"].items()}
    fv = np.array(one["fixval"])
    lo = 0
    for k in range(2):
        f, n = r[k]["fixer"], r[k]["noop"]
        assert f["fixing"] == {it: v // 2 for it, v in one["fixing"].items()}, f["fixing"]
        assert np.abs(np.array(f["fixval"]) - fv[lo:lo + 35]).max() <= ABS
        assert f["fixed_so_far"] == 3.0 and f["spec"]
        # no collective is the Fixer's: the run issues the all-reduces of a loop whose miditer does nothing
        ar = {key: v for key, v in f["calls"].items() if key.startswith("allreduce")}
        assert ar == {key: v for key, v in n["calls"].items() if key.startswith("allreduce")}, ar
        assert f["calls"]["fixer_step"] == F.CASES["farmer70"]["iters"] and n["calls"]["fixer_step"] == 0
        lo += 35


# ------------------------------------------------------------------ model bounds that differ
def test_partial_fixing_of_a_node_ends_in_the_variation_error(gpu):
    """One scenario's model upper bound differs: with x̄ on the others' bound, an ub-lag fix
    takes two of the three scenarios of the ROOT entry, and post_everything raises."""
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.extensions.fixer import Fixer
    from mpisppy_amd.opt.ph import PH

    def creator(names, **kw):
        b = farmer.batch_creator(names, **kw)
        b.ub = np.array(b.ub, dtype=np.float64, copy=True)
        b.ub[1, b.nonant_col[0]] = 600.0
        return b

    none = [None] * 3
    opts = {"solver_name": "mi355x_pdhg", "PHIterLimit": 1, "defaultPHrho": 1.0, "convthresh": -1.0,
            "verbose": False, "display_progress": False, "toc": False, "device": "cuda:0", "batch_creator": creator,
            "fixeroptions": {"verbose": False, "boundtol": 0.125,
                             "fix_arrays": {"iter0": None, "iterk": {"th": [1.0] * 3, "nb": none, "lb": none,
                                                                     "ub": [0, None, None]}}}}
    ph = PH(opts, farmer.scenario_names_creator(3), farmer.scenario_creator, extensions=Fixer,
            scenario_creator_kwargs={"crops_multiplier": 1, "num_scens": 3})
    ph.PH_Prep()
    ph.Iter0()
    e = ph.engine
    half = e.num_nodes * e.nlen_max
    xb = np.array([500.0 - 0.0625, 100.0, 100.0])
    e.node_buf.copy_(torch.as_tensor(np.concatenate([xb, xb * xb])[:2 * half], device=e.device))
    ph._PHIter = 2
    ph.extobject.miditer()
    fv = e.fixer_fixval.cpu().numpy()[:e.nn]
    assert fv[0].tolist()[0] == 500.0 and np.isnan(fv[0, 1]) and fv[0, 2] == 500.0 and np.isnan(fv[1:]).all()
    assert e.fixer_nfix.cpu().numpy().tolist() == [2, 0, 0]
    with pytest.raises(RuntimeError, match="Variation in fixing across scenarios detected"):
        ph.post_loops(ph.extensions)
    assert list(e.fixer_totals_host()) == [2, 0, 1]
    e.close()
