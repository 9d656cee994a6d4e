"""Confidence intervals on the device (mpisppy_amd.confidence_intervals, csrc/ph_gap.inc): the
moments pass against math.fsum, and the estimators, MMW, zhat4xhat and sequential sampling on
farmer against the recorded numpy / HiGHS restatement (tests/ci_ref.py,
tests/golden/mmw_farmer.json)."""
import ctypes
import json
import math
import os
import socket
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "mmw_farmer.json")))
SOLVER = "mi355x_pdhg"
XHAT = {"ROOT": np.array(GOLDEN["xhat"])}
START = GOLDEN["start"]
SUM_REL = 1e-12     # each sum against fsum(|terms|): the bound the cut pass and the nonant planes meet
G_ABS = 2e-5        # G against the fixture, times |zhat|: two expectations held to 1e-5 relative each
Z_REL = 1e-5        # the project's standing relative tolerance on an expectation
# s, std and gap_inner_bound depend on how close the L-shaped x* is to HiGHS's.  Measured on the
# MI355X (printed by the tests): at most 1.053e-7 relative (s of the third 16-scenario
# batch); asserted: ten times that
S_REL = 1.1e-6
ZMIN = min(abs(z) for c in GOLDEN["cases"].values() for z in c["zhat"])     # |zhat| of a farmer sample
CFG = types.SimpleNamespace(EF_2stage=True, EF_solver_name=SOLVER, crops_multiplier=1)


# ------------------------------------------------------------------ the kernel alone
KERNEL_CASES = [(1, [0, 1], 0), (64, [0, 64], 0), (65, [0, 1, 64, 65], 0), (257, list(range(258)), 0),
                (777, [0, 300, 301, 777], 0), (1000, [0, 499, 1501, 2000, 2000], 500)]


def _engine(S, seed, scale=1.0):
    """A farmer cm = 1 engine of S scenarios with unequal probabilities (no solve needed)."""
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.examples import farmer
    b = farmer.batch_creator(farmer.scenario_names_creator(S), num_scens=S)
    rng = np.random.RandomState(seed)
    b.prob = scale * (0.25 + rng.rand(S)) / S
    b.prob_coeff = b.prob[:, None].copy()
    return PHEngine(b, device="cuda:0"), b.prob.copy()


def _made_up(S, seed):
    """|f| about 1e5, |g| about 1e2: the cancellation the real data has."""
    rng = np.random.RandomState(1000 + seed)
    fs = -1e5 * (1.0 + 0.1 * rng.rand(S))
    fh = fs + 1e2 * rng.rand(S)
    return fh, fs


def _fsum_rows(p, fh, fs, sh, ss, seg, off):
    """The rows and the sums of |terms| by math.fsum."""
    rows, mags = [], []
    for j in range(len(seg) - 1):
        a, b = max(seg[j] - off, 0), min(seg[j + 1] - off, len(p))
        k = [i for i in range(a, b) if sh[i] == 0 and (ss is None or ss[i] == 0)]
        out = max(b - a, 0) - len(k)
        g = [(float(fh[i]) - float(fs[i])) if fs is not None else 0.0 for i in k]
        fsv = [float(fs[i]) if fs is not None else 0.0 for i in k]
        terms = [[p[i] for i in k], [p[i] * p[i] for i in k], [p[i] * gi for i, gi in zip(k, g)],
                 [p[i] * gi * gi for i, gi in zip(k, g)], [p[i] * fh[i] for i in k],
                 [p[i] * v for i, v in zip(k, fsv)]]
        rows.append([math.fsum(t) for t in terms] + [float(out), 0.0])
        mags.append([math.fsum(abs(v) for v in t) for t in terms])
    return np.array(rows).reshape(-1, 8), np.array(mags).reshape(-1, 6)


def _dev(e, a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype, device=e.device)


def _moments(e, seg, off, fh, sh, fs=None, ss=None):
    return e.gap_moments(seg, _dev(e, fh), _dev(e, sh, torch.int32), _dev(e, fs), _dev(e, ss, torch.int32),
                         s_off=off).copy()


def _check_rows(got, want, mag, what):
    assert got.shape == want.shape
    assert np.array_equal(got[:, 6:], want[:, 6:]), (what, got[:, 6], want[:, 6])
    ratio = np.abs(got[:, :6] - want[:, :6]) / np.where(mag > 0, mag, 1.0)
    assert (got[:, :6][mag == 0] == 0).all(), what
    print(f"gap_moments {what}: worst |sum - fsum| / fsum(|terms|) = {ratio.max():.2e}")
    assert ratio.max() <= SUM_REL, (what, ratio.max())
    return ratio.max()


@pytest.mark.parametrize("S,seg,off", KERNEL_CASES, ids=[f"S{c[0]}" for c in KERNEL_CASES])
def test_gap_moments_against_fsum(gpu, S, seg, off):
    e, p = _engine(S, S)
    try:
        fh, fs = _made_up(S, S)
        ok = np.zeros(S, dtype=np.int32)
        got = _moments(e, seg, off, fh, ok, fs, ok)
        want, mag = _fsum_rows(p, fh, fs, ok, ok, seg, off)
        _check_rows(got, want, mag, f"S={S}")
        assert np.array_equal(got, _moments(e, seg, off, fh, ok, fs, ok))          # the same bits twice
        ws = e.workspace_bytes()
        # the x* side NULL: g and f_star count as 0
        got0 = _moments(e, seg, off, fh, ok)
        want0, mag0 = _fsum_rows(p, fh, None, ok, None, seg, off)
        _check_rows(got0, want0, mag0, f"S={S}, no x* side")
        assert (got0[:, [2, 3, 5]] == 0).all() and np.array_equal(got0[:, [0, 1, 4]], got[:, [0, 1, 4]])
        assert e.workspace_bytes() == ws                                            # no allocation after the first call
        # statuses 1, 2, 3 in the first lane, the last lane and on a segment boundary, in either array
        spots = sorted({0, S - 1, *[min(max(v - off, 0), S - 1) for v in seg[1:-1]],
                        *[min(max(v - off - 1, 0), S - 1) for v in seg[1:-1]]})
        sh, ss = ok.copy(), ok.copy()
        for i, k in enumerate(spots):
            (sh if i % 2 == 0 else ss)[k] = 1 + i % 3
        got1 = _moments(e, seg, off, fh, sh, fs, ss)
        want1, mag1 = _fsum_rows(p, fh, fs, sh, ss, seg, off)
        _check_rows(got1, want1, mag1, f"S={S}, {len(spots)} left out")
        assert got1[:, 6].sum() == len([k for k in spots if seg[0] <= k + off < seg[-1]])
        got2 = _moments(e, seg, off, fh, np.maximum(sh, ss))
        assert np.array_equal(got2[:, 6], got1[:, 6])
    finally:
        e.close()


def test_gap_moments_probability_scale(gpu):
    """Doubling every probability changes no normalised result beyond the last bit."""
    S, seg, off = KERNEL_CASES[4]
    fh, fs = _made_up(S, S)
    ok = np.zeros(S, dtype=np.int32)
    rows = []
    for scale in (1.0, 2.0):
        e, _ = _engine(S, S, scale)
        try:
            rows.append(_moments(e, seg, off, fh, ok, fs, ok))
        finally:
            e.close()
    norm = [np.stack([m[:, 2] / m[:, 0], m[:, 3] / m[:, 0], m[:, 1] / m[:, 0] ** 2, m[:, 4] / m[:, 0],
                      m[:, 5] / m[:, 0]]) for m in rows]
    assert (np.abs(norm[1] - norm[0]) <= 2.3e-16 * np.abs(norm[0])).all()
    assert np.array_equal(rows[1][:, 0], 2 * rows[0][:, 0])


def test_gap_moments_error_returns(gpu):
    from mpisppy_amd import _lib
    e, _ = _engine(65, 65)
    try:
        f = torch.zeros(65, dtype=torch.float64, device=e.device)
        st = torch.zeros(65, dtype=torch.int32, device=e.device)
        seg = torch.tensor([0, 65], dtype=torch.int64, device=e.device)
        out = torch.zeros(8, dtype=torch.float64, device=e.device)
        P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        call = lambda h, fh, sh, fs, ss, sp, n, o: e.lib.phgpu_gap_moments(  # noqa: E731
            h, P(fh), P(sh), P(fs), P(ss), P(sp), n, 0, P(o), e._stream())
        assert call(e.h, f, st, f, st, seg, 1, out) == 0
        for args in ((None, f, st, f, st, seg, 1, out), (e.h, None, st, f, st, seg, 1, out),
                     (e.h, f, None, f, st, seg, 1, out), (e.h, f, st, f, st, None, 1, out),
                     (e.h, f, st, f, st, seg, 1, None)):
            assert call(*args) == -1 and "null argument" in _lib.last_error()
        assert call(e.h, f, st, f, st, seg, 0, out) == -1 and "nseg" in _lib.last_error()
        assert call(e.h, f, st, f, None, seg, 1, out) == -1 and "go together" in _lib.last_error()
        assert call(e.h, f, st, None, st, seg, 1, out) == -1 and "go together" in _lib.last_error()
        torch.cuda.synchronize()
    finally:
        e.close()


# ------------------------------------------------------------------ the estimators
def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _names(count, start=START):
    from mpisppy_amd.examples import farmer
    return farmer.scenario_names_creator(count, start=start)


def _check_G(got, want, zhat, what):
    d = np.abs(np.asarray(got, float) - np.asarray(want, float))
    print(f"{what}: max |G - fixture| = {d.max():.3e} (allowed {G_ABS * np.min(np.abs(zhat)):.3e})")
    assert (d <= G_ABS * np.abs(zhat)).all(), (what, got, want)


def _check_s(got, want, what):
    r = _rel(got, want)
    print(f"{what}: max relative difference to the fixture = {r:.3e} (allowed {S_REL:.1e})")
    assert r <= S_REL, (what, got, want)


@pytest.mark.parametrize("n", [7, 16])
def test_gap_estimators_one_batch(gpu, n):
    from mpisppy_amd.confidence_intervals import ciutils
    from mpisppy_amd.examples import farmer
    c = GOLDEN["cases"]["5x7" if n == 7 else "4x16"]
    info = {}
    r = ciutils.gap_estimators(XHAT, farmer, scenario_names=_names(n), cfg=CFG, solver_name=SOLVER, info=info)
    assert set(r) == {"G", "s", "seed"} and r["seed"] == START + n and info["solves"] == 2
    _check_G([r["G"]], c["Glist"][:1], c["zhat"][:1], f"gap_estimators n={n}")
    _check_s([r["s"]], c["s"][:1], f"gap_estimators n={n}: s")


def test_gap_estimators_pooled(gpu):
    from mpisppy_amd.confidence_intervals import ciutils
    r = ciutils.gap_estimators(XHAT, "mpisppy_amd.examples.farmer", scenario_names=_names(16), ArRP=2, cfg=CFG,
                               solver_name=SOLVER)
    _check_G([r["G"]], [GOLDEN["ArRP2_16"]["G"]], GOLDEN["cases"]["4x16"]["zhat"][:1], "gap_estimators ArRP=2")
    _check_s([r["s"]], [GOLDEN["ArRP2_16"]["s"]], "gap_estimators ArRP=2: s")


_XSTAR = {}


def _xstar(names, kw):
    """x* of a sample by the package's own L-shaped run, computed once per session: the tests below
    share it, so that each pays for its own evaluations only."""
    from mpisppy_amd.confidence_intervals import ciutils
    from mpisppy_amd.examples import farmer
    key = tuple(names)
    if key not in _XSTAR:
        _XSTAR[key] = ciutils.lshaped_xstar(farmer, list(names), kw, SOLVER)
    return _XSTAR[key]


def _batched(case, **kw):
    from mpisppy_amd.confidence_intervals import ciutils
    from mpisppy_amd.examples import farmer
    c = GOLDEN["cases"][case]
    info = {}
    r = ciutils.gap_estimators_batched(XHAT, farmer, c["num_batches"], c["batch_size"], START, cfg=CFG,
                                       solver_name=SOLVER, xstar_solver=_xstar, info=info, **kw)
    assert info["solves"] == 2
    return c, r


@pytest.mark.parametrize("case", ["5x7", "4x16"])
def test_batched_estimators(gpu, case):
    c, r = _batched(case)
    B, n = c["num_batches"], c["batch_size"]
    assert r["seed"] == START + B * n and r["G"].shape == r["s"].shape == (B,)
    _check_G(r["G"], c["Glist"], c["zhat"], f"gap_estimators_batched {case}")
    _check_s(r["s"], c["s"], f"gap_estimators_batched {case}: s")
    assert _rel(r["zhat"], c["zhat"]) <= Z_REL


@pytest.mark.parametrize("case", ["5x7", "4x16"])
def test_batched_equals_the_loop(gpu, case):
    from mpisppy_amd.confidence_intervals import ciutils
    from mpisppy_amd.examples import farmer
    c, r = _batched(case)
    n = c["batch_size"]
    for b in range(c["num_batches"]):
        one = ciutils.gap_estimators(XHAT, farmer, scenario_names=_names(n, START + b * n), cfg=CFG,
                                     solver_name=SOLVER, xstar_solver=_xstar)
        assert abs(one["G"] - r["G"][b]) <= G_ABS * abs(c["zhat"][b]) and _rel([one["s"]], [r["s"][b]]) <= S_REL


@pytest.mark.parametrize("case", ["5x7", "4x16"])
def test_mmw(gpu, case):
    from mpisppy_amd.confidence_intervals.mmw_ci import MMWConfidenceIntervals
    from mpisppy_amd.examples import farmer
    c = GOLDEN["cases"][case]
    info = {}
    mmw = MMWConfidenceIntervals(farmer, CFG, XHAT, c["num_batches"], batch_size=c["batch_size"], start=START,
                                 verbose=False)
    mmw.xstar_solver = _xstar
    m = mmw.run(info=info)
    assert info["solves"] == 2 and m["gap_outer_bound"] == 0 and set(m) == {
        "gap_inner_bound", "gap_outer_bound", "Gbar", "std", "Glist"}
    _check_G(m["Glist"], c["Glist"], c["zhat"], f"MMW {case}")
    _check_G([m["Gbar"]], [c["Gbar"]], [ZMIN], f"MMW {case}: Gbar")
    _check_s([m["std"], m["gap_inner_bound"]], [c["std"], c["gap_inner_bound"]], f"MMW {case}: std, gap_inner_bound")


def test_infeasible_batch_raises(gpu):
    """A candidate outside the acreage row (900 of 500 acres): every scenario is infeasible at it."""
    from mpisppy_amd.confidence_intervals import ciutils
    from mpisppy_amd.examples import farmer
    with pytest.raises(RuntimeError, match=r"batch 0 \(scenarios scen3\.\.scen9\): 7 scenario"):
        ciutils.gap_estimators_batched({"ROOT": np.array([300.0, 300.0, 300.0])}, farmer, 2, 7, START, cfg=CFG,
                                       solver_name=SOLVER)


# ------------------------------------------------------------------ zhat4xhat
def test_evaluate_samples(gpu):
    from mpisppy_amd.confidence_intervals import zhat4xhat
    from mpisppy_amd.examples import farmer
    c = GOLDEN["cases"]["4x16"]
    z, seed = zhat4xhat.evaluate_samples(XHAT["ROOT"], 4, 16, CFG, InitSeed=START, model_module=farmer)
    print(f"evaluate_samples: max relative difference to the fixture = {_rel(z, c['zhat']):.3e}")
    assert seed == START + 64 and z.shape == (4,) and _rel(z, c["zhat"]) <= Z_REL


def test_run_samples(gpu, tmp_path):
    import ci_ref as R
    from mpisppy_amd.confidence_intervals import ciutils, zhat4xhat
    from mpisppy_amd.examples import farmer
    path = str(tmp_path / "xhat.npy")
    ciutils.write_xhat(XHAT, path)
    cfg = types.SimpleNamespace(EF_solver_name=SOLVER, crops_multiplier=1, xhatpath=path, num_samples=4,
                                sample_size=16, confidence_level=0.95)
    zbar, eps = zhat4xhat.run_samples(cfg, farmer)
    f = R.fixed_objectives(R.farmer_scens(0, 64), XHAT["ROOT"]).reshape(4, 16)
    want_z, want_eps = R.zhat_halfwidth([math.fsum(row) / 16 for row in f])
    # a zhat moves by at most Z_REL |zhat|, their standard deviation by no more than that
    slack = Z_REL * np.abs(f).max()
    t = want_eps / (np.std(f.mean(axis=1)) / 2.0)
    print(f"run_samples: zhatbar {zbar} (restatement {want_z}), eps_z {eps} ({want_eps})")
    assert abs(zbar - want_z) <= slack and abs(eps - want_eps) <= t * slack / 2.0


# ------------------------------------------------------------------ sequential sampling
@pytest.mark.parametrize("crit", ["BM", "BPL"])
def test_seqsampling(gpu, crit):
    import ci_ref as R
    from mpisppy_amd.confidence_intervals.seqsampling import SeqSampling, xhat_generator_farmer
    from mpisppy_amd.examples import farmer
    g = GOLDEN["seq_" + crit]
    cfg = dict(R.SEQ_BM if crit == "BM" else R.SEQ_BPL, solver_name=SOLVER, crops_multiplier=1,
               xhat_gen_kwargs={"crops_multiplier": 1})
    ss = SeqSampling(farmer, xhat_generator_farmer, cfg, stopping_criterion=crit, solving_type="EF_2stage")
    r = ss.run(maxit=6)
    print(f"SeqSampling {crit}: T {r['T']}, history {ss.history}, CI {r['CI']}; restatement {g['history']}, {g['CI']}")
    assert set(r) == {"T", "Candidate_solution", "CI"} and r["T"] == g["T"] and ss.history[-1][0] == g["nk"]
    assert r["CI"][0] == 0 and abs(r["CI"][1] - g["CI"][1]) <= G_ABS * ZMIN
    assert r["Candidate_solution"]["ROOT"].shape == (3,)


# ------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ranks_worker(rank, world, port, out_dir):
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
        from mpisppy_amd.confidence_intervals import ciutils
        from mpisppy_amd.examples import farmer
        info = {}
        r = ciutils.gap_estimators_batched(XHAT, farmer, 4, 16, START, cfg=CFG, solver_name=SOLVER, mpicomm=Comm(),
                                           info=info)
        res = {"G": r["G"].tolist(), "s": r["s"].tolist(), "solves": info["solves"]}
        with open(os.path.join(out_dir, f"ci{rank}.json"), "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_match_one(gpu, tmp_path):
    """4 x 16 over two gloo ranks: the batch boundary at 32 is the rank boundary, the 16s fall
    inside each share; both ranks return the one-rank arrays."""
    import torch.multiprocessing as mp
    mp.spawn(_ranks_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"ci{k}.json")) for k in range(2)]
    one = _batched("4x16")[1]
    for k in range(2):
        assert r[k]["solves"] == 2
        print(f"rank {k}: G {_rel(r[k]['G'], one['G']):.2e}, s {_rel(r[k]['s'], one['s']):.2e} relative to one rank")
        assert _rel(r[k]["G"], one["G"]) <= 1e-12 and _rel(r[k]["s"], one["s"]) <= 1e-12
