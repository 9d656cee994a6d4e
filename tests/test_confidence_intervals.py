"""mpisppy_amd.confidence_intervals without a GPU: the Student-t quantile, correcting_numeric,
the xhat files, every constructor and option refusal, the host arithmetic behind the estimators,
the new library symbol, and the numpy / HiGHS restatement tests/ci_ref.py against hand-checkable
cases and against its recorded fixture tests/golden/mmw_farmer.json."""
import json
import math
import os
import re
import types

import numpy as np
import pytest

import ci_ref as R
from mpisppy_amd.confidence_intervals import ciutils, mmw_ci, seqsampling, zhat4xhat
from mpisppy_amd.examples import farmer

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "mmw_farmer.json")))
SOLVER = "mi355x_pdhg"


# ------------------------------------------------------------------ t_ppf
def test_t_ppf_against_scipy():
    from scipy import stats
    worst = 0.0
    for df in range(1, 201):
        for q in (0.8, 0.9, 0.95, 0.975, 0.99, 0.999):
            want = float(stats.t.ppf(q, df))
            worst = max(worst, abs(ciutils.t_ppf(q, df) - want) / abs(want))
    print(f"t_ppf: worst relative difference to scipy {worst:.2e}")
    assert worst <= 1e-10
    assert ciutils.t_ppf(0.5, 7) == 0.0 and ciutils.t_ppf(0.05, 4) == -ciutils.t_ppf(0.95, 4)
    with pytest.raises(ValueError):
        ciutils.t_ppf(1.0, 3)


def test_product_package_imports_no_scipy():
    pkg = os.path.join(ROOT, "mpi-sppy-1_amd", "mpisppy_amd", "confidence_intervals")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            assert not re.search(r"^\s*(import|from)\s+scipy", open(os.path.join(pkg, f)).read(), re.M), f


# ------------------------------------------------------------------ correcting_numeric
def test_correcting_numeric_branches(capsys):
    mn, mx = types.SimpleNamespace(), types.SimpleNamespace(pyo_opt_sense=-1)
    # minimisation: a large negative G comes back with a warning, a small one becomes 0
    assert ciutils.correcting_numeric(-20.0, mn, objfct=1e5) == -20.0
    assert "wrong sign" in capsys.readouterr().out
    assert ciutils.correcting_numeric(-5.0, mn, objfct=1e5) == 0
    assert ciutils.correcting_numeric(12.5, mn, objfct=1e5) == 12.5
    # maximisation: the mirror image
    assert ciutils.correcting_numeric(20.0, mx, objfct=-1e5) == 20.0
    assert "wrong sign" in capsys.readouterr().out
    assert ciutils.correcting_numeric(5.0, mx, objfct=-1e5) == 0
    assert ciutils.correcting_numeric(-12.5, mx, objfct=-1e5) == -12.5
    # the relative / absolute switch: 1e-4 |objfct| against 1e-4
    assert ciutils.correcting_numeric(-5.0, mn, relative_error=False, objfct=1e5) == -5.0
    assert ciutils.correcting_numeric(-5e-5, mn, relative_error=False, objfct=1e5) == 0
    with pytest.raises(RuntimeError, match="objective function"):
        ciutils.correcting_numeric(1.0, mn)
    # the restatement agrees on the minimisation cases
    for G in (-20.0, -5.0, 12.5):
        assert R.correcting_numeric(G, 1e5) == ciutils.correcting_numeric(G, mn, objfct=1e5)


# ------------------------------------------------------------------ xhat files
def test_xhat_file_round_trips(tmp_path):
    xhat = {"ROOT": np.array([80.0, 250.0, 170.0 + 1e-9])}
    p = str(tmp_path / "xhat.npy")
    ciutils.write_xhat(xhat, p)
    assert np.array_equal(ciutils.read_xhat(p)["ROOT"], xhat["ROOT"])
    assert np.array_equal(ciutils.read_xhat(p, delete_file=True)["ROOT"], xhat["ROOT"]) and not os.path.exists(p)
    t = str(tmp_path / "xhat.txt")
    ciutils.writetxt_xhat(xhat, t)
    assert np.array_equal(ciutils.readtxt_xhat(t)["ROOT"], xhat["ROOT"])
    ciutils.readtxt_xhat(t, delete_file=True)
    assert not os.path.exists(t)
    for fct in (ciutils.write_xhat, ciutils.writetxt_xhat):
        with pytest.raises(RuntimeError, match="2-stage"):
            fct(xhat, p, num_stages=3)
    for fct in (ciutils.read_xhat, ciutils.readtxt_xhat):
        with pytest.raises(RuntimeError, match="2-stage"):
            fct(p, num_stages=3)


# ------------------------------------------------------------------ cfg access
def test_cfg_view():
    base = types.SimpleNamespace(crops_multiplier=2, EF_solver_name=SOLVER, nothing=None)
    v = ciutils.CfgView(base, num_scens=7)
    assert v.get("num_scens") == 7 and v.crops_multiplier == 2 and v["EF_solver_name"] == SOLVER
    assert "EF_solver_name" in v and "EF_2stage" not in v and v.get("nothing", 3) == 3
    assert farmer.kw_creator(v) == {"use_integer": False, "crops_multiplier": 2, "num_scens": 7}
    w = v()
    w.quick_assign("num_scens", int, 9)
    assert w.num_scens == 9 and v.num_scens == 7 and not hasattr(base, "num_scens")
    assert ciutils.CfgView({"a": 1}).a == 1 and ciutils.CfgView(None).get("a") is None
    with pytest.raises(AttributeError):
        v.missing


# ------------------------------------------------------------------ refusals
def _incomplete():
    return types.SimpleNamespace(__name__="half", scenario_names_creator=farmer.scenario_names_creator,
                                 scenario_creator=farmer.scenario_creator)


def test_mmw_constructor_refusals(capsys):
    xhat = {"ROOT": np.array(R.FARMER_XHAT)}
    ok = types.SimpleNamespace(EF_2stage=True, EF_solver_name=SOLVER)
    M = mmw_ci.MMWConfidenceIntervals
    m = M(farmer, ok, xhat, 5, batch_size=7, start=3)
    assert m.type == "EF_2stage" and not m.multistage and m.numstages == 2
    assert M("mpisppy_amd.examples.farmer", ok, xhat, 5, batch_size=7, start=3).refmodel is farmer
    with pytest.raises(RuntimeError, match="Start must be specified"):
        M(farmer, ok, xhat, 5, batch_size=7)
    with pytest.raises(RuntimeError, match="Only EF is currently supported"):
        M(farmer, types.SimpleNamespace(EF_solver_name=SOLVER), xhat, 5, batch_size=7, start=3)
    with pytest.raises(NotImplementedError, match="sample_tree"):
        M(farmer, types.SimpleNamespace(EF_mstage=True, EF_solver_name=SOLVER), xhat, 5, batch_size=7, start=3)
    with pytest.raises(RuntimeError, match="EF_solver_name not in"):
        M(farmer, types.SimpleNamespace(EF_2stage=True), xhat, 5, batch_size=7, start=3)
    with pytest.raises(RuntimeError, match="not complete for MMW"):
        M(_incomplete(), ok, xhat, 5, batch_size=7, start=3)
    assert "missing kw_creator" in capsys.readouterr().out
    with pytest.raises(RuntimeError, match="batch size"):
        M(farmer, ok, xhat, 5, batch_size=0, start=3).run()


def test_gap_estimators_refusals():
    xhat = {"ROOT": np.array(R.FARMER_XHAT)}
    names = farmer.scenario_names_creator(7, start=3)
    with pytest.raises(NotImplementedError, match="sample_tree"):
        ciutils.gap_estimators(xhat, farmer, solving_type="EF_mstage", scenario_names=names)
    with pytest.raises(RuntimeError, match="Only EF solve"):
        ciutils.gap_estimators(xhat, farmer, solving_type="PH", scenario_names=names)
    with pytest.raises(RuntimeError, match="scenario_names"):
        ciutils.gap_estimators(xhat, farmer)
    for missing in ("scenario_names_creator", "scenario_creator", "kw_creator", "scenario_denouement"):
        mod = types.SimpleNamespace(**{k: getattr(farmer, k) for k in
                                       ("scenario_names_creator", "scenario_creator", "kw_creator",
                                        "scenario_denouement") if k != missing})
        with pytest.raises(RuntimeError, match=missing):
            ciutils.gap_estimators(xhat, mod, scenario_names=names, solver_name=SOLVER)
    with pytest.raises(RuntimeWarning, match="mutliple of 2"):
        ciutils.gap_estimators(xhat, farmer, scenario_names=names, ArRP=2, solver_name=SOLVER)
    with pytest.raises(NotImplementedError, match="sample_tree"):
        zhat4xhat.evaluate_sample_trees(None, 1, None)


def test_seqsampling_refusals_and_schedules(capsys):
    S = seqsampling.SeqSampling
    gen = seqsampling.xhat_generator_farmer
    bm = dict(R.SEQ_BM, solver_name=SOLVER)
    with pytest.raises(RuntimeError, match="missing: \\['BM_hprime'\\]"):
        S(farmer, gen, {k: v for k, v in bm.items() if k != "BM_hprime"}, stopping_criterion="BM")
    with pytest.raises(RuntimeError, match="missing: \\['BPL_eps'\\]"):
        S(farmer, gen, {"solver_name": SOLVER}, stopping_criterion="BPL")
    with pytest.raises(RuntimeError, match="Only BM and BPL"):
        S(farmer, gen, bm, stopping_criterion="XYZ")
    with pytest.raises(RuntimeError, match="solving_type None is not supported"):
        S(farmer, gen, bm, solving_type="None")
    with pytest.raises(NotImplementedError, match="sample_tree"):
        S(farmer, gen, bm, solving_type="EF_mstage")
    with pytest.raises(RuntimeError, match="not complete for seqsampling"):
        S(_incomplete(), gen, bm)
    capsys.readouterr()
    with pytest.raises(RuntimeError, match="cannot process type"):
        seqsampling.add_options(ciutils.CfgView(None), {"x": [1]})
    # the schedules against the restatement
    s = S(farmer, gen, bm, stopping_criterion="BM")
    c = R.bm_constant(bm["BM_p"], bm["BM_q"], 0.95)
    assert s._bm_constant() == pytest.approx(c, rel=1e-15)
    for k in range(1, 8):
        assert s.bm_sampsize(k, None, None, None) == R.bm_sampsize(k, bm, c)
    noq = S(farmer, gen, dict(bm, BM_q=None), stopping_criterion="BM")
    assert [noq.bm_sampsize(k, None, None, None) for k in (1, 2, 5)] == \
        [R.bm_sampsize(k, dict(bm, BM_q=None), R.bm_constant(0.2, None, 0.95)) for k in (1, 2, 5)]
    b = S(farmer, gen, dict(R.SEQ_BPL, solver_name=SOLVER), stopping_criterion="BPL")
    assert b.ArRP == 2 and [b.bpl_fsp_sampsize(k, None, None, None) for k in (1, 2, 3)] == [10, 12, 14]
    assert [R.bpl_sampsize(k, R.SEQ_BPL) for k in (1, 2, 3)] == [10, 12, 14]
    # the criteria at the restatement's recorded (n_k, G_k, s_k): continue at k = 1, stop at k = 2
    for key, obj in (("seq_BM", s), ("seq_BPL", b)):
        h = GOLDEN[key]["history"]
        assert len(h) == GOLDEN[key]["T"] == 2
        assert obj.stop_criterion(h[0][1], h[0][2], h[0][0]) and not obj.stop_criterion(h[1][1], h[1][2], h[1][0])
    st = S(farmer, gen, {"BPL_eps": 700.0, "solver_name": SOLVER}, stochastic_sampling=True, stopping_criterion="BPL")
    assert st.stochastic_sampsize(1, None, None, None) == 50
    t = ciutils.t_ppf(0.95, 49)
    root = ((1 + t * 400.0) + math.sqrt((1 + t * 400.0) ** 2 + 4 * 700.0 * 50 * 300.0)) / (2 * 700.0)
    assert st.stochastic_sampsize(2, 300.0, 400.0, 50) == math.ceil(root ** 2)


# ------------------------------------------------------------------ the library symbol
def test_gap_moments_symbol():
    import ctypes
    from mpisppy_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "phgpu.h")).read()
    assert re.search(r"^int phgpu_gap_moments\(phgpu_handle h,", hdr, re.M)
    assert "phgpu_gap_moments" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "phgpu_gap_moments")
    assert lib.phgpu_gap_moments(None, None, None, None, None, None, 1, 0, None, None) == -1
    assert "null argument" in _lib.last_error()
    assert ctypes.c_int64 in lib.phgpu_gap_moments.argtypes


# ------------------------------------------------------------------ the host arithmetic
def test_estimators_by_hand():
    # two scenarios, equal probabilities: g = (3, 9), G = 6, E g^2 = 45, sum p^2 = 1/2
    r = R.estimators_from_objectives([10.0, 20.0], [7.0, 11.0], [0.5, 0.5])
    assert r["G"] == 6.0 and r["zhat"] == 15.0 and r["zstar"] == 9.0
    assert r["s"] == pytest.approx(math.sqrt((45.0 - 36.0) / 0.5), rel=1e-15)
    # unequal probabilities on any scale: p = (1, 3) / 4
    for scale in (1.0, 0.25, 8.0):
        r = R.estimators_from_objectives([10.0, 20.0], [7.0, 11.0], [1.0 * scale, 3.0 * scale])
        assert r["G"] == pytest.approx(7.5, rel=1e-15)
        assert r["s"] == pytest.approx(math.sqrt((0.25 * 9 + 0.75 * 81 - 7.5 ** 2) / (1 - (1 + 9) / 16)), rel=1e-14)
    # a numerically small negative gap is clipped, a large one is kept
    assert R.estimators_from_objectives([1e5, 1e5], [1e5 + 1, 1e5 + 1], [0.5, 0.5])["G"] == 0.0
    assert R.estimators_from_objectives([1e5, 1e5], [1e5 + 50, 1e5 + 50], [0.5, 0.5])["G"] == -50.0


def test_moments_to_estimators_matches_restatement():
    """The product's host step from the device rows, on rows made by numpy from made-up objectives."""
    rng = np.random.RandomState(5)
    rows, want = [], []
    for n, scale in ((7, 1.0), (16, 1.0 / 3), (2, 5.0)):
        fs = -1.3e5 + 1e3 * rng.randn(n)
        fh = fs + 1e2 * rng.rand(n)
        p = scale * (0.5 + rng.rand(n))
        g = fh - fs
        rows.append([p.sum(), (p * p).sum(), (p * g).sum(), (p * g * g).sum(), (p * fh).sum(), (p * fs).sum(), 0, 0])
        want.append(R.estimators_from_objectives(fh, fs, p))
    got = ciutils.moments_to_estimators(np.array(rows), 1, None)
    for j, w in enumerate(want):
        for key in ("G", "s", "zhat", "zstar"):
            assert got[key][j] == pytest.approx(w[key], rel=1e-9), (j, key)


def test_mmw_arithmetic():
    r = R.mmw([1.0, 2.0, 3.0, 6.0])
    from scipy import stats
    assert r["Gbar"] == 3.0 and r["std"] == pytest.approx(math.sqrt(3.5)) and r["gap_outer_bound"] == 0
    assert r["gap_inner_bound"] == pytest.approx(3.0 + stats.t.ppf(0.95, 3) * math.sqrt(3.5) / 2.0)
    assert R.zhat_halfwidth([1.0, 2.0, 3.0, 6.0]) == pytest.approx((3.0, r["gap_inner_bound"] - 3.0))


# ------------------------------------------------------------------ the restatement on farmer
def test_farmer_candidate_is_the_ef_optimum():
    import lshaped_ref as LR
    _, x = LR.ef_optimum(R.farmer_scens(0, 3))
    assert np.allclose(x, R.FARMER_XHAT, atol=1e-7) and GOLDEN["xhat"] == list(R.FARMER_XHAT)


def test_restatement_reproduces_the_fixture():
    rec = R.golden_record()
    quoted = {"5x7": [170.33, 475.82, 506.45, 537.70, 234.95], "4x16": [217.49, 288.60, 592.19, 462.30]}
    for name, c in rec["cases"].items():
        g = GOLDEN["cases"][name]
        assert np.allclose(c["Glist"], quoted[name], atol=0.006)
        assert min(c["Glist"]) > 100 and 597 <= min(c["s"]) and max(c["s"]) <= 2471
        for key in ("Glist", "s", "zhat", "Gbar", "std", "gap_inner_bound"):
            assert np.allclose(c[key], g[key], rtol=1e-7, atol=0), (name, key)
    assert 597 <= min(rec["cases"]["5x7"]["s"]) < 598 and 2470 < max(rec["cases"]["4x16"]["s"]) < 2471
    assert abs(abs(rec["cases"]["4x16"]["zhat"][0]) - 1.3e5) < 1e4
    assert np.allclose([rec["ArRP2_16"]["G"], rec["ArRP2_16"]["s"]], [GOLDEN["ArRP2_16"]["G"], GOLDEN["ArRP2_16"]["s"]],
                       rtol=1e-7)
    assert np.allclose(rec["zhat_halfwidth_4x16"], GOLDEN["zhat_halfwidth_4x16"], rtol=1e-9)
    for key in ("seq_BM", "seq_BPL"):
        assert rec[key]["T"] == GOLDEN[key]["T"] == 2 and rec[key]["nk"] == GOLDEN[key]["nk"] == 12
        assert np.allclose(rec[key]["CI"], GOLDEN[key]["CI"], rtol=1e-7)
        assert np.allclose(rec[key]["history"], GOLDEN[key]["history"], rtol=1e-7)
