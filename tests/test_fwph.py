"""FWPH on the CPU: the numpy restatement tests/fwph_ref.py (mpisppy/fwph/fwph.py:91-303,
519-547), the admission of its trajectories as parity fixtures, the fixtures themselves, and
the host-only parts of the package (options checks, cfg_vanilla.fwph_spoke, the spoke's class
attributes).  The device side is tests/test_gpu_fwph.py.
"""
import functools
import json
import os
import types

import numpy as np
import pytest

import fwph_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FARMER_EF_OBJ = -108390.0     # farmer 3 scenarios EF optimum, pinned in tests/test_oracle_golden.py
FARMER_TRIVIAL = -115405.5555555555


@functools.lru_cache(maxsize=None)
def _admission(name):
    return R.admission(R.TRAJECTORIES[name])


def test_restatement_bounds_are_outer_bounds_and_improve():
    cfg = dict(R.TRAJECTORIES["farmer3"], iters=12)
    t = R.run_trajectory(cfg)
    assert abs(t["trivial"] - FARMER_TRIVIAL) <= 1e-9 * abs(FARMER_TRIVIAL)
    bounds = [o["bound"] for o in t["iters"]]
    assert all(b <= FARMER_EF_OBJ for b in bounds), bounds
    assert max(bounds) > t["trivial"], (max(bounds), t["trivial"])
    # columns grow by about two per outer iteration (the first scenario: 26 after 12)
    assert t["iters"][-1]["ncols"].tolist() == [26, 21, 25]


@pytest.mark.parametrize("name", sorted(R.TRAJECTORIES))
def test_trajectory_is_admitted_as_a_fixture(name):
    """LP-solver independence (HiGHS simplex against the oracle's interior point: x̄, W, xq and
    the bounds to 1e-6, the same column counts) and a break test that no rounding decides."""
    d, same, gam = _admission(name)
    tau = R.TRAJECTORIES[name]["tau"]
    print(f"{name}: max difference {d:.3e}; Gamma nearest above tau {min(g for g in gam if g > tau):.3e}")
    assert d <= 1e-6 and same, (d, same)
    assert not [g for g in gam if 0.5 * tau <= g <= 1.5 * tau]


@pytest.mark.parametrize("name", sorted(R.TRAJECTORIES))
def test_fixture_is_what_the_restatement_gives(name):
    fx = json.load(open(os.path.join(HERE, "golden", f"fwph_{name}.json")))
    cfg = R.TRAJECTORIES[name]
    assert {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()} == fx["config"]
    t = R.run_trajectory(cfg)
    assert abs(t["trivial"] - fx["trivial"]) <= 1e-9 * abs(fx["trivial"])
    assert len(t["iters"]) == len(fx["iters"]) == cfg["iters"]
    for o, g in zip(t["iters"], fx["iters"]):
        assert abs(o["bound"] - g["bound"]) <= 1e-9 * abs(g["bound"])
        assert abs(o["diff"] - g["diff"]) <= 1e-9 * max(1.0, abs(g["diff"]))
        assert np.abs(o["xbar"] - np.array(g["xbar"])).max() <= 1e-7
        assert np.abs(o["W"] - np.array(g["W"])).max() <= 1e-7
        assert o["ncols"].tolist() == g["ncols"] and o["nit"].tolist() == g["nit"]


def test_column_qp_on_singular_grams():
    """A repeated column and K > nn + 1: the weights are not unique, x(a) and phi are."""
    rng = np.random.default_rng(5)
    X = rng.integers(0, 5, size=(7, 2)).astype(float) * 50.0
    X[6] = X[0]
    f = -rng.random(7) * 1e4
    f[6] = f[0]
    W, rho, xbar = rng.normal(size=2) * 20, np.array([1.0, 2.5]), np.array([80.0, 120.0])
    a, x, phi = R.solve_column_qp(X, f, W, rho, xbar)
    assert a.min() >= 0 and abs(a.sum() - 1) <= 1e-12
    p = np.array([6, 1, 2, 3, 4, 5, 0])
    a2, x2, phi2 = R.solve_column_qp(X[p], f[p], W, rho, xbar)
    assert np.abs(x - x2).max() <= 1e-6 and abs(phi - phi2) <= 1e-6 * abs(phi)
    assert R.qp_gap(X, f, W, rho, xbar, a) <= 1e-6 * max(1.0, abs(R.qp_objective(X, f, W, rho, xbar, a)))


def test_a_full_store_replaces_the_least_weighted_column_but_never_the_newest():
    r = R.make_ref(R.TRAJECTORIES["farmer3"], max_cols=3)
    r.prep()
    r.cols[0] = [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0])]
    r.f[0] = [0.0, 0.0, 0.0]
    r.a[0] = np.array([0.0, 0.5, 0.0])
    r.newest[0] = 0
    r._add_column(0, np.array([9.0, 9, 9]), 1.0)
    assert r.cols[0][2][0] == 9.0 and r.newest[0] == 2          # index 0 is the newest: the tie goes to 2
    r.a[0] = np.array([0.0, 0.5, 0.0])
    r._add_column(0, np.array([7.0, 7, 7]), 1.0)
    assert r.cols[0][0][0] == 7.0 and r.newest[0] == 0          # lowest index among the ties


# ------------------------------------------------------------------ options, cfg, spoke
def _fw(**kw):
    o = {"FW_iter_limit": 3, "FW_weight": 0.0, "FW_conv_thresh": 1e-4, "solver_name": "mi355x_pdhg"}
    o.update(kw)
    return o


def _opt(fw_options, **kw):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.fwph.fwph import FWPH
    ph_options = {"solver_name": "mi355x_pdhg", "PHIterLimit": 3, "defaultPHrho": 1.0, "convthresh": 0.0,
                  "verbose": False, "display_progress": False, "toc": False}
    ph_options.update(kw.pop("ph_options", {}))
    sck = {"num_scens": 3}
    sck.update(kw.pop("scenario_creator_kwargs", {}))
    return FWPH(ph_options, fw_options, farmer.scenario_names_creator(3), farmer.scenario_creator,
                scenario_creator_kwargs=sck, **kw)


def test_options_checks():
    for missing in ("FW_iter_limit", "FW_weight", "FW_conv_thresh", "solver_name"):
        o = _fw()
        del o[missing]
        with pytest.raises(RuntimeError, match=missing):
            _opt(o)
    with pytest.raises(RuntimeError, match="FW_iter_limit set to 1"):
        _opt(_fw(FW_iter_limit=1))
    with pytest.raises(RuntimeError, match="FW_max_columns"):
        _opt(_fw(FW_max_columns=65))
    o = _fw()
    fw = _opt(o)
    assert o["time_limit"] == np.inf and o["FW_max_columns"] == 32 and fw.vb
    assert not _opt(_fw(FW_verbose=False)).vb
    # mip_solver_options go into the LP solves' options; the plugin keys among them are ignored later
    fw = _opt(_fw(mip_solver_options={"mipgap": 0.01, "eps_rel": 1e-8}))
    assert fw._lp_options({"max_iter": 64})["eps_rel"] == 1e-8 and fw._lp_options({})["mipgap"] == 0.01


def test_unsupported_inputs_raise():
    with pytest.raises(NotImplementedError, match="point_creator"):
        _opt(_fw(point_creator=lambda *a, **k: []))
    with pytest.raises(NotImplementedError, match="bundles"):
        _opt(_fw(), ph_options={"bundles_per_rank": 2})

    def quad_creator(name, **kw):
        from mpisppy_amd.examples import farmer
        m = farmer.scenario_creator(name, **kw)
        m.quad[0] = 1.0
        return m
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.fwph.fwph import FWPH
    with pytest.raises(NotImplementedError, match="q = 0"):
        FWPH({"solver_name": "mi355x_pdhg", "PHIterLimit": 3, "defaultPHrho": 1.0, "convthresh": 0.0,
              "verbose": False, "display_progress": False, "toc": False}, _fw(),
             farmer.scenario_names_creator(3), quad_creator, scenario_creator_kwargs={"num_scens": 3})


def test_cfg_vanilla_fwph_spoke_dict():
    from mpisppy_amd.cylinders.fwph_spoke import FrankWolfeOuterBound
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.fwph.fwph import FWPH
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    cfg = types.SimpleNamespace(solver_name="mi355x_pdhg", default_rho=1.0, max_iterations=7, verbose=False,
                                fwph_iter_limit=4, fwph_weight=0.25, fwph_conv_thresh=1e-3,
                                fwph_stop_check_tol=1e-5, fwph_mipgap=0.02, max_solver_threads=2)
    names = farmer.scenario_names_creator(3)
    d = vanilla.fwph_spoke(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs={"num_scens": 3})
    assert d["spoke_class"] is FrankWolfeOuterBound and d["opt_class"] is FWPH
    kw = d["opt_kwargs"]
    assert kw["FW_options"] == {"FW_iter_limit": 4, "FW_weight": 0.25, "FW_conv_thresh": 1e-3,
                                "stop_check_tol": 1e-5, "solver_name": "mi355x_pdhg", "FW_verbose": False,
                                "mip_solver_options": {"threads": 2, "mipgap": 0.02},
                                "qp_solver_options": {"threads": 2}}
    assert kw["PH_options"]["convthresh"] == 0 and kw["PH_options"]["PHIterLimit"] == 7
    assert kw["all_scenario_names"] == names and kw["scenario_creator_kwargs"] == {"num_scens": 3}
    # the reference's defaults (config.py fwph_args) for what cfg leaves out
    d = vanilla.fwph_spoke(types.SimpleNamespace(), farmer.scenario_creator, None, names)
    assert d["opt_kwargs"]["FW_options"]["FW_iter_limit"] == 10 and d["opt_kwargs"]["FW_options"]["FW_weight"] == 0.0
    fw = d["opt_class"](**{**d["opt_kwargs"], "scenario_creator_kwargs": {"num_scens": 3}})    # the dict builds
    assert fw.FW_options["FW_max_columns"] == 32


def test_spoke_class_attributes():
    from mpisppy_amd.cylinders.fwph_spoke import FrankWolfeOuterBound
    from mpisppy_amd.cylinders.hub import Hub
    from mpisppy_amd.cylinders.spoke import ConvergerSpokeType, OuterBoundSpoke
    assert issubclass(FrankWolfeOuterBound, OuterBoundSpoke)
    assert FrankWolfeOuterBound.converger_spoke_char == "F"
    assert FrankWolfeOuterBound.converger_spoke_types == (ConvergerSpokeType.OUTER_BOUND,)
    hub = Hub.__new__(Hub)
    hub.spokes = [FrankWolfeOuterBound]
    hub.initialize_spoke_indices()
    assert hub.bounds_only_indices == {1} and hub.outerbound_spoke_chars == {1: "F"}
    assert not hub.has_w_spokes and not hub.has_nonant_spokes
