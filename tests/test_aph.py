"""APH without a GPU: the numpy restatement tests/aph_ref.py against the pins of the reference's
own tests, the admission of every recorded trajectory as a parity fixture, the fixtures
themselves, and the host parts of mpisppy_amd/opt/aph.py.

Admission margins measured (largest difference between HiGHS and interior-point QPs of W, z, x̄
and, relative, theta and conv; smallest dispatch margin over 1e-6 max|phi|):
  farmer30_full 6.4e-9, no partial dispatch;  farmer30_quarter 8.8e-9, 8.9e3;
  farmer30_quarter_lag 9.8e-9, 5.6e3;  farmer30_full_lag (4 passes) 8.5e-9, no partial dispatch;
  farmer30_gamma2 9.0e-9, 1.8e3;  aircond432 (full dispatch) 1.4e-10, no partial dispatch.
"""
import json
import math
import os
import warnings

import numpy as np
import pytest

import aph_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _sig3(v):
    return float(f"{v:.3g}")


# ------------------------------------------------------------------ the reference's own tests
@pytest.mark.parametrize("frac,eobj", [(1.0, 134796.0), (0.25, 134680.0)])
def test_pins_of_the_reference_tests(frac, eobj):
    """Farmer 30 scenarios (Scenario1 .. Scenario30), PHIterLimit 2, rho 1
    (mpisppy/tests/test_aph.py:230-280): to three significant digits."""
    from oracle.models import farmer_scenario
    scens = [farmer_scenario(f"Scenario{i + 1}", 1, num_scens=30) for i in range(30)]
    conv, got, tb, recs = R.APHRef(scens, 1.0, dispatch_frac=frac).main(2)
    print(f"dispatch_frac {frac}: trivial bound {-tb:.3f} E[obj] {-got:.3f} conv {conv:.6f}")
    assert _sig3(-tb) == _sig3(137846.0)
    assert _sig3(-got) == _sig3(eobj)
    assert len(recs[0]["dispatch"]) == 30 and len(recs[1]["dispatch"]) == R.scnt_of(30, frac)


# ------------------------------------------------------------------ admission and fixtures
@pytest.mark.parametrize("name", sorted(R.TRAJECTORIES))
def test_trajectory_is_admitted_as_a_fixture(name):
    d, same, ratio = R.admission(R.TRAJECTORIES[name])
    print(f"{name}: HiGHS against interior point {d:.3e}, same dispatch lists {same}, "
          f"smallest dispatch margin / (1e-6 max|phi|) {ratio:.3e}")
    assert d <= 1e-6 and same
    assert ratio > 1.0


@pytest.mark.parametrize("name", sorted(R.TRAJECTORIES))
def test_fixture_is_what_the_restatement_gives(name):
    fx = json.load(open(os.path.join(HERE, "golden", f"aph_{name}.json")))
    cfg = R.TRAJECTORIES[name]
    assert fx["config"] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}
    t = R.run_trajectory(cfg)
    assert len(fx["iters"]) == cfg["iters"]
    for k in ("trivial", "eobj", "conv"):
        assert abs(t[k] - fx[k]) <= 1e-9 * abs(fx[k]), k
    for o, g in zip(t["iters"], fx["iters"]):
        for k in ("W", "z", "xbar"):
            assert np.abs(o[k] - np.array(g[k])).max() <= 1e-9, k
        for k in ("tau", "phi", "theta", "phisum", "abs_phi", "abs_phi_pre"):
            assert abs(o[k] - g[k]) <= 1e-9 * max(1.0, abs(g[k])), k
        assert o["conv"] == g["conv"] or abs(o["conv"] - g["conv"]) <= 1e-9 * abs(g["conv"])
        assert o["dispatch"] == g["dispatch"]
    # what the trajectories exercise
    frac = cfg.get("dispatch_frac", 1.0)
    assert [len(g["dispatch"]) for g in fx["iters"]] == [R.scnt_of(30 if cfg["model"] == "farmer" else 24, 1.0)] + \
        [R.scnt_of(30 if cfg["model"] == "farmer" else 24, frac)] * (cfg["iters"] - 1)
    assert fx["iters"][0]["theta"] == 0.0 and fx["iters"][0]["conv"] is None      # W = y = 0 at the first pass
    assert all(g["theta"] > 0.0 for g in fx["iters"][1:])


def test_the_shelf_life_key_is_the_reference_s():
    """(-max(last_iter, shelf_life - 1), phi): below shelf_life - 1 phi alone decides; past it
    the most recently dispatched scenarios come first, as the reference writes it."""
    r = R.APHRef(R.farmer_scens(6), 1.0, shelf_life=3)
    r.phis = np.array([5.0, -1.0, 3.0, -2.0, 0.0, 4.0])
    r.last_iter = np.array([1, 1, 2, 2, 1, 1])
    assert r.dispatch(3)[0] == [3, 1, 4]                    # every max(.) is 2: by phi
    r.last_iter = np.array([1, 7, 2, 9, 1, 9])
    assert r.dispatch(3)[0] == [3, 5, 1]                    # iteration 9 first (phi -2, 4), then 7
    r.round_robin = True
    r.last_phi = np.array([0.5, 0.0, 0.0, 0.0, -0.5, 0.0])
    assert r.dispatch(3)[0] == [4, 0, 2]                    # least recently dispatched first, then last phi


# ------------------------------------------------------------------ host parts
def test_dispatch_count_rounds_as_python_does():
    from mpisppy_amd.opt.aph import dispatch_count
    assert dispatch_count(30, 0.25) == 8                    # round(7.5): to even
    assert dispatch_count(10, 0.25) == 2                    # round(2.5): to even
    assert dispatch_count(10, 0.35) == 4                    # round(3.5): to even
    assert dispatch_count(3, 0.67) == 2
    assert dispatch_count(3, 0.01) == 1 and dispatch_count(1, 0.25) == 1      # the floor of 1
    assert dispatch_count(65536, 0.25) == 16384 and dispatch_count(7, 1) == 7
    assert all(dispatch_count(n, f) == R.scnt_of(n, f) for n in (1, 5, 30, 130) for f in (0.1, 0.25, 0.5, 1.0))


def _options(**more):
    o = {"solver_name": "mi355x_pdhg", "PHIterLimit": 2, "defaultPHrho": 1.0, "convthresh": 0.0, "verbose": False,
         "display_progress": False, "toc": False}
    o.update(more)
    return o


def _make(**more):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.aph import APH
    return APH(_options(**more), farmer.scenario_names_creator(3), farmer.scenario_creator,
               scenario_creator_kwargs={"num_scens": 3})


def test_options_and_their_checks():
    a = _make()
    assert (a.APHgamma, a.nu, a.use_lag, a.shelf_life, a.round_robin_dispatch) == (1, 1, False, 99, False)
    assert a.options["async_frac_needed"] == 1 and a.conv is None
    a = _make(APHgamma=2.0, APHnu=1.5, APHuse_lag=True, shelf_life=4, round_robin_dispatch=True, dispatch_frac=0.5,
              async_frac_needed=0.5, async_sleep_secs=0.5, display_convergence_detail=True)
    assert (a.APHgamma, a.nu, a.use_lag, a.shelf_life, a.round_robin_dispatch) == (2.0, 1.5, True, 4, True)
    for bad in ({"APHgamma": 0.0}, {"APHgamma": -1.0}, {"APHnu": 0.0}, {"APHnu": 2.0}, {"dispatch_frac": 0.0},
                {"dispatch_frac": 1.5}):
        with pytest.raises(RuntimeError):
            _make(**bad)
    with pytest.raises(NotImplementedError):
        _make(bundles_per_rank=2)
    with pytest.raises(ValueError):                         # PHBase's required options hold for APH
        from mpisppy_amd.examples import farmer
        from mpisppy_amd.opt.aph import APH
        o = _options()
        del o["PHIterLimit"]
        APH(o, farmer.scenario_names_creator(3), farmer.scenario_creator, scenario_creator_kwargs={"num_scens": 3})


def test_convergence_metric():
    a = _make()
    a.global_pusqnorm, a.global_pwsqnorm, a.global_pvsqnorm, a.global_pzsqnorm = 4.0, 16.0, 9.0, 36.0
    a.Compute_Convergence()
    assert a.conv == pytest.approx(2.0 / 4.0 + 3.0 / 6.0)
    a.global_pwsqnorm = 0.0                                 # no W yet: the metric keeps its value
    a.conv = None
    a.Compute_Convergence()
    assert a.conv is None


def test_aph_hub_dict():
    from types import SimpleNamespace
    from mpisppy_amd.cylinders.hub import APHHub, PHHub
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.aph import APH
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    names = farmer.scenario_names_creator(3)
    cfg = SimpleNamespace(solver_name="mi355x_pdhg", default_rho=2.0, max_iterations=7, rel_gap=1e-4, aph_gamma=1.5,
                          aph_nu=0.8, aph_frac_needed=0.6, aph_dispatch_frac=0.3, aph_sleep_seconds=0.2)
    d = vanilla.aph_hub(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs={"num_scens": 3})
    assert d["hub_class"] is APHHub and issubclass(APHHub, PHHub) and d["opt_class"] is APH
    o = d["opt_kwargs"]["options"]
    assert (o["APHgamma"], o["APHnu"], o["async_frac_needed"], o["dispatch_frac"], o["async_sleep_secs"]) == \
        (1.5, 0.8, 0.6, 0.3, 0.2)
    assert o["defaultPHrho"] == 2.0 and o["PHIterLimit"] == 7
    ph = vanilla.ph_hub(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs={"num_scens": 3})
    assert set(o) - set(ph["opt_kwargs"]["options"]) == {"APHgamma", "APHnu", "async_frac_needed", "dispatch_frac",
                                                         "async_sleep_secs"}
    d0 = vanilla.aph_hub(SimpleNamespace(), farmer.scenario_creator, None, names)
    o0 = d0["opt_kwargs"]["options"]
    assert (o0["APHgamma"], o0["APHnu"], o0["dispatch_frac"]) == (1.0, 1.0, 1.0)
    assert math.isclose(o0["async_sleep_secs"], 0.01)
