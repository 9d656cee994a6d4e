"""The xhat candidates that are functions of all scenarios (x̄, the scenario closest to x̄,
slam-max / slam-min), CPU side: the library's exports, the numpy restatement
(tests/xhat_cand_ref.py) against the oracle on farmer 30, the option / cfg_vanilla wiring
and the two-stage-only RuntimeErrors.  The device side is tests/test_gpu_xhat_candidates.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import xhat_cand_ref as R


def test_exports_and_null_handle():
    from mpisppy_amd import _lib
    assert "phgpu_nonant_stats" in _lib.EXPORTS and "phgpu_nonant_closest" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.phgpu_nonant_stats(None, None, None, None) == -1
    assert lib.phgpu_nonant_closest(None, None, None, None, None, None, None) == -1
    assert "null" in _lib.last_error()


@pytest.mark.parametrize("it", R.FARMER_ITERS)
def test_restatement_against_the_oracle(it):
    """Farmer 30, rho 1, OraclePH(solver="farmer"): the closest winner equals a brute-force
    loop and is clear of the runner-up; x̄ and slam-min are feasible, slam-max is not (the
    land row)."""
    r = R.farmer_trajectory()[it]
    v, pl = r["v"], r["planes"]
    S = v.shape[1]
    p = 1.0 / S
    # the planes against plain numpy
    np.testing.assert_allclose(pl[0], (p * v).sum(1), rtol=1e-13)
    np.testing.assert_allclose(pl[1], (p * v * v).sum(1), rtol=1e-13)
    assert np.array_equal(-pl[2], v.min(1)) and np.array_equal(pl[3], v.max(1))
    # brute force: vectorised distances, first index of the minimum
    var = pl[1] - pl[0] * pl[0]
    z = np.where(var[:, None] > 0, np.minimum(3.0, np.abs(v - pl[0][:, None]) / np.sqrt(np.where(var > 0, var, 1.0))[:, None]),
                 0.0)
    brute = z.sum(0)
    np.testing.assert_allclose(r["dist"], brute, rtol=1e-12)
    assert r["winner"] == int(np.argmin(brute))
    srt = np.sort(r["dist"])
    print(f"iter {it}: winner scen{r['winner']} dist {srt[0]:.6f} runner-up {srt[1]:.6f} margin {srt[1] - srt[0]:.3e}; "
          f"xbar {r['xbar_obj']}, slam-min {r['slammin_obj']}, slam-max {r['slammax_obj']}, closest {r['closest_obj']}")
    assert srt[1] - srt[0] >= 1e-6
    assert r["xbar_obj"] is not None and r["slammin_obj"] is not None
    assert r["slammax_obj"] is None
    assert r["closest_obj"] is not None


def test_post_everything_state_is_clear_of_a_tie():
    """The state XhatClosest.post_everything sees after 5 PH iterations (the x̄ of the solve
    before the last): its winner too is clear of the runner-up."""
    r = R.farmer_trajectory()["post"]
    srt = np.sort(r["dist"])
    print("post_everything: winner", r["winner"], "margin", srt[1] - srt[0])
    assert srt[1] - srt[0] >= 1e-6 and r["closest_obj"] is not None


def test_tie_rules():
    assert R.local_winner([2.0, 1.0, 1.0, 3.0]) == (1.0, 1)          # lowest index within a rank
    assert R.rank_winner([1.0, 1.0, 2.0]) == 1                       # highest rank between ranks
    assert R.rank_winner([0.5, 1.0]) == 0
    v = np.array([[1.0, 2.0, 3.0, 30.0], [5.0, 5.0, 5.0, 5.0]])
    p = 0.25
    xbar, xsq = (p * v).sum(1), (p * v * v).sum(1)
    d = R.distances(v, xbar, xsq)
    assert xsq[1] - xbar[1] * xbar[1] == 0.0                         # the constant column is skipped
    sd = np.sqrt(xsq[0] - xbar[0] ** 2)
    np.testing.assert_allclose(d, np.minimum(3.0, np.abs(v[0] - xbar[0]) / sd), rtol=1e-15)


def _cfg(**kw):
    return SimpleNamespace(solver_name="mi355x_pdhg", default_rho=1.0, max_iterations=5, rel_gap=1e-4,
                           device="cuda:0", toc=False, iterk_solver_options={"eps_rel": 1e-8}, **kw)


def test_cfg_vanilla_wiring():
    from mpisppy_amd.cylinders.slam_heuristic import SlamMaxHeuristic, SlamMinHeuristic
    from mpisppy_amd.cylinders.spoke import ConvergerSpokeType, InnerBoundNonantSpoke
    from mpisppy_amd.cylinders.xhatxbar_bounder import XhatXbarInnerBound
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    names = farmer.scenario_names_creator(3)
    kw = {"num_scens": 3}
    d = vanilla.xhatxbar_spoke(_cfg(xhat_scen_limit=7), farmer.scenario_creator, None, names,
                               scenario_creator_kwargs=kw)
    assert d["spoke_class"] is XhatXbarInnerBound and d["opt_class"] is Xhat_Eval
    o = d["opt_kwargs"]["options"]
    assert o["bundles_per_rank"] == 0
    assert o["xhat_xbar_options"] == {"xhat_solver_options": {"eps_rel": 1e-8}, "scen_limit": 7,
                                      "dump_prefix": "delme", "csvname": "xbar.csv"}
    assert d["opt_kwargs"]["all_scenario_names"] == names and d["opt_kwargs"]["scenario_creator_kwargs"] == kw
    assert "variable_probability" in d["opt_kwargs"]
    for fn, cls in ((vanilla.slammax_spoke, SlamMaxHeuristic), (vanilla.slammin_spoke, SlamMinHeuristic)):
        d = fn(_cfg(), farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
        assert d["spoke_class"] is cls and d["opt_class"] is Xhat_Eval
        assert d["opt_kwargs"]["options"]["bundles_per_rank"] == 0
        assert d["opt_kwargs"]["options"]["iterk_solver_options"] == {"eps_rel": 1e-8}
        assert cls.converger_spoke_char == "S" and issubclass(cls, InnerBoundNonantSpoke)
    assert XhatXbarInnerBound.converger_spoke_char == "B"
    assert XhatXbarInnerBound.converger_spoke_types == (ConvergerSpokeType.INNER_BOUND,
                                                        ConvergerSpokeType.NONANT_GETTER)


def test_extension_options():
    from mpisppy_amd.extensions.xhatbase import XhatBase
    from mpisppy_amd.extensions.xhatclosest import XhatClosest
    from mpisppy_amd.extensions.xhatxbar import XhatXbar
    opt = SimpleNamespace(cylinder_rank=0, n_proc=1, all_scenario_names=["scen0", "scen1"], multistage=False,
                          options={"verbose": False,
                                   "xhat_xbar_options": {"xhat_solver_options": {"eps_rel": 1e-7}, "keep_solution": False},
                                   "xhat_closest_options": {"xhat_solver_options": {"max_iter": 64}}})
    xb, xc = XhatXbar(opt), XhatClosest(opt)
    assert isinstance(xb, XhatBase) and isinstance(xc, XhatBase)
    assert xb.solver_options == {"eps_rel": 1e-7} and xb.keep_solution is False
    assert xc.solver_options == {"max_iter": 64} and xc.keep_solution is True
    xc.pre_iter0()
    with pytest.raises(KeyError):
        XhatXbar(SimpleNamespace(cylinder_rank=0, n_proc=1, all_scenario_names=["a"], options={}))


def _aircond_xhat_eval():
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    bf = [4, 3, 2]
    opts = {"solver_name": "mi355x_pdhg", "verbose": False, "toc": False, "batch_creator": aircond.batch_creator,
            "xhat_closest_options": {"xhat_solver_options": {}}}
    return Xhat_Eval(opts, aircond.scenario_names_creator(24), aircond.scenario_creator,
                     all_nodenames=create_nodenames_from_branching_factors(bf),
                     scenario_creator_kwargs={"branching_factors": bf, "start_seed": 0})


def test_two_stage_only_errors():
    """Slam and closest on aircond 4-3-2 raise the reference's RuntimeErrors (no GPU needed:
    the checks come before any engine is made)."""
    from mpisppy_amd.cylinders.slam_heuristic import SlamMaxHeuristic, SlamMinHeuristic
    from mpisppy_amd.extensions.xhatclosest import XhatClosest
    xe = _aircond_xhat_eval()
    assert xe.multistage and xe.engine is None
    for cls in (SlamMaxHeuristic, SlamMinHeuristic):
        with pytest.raises(RuntimeError, match=f"The {cls.__name__} only supports two-stage models at this time."):
            cls(xe).main()
    with pytest.raises(RuntimeError, match="xhatclosest not done for multi-stage"):
        XhatClosest(xe).pre_iter0()
    assert xe.engine is None
    # and the spokes insist on an Xhat_Eval
    from mpisppy_amd.cylinders.xhatxbar_bounder import XhatXbarInnerBound
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.spopt import SPOpt
    plain = SPOpt({"solver_name": "mi355x_pdhg", "verbose": False, "toc": False}, farmer.scenario_names_creator(3),
                  farmer.scenario_creator, scenario_creator_kwargs={"num_scens": 3})
    for cls, name in ((SlamMinHeuristic, "SlamMinHeuristic"), (XhatXbarInnerBound, "XhatXbarInnerBound")):
        with pytest.raises(RuntimeError, match=f"{name} must be used with Xhat_Eval."):
            cls(plain).main()
