"""The Fixer's rule, tuples and options on the CPU (tests/fixer_ref.py is the numpy restatement
of mpisppy/extensions/fixer.py the GPU tests compare the device with):

* a decision table of hand-written cases against ``fixer_ref.rule``;
* ``Fixer_tuple``'s warnings, ``Fixer.populate``'s threshold and lag variation errors,
  ``uniform_fix_list_fct`` and ``cfg_vanilla.add_fixer``;
* the exported ``phgpu_fixer_step`` and its argtypes;
* the three trajectories tests/test_gpu_fixer.py runs on the device: the fixing the
  reference's rule gives, and every counter decision at least 10 % (relative, |diff| against
  th²) away from flipping -- a condition on the inputs that keeps a 1e-5 error in x from
  changing a decision.
"""
import ctypes
import types

import numpy as np
import pytest

import fixer_ref as F

NAN = float("nan")
NONE = -1


def _one(iter0, xb, diff, th=2.0, nb=NONE, lb=NONE, ub=NONE, l=0.0, u=100.0, bt=0.5, count=0, fixval=NAN):
    """The rule for one entry with xsq = xb² - diff: (count, fixval, newly fixed)."""
    c, fv, new, _ = F.rule(iter0, np.array([xb]), np.array([xb * xb - diff]), th, nb, lb, ub, np.array([l]),
                           np.array([u]), bt, np.array([count]), np.array([fixval]))
    return int(c[0]), float(fv[0]), bool(new[0])


# (iter0, kwargs) -> (count, fixval or None for NaN, newly fixed); th = 2 so th² = 4, boundtol 0.5
TABLE = [
    # iter0: non-strict convergence (|diff| == th² is converged), counters untouched
    ((True, dict(xb=8.0, diff=4.0, nb=0, count=3)), (3, 8.0, True)),
    ((True, dict(xb=8.0, diff=-4.0, nb=5)), (0, 8.0, True)),             # the lag's value is not tested
    ((True, dict(xb=8.0, diff=4.5, nb=0)), (0, None, False)),
    ((True, dict(xb=8.0, diff=-4.5, nb=0)), (0, None, False)),
    ((True, dict(xb=8.0, diff=0.0)), (0, None, False)),                  # all lags None
    ((True, dict(xb=0.25, diff=0.0, lb=7)), (0, 0.0, True)),             # on the lower bound
    ((True, dict(xb=0.5, diff=0.0, lb=7)), (0, None, False)),            # xb - l < boundtol is strict
    ((True, dict(xb=99.75, diff=0.0, ub=0)), (0, 100.0, True)),
    ((True, dict(xb=99.5, diff=0.0, ub=0)), (0, None, False)),
    ((True, dict(xb=0.25, diff=0.0, nb=0, lb=0)), (0, 0.25, True)),      # branch order: nb first
    ((True, dict(xb=0.25, diff=0.0, lb=0, ub=0, u=0.5)), (0, 0.0, True)),   # then lb before ub
    # iterk: strict convergence, the counter first
    ((False, dict(xb=8.0, diff=4.0, nb=0, count=3)), (0, None, False)),  # |diff| == th² resets
    ((False, dict(xb=8.0, diff=-4.0, nb=0, count=3)), (0, None, False)),
    ((False, dict(xb=8.0, diff=2.0, nb=3, count=1)), (2, None, False)),
    ((False, dict(xb=8.0, diff=2.0, nb=3, count=2)), (3, 8.0, True)),    # nb <= count
    ((False, dict(xb=0.25, diff=2.0, lb=3, count=2)), (3, None, False)),  # lb < count is strict
    ((False, dict(xb=0.25, diff=2.0, lb=3, count=3)), (4, 0.0, True)),
    ((False, dict(xb=99.75, diff=2.0, ub=3, count=2)), (3, None, False)),
    ((False, dict(xb=99.75, diff=2.0, ub=3, count=3)), (4, 100.0, True)),
    ((False, dict(xb=8.0, diff=2.0, nb=0, count=0)), (1, 8.0, True)),    # lag 0: at the first hit
    ((False, dict(xb=0.25, diff=2.0, lb=0, count=0)), (1, 0.0, True)),   # 0 < 1
    ((False, dict(xb=8.0, diff=5.0, nb=0, count=0)), (0, None, False)),  # count 0: nothing, even with lag 0
    ((False, dict(xb=8.0, diff=2.0, count=7)), (8, None, False)),        # None lags never fix
    ((False, dict(xb=0.25, diff=2.0, nb=9, lb=1, count=4)), (5, 0.0, True)),     # nb not due: lb takes it
    ((False, dict(xb=0.25, diff=2.0, nb=5, lb=1, count=4)), (5, 0.25, True)),    # nb due: first branch
    ((False, dict(xb=0.5, diff=2.0, lb=0, ub=0, u=0.75, count=4)), (5, 0.75, True)),   # lb not near, ub near
    # skipped entries: fixed before, or fixed in the model; the counter is left alone
    ((False, dict(xb=8.0, diff=0.0, nb=0, count=2, fixval=3.0)), (2, 3.0, False)),
    ((False, dict(xb=8.0, diff=9.0, nb=0, count=2, fixval=3.0)), (2, 3.0, False)),
    ((False, dict(xb=8.0, diff=0.0, nb=0, count=2, l=8.0, u=8.0)), (2, None, False)),
    ((True, dict(xb=8.0, diff=0.0, nb=0, fixval=3.0)), (0, 3.0, False)),
    # clipping to the model bounds
    ((False, dict(xb=120.0, diff=0.0, nb=0)), (1, 100.0, True)),
    ((True, dict(xb=-3.0, diff=0.0, nb=0)), (0, 0.0, True)),
]


@pytest.mark.parametrize("case,want", TABLE)
def test_decision_table(case, want):
    iter0, kw = case
    c, fv, new = _one(iter0, **kw)
    assert (c, new) == (want[0], want[2])
    assert (np.isnan(fv) and want[1] is None) or fv == want[1]


def test_arrival_and_no_tuple():
    """Entries skipped at iter0 are the ones fixed on arrival; th = 0 with no lag (a nonant
    without a tuple) is never counted or fixed."""
    l = np.array([0.0, 5.0, 0.0])
    u = np.array([9.0, 5.0, 9.0])
    fv = np.array([NAN, NAN, 2.0])
    _, _, new, arrived = F.rule(True, np.full(3, 5.0), np.full(3, 25.0), 1.0, 0, NONE, NONE, l, u, 0.5,
                                np.zeros(3, int), fv)
    assert new.tolist() == [True, False, False] and arrived.tolist() == [False, True, True]
    c, fv, new, arrived = F.rule(False, np.full(3, 5.0), np.full(3, 25.0), 0.0, NONE, NONE, NONE, 0.0, 9.0, 0.5,
                                 np.zeros(3, int), np.full(3, NAN))
    assert not new.any() and not arrived.any() and c.tolist() == [0, 0, 0]


# ------------------------------------------------------------------ tuples and options
def test_fixer_tuple_warnings(capsys):
    from mpisppy_amd.extensions.fixer import Fixer_tuple
    v = types.SimpleNamespace(name="x[1]")
    assert Fixer_tuple(v) == (id(v), 0, None, None, None)
    assert "but no arguments were given" in capsys.readouterr().out
    assert Fixer_tuple(v, th=2.0, nb=1, lb=3, ub=4) == (id(v), 2.0, 1, 3, 4)
    out = capsys.readouterr().out
    assert "with nb < lb, which means lb will be ignored" in out and "with nb < ub, which means ub will be" in out
    assert Fixer_tuple(v, th=2.0, nb=3, lb=3, ub=0) == (id(v), 2.0, 3, 3, 0)
    assert capsys.readouterr().out == ""


def _fake_ph(S=3, fct=None, **fixeroptions):
    from mpisppy_amd.batch import batch_from_models
    from mpisppy_amd.examples import farmer
    names = farmer.scenario_names_creator(S)
    models = [farmer.scenario_creator(n, num_scens=S) for n in names]
    fo = dict({"verbose": False, "boundtol": 0.01, "id_fix_list_fct": fct}, **fixeroptions)
    return types.SimpleNamespace(cylinder_rank=0, batch=batch_from_models(names, models),
                                 options={"verbose": False, "display_progress": False, "fixeroptions": fo},
                                 local_scenarios=dict(zip(names, models)), local_scenario_names=names)


def test_populate_resolves_ids_and_rejects_variation(capsys):
    from mpisppy_amd.extensions.fixer import Fixer, Fixer_tuple, uniform_fix_list_fct
    ph = _fake_ph(fct=uniform_fix_list_fct(10.0, nb=3, lb=1, iter0={"th": 5.0, "ub": 0}))
    fx = Fixer(ph)
    assert fx.miditer_on_device
    fx.populate(ph.local_scenarios)
    th, nb, lb, ub = fx._arrays["iterk"]
    assert th.tolist() == [10.0] * 3 and nb.tolist() == [3] * 3 and lb.tolist() == [1] * 3 and ub.tolist() == [-1] * 3
    th, nb, lb, ub = fx._arrays["iter0"]
    assert th.tolist() == [5.0] * 3 and nb.tolist() == [-1] * 3 and ub.tolist() == [0] * 3

    def nonants(s):
        return [v for nd in s._mpisppy_node_list for v in nd.nonant_vardata_list]

    # one nonant only: the others have no tuple (th 0, no lag)
    def second_only(s):
        return [], [Fixer_tuple(nonants(s)[1], th=4.0, nb=0)]
    fx = Fixer(_fake_ph(fct=second_only))
    fx.populate(fx.ph.local_scenarios)
    assert fx._arrays["iterk"][0].tolist() == [0.0, 4.0, 0.0] and fx._arrays["iterk"][1].tolist() == [-1, 0, -1]

    def vary_th(s):
        t = 4.0 if s.name == "scen1" else 3.0
        return [Fixer_tuple(v, th=3.0) for v in nonants(s)], [Fixer_tuple(v, th=t, nb=1) for v in nonants(s)]
    fx = Fixer(_fake_ph(fct=vary_th))
    with pytest.raises(RuntimeError, match="Attempt to vary fixer threshold across scenarios"):
        fx.populate(fx.ph.local_scenarios)

    def vary_th0(s):
        t = 4.0 if s.name == "scen2" else 3.0
        return [Fixer_tuple(v, th=t) for v in nonants(s)], [Fixer_tuple(v, th=3.0, nb=1) for v in nonants(s)]
    fx = Fixer(_fake_ph(fct=vary_th0))
    with pytest.raises(RuntimeError, match="Attempt to vary iter0 fixer threshold across scenarios"):
        fx.populate(fx.ph.local_scenarios)

    def vary_lag(s):
        n = 2 if s.name == "scen1" else 1
        return [Fixer_tuple(v, th=3.0) for v in nonants(s)], [Fixer_tuple(v, th=3.0, nb=n) for v in nonants(s)]
    fx = Fixer(_fake_ph(fct=vary_lag))
    with pytest.raises(ValueError, match="lags"):
        fx.populate(fx.ph.local_scenarios)

    def not_nonant(s):
        return [], [Fixer_tuple(s.vars[-1], th=3.0, nb=1)]
    fx = Fixer(_fake_ph(fct=not_nonant))
    with pytest.raises(KeyError):
        fx.populate(fx.ph.local_scenarios)
    assert "Are you trying to fix a Var that is not nonant?" in capsys.readouterr().out

    # None tuples for a scenario: nothing is populated for that kind (miditer warns)
    fx = Fixer(_fake_ph(fct=lambda s: (None, [Fixer_tuple(v, th=3.0, nb=1) for v in nonants(s)])))
    fx.populate(fx.ph.local_scenarios)
    assert fx._arrays["iter0"] is None and fx._arrays["iterk"] is not None


def test_fix_arrays_and_progress_options():
    from mpisppy_amd.extensions.fixer import Fixer
    ph = _fake_ph(fix_arrays={"iter0": None, "iterk": {"th": [1.0, 2.0, 3.0], "nb": [None, 0, 4], "ub": [2, -1, None]}})
    ph.local_scenarios = {}
    fx = Fixer(ph)
    fx.populate(ph.local_scenarios)
    assert fx._arrays["iter0"] is None
    th, nb, lb, ub = fx._arrays["iterk"]
    assert th.tolist() == [1.0, 2.0, 3.0] and nb.tolist() == [-1, 0, 4] and lb.tolist() == [-1] * 3
    assert ub.tolist() == [2, -1, -1]
    ph.options["fixeroptions"]["fix_arrays"] = {"iterk": {"th": [1.0, 2.0]}}
    with pytest.raises(ValueError, match="length 3"):
        Fixer(ph).populate({})
    del ph.options["fixeroptions"]["fix_arrays"]
    with pytest.raises(RuntimeError, match="fix_arrays"):
        Fixer(ph).populate({})
    for key, where in (("display_progress", ph.options), ("verbose", ph.options),
                       ("verbose", ph.options["fixeroptions"])):
        where[key] = True
        assert not Fixer(ph).miditer_on_device            # the progress line reads the totals back
        where[key] = False


def test_add_fixer_wires_the_hub():
    from mpisppy_amd.extensions.fixer import Fixer
    from mpisppy_amd.extensions.extension import MultiExtension
    from mpisppy_amd.extensions.norm_rho_updater import NormRhoUpdater
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    fct = object()
    cfg = types.SimpleNamespace(fixer_tol=1e-3, id_fix_list_fct=fct)
    hub = vanilla.add_fixer({"opt_kwargs": {"options": {}}}, cfg)
    assert hub["opt_kwargs"]["extensions"] is Fixer
    assert hub["opt_kwargs"]["options"]["fixeroptions"] == {"verbose": False, "boundtol": 1e-3, "id_fix_list_fct": fct}
    hub = vanilla.add_fixer({"opt_kwargs": {"options": {}, "extensions": NormRhoUpdater}}, cfg)
    assert hub["opt_kwargs"]["extensions"] is MultiExtension
    assert hub["opt_kwargs"]["extension_kwargs"]["ext_classes"] == [NormRhoUpdater, Fixer]


# ------------------------------------------------------------------ the C-ABI
def test_fixer_step_is_exported_and_typed():
    from mpisppy_amd import _lib
    assert "phgpu_fixer_step" in _lib.EXPORTS
    L = _lib.load()
    f = L.phgpu_fixer_step
    assert f.restype is ctypes.c_int and len(f.argtypes) == 12
    assert f.argtypes[1]._type_ is _lib.FixerParams and all(a is ctypes.c_void_p for a in f.argtypes[2:])
    assert [n for n, _ in _lib.FixerParams._fields_] == ["boundtol", "iter0"]
    assert ctypes.sizeof(_lib.FixerParams) == 16
    assert f(None, None, *([None] * 10)) != 0 and "null argument" in _lib.last_error()


# ------------------------------------------------------------------ the trajectories
@pytest.mark.parametrize("case", list(F.CASES))
def test_trajectory_fixes_where_the_reference_rule_does_and_keeps_clear_of_the_threshold(case):
    o = F.trajectory(case)
    got = {r["iter"]: int(r["nfix"].sum()) for r in o.log if r["nfix"].sum()}
    margin = min(r["margin"] for r in o.log)
    print(case, "fixing", got, "smallest margin", margin, "totals", o.totals.tolist())
    assert got == F.CASES[case]["fixed"]
    assert margin >= 0.1
    assert o.totals.tolist() == [sum(got.values()), 0, 0]
    # every call fixed whole node entries, and a fixed entry holds x there from then on
    nloc = np.bincount(o.key.ravel(), minlength=o.nkeys)
    for r in o.log:
        assert ((r["nfix"] == 0) | (r["nfix"] == nloc)).all()
    fixed = ~np.isnan(o.fixval)
    assert np.abs(o.x[fixed] - o.fixval[fixed]).max() == 0.0
