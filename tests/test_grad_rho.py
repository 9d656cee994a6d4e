"""The numpy restatement of the gradient-rho tools (tests/grad_rho_ref.py) against the values
the reference pins in mpisppy/tests/test_gradient_rho.py, and the host-side parts of the
package's classes (csv formats, MultRhoUpdater's rule) on stub PH objects.  No GPU.

State of the pinned values: farmer scen0..2, crops_multiplier 1, rho 1, after Iter0 (x̄ = 0 for
the two per-scenario denominators) and then Compute_Xbar (for _grad_denom and compute_rho).
test_find_grad_rho's 0.00079... is NOT pinned: it is computed after find_grad_cost's xhat solve
has moved the scenarios' x, state this restatement (which needs no solve) never has.
"""
import os

import numpy as np
import pytest
import torch

import grad_rho_ref as G
import norm_rho_ref as N

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "rho_test_data")
NAMES = ["DevotedAcreage[CORN0]", "DevotedAcreage[SUGAR_BEETS0]", "DevotedAcreage[WHEAT0]"]


@pytest.fixture(scope="module")
def farmer3():
    """(x, x̄ after compute_xbar, pcoef) of the oracle after Iter0; x̄ = 0 before."""
    st = N.make("farmer3")
    st.iter0()
    o = st.o
    x = o.x.copy()
    assert not o.xbar.any()
    o.compute_xbar()
    return x, o.xbar.copy(), st.pcoef


@pytest.fixture(scope="module")
def fixture_cost():
    c = G.read_cost_csv(os.path.join(DATA, "grad_cost.csv"))
    return np.array([[c[(f"scen{s}", v)] for v in NAMES] for s in range(3)])


def test_new_entries_are_exported_and_refuse_null_handles():
    from mpisppy_amd import _lib
    lib = _lib.load()
    for name in ("phgpu_grad_cost", "phgpu_w_diff", "phgpu_rho_ratio_stats", "phgpu_rho_from_stats"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.phgpu_grad_cost(None, None, None, None) == -1
    assert lib.phgpu_w_diff(None, None, None, None, None) == -1
    assert lib.phgpu_rho_ratio_stats(None, None, None, None, None, None, None) == -1
    assert lib.phgpu_rho_from_stats(None, None, 3, 0.5, None, 0.05, None, None, None) == -1


def test_denominators_at_xbar_zero(farmer3):
    x = farmer3[0]
    zero = np.zeros_like(x)
    assert G.w_denom(x, zero)[0][0] == pytest.approx(25.0, abs=1e-7)          # test_w_denom
    assert G.prox_denom(x, zero)[0][0] == pytest.approx(1250.0, abs=1e-5)     # test_prox_denom


def test_grad_denom(farmer3):
    x, xbar, pcoef = farmer3
    assert G.grad_denom(x, xbar, pcoef)[0] == pytest.approx(21.48148148148148, abs=1e-7)
    # the lower bound 1 / rho_relative_bound takes over where the scenarios agree
    assert np.array_equal(G.grad_denom(xbar, xbar, pcoef, rel_bound=1e3), np.full(3, 1e-3))


def test_order_stat():
    assert G.order_stat([4, 3, 1, 5, 2], 0.4) == 2.6                          # test_order_stat
    lst = [4, 3, 1, 5, 2]
    assert G.order_stat(lst, 0.0) == 1 and G.order_stat(lst, 0.5) == 3 and G.order_stat(lst, 1.0) == 5
    assert G.order_stat(lst, 0.9) == pytest.approx(1 + 0.9 * 2 * 2)


def test_compute_rho_reproduces_the_fixture(farmer3, fixture_cost):
    x, xbar, pcoef = farmer3
    rho = G.read_rho_csv(os.path.join(DATA, "rho.csv"))
    want = np.array([rho[v] for v in NAMES])
    assert want.tolist() == [6.982758620689654, 5.175000000000001, 7.97727272727273]
    got = G.compute_rho(fixture_cost, x, xbar, 0.4, G.grad_denom(x, xbar, pcoef))
    np.testing.assert_allclose(got, want, rtol=1e-7)                          # the oracle's x is exact to ~1e-8
    dep = G.compute_rho(fixture_cost, x, xbar, 0.4)
    assert dep[0] == pytest.approx(0.05230103406621424, rel=1e-7)            # test_compute_rho
    # the scenario-dependent denominator is ONE scalar per scenario: the largest entry of both
    # per-nonant arrays (a per-nonant maximum gives another number)
    per_nonant = np.abs(fixture_cost / np.maximum(G.w_denom(x, xbar), G.prox_denom(x, xbar)))
    assert abs(G.order_stat(per_nonant[:, 0], 0.4) - 0.0523) > 1e-3


def test_planes_carry_the_order_statistic(farmer3, fixture_cost):
    """sum, -min and max per nonant are all _order_stat needs (what the device reduces to)."""
    x, xbar, _ = farmer3
    r = G.ratios(fixture_cost, x, xbar)
    p = G.planes(r)
    from mpisppy_amd.utils.find_rho import order_stat
    for alpha in (0.0, 0.4, 0.5, 0.9, 1.0):
        got = [order_stat(alpha, p[0, k] / 3, -p[1, k], p[2, k]) for k in range(3)]
        np.testing.assert_allclose(got, G.compute_rho(fixture_cost, x, xbar, alpha), rtol=1e-15)


def test_gate():
    assert not G.gate_open(0.0, 1.0) and not G.gate_open(0.0, 0.0) and not G.gate_open(float("nan"), 1.0)
    assert G.gate_open(1.0, 0.951) and not G.gate_open(1.0, 0.949)
    assert G.gate_open(1.0, 1.049) and not G.gate_open(1.0, 1.051)


def test_true_costs_and_the_reference_labels(fixture_cost):
    """The fixture labels CORN with WHEAT's cost: compute_grad indexes the gradient, which is in
    NLP variable order, by nonant position.  The true derivative is FARMER_COST."""
    assert fixture_cost[0].tolist() == [-150.0, -230.0, -260.0]
    assert G.FARMER_COST.tolist() == [-230.0, -260.0, -150.0]
    assert sorted(fixture_cost[0]) == sorted(G.FARMER_COST)
    c, q, xn = np.array([230.0, 260.0, 150.0]), np.array([0.0, 2.0, 0.0]), np.array([1.0, 3.0, 5.0])
    assert G.grad_cost(c, q, xn).tolist() == [-230.0, -266.0, -150.0]


@pytest.mark.parametrize("case", ["farmer3", "farmer1000"])
def test_stepped_oracle_rewrites_where_the_issue_says(case):
    g = G.trajectory(case)
    assert g.applied_iterations() == G.CASES[case]["applied"]
    ratios = [r["ratio"] for r in g.log[1:]]                     # iteration 1: prev = 0, inf
    assert g.log[0]["ratio"] == float("inf")
    assert not any(0.04 <= r <= 0.06 for r in ratios), ratios    # no decision near the threshold
    if case == "farmer1000":
        conv = {r["iter"]: r["conv"] for r in g.log}
        assert len(g.log) == 22 and conv[21] > 1e-3 > conv[22]
    # W_diff equals conv while rho = 1 (W moves by rho (x - x̄))
    first = min(g.applied_iterations())
    for r in g.log[:first]:
        assert r["w_diff"] == pytest.approx(r["conv"], rel=1e-12)


# ---------------------------------------------------------------- the package's host parts
class _Comm:
    def allgather_object(self, obj):
        return [obj]

    def Barrier(self):
        pass


class _Batch:
    nonant_names = NAMES
    nn = 3


class _Engine:
    """What Find_Grad / Find_Rho / MultRhoUpdater touch, on CPU tensors."""
    nn, S, device = 3, 3, torch.device("cpu")
    num_nodes, nlen_max = 1, 3

    def __init__(self, x, xbar):
        self.xh, self.xbarh = x, xbar
        self.xbar = torch.as_tensor(xbar.T.copy())
        self.rho = torch.ones(3, 3, dtype=torch.float64)

    def _flush_xbar(self):
        pass

    _flush_step = _flush_xbar

    def grad_cost(self, xn):
        return torch.as_tensor(np.tile(G.FARMER_COST[:, None], (1, 3))) + 0.0 * xn

    def total_scenarios(self):
        return 3

    def rho_ratio_stats(self, cost, indep_denom, rel_bound):
        assert not indep_denom
        return torch.as_tensor(G.planes(G.ratios(cost.numpy().T, self.xh, self.xbarh))).view(3, 1, 3)


class _PH:
    multistage = False
    cylinder_rank = 0
    mpicomm = _Comm()
    batch = _Batch()
    local_scenario_names = ["scen0", "scen1", "scen2"]
    convobject = None

    def __init__(self, x, xbar, options=None):
        self.engine = _Engine(x, xbar)
        self.options = options or {}


def test_cost_csv_round_trip(farmer3, tmp_path):
    from mpisppy_amd.utils import find_rho, gradient
    x, xbar, _ = farmer3
    # the reader keeps the reference's line[2][:-2] and reads the fixture as the csv module does
    c = find_rho.read_cost_file(os.path.join(DATA, "grad_cost.csv"))
    assert c == G.read_cost_csv(os.path.join(DATA, "grad_cost.csv")) and len(c) == 9
    fn = str(tmp_path / "cost.csv")
    cfg = {"grad_cost_file": fn, "order_stat": 0.4}
    fg = gradient.Find_Grad(_PH(x, xbar), cfg)
    fg.write_grad_cost()
    assert open(fn, newline="").read().startswith("#grad cost values\r\nscen0,DevotedAcreage[CORN0],-230.0\r\n")
    back = find_rho.read_cost_file(fn)
    assert back == fg.c and back[("scen2", NAMES[2])] == -150.0
    # a value whose repr does not end in ".0" survives too (the two characters cut are "\r\n")
    with open(fn, "a") as f:
        import csv
        csv.writer(f).writerow(["scen9", "v", str(-0.1234567890123)])
    assert find_rho.read_cost_file(fn)[("scen9", "v")] == -0.1234567890123


def test_rho_csv_round_trip_and_setter(farmer3, fixture_cost, tmp_path):
    from mpisppy_amd.utils import find_rho
    x, xbar, _ = farmer3
    fn = str(tmp_path / "rho.csv")
    cfg = {"whatpath": os.path.join(DATA, "grad_cost.csv"), "rho_file": fn, "order_stat": 0.4}
    fr = find_rho.Find_Rho(_PH(x, xbar), cfg)
    rho = fr.compute_rho()
    np.testing.assert_allclose([rho[v] for v in NAMES], G.compute_rho(fixture_cost, x, xbar, 0.4), rtol=1e-14)
    fr.write_rho()
    assert find_rho.read_rho_file(fn) == rho == G.read_rho_csv(fn)
    assert find_rho.read_rho_file(os.path.join(DATA, "rho.csv")) == G.read_rho_csv(os.path.join(DATA, "rho.csv"))
    assert fr._order_stat([4, 3, 1, 5, 2]) == 2.6

    # Set_Rho.rho_setter on a scenario with the farmer's nonant names (test_rho_setter)
    class V:
        def __init__(self, name):
            self.name = name

    class Node:
        nonant_vardata_list = [V(n) for n in NAMES]

    class Scen:
        _mpisppy_node_list = [Node()]

    lst = find_rho.Set_Rho({"rho_path": os.path.join(DATA, "rho.csv")}).rho_setter(Scen())
    assert len(lst) == 3 and lst[0] == (id(Node.nonant_vardata_list[0]), 6.982758620689654)
    with pytest.raises(RuntimeError, match="not found in the scenario"):
        Node.nonant_vardata_list = Node.nonant_vardata_list[:2]
        find_rho.Set_Rho({"rho_path": os.path.join(DATA, "rho.csv")}).rho_setter(Scen())


def test_xhat_sources(farmer3):
    from mpisppy_amd.utils import gradient
    x, xbar, _ = farmer3
    want = np.load(os.path.join(DATA, "farmer_cyl_nonants.npy"))
    for cfg in ({"xhatpath": os.path.join(DATA, "farmer_cyl_nonants.npy")}, {"xhat": want}, {"xhat": {"ROOT": want}}):
        v = gradient.Find_Grad(_PH(x, xbar), cfg)._xhat_dev()
        assert tuple(v.shape) == (3, 3) and np.array_equal(v.numpy(), np.tile(want[:, None], (1, 3)))
    assert np.array_equal(gradient.Find_Grad(_PH(x, xbar), {})._xhat_dev().numpy(), xbar.T)   # default: x̄
    with pytest.raises(RuntimeError, match="Could not find file"):
        gradient.Find_Grad(_PH(x, xbar), {"xhatpath": "/nonexistent.npy"})._xhat_dev()


def test_mult_rho_rule_on_a_made_up_sequence(farmer3):
    """best-so-far, the start / stop iterations and conv == 0, package class against the
    restatement (mult_rho_updater.py:78-100)."""
    from mpisppy_amd.extensions.mult_rho_updater import MultRhoUpdater
    x, xbar, _ = farmer3
    #        it:  1    2    3    4    5    6    7    8    9
    convs = [9.0, 4.0, 2.0, 3.0, 2.0, 1.0, 0.0, 0.5, 0.25]
    for opts, acted in (({}, [2, 3, 6]),                       # 1 attaches; 4, 5 no new best; 7: conv == 0
                        ({"rho_update_start_iteration": 3}, [6]),          # 3 attaches
                        ({"rho_update_stop_iteration": 3}, [2, 3])):
        ph = _PH(x, xbar, {"mult_rho_options": opts})
        ph.engine.rho = torch.tensor([[1.0, 2.0, 3.0]] * 3, dtype=torch.float64).T.contiguous()
        ext = MultRhoUpdater(ph)
        ref = G.MultRho(ph.engine.rho.numpy().T.copy(), start=opts.get("rho_update_start_iteration"),
                        stop=opts.get("rho_update_stop_iteration"))
        for it, conv in enumerate(convs, 1):
            ph._PHIter, ph.conv = it, conv
            ext.miditer()
            ref.miditer(it, conv)
            np.testing.assert_allclose(ph.engine.rho.numpy().T, ref.rho, rtol=1e-15)
        assert ext.acted == ref.acted == acted
        assert ext.best_conv == ref.best == (2.0 if "rho_update_stop_iteration" in opts else 0.0)
    # conv equal to the tolerance at the first new best attaches nothing (:56)
    ph = _PH(x, xbar, {"mult_rho_options": {"convergence_tolerance": 9.0}})
    ext = MultRhoUpdater(ph)
    ph._PHIter, ph.conv = 1, 9.0
    ext.miditer()
    assert ext._first_rho is None and ext.best_conv == 9.0
