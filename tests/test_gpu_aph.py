"""APH's device passes (phgpu_aph_*, phgpu_select_smallest, phgpu_solve_list; include/phgpu.h)
against numpy.

* the passes alone from constructed inputs (farmer S = 130: three waves, the last ragged;
  aircond [4, 3, 2]: waves span nodes; the same batch on a shared-matrix handle): first and not
  first, a partial mask, an all-zero mask, rho differing per nonant, the lagged copies, variable
  probabilities.  Element-wise results at 1e-12 max(1, |value|); every sum within 1e-12 of the
  sum of its summands' magnitudes (what reordering can cost at these sizes); theta = 0 when
  tau <= 0 or phi <= 0; the same bits twice;
* the selection against Python's stable sort, exactly;
* the list solve against a full solve from the same state.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

AIR_KW = {"start_seed": 1134}
EL = 1e-12


def _engine(model, S=130, cm=1):
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.examples import aircond, farmer
    if model == "farmer":
        b = farmer.batch_creator(farmer.scenario_names_creator(S), crops_multiplier=cm, num_scens=S)
    else:
        b = aircond.batch_creator(aircond.scenario_names_creator(24), branching_factors=[4, 3, 2], **AIR_KW)
    return PHEngine(b, device="cuda:0", shared=True if model == "aircond_shared" else None)


def _put(t, a):
    t[:a.shape[0]].copy_(torch.as_tensor(np.ascontiguousarray(a), dtype=t.dtype, device=t.device))


def _get(t, rows=None):
    a = t.cpu().numpy()
    return a if rows is None else a[:rows]


def _close(got, want):
    return np.abs(got - want) <= EL * np.maximum(1.0, np.abs(want))


class Tree:
    """The node entry of every (nonant, scenario) and the probabilities, on the host."""

    def __init__(self, e, pvar=None):
        b = e.batch
        d = np.asarray(b.nonant_depth)
        self.idx = e.node_of.cpu().numpy()[d].astype(np.int64) * e.nlen_max + np.asarray(b.nonant_off)[:, None]
        self.pc = np.asarray(b.prob_coeff, dtype=float).T[d] if pvar is None else np.asarray(pvar, dtype=float).T
        self.p = np.asarray(b.prob, dtype=float)
        self.half = e.num_nodes * e.nlen_max

    def plane(self, v):
        """(sums, sums of magnitudes) of v [nn, S] per node entry."""
        a, m = np.zeros(self.half), np.zeros(self.half)
        np.add.at(a, self.idx, v)
        np.add.at(m, self.idx, np.abs(v))
        return a, m


def _set_x(e, xn):
    e.x.zero_()
    e.x[torch.as_tensor(np.asarray(e.batch.nonant_col), device=e.device)] = torch.as_tensor(xn, device=e.device)


def _masks(S, rng):
    part = (rng.random(S) < 0.4).astype(np.int32)
    part[0], part[S - 1] = 1, 0
    return {"all": None, "part": part, "none": np.zeros(S, dtype=np.int32)}


def _run_passes(e, tree, first, mask, use_lag, red_kind, seed, gamma=2.0, nu=1.5):
    """One reduce / norms / update / mark sequence from inputs drawn with ``seed``; everything
    checked against numpy, the device results returned as bytes."""
    rng = np.random.default_rng(seed)
    nn, S = e.nn, e.S
    xn = rng.integers(0, 6, size=(nn, S)).astype(float) * 40.0 + rng.random((nn, S))
    W, z = rng.normal(size=(nn, S)) * 20.0, rng.random((nn, S)) * 200.0
    Wl, zl = rng.normal(size=(nn, S)) * 20.0, rng.random((nn, S)) * 200.0
    y0 = rng.normal(size=(nn, S)) * 30.0
    rho = (0.5 + 0.25 * np.arange(nn))[:, None] * np.ones((1, S))
    e.aph_init(use_lag=use_lag)
    _set_x(e, xn)
    _put(e.W, W), _put(e.aph_z, z), _put(e.rho, rho), _put(e.aph_y, y0)
    if use_lag:
        _put(e.aph_W_lag, Wl), _put(e.aph_z_lag, zl)
    mdev = None if mask is None else torch.as_tensor(mask, device=e.device)
    # ---- reduce
    e.aph_reduce(first, mdev)
    Wu, zu = (Wl, zl) if use_lag else (W, z)
    sel = np.ones(S, bool) if mask is None else mask.astype(bool)
    y = np.zeros((nn, S)) if first else np.where(sel[None, :], Wu + rho * (xn - zu), y0)
    yd = _get(e.aph_y, nn)
    assert _close(yd, y).all()
    if not first and mask is not None:
        assert (yd[:, ~sel] == y0[:, ~sel]).all()              # the other scenarios keep y, bit for bit
    planes = _get(e.aph_planes).reshape(3, tree.half)
    for j, v in enumerate((tree.pc * xn, tree.pc * xn * xn, tree.pc * yd)):
        a, m = tree.plane(v)
        assert (np.abs(planes[j] - a) <= EL * m).all(), (j, np.abs(planes[j] - a).max())
    # ---- norms
    e.aph_norms(gamma)
    xb, yb = planes[0][tree.idx], planes[2][tree.idx]
    u = xn - xb
    assert (_get(e.xbar, nn) == xb).all() and _close(_get(e.aph_u, nn), u).all()
    ud = _get(e.aph_u, nn)
    phi = tree.p * ((z - xn) * (W - yd)).sum(0)
    phim = tree.p * np.abs((z - xn) * (W - yd)).sum(0)
    assert (np.abs(_get(e.aph_phi) - phi) <= EL * np.maximum(1.0, phim)).all()
    usq, vsq = (u * u).sum(0), (yb * yb).sum(0)
    red = _get(e.aph_red)
    for j, (v, m) in enumerate(((tree.p * (usq + vsq / gamma), None), (phi, phim), (tree.p * usq, None),
                                (tree.p * vsq, None))):
        m = np.abs(v) if m is None else m
        assert abs(red[j] - v.sum()) <= EL * m.sum(), (j, red[j], v.sum())
    assert red[4] == 0.0 and red[5] == 0.0                      # no update yet: no W / z norms to send
    # ---- update
    if red_kind == "tau0":
        e.aph_red[0] = 0.0
    elif red_kind == "phineg":
        e.aph_red[1] = -abs(red[1]) - 1.0
    elif red_kind == "pos":
        e.aph_red[0], e.aph_red[1] = 3.0e5, 7.0e4
    tau, gphi = (float(v) for v in _get(e.aph_red)[:2])
    theta = gphi * nu / tau if (tau > 0 and gphi > 0) else 0.0
    if red_kind in ("tau0", "phineg"):
        assert theta == 0.0
    e.aph_update(first, nu, gamma)
    (pw, pz, th, phs), _ = e.aph_scalars()
    assert th == theta or abs(th - theta) <= EL * abs(theta)
    Wn = W + th * ud
    zn = xb if first else z + th * yb / gamma
    assert _close(_get(e.W, nn), Wn).all() and _close(_get(e.aph_z, nn), zn).all()
    Wd, zd = _get(e.W, nn), _get(e.aph_z, nn)
    phi2 = tree.p * ((zd - xn) * (Wd - yd)).sum(0)
    phi2m = tree.p * np.abs((zd - xn) * (Wd - yd)).sum(0)
    assert (np.abs(_get(e.aph_phi) - phi2) <= EL * np.maximum(1.0, phi2m)).all()
    for got, v, m in ((pw, tree.p * (Wd * Wd).sum(0), None), (pz, tree.p * (zd * zd).sum(0), None),
                      (phs, phi2, phi2m)):
        m = np.abs(v) if m is None else m
        assert abs(got - v.sum()) <= EL * m.sum(), (got, v.sum())
    # ---- mark, both orders
    mk = (rng.random(S) < 0.5).astype(np.int32)
    li0 = rng.integers(0, 9, size=S).astype(np.int32)
    lp0 = rng.normal(size=S)
    out = [yd.tobytes(), planes.tobytes(), red.tobytes(), Wd.tobytes(), zd.tobytes(),
           np.array([pw, pz, th, phs]).tobytes(), _get(e.aph_phi).tobytes()]
    for rr, shelf in ((False, 4), (True, 4)):
        _put(e.aph_mask, mk), _put(e.aph_last_iter, li0), _put(e.aph_last_phi, lp0)
        e.aph_mark(6, shelf, rr)
        li = np.where(mk == 1, 6, li0)
        assert (_get(e.aph_last_iter) == li).all()
        assert (_get(e.aph_last_phi) == np.where(mk == 1, _get(e.aph_phi), lp0)).all()
        k1 = li.astype(float) if rr else -np.maximum(li, shelf - 1).astype(float)
        assert (_get(e.aph_k1) == k1).all()
        if use_lag:                                            # W and z as of the last dispatch
            m2 = (mk == 1)[None, :]
            assert (_get(e.aph_W_lag, nn) == np.where(m2, Wd, Wl)).all()
            assert (_get(e.aph_z_lag, nn) == np.where(m2, zd, zl)).all()
            _put(e.aph_W_lag, Wl), _put(e.aph_z_lag, zl)
    return out


@pytest.mark.parametrize("model", ["farmer", "aircond", "aircond_shared"])
def test_passes_against_numpy(gpu, model):
    e = _engine(model)
    try:
        tree = Tree(e)
        ws0 = e.workspace_bytes()
        masks = _masks(e.S, np.random.default_rng(5))
        cases = [(True, "all", False, "as_is"), (False, "all", False, "pos"), (False, "part", False, "pos"),
                 (False, "none", False, "tau0"), (False, "part", True, "phineg"), (True, "part", True, "pos")]
        for ci, (first, mk, lag, rk) in enumerate(cases):
            a = _run_passes(e, tree, first, masks[mk], lag, rk, 300 + ci)
            b = _run_passes(e, tree, first, masks[mk], lag, rk, 300 + ci)
            assert a == b, "the passes gave other bits on the second run"
        assert e.workspace_bytes() > ws0                        # the passes' workspaces are counted
        # variable probabilities: the node sums use pvar, the scalar sums the scenario probabilities
        pv = np.asarray(e.batch.prob_coeff, dtype=float)[:, np.asarray(e.batch.nonant_depth)].copy()
        pv[::3, 0] *= 0.5
        pv[1::4, e.nn - 1] = 0.0
        e.set_nonant_probs(pv)
        _run_passes(e, Tree(e, pvar=pv), False, masks["part"], False, "pos", 400)
        e.set_nonant_probs(None)
    finally:
        e.close()


# ------------------------------------------------------------------ the selection
def _key_sets(S, rng):
    d = rng.normal(size=S) * 1e3
    two = np.where(rng.random(S) < 0.5, -3.0, 7.5)
    heavy1, heavy2 = rng.integers(0, 3, size=S).astype(float), rng.integers(-2, 2, size=S).astype(float) * 0.25
    zeros = np.where(rng.random(S) < 0.5, -0.0, 0.0)
    signs = rng.integers(-2, 3, size=S).astype(float) * np.where(rng.random(S) < 0.5, 1e-300, 1e300)
    signs = np.where(signs == 0.0, zeros, signs)
    return {"distinct": (rng.permutation(S).astype(float) - S / 2, d),
            "distinct_k2_only": (None, d),
            "two_values": (two, d),
            "all_equal": (np.full(S, 2.0), np.full(S, -1.0)),
            "heavy_ties": (heavy1, heavy2),
            "zeros_and_signs": (zeros[::-1].copy(), signs)}


@pytest.mark.parametrize("S", [1, 64, 65, 130, 5000])
def test_select_smallest_is_the_stable_sort(gpu, S):
    e = _engine("farmer", S=S)
    try:
        rng = np.random.default_rng(1000 + S)
        k1d = torch.zeros(S, dtype=torch.float64, device=e.device)
        k2d = torch.zeros(S, dtype=torch.float64, device=e.device)
        mask = torch.zeros(S, dtype=torch.int32, device=e.device)
        lst = torch.zeros(S, dtype=torch.int32, device=e.device)
        for name, (k1, k2) in _key_sets(S, rng).items():
            a1 = np.zeros(S) if k1 is None else k1
            order = sorted(range(S), key=lambda s: (a1[s], k2[s], s))
            if k1 is not None:
                k1d.copy_(torch.as_tensor(k1))
            k2d.copy_(torch.as_tensor(k2))
            for count in sorted({c for c in (1, 33, S - 1, S) if 1 <= c <= S}):
                want = sorted(order[:count])
                res = []
                for _ in range(2):
                    mask.fill_(-5), lst.fill_(-5)
                    e.select_smallest(None if k1 is None else k1d, k2d, count, mask, lst)
                    res.append((mask.cpu().numpy().copy(), lst.cpu().numpy().copy()))
                m, li = res[0]
                assert li[:count].tolist() == want, (name, S, count)
                assert (li[count:] == -5).all()
                wm = np.zeros(S, dtype=np.int32)
                wm[want] = 1
                assert (m == wm).all(), (name, S, count)
                assert (res[1][0] == m).all() and (res[1][1] == li).all()
        with pytest.raises(Exception):
            e.select_smallest(None, k2d, 0, mask, lst)
        with pytest.raises(Exception):
            e.select_smallest(None, k2d, S + 1, mask, lst)
    finally:
        e.close()


# ------------------------------------------------------------------ the list solve
def _ph_state(e):
    """A PH-like state after a cold solve: x̄ near the solution's mean, W small, rho per nonant."""
    nn, S = e.nn, e.S
    xn = e.nonant_x_dev().cpu().numpy()[:nn]
    xbar = np.repeat(xn.mean(1, keepdims=True), S, 1)
    rho = (1.0 + 0.5 * np.arange(nn) % 3)[:, None] * np.ones((1, S))
    W = rho * (xn - xbar) * 0.5
    _put(e.W, W), _put(e.rho, rho), _put(e.xbar, xbar)
    e.set_terms(True, True)


def _outs(e):
    return {k: getattr(e, k).cpu().numpy().copy() for k in ("x", "obj", "bound", "status", "iters")}


def _agree(e, a, b, idx):
    cols = np.asarray(e.batch.nonant_col)
    xa, xb = a["x"][cols][:, idx], b["x"][cols][:, idx]
    assert (np.abs(xa - xb) <= 1e-5 * np.maximum(1.0, np.abs(xb))).all(), np.abs(xa - xb).max()
    for k in ("obj", "bound"):
        assert (np.abs(a[k][idx] - b[k][idx]) <= 1e-5 * np.abs(b[k][idx])).all(), k


@pytest.mark.parametrize("cm,pdhg", [(1, False), (10, False), (10, True)])
def test_solve_list_against_the_full_solve(gpu, monkeypatch, cm, pdhg):
    """Farmer 130 with the PH terms on: on the handle's default path (6 for both patterns, the
    list solve on path 5 of that module) and, for cm = 10, with the interior point taken out of
    the automatic choice, so that the full solves run on the handle's PDHG path and the list
    solve on k_solve."""
    S = 130
    if pdhg:
        monkeypatch.setenv("PHGPU_IPM", "0")
    ea, eb = _engine("farmer", S=S, cm=cm), _engine("farmer", S=S, cm=cm)
    try:
        assert (ea.kernel_info()["path"] != 6) == pdhg
        rng = np.random.default_rng(77)
        lst = np.sort(rng.choice(S, size=41, replace=False)).astype(np.int32)
        lst[0], lst[-1] = 0, S - 1
        lst = np.unique(lst)
        rest = np.setdiff1d(np.arange(S), lst)
        for e in (ea, eb):
            e.solve(warm=False)
            _ph_state(e)
        before = _outs(eb)
        ea.solve(warm=True)
        full = _outs(ea)
        ld = torch.as_tensor(lst, device=eb.device)
        assert eb.solve_list(ld, 0) == 0                          # an empty list launches nothing
        assert all((_outs(eb)[k] == before[k]).all() for k in before)
        assert eb.solve_list(ld, len(lst)) == 0
        part = _outs(eb)
        _agree(eb, part, full, lst)
        for k in before:                                          # the unlisted entries: bit for bit
            assert (part[k][..., rest] == before[k][..., rest]).all(), k
        assert (part["status"][lst] == 0).all()
        eb.solve(warm=True)                                       # a following full warm solve
        _agree(eb, _outs(eb), full, np.arange(S))
        # the full list
        al = torch.arange(S, dtype=torch.int32, device=eb.device)
        assert eb.solve_list(al, S) == 0
        _agree(eb, _outs(eb), full, np.arange(S))
    finally:
        ea.close()
        eb.close()


def test_solve_list_on_a_shared_matrix_handle(gpu):
    e = _engine("aircond_shared")
    try:
        e.solve(warm=False)
        ld = torch.arange(4, dtype=torch.int32, device=e.device)
        assert e.solve_list(ld, 4) == -3
        assert e.solve_list(ld, 0) == 0
    finally:
        e.close()
