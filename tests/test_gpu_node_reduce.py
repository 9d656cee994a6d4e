"""The PH-side reductions of csrc/ph_reduce.inc through the C ABI alone, on seeded synthetic
device arrays (magnitudes over nine decades, mixed signs), without a solve: phgpu_ph_reduce,
phgpu_ph_residuals, phgpu_nonant_stats, phgpu_ph_update_ex's conv and phgpu_w_diff on every
shape, phgpu_rho_ratio_stats and phgpu_nonant_closest on the two-stage ones.

The shapes are the smallest that reach each branch of the node-segmented final kernel
(k_node_final, and k_xbar_final for x̄: 256 threads, thread t sums chunk t of C = ceil(waves /
256) waves) and of the last-block ticket:

* two-stage S = 1, 63, 64, 65: one wave, a ragged wave, two waves; the single-node fast path,
  whose sums are stored (one tree node, every plane entry a nonant's: no clearing launch);
* two-stage S = 65 with a gap in the nonant offsets: the planes are cleared first, the fast
  path adds, the entry no nonant owns keeps its identity;
* two-stage S = 16,449: 258 waves, C = 2, the last threads' chunks are empty;
* aircond 4-3-2, S = 24: every wave spans nodes, so the atomic route and tag -1;
* a minimal LP over the tree [8, 65, 64], S = 33,280: 520 waves, C = 3; a third-stage node is
  one wave (first, complete middle and last run in one chunk), a second-stage node 65 waves
  (runs across many chunks, flushed by their owner), the root a single node.  The reductions
  never read the constraint data, so one row serves.

Every output against a host reference: sums within 1e-13 * sum |terms| of math.fsum of the same
products (the bound of tests/test_gpu_reductions.py: fp64 products and at most ~2^9 roundings
in sequence along any path of these reductions -- a wave's tree, a chunk of 3, a run's 256
owners -- of 1.1e-16 each); maxima, rho_last, the x̄ scatter and W_prev exactly; a second call
bit for bit, except the node sums of aircond 4-3-2: its mixed waves add by fp64 atomics in the
order the hardware performs them, which the design does not fix (sums of wave-uniform nodes
are deterministic; maxima, conv and w_diff do not go through that route).  The outputs hold
1e30 beforehand (stale data must not survive).

phgpu_nonant_closest: var = x̄² - x̄ x̄ may be contracted to one fused multiply-add on the
device, half an ulp of x̄ x̄ away from numpy's; the test's variances are at least x̄ x̄ / 4, so a
term moves by under 1e-15 relative and the distances are compared at 1e-13 * sum |terms|.  The
argmin is checked exactly against the device's own distances (smallest value, lowest index),
with the host's best scenario copied to a second index in another block: an exact tie.
"""
import math

import numpy as np
import pytest

import norm_rho_ref as R

pytestmark = pytest.mark.gpu

TWO_STAGE = ["S1", "S63", "S64", "S65", "S65gap", "S16449"]
CASES = TWO_STAGE + ["air432", "bf8_65_64"]
_ENGINES = {}


def _lp_batch(S, bf, offs=None):
    """S scenarios of one row  sum x <= 10 n, x in [0, 10], over the tree with branching factors
    ``bf`` (None: two-stage) and random probabilities.  Two-stage: three root nonants at
    offsets ``offs``; else two root, two second-stage and one third-stage nonant."""
    from mpisppy_amd.batch import ScenarioBatch
    rng = np.random.default_rng(S)
    if bf is None:
        depth_of, off_of = [0, 0, 0], list(offs or [0, 1, 2])
        width = [S]
    else:
        assert S == int(np.prod(bf)) and len(bf) == 3
        depth_of, off_of = [0, 0, 1, 1, 2], [0, 1, 0, 1, 0]
        width = [S, bf[1] * bf[2], bf[2]]         # scenarios per node at each depth
    nn, D = len(depth_of), len(width)
    n = nn + 1
    first = np.concatenate([[0], np.cumsum([S // w for w in width])])
    node_of = np.stack([first[d] + np.arange(S) // width[d] for d in range(D)], axis=1)
    names = [f"n{i}" for i in range(first[-1])]
    prob = rng.random(S) + 0.1
    prob /= prob.sum()
    pnode = np.stack([np.bincount(node_of[:, d], weights=prob, minlength=first[-1])[node_of[:, d]]
                      for d in range(D)], axis=1)
    return ScenarioBatch([f"s{i}" for i in range(S)], np.array([0, n], np.int32), np.arange(n, dtype=np.int32),
                         np.ones((S, n)), np.ones((S, n)), np.zeros((S, n)), np.full((S, n), 10.0),
                         np.full((S, 1), -np.inf), np.full((S, 1), 10.0 * n), np.zeros((S, n)), np.zeros(S),
                         np.arange(n - 1, n - 1 - nn, -1).astype(np.int32), np.array(depth_of, np.int32),
                         np.array(off_of, np.int32), node_of.astype(np.int32), names, prob, prob[:, None] / pnode)


def _batch(case):
    if case == "air432":
        from mpisppy_amd.examples import aircond
        return aircond.batch_creator(aircond.scenario_names_creator(24), branching_factors=R.AIR_BF, **R.AIR_KW)
    if case == "bf8_65_64":
        return _lp_batch(8 * 65 * 64, [8, 65, 64])
    if case == "S65gap":
        return _lp_batch(65, None, offs=[0, 1, 3])
    return _lp_batch(int(case[1:]), None)


@pytest.fixture(scope="module")
def engine(gpu):
    """Handles by case (made once, closed with the module)."""
    from mpisppy_amd.engine import PHEngine

    def get(case):
        if case not in _ENGINES:
            _ENGINES[case] = PHEngine(_batch(case), device="cuda:0")
        return _ENGINES[case]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


# ------------------------------------------------------------------ inputs and device calls
def _spread(rng, shape):
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3, 6, size=shape)


def _inputs(e, seed):
    """Host arrays: x [n, S]; xbar, rho, W, W_prev, v, cost [nn, S]; node [2 half]; xb, xsq, gden
    [nlen_max]."""
    rng = np.random.default_rng(seed)
    nn, S, half = e.nn, e.S, e.num_nodes * e.nlen_max
    a = {"x": _spread(rng, (e.n, S)), "node": _spread(rng, 2 * half)}
    for k in ("xbar", "W", "W_prev", "v", "cost"):
        a[k] = _spread(rng, (nn, S))
    a["rho"] = 10.0 ** rng.uniform(-3, 6, size=(nn, S))
    a["gden"] = 10.0 ** rng.uniform(-3, 3, size=e.nlen_max)
    # x̄ and x̄² of the closest-scenario measure: variances in [x̄²/4, 2 x̄²], one nonant's not
    # positive (skipped); the best scenario's column copied into another block (an exact tie)
    a["xb"] = _spread(rng, e.nlen_max)
    a["xsq"] = a["xb"] ** 2 * (1.0 + rng.uniform(0.25, 2.0, size=e.nlen_max))
    a["xsq"][int(e.batch.nonant_off[0])] = 0.5 * a["xb"][int(e.batch.nonant_off[0])] ** 2
    if e.num_nodes == 1:
        dist = _closest_terms(e, a).sum(axis=0)
        i0 = int(np.argmin(dist))
        # (the host's best is best by far more than the comparison's rounding)
        assert S == 1 or np.delete(dist, i0).min() > dist[i0] * (1.0 + 1e-9)
        a["tie"] = (i0, (i0 + 300) % S)
        a["v"][:, a["tie"][1]] = a["v"][:, i0]
    return a


def _closest_terms(e, a):
    off = np.asarray(e.batch.nonant_off)
    xb, var = a["xb"][off][:, None], (a["xsq"] - a["xb"] * a["xb"])[off][:, None]
    with np.errstate(invalid="ignore"):
        t = np.minimum(3.0, np.abs(a["v"] - xb) / np.sqrt(var))
    return np.where(var > 0.0, t, 0.0)


def _outputs(e, a):
    """Every output of one call of each entry point on the inputs ``a``, as host arrays."""
    import torch
    from mpisppy_amd import _lib
    dev, lib, h, st = e.device, e.lib, e.h, e._stream()
    half = e.num_nodes * e.nlen_max
    d = {k: torch.as_tensor(v, device=dev) for k, v in a.items() if k != "tie"}
    P = lambda t: t.data_ptr()  # noqa: E731
    stale = lambda *s: torch.full(s, 1e30, dtype=torch.float64, device=dev)  # noqa: E731
    out = {}
    node_buf = stale(2 * half)
    _lib.check(lib.phgpu_ph_reduce(h, P(d["x"]), P(node_buf), st), "ph_reduce")
    out["xbar_sums"] = node_buf
    planes, rho_last = stale(4 * half), stale(half)
    _lib.check(lib.phgpu_ph_residuals(h, P(d["x"]), P(d["xbar"]), P(d["rho"]), P(planes), P(rho_last), st),
               "ph_residuals")
    out["resid"], out["rho_last"] = planes, rho_last
    nstats = stale(4 * half)
    _lib.check(lib.phgpu_nonant_stats(h, P(d["v"]), P(nstats), st), "nonant_stats")
    out["nstats"] = nstats
    xbar, conv = stale(e.nn, e.S), stale(1)
    _lib.check(lib.phgpu_ph_update_ex(h, P(d["x"]), P(d["node"]), P(xbar), 0, 0, 0, P(conv), 0, st), "ph_update_ex")
    out["scatter"], out["conv"] = xbar, conv
    W_prev, wd = d["W_prev"].clone(), stale(1)
    _lib.check(lib.phgpu_w_diff(h, P(d["W"]), P(W_prev), P(wd), st), "w_diff")
    out["w_diff"], out["W_prev"] = wd, W_prev
    if e.num_nodes == 1:
        for name, g in (("rr_own", 0), ("rr_gden", P(d["gden"]))):
            rr = stale(3 * half)
            _lib.check(lib.phgpu_rho_ratio_stats(h, P(d["cost"]), P(d["x"]), P(d["xbar"]), g, P(rr), st),
                       "rho_ratio_stats")
            out[name] = rr
        dist, best = stale(e.S), stale(2)
        _lib.check(lib.phgpu_nonant_closest(h, P(d["v"]), P(d["xb"]), P(d["xsq"]), P(dist), P(best), st),
                   "nonant_closest")
        out["dist"], out["best"] = dist, best
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ host reference
def _keys(e):
    """[nn, S] plane index (node, offset) of every local (nonant, scenario)."""
    b = e.batch
    node_of = e.node_of.cpu().numpy().reshape(-1, e.S)
    return np.stack([node_of[int(b.nonant_depth[k])] * e.nlen_max + int(b.nonant_off[k]) for k in range(e.nn)])


def _runs(key_k):
    """(entry, first, end) of the runs of equal entries in one nonant's keys (tree order: a
    node's scenarios are consecutive)."""
    cut = np.flatnonzero(np.diff(key_k)) + 1
    lo = np.concatenate([[0], cut])
    hi = np.concatenate([cut, [len(key_k)]])
    assert len(set(key_k[lo].tolist())) == len(lo), "a node's scenarios are not one run"
    return [(int(key_k[a]), int(a), int(b)) for a, b in zip(lo, hi)]


def _check_sum(got, want_terms, what):
    want, scale = math.fsum(want_terms), math.fsum(np.abs(want_terms))
    print(f"{what}: got {got!r} want {want!r} err/scale {abs(got - want) / scale if scale else 0.0:.2e}")
    assert abs(got - want) <= 1e-13 * scale, (what, got, want, scale)


def _check_planes(e, got, key, terms, kinds, what):
    """got [len(kinds) * half]; terms[j] [nn, S]; kinds[j] 's' (sum) or 'm' (maximum)."""
    half = e.num_nodes * e.nlen_max
    got = got.reshape(len(kinds), half)
    seen = np.zeros(half, bool)
    worst = 0.0
    for k in range(e.nn):
        for ent, a, b in _runs(key[k]):
            seen[ent] = True
            for j, kind in enumerate(kinds):
                t = terms[j][k, a:b]
                if kind == "m":
                    assert got[j, ent] == t.max(), (what, j, k, ent, got[j, ent], t.max())
                else:
                    want, scale = math.fsum(t), math.fsum(np.abs(t))
                    worst = max(worst, abs(got[j, ent] - want) / scale if scale else 0.0)
                    assert abs(got[j, ent] - want) <= 1e-13 * scale, (what, j, k, ent, got[j, ent], want, scale)
    print(f"{what}: largest |sum - fsum| / sum |terms| = {worst:.2e}")
    for j, kind in enumerate(kinds):            # entries no local scenario reaches: the identity
        ident = -np.inf if kind == "m" else 0.0
        assert (got[j, ~seen] == ident).all(), (what, j, got[j, ~seen])
    return seen


def _pcoef(e):
    return e.prob_coeff.cpu().numpy().reshape(-1, e.S)[np.asarray(e.batch.nonant_depth)]


@pytest.mark.parametrize("case", CASES)
def test_node_sums_conv_and_w_diff(engine, case):
    e = engine(case)
    a = _inputs(e, 7)
    got = _outputs(e, a)
    key, pc = _keys(e), _pcoef(e)
    prob = e.prob.cpu().numpy()
    xn = a["x"][np.asarray(e.batch.nonant_col)]
    half = e.num_nodes * e.nlen_max
    _check_planes(e, got["xbar_sums"], key, [pc * xn, pc * xn * xn], "ss", "ph_reduce")
    ad = np.abs(xn - a["xbar"])
    seen = _check_planes(e, got["resid"], key, [prob * ad, pc * ad, a["rho"], prob * a["rho"]], "ssss", "residuals")
    last = np.zeros(half)                       # the rho of a node's last local scenario; else 0
    for k in range(e.nn):
        for ent, _, b in _runs(key[k]):
            last[ent] = a["rho"][k, b - 1]
    assert np.array_equal(got["rho_last"], last) and (last[~seen] == 0.0).all()
    _check_planes(e, got["nstats"], key, [pc * a["v"], pc * a["v"] * a["v"], -a["v"], a["v"]], "ssmm", "nonant_stats")
    # the update: x̄ scattered exactly, conv = sum |x - x̄| / (S nn)
    want = a["node"][key]
    assert np.array_equal(got["scatter"], want)
    scale = 1.0 / (float(e.S) * float(e.nn))
    _check_sum(got["conv"][0] / scale, np.abs(xn - want).ravel(), "conv / scale")
    _check_sum(got["w_diff"][0] * float(e.nn * e.S), np.abs(a["W"] - a["W_prev"]).ravel(), "w_diff x (S nn)")
    assert np.array_equal(got["W_prev"], a["W"])
    again = _outputs(e, a)
    half4 = 4 * half
    for k in got:
        g, r = got[k], again[k]
        if case == "air432" and k in ("xbar_sums", "resid", "nstats"):   # atomic sums: see the docstring
            if k == "nstats":                                            # (its maxima are order-free)
                g, r = g[half4 // 2:], r[half4 // 2:]
            else:
                continue
        assert np.array_equal(g, r), (case, k, "two calls differ")


@pytest.mark.parametrize("case", TWO_STAGE)
def test_two_stage_ratio_stats_and_closest(engine, case):
    e = engine(case)
    a = _inputs(e, 7)
    got = _outputs(e, a)
    key = _keys(e)
    off = np.asarray(e.batch.nonant_off)
    dx = a["x"][np.asarray(e.batch.nonant_col)] - a["xbar"]
    own = np.maximum(np.abs(dx), 2.0 * (dx * dx)).max(axis=0)
    for name, den in (("rr_own", own[None, :]), ("rr_gden", a["gden"][off][:, None])):
        r = np.abs(a["cost"]) / den
        _check_planes(e, got[name], key, [r, -r, r], "smm", name)
    terms = _closest_terms(e, a)
    worst = 0.0
    for s in range(e.S):
        want, scale = math.fsum(terms[:, s]), math.fsum(np.abs(terms[:, s]))
        worst = max(worst, abs(got["dist"][s] - want) / scale if scale else 0.0)
        assert abs(got["dist"][s] - want) <= 1e-13 * scale, (s, got["dist"][s], want)
    print(f"closest: largest |dist - fsum| / sum |terms| = {worst:.2e}")
    # the smallest distance and the lowest index attaining it, exactly; the tie's two scenarios
    # have the same distance to the bit, and the lower index wins
    i0, i1 = a["tie"]
    assert got["dist"][i0] == got["dist"][i1]
    dmin = got["dist"].min()
    assert got["best"][0] == dmin and got["best"][1] == float(np.flatnonzero(got["dist"] == dmin)[0])
    if e.S > 1:
        assert dmin == got["dist"][i0] and int(got["best"][1]) == min(i0, i1), (got["best"], i0, i1)
    again = _outputs(e, a)
    for k in got:
        assert np.array_equal(got[k], again[k]), (case, k, "two calls differ")
