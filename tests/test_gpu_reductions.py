"""phgpu_status_counts and phgpu_expectations, the reductions that turn the solve outputs into
the numbers PH reports (SPOpt.solve_loop's gripe, Eobjective / Ebound / E1 / feas_prob), on
synthetic device arrays over farmer handles of S = 1, 63, 64, 65, 4097 and 16391 scenarios.

k_status_counts runs one block of 1,024 threads: a four-deep unrolled int4 loop, a single int4
loop and a scalar tail, and a scalar-only route for a status pointer that is not 16-byte
aligned.  At S = 16391, S / 4 = 4097 > 4 * 1024, so all three loops run; the view offset by
one element takes the unaligned route.  Counts are compared with np.bincount exactly.

phgpu_expectations' five sums are compared with math.fsum of the same products within
1e-13 * sum |terms| (fp64 products and a tree sum of at most ~2^15 terms: <= 16 roundings of
1.1e-16 each) and must repeat bit for bit (the sum is documented as deterministic).
"""
import math

import numpy as np
import pytest

from test_gpu_scale import _tiny_batch

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 4097, 16391]
_ENGINES = {}


@pytest.fixture(scope="module")
def farmer_engine(gpu):
    """Farmer handles by S (made once per size, closed with the module)."""
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.examples import farmer

    def get(S):
        if S not in _ENGINES:
            b = farmer.batch_creator(farmer.scenario_names_creator(S), crops_multiplier=1, num_scens=S)
            _ENGINES[S] = PHEngine(b, device="cuda:0")
        return _ENGINES[S]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _counts(e, status_dev):
    import torch
    from mpisppy_amd import _lib
    out = torch.full((4,), -7, dtype=torch.int32, device=e.device)
    _lib.check(e.lib.phgpu_status_counts(e.h, status_dev.data_ptr(), out.data_ptr(), e._stream()), "status_counts")
    return out.cpu().numpy()


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("absent", [None, 2])
def test_status_counts_aligned_and_unaligned(farmer_engine, S, absent):
    import torch
    e = farmer_engine(S)
    rng = np.random.default_rng(S + (absent or 0))
    st = rng.integers(0, 4, size=S).astype(np.int32)
    if absent is not None:
        st[st == absent] = 0
    want = np.bincount(st, minlength=4)
    aligned = torch.as_tensor(st, device=e.device)
    assert aligned.data_ptr() % 16 == 0
    assert np.array_equal(_counts(e, aligned), want), (S, "aligned")
    buf = torch.full((S + 1,), 3, dtype=torch.int32, device=e.device)   # (element 0 is not counted)
    view = buf[1:]
    view.copy_(aligned)
    assert view.data_ptr() % 16 == 4
    assert np.array_equal(_counts(e, view), want), (S, "offset by one element")


def test_status_counts_match_solve_stats_on_mixed_statuses(gpu):
    """A real solve whose statuses mix: one primal-infeasible scenario, the others with costs
    spread so that an iteration cap between their iteration counts leaves some at ITER_LIMIT
    (path 1, the global-memory PDHG).  The first four words of phgpu_solve_stats equal
    phgpu_status_counts on the same status buffer, and both equal the host's count."""
    import torch
    from mpisppy_amd import _lib
    from mpisppy_amd.engine import PHEngine
    S, bad = 70, 37
    b = _tiny_batch(S, bad, "primal")
    rng = np.random.default_rng(5)
    b.c[:] *= rng.uniform(0.2, 5.0, size=b.c.shape)      # different iteration counts per scenario
    b.ru[:, 0] = rng.uniform(2.0, 8.0, size=S)
    b.rl[bad, 0], b.ru[bad, 0] = 25.0, np.inf
    e = PHEngine(b, device="cuda:0")
    try:
        e.solve(_lib.default_options(kernel=1, infeas_start=0, check_every=16), warm=False)
        st, it = e.host("status"), e.host("iters")
        others = np.delete(np.arange(S), bad)
        assert st[bad] == _lib.PRIMAL_INFEASIBLE and (st[others] == 0).all(), (st, it)
        # a cap (a multiple of check_every = 16) that certifies the infeasible scenario and
        # splits the others
        # (a scenario whose test passes at iteration max_iter is already at the limit)
        cap = int(max(it[bad], np.median(it[others])))
        cap = (cap + 15) // 16 * 16 + 16
        print(f"iters: bad {it[bad]}, others {it[others].min()}..{it[others].max()}, cap {cap}", flush=True)
        assert it[others].min() < cap < it[others].max(), (cap, it)
        e.solve(_lib.default_options(kernel=1, infeas_start=0, check_every=16, max_iter=cap), warm=False)
        st = e.host("status")
        want = np.bincount(st, minlength=4)
        assert want[0] > 0 and want[1] > 0 and want[2] == 1, want
        stats = torch.zeros(6, dtype=torch.int64, device=e.device)
        _lib.check(e.lib.phgpu_solve_stats(e.h, stats.data_ptr(), e._stream()), "solve_stats")
        got = _counts(e, e.status)
        assert np.array_equal(got, want), (got, want)
        assert np.array_equal(stats.cpu().numpy()[:4], got), (stats, got)
    finally:
        e.close()


def _expect(e, obj, bound, st):
    import torch
    from mpisppy_amd import _lib
    out = torch.full((5,), float("nan"), dtype=torch.float64, device=e.device)
    args = [torch.as_tensor(a, device=e.device) for a in (obj, bound, st)]
    _lib.check(e.lib.phgpu_expectations(e.h, args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(),
                                        out.data_ptr(), e._stream()), "expectations")
    return out.cpu().numpy()


@pytest.mark.parametrize("S", SIZES)
def test_expectations_vs_fsum(farmer_engine, S):
    from mpisppy_amd import _lib
    e = farmer_engine(S)
    p = e.batch.prob
    rng = np.random.default_rng(S)
    mag = 10.0 ** rng.uniform(-3, 6, size=(2, S))
    obj, bound = rng.choice([-1.0, 1.0], size=(2, S)) * mag
    st = rng.integers(0, 4, size=S).astype(np.int32)
    got = _expect(e, obj, bound, st)
    terms = [p * obj, p * bound, p, np.where(st <= 1, p, 0.0), np.where(st == 0, p, 0.0)]
    for k, t in enumerate(terms):
        want, scale = math.fsum(t), math.fsum(np.abs(t))
        assert abs(got[k] - want) <= 1e-13 * scale, (S, k, got[k], want)
    assert np.array_equal(_expect(e, obj, bound, st), got), "two calls differ"
    # one scenario primal infeasible with obj = bound = +inf
    s = S // 2
    obj2, bound2, st2 = obj.copy(), bound.copy(), st.copy()
    obj2[s] = bound2[s] = np.inf
    st2[s] = _lib.PRIMAL_INFEASIBLE
    inf = _expect(e, obj2, bound2, st2)
    assert inf[0] == np.inf and inf[1] == np.inf, inf
    assert inf[2] == got[2], (inf[2], got[2])
    for k, was in ((3, st[s] <= 1), (4, st[s] == 0)):
        drop = p[s] if was else 0.0
        assert abs((got[k] - inf[k]) - drop) <= 1e-13 * math.fsum(p), (S, k, got[k], inf[k], drop)
