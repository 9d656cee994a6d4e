"""PH with bundles without a GPU: the CPU restatement (tests/bundle_ref.py) through
the interior point's numpy text against exact solves of each bundle, the slicing and names against
the reference's formula, the kernels' own text run on the host over several segments
(tests/bundle_host.cpp) against the restatement bundle by bundle, the C entries, and the refusals."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bundle_ref as B
import ef_ref as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "include", "phgpu.h")
LIB = os.path.join(ROOT, "mpi-sppy-1_amd", "mpisppy_amd", "libphgpu.so")
BUNDLE_SYMBOLS = ["phgpu_bundle_init", "phgpu_bundle_start", "phgpu_bundle_schur", "phgpu_bundle_direction",
                  "phgpu_bundle_step", "phgpu_bundle_export"]
TRAJ_TOL = 1e-5            # W and x̄: the project's tolerance (BASELINE.json)
BOUND_REL = 1e-8


# ------------------------------------------------------------------ the restatement against exact solves
def test_interior_point_bundles_follow_the_exact_trajectory():
    """Farmer S = 10, cm = 1, 3 bundles (3, 3, 4), rho = 1, 10 iterations at tol 1e-10.  Measured:
    max |dW| 1.3e-6, max |dx̄| 8.5e-7, trivial bound 7.9e-12 relative, 17 to 36 iterations."""
    ex = B.farmer_run(10, 1, 3, 10, "exact")
    ip = B.farmer_run(10, 1, 3, 10, "efref")
    assert [len(b) for b in ex.bundles] == [3, 3, 4]
    dW = max(np.abs(a["W"] - b["W"]).max() for a, b in zip(ex.history, ip.history))
    dx = max(np.abs(a["xbar"] - b["xbar"]).max() for a, b in zip(ex.history, ip.history))
    rel = abs(ip.trivial_bound - ex.trivial_bound) / abs(ex.trivial_bound)
    print(f"max |dW| {dW:.2e} max |dxbar| {dx:.2e} trivial bound {ip.trivial_bound:.6f} / {ex.trivial_bound:.6f} ({rel:.1e}) "
          f"iterations {min(map(min, ip.ipm_iters))}..{max(map(max, ip.ipm_iters))}")
    assert len(ex.history) == len(ip.history) == 10 and ip.failures == 0
    assert dW <= TRAJ_TOL and dx <= TRAJ_TOL
    assert rel <= BOUND_REL
    # within a bundle every scenario carries the bundle's nonants
    for ks in ip.bundles:
        assert np.array_equal(ip.x[ks], np.broadcast_to(ip.x[ks[0]], (len(ks), ip.nn)))


@pytest.mark.parametrize("mode", ["exact", "efref"])
def test_one_bundle_is_the_extensive_form(mode):
    ph = B.farmer_run(10, 1, 1, 1, mode)
    obj, z = E.ef_optimum(ph.scens, ph.data)
    assert abs(ph.trivial_bound - obj) <= BOUND_REL * abs(obj)
    assert np.abs(ph.iter0_x - z).max() <= 1e-6
    assert ph.history[0]["conv"] < 1e-10


def test_bundles_tighten_the_trivial_bound():
    plain = B.farmer_run(10, 1, 10, 0, "exact").trivial_bound        # one scenario per bundle: plain PH
    bundled = B.farmer_run(10, 1, 3, 10, "exact").trivial_bound
    ef = B.farmer_run(10, 1, 1, 1, "exact").trivial_bound
    print(f"trivial bound: plain {plain:.2f} bundled {bundled:.2f} extensive form {ef:.2f}")
    assert plain < bundled < ef
    assert abs(bundled + 122466.38) <= 0.01 and abs(plain + 128329.37) <= 0.01


# ------------------------------------------------------------------ slicing and names
SOLVER = "mi355x_pdhg"


def _options(**kw):
    o = {"solver_name": SOLVER, "PHIterLimit": 2, "defaultPHrho": 1.0, "convthresh": 1e-8, "verbose": False,
         "display_progress": False, "toc": False}
    o.update(kw)
    return o


def _ph(S, cls=None, comm=None, **kw):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.ph import PH
    extra = {k: kw.pop(k) for k in ("extensions",) if k in kw}
    return (cls or PH)(_options(**kw), farmer.scenario_names_creator(S), farmer.scenario_creator,
                       scenario_creator_kwargs={"num_scens": S}, mpicomm=comm, **extra)


def _rank_of(r, size):
    from mpisppy_amd.comm import Comm

    class _Rank(Comm):
        def __init__(self):
            self.group, self.rank, self.size = None, r, size
    return _Rank()


def _reference_names(S, n_proc, bpr):
    """names_in_bundles by the reference's formula, written out here on its own."""
    names = [f"scen{i}" for i in range(S)]
    out = {}
    for r in range(n_proc):
        avg_r = S / n_proc
        mine = names if n_proc == 1 else names[int(r * avg_r):int((r + 1) * avg_r)]
        avg = len(mine) / bpr
        out[r] = {b: mine[int(b * avg):int((b + 1) * avg)] for b in range(bpr)}
    return out


def test_slicing_one_rank_three_bundles():
    ph = _ph(10, bundles_per_rank=3)
    assert ph.bundling and ph.names_in_bundles == _reference_names(10, 1, 3) == B.names_in_bundles(ph.all_scenario_names, 1, 3)
    assert [len(v) for v in ph.names_in_bundles[0].values()] == [3, 3, 4]
    subs = ph.local_subproblems
    assert list(subs) == ["rank0bundle0", "rank0bundle1", "rank0bundle2"]
    assert subs["rank0bundle2"].scen_list == ["scen6", "scen7", "scen8", "scen9"]
    assert np.allclose([s._mpisppy_probability for s in subs.values()], [0.3, 0.3, 0.4])
    seg, zlb, zub, ncomp, cmax, qp = ph._bundle_data()
    assert list(seg) == [0, 3, 6, 10] and zlb.shape == (3, 3) and np.all(zlb == 0.0) and np.all(zub == 500.0) and not qp
    # the finite bounds and max |c| of each bundle: what the restatement counts on the same scenarios
    d = E.batch_data(ph.batch)
    refs = [E.EFRef(data=tuple(a[s0:s1] for a in d[:8]) + (d[8],)) for s0, s1 in zip(seg[:-1], seg[1:])]
    assert list(ncomp) == [r.ncomp for r in refs] and list(cmax) == [r.cmax for r in refs]


def test_slicing_two_ranks_two_bundles_each():
    ref = _reference_names(12, 2, 2)
    for r in (0, 1):
        ph = _ph(12, comm=_rank_of(r, 2), bundles_per_rank=2)
        assert ph.names_in_bundles == ref == B.names_in_bundles(ph.all_scenario_names, 2, 2)
        assert list(ph.local_subproblems) == [f"rank{r}bundle0", f"rank{r}bundle1"]
        assert [s.scen_list for s in ph.local_subproblems.values()] == [ref[r][0], ref[r][1]]
        assert [(s.first, s.last) for s in ph.local_subproblems.values()] == [(0, 3), (3, 6)]
    assert ref[1][1] == ["scen9", "scen10", "scen11"]


def test_not_enough_scenarios():
    with pytest.raises(RuntimeError, match="Not enough scenarios to satisfy the bundles_per_rank requirement"):
        _ph(3, bundles_per_rank=4)
    with pytest.raises(RuntimeError, match="Not enough scenarios"):
        B.bundle_slices([0, 1], 3)


def test_without_bundles_nothing_changes():
    ph = _ph(3)
    assert not ph.bundling and ph.local_subproblems is ph.local_scenarios and not hasattr(ph, "names_in_bundles")


def test_classes_that_do_not_serve_bundles_still_raise():
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.fwph.fwph import FWPH
    from mpisppy_amd.opt.aph import APH
    from mpisppy_amd.opt.ef import ExtensiveForm
    from mpisppy_amd.opt.lshaped import LShapedMethod
    from mpisppy_amd.opt.sc import SchurComplement
    from mpisppy_amd.spbase import SPBase
    from mpisppy_amd.spopt import SPOpt
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    names, kw = farmer.scenario_names_creator(4), {"num_scens": 4}
    o = _options(bundles_per_rank=2)
    for cls in (SPBase, SPOpt, Xhat_Eval, APH, LShapedMethod):
        with pytest.raises(NotImplementedError, match="bundles"):
            cls(dict(o), names, farmer.scenario_creator, scenario_creator_kwargs=kw)
    with pytest.raises(NotImplementedError, match="bundles"):
        FWPH(dict(o), {"FW_iter_limit": 1}, names, farmer.scenario_creator, scenario_creator_kwargs=kw)
    with pytest.raises(NotImplementedError, match="bundles"):
        ExtensiveForm(dict(o, solver=SOLVER), names, farmer.scenario_creator, scenario_creator_kwargs=kw)
    with pytest.raises(ValueError, match="does not support bundling"):
        SchurComplement(dict(o), names, farmer.scenario_creator, scenario_creator_kwargs=kw)


def test_refusals_that_need_no_device():
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.extensions.fixer import Fixer
    from mpisppy_amd.opt.ph import PH
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    with pytest.raises(NotImplementedError, match="Fixer"):
        _ph(6, bundles_per_rank=2, extensions=Fixer, fixeroptions={"boundtol": 0.01, "id_fix_list_fct": None})
    bfs = [2, 2]
    with pytest.raises(RuntimeError, match="two-stage"):
        PH(_options(bundles_per_rank=2), aircond.scenario_names_creator(4), aircond.scenario_creator,
           all_nodenames=create_nodenames_from_branching_factors(bfs),
           scenario_creator_kwargs={"branching_factors": bfs, "start_seed": 1134})
    with pytest.raises(NotImplementedError, match="shared-matrix"):
        _ph(6, bundles_per_rank=2, shared_matrix=True)
    with pytest.raises(NotImplementedError, match="fused_ph_loop"):
        _ph(6, bundles_per_rank=2, fused_ph_loop=True)._fused_loop(False)
    with pytest.raises(NotImplementedError, match="speculative_solve"):
        _ph(6, bundles_per_rank=2, speculative_solve=True)._speculate(False)
    assert _ph(6, bundles_per_rank=2)._speculate(False) is False
    with pytest.raises(NotImplementedError, match="fixing the nonants"):
        _ph(6, bundles_per_rank=2)._fix_nonants({"ROOT": [80.0, 250.0, 170.0]})
    with pytest.raises(ValueError, match="bundle_tol"):
        _ph(6, bundles_per_rank=2, bundle_tol=0.0)
    ph = _ph(6, bundles_per_rank=2)
    assert ph.bundle_tol == 1e-10 and ph.bundle_step_tol == ZTOL and ph.bundle_max_iter == 100


def test_post_solve_hooks_receive_the_bundles():
    """post_solve gets each bundle object with the bundle's objective sum_s (p_s / p_B) obj_s, status and iterations
    (the engine's outputs stood in for by arrays)."""
    ph = _ph(10, bundles_per_rank=3)
    S, n = ph.batch.S, ph.batch.n

    class _Outputs:
        vals = {"x": np.zeros((S, n)), "status": np.array([0] * 6 + [1] * 4), "obj": np.arange(10.0), "bound": np.arange(10.0),
                "iters": np.array([17] * 3 + [18] * 3 + [100] * 4)}

        def host(self, k):
            return self.vals[k]

    class _Ext:
        got = []

        def post_solve(self, sp, res):
            self.got.append((sp.name, sp.scen_list, res.status, res.iterations, res.Problem[0].Upper_bound))

    ph.engine = _Outputs()
    ph._post_solve_hooks(_Ext())
    ph.engine = None
    assert [g[0] for g in _Ext.got] == ["rank0bundle0", "rank0bundle1", "rank0bundle2"]
    assert _Ext.got[2][1:4] == (["scen6", "scen7", "scen8", "scen9"], 1, 100)
    assert np.allclose([g[4] for g in _Ext.got], [1.0, 4.0, 7.5])


def test_a_bundle_without_an_interior_is_refused():
    from mpisppy_amd.examples import farmer

    def pinned(name, **kw):
        m = farmer.scenario_creator(name, **kw)
        j = m.find_var("DevotedAcreage[CORN0]").index
        if name == "scen4":
            m.lb[j] = m.ub[j] = 80.0
        return m

    from mpisppy_amd.opt.ph import PH
    ph = PH(_options(bundles_per_rank=2), farmer.scenario_names_creator(6), pinned, scenario_creator_kwargs={"num_scens": 6})
    with pytest.raises(NotImplementedError, match="bundle rank0bundle1: nonant 0 has the bounds"):
        ph._bundle_data()


# ------------------------------------------------------------------ the kernels' text on the host
def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if p:
            return p
    pytest.fail("no C++ compiler for tests/bundle_host.cpp", pytrace=False)


INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "mpi-sppy-1_amd", "csrc")]
SRC = os.path.join(HERE, "bundle_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bundle_host")
    so = str(d / "libbundle_host.so")
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-fPIC", "-shared", *INC, "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.bundle_host_solve.restype = ctypes.c_int
    return lib


def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with AddressSanitizer and UBSan: a stand-alone program."""
    exe = str(tmp_path / "bundle_host_san")
    subprocess.run([_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-DBUNDLE_HOST_MAIN", *INC, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr


ZTOL = 1e-8               # spopt.DEFAULT_BUNDLE_STEP_TOL


def host_solve(lib, ph, tol=1e-10, max_iter=100, ztol=ZTOL):
    """Every bundle of the BundlePH's current state at once on the host; and the restatement of each."""
    parts = [ph.bundle_data(b)[0] for b in range(len(ph.bundles))]
    refs = [E.EFRef(data=d, tol=tol, max_iter=max_iter) for d in parts]
    oks = [r.run() for r in refs]
    data = tuple(np.concatenate([d[k] for d in parts]) for k in range(8)) + (parts[0][8],)
    A, rl, ru, lb, ub, c, q, p, idx = data
    S, m, n = A.shape
    nn, G = len(idx), len(parts)
    row_ptr, col_idx, val = E.csr(data)
    T = lambda a: np.ascontiguousarray(a.T)  # noqa: E731
    P = lambda a, t=ctypes.c_double: a.ctypes.data_as(ctypes.POINTER(t))  # noqa: E731
    arrs = [T(val), T(c), T(q), T(lb), T(ub), T(rl), T(ru), np.ascontiguousarray(p)]
    seg = np.concatenate([[0], np.cumsum([len(b) for b in ph.bundles])]).astype(np.int32)
    zlb = np.ascontiguousarray([d[3][:, idx].max(axis=0) for d in parts])
    zub = np.ascontiguousarray([d[4][:, idx].min(axis=0) for d in parts])
    ncomp = np.array([float(r.ncomp) for r in refs])
    cmax = np.array([r.cmax for r in refs])
    ntri = nn * (nn + 1) // 2
    x, y, z = np.zeros((n, S)), np.zeros((m, S)), np.zeros((G, nn))
    first, obj = np.zeros((G, ntri + nn)), np.zeros(G)
    iters, status = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    nc = np.ascontiguousarray(idx, dtype=np.int32)
    bad = lib.bundle_host_solve(ctypes.c_int64(S), n, m, len(col_idx), nn, P(row_ptr, ctypes.c_int32), P(col_idx, ctypes.c_int32),
                                P(nc, ctypes.c_int32), *[P(a) for a in arrs], G, P(seg, ctypes.c_int32), P(zlb), P(zub),
                                P(ncomp), P(cmax), ctypes.c_double(tol), ctypes.c_double(ztol), int(any(r.qp for r in refs)), max_iter, P(x), P(y),
                                P(z), P(first), P(obj), P(iters, ctypes.c_int32), P(status, ctypes.c_int32))
    return bad, x.T, z, first, obj, iters, status, refs, oks, seg


def _state(S, bpr, it):
    """A BundlePH of its own in the exact run's state after PH iteration ``it`` (0: Iter0's LPs)."""
    src = B.farmer_run(S, 1, bpr, max(it, 1), "exact")
    ph = B.BundlePH(src.scens, 1.0, bpr)
    if it:
        ph.W, ph.xbar = src.history[it - 1]["W"].copy(), src.history[it - 1]["xbar"].copy()
        ph.W_on = ph.prox_on = 1
    return ph


@pytest.mark.parametrize("S,bpr,it", [(10, 3, 0), (10, 3, 5), (130, 7, 0), (130, 7, 2)])
def test_host_kernels_follow_the_restatement_bundle_by_bundle(host, S, bpr, it):
    """Per bundle: the first pass's C and right-hand side to 1e-10 (as tests/test_ef.py: the host
    factors by LDL', numpy by LU), the objective to 1e-9 relative (both stop at 1e-10: by weak
    duality each is within a few 1e-10 (1 + |obj|) of the optimum), the iteration counts as
    tests/test_ef.py bounds them.  Bundles end at different iterations, so per-segment termination runs."""
    ph = _state(S, bpr, it)
    bad, x, z, first, obj, iters, status, refs, oks, seg = host_solve(host, ph)
    nn = ph.nn
    tri = np.tril_indices(nn)
    assert bad == 0 and all(oks) and np.all(status == 0)
    for g, ref in enumerate(refs):
        C, rhs = ref.first
        Cs = C.copy()
        Cs[np.arange(nn), np.arange(nn)] = np.diag(C) / (1.0 + E.EFRef.REG) - ref.qz - ref.theta0
        assert np.abs(first[g, :len(tri[0])] - Cs[tri]).max() <= 1e-10 * np.abs(Cs).max()
        assert np.abs(first[g, len(tri[0]):] - (rhs + ref.rz0)).max() <= 1e-10 * max(1.0, np.abs(rhs + ref.rz0).max())
        assert abs(obj[g] - ref.obj) <= 1e-9 * abs(ref.obj), (g, obj[g], ref.obj)
        assert 0 < iters[g] <= 2 * ref.it
        sl = slice(seg[g], seg[g + 1])
        assert np.array_equal(x[sl][:, ph.data[8]], np.broadcast_to(z[g], (seg[g + 1] - seg[g], nn)))
    print(f"S={S} bundles={bpr} PH iteration {it}: host iterations {list(iters)} restatement {[r.it for r in refs]} "
          f"worst objective error {max(abs(o - r.obj) / abs(r.obj) for o, r in zip(obj, refs)):.1e}")
    if (S, bpr) == (10, 3):
        assert len(set(iters)) >= 2


def test_refinement_of_dz_on_the_engines_own_model(host):
    """The engine's farmer holds the quota as column bounds where the oracle's model has rows.  On it,
    after PH iteration 1, the third bundle's dual residual stalls at 2.3e-10 (1 + max |c|) in the
    restatement, which then divides by a slack of zero: the regularisation of the Schur complement
    leaves EF_REG diag(C) dz in z's stationarity row and C grows like 1 / mu.  The segmented solve
    corrects dz for it (ef_seg_refine) and passes its test (residuals 1e-10, z's step 1e-8) in 20 iterations; objectives against the
    exact solve of the explicit bundle problem.  z: the test bounds the duality gap by tol (1 + |obj|),
    the objective is rho-strongly convex in z (rho = 1), so |z - z*| <= sqrt(2 tol (1 + |obj|) / rho) =
    5.8e-3 is what the residuals guarantee; measured 9.0e-8, 3.1e-9 and 4.9e-6 (1.3e-4 at 17 iterations
    without the step criterion of ef_seg_test)."""
    ph = _state(10, 3, 1)
    ph.data = E.batch_data(_ph(10, bundles_per_rank=3).batch)
    with np.errstate(all="ignore"):
        bad, x, z, first, obj, iters, status, refs, oks, seg = host_solve(host, ph)
    print(f"engine's model, PH iteration 1: host iterations {list(iters)} status {list(status)}; restatement {[r.it for r in refs]} {oks}")
    assert oks == [True, True, False]                   # (what the correction is for; the restatement has none)
    assert bad == 0 and np.all(status == 0) and iters.max() <= 25
    for g in range(3):
        zx, want = ph.solve_bundle_exact(g)
        want -= ph.bundle_data(g)[1]
        assert abs(obj[g] - want) <= 1e-9 * abs(want), (g, obj[g], want)
        print(f"bundle {g}: |z - exact| {np.abs(z[g] - zx).max():.1e}")
        assert np.abs(z[g] - zx).max() <= np.sqrt(2.0 * 1e-10 * (1.0 + abs(want)) / 1.0)


def test_host_iteration_limit_is_per_bundle(host):
    """max_iter = 3: no bundle passes; status ITER_LIMIT, the iterates finite."""
    ph = _state(10, 3, 0)
    bad, x, z, *_, iters, status, refs, oks, seg = host_solve(host, ph, max_iter=3)
    assert bad == 3 and np.all(status == 1) and np.all(iters == 3) and np.all(np.isfinite(x))


# ------------------------------------------------------------------ the C entries
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build(verbose=False)
    return ctypes.CDLL(LIB)


def test_entries_declared_exported_and_typed(lib):
    txt = open(HDR).read()
    from mpisppy_amd import _lib
    L = _lib.load()
    for s in BUNDLE_SYMBOLS:
        m = re.search(rf"^int\s+{s}\s*\(([^;]*)\);", txt, re.M | re.S)
        assert m, s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS
        fn = getattr(L, s)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(m.group(1).split(",")), s


def test_null_handle_is_an_error(lib):
    from mpisppy_amd import _lib
    from mpisppy_amd.engine import PHEngine
    L = _lib.load()
    n = None
    assert L.phgpu_bundle_init(n, 1, n, n, n, n, n, 1e-10, 1e-8, 0, n) == -1
    assert L.phgpu_bundle_start(n, n) == -1
    assert L.phgpu_bundle_schur(n, 0, n, n, n, n) == -1
    assert L.phgpu_bundle_direction(n, 0, n, n) == -1
    assert L.phgpu_bundle_step(n, 0, n) == -1
    assert L.phgpu_bundle_export(n, n, n, n, n, n, n, n) == -1
    assert "null" in _lib.last_error()
    for m in ("bundle_init", "bundle_start", "bundle_schur", "bundle_direction", "bundle_step", "bundle_read", "bundle_solve"):
        assert callable(getattr(PHEngine, m)), m
