"""The extensive form's interior point without a GPU: the numpy restatement
(tests/ef_ref.py) against HiGHS, the kernels' own text run on the host (tests/ef_host.cpp) against
the restatement, the C entries, and what the two classes refuse."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ef_ref as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "include", "phgpu.h")
LIB = os.path.join(ROOT, "mpi-sppy-1_amd", "mpisppy_amd", "libphgpu.so")
EF_SYMBOLS = ["phgpu_ef_init", "phgpu_ef_schur", "phgpu_ef_direction", "phgpu_ef_step", "phgpu_ef_export"]
TOL = 1e-8
# The test stops at a relative gap, primal and dual residual of TOL each: by weak duality the
# objective is then within a few TOL (1 + |obj|) of the optimum.  Ten times TOL.
OBJ_REL = 1e-7
LP_CASES = [(3, 1), (130, 2), (67, 3)]
case = E.farmer_case


# ------------------------------------------------------------------ the restatement against HiGHS
@pytest.mark.parametrize("S,cm", LP_CASES)
def test_restatement_matches_highs_on_farmer(S, cm):
    sc, data, ref, ok, (obj, z) = case(S, cm)
    x, y = ref.solution()
    k = E.ef_kkt(sc, x, y, data)
    print(f"farmer S={S} cm={cm}: HiGHS {obj:.8f} restatement {ref.obj:.8f} rel {abs(ref.obj - obj) / abs(obj):.1e} "
          f"iterations {ref.it} z error {np.abs(ref.z.v - z).max():.1e} certificate {k['pres']:.1e} {k['dres']:.1e}")
    assert ok and ref.it <= 40
    assert abs(ref.obj - obj) <= OBJ_REL * abs(obj)
    assert k["pres"] <= 1e-6 and k["dres"] <= 1e-5            # the thresholds of tests/test_gpu_kkt.py
    assert abs(k["obj"] - obj) <= OBJ_REL * abs(obj)
    if (S, cm) == (3, 1):
        assert abs(obj + 108390.0) <= 1e-6 and np.abs(np.sort(ref.z.v) - [80.0, 170.0, 250.0]).max() <= 1e-5


def test_restatement_solves_the_farmer_qp():
    """quad = 0.01 on every column.  HiGHS's QP solver stops well short of the optimum here (its x
    is good to 1e-3, oracle/lpqp.py), so the restatement's objective may be BELOW it but not above
    by more than the bound, and the certificate decides."""
    sc, data, ref, ok, (obj, z) = case(3, 1, 0.01)
    x, y = ref.solution()
    k = E.ef_kkt(sc, x, y, data)
    print(f"farmer QP: HiGHS {obj:.8f} restatement {ref.obj:.8f} iterations {ref.it} z error {np.abs(ref.z.v - z).max():.1e}")
    assert ok and ref.qp and ref.it <= 40
    assert ref.obj - obj <= OBJ_REL * abs(obj) and abs(ref.obj - obj) <= 1e-6 * abs(obj)
    assert k["pres"] <= 1e-6 and k["dres"] <= 1e-5


def test_the_certificate_rejects_a_wrong_answer():
    sc, data, ref, _, _ = case(3, 1)
    x, y = ref.solution()
    assert E.ef_kkt(sc, x, 1.01 * y, data)["dres"] > 1e-5
    x2 = x.copy()
    x2[1, data[8][0]] += 1.0                                   # one scenario's copy of a nonant
    assert E.ef_kkt(sc, x2, y, data)["pres"] > 1e-6


# ------------------------------------------------------------------ the kernels' text on the host
def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if p:
            return p
    pytest.fail("no C++ compiler for tests/ef_host.cpp", pytrace=False)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("ef_host")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "mpi-sppy-1_amd", "csrc")]
    src = os.path.join(HERE, "ef_host.cpp")
    so = str(d / "libef_host.so")
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-fPIC", "-shared", *inc, "-o", so, src], check=True)
    exe = str(d / "ef_host")               # the same file as a stand-alone program (its own main)
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-DEF_HOST_MAIN", *inc, "-o", exe, src], check=True)
    assert subprocess.run([exe], capture_output=True, timeout=60).returncode == 0
    lib = ctypes.CDLL(so)
    lib.ef_host_solve.restype = ctypes.c_int
    return lib


def host_solve(lib, data, ref, tol=TOL, max_iter=100):
    A, rl, ru, lb, ub, c, q, p, idx = data
    S, m, n = A.shape
    nn = len(idx)
    row_ptr, col_idx, val = E.csr(data)
    T = lambda a: np.ascontiguousarray(a.T)  # noqa: E731
    P = lambda a, t=ctypes.c_double: a.ctypes.data_as(ctypes.POINTER(t))  # noqa: E731
    arrs = [T(val), T(c), T(q), T(lb), T(ub), T(rl), T(ru), np.ascontiguousarray(p)]
    zlb, zub = lb[:, idx].max(axis=0), ub[:, idx].min(axis=0)
    cz, qz = p @ c[:, idx], p @ q[:, idx]
    x, y, z = np.zeros((n, S)), np.zeros((m, S)), np.zeros(nn)
    first, info = np.zeros(nn * (nn + 1) // 2 + nn), np.zeros(8)
    nc = np.ascontiguousarray(idx, dtype=np.int32)
    st = lib.ef_host_solve(ctypes.c_int64(S), n, m, len(col_idx), nn, P(row_ptr, ctypes.c_int32), P(col_idx, ctypes.c_int32),
                           P(nc, ctypes.c_int32), *[P(a) for a in arrs], P(zlb), P(zub), P(cz), P(qz),
                           ctypes.c_double(ref.ncomp), ctypes.c_double(ref.cmax), ctypes.c_double(tol), int(ref.qp),
                           max_iter, P(x), P(y), P(z), P(first), P(info))
    return st, x.T, y.T, z, first, info


@pytest.mark.parametrize("S,cm,quad", [(3, 1, 0.0), (130, 2, 0.0), (67, 3, 0.0), (3, 1, 0.01)])
def test_host_kernels_follow_the_restatement(host, S, cm, quad):
    """The first scenario pass's C and right-hand side against the restatement's (both sum the same
    per-scenario terms, the host by LDL' and numpy by LU: 1e-10 of the largest entry, the
    conditioning of the starting N_s times the unit roundoff with room), then the whole solve."""
    sc, data, ref, ok, (obj, _) = case(S, cm, quad)
    st, x, y, z, first, info = host_solve(host, data, ref)
    nn = len(z)
    tri = np.tril_indices(nn)
    C, rhs = ref.first
    Cs = C.copy()
    Cs[np.arange(nn), np.arange(nn)] = np.diag(C) / (1.0 + E.EFRef.REG) - ref.qz - ref.theta0     # without Dz^-1
    assert np.abs(first[:len(tri[0])] - Cs[tri]).max() <= 1e-10 * np.abs(Cs).max()
    assert np.abs(first[len(tri[0]):] - (rhs + ref.rz0)).max() <= 1e-10 * max(1.0, np.abs(rhs + ref.rz0).max())
    k = E.ef_kkt(sc, x, y, data)
    print(f"host S={S} cm={cm} quad={quad}: status {st} iterations {info[0]:.0f} (restatement {ref.it}) objective {info[5]:.8f} "
          f"|z - restatement| {np.abs(z - ref.z.v).max():.1e} certificate {k['pres']:.1e} {k['dres']:.1e}")
    assert st == 0 and info[6] == 1.0
    assert info[0] <= 2 * ref.it
    assert abs(info[5] - ref.obj) <= OBJ_REL * abs(ref.obj)
    assert np.array_equal(x[:, data[8]], np.broadcast_to(z, (S, nn)))           # the nonants: the same bits everywhere
    assert k["pres"] <= 1e-6 and k["dres"] <= 1e-5


def test_host_iteration_limit_is_reported(host):
    sc, data, ref, _, _ = case(3, 1)
    st, *_, info = host_solve(host, data, ref, max_iter=2)
    assert st == 1 and info[6] == 0.0 and info[0] == 2


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
    for s in EF_SYMBOLS:
        m = re.search(rf"^int\s+{s}\s*\(([^;]*)\);", txt, re.M | re.S)
        assert m, s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS
        fn = getattr(L, s)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(m.group(1).split(",")), s          # one ctypes type per C argument


def test_null_handle_is_an_error(lib):
    from mpisppy_amd import _lib
    L = _lib.load()
    n = None
    assert L.phgpu_ef_init(n, n, n, n, n, 1.0, 1.0, 1e-8, 0, n) == -1
    assert L.phgpu_ef_schur(n, 0, n, n, n) == -1
    assert L.phgpu_ef_direction(n, 0, n, n, n, n) == -1
    assert L.phgpu_ef_step(n, 0, n, n, n) == -1
    assert L.phgpu_ef_export(n, n, n, n, n, n, n, n, n) == -1
    assert "null" in _lib.last_error()


# ------------------------------------------------------------------ the classes' surface and refusals
SOLVER = "mi355x_pdhg"


def _farmer(cls, S=3, options=None, creator=None, **kw):
    from mpisppy_amd.examples import farmer
    o = {"solver": SOLVER, "toc": False}
    o.update(options or {})
    return cls(o, farmer.scenario_names_creator(S), creator or farmer.scenario_creator,
               scenario_creator_kwargs={"num_scens": S}, **kw)


def test_python_surface():
    from mpisppy_amd.confidence_intervals.ciutils import ef_xstar_solver
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.opt.ef import ExtensiveForm
    from mpisppy_amd.opt.sc import SchurComplement
    from mpisppy_amd.spbase import SPBase
    for m in ("ef_init", "ef_schur", "ef_direction", "ef_step", "ef_iteration", "ef_read", "ef_export"):
        assert callable(getattr(PHEngine, m)), m
    for m in ("solve_extensive_form", "get_objective_value", "get_root_solution", "nonants", "nonants_to_csv", "scenarios"):
        assert callable(getattr(ExtensiveForm, m)), m
    assert callable(SchurComplement.solve) and callable(ef_xstar_solver("mpisppy_amd.examples.farmer"))
    assert callable(SPBase.gather_var_values_to_rank0) and callable(SPBase.report_var_values_at_rank0)


def test_constructor_and_option_errors():
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.ef import ExtensiveForm
    from mpisppy_amd.opt.sc import SchurComplement
    with pytest.raises(ValueError, match="solver"):
        ExtensiveForm({"toc": False}, farmer.scenario_names_creator(3), farmer.scenario_creator,
                      scenario_creator_kwargs={"num_scens": 3})
    with pytest.raises(RuntimeError, match="not served"):
        _farmer(ExtensiveForm, options={"solver": "gurobi"})
    with pytest.raises(NotImplementedError, match="bundles"):
        _farmer(ExtensiveForm, options={"bundles_per_rank": 2})
    with pytest.raises(ValueError, match="does not support bundling"):
        _farmer(SchurComplement, options={"bundles_per_rank": 2})
    with pytest.raises(NotImplementedError, match="shared-matrix"):
        _farmer(SchurComplement, options={"shared_matrix": True})
    ef = _farmer(ExtensiveForm)
    assert not ef.first_stage_solution_available and not ef.tree_solution_available
    assert [nm for nm, _ in ef.scenarios()] == ["scen0", "scen1", "scen2"]
    with pytest.raises(ValueError, match="not been solved"):
        ef.get_objective_value()
    with pytest.raises(ValueError, match="not served"):
        ef.solve_extensive_form(solver_options={"Method": 2})


def test_a_multistage_tree_is_refused():
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.opt.sc import SchurComplement
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    bfs = [2, 2]
    with pytest.raises(RuntimeError, match="two-stage"):
        SchurComplement({"toc": False}, aircond.scenario_names_creator(4), aircond.scenario_creator,
                        all_nodenames=create_nodenames_from_branching_factors(bfs),
                        scenario_creator_kwargs={"branching_factors": bfs, "start_seed": 1134})


def test_problems_without_an_interior_are_refused():
    """A nonant whose tightest bounds coincide; a first-stage row with equal sides."""
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.sc import SchurComplement

    def pinned(name, **kw):
        m = farmer.scenario_creator(name, **kw)
        j = m.find_var("DevotedAcreage[CORN0]").index
        m.lb[j] = m.ub[j] = 80.0 if name == "scen0" else m.lb[j]
        if name != "scen0":
            m.ub[j] = 80.0                     # scen0 fixes it at 80, the others cap it there
        return m

    def acreage_equality(name, **kw):
        m = farmer.scenario_creator(name, **kw)
        terms, _, ru, nm = m.rows[0]
        m.rows[0] = (terms, ru, ru, nm)
        return m

    with pytest.raises(NotImplementedError, match="nonant 0 has the bounds"):
        _farmer(SchurComplement, creator=pinned)._problem_data()
    with pytest.raises(NotImplementedError, match="only nonant columns and equal sides"):
        _farmer(SchurComplement, creator=acreage_equality)._problem_data()
    zlb, zub, cz, qz, ncomp, cmax, qp = _farmer(SchurComplement)._problem_data()
    assert np.all(zlb == 0.0) and np.all(zub == 500.0) and not qp and cmax == 100000.0
    assert np.allclose(np.sort(cz), [150.0, 230.0, 260.0])
