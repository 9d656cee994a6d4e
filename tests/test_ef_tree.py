"""The multistage extensive form without a GPU: what ExtensiveForm accepts and
refuses on a tree, the numpy restatement (tests/ef_tree_ref.py) against HiGHS, and the kernels' own
text run on the host (tests/ef_tree_host.cpp): the elimination alone against numpy on random
systems with tree sparsity, then the whole solve against the restatement and HiGHS."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ef_tree_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "include", "phgpu.h")
LIB = os.path.join(ROOT, "mpi-sppy-1_amd", "mpisppy_amd", "libphgpu.so")
EFT_SYMBOLS = ["phgpu_eft_init", "phgpu_eft_schur", "phgpu_eft_direction", "phgpu_eft_step", "phgpu_eft_export"]
REL = 1e-5                  # the project's standing relative objective bar
# HiGHS on this machine, start_seed = 0, default aircond arguments: a check of the assembly
HIGHS = {(2, 2): 585.7299917, (3, 2): 600.6908515, (4, 3, 2): 969.3521891}
TREES = [((2, 2), 0.0), ((3, 2), 0.0), ((4, 3, 2), 0.0), ((3, 2), 0.3)]


aircond_opt, case = R.aircond_opt, R.case


# ------------------------------------------------------------------ the classes on a tree
def test_extensive_form_takes_a_tree_and_gives_per_node_data():
    from mpisppy_amd.opt.ef import ExtensiveForm
    ef = aircond_opt(ExtensiveForm, (2, 2))
    b = ef.batch
    assert b.depth == 2 and len(b.node_names) == 3 and b.nn == 4
    (nlens, depth, parent, seg_start), zlb, zub, cz, qz, ncomp, cmax, qp = ef._problem_data()
    assert list(nlens) == [2, 2] and list(depth) == [0, 1, 1] and list(parent) == [-1, 0, 0] and list(seg_start) == [0, 2, 4]
    lay = R.Layout(b)
    want = R.z_data(b, lay)
    for got, w in zip((zlb, zub, cz, qz), want):
        assert got.shape == (6,) and np.array_equal(got, w)
    assert np.allclose(cz[:2], b.prob @ b.c[:, b.nonant_col[:2]])                  # ROOT: over all scenarios
    assert np.allclose(cz[2:4], b.prob[:2] @ b.c[:2][:, b.nonant_col[2:]])          # ROOT_0: over its two
    assert not qp and cmax == np.abs(b.c).max() and ncomp == R.TreeEFRef(b).ncomp
    assert not ef.first_stage_solution_available and not ef.tree_solution_available
    with pytest.raises(ValueError, match="not been solved"):
        list(ef.nonants())


def test_schur_complement_still_refuses_a_tree():
    from mpisppy_amd.opt.sc import SchurComplement
    with pytest.raises(RuntimeError, match="two-stage"):
        aircond_opt(SchurComplement, (2, 2))


def test_a_scenario_order_that_splits_a_node_is_refused():
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.opt.ef import ExtensiveForm
    n = aircond.scenario_names_creator(4)
    ef = aircond_opt(ExtensiveForm, (2, 2), names=[n[0], n[2], n[1], n[3]])
    with pytest.raises(RuntimeError, match="not in tree order: the scenarios of node ROOT_0 are not contiguous"):
        ef._problem_data()


def test_entries_declared_exported_and_typed():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build(verbose=False)
    lib = ctypes.CDLL(LIB)
    txt = open(HDR).read()
    from mpisppy_amd import _lib
    from mpisppy_amd.engine import PHEngine
    L = _lib.load()
    for s in EFT_SYMBOLS:
        m = re.search(rf"^int\s+{s}\s*\(([^;]*)\);", txt, re.M | re.S)
        assert m and hasattr(lib, s) and s in _lib.EXPORTS, s
        fn = getattr(L, s)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(m.group(1).split(",")), s
    n = None
    assert L.phgpu_eft_init(n, 2, n, 3, n, n, n, n, n, n, n, 1.0, 1.0, 1e-8, 0, n) == -1
    assert L.phgpu_eft_schur(n, 0, n, n, n) == -1 and L.phgpu_eft_direction(n, 0, n, n) == -1
    assert L.phgpu_eft_step(n, 0, n) == -1 and L.phgpu_eft_export(n, n, n, n, n, n, n, n, n) == -1
    for m in ("eft_init", "eft_schur", "eft_direction", "eft_step", "eft_iteration", "eft_read", "eft_export"):
        assert callable(getattr(PHEngine, m)), m


# ------------------------------------------------------------------ the restatement against HiGHS
@pytest.mark.parametrize("bfs,quad", TREES)
def test_restatement_matches_highs_on_aircond_trees(bfs, quad):
    b, ref, ok, (obj, _) = case(bfs, quad)
    got = ref.obj + ref.const
    x, y = ref.solution()
    k = R.tree_kkt(b, x, y)
    print(f"aircond {bfs} quad={quad}: HiGHS {obj:.7f} restatement {got:.7f} rel {abs(got - obj) / abs(obj):.1e} "
          f"iterations {ref.it} certificate {k['pres']:.1e} {k['dres']:.1e}")
    if not quad:
        assert abs(obj - HIGHS[bfs]) <= 1e-6
    assert ok and ref.it < ref.max_iter
    assert abs(got - obj) <= REL * abs(obj)
    assert k["pres"] <= 1e-6 and k["dres"] <= 1e-5
    slot = np.full(b.n, -1)                     # none has a row made of nonant columns only
    slot[b.nonant_col] = np.arange(b.nn)
    assert all(np.any(slot[b.col_idx[b.row_ptr[i]:b.row_ptr[i + 1]]] < 0) for i in range(b.m))


# ------------------------------------------------------------------ the kernels' text on the host
def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if p:
            return p
    pytest.fail("no C++ compiler for tests/ef_tree_host.cpp", pytrace=False)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("ef_tree_host")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "mpi-sppy-1_amd", "csrc")]
    src = os.path.join(HERE, "ef_tree_host.cpp")
    so = str(d / "libef_tree_host.so")
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-fPIC", "-shared", *inc, "-o", so, src], check=True)
    exe = str(d / "ef_tree_host")          # the same file as a stand-alone program (its own main)
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-DEF_TREE_HOST_MAIN", *inc, "-o", exe, src], check=True)
    assert subprocess.run([exe], capture_output=True, timeout=60).returncode == 0
    lib = ctypes.CDLL(so)
    lib.eft_host_linear.restype = ctypes.c_int
    lib.eft_host_solve.restype = ctypes.c_int
    return lib


def P(a, t=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _tree(bfs):
    """(node_depth, node_parent) of the non-leaf nodes of a tree with the branching factors bfs (the
    last one is the leaves'), numbered depth by depth with siblings adjacent."""
    depth, parent, level = [0], [-1], [0]
    for d, bf in enumerate(bfs[:-1], start=1):
        nxt = []
        for p in level:
            for _ in range(bf):
                nxt.append(len(depth))
                depth.append(d)
                parent.append(p)
        level = nxt
    return np.array(depth, dtype=np.int32), np.array(parent, dtype=np.int32)


@pytest.mark.parametrize("nlens,bfs", [([3, 1], [3, 1]), ([3, 1, 2], [4, 3, 1])])
def test_host_elimination_against_numpy(host, nlens, bfs):
    """Random symmetric positive definite systems with tree sparsity: every node's summed matrix
    and right-hand side against a numpy dense assembly (1e-10 relative, the bar of test_ef.py), and
    the relative residual of the tree solve against what numpy.linalg.solve leaves on the same dense
    system, with a factor 100 of room for the different elimination orders."""
    rng = np.random.default_rng(7)
    depth, parent = _tree(bfs)
    nl = np.array(nlens, dtype=np.int32)
    D, Nn, nn = len(nlens), len(depth), int(sum(nlens))
    zoff = np.concatenate([[0], np.cumsum(nl[depth])])
    Ztot = int(zoff[-1])

    def path(n):
        out = []
        while n >= 0:
            out = list(range(zoff[n], zoff[n + 1])) + out
            n = parent[n]
        return np.array(out)
    deep = np.flatnonzero(depth == D - 1)
    G = len(deep)
    B = rng.standard_normal((G, nn, nn + 2))
    segA = np.einsum("gik,gjk->gij", B, B)
    segb = rng.standard_normal((G, nn))
    dd, rr = rng.uniform(0.5, 2.0, Ztot), rng.standard_normal(Ztot)
    C, r = np.diag(dd), rr.copy()
    for g, n in enumerate(deep):
        C[np.ix_(path(n), path(n))] += segA[g]
        r[path(n)] += segb[g]
    nodeA, nodeb, dz = np.zeros((Nn, nn, nn)), np.zeros((Nn, nn)), np.zeros(Ztot)
    assert host.eft_host_linear(D, P(nl, ctypes.c_int32), Nn, P(depth, ctypes.c_int32), P(parent, ctypes.c_int32),
                                P(np.ascontiguousarray(np.tril(segA))), P(segb), P(dd), P(rr), P(nodeA), P(nodeb), P(dz)) == 0
    # per node: the Schur complement onto its path of everything strictly below it
    worst = 0.0
    for n in range(Nn):
        pth = path(n)
        below = [k for g, m in enumerate(deep) if n in _ancestors(m, parent) for k in path(m) if k not in pth]
        below = np.array(sorted(set(below)), dtype=np.int64)
        Cn, rn = np.zeros((Ztot, Ztot)), np.zeros(Ztot)
        Cn[below, below] = dd[below]
        rn[below] = rr[below]
        for g, m in enumerate(deep):
            if n in _ancestors(m, parent):
                Cn[np.ix_(path(m), path(m))] += segA[g]
                rn[path(m)] += segb[g]
        A, bb = Cn[np.ix_(pth, pth)], rn[pth]
        if len(below):
            X = np.linalg.solve(Cn[np.ix_(below, below)], np.column_stack([Cn[np.ix_(below, pth)], rn[below]]))
            A = A - Cn[np.ix_(pth, below)] @ X[:, :-1]
            bb = bb - Cn[np.ix_(pth, below)] @ X[:, -1]
        Pd = len(pth)
        ea = np.abs(np.tril(nodeA[n, :Pd, :Pd]) - np.tril(A)).max() / np.abs(A).max()
        eb = np.abs(nodeb[n, :Pd] - bb).max() / max(1.0, np.abs(bb).max())
        worst = max(worst, ea, eb)
    res_tree = np.linalg.norm(C @ dz - r) / np.linalg.norm(r)
    res_np = np.linalg.norm(C @ np.linalg.solve(C, r) - r) / np.linalg.norm(r)
    print(f"nlens {nlens} tree {bfs[:-1]}: {Nn} nodes, Ztot {Ztot}; per-node sums worst relative error {worst:.1e}; "
          f"residual tree {res_tree:.2e} numpy {res_np:.2e}")
    assert worst <= 1e-10
    assert res_tree <= 100.0 * res_np


def _ancestors(n, parent):
    out = set()
    while n >= 0:
        out.add(n)
        n = parent[n]
    return out


def host_solve(lib, ef, ref, tol=1e-8, max_iter=100):
    b = ef.batch
    (nlens, depth, parent, seg_start), zlb, zub, cz, qz, ncomp, cmax, qp = ef._problem_data()
    T = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)  # noqa: E731
    arrs = [T(b.A_val), T(b.c), T(b.q), T(b.lb), T(b.ub), T(b.rl), T(b.ru), np.ascontiguousarray(b.prob)]
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    row_ptr, col_idx, nc = i4(b.row_ptr), i4(b.col_idx), i4(b.nonant_col)
    Nn, Ztot = len(depth), len(zlb)
    x, y, z = np.zeros((b.n, b.S)), np.zeros((b.m, b.S)), np.zeros(Ztot)
    nodeA, nodeb, info = np.zeros((Nn, b.nn, b.nn)), np.zeros((Nn, b.nn)), np.zeros(8)
    st = lib.eft_host_solve(ctypes.c_int64(b.S), b.n, b.m, len(col_idx), b.nn, P(row_ptr, ctypes.c_int32),
                            P(col_idx, ctypes.c_int32), P(nc, ctypes.c_int32), *[P(a) for a in arrs], len(nlens),
                            P(i4(nlens), ctypes.c_int32), Nn, P(i4(depth), ctypes.c_int32), P(i4(parent), ctypes.c_int32),
                            P(i4(seg_start), ctypes.c_int32), P(zlb), P(zub), P(cz), P(qz), ctypes.c_double(ncomp),
                            ctypes.c_double(cmax), ctypes.c_double(tol), int(qp), max_iter, P(x), P(y), P(z), P(nodeA),
                            P(nodeb), P(info))
    return st, x.T, y.T, z, nodeA, nodeb, info


def check_node_systems(ref, nodeA, nodeb):
    """every node's first matrix and right-hand side against the restatement's elimination, 1e-10
    relative to the matrix's (the vector's) largest entry"""
    worst = 0.0
    for n, (A, bb) in ref.node_systems().items():
        Pd = len(bb)
        worst = max(worst, np.abs(np.tril(nodeA[n, :Pd, :Pd]) - np.tril(A)).max() / np.abs(A).max(),
                    np.abs(nodeb[n, :Pd] - bb).max() / max(1.0, np.abs(bb).max()))
    return worst


@pytest.mark.parametrize("bfs,quad", TREES + [((3, 5, 10), 0.0)])
def test_host_kernels_follow_the_restatement(host, bfs, quad):
    from mpisppy_amd.opt.ef import ExtensiveForm
    b, ref, ok, (obj, _) = case(bfs, quad)
    ef = aircond_opt(ExtensiveForm, bfs, quad)
    st, x, y, z, nodeA, nodeb, info = host_solve(host, ef, ref)
    worst = check_node_systems(ref, nodeA, nodeb)
    got = info[5] + ref.const
    k = R.tree_kkt(b, x, y)
    print(f"host aircond {bfs} quad={quad}: status {st} iterations {info[0]:.0f} (restatement {ref.it}) objective {got:.7f} "
          f"HiGHS {obj:.7f} |z - restatement| {np.abs(z - ref.z.v).max():.1e} node systems {worst:.1e} "
          f"certificate {k['pres']:.1e} {k['dres']:.1e}")
    assert ok and st == 0 and info[6] == 1.0
    assert worst <= 1e-10
    assert info[0] <= 2 * ref.it
    assert abs(got - obj) <= REL * abs(obj)
    assert np.array_equal(x[:, b.nonant_col], z[ref.lay.zidx])            # the nonants: the node's bits in every scenario
    assert k["pres"] <= 1e-6 and k["dres"] <= 1e-5


def test_host_solve_on_the_synthetic_tree(host):
    """nlens = [3, 1, 2] over a 2,3,2 tree, boxed columns and ranged rows around a known feasible
    point: the offsets differ by depth, and a middle level both receives and gives."""
    ef, b, ref, ok, (obj, _) = R.synthetic_case()
    st, x, y, z, nodeA, nodeb, info = host_solve(host, ef, ref)
    worst = check_node_systems(ref, nodeA, nodeb)
    k = R.tree_kkt(b, x, y)
    print(f"host synthetic: status {st} iterations {info[0]:.0f} (restatement {ref.it}) objective {info[5]:.7f} HiGHS {obj:.7f} "
          f"node systems {worst:.1e} certificate {k['pres']:.1e} {k['dres']:.1e}")
    assert ok and st == 0 and info[6] == 1.0 and worst <= 1e-10 and info[0] <= 2 * ref.it
    assert abs(info[5] - obj) <= REL * abs(obj)
    assert np.array_equal(x[:, b.nonant_col], z[ref.lay.zidx])
    assert k["pres"] <= 1e-6 and k["dres"] <= 1e-5
