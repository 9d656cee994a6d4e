"""The conditioned multistage extensive form without a GPU: z entries held at values
(phgpu_eft_fix).  The kernels' own text on the host (tests/ef_cond_host.cpp): the elimination with
held entries against a dense numpy assembly, then the whole conditioned solve against HiGHS and the
restatement (tests/ef_cond_ref.py); what ExtensiveForm.fix_node_nonants takes and refuses; the new
entry's declaration and export."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ef_cond_ref as C
import ef_tree_ref as R
from test_ef_tree import HDR, HERE, LIB, P, REL, ROOT, _ancestors, _compiler, _tree

NAN = float("nan")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("ef_cond_host")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "mpi-sppy-1_amd", "csrc")]
    src = os.path.join(HERE, "ef_cond_host.cpp")
    so = str(d / "libef_cond_host.so")
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-fPIC", "-shared", *inc, "-o", so, src], check=True)
    exe = str(d / "ef_cond_host")          # the same file as a stand-alone program (its own main)
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-DEF_COND_HOST_MAIN", *inc, "-o", exe, src], check=True)
    assert subprocess.run([exe], capture_output=True, timeout=60).returncode == 0
    lib = ctypes.CDLL(so)
    lib.eft_cond_host_linear.restype = ctypes.c_int
    lib.eft_cond_host_solve.restype = ctypes.c_int
    return lib


# ------------------------------------------------------------------ the elimination alone
# (nlens, branching factors with the leaves' last, held z entries): the synthetic shape with ROOT's
# middle entry and all of depth-1 node 1 (its one entry, z index 3); aircond (2,2) with all of ROOT;
# the synthetic shape with a deepest node and an entry of another held; everything held
LINEAR = [([3, 1, 2], [2, 3, 1], [1, 3]), ([2, 2], [2, 1], [0, 1]), ([3, 1, 2], [2, 3, 1], [5, 6, 10]),
          ([3, 1, 2], [2, 3, 1], list(range(17)))]


@pytest.mark.parametrize("nlens,bfs,held", LINEAR)
def test_host_conditioned_elimination_against_numpy(host, nlens, bfs, held):
    """Random symmetric positive definite systems with tree sparsity and held entries: every node's
    summed matrix and right-hand side against a dense numpy assembly in which a held entry's row and
    column are the identity's and its right-hand side 0 (1e-10 relative), dz of the held entries
    exactly 0.0, and the residual of the tree solve on that dense system against numpy's own."""
    rng = np.random.default_rng(11)
    depth, parent = _tree(bfs)
    nl = np.array(nlens, dtype=np.int32)
    D, Nn, nn = len(nlens), len(depth), int(sum(nlens))
    zoff = np.concatenate([[0], np.cumsum(nl[depth])])
    Ztot = int(zoff[-1])
    hm = np.zeros(Ztot, dtype=np.int32)
    hm[held] = 1
    hb = hm.astype(bool)

    def path(n):
        out = []
        while n >= 0:
            out = list(range(zoff[n], zoff[n + 1])) + out
            n = parent[n]
        return np.array(out)

    def hold(Cm, r, idx):
        for k in idx:
            Cm[k, :] = 0.0
            Cm[:, k] = 0.0
            Cm[k, k] = 1.0
            r[k] = 0.0
    deep = np.flatnonzero(depth == D - 1)
    G = len(deep)
    B = rng.standard_normal((G, nn, nn + 2))
    segA = np.einsum("gik,gjk->gij", B, B)
    segb = rng.standard_normal((G, nn))
    dd, rr = rng.uniform(0.5, 2.0, Ztot), rng.standard_normal(Ztot)
    Cd, r = np.diag(dd), rr.copy()
    for g, n in enumerate(deep):
        Cd[np.ix_(path(n), path(n))] += segA[g]
        r[path(n)] += segb[g]
    hold(Cd, r, np.flatnonzero(hb))
    nodeA, nodeb, dz = np.zeros((Nn, nn, nn)), np.zeros((Nn, nn)), np.zeros(Ztot)
    assert host.eft_cond_host_linear(D, P(nl, ctypes.c_int32), Nn, P(depth, ctypes.c_int32), P(parent, ctypes.c_int32),
                                     P(np.ascontiguousarray(np.tril(segA))), P(segb), P(dd), P(rr), P(hm, ctypes.c_int32),
                                     P(nodeA), P(nodeb), P(dz)) == 0
    worst = 0.0
    for n in range(Nn):              # per node: the Schur complement onto its path of everything strictly below it
        pth = path(n)
        below = [k for m in deep if n in _ancestors(m, parent) for k in path(m) if k not in pth]
        below = np.array(sorted(set(below)), dtype=np.int64)
        Cn, rn = np.zeros((Ztot, Ztot)), np.zeros(Ztot)
        Cn[below, below] = dd[below]
        rn[below] = rr[below]
        for g, m in enumerate(deep):
            if n in _ancestors(m, parent):
                Cn[np.ix_(path(m), path(m))] += segA[g]
                rn[path(m)] += segb[g]
        hold(Cn, rn, [k for k in below if hb[k]])
        A, bb = Cn[np.ix_(pth, pth)], rn[pth]
        if len(below):
            X = np.linalg.solve(Cn[np.ix_(below, below)], np.column_stack([Cn[np.ix_(below, pth)], rn[below]]))
            A = A - Cn[np.ix_(pth, below)] @ X[:, :-1]
            bb = bb - Cn[np.ix_(pth, below)] @ X[:, -1]
        Pd = len(pth)
        worst = max(worst, np.abs(np.tril(nodeA[n, :Pd, :Pd]) - np.tril(A)).max() / np.abs(A).max(),
                    np.abs(nodeb[n, :Pd] - bb).max() / max(1.0, np.abs(bb).max()))
    nr = max(np.linalg.norm(r), 1.0)
    res_tree = np.linalg.norm(Cd @ dz - r) / nr
    res_np = np.linalg.norm(Cd @ np.linalg.solve(Cd, r) - r) / nr
    print(f"nlens {nlens} tree {bfs[:-1]} held {held}: per-node sums worst relative error {worst:.1e}; residual tree "
          f"{res_tree:.2e} numpy {res_np:.2e}; held dz {dz[hb]}")
    assert worst <= 1e-10
    assert np.all(dz[hb] == 0.0) and not np.any(np.signbit(dz[hb]))
    # (the diagonal's relative regularisation of 1e-13 is in the tree solve and not in the dense system)
    assert res_tree <= max(100.0 * res_np, 1e-11)


# ------------------------------------------------------------------ the whole conditioned solve
def cond_host_solve(lib, ef, zfix, tol=1e-8, max_iter=100):
    b = ef.batch
    ef.free_node_nonants()
    (nlens, depth, parent, seg_start), zlb, zub, cz, qz, ncomp, cmax, qp = ef._problem_data()
    T = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)  # noqa: E731
    arrs = [T(b.A_val), T(b.c), T(b.q), T(b.lb), T(b.ub), T(b.rl), T(b.ru), np.ascontiguousarray(b.prob)]
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    row_ptr, col_idx, nc = i4(b.row_ptr), i4(b.col_idx), i4(b.nonant_col)
    Nn, Ztot = len(depth), len(zlb)
    x, y, z = np.zeros((b.n, b.S)), np.zeros((b.m, b.S)), np.zeros(Ztot)
    nodeA, nodeb, info, hdz = np.zeros((Nn, b.nn, b.nn)), np.zeros((Nn, b.nn)), np.zeros(8), np.full(1, -1.0)
    zfix = np.ascontiguousarray(zfix, dtype=np.float64)
    st = lib.eft_cond_host_solve(ctypes.c_int64(b.S), b.n, b.m, len(col_idx), b.nn, P(row_ptr, ctypes.c_int32),
                                 P(col_idx, ctypes.c_int32), P(nc, ctypes.c_int32), *[P(a) for a in arrs], len(nlens),
                                 P(i4(nlens), ctypes.c_int32), Nn, P(i4(depth), ctypes.c_int32), P(i4(parent), ctypes.c_int32),
                                 P(i4(seg_start), ctypes.c_int32), P(zlb), P(zub), P(cz), P(qz), ctypes.c_double(ncomp),
                                 ctypes.c_double(cmax), ctypes.c_double(tol), int(qp), max_iter, P(x), P(y), P(z), P(nodeA),
                                 P(nodeb), P(info), P(zfix), P(hdz))
    return st, x.T, y.T, z, info, float(hdz[0])


def check_cond_host(host, ef, key, zfix, const=0.0):
    b = ef.batch
    case = C.cond_case(key, b, zfix)
    assert case["ok"], "HiGHS finds the conditioned problem infeasible, or the restatement did not converge"
    ref, obj, lay = case["ref"], case["obj"], case["lay"]
    held = ~np.isnan(zfix)
    st, x, y, z, info, hdz = cond_host_solve(host, ef, zfix)
    k = C.cond_kkt(b, x, y, zfix)
    got = info[5] + const
    print(f"host {key}: status {st} iterations {info[0]:.0f} (restatement {ref.it}) objective {got:.7f} HiGHS {obj:.7f} "
          f"restatement {ref.obj + ref.const:.7f} held dz {hdz} certificate {k['pres']:.1e} {k['dres']:.1e}")
    assert st == 0 and info[6] == 1.0
    assert hdz == 0.0                                                      # dz of the held entries: exactly 0
    assert info[0] <= 2 * ref.it
    assert abs(ref.obj + ref.const - obj) <= REL * abs(obj)                # the restated solve to HiGHS's objective
    assert abs(got - obj) <= REL * abs(obj)
    assert np.array_equal(z[held], zfix[held])                             # the held values: bit for bit
    assert np.array_equal(x[:, b.nonant_col], z[lay.zidx])
    assert k["pres"] <= 1e-6 and k["dres"] <= 1e-5


def test_host_conditioned_solve_on_the_synthetic_tree(host):
    """nlens = [3, 1, 2] over a 2,3,2 tree: ROOT's middle entry and all of depth-1 node ROOT_1 held, at
    the midpoint between the bounds' centre and HiGHS's unconditioned optimum (inside the bounds;
    whether the rows allow it is what ``ok`` says)."""
    ef, b, _, _, (_, zopt) = R.synthetic_case()
    lay = R.Layout(b)
    zlb, zub, _, _ = R.z_data(b, lay)
    v = 0.5 * (zopt + 0.5 * (zlb + zub))
    zfix = np.full(lay.Ztot, NAN)
    zfix[[1, 3]] = v[[1, 3]]
    check_cond_host(host, ef, "synthetic/root1+node2", zfix)


def test_host_conditioned_solve_on_aircond_with_root_held(host):
    from mpisppy_amd.opt.ef import ExtensiveForm
    ef = R.aircond_opt(ExtensiveForm, (2, 2))
    lay = R.Layout(ef.batch)
    zfix = C.zfix_of(lay, ef.batch.node_names, {"ROOT": [150.0, 20.0]})
    const = float(ef.batch.prob @ ef.batch.obj_const)
    check_cond_host(host, ef, "aircond22/root", zfix, const)


# ------------------------------------------------------------------ ExtensiveForm.fix_node_nonants
def test_fix_node_nonants_takes_a_cache_and_refuses_what_it_cannot_hold():
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.ef import ExtensiveForm
    ef = R.aircond_opt(ExtensiveForm, (3, 2, 2))
    assert ef._held_z() is None
    ef.fix_node_nonants({"ROOT": [NAN, 5.0], "ROOT_1": [7.0, NAN], "ROOT_2_1": None})
    z = ef._held_z()
    lay = R.Layout(ef.batch)
    assert z.shape == (lay.Ztot,) and np.isnan(z[0]) and z[1] == 5.0
    n = list(ef.batch.node_names).index("ROOT_1")
    assert z[lay.zoff[n]] == 7.0 and np.isnan(z[lay.zoff[n] + 1]) and np.count_nonzero(~np.isnan(z)) == 2
    data = ef._problem_data()                       # (ncomp as phgpu_eft_init takes it: phgpu_eft_fix leaves the held out)
    assert data[5] == R.TreeEFRef(ef.batch).ncomp
    ef.free_node_nonants()
    assert ef._held_z() is None
    ef.fix_node_nonants({"ROOT": [NAN, NAN]})
    assert ef._held_z() is None
    with pytest.raises(RuntimeError, match="not a non-leaf node"):
        ef.fix_node_nonants({"ROOT_9": [1.0, 2.0]})
    with pytest.raises(RuntimeError, match="has 2 nonants, 3 values"):
        ef.fix_node_nonants({"ROOT": [1.0, 2.0, 3.0]})
    with pytest.raises(ValueError, match="not been solved"):
        ef.node_objectives(1)
    two = ExtensiveForm({"solver": R.SOLVER, "toc": False}, farmer.scenario_names_creator(3), farmer.scenario_creator,
                        scenario_creator_kwargs={"num_scens": 3})
    with pytest.raises(NotImplementedError, match="multistage"):
        two.fix_node_nonants({"ROOT": [1.0, 2.0, 3.0]})


def test_a_shut_column_is_refused_unless_it_is_held():
    from mpisppy_amd.opt.ef import ExtensiveForm
    ef = R.aircond_opt(ExtensiveForm, (2, 2))
    j = ef.batch.nonant_col[1]
    ef.batch.lb[:, j] = ef.batch.ub[:, j] = 0.0          # OvertimeProd of stage 1 shut in every scenario
    with pytest.raises(NotImplementedError, match="nonant 1 of node ROOT .* no interior"):
        ef._problem_data()
    ef.fix_node_nonants({"ROOT": [NAN, 0.0]})
    _, zlb, zub = ef._problem_data()[:3]
    assert zlb[1] < 0.0 < zub[1]                         # (what phgpu_eft_init is given around the held value)


# ------------------------------------------------------------------ the entry
def test_eft_fix_declared_exported_and_typed():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build(verbose=False)
    lib = ctypes.CDLL(LIB)
    txt = open(HDR).read()
    from mpisppy_amd import _lib
    from mpisppy_amd.engine import PHEngine
    L = _lib.load()
    m = re.search(r"^int\s+phgpu_eft_fix\s*\(([^;]*)\);", txt, re.M | re.S)
    assert m and hasattr(lib, "phgpu_eft_fix") and "phgpu_eft_fix" in _lib.EXPORTS
    fn = L.phgpu_eft_fix
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(m.group(1).split(",")) == 3
    assert L.phgpu_eft_fix(None, None, None) == -1
    assert callable(PHEngine.eft_fix)
