"""The master LP's arithmetic on the host: csrc/ph_lshaped.inc compiled for one thread (LS_HOST,
tests/lshaped_host.cpp) against HiGHS on the masters of the restatement's farmer runs and on the
constructed ones of tests/test_gpu_lshaped.py.  The device runs the same text with 256 threads."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import lshaped_ref as R
from oracle.models import farmer_scenario

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REL = 1e-9          # a tenth of the method's default tol (1e-8): what that default rests on
FEAS = 1e-7


def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if p:
            return p
    pytest.fail("no C++ compiler for tests/lshaped_host.cpp", pytrace=False)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("lshaped_host")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "mpi-sppy-1_amd", "csrc")]
    src = os.path.join(HERE, "lshaped_host.cpp")
    so = str(d / "liblshaped_host.so")
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-fPIC", "-shared", *inc, "-o", so, src], check=True)
    # the same file as a stand-alone program (its own main: a feasible and an infeasible master)
    exe = str(d / "lshaped_host")
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-DLS_HOST_MAIN", *inc, "-o", exe, src], check=True)
    assert subprocess.run([exe], capture_output=True, timeout=60).returncode == 0
    return ctypes.CDLL(so)


def _solve(lib, nn, G, cuts, Rr, rl, ru, xlb, xub, etalb, max_cuts=None, x0=None):
    P = lambda a, t=ctypes.c_double: a.ctypes.data_as(ctypes.POINTER(t))  # noqa: E731
    K = len(cuts)
    grp = np.array([c[0] for c in cuts] + [0], dtype=np.int32)
    a = np.ascontiguousarray(np.array([c[1] for c in cuts] + [np.zeros(nn)], float))
    b = np.array([c[2] for c in cuts] + [0.0], float)
    Rr = np.ascontiguousarray(Rr, float).reshape(-1, nn) if len(rl) else np.zeros((1, nn))
    rl_, ru_ = np.array(list(rl) + [0.0], float), np.array(list(ru) + [0.0], float)
    z, info = np.zeros(nn + G), np.zeros(6)
    x0 = np.zeros(nn) if x0 is None else np.ascontiguousarray(x0, float)
    xlb, xub, etalb = (np.ascontiguousarray(v, float) for v in (xlb, xub, etalb))
    lib.ls_host_master(nn, G, max_cuts or max(K, 1), K, P(grp, ctypes.c_int32), P(a), P(b), len(rl), P(Rr), P(rl_),
                       P(ru_), P(xlb), P(xub), P(etalb), P(x0), ctypes.c_double(1e-9), P(z), P(info))
    return z, info


def _check(lib, name, nn, G, cuts, Rr, rl, ru, xlb, xub, etalb, **kw):
    x, eta, obj, st = R.solve_master(nn, G, cuts, Rr, rl, ru, xlb, xub, etalb)
    assert st == 0
    z, info = _solve(lib, nn, G, cuts, Rr, rl, ru, xlb, xub, etalb, **kw)
    rel = abs(info[0] - obj) / max(1.0, abs(obj))
    viol = R.master_violation(z, nn, G, cuts, Rr, rl, ru, xlb, xub, etalb)
    print(f"{name}: {len(cuts)} cuts, HiGHS {obj:.10f} host {info[0]:.10f} rel {rel:.2e} violation {viol:.1e} "
          f"iterations {info[2]:.0f}")
    assert info[1] == 0 and info[2] <= 200, (name, info)
    assert rel <= REL and viol <= FEAS, (name, rel, viol)
    return rel, x


@pytest.mark.parametrize("S,G,cm", [(3, None, 1), (3, 1, 1), (12, None, 2), (96, 32, 1)])
def test_every_master_of_a_farmer_run(host, S, G, cm):
    """Cold, and warm from the previous master's vertex as the device starts."""
    scens = [farmer_scenario(f"scen{i}", cm, num_scens=S) for i in range(S)]
    ref = R.LShapedRef(scens, G=G, tol=1e-8)
    assert ref.run()
    prev, worst = None, 0.0
    for mi, K in enumerate(ref.masters):
        args = (ref.nn, ref.G, ref.cuts[:K], ref.R, ref.rl, ref.ru, ref.xlb, ref.xub, ref.etalb)
        worst = max(worst, _check(host, f"S={S} master {mi} cold", *args)[0])
        r, prev = _check(host, f"S={S} master {mi} warm", *args, x0=prev)
        worst = max(worst, r)
    print(f"S={S} G={ref.G}: worst relative difference {worst:.2e}")


def test_constructed_masters(host):
    rng = np.random.default_rng(11)
    nn, G = 3, 2
    xlb, xub, etalb = np.zeros(nn), np.full(nn, 10.0), np.full(G, -100.0)
    Z, e = np.zeros((0, nn)), np.zeros(0)

    def rc(n, span=0.0):
        return [(i % G, rng.uniform(-1, 1, nn) * 10 ** rng.uniform(0, span), float(rng.uniform(-5, 5))) for i in range(n)]
    cuts = rc(8)
    _check(host, "repeated cut", nn, G, cuts + [cuts[0]] * 4, Z, e, e, xlb, xub, etalb)
    _check(host, "equality row", nn, G, cuts, np.ones((1, nn)), np.array([7.0]), np.array([7.0]), xlb, xub, etalb)
    fl, fu = xlb.copy(), xub.copy()
    fl[1], fu[1] = -np.inf, np.inf
    _check(host, "free column", nn, G, cuts, Z, e, e, fl, fu, etalb)
    _check(host, "coefficients 1 to 1e5", nn, G, rc(12, 5.0), Z, e, e, xlb, xub, etalb)
    _check(host, "full store", nn, G, cuts, Z, e, e, xlb, xub, etalb, max_cuts=len(cuts))
    _check(host, "no cuts", nn, G, [], Z, e, e, xlb, xub, etalb)
    Rr, rl, ru = np.ones((2, nn)), np.array([-np.inf, 2.0]), np.array([1.0, np.inf])
    assert R.solve_master(nn, G, cuts, Rr, rl, ru, xlb, xub, etalb)[3] == 2
    _, info = _solve(host, nn, G, cuts, Rr, rl, ru, xlb, xub, etalb)
    assert info[1] == 2 and info[2] <= 200            # PHGPU_PRIMAL_INFEASIBLE within the cap
