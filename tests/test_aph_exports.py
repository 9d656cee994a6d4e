"""The APH entries of the C-ABI (include/phgpu.h): declared, exported, typed in _lib.py, and
their host-side argument checks (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "phgpu.h")
LIB = os.path.join(ROOT, "mpi-sppy-1_amd", "mpisppy_amd", "libphgpu.so")
APH_SYMBOLS = ["phgpu_aph_reduce", "phgpu_aph_norms", "phgpu_aph_update", "phgpu_aph_mark",
               "phgpu_select_smallest", "phgpu_solve_list"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build(verbose=False)
    return ctypes.CDLL(LIB)


def test_declared_exported_and_typed(lib):
    txt = open(HDR).read()
    from mpisppy_amd import _lib
    L = _lib.load()
    for s in APH_SYMBOLS:
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
    assert L.phgpu_aph_reduce(n, 1, n, n, n, n, n, n, n, n) == -1
    assert L.phgpu_aph_norms(n, 1.0, n, n, n, n, n, n, n, n, n, n) == -1
    assert L.phgpu_aph_update(n, 1, 1.0, 1.0, n, n, n, n, n, n, n, n, n, n) == -1
    assert L.phgpu_aph_mark(n, n, 1, 99, 0, n, n, n, n, n, n, n, n, n) == -1
    assert L.phgpu_select_smallest(n, n, n, 1, n, n, n) == -1
    assert L.phgpu_solve_list(n, n, n, 0, n, n, n, n, n, n, n) == -1
    assert "null" in _lib.last_error()


def test_python_surface():
    from mpisppy_amd.cylinders.hub import APHHub                          # noqa: F401
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.opt.aph import APH
    from mpisppy_amd.utils.cfg_vanilla import aph_hub                     # noqa: F401
    for m in ("aph_init", "aph_bind", "aph_reduce", "aph_norms", "aph_update", "aph_scalars", "aph_mark",
              "select_smallest", "solve_list"):
        assert callable(getattr(PHEngine, m)), m
    for m in ("APH_main", "APH_iterk", "APH_solve_loop", "Compute_Convergence"):
        assert callable(getattr(APH, m)), m
