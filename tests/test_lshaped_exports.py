"""The L-shaped entries of the C-ABI (include/phgpu.h): declared, exported, typed in _lib.py, and
their host-side argument checks (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "phgpu.h")
LIB = os.path.join(ROOT, "mpi-sppy-1_amd", "mpisppy_amd", "libphgpu.so")
LS_SYMBOLS = ["phgpu_lshaped_init", "phgpu_lshaped_cuts", "phgpu_lshaped_append", "phgpu_lshaped_master",
              "phgpu_lshaped_load", "phgpu_lshaped_export"]


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
    for s in LS_SYMBOLS:
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
    assert L.phgpu_lshaped_init(n, 1, 1, 0, 1, 0, n, n, n, n, n, n, n) == -1
    assert L.phgpu_lshaped_cuts(n, n, n, n, n, n, n) == -1
    assert L.phgpu_lshaped_append(n, n, n, 1e-8, n, n) == -1
    assert L.phgpu_lshaped_master(n, n, n, n, n, n) == -1
    assert L.phgpu_lshaped_load(n, 0, n, n, n, n) == -1
    assert L.phgpu_lshaped_export(n, n, n, n, n, n) == -1
    assert "null" in _lib.last_error()


def test_python_surface():
    from mpisppy_amd.cylinders.hub import LShapedHub                      # noqa: F401
    from mpisppy_amd.cylinders.lshaped_bounder import XhatLShapedInnerBound
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.opt.lshaped import LShapedMethod
    from mpisppy_amd.utils.cfg_vanilla import lshaped_hub, xhatlshaped_spoke    # noqa: F401
    assert XhatLShapedInnerBound.converger_spoke_char == "X"
    for m in ("lshaped_init", "lshaped_cuts", "lshaped_append", "lshaped_master", "lshaped_read", "lshaped_load",
              "lshaped_export"):
        assert callable(getattr(PHEngine, m)), m
    for m in ("lshaped_algorithm", "options_check"):
        assert callable(getattr(LShapedMethod, m)), m
