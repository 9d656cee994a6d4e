"""The handle's device memory: every buffer has one owner, phgpu_destroy frees
them all, and phgpu_workspace_bytes counts each once.

* phgpu_set_scenarios again on a shared-matrix handle leaves workspace_bytes where the first
  call put it (the per-scenario column / row lists are re-allocated, their bytes given back);
* create / exercise / close rounds over the solve paths and the first-use workspaces: no
  error, and the same workspace_bytes at the same point of every round (per-handle, exact);
* the card's free memory over such rounds of a handle of >= 32 MB: a handle that destroy did
  not free would cost a whole workspace_bytes per round; the margin is half of one.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

AIR_KW = {"start_seed": 1134}      # aircond with the model's own default parameters (tests/fixer_ref.py)


def _engine(model, S, bf=None):
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.examples import aircond, farmer
    if model == "farmer":
        b = farmer.batch_creator(farmer.scenario_names_creator(S), crops_multiplier=1, num_scens=S)
    else:
        b = aircond.batch_creator(aircond.scenario_names_creator(S), branching_factors=bf, **AIR_KW)
    return PHEngine(b, device="cuda:0", shared=True if model == "aircond_shared" else None)


def _set_scenarios(e):
    """phgpu_set_scenarios with the engine's own data, through the C ABI."""
    from mpisppy_amd import _lib
    from mpisppy_amd.engine import _ptr
    _lib.check(e.lib.phgpu_set_scenarios(
        e.h, _ptr(e.A_val), _ptr(e.c), _ptr(e.lb), _ptr(e.ub), _ptr(e.rl), _ptr(e.ru), _ptr(e.q),
        _ptr(e.obj_const), _ptr(e.prob), _ptr(e.node_of), _ptr(e.prob_coeff), e._stream()), "phgpu_set_scenarios")


def test_set_scenarios_again_does_not_grow_the_workspace(gpu):
    from mpisppy_amd import _lib
    e = _engine("aircond_shared", 24, [4, 3, 2])
    assert e.shared
    first = e.workspace_bytes()                      # the constructor made the first call
    assert first > 0
    for call in (2, 3):
        _set_scenarios(e)
        assert e.workspace_bytes() == first, call
    e.solve(_lib.default_options(), warm=False)      # the re-allocated lists still serve a solve
    assert (e.host("status") == _lib.OPTIMAL).all()
    assert e.workspace_bytes() == first
    e.close()


def _with_env(key, value, fn):
    keep = os.environ.get(key)
    os.environ[key] = value
    try:
        fn()
    finally:
        if keep is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = keep


def _round(model, S, bf):
    """One handle's life; workspace_bytes after every step."""
    from mpisppy_amd import _lib
    e = _engine(model, S, bf)
    ws = [e.workspace_bytes()]
    info = e.kernel_info()
    assert info["instance"] >= 0 and info["wg_instance"] >= 0, info

    def opts(kernel):
        o = _lib.default_options()
        o.kernel = kernel
        return o

    e.solve(opts(3), warm=False)                                       # the records
    ws.append(e.workspace_bytes())
    _with_env("PHGPU_REG_REC", "1", lambda: e.solve(opts(2)))         # record mode, warm from the records
    assert e.kernel_info()["rec"] == 1
    ws.append(e.workspace_bytes())
    e.solve(opts(0), speculative=True)                                 # the default path, the other warm slot
    e.commit()
    ws.append(e.workspace_bytes())
    assert (e.host("status") == _lib.OPTIMAL).all()
    # the first call of four entry points that allocate their workspace then
    e.residuals()
    ws.append(e.workspace_bytes())
    e.nonant_stats(e.W)
    ws.append(e.workspace_bytes())
    e.w_diff()
    ws.append(e.workspace_bytes())
    none = torch.full((e.nn,), -1, dtype=torch.int32)
    e.fixer_step(_lib.FixerParams(boundtol=0.125, iter0=1), e.fixer_arg(np.ones(e.nn), torch.float64),
                 e.fixer_arg(none, torch.int32), e.fixer_arg(none, torch.int32), e.fixer_arg(none, torch.int32))
    ws.append(e.workspace_bytes())
    torch.cuda.synchronize()
    e.close()
    return ws


@pytest.mark.parametrize("model,S,bf", [("farmer", 130, None),            # three waves, the last ragged
                                        ("aircond", 24, [4, 3, 2])])      # waves span nodes
def test_rounds_of_create_exercise_close(gpu, model, S, bf):
    first = _round(model, S, bf)
    assert all(b >= a for a, b in zip(first, first[1:])) and first[-1] > first[3], first
    for r in range(3):
        assert _round(model, S, bf) == first, r


def test_destroy_gives_the_memory_back(gpu):
    """Four rounds of a farmer handle of >= 32 MB on the default path.  Free device memory after
    round 4 against after round 2: a handle that was not freed costs workspace_bytes per round,
    two rounds four times the margin of half of one."""
    from mpisppy_amd import _lib
    free, ws = [], 0
    for r in range(4):
        e = _engine("farmer", 20000)
        e.solve(_lib.default_options(), warm=False)
        e.solve(_lib.default_options(), speculative=True)
        e.commit()
        e.residuals()
        assert (e.host("status") == _lib.OPTIMAL).all()
        ws = e.workspace_bytes()
        e.close()
        del e
        torch.cuda.synchronize()
        torch.cuda.empty_cache()                     # torch's own cache is not what is measured
        free.append(torch.cuda.mem_get_info()[0])
    assert ws >= 32 * 1024 * 1024, ws
    print("workspace_bytes", ws, "free after each round", free)
    assert free[3] >= free[1] - ws // 2, (free, ws)
