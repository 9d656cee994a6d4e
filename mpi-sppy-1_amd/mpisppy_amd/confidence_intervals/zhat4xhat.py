"""ẑ of a candidate on fresh samples (the two-stage counterpart of
mpisppy/confidence_intervals/zhat4xhat.py:15-122).  The reference samples one tree after the other
and evaluates each with its own Xhat_Eval; here all ``num_samples * sample_size`` scenarios are
ONE Xhat_Eval, one batched solve with the nonants fixed at x̂, and one ``engine.gap_moments`` call
with the x* side left out."""
import numpy as np

from . import ciutils


def evaluate_sample_trees(*args, **kwargs):
    raise NotImplementedError("evaluate_sample_trees needs sample_tree (multistage), which this engine does not "
                              "serve; use evaluate_samples for a two-stage problem")


def evaluate_samples(xhat_one, num_samples, sample_size, cfg, InitSeed=0, model_module=None, mpicomm=None):
    """ẑ(x̂) of ``num_samples`` samples of ``sample_size`` scenarios, numbered from ``InitSeed``:
    (zhats [num_samples], the advanced seed).  ``xhat_one``: the candidate's values (a list or
    array, not a dict)."""
    from ..comm import Comm
    from ..utils.xhat_eval import Xhat_Eval
    lcfg = ciutils.CfgView(cfg, num_scens=int(sample_size), _mpisppy_probability=1 / int(sample_size))
    m = ciutils.model_module(model_module if model_module is not None else lcfg["model_module_name"])
    ciutils.check_module(m)
    B, n = int(num_samples), int(sample_size)
    names = m.scenario_names_creator(B * n, start=InitSeed)
    _, sp_options = ciutils._split_solver_options(lcfg, None)
    opts = {"solver_name": lcfg.get("EF_solver_name", lcfg.get("solver_name")), "toc": False, "verbose": False,
            "device": lcfg.get("device"), "solver_options": sp_options}
    if hasattr(m, "batch_creator"):
        opts["batch_creator"] = m.batch_creator
    ev = Xhat_Eval(opts, names, m.scenario_creator, m.scenario_denouement, scenario_creator_kwargs=m.kw_creator(lcfg),
                   mpicomm=mpicomm if mpicomm is not None else Comm())
    try:
        ev._lazy_create_solvers()
        if ev.multistage or ev.batch.depth != 1:
            raise NotImplementedError("multistage sampling (sample_tree.py) is not served: two-stage only")
        ev._fix_nonants({"ROOT": np.asarray(xhat_one, dtype=np.float64)})
        ev.solve_loop(solver_options=sp_options)
        e = ev.engine
        M = e.gap_moments(np.arange(B + 1, dtype=np.int64) * n, e.obj, e.status)
        sense = ev.batch.sense
    finally:
        if ev.engine is not None:
            ev.engine.close()
    bad = np.nonzero(M[:, 6] > 0)[0]
    if len(bad):
        j = int(bad[0])
        raise RuntimeError(f"sample {j} (scenarios {names[j * n]}..{names[(j + 1) * n - 1]}): {int(M[j, 6])} "
                           f"scenario(s) were not solved to optimality at the candidate")
    return sense * M[:, 4] / M[:, 0], InitSeed + B * n


def run_samples(cfg, model_module):
    """zhat4xhat.py:100-122: (zhatbar, eps_z) of ``cfg.num_samples`` samples of ``cfg.sample_size``
    (default ``cfg.num_scens``) scenarios at the candidate stored at ``cfg.xhatpath``."""
    cfg = ciutils.CfgView(cfg)
    xhat_one = ciutils.read_xhat(cfg["xhatpath"])["ROOT"]
    sample_size = cfg.get("sample_size", cfg.get("num_scens"))
    if not sample_size:
        raise RuntimeError("run_samples needs sample_size (or num_scens) in cfg")
    zhats, _ = evaluate_samples(xhat_one, cfg["num_samples"], sample_size, cfg, InitSeed=0, model_module=model_module)
    confidence_level = cfg.get("confidence_level", 0.95)
    zhatbar = np.mean(zhats)
    s_zhat = np.std(np.array(zhats))
    t_zhat = ciutils.t_ppf(confidence_level, len(zhats) - 1)
    eps_z = t_zhat * s_zhat / np.sqrt(len(zhats))
    print("zhatbar: ", zhatbar)
    print("estimate: ", [zhatbar - eps_z, zhatbar + eps_z])
    print("confidence_level", confidence_level)
    return zhatbar, eps_z
