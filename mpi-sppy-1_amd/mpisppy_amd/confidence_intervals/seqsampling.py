"""Sequential sampling: a candidate and a confidence interval on its optimality gap from samples
of growing size (mirrors mpisppy/confidence_intervals/seqsampling.py:33-524).

    [bm2011]  Bayraksan, Morton: A Sequential Sampling Procedure for Stochastic Programming,
              Operations Research 59(4), 898-913 (2011)
    [bpl2012] Bayraksan, Pierre-Louis: Fixed-Width Sequential Stopping Rules for a Class of
              Stochastic Programs, SIAM Journal on Optimization 22(4), 1518-1548 (2012)

Two-stage problems only (``IndepScens_SeqSampling`` and multi_seqsampling.py stay out).  Every
iteration's G_k and s_k is one ``ciutils.gap_estimators`` call: two batched solves and one read.

DEPARTURES from the reference.  ``cfg`` is any object with the option names (not only a Config).
When the candidate is resampled completely (``kf_xhat``), its sample has m_k = sample_size_ratio *
n_k scenarios as [bm2011] states (seqsampling.py:448 takes n_{k-1} there while counting m_k);
``kf_Gs`` is read under that name (seqsampling.py:478 reads ``kf_GS``); ``BPL_n0min`` defaults to
50 for stochastic sampling (seqsampling.py:193-194 cannot run).
"""
import numpy as np

from .. import global_toc
from ..comm import Comm
from . import ciutils


def is_needed(cfg, needed_things, message=""):
    cfg = ciutils.CfgView(cfg)
    absent = [i for i in needed_things if i not in cfg]
    if absent:
        raise RuntimeError("Some options are missing from this list of required options:\n"
                           f"{needed_things}\n"
                           f"missing: {absent}\n"
                           f"{message}")


def add_options(cfg, optional_things):
    """Defaults for the options that Bayraksan et al establish: set those ``cfg`` does not have."""
    for i, v in optional_things.items():
        if i not in cfg:
            if not isinstance(v, (str, int, float, bool, dict)):
                raise RuntimeError(f"add_options cannot process type {type(v)} for option {i}:{v}")
            cfg.quick_assign(i, type(v), v)


def xhat_generator_farmer(scenario_names, solver_name=None, solver_options=None, crops_multiplier=1):
    """For developer testing: the candidate that minimises the farmer sample problem over
    ``scenario_names`` ({"ROOT": x}), by the L-shaped method."""
    from ..examples import farmer
    tol, sp_options = ciutils._split_solver_options(None, solver_options)
    kw = {"use_integer": False, "crops_multiplier": crops_multiplier, "num_scens": len(scenario_names)}
    return {"ROOT": ciutils.lshaped_xstar(farmer, list(scenario_names), kw, solver_name, tol=tol,
                                          sp_options=sp_options)}


class SeqSampling:
    """``refmodel``: a model module or its dotted name; ``xhat_generator``: a function
    (scenario_names, solver_name=, solver_options=, **xhat_gen_kwargs) -> {"ROOT": x̂};
    ``cfg``: the options -- ``solver_name`` (or ``EF_solver_name``), ``solver_options``,
    ``sample_size_ratio`` (1), ``xhat_gen_kwargs`` ({}), ``ArRP`` (1), ``kf_Gs`` (1), ``kf_xhat``
    (1), ``confidence_level`` (0.95) and those of the criterion: BM_h, BM_hprime, BM_eps,
    BM_eps_prime, BM_p (and BM_q) for "BM"; BPL_eps (BPL_c0, BPL_c1, functions_dict with a
    growth_function, or BPL_n0min with ``stochastic_sampling``) for "BPL"."""

    def __init__(self, refmodel, xhat_generator, cfg, stochastic_sampling=False, stopping_criterion="BM",
                 solving_type="EF_2stage"):
        self.refmodel = ciutils.model_module(refmodel)
        self.refmodelname = refmodel
        self.xhat_generator = xhat_generator
        self.cfg = cfg = ciutils.CfgView(cfg)
        self.stochastic_sampling = stochastic_sampling
        self.stopping_criterion = stopping_criterion
        self.solving_type = solving_type
        self.sample_size_ratio = cfg.get("sample_size_ratio", 1)
        self.xhat_gen_kwargs = cfg.get("xhat_gen_kwargs", {})
        complete = True
        for fct in ("scenario_names_creator", "scenario_creator", "kw_creator"):    # denouement can be missing
            if not hasattr(self.refmodel, fct):
                print(f"Module {refmodel} is missing {fct}")
                complete = False
        if not complete:
            raise RuntimeError(f"Module {refmodel} not complete for seqsampling")
        if self.stochastic_sampling:
            add_options(cfg, {"BPL_n0min": 50})
        if self.stopping_criterion == "BM":
            is_needed(cfg, ["BM_eps_prime", "BM_hprime", "BM_eps", "BM_h", "BM_p"])
        elif self.stopping_criterion == "BPL":
            is_needed(cfg, ["BPL_eps"])
            if not self.stochastic_sampling:
                add_options(cfg, {"BPL_c1": 2, "functions_dict": {"growth_function": (lambda x: x - 1)}})
        else:
            raise RuntimeError("Only BM and BPL criteria are supported at this time.")
        for oname, default in (("BM_eps_prime", None), ("BM_hprime", None), ("BM_eps", None), ("BM_h", None),
                               ("BM_p", None), ("BM_q", None), ("BPL_eps", None), ("BPL_c0", 50), ("BPL_c1", 2),
                               ("BPL_n0min", 50), ("functions_dict", None), ("confidence_level", 0.95),
                               ("ArRP", 1), ("kf_Gs", 1), ("kf_xhat", 1)):
            setattr(self, oname, cfg.get(oname, default))
        self.solver_name = cfg.get("EF_solver_name", cfg.get("solver_name"))
        self.solver_options = cfg.get("EF_solver_options", cfg.get("solver_options"))
        assert self.solver_name is not None
        if self.solving_type == "EF_2stage":
            self.multistage = False
        elif self.solving_type == "EF_mstage":
            raise NotImplementedError("EF_mstage needs sample_tree, which this engine does not serve: two-stage "
                                      "problems only (IndepScens_SeqSampling stays out)")
        else:
            raise RuntimeError(f"The solving_type {self.solving_type} is not supported. If you want to run a 2-stage "
                               f"problem, please use a solving_type in ['EF_2stage'].")
        self.stop_criterion = self.bm_stopping_criterion if self.stopping_criterion == "BM" \
            else self.bpl_stopping_criterion
        if self.stochastic_sampling:
            self.sample_size = self.stochastic_sampsize
        elif self.stopping_criterion == "BM":
            self.sample_size = self.bm_sampsize
        else:
            self.sample_size = self.bpl_fsp_sampsize
        self.ScenCount = 0          # scenarios used so far: every sample is new

    # [bm2011] (4): keep sampling while G_k > h' s_k + eps'
    def bm_stopping_criterion(self, G, s, nk):
        return G > self.BM_hprime * s + self.BM_eps_prime

    # [bpl2012]: keep sampling while G_k + t s_k / sqrt(n_k) + 1 / sqrt(n_k) > eps
    def bpl_stopping_criterion(self, G, s, nk):
        t = ciutils.t_ppf(self.confidence_level, nk - 1)
        return G + t * s / np.sqrt(nk) + 1 / np.sqrt(nk) > self.BPL_eps

    def _bm_constant(self, r=2):
        """c_p of [bm2011] (5), or c_pq of (14) when BM_q is given."""
        if self.confidence_level is None:
            raise RuntimeError("We need the confidence level to compute the constant cp")
        j = np.arange(1, 1000)
        if self.BM_q is None:
            tot = np.sum(np.power(j, -self.BM_p * np.log(j)))
        else:
            tot = np.sum(np.exp(-self.BM_p * np.power(j, 2 * self.BM_q / r)))
        return max(1, 2 * np.log(tot / (np.sqrt(2 * np.pi) * (1 - self.confidence_level))))

    def bm_sampsize(self, k, G, s, nk_m1, r=2):
        c = self.c if hasattr(self, "c") else self._bm_constant(r)
        if self.BM_q is None:
            growth = 2 * self.BM_p * np.log(k) ** 2                  # (5)
        else:
            growth = 2 * self.BM_p * np.power(k, 2 * self.BM_q / r)  # (14)
        return int(np.ceil((c + growth) / (self.BM_h - self.BM_hprime) ** 2))

    def bpl_fsp_sampsize(self, k, G, s, nk_m1):
        return int(np.ceil(self.BPL_c0 + self.BPL_c1 * self.functions_dict["growth_function"](k)))

    def stochastic_sampsize(self, k, G, s, nk_m1):
        """[bpl2012] section 5: the larger root of a quadratic in sqrt(n)."""
        if k == 1:
            return int(np.ceil(max(self.BPL_n0min, np.log(1 / self.BPL_eps))))
        t = ciutils.t_ppf(self.confidence_level, nk_m1 - 1)
        a, b, c = -self.BPL_eps, 1 + t * s, nk_m1 * G
        maxroot = -(np.sqrt(b ** 2 - 4 * a * c) + b) / (2 * a)
        return int(np.ceil(maxroot ** 2))

    def _candidate(self, names):
        xgo = dict(self.xhat_gen_kwargs)
        for key in ("solver_name", "solver_options", "scenario_names"):     # given explicitly
            xgo.pop(key, None)
        return self.xhat_generator(names, solver_name=self.solver_name, solver_options=self.solver_options, **xgo)

    def _estimators(self, xhat_k, names, nk):
        return ciutils.gap_estimators(
            xhat_k, self.refmodel, solving_type=self.solving_type, scenario_names=names, ArRP=self.ArRP,
            cfg=ciutils.CfgView(self.cfg, num_scens=nk),
            scenario_denouement=getattr(self.refmodel, "scenario_denouement", None),
            solver_name=self.solver_name, solver_options=self.solver_options)

    def run(self, maxit=200):
        """seqsampling.py:331-524: {"T": iterations, "Candidate_solution": x̂, "CI": [0, upper end]}."""
        refmodel, mult = self.refmodel, self.sample_size_ratio
        k = 1
        if self.stopping_criterion == "BM":
            if self.BM_q is not None and self.BM_q < 1:
                raise RuntimeError("Parameter q should be greater than 1.")
            self.c = self._bm_constant()
        lower_bound_k = self.sample_size(k, None, None, None)
        # step 0: the candidate from m_1 = mult n_1 scenarios
        mk = int(np.floor(mult * lower_bound_k))
        xhat_names = refmodel.scenario_names_creator(mk, start=self.ScenCount)
        self.ScenCount += mk
        xhat_k = self._candidate(xhat_names)
        # step 1: G_1 and s_1 from n_1 new scenarios
        nk = self.ArRP * int(np.ceil(lower_bound_k / self.ArRP))
        est_names = refmodel.scenario_names_creator(nk, start=self.ScenCount)
        self.ScenCount += nk
        estim = self._estimators(xhat_k, est_names, nk)
        Gk, sk = estim["G"], estim["s"]
        self.history = [(nk, Gk, sk)]
        # steps 2, 3
        while self.stop_criterion(Gk, sk, nk) and k < maxit:
            k += 1
            nk_m1, mk_m1 = nk, mk
            lower_bound_k = self.sample_size(k, Gk, sk, nk_m1)
            mk = int(np.floor(mult * lower_bound_k))
            assert mk >= mk_m1, "Our sample size should be increasing"
            if k % self.kf_xhat == 0:       # only new scenarios for the candidate
                xhat_names = refmodel.scenario_names_creator(mk, start=self.ScenCount)
                self.ScenCount += mk
            else:                           # the previous ones and what is missing
                xhat_names = xhat_names + refmodel.scenario_names_creator(mk - mk_m1, start=self.ScenCount)
                self.ScenCount += mk - mk_m1
            xhat_k = self._candidate(xhat_names)
            nk = self.ArRP * int(np.ceil(lower_bound_k / self.ArRP))
            assert nk >= nk_m1, "Our sample size should be increasing"
            if k % self.kf_Gs == 0:
                est_names = refmodel.scenario_names_creator(nk, start=self.ScenCount)
                self.ScenCount += nk
            else:
                est_names = est_names + refmodel.scenario_names_creator(nk - nk_m1, start=self.ScenCount)
                self.ScenCount += nk - nk_m1
            estim = self._estimators(xhat_k, est_names, nk)
            Gk, sk = estim["G"], estim["s"]
            self.history.append((nk, Gk, sk))
            if k % 10 == 0 and Comm().Get_rank() == 0:
                print(f"k={k}\nn_k={nk}\nG_k={Gk}\ns_k={sk}")
        # step 4
        if k == maxit:
            raise RuntimeError(f"The loop terminated after {maxit} iteration with no acceptable solution")
        upper_bound = self.BM_h * sk + self.BM_eps if self.stopping_criterion == "BM" else self.BPL_eps
        global_toc(f"G={Gk} sk={sk}; xhat has been computed with {nk * mult} observations.", Comm().Get_rank() == 0)
        return {"T": k, "Candidate_solution": xhat_k, "CI": [0, upper_bound]}
