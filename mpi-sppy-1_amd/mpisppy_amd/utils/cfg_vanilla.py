"""Cylinder dict builders (mirrors mpisppy/utils/cfg_vanilla.py:41-495 for the cylinders
this engine serves: ph_hub, aph_hub, lshaped_hub, fwph_spoke, lagrangian_spoke, xhatshuffle_spoke, xhatxbar_spoke,
xhatlshaped_spoke, slammax_spoke, slammin_spoke; extension_adder, add_fixer and add_wxbar_read_write for the hub's
extensions).

``cfg`` is any object with the reference's config attribute names (solver_name,
default_rho, max_iterations, rel_gap, ...); missing attributes take the reference's
defaults.  The returned dicts feed ``WheelSpinner(hub_dict, list_of_spoke_dict)``.
"""
import copy

from ..cylinders.fwph_spoke import FrankWolfeOuterBound
from ..cylinders.hub import APHHub, LShapedHub, PHHub
from ..cylinders.lagrangian_bounder import LagrangianOuterBound
from ..cylinders.lshaped_bounder import XhatLShapedInnerBound
from ..cylinders.slam_heuristic import SlamMaxHeuristic, SlamMinHeuristic
from ..cylinders.xhatxbar_bounder import XhatXbarInnerBound
from ..cylinders.xhatshufflelooper_bounder import XhatShuffleInnerBound
from ..convergers.norm_rho_converger import NormRhoConverger
from ..convergers.primal_dual_converger import PrimalDualConverger
from ..extensions.extension import MultiExtension
from ..extensions.fixer import Fixer
from ..extensions.gradient_extension import Gradient_extension
from ..extensions.mult_rho_updater import MultRhoUpdater
from ..extensions.norm_rho_updater import NormRhoUpdater
from ..fwph.fwph import FWPH
from ..opt.aph import APH
from ..opt.lshaped import LShapedMethod
from ..opt.ph import PH
from ..phbase import PHBase
from .xhat_eval import Xhat_Eval
from .wxbarreader import WXBarReader
from .wxbarwriter import WXBarWriter


def _get(cfg, name, default=None):
    v = getattr(cfg, name, default)
    return default if v is None else v


# cfg_vanilla.py:41-62
def shared_options(cfg):
    shoptions = {
        "solver_name": _get(cfg, "solver_name", "mi355x_pdhg"),
        "defaultPHrho": _get(cfg, "default_rho", 1.0),
        "convthresh": 0,
        "PHIterLimit": _get(cfg, "max_iterations", 1),
        "verbose": _get(cfg, "verbose", False),
        "display_progress": _get(cfg, "display_progress", False),
        "display_convergence_detail": _get(cfg, "display_convergence_detail", False),
        "iter0_solver_options": dict(_get(cfg, "iter0_solver_options", {})),
        "iterk_solver_options": dict(_get(cfg, "iterk_solver_options", {})),
        "tee-rank0-solves": _get(cfg, "tee_rank0_solves", False),
        "trace_prefix": getattr(cfg, "trace_prefix", None),
        "device": getattr(cfg, "device", None),
        "toc": _get(cfg, "toc", True),
    }
    if getattr(cfg, "batch_creator", None) is not None:
        shoptions["batch_creator"] = cfg.batch_creator
    return shoptions


# cfg_vanilla.py:77-125
def ph_hub(cfg, scenario_creator, scenario_denouement, all_scenario_names, scenario_creator_kwargs=None,
           ph_extensions=None, extension_kwargs=None, ph_converger=None, rho_setter=None,
           variable_probability=None, all_nodenames=None):
    options = copy.deepcopy(shared_options(cfg))
    options["convthresh"] = _get(cfg, "intra_hub_conv_thresh", 1e-10)
    options["bundles_per_rank"] = _get(cfg, "bundles_per_rank", 0)
    return {
        "hub_class": PHHub,
        "hub_kwargs": {"options": {"rel_gap": getattr(cfg, "rel_gap", None),
                                   "abs_gap": getattr(cfg, "abs_gap", None),
                                   "max_stalled_iters": getattr(cfg, "max_stalled_iters", None)}},
        "opt_class": PH,
        "opt_kwargs": {
            "options": options,
            "all_scenario_names": all_scenario_names,
            "scenario_creator": scenario_creator,
            "scenario_creator_kwargs": scenario_creator_kwargs,
            "scenario_denouement": scenario_denouement,
            "rho_setter": rho_setter,
            "variable_probability": variable_probability,
            "extensions": ph_extensions,
            "extension_kwargs": extension_kwargs,
            "ph_converger": ph_converger,
            "all_nodenames": all_nodenames,
        },
    }


# cfg_vanilla.py:128-161
def aph_hub(cfg, scenario_creator, scenario_denouement, all_scenario_names, scenario_creator_kwargs=None,
            ph_extensions=None, extension_kwargs=None, rho_setter=None, variable_probability=None,
            all_nodenames=None):
    hub_dict = ph_hub(cfg, scenario_creator, scenario_denouement, all_scenario_names,
                      scenario_creator_kwargs=scenario_creator_kwargs, ph_extensions=ph_extensions,
                      extension_kwargs=extension_kwargs, rho_setter=rho_setter,
                      variable_probability=variable_probability, all_nodenames=all_nodenames)
    hub_dict["hub_class"] = APHHub
    hub_dict["opt_class"] = APH
    options = hub_dict["opt_kwargs"]["options"]
    options["APHgamma"] = _get(cfg, "aph_gamma", 1.0)
    options["APHnu"] = _get(cfg, "aph_nu", 1.0)
    options["async_frac_needed"] = _get(cfg, "aph_frac_needed", 1.0)     # accepted and ignored (opt/aph.py)
    options["dispatch_frac"] = _get(cfg, "aph_dispatch_frac", 1.0)
    options["async_sleep_secs"] = _get(cfg, "aph_sleep_seconds", 0.01)   # accepted and ignored
    return hub_dict


# cfg_vanilla.py:277-317
def fwph_spoke(cfg, scenario_creator, scenario_denouement, all_scenario_names, scenario_creator_kwargs=None,
               all_nodenames=None):
    shoptions = shared_options(cfg)
    mip_solver_options, qp_solver_options = dict(), dict()
    if getattr(cfg, "max_solver_threads", None) is not None:
        mip_solver_options["threads"] = cfg.max_solver_threads
        qp_solver_options["threads"] = cfg.max_solver_threads
    if getattr(cfg, "fwph_mipgap", None) is not None:
        mip_solver_options["mipgap"] = cfg.fwph_mipgap      # accepted and ignored: the "MIP" is an LP here
    fw_options = {
        "FW_iter_limit": _get(cfg, "fwph_iter_limit", 10),
        "FW_weight": _get(cfg, "fwph_weight", 0.0),
        "FW_conv_thresh": _get(cfg, "fwph_conv_thresh", 1e-4),
        "stop_check_tol": _get(cfg, "fwph_stop_check_tol", 1e-4),
        "solver_name": shoptions["solver_name"],
        "FW_verbose": shoptions["verbose"],
        "mip_solver_options": mip_solver_options,
        "qp_solver_options": qp_solver_options,
    }
    if getattr(cfg, "fwph_max_columns", None) is not None:
        fw_options["FW_max_columns"] = cfg.fwph_max_columns
    return {
        "spoke_class": FrankWolfeOuterBound,
        "opt_class": FWPH,
        "opt_kwargs": {
            "PH_options": shoptions,  # be sure convthresh is zero for fwph
            "FW_options": fw_options,
            "all_scenario_names": all_scenario_names,
            "scenario_creator": scenario_creator,
            "scenario_creator_kwargs": scenario_creator_kwargs,
            "scenario_denouement": scenario_denouement,
            "all_nodenames": all_nodenames,
        },
    }


# cfg_vanilla.py:320-353
def lagrangian_spoke(cfg, scenario_creator, scenario_denouement, all_scenario_names,
                     scenario_creator_kwargs=None, rho_setter=None, all_nodenames=None):
    return {
        "spoke_class": LagrangianOuterBound,
        "opt_class": PHBase,
        "opt_kwargs": {
            "options": copy.deepcopy(shared_options(cfg)),
            "all_scenario_names": all_scenario_names,
            "scenario_creator": scenario_creator,
            "scenario_creator_kwargs": scenario_creator_kwargs,
            "scenario_denouement": scenario_denouement,
            "rho_setter": rho_setter,
            "all_nodenames": all_nodenames,
        },
    }


# cfg_vanilla.py:457-492
def xhatshuffle_spoke(cfg, scenario_creator, scenario_denouement, all_scenario_names, all_nodenames=None,
                      scenario_creator_kwargs=None):
    shoptions = shared_options(cfg)
    xhat_options = copy.deepcopy(shoptions)
    xhat_options["bundles_per_rank"] = 0
    xhat_options["xhat_looper_options"] = {
        "xhat_solver_options": shoptions["iterk_solver_options"],
        "dump_prefix": "delme",
        "csvname": "looper.csv",
        "tries_per_sync": _get(cfg, "xhat_tries_per_sync", 1),
    }
    if getattr(cfg, "add_reversed_shuffle", None) is not None:
        xhat_options["xhat_looper_options"]["reverse"] = cfg.add_reversed_shuffle
    if getattr(cfg, "xhatshuffle_iter_step", None) is not None:
        xhat_options["xhat_looper_options"]["iter_step"] = cfg.xhatshuffle_iter_step
    return {
        "spoke_class": XhatShuffleInnerBound,
        "opt_class": Xhat_Eval,
        "opt_kwargs": {
            "options": xhat_options,
            "all_scenario_names": all_scenario_names,
            "scenario_creator": scenario_creator,
            "scenario_creator_kwargs": scenario_creator_kwargs,
            "scenario_denouement": scenario_denouement,
            "all_nodenames": all_nodenames,
        },
    }


# cfg_vanilla.py:424-454
def xhatxbar_spoke(cfg, scenario_creator, scenario_denouement, all_scenario_names, scenario_creator_kwargs=None,
                   variable_probability=None, all_nodenames=None):
    shoptions = shared_options(cfg)
    xhat_options = copy.deepcopy(shoptions)
    xhat_options["bundles_per_rank"] = 0
    xhat_options["xhat_xbar_options"] = {
        "xhat_solver_options": shoptions["iterk_solver_options"],
        "scen_limit": _get(cfg, "xhat_scen_limit", 3),
        "dump_prefix": "delme",
        "csvname": "xbar.csv",
    }
    return {
        "spoke_class": XhatXbarInnerBound,
        "opt_class": Xhat_Eval,
        "opt_kwargs": {
            "options": xhat_options,
            "all_scenario_names": all_scenario_names,
            "scenario_creator": scenario_creator,
            "scenario_creator_kwargs": scenario_creator_kwargs,
            "scenario_denouement": scenario_denouement,
            "variable_probability": variable_probability,
            "all_nodenames": all_nodenames,
        },
    }


# this project's convenience, as aph_hub (the reference builds the dict by hand,
# examples/farmer/farmer_lshapedhub.py:60-85)
def lshaped_hub(cfg, scenario_creator, scenario_denouement, all_scenario_names, scenario_creator_kwargs=None,
                all_nodenames=None):
    sh = shared_options(cfg)
    options = {
        "root_solver": sh["solver_name"],
        "sp_solver": sh["solver_name"],
        "solver_name": sh["solver_name"],
        "root_solver_options": dict(_get(cfg, "root_solver_options", {})),
        "sp_solver_options": dict(sh["iterk_solver_options"]),
        "max_iter": _get(cfg, "max_iterations", 30),
        "tol": _get(cfg, "lshaped_tol", None),
        "cut_groups": getattr(cfg, "cut_groups", None),
        "valid_eta_lb": getattr(cfg, "valid_eta_lb", None),
        "verbose": sh["verbose"],
        "device": sh["device"],
        "toc": sh["toc"],
    }
    if options["tol"] is None:
        del options["tol"]
    if "batch_creator" in sh:
        options["batch_creator"] = sh["batch_creator"]
    return {
        "hub_class": LShapedHub,
        "hub_kwargs": {"options": {"rel_gap": getattr(cfg, "rel_gap", None),
                                   "abs_gap": getattr(cfg, "abs_gap", None),
                                   "max_stalled_iters": getattr(cfg, "max_stalled_iters", None)}},
        "opt_class": LShapedMethod,
        "opt_kwargs": {
            "options": options,
            "all_scenario_names": all_scenario_names,
            "scenario_creator": scenario_creator,
            "scenario_creator_kwargs": scenario_creator_kwargs,
            "scenario_denouement": scenario_denouement,
            "all_nodenames": all_nodenames,
        },
    }


# cfg_vanilla.py:529-552
def xhatlshaped_spoke(cfg, scenario_creator, scenario_denouement, all_scenario_names, scenario_creator_kwargs=None):
    xhat_options = copy.deepcopy(shared_options(cfg))
    xhat_options["bundles_per_rank"] = 0
    return {
        "spoke_class": XhatLShapedInnerBound,
        "opt_class": Xhat_Eval,
        "opt_kwargs": {
            "options": xhat_options,
            "all_scenario_names": all_scenario_names,
            "scenario_creator": scenario_creator,
            "scenario_creator_kwargs": scenario_creator_kwargs,
            "scenario_denouement": scenario_denouement,
        },
    }


def _slam_spoke(spoke_class, cfg, scenario_creator, scenario_denouement, all_scenario_names,
                scenario_creator_kwargs):
    xhat_options = copy.deepcopy(shared_options(cfg))
    xhat_options["bundles_per_rank"] = 0
    return {
        "spoke_class": spoke_class,
        "opt_class": Xhat_Eval,
        "opt_kwargs": {
            "options": xhat_options,
            "all_scenario_names": all_scenario_names,
            "scenario_creator": scenario_creator,
            "scenario_creator_kwargs": scenario_creator_kwargs,
            "scenario_denouement": scenario_denouement,
        },
    }


# cfg_vanilla.py:554-576
def slammax_spoke(cfg, scenario_creator, scenario_denouement, all_scenario_names, scenario_creator_kwargs=None):
    return _slam_spoke(SlamMaxHeuristic, cfg, scenario_creator, scenario_denouement, all_scenario_names,
                       scenario_creator_kwargs)


# cfg_vanilla.py:578-600
def slammin_spoke(cfg, scenario_creator, scenario_denouement, all_scenario_names, scenario_creator_kwargs=None):
    return _slam_spoke(SlamMinHeuristic, cfg, scenario_creator, scenario_denouement, all_scenario_names,
                       scenario_creator_kwargs)


# cfg_vanilla.py:164-181
def extension_adder(hub_dict, ext_class):
    ok = hub_dict["opt_kwargs"]
    if ok.get("extensions") is None:
        ok["extensions"] = ext_class
    elif ok["extensions"] == MultiExtension:
        if ok.get("extension_kwargs") is None:
            ok["extension_kwargs"] = {"ext_classes": []}
        if ext_class not in ok["extension_kwargs"]["ext_classes"]:
            ok["extension_kwargs"]["ext_classes"].append(ext_class)
    elif ok["extensions"] != ext_class:
        ok["extension_kwargs"] = {"ext_classes": [ok["extensions"], ext_class]}
        ok["extensions"] = MultiExtension
    return hub_dict


# cfg_vanilla.py:184-191 (cfg.fixer_tol, cfg.id_fix_list_fct; with a batch_creator
# cfg.fix_arrays, the per-nonant arrays of extensions/fixer.py)
def add_fixer(hub_dict, cfg):
    hub_dict = extension_adder(hub_dict, Fixer)
    fixeroptions = {"verbose": False, "boundtol": cfg.fixer_tol,
                    "id_fix_list_fct": getattr(cfg, "id_fix_list_fct", None)}
    if getattr(cfg, "fix_arrays", None) is not None:
        fixeroptions["fix_arrays"] = cfg.fix_arrays
    hub_dict["opt_kwargs"]["options"]["fixeroptions"] = fixeroptions
    return hub_dict


# examples/farmer/farmer_cylinders.py:67-75 (farmer_rho_demo.py:80-84): the converger class
# the flags ask for
def converger_from_cfg(cfg):
    if _get(cfg, "use_norm_rho_converger", False):
        if not _get(cfg, "use_norm_rho_updater", False):
            raise RuntimeError("--use-norm-rho-converger requires --use-norm-rho-updater")
        return NormRhoConverger
    if _get(cfg, "primal_dual_converger", False):
        return PrimalDualConverger
    return None


# examples/farmer/farmer_cylinders.py:110-113 (cfg.use_norm_rho_updater).  The reference
# scripts hard-wire {'verbose': True}; here the table is printed only when
# cfg.norm_rho_options asks for it, since printing it reads rho back every iteration
def add_norm_rho_updater(hub_dict, cfg):
    if _get(cfg, "use_norm_rho_updater", False):
        hub_dict = extension_adder(hub_dict, NormRhoUpdater)
        hub_dict["opt_kwargs"]["options"]["norm_rho_options"] = dict(_get(cfg, "norm_rho_options", {}))
    return hub_dict


# examples/farmer/farmer_rho_demo.py:100-120 (cfg.rho_setter -> Gradient_extension with
# gradient_extension_options = {'cfg': cfg}; config.py:613-658 gradient_args / rho_args:
# order_stat, rho_relative_bound, xhatpath).  The flag is cfg.grad_rho_setter or the
# reference's cfg.rho_setter; the options are copied into a dict, and since cost and rho stay
# on the device there are no file names among them
def add_gradient_rho(hub_dict, cfg):
    if _get(cfg, "grad_rho_setter", False) or _get(cfg, "rho_setter", False) is True:
        hub_dict = extension_adder(hub_dict, Gradient_extension)
        o = dict(_get(cfg, "gradient_extension_options", {}))
        for name, default in (("order_stat", None), ("rho_relative_bound", 1e3), ("xhatpath", None), ("xhat", None),
                              ("indep_denom", False), ("dual_update_threshold", 0.05)):
            if name not in o and _get(cfg, name, default) is not None:
                o[name] = _get(cfg, name, default)
        hub_dict["opt_kwargs"]["options"]["gradient_extension_options"] = o
    return hub_dict


# examples/farmer/farmer_cylinders.py (cfg.mult_rho -> MultRhoUpdater with
# cfg.mult_rho_to_dict(), config.py:487-516); a cfg without that method gives its
# mult_rho_* attributes or a ready ``mult_rho_options`` dict
def add_mult_rho_updater(hub_dict, cfg):
    if _get(cfg, "mult_rho", False):
        hub_dict = extension_adder(hub_dict, MultRhoUpdater)
        o = dict(_get(cfg, "mult_rho_options", {}))
        for name in ("convergence_tolerance", "rho_update_stop_iteration", "rho_update_start_iteration"):
            if name not in o and getattr(cfg, "mult_rho_" + name.replace("rho_", "", 1), None) is not None:
                o[name] = getattr(cfg, "mult_rho_" + name.replace("rho_", "", 1))
        hub_dict["opt_kwargs"]["options"]["mult_rho_options"] = o
    return hub_dict


# examples/farmer/farmer_cylinders.py:67-75 and 103-108 (cfg.use_norm_rho_converger,
# cfg.primal_dual_converger, cfg.primal_dual_converger_tol; no tracker)
def add_ph_converger(hub_dict, cfg):
    conv = converger_from_cfg(cfg)
    if conv is not None:
        hub_dict["opt_kwargs"]["ph_converger"] = conv
    if conv is PrimalDualConverger:
        hub_dict["opt_kwargs"]["options"]["primal_dual_converger_options"] = {
            "verbose": bool(_get(cfg, "verbose", False)),
            "tol": _get(cfg, "primal_dual_converger_tol", 1e-2),
        }
    return hub_dict


# cfg_vanilla.py:202-224 (options stay loose in the hub's options dict, as there)
def add_wxbar_read_write(hub_dict, cfg):
    if getattr(cfg, "init_W_fname", None) is not None or getattr(cfg, "init_Xbar_fname", None) is not None:
        hub_dict = extension_adder(hub_dict, WXBarReader)
        hub_dict["opt_kwargs"]["options"].update({
            "init_W_fname": getattr(cfg, "init_W_fname", None),
            "init_Xbar_fname": getattr(cfg, "init_Xbar_fname", None),
            "init_separate_W_files": bool(getattr(cfg, "init_separate_W_files", False)),
        })
    if getattr(cfg, "W_fname", None) is not None or getattr(cfg, "Xbar_fname", None) is not None:
        hub_dict = extension_adder(hub_dict, WXBarWriter)
        hub_dict["opt_kwargs"]["options"].update({
            "W_fname": getattr(cfg, "W_fname", None),
            "Xbar_fname": getattr(cfg, "Xbar_fname", None),
            "separate_W_files": bool(getattr(cfg, "separate_W_files", False)),
        })
    return hub_dict
