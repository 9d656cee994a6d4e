"""Find_Rho / Set_Rho: rho from a cost vector by the WW heuristic rho = |cost| / |x - x̄|
(mirrors mpisppy/utils/find_rho.py:45-259; the Config / argparse driver get_rho_from_W,
:264-327, is not carried over).  Two-stage problems only, as the reference (:89, :109, :128).

``cfg`` is a dict or any object with the reference's attribute names: ``whatpath`` (a cost /
What csv: ``scenario,variable,value`` rows), ``rho_file``, ``rho_path``, ``order_stat``,
``rho_relative_bound``.  The cost comes from that file or from a device [nn, S] array
(Find_Grad's).

The per-scenario ratios never leave the device: engine.rho_ratio_stats reduces them to each
nonant's sum, minimum and maximum (phgpu_rho_ratio_stats + one SUM and one MAX all-reduce),
which is all _order_stat needs.  ``compute_rho`` returns {nonant name: rho} on EVERY rank; the
reference gathers to rank 0, returns it there only, and hands it to the rho setter through a
file.  ``apply`` writes the same rho to every local scenario on the device.
"""
import csv
import os

import numpy as np
import torch

from .wxbarutils import nonant_names


def cfg_get(cfg, name, default=None):
    """``cfg.name`` / ``cfg[name]``; ``default`` when missing, None or the empty string."""
    v = cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)
    return default if v is None or (isinstance(v, str) and v == "") else v


def read_cost_file(path):
    """find_rho.py:69-75, the reference's parsing kept: '#' lines skipped, the third field
    without its last two characters.  Those are the "\\r\\n" the csv module ends a row with;
    the file is opened without newline translation, so that they are both still there."""
    if not os.path.exists(path):
        raise RuntimeError("Could not find file {fn}".format(fn=path))
    c = dict()
    with open(path, "r", newline="") as f:
        for line in f:
            if line.startswith("#"):
                continue
            line = line.split(",")
            cval = float(line[2][:-2])
            c[(line[0], line[1])] = cval
    return c


def order_stat(alpha, rho_mean, rho_min, rho_max):
    """find_rho.py:159-168 from the three statistics."""
    assert alpha is not None and alpha != -1.0, "you need to set the order statistic parameter for rho (order_stat)"
    assert (alpha >= 0 and alpha <= 1), "0 is the min, 0.5 the average, 1 the max"
    if alpha == 0.5:
        return rho_mean
    if alpha < 0.5:
        return (rho_min + alpha * 2 * (rho_mean - rho_min))
    return (2 * rho_mean - rho_max) + alpha * 2 * (rho_max - rho_mean)


class Find_Rho:
    """find_rho.py:45-75.  ``c``: {(scenario name, nonant name): cost} when read from a file."""

    def __init__(self, ph_object, cfg, cost=None, refresh_xbar=True):
        """``cost``: a device [nn, S] array used instead of ``cfg.whatpath``.  ``refresh_xbar``:
        the scenario-independent denominator recomputes x̄ from the current x first, as
        _grad_denom does (find_rho.py:125); False inside the PH loop, where x̄ is current."""
        self.ph_object = ph_object
        self.cfg = cfg
        self.c = dict()
        self.cost = cost
        self.refresh_xbar = refresh_xbar
        if ph_object.multistage:
            raise RuntimeError("compute rho only works for two stage for now")
        if cost is None and cfg_get(cfg, "whatpath") is not None:
            self.c = read_cost_file(cfg_get(cfg, "whatpath"))

    # -- the cost as a device array
    def _cost_dev(self):
        if self.cost is not None:
            return self.cost
        if not self.c:
            raise RuntimeError("to compute rhos you have to give a cost array or the name of a What csv file "
                               "(whatpath)")
        ph = self.ph_object
        e = ph.engine
        names = nonant_names(ph)
        host = np.array([[self.c[(sname, vname)] for sname in ph.local_scenario_names] for vname in names],
                        dtype=np.float64).reshape(e.nn, e.S)
        self.cost = torch.as_tensor(host, device=e.device)
        return self.cost

    # -- host views of the reference's three denominators (s: local scenario index)
    def _dx(self):
        e = self.ph_object.engine
        return np.abs(e.nonant_x() - e.host("xbar")[:, :e.nn])

    def _w_denom(self, s):
        return self._dx()[s]                                            # find_rho.py:78-95

    def _prox_denom(self, s):
        return 2 * np.square(self._dx()[s])                             # find_rho.py:98-115

    def _refresh(self):
        e = self.ph_object.engine
        e.compute_xbar()
        e.update(update_W=False)
        e.convergence_diff()

    def _grad_denom(self):
        """find_rho.py:118-147, on every rank."""
        if self.refresh_xbar:
            self._refresh()
        e = self.ph_object.engine
        e.residuals()
        g = e.residual_planes()[1][:e.nn]
        return np.maximum(np.ones(len(g)) / float(cfg_get(self.cfg, "rho_relative_bound", 1e3)), g)

    def _order_stat(self, rho_list):
        rho_list = np.asarray(rho_list, dtype=np.float64)
        return order_stat(cfg_get(self.cfg, "order_stat", -1.0), np.mean(rho_list), np.min(rho_list), np.max(rho_list))

    def _stats(self, indep_denom):
        if indep_denom and self.refresh_xbar:
            self._refresh()
        e = self.ph_object.engine
        return e.rho_ratio_stats(self._cost_dev(), indep_denom, float(cfg_get(self.cfg, "rho_relative_bound", 1e3)))

    # find_rho.py:170-204
    def compute_rho(self, indep_denom=False):
        e = self.ph_object.engine
        p = self._stats(indep_denom).reshape(3, -1).cpu().numpy()[:, :e.nn]
        alpha = cfg_get(self.cfg, "order_stat", -1.0)
        S_total = e.total_scenarios()
        return {vname: float(order_stat(alpha, p[0, k] / S_total, -p[1, k], p[2, k]))
                for k, vname in enumerate(nonant_names(self.ph_object))}

    def apply(self, indep_denom=False, gate=None, thr=0.05, applied=None):
        """The same rho written to every local scenario on the device (engine.find_rho), if the
        dual metric ``gate`` moved by at most ``thr``; nothing is read back."""
        if indep_denom and self.refresh_xbar:
            self._refresh()
        self.ph_object.engine.find_rho(self._cost_dev(), float(cfg_get(self.cfg, "order_stat", -1.0)), indep_denom,
                                       float(cfg_get(self.cfg, "rho_relative_bound", 1e3)), gate=gate, thr=thr,
                                       applied=applied)

    # find_rho.py:207-218
    def write_rho(self):
        fn = cfg_get(self.cfg, "rho_file")
        if fn is None:
            return
        rho_data = self.compute_rho()
        if self.ph_object.cylinder_rank == 0:
            with open(fn, "w") as f:
                writer = csv.writer(f)
                writer.writerow(["#Rho values"])
                for (vname, rho) in rho_data.items():
                    writer.writerow([vname, rho])


def read_rho_file(path):
    """{variable name: rho} of a rho csv (find_rho.py:246-252)."""
    out = dict()
    with open(path) as infile:
        for row in csv.reader(infile):
            if not row or row[0].startswith("#"):
                continue
            out[row[0]] = float(row[1])
    return out


class Set_Rho:
    """find_rho.py:221-259: a ``rho_setter`` that reads ``cfg.rho_path``.  It serves this
    package's rho_setter protocol (PHBase._use_rho_setter): per-scenario models are needed,
    so it is for PH objects built from a scenario_creator, not from a batch_creator."""

    def __init__(self, cfg):
        self.cfg = cfg

    def rho_setter(self, scenario):
        assert self.cfg is not None, "you have to give the rho_setter a cfg"
        rhofile = cfg_get(self.cfg, "rho_path")
        assert rhofile is not None, "use rho_path to give the path of your rhos file"
        rhos = read_rho_file(rhofile)
        byname = {v.name: v for nd in scenario._mpisppy_node_list for v in nd.nonant_vardata_list}
        rho_list = list()
        for fullname, rho in rhos.items():
            vo = byname.get(fullname)
            if vo is None:
                raise RuntimeError(f"rho values from {rhofile} found Var {fullname} "
                                   f"that is not found in the scenario given (name={getattr(scenario, 'name', None)})")
            rho_list.append((id(vo), rho))
        return rho_list
