"""Find_Grad: the gradient cost of every scenario at an xhat and the rho it gives, on the
device (mirrors mpisppy/utils/gradient.py:44-175; the Config / argparse driver
grad_cost_and_rho, :181-247, is not carried over).

``cfg`` is a dict or any object with the reference's attribute names: ``xhatpath`` (a .npy
file of the ROOT nonants, ciutils.read_xhat), ``grad_cost_file``, ``grad_rho_file``,
``order_stat``, ``rho_relative_bound``; and, in place of a file, ``xhat`` (an array or
``{"ROOT": array}``).  Without an xhat the cost is taken at the current x̄.

Deviations from the reference, all stated in DESIGN.md 3.14:

* the cost is the derivative with respect to the nonant itself.  compute_grad indexes
  pynumero's gradient, which is in NLP variable order, by the nonant's position
  (gradient.py:78-80), so its farmer costs are labelled with the wrong crops;
* no solve: the objective is linear plus a diagonal quadratic, so the nonants' derivative
  depends on the nonant values alone (engine.grad_cost -> phgpu_grad_cost);
* the cost is that of the stored objective, a minimisation (a maximise model is stored
  negated); only its absolute value enters rho;
* the cost dictionary and the rho dictionary exist on every rank, not on rank 0 only.
"""
import csv
import os

import numpy as np
import torch

from . import find_rho
from .find_rho import cfg_get
from .wxbarutils import nonant_names


def cfg_set(cfg, name, value):
    if isinstance(cfg, dict):
        cfg[name] = value
    else:
        setattr(cfg, name, value)


class Find_Grad:
    """gradient.py:44-61.  ``c``: {(scenario name, nonant name): cost} once asked for;
    ``cost``: the device [nn, S] cost of this rank's scenarios."""

    def __init__(self, ph_object, cfg):
        self.ph_object = ph_object
        self.cfg = cfg
        self.c = dict()
        self.cost = None

    def _two_stage(self):
        if self.ph_object.multistage:
            raise RuntimeError("gradient cost and rho only work for two stage for now")   # find_rho.py:89

    def _xhat_dev(self):
        """The [nn, S] evaluation point: cfg xhat / xhatpath for every scenario, else x̄."""
        e = self.ph_object.engine
        xhat = cfg_get(self.cfg, "xhat")
        if xhat is None and cfg_get(self.cfg, "xhatpath") is not None:
            path = cfg_get(self.cfg, "xhatpath")
            if not os.path.exists(path):
                raise RuntimeError("Could not find file {fn}".format(fn=path))
            xhat = np.load(path)                                       # ciutils.read_xhat
        if xhat is None:
            e._flush_xbar()
            return e.xbar
        if isinstance(xhat, dict):
            xhat = xhat["ROOT"]
        v = torch.as_tensor(np.asarray(xhat, dtype=np.float64).reshape(-1), device=e.device)
        if v.numel() != e.nn:
            raise RuntimeError(f"xhat has {v.numel()} entries, the scenarios have {e.nn} nonants")
        return v[:, None].expand(e.nn, e.S).contiguous()

    # gradient.py:65-122
    def find_grad_cost(self, want_dict=None):
        """Fill ``cost`` on the device; with ``want_dict`` (default: when cfg names a
        grad_cost_file) also ``c``, gathered over the ranks."""
        self._two_stage()
        e = self.ph_object.engine
        self.cost = e.grad_cost(self._xhat_dev())
        if want_dict is None:
            want_dict = cfg_get(self.cfg, "grad_cost_file") is not None
        if want_dict:
            host = self.cost[:e.nn].T.cpu().numpy()
            names = nonant_names(self.ph_object)
            local = {(sname, vname): float(host[s, k])
                     for s, sname in enumerate(self.ph_object.local_scenario_names)
                     for k, vname in enumerate(names)}
            self.c = {key: val for part in self.ph_object.mpicomm.allgather_object(local)
                      for key, val in part.items()}
        return self.cost

    # gradient.py:125-141
    def write_grad_cost(self):
        self.find_grad_cost(want_dict=True)
        if self.ph_object.cylinder_rank == 0:
            with open(cfg_get(self.cfg, "grad_cost_file"), "a") as f:
                writer = csv.writer(f)
                writer.writerow(["#grad cost values"])
                for (sname, vname), val in self.c.items():
                    writer.writerow([sname, vname, str(val)])
        self.ph_object.mpicomm.Barrier()

    # gradient.py:146-157: from the device cost when there is one, else from the cost file
    def find_grad_rho(self, indep_denom=False):
        if self.cost is not None:
            return find_rho.Find_Rho(self.ph_object, self.cfg, cost=self.cost).compute_rho(indep_denom)
        fn = cfg_get(self.cfg, "grad_cost_file")
        assert fn is not None, "to compute rho you have to give the name of a csv file (grad_cost_file)"
        if not os.path.exists(fn):
            raise RuntimeError("Could not find file {fn}".format(fn=fn))
        cfg_set(self.cfg, "whatpath", fn)
        return find_rho.Find_Rho(self.ph_object, self.cfg).compute_rho(indep_denom)

    # gradient.py:159-175
    def write_grad_rho(self):
        fn = cfg_get(self.cfg, "grad_rho_file")
        if fn is None:
            return
        rho_data = self.find_grad_rho()
        if self.ph_object.cylinder_rank == 0:
            with open(fn, "a", newline="") as f:
                writer = csv.writer(f)
                writer.writerow(["#grad rho values"])
                for vname, rho in rho_data.items():
                    writer.writerow([vname, rho])
        self.ph_object.mpicomm.Barrier()
