"""Fixer: WW-style fixing of converged nonants, on the device (mirrors
mpisppy/extensions/fixer.py:20-329).

The reference walks every scenario's tuples on the host, keeps a counter per (scenario,
nonant) of the consecutive iterations in which |x̄² - E[x²]| stayed under the squared
threshold, and calls ``xvar.fix`` after a lag.  Here the counters, the decisions and the
bound rewrite are one device pass over every local (nonant, scenario)
(engine.fixer_step -> phgpu_fixer_step, include/phgpu.h), enqueued from ``miditer`` with no
host synchronisation; the rule itself is restated there line by line.

Options, as in the reference: ``options["fixeroptions"] = {"verbose", "boundtol",
"id_fix_list_fct"}`` with ``id_fix_list_fct(scenario) -> (iter0 tuples | None, iterk tuples |
None)`` of ``Fixer_tuple`` keyed by ``id(var)``.  With a ``batch_creator`` there are no
per-scenario models: pass ``fixeroptions["fix_arrays"] = {"iter0": {...}, "iterk": {...}}``,
each with ``th`` / ``nb`` / ``lb`` / ``ub`` arrays of length nn (None or a negative lag: the
reference's None), or None in place of a dict for "no tuples".

THIS DEPARTS FROM fixer.py in two places:

* lags are per nonant, not per nonant and scenario (thresholds already are, fixer.py:88-102):
  ``populate`` raises the reference's RuntimeError for thresholds and a ValueError for lags
  that differ between local scenarios;
* "Variation in fixing across scenarios" is tested per node entry (a call must newly fix
  none or all of a node entry's local scenarios) where the reference tests
  ``raw_fixed % len(local_scenarios)`` (fixer.py:217-223, 302-304): the same test for two
  stages, but on a tree that one raises on legitimate per-node fixing.  It is raised where
  the totals are read: at each progress line with ``display_progress`` / ``verbose``,
  otherwise once in ``post_everything``.  The reference's second iter0 test (fixed on arrival
  in some scenarios only) is not made.

A nonant without a tuple has th = 0 and no lags: it is never fixed and its counter stays 0
(the reference's ``_update_fix_counts`` would raise KeyError for it, fixer.py:122).
``fixed_so_far`` / ``fixed_prior_iter0`` keep the reference's formula (entries / local
scenarios).  ``verbose`` prints the progress line only, not the reference's line per fixed
variable (the values stay on the device).
"""
import numpy as np

from .. import _lib
from .extension import Extension


def Fixer_tuple(xvar, th=None, nb=None, lb=None, ub=None):
    """fixer.py:20-48: (id(xvar), th, nb, lb, ub), with the reference's warnings."""
    if th is None and nb is None and lb is None and ub is None:
        print("warning: Fixer_tuple called for Var=", xvar.name, "but no arguments were given")
    if th is None:
        th = 0
    if nb is not None and lb is not None and nb < lb:
        print("warning: Fixer_tuple called for Var=", xvar.name, "with nb < lb, which means lb will be ignored.")
    if nb is not None and ub is not None and nb < ub:
        print("warning: Fixer_tuple called for Var=", xvar.name, "with nb < ub, which means ub will be ignored.")
    return (id(xvar), th, nb, lb, ub)


def uniform_fix_list_fct(th, nb=None, lb=None, ub=None, iter0=None):
    """An ``id_fix_list_fct`` that gives every nonant of a LinearModel the same iterk tuple
    (th, nb, lb, ub).  ``iter0``: a dict of the same four for the iter0 tuples; None gives
    iter0 tuples with the threshold and no lag, which never fix."""
    i0 = dict(iter0) if iter0 is not None else {"th": th}

    def fct(scenario):
        xs = [v for nd in scenario._mpisppy_node_list for v in nd.nonant_vardata_list]
        return ([Fixer_tuple(v, **i0) for v in xs], [Fixer_tuple(v, th=th, nb=nb, lb=lb, ub=ub) for v in xs])

    return fct


def _lag(v):
    return -1 if v is None or int(v) < 0 else int(v)


class Fixer(Extension):
    # fixer.py:52-64
    def __init__(self, ph):
        super().__init__(ph)
        if getattr(ph, "bundling", False):
            raise NotImplementedError("the Fixer is not served with bundles: it fixes nonant columns, and a bundle's "
                                      "interior point needs an interior in every nonant")
        self.ph = ph
        self.cylinder_rank = self.ph.cylinder_rank
        self.options = ph.options
        self.fixeroptions = self.options["fixeroptions"]  # required
        self.verbose = bool(self.options["verbose"] or self.fixeroptions.get("verbose", False))
        self.id_fix_list_fct = self.fixeroptions.get("id_fix_list_fct")
        self.dprogress = bool(ph.options["display_progress"])
        self.fixed_prior_iter0 = 0
        self.fixed_so_far = 0
        self.boundtol = float(self.fixeroptions["boundtol"])
        # miditer only enqueues device work unless the progress line reads the totals back
        self.miditer_on_device = not (self.verbose or self.dprogress)
        self._arrays = {"iter0": None, "iterk": None}
        self._dev = {}

    # fixer.py:66-102: per nonant th and lags of the iter0 and the iterk tuples
    def populate(self, local_scenarios):
        self._populate_arrays(local_scenarios)
        e = getattr(self.ph, "engine", None)
        if e is not None:
            # the state and the per-nonant inputs go to the device here, outside the PH loop
            import torch
            e.fixer_prepare()
            for which, arrays in self._arrays.items():
                if arrays is not None:
                    self._dev[which] = (e.fixer_arg(arrays[0], torch.float64),) + tuple(
                        e.fixer_arg(torch.as_tensor(a), torch.int32) for a in arrays[1:])

    def _populate_arrays(self, local_scenarios):
        self.local_scenarios = local_scenarios
        nn = self.ph.batch.nn
        self._nlocal = max(1, len(self.ph.local_scenario_names))
        if not local_scenarios:
            fa = self.fixeroptions.get("fix_arrays")
            if fa is None:
                raise RuntimeError("Fixer needs per-scenario models for id_fix_list_fct; with a batch_creator "
                                   "pass fixeroptions['fix_arrays']")
            for which in ("iter0", "iterk"):
                d = fa.get(which)
                if d is None:
                    continue
                th = np.zeros(nn) if d.get("th") is None else np.asarray(d["th"], dtype=np.float64)
                lags = [np.array([_lag(v) for v in (d.get(key) if d.get(key) is not None else [None] * nn)],
                                 dtype=np.int32) for key in ("nb", "lb", "ub")]
                if any(len(a) != nn for a in [th] + lags):
                    raise ValueError(f"fix_arrays[{which!r}] arrays must have length {nn}")
                self._arrays[which] = (th, *lags)
            return
        per = {"iter0": [], "iterk": []}
        for sname, s in local_scenarios.items():
            id2k = {}
            k = 0
            for nd in s._mpisppy_node_list:
                for v in nd.nonant_vardata_list:
                    id2k[id(v)] = k
                    k += 1
            for which, tuples in zip(("iter0", "iterk"), self.id_fix_list_fct(s)):
                if tuples is None:
                    per[which].append(None)
                    continue
                th = np.zeros(nn)
                lags = np.full((3, nn), -1, dtype=np.int32)
                for (varid, t, nb, lb, ub) in tuples:
                    try:
                        k = id2k[varid]
                    except KeyError:
                        print("Are you trying to fix a Var that is not nonant?")
                        raise
                    th[k] = t
                    lags[:, k] = (_lag(nb), _lag(lb), _lag(ub))
                per[which].append((sname, th, lags))
        for which, rows in per.items():
            if any(r is None for r in rows):
                continue                      # miditer warns and does nothing (fixer.py:148-150, 243-245)
            _, th0, lags0 = rows[0]
            for sname, th, lags in rows[1:]:
                if not np.array_equal(th, th0):
                    k = int(np.flatnonzero(th != th0)[0])
                    print(sname, k, th[k])
                    raise RuntimeError("Attempt to vary iter0 fixer threshold across scenarios."
                                       if which == "iter0" else
                                       "Attempt to vary fixer threshold across scenarios")
                if not np.array_equal(lags, lags0):
                    raise ValueError(f"Attempt to vary {which} fixer lags across scenarios ({sname}): "
                                     "lags are per nonant on this engine")
            self._arrays[which] = (th0, lags0[0], lags0[1], lags0[2])

    # display progress utility (fixer.py:110-112)
    def _dp(self, msg):
        if (self.dprogress or self.verbose) and self.cylinder_rank == 0:
            print("(rank0) " + msg)

    def _read_totals(self):
        fixed, arrived, variation = self.ph.engine.fixer_totals_host()
        self.fixed_so_far = fixed / self._nlocal
        self.fixed_prior_iter0 = arrived / self._nlocal
        return variation

    def _check_variation(self, variation):
        if variation:
            raise RuntimeError("Variation in fixing across scenarios detected in fixer.py")

    def post_iter0(self):
        """fixer.py:309-312: the data structures; that is all that can be done here."""
        self.populate(self.ph.local_scenarios)

    # fixer.py:314-322 (iter0: 131-223, iterk: 226-304)
    def miditer(self):
        iter0 = self.ph._PHIter == 1
        which = "iter0" if iter0 else "iterk"
        arrays = self._arrays[which]
        if arrays is None:
            print("WARNING: No Iter0 fixer tuple" if iter0 else "MAJOR WARNING: No Iter k fixer tuple",
                  "for some local scenario of rank", self.cylinder_rank)
            return
        e = self.ph.engine
        dev = self._dev[which]
        e.fixer_step(_lib.FixerParams(boundtol=self.boundtol, iter0=1 if iter0 else 0), *dev)
        if self.dprogress or self.verbose:
            variation = self._read_totals()
            self._dp("Unique vars fixed so far - %d (%d prior to iteration 0)"
                     % (self.fixed_so_far + self.fixed_prior_iter0, self.fixed_prior_iter0))
            self._check_variation(variation)

    # fixer.py:327-329
    def post_everything(self):
        variation = self._read_totals()
        self._dp("Final unique vars fixed by fixer= %s" % (self.fixed_so_far))
        self._check_variation(variation)
