"""ExtensiveForm (mirrors mpisppy/opt/ef.py): the extensive form of all scenarios,
solved by the Schur-complement interior point of ``opt/sc.py`` on one rank.

Same constructor and methods as the reference: ``solve_extensive_form``, ``get_objective_value``,
``get_root_solution``, ``nonants``, ``nonants_to_csv``, ``scenarios``.  The reference builds one
Pyomo model with a reference variable per nonant and hands it to ``options["solver"]``; here
``options["solver"]`` names this engine (one of ``spopt.SOLVER_NAMES``) and no model of the whole
is built: the scenarios stay a batch and the nonants are one vector z on the device.

DEPARTURES.  Two-stage continuous problems only (a multistage tree raises RuntimeError);
``bundles_per_rank`` raises NotImplementedError; ``solver_options`` takes ``tol`` and ``max_iter``.
The results object is the kind ``spopt.py`` builds for a scenario (termination condition, bounds);
``first_stage_solution_available`` and ``tree_solution_available`` are set by an optimal solve only.
"""
from .. import _lib
from ..comm import Comm
from ..spopt import ScenarioResults, SOLVER_NAMES
from .sc import SchurComplement


class _OneRank(Comm):
    """The extensive form is one problem: it does not split over the ranks of a process group."""

    def __init__(self):
        self.group, self.rank, self.size = None, 0, 1


class ExtensiveForm(SchurComplement):
    # ef.py:39-64
    def __init__(self, options, all_scenario_names, scenario_creator, scenario_creator_kwargs=None,
                 all_nodenames=None, model_name=None, suppress_warnings=False):
        options = dict(options or {})
        self._options_check(["solver"], options)
        if options["solver"] not in SOLVER_NAMES:
            raise RuntimeError(f"solver {options['solver']!r} is not served by this engine; use one of {SOLVER_NAMES}")
        if options.get("bundles_per_rank", 0):
            raise NotImplementedError("bundles (spbase.py:184-216) are outside the batched engine: the extensive "
                                      "form is solved over the scenarios themselves")
        options["solver_name"] = options["solver"]
        super().__init__(options, all_scenario_names, scenario_creator, scenario_creator_kwargs=scenario_creator_kwargs,
                         all_nodenames=all_nodenames, mpicomm=_OneRank(), model_name=model_name,
                         suppress_warnings=suppress_warnings)

    # ef.py:66-95
    def solve_extensive_form(self, solver_options=None, tee=False):
        so = {k: v for k, v in (solver_options or {}).items() if k not in self.FOREIGN_SOLVER_OPTIONS}
        unknown = set(so) - {"tol", "max_iter"}
        if unknown:
            raise ValueError(f"solver_options {sorted(unknown)} are not served; the interior point takes tol and max_iter")
        self.tol = float(so.get("tol", self.tol))
        self.max_iter = int(so.get("max_iter", self.max_iter))
        self.verbose = self.verbose or bool(tee)
        self.first_stage_solution_available = False
        self.tree_solution_available = False
        done = self._run()
        obj = self.get_objective_value()
        return ScenarioResults(_lib.OPTIMAL if done else _lib.ITER_LIMIT, obj, obj, self.iterations, self.batch.sense)

    # ef.py:97-112
    def get_objective_value(self):
        if self.engine is None or self.status is None:
            raise ValueError("Could not extract EF objective value with error: the extensive form has not been solved")
        return self.Eobjective()

    def _nonant_names(self):
        b = self.batch
        if b.nonant_names is not None:
            return list(b.nonant_names)
        return [b.var_names[j] if b.var_names is not None else f"x[{j}]" for j in b.nonant_col]

    # ef.py:114-129
    def get_root_solution(self):
        if self.status is None:
            raise ValueError("the extensive form has not been solved")
        return {nm: float(v) for nm, v in zip(self._nonant_names(), self.root_nonants())}

    # ef.py:131-139 (sputils.ef_nonants)
    def nonants(self):
        for nm, v in self.get_root_solution().items():
            yield "ROOT", nm, v

    # ef.py:141-147 (sputils.ef_nonants_csv)
    def nonants_to_csv(self, filename):
        with open(filename, "w") as f:
            f.write("Node, EF_VarName, Value\n")
            for nd, nm, v in self.nonants():
                f.write(f"{nd}, {nm}, {v}\n")

    # ef.py:149-157
    def scenarios(self):
        yield from self.local_scenarios.items()
