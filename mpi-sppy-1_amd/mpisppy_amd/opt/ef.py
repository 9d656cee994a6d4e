"""ExtensiveForm (mirrors mpisppy/opt/ef.py): the extensive form of all
scenarios, solved by the Schur-complement interior point of ``opt/sc.py`` on one rank.  On a
multistage tree (``all_nodenames``, as ``sputils.create_EF`` ties the nonants of every non-leaf
node) the Schur complement is eliminated along the tree (phgpu_eft_*).

Same constructor and methods as the reference: ``solve_extensive_form``, ``get_objective_value``,
``get_root_solution``, ``nonants``, ``nonants_to_csv``, ``scenarios``.  The reference builds one
Pyomo model with a reference variable per nonant and hands it to ``options["solver"]``; here
``options["solver"]`` names this engine (one of ``spopt.SOLVER_NAMES``) and no model of the whole
is built: the scenarios stay a batch and the nonants are one vector z on the device.

On a tree, ``fix_node_nonants`` holds the nonants of chosen nodes at given values for the solves that
follow (the CONDITIONED extensive form, DESIGN.md 3.24: what sample_tree.py's SampleSubtree does by
fixing its ancestors' Vars); ``node_objectives`` then gives every subtree's own objective.

DEPARTURES.  Continuous problems; a tree must have all its scenarios at the same depth and the
scenarios in tree order, so that every node's scenarios are contiguous (RuntimeError otherwise);
the whole path has at most 64 nonants; ``bundles_per_rank`` raises NotImplementedError; ``solver_options`` takes ``tol`` and ``max_iter``.
The results object is the kind ``spopt.py`` builds for a scenario (termination condition, bounds);
``first_stage_solution_available`` and ``tree_solution_available`` are set by an optimal solve only.
"""
import numpy as np

from .. import _lib
from ..comm import Comm
from ..spopt import ScenarioResults, SOLVER_NAMES
from .sc import SchurComplement


class _OneRank(Comm):
    """The extensive form is one problem: it does not split over the ranks of a process group."""

    def __init__(self):
        self.group, self.rank, self.size = None, 0, 1


class ExtensiveForm(SchurComplement):
    _serves_trees = True

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

    def _tree_layout(self):
        """The non-leaf nodes as phgpu_eft_init takes them, from the batch's node_of: (nlens [D],
        node_depth, node_parent [Nn], seg_start [G + 1]).  Refuses, saying which condition failed, a
        tree whose nodes are not numbered depth by depth with siblings adjacent and one whose
        scenarios are not in tree order."""
        b = self.batch
        D, nof = b.depth, np.asarray(b.node_of)
        Nn = len(b.node_names)
        if not np.all(np.diff(b.nonant_depth) >= 0):
            raise RuntimeError("the nonants of a scenario are not ordered by the depth of their node")
        depth, parent = np.full(Nn, -1, dtype=np.int32), np.full(Nn, -1, dtype=np.int32)
        for d in range(D):
            ids = nof[:, d]
            if np.any(depth[ids] >= 0) and np.any(depth[ids][depth[ids] >= 0] != d):
                raise RuntimeError(f"the scenarios do not all have the same depth: a node of depth {d} is at another depth "
                                   f"in another scenario")
            depth[ids] = d
            if d:
                if np.any((parent[ids] >= 0) & (parent[ids] != nof[:, d - 1])):
                    raise RuntimeError(f"a node of depth {d} has two parents")
                parent[ids] = nof[:, d - 1]
            runs = 1 + int(np.count_nonzero(np.diff(ids)))
            if runs != len(np.unique(ids)):
                nd = next(n for n in np.unique(ids) if np.count_nonzero(np.diff(np.flatnonzero(ids == n)) > 1))
                raise RuntimeError(f"the local scenarios are not in tree order: the scenarios of node {b.node_names[nd]} are not "
                                   f"contiguous")
        if np.any(depth < 0):
            nd = int(np.flatnonzero(depth < 0)[0])
            raise RuntimeError(f"node {b.node_names[nd]} has none of the scenarios: the extensive form takes the whole tree")
        ok = depth[0] == 0 and np.all(np.diff(depth) >= 0) and np.all(np.diff(depth) <= 1)
        for d in range(1, D):
            ok = ok and bool(np.all(np.diff(parent[depth == d]) >= 0))
            ok = ok and bool(np.all(np.diff(nof[:, d]) >= 0))
        if not ok:
            raise RuntimeError("the tree's nodes are not numbered depth by depth with siblings adjacent (node_names order)")
        deep = nof[:, D - 1]
        seg_start = np.concatenate([[0], 1 + np.flatnonzero(np.diff(deep)), [b.S]]).astype(np.int32)
        return np.asarray(b.nlens(), dtype=np.int32), depth, parent, seg_start

    def _problem_data(self):
        """Two-stage: SchurComplement's.  A tree: (layout, zlb, zub, cz, qz [Ztot], ncomp, cmax, qp) with
        z's data per node as ``SchurComplement._global_data`` has them once: the tightest bounds and
        the probability-weighted cost and diagonal over the node's scenarios."""
        if not self._tree:
            return super()._problem_data()
        b = self.batch
        if b.nn > 64 or b.m > 64:
            raise NotImplementedError(f"the Schur-complement interior point serves nn <= 64 and m <= 64 (path nn {b.nn}, m {b.m})")
        layout = self._tree_layout()
        nlens, depth, parent, _ = layout
        nc = np.asarray(b.nonant_col, dtype=np.int64)
        slot = np.full(b.n, -1, dtype=np.int64)
        slot[nc] = np.arange(b.nn)
        for i in range(b.m):
            cols = b.col_idx[b.row_ptr[i]:b.row_ptr[i + 1]]
            if len(cols) and np.all(slot[cols] >= 0) and np.any(b.rl[:, i] == b.ru[:, i]):
                s = int(np.flatnonzero(b.rl[:, i] == b.ru[:, i])[0])
                raise NotImplementedError(f"row {i} has only nonant columns and equal sides [{b.rl[s, i]}, {b.ru[s, i]}] in "
                                          f"scenario {s}: its block of the scenario's normal matrix has no interior")
        zoff = np.concatenate([[0], np.cumsum(nlens[depth])])
        Ztot = int(zoff[-1])
        zlb, zub, cz, qz = np.full(Ztot, -np.inf), np.full(Ztot, np.inf), np.zeros(Ztot), np.zeros(Ztot)
        P = np.concatenate([[0], np.cumsum(nlens)])
        for d in range(b.depth):
            cols = nc[P[d]:P[d + 1]]
            for o, j in enumerate(cols):
                zi = zoff[b.node_of[:, d]] + o
                np.maximum.at(zlb, zi, b.lb[:, j])
                np.minimum.at(zub, zi, b.ub[:, j])
                np.add.at(cz, zi, b.prob * b.c[:, j])
                np.add.at(qz, zi, b.prob * b.q[:, j])
        held = self._held_z()
        free = np.ones(Ztot, dtype=bool) if held is None else np.isnan(held)
        if not np.all(zlb[free] < zub[free]):
            k = int(np.flatnonzero(free & ~(zlb < zub))[0])
            nd = int(np.searchsorted(zoff, k, side="right") - 1)
            raise NotImplementedError(f"nonant {k - zoff[nd]} of node {b.node_names[nd]} has the bounds [{zlb[k]}, {zub[k]}] over "
                                      f"its scenarios: a fixed column leaves the interior point no interior")
        # an entry held through fix_node_nonants needs no interior: where its bounds coincide at its
        # value, phgpu_eft_init (which asks zlb < zub of every entry) gets a box around them
        if held is not None:
            shut = (zlb == zub) & (held == zlb)
            zlb[shut] -= 1.0
            zub[shut] += 1.0
        oth = np.setdiff1d(np.arange(b.n), nc)
        ranged = b.rl < b.ru
        # (ncomp counts every z entry's finite bounds, as phgpu_eft_init takes it; phgpu_eft_fix leaves
        # the held entries' out again)
        ncomp = (np.isfinite(b.lb[:, oth]).sum() + np.isfinite(b.ub[:, oth]).sum() + (np.isfinite(b.rl) & ranged).sum()
                 + (np.isfinite(b.ru) & ranged).sum() + np.isfinite(zlb).sum() + np.isfinite(zub).sum())
        return layout, zlb, zub, cz, qz, float(ncomp), float(np.abs(b.c).max(initial=0.0)), bool(np.any(b.q))

    # ------------------------------------------------------------------ the conditioned extensive form
    def fix_node_nonants(self, cache):
        """Hold the nonants of nodes at values in every ``solve_extensive_form`` that follows:
        ``cache`` is {node name: values}; a node that is missing and an entry that is NaN stay free.
        After the solve ``nonants()`` and ``tree_nonants()`` return the held values bit for bit.
        ``free_node_nonants()`` undoes it.  A two-stage problem (phgpu_ef_*) is not served."""
        if not self._tree:
            raise NotImplementedError("fix_node_nonants serves the multistage extensive form only: with ROOT's nonants "
                                      "held a two-stage problem is S separate scenario problems (Xhat_Eval)")
        b = self.batch
        nlens, depth, _, _ = self._tree_layout()
        fix = {}
        for nd, vals in dict(cache).items():
            if nd not in b.node_names:
                raise RuntimeError(f"fix_node_nonants: {nd} is not a non-leaf node of the tree")
            if vals is None:
                continue
            v = np.array(vals, dtype=np.float64).reshape(-1)
            want = int(nlens[depth[list(b.node_names).index(nd)]])
            if len(v) != want:
                raise RuntimeError(f"fix_node_nonants: node {nd} has {want} nonants, {len(v)} values given")
            fix[nd] = v
        self._node_fix = fix or None

    def free_node_nonants(self):
        self._node_fix = None

    def _held_z(self):
        fix = getattr(self, "_node_fix", None)
        if not fix:
            return None
        nlens, depth, _, _ = self._tree_layout()
        zoff = np.concatenate([[0], np.cumsum(nlens[depth])])
        z = np.full(int(zoff[-1]), np.nan)
        names = list(self.batch.node_names)
        for nd, v in fix.items():
            n = names.index(nd)
            z[zoff[n]:zoff[n + 1]] = v
        return None if np.all(np.isnan(z)) else z

    def node_objectives(self, depth):
        """Per node of tree depth ``depth`` (0: ROOT), in node order: (node name, sum of p_s f_s over
        the node's scenarios / the node's probability) of the last solve -- with the nodes above held,
        the objective of that node's subtree alone (sample_tree.py's EF_Obj).  One read of the
        exported per-scenario objectives, summed in index order."""
        if self.status is None:
            raise ValueError("the extensive form has not been solved")
        b = self.batch
        if not 0 <= depth < b.depth:
            raise ValueError(f"depth {depth} (the tree has the non-leaf depths 0..{b.depth - 1})")
        f = b.sense * self.engine.obj.cpu().numpy()
        ids = np.asarray(b.node_of)[:, depth]
        out = []
        for n in np.unique(ids):
            ss = np.flatnonzero(ids == n)
            num = den = 0.0
            for s in ss:
                num += b.prob[s] * f[s]
                den += b.prob[s]
            out.append((b.node_names[n], num / den))
        return out

    def tree_nonants(self):
        """z of the last solve per non-leaf node, in ``node_names`` order: [(node name, values)]."""
        b = self.batch
        z = self.engine.ef_z.cpu().numpy()
        if not self._tree:
            return [("ROOT", z)]
        nlens, depth, _, _ = self._tree_layout()
        zoff = np.concatenate([[0], np.cumsum(nlens[depth])])
        return [(b.node_names[n], z[zoff[n]:zoff[n + 1]]) for n in range(len(depth))]

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
        return {nm: float(v) for nm, v in zip(self._nonant_names(), self.root_nonants())}       # (ROOT's only)

    # ef.py:131-139 (sputils.ef_nonants): every non-leaf node's, in node_names order
    def nonants(self):
        if self.status is None:
            raise ValueError("the extensive form has not been solved")
        names = self._nonant_names()
        P = np.concatenate([[0], np.cumsum(self.batch.nlens())])
        dep = {nd: d for d in range(self.batch.depth) for nd in np.asarray(self.batch.node_names, dtype=object)[
            np.unique(self.batch.node_of[:, d])]}
        for nd, vals in self.tree_nonants():
            for nm, v in zip(names[P[dep[nd]]:P[dep[nd] + 1]], vals):
                yield nd, nm, float(v)

    # ef.py:141-147 (sputils.ef_nonants_csv)
    def nonants_to_csv(self, filename):
        with open(filename, "w") as f:
            f.write("Node, EF_VarName, Value\n")
            for nd, nm, v in self.nonants():
                f.write(f"{nd}, {nm}, {v}\n")

    # ef.py:149-157
    def scenarios(self):
        yield from self.local_scenarios.items()
