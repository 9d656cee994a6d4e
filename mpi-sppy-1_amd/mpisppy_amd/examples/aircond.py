"""Multistage aircond inventory model (mirrors mpisppy/tests/examples/aircond.py).

``scenario_creator`` restates aircond.py:88-330 for ``start_ups=False`` (the LP/QP
case; start-up binaries are outside this engine's hot path) as a LinearModel;
``batch_creator`` builds a rank's scenarios at once.  For multistage sampling
(confidence_intervals/sample_tree.py): ``sample_tree_scen_creator`` (aircond.py:332-374) and its
vectorised form ``sample_forest_batch_creator``, which builds all subtrees of one stage at once.
"""
import numpy as np

from ..model import LinearModel, INF
from ..sputils import extract_num, node_idx, create_nodenames_from_branching_factors
from ..scenario_tree import ScenarioNode
from ..batch import batch_from_models, ScenarioBatch

# Interior-point constants measured for this model (PH option "ipm_tuning" ->
# phgpu_set_ipm_tuning): a lower centring floor and a deeper warm-start push.  Config 4
# (65,536 scenarios, one lane per scenario): 2,759-2,791 PH it/s against 2,556-2,576 with the
# library's 0.01 / 0.1, max / mean IPM iterations per PH solve 18 / 7.7 against 20 / 7.9
# (profiles/r05/x); farmer gains nothing from them (8,906-8,919 against 8,971-8,975).
IPM_TUNING = {"IPM_SIG_MIN": 0.003, "IPM_WARM_T": 0.3}

# aircond.py:19-35 ("Do not edit these defaults!")
PARMS = {
    "mu_dev": 0.0, "sigma_dev": 40.0, "start_ups": False, "StartUpCost": 300.0,
    "start_seed": 1134, "min_d": 0.0, "max_d": 400.0, "starting_d": 200.0,
    "BeginInventory": 200.0, "InventoryCost": 0.5, "LastInventoryCost": -0.8,
    "Capacity": 200.0, "RegularProdCost": 1.0, "OvertimeProdCost": 3.0,
    "NegInventoryCost": 5.0, "QuadShortCoeff": 0.0,
}


def _kw(kwargs, p):
    return kwargs.get(p, PARMS[p])


def demands_creator(sname, sample_branching_factors, root_name="ROOT", **kwargs):
    """aircond.py:37-67: demand path from per-node seeds start_seed + node_idx."""
    if "start_seed" not in kwargs:
        raise RuntimeError(f"start_seed not in kwargs={kwargs}")
    start_seed = kwargs["start_seed"]
    max_d = kwargs.get("max_d", 400)
    min_d = kwargs.get("min_d", 0)
    mu_dev = kwargs.get("mu_dev", None)
    sigma_dev = kwargs.get("sigma_dev", None)
    scennum = extract_num(sname)
    prod = int(np.prod(sample_branching_factors))
    s = int(scennum % prod)
    d = kwargs.get("starting_d", 200)
    demands = [d]
    nodenames = [root_name]
    for bf in sample_branching_factors:
        assert prod % bf == 0
        prod = prod // bf
        nodenames.append(str(s // prod))
        s = s % prod
    stagelist = [int(x) for x in nodenames[1:]]
    rs = np.random.RandomState()
    for t in range(1, len(nodenames)):
        rs.seed(start_seed + node_idx(stagelist[:t], sample_branching_factors))
        d = min(max_d, max(min_d, d + rs.normal(mu_dev, sigma_dev)))
        demands.append(d)
    return demands, nodenames


def scenario_creator(sname, **kwargs):
    """aircond.py:304-330 (+ the stage models 88-182 and material balance 212-222)."""
    if "start_seed" not in kwargs:
        raise RuntimeError("start_seed not in kwargs")
    if "branching_factors" not in kwargs:
        raise RuntimeError("scenario_creator for aircond needs branching_factors in kwargs")
    if _kw(kwargs, "start_ups"):
        raise NotImplementedError("start_ups (binaries) is outside the LP/QP hot path")
    # parameters the caller leaves out take the module defaults (what kw_creator does
    # in the reference, aircond.py:19-35 / 441-460)
    kwargs = {**{k: v for k, v in PARMS.items() if k != "start_seed"}, **kwargs}
    bfs = list(kwargs["branching_factors"])
    demands, nodenames = demands_creator(sname, bfs, **kwargs)
    mdl, st = _model_from_demands(sname, demands, kwargs)
    mdl._mpisppy_node_list = _nodes_for_scen(mdl, st, nodenames, bfs)
    mdl._mpisppy_probability = 1 / np.prod(bfs)
    return mdl


def _model_from_demands(sname, demands, kwargs):
    """aircond_model_creator (aircond.py:184-249): the stage models and the material balance."""
    T = len(demands)
    cap = _kw(kwargs, "Capacity")
    bigM = cap * 25
    qsc = _kw(kwargs, "QuadShortCoeff")
    mdl = LinearModel(sname)
    st = {}
    for t in range(1, T + 1):
        last = t == T
        Reg = mdl.var(f"stage_model_{t}.RegularProd", 0.0, bigM, _kw(kwargs, "RegularProdCost"))
        Over = mdl.var(f"stage_model_{t}.OvertimeProd", 0.0, bigM, _kw(kwargs, "OvertimeProdCost"))
        Inv = mdl.var(f"stage_model_{t}.Inventory", -bigM, bigM, 0.0)
        neg = mdl.var(f"stage_model_{t}.negInventory", 0.0, bigM, _kw(kwargs, "NegInventoryCost"),
                      2.0 * qsc if (qsc > 0 and not last) else 0.0)
        pos = mdl.var(f"stage_model_{t}.posInventory", 0.0, bigM,
                      _kw(kwargs, "LastInventoryCost") if last else _kw(kwargs, "InventoryCost"))
        mdl.row([(Reg, 1.0)], -INF, cap, f"stage_model_{t}.MaximumCapacity")
        mdl.row([(Inv, 1.0), (pos, -1.0), (neg, 1.0)], 0.0, 0.0, f"stage_model_{t}.doleInventory")
        st[t] = (Reg, Over, Inv, neg, pos)
    for t in range(1, T + 1):
        Reg, Over, Inv, _, _ = st[t]
        terms = [(Reg, 1.0), (Over, 1.0), (Inv, -1.0)]
        rhs = demands[t - 1]
        if t == 1:
            rhs -= _kw(kwargs, "BeginInventory")
        else:
            terms.append((st[t - 1][2], 1.0))
        mdl.row(terms, rhs, rhs, f"MaterialBalance[{t}]")
    mdl.demands = demands
    mdl.stage_vars = st
    return mdl, st


def _nodes_for_scen(mdl, st, nodenames, bfs, starting_stage=1):
    """MakeNodesforScen, aircond.py:251-302: up to ``starting_stage`` one node per stage (ROOT,
    ROOT_0, ROOT_0_0, ...), below it the sample tree's."""
    T = len(st)
    nodes = [ScenarioNode("ROOT", 1.0, 1, None, [st[1][0], st[1][1]], mdl)]
    ndn = "ROOT"
    for t in range(2, T):
        parent = ndn
        if t <= starting_stage:
            ndn, cp = parent + "_0", 1.0
        else:
            ndn, cp = parent + "_" + nodenames[t - starting_stage], 1.0 / bfs[t - starting_stage - 1]
        nodes.append(ScenarioNode(ndn, cp, t, None, [st[t][0], st[t][1]], mdl, parent_name=parent))
    return nodes


def sample_tree_scen_creator(sname, stage, sample_branching_factors, seed, given_scenario=None,
                             **scenario_creator_kwargs):
    """aircond.py:332-374: a scenario of the sample subtree that starts at ``stage``: the demands of
    stages 1..stage are ``given_scenario``'s, the later ones are sampled with ``seed`` over
    ``sample_branching_factors`` (as in the reference, that walk restarts from ``starting_d``, not
    from the demand of the stage it starts at)."""
    kw = {**{k: v for k, v in PARMS.items() if k != "start_seed"}, **scenario_creator_kwargs}
    if _kw(kw, "start_ups"):
        raise NotImplementedError("start_ups (binaries) is outside the LP/QP hot path")
    if given_scenario is None:
        if stage != 1:
            raise RuntimeError("sample_tree_scen_creator for aircond needs a 'given_scenario' argument if the starting "
                               "stage is greater than 1")
        past = [_kw(kw, "starting_d")]
    else:
        past = list(given_scenario.demands[:stage])
    bfs = list(sample_branching_factors)
    future, nodenames = demands_creator(sname, bfs, root_name="ROOT" + "_0" * (stage - 1), **{**kw, "start_seed": seed})
    mdl, st = _model_from_demands(sname, past + future[1:], kw)
    mdl._mpisppy_probability = 1 / np.prod(bfs)
    mdl._mpisppy_node_list = _nodes_for_scen(mdl, st, nodenames, bfs, starting_stage=stage)
    return mdl


def kw_creator(cfg, optionsin=None):
    """aircond.py:421-457: the creators' keyword arguments from ``optionsin`` (which wins) and
    ``cfg`` (a mapping or an object with the option names as attributes), else the defaults."""
    options = optionsin if optionsin is not None else {}
    if "kwargs" in options:
        return options["kwargs"]

    def look(name):
        v = options.get(name)
        if v is None:
            v = cfg.get(name) if hasattr(cfg, "get") else getattr(cfg, name, None)
        return v
    kwargs = {"branching_factors": look("branching_factors")}
    for name, default in PARMS.items():
        v = look(name)
        kwargs[name] = default if v is None else v
    return kwargs


def scenario_denouement(rank, scenario_name, scenario):
    pass


def scenario_names_creator(num_scens, start=None):
    if start is None:
        start = 0
    return [f"scen{i}" for i in range(start, start + num_scens)]


def general_rho_setter(scenario_instance, rho_scale_factor=1.0):
    """aircond.py:69-79: rho = production cost * factor on each stage's nonants."""
    out = []
    for nd in scenario_instance._mpisppy_node_list:
        reg, over = nd.nonant_vardata_list
        out.append((id(reg), scenario_instance.cost[reg.index] * rho_scale_factor))
        out.append((id(over), scenario_instance.cost[over.index] * rho_scale_factor))
    return out


def dual_rho_setter(scenario_instance):
    return general_rho_setter(scenario_instance, rho_scale_factor=0.0001)


def primal_rho_setter(scenario_instance):
    return general_rho_setter(scenario_instance, rho_scale_factor=0.01)


def batch_creator(scenario_names, **kwargs):
    """Vectorised ScenarioBatch for ``scenario_names``: the pattern comes from one
    template scenario; per scenario only the material-balance right-hand sides
    (demands) and tree node ids change."""
    names = list(scenario_names)
    kwargs = {**{k: v for k, v in PARMS.items() if k != "start_seed"}, **kwargs}
    bfs = list(kwargs["branching_factors"])
    tmpl = scenario_creator(names[0], **kwargs)
    all_nodes = create_nodenames_from_branching_factors(bfs)
    nonleaf = [nd for nd in all_nodes if nd.count("_") < len(bfs)]
    tb = batch_from_models([names[0]], [tmpl], node_names=nonleaf)
    S = len(names)
    T = len(bfs) + 1
    # material balance rows are the last T kept rows (singleton capacity rows folded)
    mb = np.arange(tb.m - T, tb.m)
    rl = np.repeat(tb.rl, S, axis=0)
    ru = np.repeat(tb.ru, S, axis=0)
    node_of = np.empty((S, T - 1), dtype=np.int32)
    nid = {nd: i for i, nd in enumerate(nonleaf)}
    begin = _kw(kwargs, "BeginInventory")
    for s, nm in enumerate(names):
        dem, nodenames = demands_creator(nm, bfs, **kwargs)
        rhs = np.array(dem, dtype=np.float64)
        rhs[0] -= begin
        rl[s, mb] = rhs
        ru[s, mb] = rhs
        ndn = "ROOT"
        node_of[s, 0] = 0
        for t in range(2, T):
            ndn = ndn + "_" + nodenames[t - 1]
            node_of[s, t - 1] = nid[ndn]
    rep = lambda a: np.repeat(a, S, axis=0)  # noqa: E731
    prob = np.full(S, 1.0 / np.prod(bfs))
    uncond = np.array([1.0] + [1.0 / np.prod(bfs[:d]) for d in range(1, T - 1)])
    prob_coeff = prob[:, None] / uncond[None, :]
    return ScenarioBatch(names, tb.row_ptr, tb.col_idx, rep(tb.A_val), rep(tb.c), rep(tb.lb),
                         rep(tb.ub), rl, ru, rep(tb.q), rep(tb.obj_const), tb.nonant_col,
                         tb.nonant_depth, tb.nonant_off, node_of, nonleaf, prob, prob_coeff,
                         tb.sense, tb.var_names, tb.nonant_names)


def sample_forest_batch_creator(tree_demands, stage, seeds, **kwargs):
    """All sample subtrees that start at ``stage`` (>= 2) as ONE ScenarioBatch with the shape of the
    sample tree itself (confidence_intervals/sample_tree.py), whose
    ``branching_factors`` are among the keyword arguments.  ``tree_demands``
    [prod(bf), T]: the sample tree's demands per scenario, in tree order; ``seeds``: the seed of each
    node of that stage, in node order.  Scenario s of the result keeps the sample tree's demands of
    stages 1..stage (its node's) and takes those of the later stages from
    ``sample_tree_scen_creator`` with its node's seed; within a node the scenarios are in the
    subtree's tree order (scenario number modulo the subtree's size, as ``demands_creator`` places
    them).  The rows, columns, bounds and costs equal ``batch_from_models`` over those models array
    for array; nodes and probabilities are the sample tree's (a subtree's own probabilities are these
    over its node's)."""
    kw = {**{k: v for k, v in PARMS.items() if k != "start_seed"}, **kwargs}
    bfs = list(kw["branching_factors"])         # (the sample tree's, as batch_creator takes them)
    t = int(stage)
    T = len(bfs) + 1
    if not 2 <= t < T:
        raise RuntimeError(f"sample_forest_batch_creator: stage {t} of a {T}-stage tree has no subtrees to sample")
    dem = np.array(tree_demands, dtype=np.float64)
    S, sub = int(np.prod(bfs)), int(np.prod(bfs[t - 1:]))
    if dem.shape != (S, T) or len(seeds) != S // sub:
        raise RuntimeError(f"sample_forest_batch_creator: demands {dem.shape} for {S} scenarios of {T} stages, "
                           f"{len(seeds)} seeds for {S // sub} nodes of stage {t}")
    names = []
    for j, seed in enumerate(seeds):
        for pos in range(sub):
            nm = f"scen{int(seed) + (pos - int(seed)) % sub}"
            fut, _ = demands_creator(nm, bfs[t - 1:], root_name="ROOT" + "_0" * (t - 1), **{**kw, "start_seed": int(seed)})
            dem[j * sub + pos, :t] = dem[j * sub, :t]
            dem[j * sub + pos, t:] = fut[1:]
            names.append(nm)
    tmpl, _ = _model_from_demands(names[0], list(dem[0]), kw)
    tmpl._mpisppy_node_list = _nodes_for_scen(tmpl, tmpl.stage_vars, ["ROOT"] + ["0"] * len(bfs), bfs)
    tmpl._mpisppy_probability = 1.0 / S
    nonleaf = [nd for nd in create_nodenames_from_branching_factors(bfs) if nd.count("_") < len(bfs)]
    tb = batch_from_models([names[0]], [tmpl], node_names=nonleaf)
    mb = np.arange(tb.m - T, tb.m)                  # the material balance rows, as in batch_creator
    rl, ru = np.repeat(tb.rl, S, axis=0), np.repeat(tb.ru, S, axis=0)
    rhs = dem.copy()
    rhs[:, 0] -= _kw(kw, "BeginInventory")
    rl[:, mb] = rhs
    ru[:, mb] = rhs
    first = np.concatenate([[0], np.cumsum([int(np.prod(bfs[:d])) for d in range(T - 2)])])   # first node id per depth
    node_of = np.array([[first[d] + s // int(np.prod(bfs[d:])) for d in range(T - 1)] for s in range(S)], dtype=np.int32)
    rep = lambda a: np.repeat(a, S, axis=0)  # noqa: E731
    prob = np.full(S, 1.0 / S)
    uncond = np.array([1.0] + [1.0 / np.prod(bfs[:d]) for d in range(1, T - 1)])
    b = ScenarioBatch(names, tb.row_ptr, tb.col_idx, rep(tb.A_val), rep(tb.c), rep(tb.lb), rep(tb.ub), rl, ru, rep(tb.q),
                      rep(tb.obj_const), tb.nonant_col, tb.nonant_depth, tb.nonant_off, node_of, nonleaf, prob,
                      prob[:, None] / uncond[None, :], tb.sense, tb.var_names, tb.nonant_names)
    b.demands = dem
    return b
