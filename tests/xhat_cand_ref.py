"""Numpy restatement of the xhat candidates that are functions of all scenarios (TEST
INFRASTRUCTURE ONLY): mpisppy/extensions/xhatxbar.py:38-55 (x̄ itself),
mpisppy/extensions/xhatclosest.py:37-65 (the scenario closest to x̄, with both tie rules) and
mpisppy/cylinders/slam_heuristic.py:57-67, 84 (column-wise max / min).

Arrays are [nn, S] like the device layout (nonant-major); ``key[k, s]`` is the index
(node * nlen_max + offset) of nonant k of scenario s in a node-indexed plane.
"""
import functools
import math

import numpy as np


def keys(node_of, nonant_depth, nonant_off, nlen_max):
    """node_of [depth, S] (global node ids) -> key [nn, S]."""
    node_of = np.asarray(node_of).reshape(-1, np.asarray(node_of).shape[-1])
    return np.stack([node_of[int(d)] * nlen_max + int(o) for d, o in zip(nonant_depth, nonant_off)])


def planes(v, key, pcoef, half):
    """The four planes of phgpu_nonant_stats, [4, half], planes 0-1 by math.fsum, and the
    sums of |terms| of planes 0-1 ([2, half]) that scale their tolerance.  Entries no scenario
    reaches: 0 / -inf."""
    v, key, pcoef = np.asarray(v, dtype=np.float64), np.asarray(key), np.asarray(pcoef, dtype=np.float64)
    out = np.zeros((4, half))
    out[2:] = -np.inf
    mag = np.zeros((2, half))
    for i in np.unique(key):
        m = key == i
        a, b = pcoef[m] * v[m], pcoef[m] * v[m] * v[m]
        out[0, i], out[1, i] = math.fsum(a), math.fsum(b)
        mag[0, i], mag[1, i] = math.fsum(np.abs(a)), math.fsum(np.abs(b))
        out[2, i], out[3, i] = np.max(-v[m]), np.max(v[m])
    return out, mag


def xbar_candidate(pl):
    """xhatxbar.py:49-51: every nonant at its node's x̄."""
    return pl[0]


def slam_candidate(pl, which):
    """slam_heuristic.py:65 + 84 with np.amax / np.amin."""
    return pl[3] if which == "max" else -pl[2]


def distances(v, xbar, xsqbar):
    """xhatclosest.py:37-45 for a two-stage tree: dist[s], loops as the reference's."""
    v = np.asarray(v, dtype=np.float64)
    nn, S = v.shape
    out = np.zeros(S)
    for s in range(S):
        dist = 0
        for k in range(nn):
            diff = v[k, s] - xbar[k]
            variance = xsqbar[k] - xbar[k] * xbar[k]
            if variance > 0:
                stdev = np.sqrt(variance)
                dist += min(3, abs(diff) / stdev)
        out[s] = dist
    return out


def local_winner(dist):
    """xhatclosest.py:46-51: the strict < scan keeps the first (lowest) index of a tie."""
    best, win = None, None
    for s, d in enumerate(dist):
        if win is None or d < best:
            best, win = d, s
    return float(best), win


def rank_winner(local_mins):
    """xhatclosest.py:53-65: MIN of the distances, then MAX of rank-or--1 -- the highest
    rank among those attaining the minimum."""
    g = min(local_mins)
    return max(r if not (g < d) else -1 for r, d in enumerate(local_mins))


# ------------------------------------------------------------------ farmer 30 with the oracle
FARMER_S = 30
FARMER_ITERS = (1, 2, 3, 5)


def farmer_scens(S=FARMER_S):
    from oracle.models import farmer_scenario
    names = [f"scen{i}" for i in range(S)]
    scens = [farmer_scenario(n, 1, num_scens=S) for n in names]
    for s in scens:
        if s.prob is None:
            s.prob = 1.0 / S
    return names, scens


@functools.lru_cache(maxsize=None)
def farmer_trajectory():
    """OraclePH(solver="farmer") on farmer 30, rho 1: per PH iteration in FARMER_ITERS the hub's
    nonants after that iteration's solve ([nn, S]), their planes, the three candidates'
    xhat_objective, the distances and the closest scenario with its objective.  Computed once
    per session, read-only."""
    from oracle.models import farmer_yields
    from oracle.ph import OraclePH
    from oracle.wheel import xhat_objective
    names, scens = farmer_scens()
    crops = sorted(farmer_yields("scen0", 1)[0])
    o = OraclePH(scens, 1.0, solver="farmer", farmer_info=(crops, [farmer_yields(n, 1)[1] for n in names], 1))
    o.iter0()
    o.iterk_loop(max(FARMER_ITERS), -1.0)
    S, nn = FARMER_S, o.nn
    key = np.tile(np.arange(nn)[:, None], (1, S))
    pcoef = np.tile(np.array([s.prob for s in scens])[None, :], (nn, 1))
    out = {}
    for it in FARMER_ITERS:
        v = o.history[it - 1]["x"].T.copy()
        pl, mag = planes(v, key, pcoef, nn)
        dist = distances(v, pl[0], pl[1])
        dmin, win = local_winner(dist)
        rec = {"v": v, "planes": pl, "mag": mag, "dist": dist, "winner": win, "dmin": dmin,
               "xbar_obj": xhat_objective(scens, {"ROOT": xbar_candidate(pl)}),
               "slammin_obj": xhat_objective(scens, {"ROOT": slam_candidate(pl, "min")}),
               "slammax_obj": xhat_objective(scens, {"ROOT": slam_candidate(pl, "max")}),
               "closest_obj": xhat_objective(scens, {"ROOT": v[:, win]})}
        out[it] = rec
    # XhatClosest.post_everything after 5 PH iterations (xhatclosest.py:105-112): the current
    # nonants (the last solve's) against the x̄ / x̄² PH holds, which are those of the solve before
    v = o.x.T.copy()
    dist = distances(v, o.node_xbar["ROOT"], o.node_xsqbar["ROOT"])
    dmin, win = local_winner(dist)
    out["post"] = {"v": v, "xbar": o.node_xbar["ROOT"].copy(), "xsqbar": o.node_xsqbar["ROOT"].copy(),
                   "dist": dist, "winner": win, "dmin": dmin,
                   "closest_obj": xhat_objective(scens, {"ROOT": v[:, win]})}
    return out
