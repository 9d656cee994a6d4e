"""The confidence-interval package in numpy / HiGHS: a restatement of the formulas of DESIGN.md
3.20 (after mpisppy/confidence_intervals/ciutils.py:285-313 and 400-424, mmw_ci.py:168-176,
zhat4xhat.py:113-116 and seqsampling.py:265-328) over oracle.models scenarios, the reference of
tests/test_confidence_intervals.py and tests/test_gpu_confidence_intervals.py.  Written from
reading those lines; it holds none of their text.

x* of a sample problem is the extensive form's optimum by HiGHS (lshaped_ref.ef_optimum), the
per-scenario objectives are LPs with the nonants fixed (lshaped_ref.lp_highs), and every sum is
math.fsum.  Minimisation problems.
"""
import math

import numpy as np
from scipy import stats

import lshaped_ref as LR

FARMER_XHAT = (80.0, 250.0, 170.0)      # the EF optimum of scen0..2, cm = 1, in nonant order
START = 3                               # the first scenario after the candidate's sample
CASES = {"5x7": (5, 7), "4x16": (4, 16)}            # (num_batches, batch_size) from START
# The sequential procedures: the reference's developer-test options (seqsampling.py:536-562) with
# h, h' (BM) and eps, c0 (BPL) scaled so that farmer, whose G is a few hundred and s about a
# thousand, stops at T = 2; the deciding comparisons are then 309 > 267 and 63 < 81 (BM), 926 > 700
# and 354 < 700 (BPL), far from what the x* of two solvers can move
SEQ_BM = {"BM_h": 1.0, "BM_hprime": 0.2, "BM_eps": 0.5, "BM_eps_prime": 0.4, "BM_p": 0.2, "BM_q": 1.2}
SEQ_BPL = {"BPL_eps": 700.0, "BPL_c0": 10, "ArRP": 2}


def farmer_scens(start, count, cm=1):
    from oracle.models import farmer_scenario
    return [farmer_scenario(f"scen{i}", cm, num_scens=count) for i in range(start, start + count)]


def fixed_objectives(scens, x):
    """Objective of every scenario with its nonants fixed at x."""
    idx = np.array(scens[0].nonant_indices())
    out = []
    for sc in scens:
        A, rl, ru, lb, ub, c, _ = sc.arrays()
        lb, ub = lb.copy(), ub.copy()
        lb[idx] = x
        ub[idx] = x
        out.append(LR.lp_highs(A, rl, ru, lb, ub, c)[1])
    return np.array(out)


def correcting_numeric(G, objfct, relative_error=True, threshold=1e-4):
    """Minimisation: a small negative G is rounding and becomes 0, a large one is returned."""
    crit = threshold * abs(objfct) if relative_error else threshold
    if G <= -crit:
        return G
    return max(0.0, G)


def estimators_from_objectives(f_hat, f_star, prob):
    """G, s, ẑ(x̂), ẑ(x*) of one sample from its per-scenario objectives and probabilities (any
    common scale)."""
    p = [float(v) for v in prob]
    g = [float(a) - float(b) for a, b in zip(f_hat, f_star)]
    sp = math.fsum(p)
    G = math.fsum(pi * gi for pi, gi in zip(p, g)) / sp
    ssq = math.fsum(pi * gi * gi for pi, gi in zip(p, g)) / sp
    psq = math.fsum(pi * pi for pi in p) / (sp * sp)
    zhat = math.fsum(pi * fi for pi, fi in zip(p, f_hat)) / sp
    zstar = math.fsum(pi * fi for pi, fi in zip(p, f_star)) / sp
    s = math.sqrt(max((ssq - G * G) / (1.0 - psq), 0.0))
    G = correcting_numeric(G, zhat, relative_error=abs(zstar) > 1)
    return {"G": G, "s": s, "zhat": zhat, "zstar": zstar}


def gap_estimators(scens, xhat, ArRP=1):
    """{"G", "s", "zhat", "zstar", "xstar"} of the sample ``scens`` at the candidate ``xhat``;
    ArRP > 1 pools the estimators of ArRP consecutive sub-samples."""
    n = len(scens)
    if ArRP > 1:
        assert n % ArRP == 0
        sub = n // ArRP
        parts = [gap_estimators(scens[k * sub:(k + 1) * sub], xhat) for k in range(ArRP)]
        return {"G": float(np.mean([p["G"] for p in parts])),
                "s": float(np.linalg.norm([p["s"] for p in parts]) / np.sqrt(sub)),
                "zhat": float(np.mean([p["zhat"] for p in parts])),
                "zstar": float(np.mean([p["zstar"] for p in parts])), "xstar": [p["xstar"] for p in parts]}
    _, xstar = LR.ef_optimum(scens)
    r = estimators_from_objectives(fixed_objectives(scens, np.asarray(xhat, float)), fixed_objectives(scens, xstar),
                                   [sc.prob for sc in scens])
    r["xstar"] = xstar
    return r


def mmw(Glist, confidence_level=0.95):
    """The MMW result from the batches' G."""
    G = np.asarray(Glist, float)
    std, Gbar = float(np.std(G)), float(np.mean(G))
    t = float(stats.t.ppf(confidence_level, len(G) - 1))
    return {"gap_inner_bound": Gbar + t * std / math.sqrt(len(G)), "gap_outer_bound": 0, "Gbar": Gbar, "std": std,
            "Glist": G}


def mmw_farmer(xhat, num_batches, batch_size, start, cm=1, confidence_level=0.95):
    ests = [gap_estimators(farmer_scens(start + b * batch_size, batch_size, cm), xhat) for b in range(num_batches)]
    r = mmw([e["G"] for e in ests], confidence_level)
    r["s"] = np.array([e["s"] for e in ests])
    r["zhat"] = np.array([e["zhat"] for e in ests])
    return r


def zhat_halfwidth(zhats, confidence_level=0.95):
    z = np.asarray(zhats, float)
    t = float(stats.t.ppf(confidence_level, len(z) - 1))
    return float(np.mean(z)), t * float(np.std(z)) / math.sqrt(len(z))


# ------------------------------------------------------------------ sequential sampling
def bm_constant(p, q, confidence_level, r=2):
    j = np.arange(1, 1000)
    tot = np.sum(np.power(j, -p * np.log(j))) if q is None else np.sum(np.exp(-p * np.power(j, 2 * q / r)))
    return max(1, 2 * np.log(tot / (np.sqrt(2 * np.pi) * (1 - confidence_level))))


def bm_sampsize(k, o, c, r=2):
    growth = 2 * o["BM_p"] * np.log(k) ** 2 if o.get("BM_q") is None else 2 * o["BM_p"] * np.power(k, 2 * o["BM_q"] / r)
    return int(np.ceil((c + growth) / (o["BM_h"] - o["BM_hprime"]) ** 2))


def bpl_sampsize(k, o):
    return int(np.ceil(o.get("BPL_c0", 50) + o.get("BPL_c1", 2) * (k - 1)))


def seqsampling_farmer(o, criterion, cm=1, maxit=200):
    """The sequential procedure on farmer with every sample new (kf_Gs = kf_xhat = 1), the
    candidate of iteration k the EF optimum of its m_k scenarios.  ``o``: the options.
    {"T", "nk", "CI", "history" [(n_k, G_k, s_k)], "xhat"}."""
    conf = o.get("confidence_level", 0.95)
    ArRP, mult = o.get("ArRP", 1), o.get("sample_size_ratio", 1)
    c = bm_constant(o["BM_p"], o.get("BM_q"), conf) if criterion == "BM" else None
    size = (lambda k: bm_sampsize(k, o, c)) if criterion == "BM" else (lambda k: bpl_sampsize(k, o))

    def go_on(G, s, nk):
        if criterion == "BM":
            return G > o["BM_hprime"] * s + o["BM_eps_prime"]
        t = float(stats.t.ppf(conf, nk - 1))
        return G + t * s / math.sqrt(nk) + 1 / math.sqrt(nk) > o["BPL_eps"]

    count, k, hist = 0, 0, []
    while True:
        k += 1
        lb = size(k)
        mk = int(np.floor(mult * lb))
        _, xhat = LR.ef_optimum(farmer_scens(count, mk, cm))
        count += mk
        nk = ArRP * int(np.ceil(lb / ArRP))
        e = gap_estimators(farmer_scens(count, nk, cm), xhat, ArRP)
        # (each sub-sample's scenarios carry the probability 1 / n_k; the estimators do not
        # depend on the common scale)
        count += nk
        hist.append((nk, e["G"], e["s"]))
        if not (go_on(e["G"], e["s"], nk) and k < maxit):
            break
    if k == maxit:
        raise RuntimeError("no acceptable solution")
    up = o["BM_h"] * e["s"] + o["BM_eps"] if criterion == "BM" else o["BPL_eps"]
    return {"T": k, "nk": nk, "CI": [0, float(up)], "history": hist, "xhat": xhat}


def golden_record():
    """What tests/golden/mmw_farmer.json holds: the MMW results of CASES at FARMER_XHAT, the
    pooled estimator of the first 16-scenario batch and the two sequential runs."""
    rec = {"xhat": list(FARMER_XHAT), "start": START, "cases": {}}
    for name, (B, n) in CASES.items():
        r = mmw_farmer(FARMER_XHAT, B, n, START)
        rec["cases"][name] = {"num_batches": B, "batch_size": n, "Glist": r["Glist"].tolist(), "s": r["s"].tolist(),
                              "zhat": r["zhat"].tolist(), "Gbar": r["Gbar"], "std": r["std"],
                              "gap_inner_bound": r["gap_inner_bound"]}
    p = gap_estimators(farmer_scens(START, 16), FARMER_XHAT, 2)
    rec["ArRP2_16"] = {"G": p["G"], "s": p["s"]}
    rec["zhat_halfwidth_4x16"] = list(zhat_halfwidth(rec["cases"]["4x16"]["zhat"]))
    for key, o, crit in (("seq_BM", SEQ_BM, "BM"), ("seq_BPL", SEQ_BPL, "BPL")):
        r = seqsampling_farmer(o, crit)
        rec[key] = {"T": r["T"], "nk": r["nk"], "CI": r["CI"], "history": [list(h) for h in r["history"]],
                    "xhat": list(r["xhat"])}
    return rec
