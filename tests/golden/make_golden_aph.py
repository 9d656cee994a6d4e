"""Generate tests/golden/aph_*.json: APH trajectories of the numpy restatement tests/aph_ref.py
(interior-point QPs) on the configurations admitted as parity fixtures (tests/test_aph.py asserts
the admission: the same trajectory with HiGHS QPs to 1e-6 with identical dispatch lists, and at
every dispatch a gap of more than 1e-6 max|phi| between the last key taken and the first left out).

Run:  python tests/golden/make_golden_aph.py
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
warnings.simplefilter("ignore")

import aph_ref as R  # noqa: E402


def record(cfg, qp="ipm"):
    t = R.run_trajectory(cfg, qp)
    return {"config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, "trivial": t["trivial"],
            "eobj": t["eobj"], "conv": t["conv"],
            "iters": [{"tau": o["tau"], "phi": o["phi"], "theta": o["theta"], "conv": o["conv"],
                       "phisum": o["phisum"], "abs_phi_pre": o["abs_phi_pre"], "abs_phi": o["abs_phi"], "W": o["W"].tolist(), "z": o["z"].tolist(),
                       "xbar": o["xbar"].tolist(), "dispatch": o["dispatch"]} for o in t["iters"]]}


def main():
    for name, cfg in R.TRAJECTORIES.items():
        path = os.path.join(HERE, f"aph_{name}.json")
        with open(path, "w") as f:
            json.dump(record(cfg), f)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
