"""Generate tests/golden/fwph_*.json: FWPH trajectories of the numpy restatement tests/fwph_ref.py
(HiGHS LPs) on the farmer cases admitted as parity fixtures (tests/test_fwph.py asserts the
admission: the same trajectory with interior-point LPs to 1e-6, no Gamma in [0.5 tau, 1.5 tau]).

Run:  python tests/golden/make_golden_fwph.py
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

import fwph_ref as R  # noqa: E402


def record(cfg):
    t = R.run_trajectory(cfg)
    return {"config": {k: v for k, v in cfg.items()}, "trivial": t["trivial"],
            "iters": [{"bound": o["bound"], "diff": o["diff"], "xbar": o["xbar"].tolist(), "W": o["W"].tolist(),
                       "ncols": o["ncols"].tolist(), "nit": o["nit"].tolist()} for o in t["iters"]]}


def main():
    for name, cfg in R.TRAJECTORIES.items():
        path = os.path.join(HERE, f"fwph_{name}.json")
        with open(path, "w") as f:
            json.dump(record(cfg), f)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
