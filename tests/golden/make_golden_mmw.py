"""Generate tests/golden/mmw_farmer.json: the Mak-Morton-Wood estimators, the zhat4xhat half-width
and the sequential-sampling runs of the numpy / HiGHS restatement tests/ci_ref.py on farmer
(cm = 1) at the candidate (80, 250, 170).  tests/test_confidence_intervals.py recomputes it; the
GPU tests read it.

Run:  python tests/golden/make_golden_mmw.py
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

import ci_ref as R  # noqa: E402


def main():
    path = os.path.join(HERE, "mmw_farmer.json")
    with open(path, "w") as f:
        json.dump(R.golden_record(), f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
