"""Writes profiles/float64_path_check.json: the measured error and bound of every (case, task, entry point, output) comparison of
tests/test_gpu_float64_path.py - the float64 path of ill-conditioned tasks (csrc/refine64.h) against the float64 oracle on the seeded cases
of tests/r64_inputs.py.  Needs the GPU.

    python tools/float64_path_check.py [--out FILE]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import r64_inputs as I  # noqa: E402
import test_gpu_float64_path as T  # noqa: E402


def main():
    out = os.path.join(ROOT, "profiles", "float64_path_check.json")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    dev = torch.device("cuda:0")
    records = T.all_records(dev)
    worst = max(records, key=lambda r: r["error"] / r["bound"])
    doc = dict(units="max |got - ref| / max |ref| per output; bound = 2 (S_k + R slack_k), see tests/r64_inputs.py",
               device_name=torch.cuda.get_device_properties(0).name,
               pivot_ratios={name: [I.pivot_ratios(name, t) for t in range(len(I.CASES[name]["tasks"]))] for name in I.CASES},
               worst=dict(worst, ratio=worst["error"] / worst["bound"]),
               above_bound=[r for r in records if not r["error"] <= r["bound"]], records=records)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(worst=doc["worst"], above_bound=doc["above_bound"], n=len(records)), indent=1))


if __name__ == "__main__":
    main()
