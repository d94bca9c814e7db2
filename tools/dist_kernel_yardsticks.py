"""Writes profiles/dist_kernel_yardsticks.json: the figures behind the random-feature check of tests/test_gpu_dist_median.py.

On the CPU, for the random features of tests/gp_stage_inputs.py (standard normal, 130 support and 68 query points, d = 32 and d = 96): the
error of the distance stage evaluated sequentially in float32 (the yardstick; the test's bound is twice it), of the emulated six-term
split and of the variants without x0 y2, x2 y0 or both, all against float64 in units of |x|^2 + |y|^2 + 2 sum |x||y| on the centred rows.
With a GPU, the device's own errors on the same inputs are added under "device".

    python tools/dist_kernel_yardsticks.py [--out FILE]     # the CPU numbers are deterministic for a given torch build
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gp_stage_inputs as I  # noqa: E402


def main():
    out = os.path.join(ROOT, "profiles", "dist_kernel_yardsticks.json")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    doc = dict(units="max |D2 - D2_float64| / (|x|^2 + |y|^2 + 2 sum_k |x||y|), rows centred with the evaluation's own column mean",
               shape=dict(n_s=I.RANDOM_NS, n_q=I.RANDOM_NQ), random=[])
    gpu = torch.cuda.is_available()
    if gpu:
        import test_gpu_dist_median as T
        doc["device_name"] = torch.cuda.get_device_properties(0).name
    for d in I.RANDOM_D:
        yard, emu = I.dist_yardstick(d), I.split_emulation_errors(d)
        name = lambda k: "six_terms" if not k else "without_" + "_".join("x%dy%d" % ij for ij in k)
        row = dict(d=d, f32_sequential=yard, bound={k: 2 * v for k, v in yard.items()}, emulation={name(k): v for k, v in emu.items()})
        if gpu:
            row["device"] = T.random_figures(torch.device("cuda:0"), d)
        doc["random"].append(row)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
