"""Writes profiles/gnn_kernel_yardsticks.json: the float32 yardsticks behind the rule-B literals of tests/test_gpu_gnn_kernels.py.

For every case of tests/gnn_kernel_inputs.py the references of oracle/gnn_kernel_refs.py are evaluated twice on the CPU, in float64
and - the same code, the same float32 inputs - in float32.  E32 is the largest float32 error of an output relative to that output's
largest entry (the per-row outputs of the block in three groups of rows, ``gnn_kernel_inputs.block_row_err``); the literal of an
(operation, output) is 4 x the largest E32 over its cases, rounded up to one significant digit and never below 2^-20
(``gnn_kernel_inputs.literal_for``).  No GPU and no kernel output is involved.

    python tools/gnn_kernel_yardsticks.py          # rewrites the file; the numbers are deterministic for a given torch build
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gnn_kernel_inputs as I  # noqa: E402


def main():
    torch.set_num_threads(1)   # one summation order for the float32 side
    entries = []

    def measure(op, case, shape, ref, seed, **extra):
        r64, r32 = ref(case), ref(case, torch.float32)
        for name in I.RULE_B[op]:
            e = I.block_row_err(case, r32[name], r64[name]) if op == "block" and name in I.BLOCK_PER_ROW else I.rel_err(r32[name], r64[name])
            entries.append(dict(op=op, output=name, shape=list(shape), seed=seed, E32=e, **extra))

    for hid, V, alpha in I.BLOCK_CASES:
        measure("block", I.block_case(hid, V, alpha), (hid, V), I.block_ref, 300, alpha=alpha)
    for scores in I.SCORES:
        for shape in I.POOL_SHAPES:
            measure("pool", I.pool_case(*shape, scores), shape, I.pool_ref, 400, scores=scores)
        for shape in I.HIDDEN_SHAPES:
            measure("hidden", I.hidden_case(*shape, scores), shape, I.hidden_ref, 500, scores=scores)
    literals = {}
    for op, names in I.RULE_B.items():
        literals[op] = {}
        for name in names:
            worst = max(e["E32"] for e in entries if e["op"] == op and e["output"] == name)
            literals[op][name] = dict(E32_max=worst, literal=I.literal_for(worst))
    out = dict(note="float32 CPU evaluation of oracle/gnn_kernel_refs.py against its float64 evaluation on the inputs of "
                    "tests/gnn_kernel_inputs.py; literal = max(4 E32_max rounded up to one significant digit, 2^-20)",
               torch=torch.__version__, literals=literals, entries=entries)
    path = os.path.join(ROOT, "profiles", "gnn_kernel_yardsticks.json")
    with open(path, "w") as f:   # one record per line
        f.write("{\n")
        for k in ("note", "torch"):
            f.write(" %s: %s,\n" % (json.dumps(k), json.dumps(out[k])))
        f.write(' "literals": {\n%s\n },\n' % ",\n".join("  %s: %s" % (json.dumps(op), json.dumps(v)) for op, v in literals.items()))
        f.write(' "entries": [\n%s\n ]\n}\n' % ",\n".join("  " + json.dumps(e) for e in entries))
    for op in literals:
        print(op, {k: "%.1e -> %.0e" % (v["E32_max"], v["literal"]) for k, v in literals[op].items()})


if __name__ == "__main__":
    main()
