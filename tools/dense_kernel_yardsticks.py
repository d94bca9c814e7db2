"""Writes profiles/dense_kernel_yardsticks.json: the figures behind checks 6 and 7 of tests/test_gpu_dense_kernels.py.

On the CPU, for the random inputs of tests/dense_kernel_inputs.py (x ~ 1.5 N(0, 1), w ~ N(0, 1) / sqrt(K), M = N = 256): the error of a
float32 sequential sum (the yardstick; the test's bound is twice it), of the emulated six-term product and of every five-term
product, all against float64 in units of sum |x||w|.  With a GPU, the kernels' own errors on the same inputs and at the
k_dense3_sk shape, and the mean signed relative error on same-sign data (forward, weight gradient, torch.matmul in float32).

    python tools/dense_kernel_yardsticks.py [--out FILE]     # the CPU numbers are deterministic for a given torch build
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dense_kernel_inputs as I  # noqa: E402


def main():
    out = os.path.join(ROOT, "profiles", "dense_kernel_yardsticks.json")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    doc = dict(units="max |y - x w^T| / sum_k |x||w| against float64", rounding=[], same_sign=None)
    if torch.cuda.is_available():
        import test_gpu_dense_kernels as T
        from adkf_ift_amd import _lib
        lib, dev = _lib.load(), torch.device("cuda:0")
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        doc["device"] = dict(name=torch.cuda.get_device_properties(dev).name, compute_units=cus)
        for K, M in ((32, 256), (256, 256), (256, 128 * cus + 77)):
            doc["rounding"].append(T.rounding_figures(lib, dev, K, M))
        doc["same_sign"] = dict(shape=list(I.SAME_SIGN), what="mean of (got - ref) / ref, operands uniform in [1, 2)", **T.same_sign_figures(lib, dev))
    else:
        for K in I.ROUNDING_K:
            c = I.normal_case(256, 256, K)
            five = I.five_term_errors(c["x"], c["w"])
            bound, yard = I.rounding_bound(c["x"], c["w"], min(v for k, v in five.items() if k is not None))
            doc["rounding"].append(dict(M=256, N=256, K=K, kernel=None, f32_sequential=yard, bound=bound, six_term_emulation=five[None],
                                        five_term_emulation={"%d%d" % k: v for k, v in five.items() if k is not None}))
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
