"""adkf_jackknife_pool against adkf_predict_pool at the same shape, on one GPU.

The jackknife side: gp_ops.jackknife_pool with lo / hi [T, 1, rows] written, one level, plain and scaled, no selection.
The baseline: gp_ops.predict_pool with mean / var [T, rows] written - the walk the jackknife's tile is built on.
The split: the same jackknife call at a level without a rank (NaN): the walk still forms the row tile C = K A^-1 a second time and
the fold values, and writes the infinities, but counts nothing - so "jackknife - no_rank" is the selection and "no_rank - predict"
the second product with the fold values.
Every side is warmed up, then timed alternately with device events around enough calls for at least half a second of work.

Usage: python tools/bench_jackknife_pool.py [--tasks 256] [--ns 128] [--d 256] [--rows 16384] [--alpha 0.1] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adkf_ift_amd import _lib, gp_ops  # noqa: E402


def timed(fn, n):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=256)
    ap.add_argument("--ns", type=int, default=128)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T, ns, d, rows = a.tasks, a.ns, a.d, a.rows
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1)) + 0.1 * torch.randn(T, ns, device=dev, generator=g)
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi, _ = gp_ops.init_params_batch(b, True, True)   # phi GIVEN (the median heuristic): every call pays the same inner stage
    X = torch.randn(rows, d, device=dev, generator=g) @ W

    def jk(alpha, scaled):
        return lambda: gp_ops.jackknife_pool(b, phi, X, alpha=(alpha,), scaled=scaled, want_loo=False)

    sides = {"predict_pool_mean_var": lambda: gp_ops.predict_pool(b, phi, X, want_mean=True, want_var=True),
             "jackknife_plain": jk(a.alpha, False), "jackknife_scaled": jk(a.alpha, True),
             "no_rank_plain": jk(float("nan"), False), "no_rank_scaled": jk(float("nan"), True)}
    o1, o2 = sides["jackknife_scaled"](), sides["jackknife_scaled"]()
    gp_ops.check_info(o1["info"])
    torch.cuda.synchronize()
    n_calls = {}
    for name, fn in sides.items():          # warm-up, and the number of calls that makes half a second
        fn()
        n_calls[name] = max(1, int(np.ceil(0.5 / timed(fn, 2))))
    ts = {name: [] for name in sides}
    for _ in range(a.reps):
        for name, fn in sides.items():
            ts[name].append(timed(fn, n_calls[name]))
    med = {name: float(np.median(x)) for name, x in ts.items()}
    base = med["predict_pool_mean_var"]
    lib = _lib.load()
    rec = {"shape": f"T={T} ns={ns} d={d} rows={rows} L=1 alpha={a.alpha} matern; lo/hi [T, 1, rows] against predict_pool mean/var [T, rows]",
           "seconds": med, "calls_per_timing": n_calls,
           "plain_over_predict": med["jackknife_plain"] / base, "scaled_over_predict": med["jackknife_scaled"] / base,
           "second_product_and_folds_s": {"plain": med["no_rank_plain"] - base, "scaled": med["no_rank_scaled"] - base},
           "selection_s": {"plain": med["jackknife_plain"] - med["no_rank_plain"], "scaled": med["jackknife_scaled"] - med["no_rank_scaled"]},
           "scratch_bytes": int(lib.adkf_jackknife_pool_scratch_bytes(T, ns, 1, 0)),
           "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()},
           "repeat_is_bit_equal": bool(torch.equal(o1["lo"].view(torch.int32), o2["lo"].view(torch.int32)) and
                                       torch.equal(o1["hi"].view(torch.int32), o2["hi"].view(torch.int32))),
           "mean_width_scaled": float((o1["hi"] - o1["lo"]).mean()),
           "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
