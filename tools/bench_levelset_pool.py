"""adkf_levelset_pool against adkf_believer_pool at the same shape, on one GPU.

The level-set sides: gp_ops.levelset_pool at q picks with no trace and no cls - STRADDLE and PROB, each with and without counts /
hits (without them the call issues no atomic at all).  The baseline: gp_ops.believer_pool at the same q, log EI, no trace - the same
walks, downdate and step with log EI in the place of the level-set row and no reduction of the pool.  Reported: the four ratios
t_levelset / t_believer; there is no target.  Every side is warmed up, then timed alternately with device events around enough calls
for at least half a second of work.

Usage: python tools/bench_levelset_pool.py [--tasks 16] [--ns 128] [--d 256] [--rows 100000] [--q 8] [--reps 5] [--out FILE]"""
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
    ap.add_argument("--tasks", type=int, default=16)
    ap.add_argument("--ns", type=int, default=128)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T, ns, d, rows, q = a.tasks, a.ns, a.d, a.rows, a.q
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1)) + 0.1 * torch.randn(T, ns, device=dev, generator=g)
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi, _ = gp_ops.init_params_batch(b, True, True)   # phi GIVEN (the median heuristic): every call pays the same inner stage
    X = torch.randn(rows, d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    tau = best.clone()
    ls = lambda score, counts: (lambda: gp_ops.levelset_pool(b, phi, X, tau=tau, beta=1.96, q=q, score=score, want_counts=counts))
    sides = {"believer": lambda: gp_ops.believer_pool(b, phi, X, best_f=best, q=q, log_ei=True),
             "straddle": ls("straddle", False), "straddle_counts": ls("straddle", True),
             "prob": ls("prob", False), "prob_counts": ls("prob", True)}
    rec = {"shape": f"T={T} ns={ns} d={d} rows={rows} q={q} matern; no trace, no cls; believer: log EI"}
    o1, o2 = sides["prob_counts"](), sides["prob_counts"]()
    gp_ops.check_info(o1["info"])
    rec["repeat_is_bit_equal"] = bool(torch.equal(o1["sel_idx"], o2["sel_idx"]) and torch.equal(o1["sel_val"].view(torch.int32), o2["sel_val"].view(torch.int32))
                                      and torch.equal(o1["counts"], o2["counts"]) and torch.equal(o1["hits"].view(torch.int32), o2["hits"].view(torch.int32)))
    rec["all_selected"] = bool((o1["sel_idx"] >= 0).all())
    rec["counts_cover_the_pool"] = bool((o1["counts"].sum(-1) == rows).all())
    rec["counts_step0_task0"] = o1["counts"][0, 0].tolist()
    rec["scratch_bytes"] = {"believer": int(_lib.load().adkf_believer_pool_scratch_bytes(T, ns, d, q)),
                            "levelset": int(_lib.load().adkf_levelset_pool_scratch_bytes(T, ns, d, q))}
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
    rec.update({"seconds": med, "calls_per_timing": n_calls,
                "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()}, "all_s": ts})
    rec.update({f"{n}_over_believer": med[n] / med["believer"] for n in sides if n != "believer"})
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
