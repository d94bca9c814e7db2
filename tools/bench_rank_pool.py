"""adkf_rank_pool against the walk alone and against today's workaround, at the family's shape, on one GPU.

The ranking sides: gp_ops.rank_pool, score = mean, at k in {64, 1024, 16384, 65536} with M in {0, 64} named rows.  The baselines:
  (a) gp_ops.predict_pool(topk=64, score="mean") with no per-row output - the walk alone, so rank / (a) is the price of chunking plus
      k_rank_chunk;
  (b) the workaround: gp_ops.predict_pool(want_mean=True) followed by torch.topk(k) on [T, rows] - time and peak device memory.
The batch is fitted once and every call reuses the fit's state (REUSE_DIST | REUSE_INNER).  Every side is warmed up, then single warm
calls are timed alternately with device events; medians.  The share of a ranking call spent in k_rank_chunk comes from the device
times of one profiled call (torch.profiler).  There is no target.

Usage: python tools/bench_rank_pool.py [--tasks 256] [--ns 128] [--d 256] [--rows 100000] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adkf_ift_amd import _lib, gp_ops  # noqa: E402

KS, MS = (64, 1024, 16384, 65536), (0, 64)


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / 1e3


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def chunk_share(fn):
    """(seconds in k_rank_chunk, seconds in every kernel) of one call, from the profiler's device times; None where it has none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_time = lambda e: getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
        rows = [(e.key, dev_time(e)) for e in prof.key_averages()]
        total = sum(t for _, t in rows)
        mine = sum(t for n, t in rows if "k_rank_chunk" in n)
        return (mine / 1e6, total / 1e6) if total > 0 else None
    except Exception as e:   # the profiler is a convenience here
        print(f"[bench_rank_pool] no kernel times: {e}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=256)
    ap.add_argument("--ns", type=int, default=128)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T, ns, d, rows = a.tasks, a.ns, a.d, a.rows
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1)) + 0.1 * torch.randn(T, ns, device=dev, generator=g)
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST | gp_ops.DEFER_REFINE
    phi, _, _, _, info = gp_ops.fit(b, phi0, 60)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.randn(rows, d, device=dev, generator=g) @ W
    refs = torch.randint(0, rows, (T, 64), device=dev, generator=g)
    ks = [k for k in KS if k <= _lib.RANK_K_MAX]
    sides = {"walk_topk64": lambda: gp_ops.predict_pool(b, phi, X, maximize=True, score="mean", want_mean=False, want_var=False, topk=64)}
    for k in ks:
        for M in MS:
            sides[f"rank_k{k}_M{M}"] = (lambda k=k, M=M: gp_ops.rank_pool(b, phi, X, maximize=True, score="mean", topk=k,
                                                                          rank_rows=refs if M else None))
        kk = min(k, rows)
        sides[f"workaround_k{k}"] = (lambda kk=kk: torch.topk(gp_ops.predict_pool(b, phi, X, want_var=False, want_ei=False)["mean"], kk, dim=1))
    rec = {"shape": f"T={T} ns={ns} d={d} rows={rows} matern, score = +mean, REUSE_INNER after a fit; single warm calls, medians of {a.reps}"}
    # the answers agree where they overlap: the first 64 of every ranking call are the walk's selection
    w = sides["walk_topk64"]()
    gp_ops.check_info(w["info"])
    r = sides[f"rank_k{ks[-1]}_M64"]()
    rec["prefix_is_predict_pools"] = bool(torch.equal(r["top_idx"][:, :64], w["top_idx"]) and
                                          torch.equal(r["top_val"][:, :64].contiguous().view(torch.int32), w["top_val"].view(torch.int32)))
    rec["n_ranked_is_rows"] = bool((r["n_ranked"] == rows).all())
    lib = _lib.load()
    rec["scratch_bytes"] = {f"rank_k{k}_M{M}": int(lib.adkf_rank_pool_scratch_bytes(T, k, M, d)) for k in ks for M in MS}
    rec["scratch_bytes"]["walk_topk64"] = int(lib.adkf_predict_pool_scratch_bytes(T, 64))
    rec["peak_device_bytes"] = {n: peak_bytes(fn) for n, fn in sides.items()}
    for fn in sides.values():   # warm
        fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in sides}
    for _ in range(a.reps):
        for n, fn in sides.items():
            ts[n].append(timed(fn))
    med = {n: float(np.median(x)) for n, x in ts.items()}
    rec["seconds"] = med
    rec["spread_max_minus_min_over_median"] = {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()}
    rec["rank_over_walk"] = {n: med[n] / med["walk_topk64"] for n in sides if n.startswith("rank_")}
    rec["rank_over_workaround"] = {f"rank_k{k}_M{M}": med[f"rank_k{k}_M{M}"] / med[f"workaround_k{k}"] for k in ks for M in MS}
    share = {}
    for k in ks:
        for M in MS:
            s = chunk_share(sides[f"rank_k{k}_M{M}"])
            share[f"rank_k{k}_M{M}"] = None if s is None else {"k_rank_chunk_s": s[0], "all_kernels_s": s[1], "share": s[0] / s[1]}
    rec["k_rank_chunk_share"] = share
    rec["all_s"] = ts
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
