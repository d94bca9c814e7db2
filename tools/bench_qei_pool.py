"""adkf_qei_pool against adkf_thompson_pool at the same shape, on one GPU.

The q-EI side: gp_ops.qei_pool at q picks with S = 64 and S = 256 draws, noisy incumbents, no trace, no inc.
The baseline: gp_ops.thompson_pool with S = 64 draws and no paths - one walk of the tile that q-EI walks q times, with its residual
and solve (which q-EI runs once per call).  With ADKF_LIB pointing at another build of the library the same tool times that build's
Thompson call (the q-EI sides are skipped where the library has no adkf_qei_pool).
Reported: t_qei(S = 64) / (q t_thompson) - the epilogue's per-row reduction against Thompson's per-lane scan, the residual and the solve
once instead of q times - and t_qei(S = 256) / t_qei(S = 64), what sharing the feature and kernel panels between four sample blocks buys
(4 without sharing).  Every side is warmed up, then timed alternately with device events around enough calls for at least half a
second of work.

Usage: python tools/bench_qei_pool.py [--tasks 16] [--ns 128] [--d 256] [--rows 100000] [--features 1024] [--q 8] [--reps 5] [--out FILE]"""
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
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T, ns, d, rows, m, q = a.tasks, a.ns, a.d, a.rows, a.features, a.q
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1)) + 0.1 * torch.randn(T, ns, device=dev, generator=g)
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi, _ = gp_ops.init_params_batch(b, True, True)   # phi GIVEN (the median heuristic): every call pays the same inner stage
    X = torch.randn(rows, d, device=dev, generator=g) @ W
    omega, phase = gp_ops.rff_basis("matern", d, m, generator=torch.Generator().manual_seed(1), device=dev)
    w = torch.randn(T, 256, m, device=dev, generator=g)
    eps = torch.randn(T, 256, ns, device=dev, generator=g)
    cut = lambda S: dict(omega=omega, phase=phase, n_samples=S, w=w[:, :S].contiguous(), eps=eps[:, :S].contiguous())
    k64, k256 = cut(64), cut(256)
    have_qei = hasattr(_lib.load(), "adkf_qei_pool") and hasattr(gp_ops, "qei_pool")
    sides = {"thompson_S64": lambda: gp_ops.thompson_pool(b, phi, X, **k64)}
    if have_qei:
        sides["qei_S64"] = lambda: gp_ops.qei_pool(b, phi, X, q=q, **k64)
        sides["qei_S256"] = lambda: gp_ops.qei_pool(b, phi, X, q=q, **k256)
        sides["qei_S64_q1"] = lambda: gp_ops.qei_pool(b, phi, X, q=1, **k64)
    rec = {"shape": f"T={T} ns={ns} d={d} rows={rows} m={m} q={q} matern; no per-row output", "library": os.path.relpath(_lib.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))}
    if have_qei:
        o1, o2 = sides["qei_S256"](), sides["qei_S256"]()
        gp_ops.check_info(o1["info"])
        rec["repeat_is_bit_equal"] = bool(torch.equal(o1["sel_idx"], o2["sel_idx"]) and torch.equal(o1["sel_val"].view(torch.int32), o2["sel_val"].view(torch.int32)))
        rec["mc_qei_of_the_batch_mean"] = float(o1["sel_val"].sum(1).mean())
        rec["scratch_bytes"] = {S: int(_lib.load().adkf_qei_pool_scratch_bytes(T, ns, S, m)) for S in (64, 256)}
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
    if have_qei:
        rec["qei_S64_over_q_thompson"] = med["qei_S64"] / (q * med["thompson_S64"])
        rec["qei_S256_over_qei_S64"] = med["qei_S256"] / med["qei_S64"]
        rec["per_step_s"] = {"S64": (med["qei_S64"] - med["qei_S64_q1"]) / max(1, q - 1)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
