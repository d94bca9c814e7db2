"""adkf_mix_pool against the host combination it replaces, on one GPU.

The mixture side: gp_ops.mix_pool(score="log_ei", topk=8, nothing per row) over G groups of M replicas each (T = G M tasks).
The host side: gp_ops.predict_pool with all three per-row outputs [T, rows] (mean, var, log EI), then the mixture and the selection
in torch: the log-sum-exp of log EI + log wt over the members, the mixture mean and total variance, topk.
Also timed: predict_pool with the three outputs alone (what stage A of the mixture costs, plus its stores to HBM) and
predict_pool(k, log EI) on the same batch (each replica scored at its own phi, no mixture).
Every side is warmed up, then timed alternately with device events around enough calls for at least half a second of work.

Usage: python tools/bench_mix_pool.py [--groups 32] [--members 8] [--ns 64] [--d 256] [--rows 100000] [--k 8] [--reps 5] [--out FILE]"""
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
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--ns", type=int, default=64)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    G, M, ns, d, rows, k = a.groups, a.members, a.ns, a.d, a.rows, a.k
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(G, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b0 = gp_ops.GPBatch(Zs, ys, torch.empty(G, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b0, True, True)
    phi, _, _, _, info = gp_ops.fit(b0, phi0, 200)
    gp_ops.check_info(info)
    phis = gp_ops.phi_laplace_samples(b0, phi, M, generator=torch.Generator().manual_seed(1))
    b, members = gp_ops.replicate_batch(b0, M)
    phis = phis.reshape(G * M, 3).contiguous()
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.min(1).values.repeat_interleave(M).contiguous()
    logw = torch.full((G, M, 1), -float(np.log(M)), device=dev)

    def f_mix():
        return gp_ops.mix_pool(b, phis, X, members=members, best_f=best, score="log_ei", latent=True, want_mean=False, want_var=False,
                               want_score=False, topk=k)

    def f_three():
        return gp_ops.predict_pool(b, phis, X, latent=True, best_f=best, want_mean=True, want_var=True, want_ei=True, log_ei=True)

    def f_host():
        pp = f_three()
        m, v, le = (pp[n].view(G, M, rows) for n in ("mean", "var", "ei"))
        score = torch.logsumexp(le + logw, 1)
        mean = m.mean(1)
        var = v.mean(1) + ((m - mean[:, None]) ** 2).mean(1)
        top = torch.topk(score, k, 1)
        return mean, var, top

    def f_map():
        return gp_ops.predict_pool(b, phis, X, latent=True, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=k, log_ei=True)

    sides = {"mix_pool": f_mix, "host_combination": f_host, "predict_pool_three_outputs": f_three, "predict_pool_topk": f_map}
    o1, o2 = f_mix(), f_mix()
    gp_ops.check_info(o1["info"])
    host = f_host()
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
    lib = _lib.load()
    rec = {"shape": f"mix G={G} M={M} T={G * M} ns={ns} d={d} rows={rows} k={k} matern log_ei latent; host: predict_pool mean+var+log EI [T, rows] + torch",
           "seconds": med, "calls_per_timing": n_calls,
           "host_over_mix": med["host_combination"] / med["mix_pool"], "mix_over_predict_topk": med["mix_pool"] / med["predict_pool_topk"],
           "stage_a_share_upper_bound": med["predict_pool_three_outputs"] / med["mix_pool"],
           "per_row_bytes_host_side": 3 * 4 * G * M * rows, "scratch_bytes": int(lib.adkf_mix_pool_scratch_bytes(G * M, G, k)),
           "workspace_bytes": int(lib.adkf_workspace_bytes(G * M, ns, 0, d)), "chunk_rows": int(_lib.MIX_CHUNK_ROWS),
           "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()},
           "repeat_is_bit_equal": bool(torch.equal(o1["top_idx"], o2["top_idx"]) and
                                       torch.equal(o1["top_val"].view(torch.int32), o2["top_val"].view(torch.int32))),
           "top1_agrees_with_host": float((o1["top_idx"][:, 0] == host[2].indices[:, 0]).float().mean()),
           "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
