"""adkf_predict_grad against adkf_predict_marginal on the same packed rows, and against a torch restatement with autograd, on one GPU.

The gradient side: gp_ops.predict_grad with all three cotangents (EI), dZq [rows, d] written.
The baseline: gp_ops.predict_marginal with mean, var and EI written - the walk the gradient's tile is built on.
The torch side: the same posterior restated with torch on the device (cdist-free distances, cholesky_solve against the per-task
factor, EI) and differentiated by autograd, the factorisation outside the timed region.
The split: predict_grad with g_mean alone at d_small = 64 columns of the same rows, against predict_marginal there: how the cost
moves with d (the first and the third product scale with d, the second does not); and both calls on a fitted batch with
REUSE_INNER, where nothing but the streaming launches is left (the other sides pay the inner stage of T tasks in every call).
Every side is warmed up, then timed alternately with device events around enough calls for at least half a second of work.

Usage: python tools/bench_predict_grad.py [--tasks 256] [--ns 128] [--d 256] [--rows 16384] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adkf_ift_amd import gp_ops  # noqa: E402


def timed(fn, n):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / 1e3 / n


def torch_side(Zs, ys, phi, X, q_off, best, cots):
    """sum(g_mean m + g_var v + g_ei EI) of the packed rows, restated with torch and differentiated by autograd (Matern-5/2)."""
    T, ns, d = Zs.shape
    sp = torch.nn.functional.softplus
    noise, os_, ls = sp(phi[:, 0]) + 1e-4, sp(phi[:, 1]), sp(phi[:, 2])

    def kern(a, b_, t):
        d2 = ((a * a).sum(-1)[:, None] + (b_ * b_).sum(-1)[None, :] - 2.0 * a @ b_.T).clamp_min(0.0) / (ls[t] * ls[t])
        r = torch.sqrt(d2 + 1e-30)
        return os_[t] * (1.0 + 5.0 ** 0.5 * r + (5.0 / 3.0) * d2) * torch.exp(-(5.0 ** 0.5) * r)

    Ls = [torch.linalg.cholesky(kern(Zs[t], Zs[t], t) + noise[t] * torch.eye(ns, device=Zs.device)) for t in range(T)]
    off = q_off.tolist()

    def run():
        x = X.detach().clone().requires_grad_(True)
        total = x.new_zeros(())
        for t in range(T):
            lo, hi = off[t], off[t + 1]
            if hi == lo:
                continue
            K = kern(x[lo:hi], Zs[t], t)
            C = torch.cholesky_solve(K.T, Ls[t]).T
            m, v = C @ ys[t], os_[t] - (C * K).sum(1)
            s = torch.sqrt(v.clamp_min(1e-12))
            u = (best[t] - m) / s
            ei = s * (u * 0.5 * torch.erfc(-u / 2.0 ** 0.5) + torch.exp(-0.5 * u * u) / (2.0 * np.pi) ** 0.5)
            total = total + (cots[0][lo:hi] * m).sum() + (cots[1][lo:hi] * v).sum() + (cots[2][lo:hi] * ei).sum()
        (g,) = torch.autograd.grad(total, x)
        return g
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=256)
    ap.add_argument("--ns", type=int, default=128)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16384)
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
    per = [rows // T + (1 if t < rows % T else 0) for t in range(T)]
    q_off = torch.tensor([0] + list(np.cumsum(per)), dtype=torch.int64, device=dev)
    best = ys.median(1).values.contiguous()
    cots = [torch.randn(rows, device=dev, generator=g) for _ in range(3)]
    ds = min(64, d)
    bs = gp_ops.GPBatch(Zs[..., :ds].contiguous(), ys, torch.empty(T, 4, device=dev), "matern")
    phis, _ = gp_ops.init_params_batch(bs, True, True)
    Xs = X[:, :ds].contiguous()

    sides = {"predict_marginal_ei": lambda: gp_ops.predict_marginal(b, phi, X, q_off, best_f=best),
             "predict_grad_all": lambda: gp_ops.predict_grad(b, phi, X, q_off, g_mean=cots[0], g_var=cots[1], g_ei=cots[2], best_f=best),
             "predict_grad_mean": lambda: gp_ops.predict_grad(b, phi, X, q_off, g_mean=cots[0]),
             "predict_marginal_d_small": lambda: gp_ops.predict_marginal(bs, phis, Xs, q_off),
             "predict_grad_mean_d_small": lambda: gp_ops.predict_grad(bs, phis, Xs, q_off, g_mean=cots[0]),
             "torch_autograd": torch_side(Zs, ys, phi, X, q_off.cpu(), best, cots)}
    # the streaming launches alone: a second batch fitted once, then every call reuses the fit's inner state (REUSE_INNER)
    br = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phir0, _ = gp_ops.init_params_batch(br, True, True)
    br.flags = gp_ops.REUSE_DIST
    phir, _, _, _, info = gp_ops.fit(br, phir0, 20)
    gp_ops.check_info(info)
    br.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    sides["predict_marginal_ei_reuse"] = lambda: gp_ops.predict_marginal(br, phir, X, q_off, best_f=best)
    sides["predict_grad_all_reuse"] = lambda: gp_ops.predict_grad(br, phir, X, q_off, g_mean=cots[0], g_var=cots[1], g_ei=cots[2], best_f=best)
    o1, o2 = sides["predict_grad_all"](), sides["predict_grad_all"]()
    gp_ops.check_info(o1[1])
    gt = sides["torch_autograd"]()
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
    base = med["predict_marginal_ei"]
    rec = {"shape": f"T={T} ns={ns} d={d} rows={rows} matern; dZq [rows, d] against predict_marginal mean/var/ei [rows]; d_small={ds}",
           "seconds": med, "calls_per_timing": n_calls,
           "grad_over_predict": med["predict_grad_all"] / base, "grad_mean_over_predict": med["predict_grad_mean"] / base,
           "grad_over_predict_d_small": med["predict_grad_mean_d_small"] / med["predict_marginal_d_small"],
           "grad_over_predict_reuse": med["predict_grad_all_reuse"] / med["predict_marginal_ei_reuse"],
           "torch_over_grad": med["torch_autograd"] / med["predict_grad_all"],
           "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()},
           "repeat_is_bit_equal": bool(torch.equal(o1[0].view(torch.int32), o2[0].view(torch.int32))),
           "max_diff_vs_torch_over_max": float((o1[0] - gt).abs().max() / gt.abs().max()),
           "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
