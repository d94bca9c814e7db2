"""The float64 reference of adkf_mix_pool from GIVEN member values - the means m, variances v and EIs (or log EIs) e of a group's used
members at every row, as float arrays [n, rows] - for all four scores, with the error units of the GPU test, its constants, and the
problems the CPU and the GPU tests share.  The library normalises the weights in float32 (weights_of does the same), so the
reference and the call weigh with the same numbers."""
import numpy as np
import torch

import jes_ref as J

EPS32 = 2.0 ** -24
CLAMP = 1e-12
LATENT, MAXIMIZE, SCORE_MEAN, LOG_EI, SCORE_BALD = 1, 2, 4, 16, 32

# The float32 outputs against this reference at the call's own float32 members (tests/test_gpu_mix_pool.py): each constant is 4 times
# the largest ratio that test prints on the MI355X, rounded up to a power of two; the factor 4 is for shapes, seeds, compilers and
# libms the test does not visit.  eps32 here is 2^-24, half an ulp.  Largest ratios printed per case (rbf M = 3; matern M = 64;
# matern M = 5 with blocked tasks, padding and unequal weights; ARD M = 4):
#   mean (and the mean score) 1.608, 2.232, 1.815, 1.780        4 x 2.232 = 8.9 -> 16
#   var (latent and noisy)    2.145, 2.159, 2.348, 1.888        4 x 2.348 = 9.4 -> 16
#   ei                        1.704, 2.410, 1.777, 1.680        4 x 2.410 = 9.6 -> 16
#   log_ei (near, mid, far)   0.944, 1.230, 0.985, 0.953        4 x 1.230 = 4.9 -> 8
#   bald                      0.528, 0.525, 0.568, 0.477        4 x 0.568 = 2.3 -> 4
# See DESIGN.md, "Hyperparameter-marginalised prediction and acquisition".
EVAL_C_MEAN = 16.0
EVAL_C_VAR = 16.0
EVAL_C_EI = 16.0
EVAL_C_LOG = 8.0
EVAL_C_BALD = 4.0

# the GPU problems: (kernel, n_s per group, d, rows, M, spread); the last one is an ARD batch
CASES = [("rbf", [32, 29], 16, 200, 3, 0.3), ("matern", [16], 8, 130, 64, 0.3), ("matern", [200, 133, 64], 16, 130, 5, 0.3),
         ("rbf", [24, 17], 12, 65, 4, 0.3)]
CASE_ARD = [False, False, False, True]
MID_SHIFT, FAR_SHIFT = 4.0, 25.0


def weights_of(mem_row, w_row=None):
    """(tasks [n], wt [n] float64) of one group as the library forms them: the used entries in entry order, W their float32 sum in
    that order, wt = float32(w / W).  None for a group that cannot be evaluated by its table alone (T is not known here)."""
    ts, ws = [], []
    W = np.float32(-0.0)
    for j, t in enumerate(mem_row):
        if t == -1:
            continue
        w = np.float32(1.0 if w_row is None else w_row[j])
        if not (w >= 0) or np.isinf(w):
            return None
        if w > 0:
            ts.append(int(t)); ws.append(w); W = np.float32(W + w)
    if not ts or not np.isfinite(W):
        return None
    return np.array(ts), np.array([np.float32(w / W) for w in ws], np.float64)


def mix(m, v, e, wt, maximize=False, log=False):
    """The mixture of n members over the rows, in float64: m, v [n, rows], e [n, rows] the members' EI (log: their log EI) or None,
    wt [n].  Returns dict(mean, var, ei, log_ei, smean, bald) and the units unit_mean, unit_var, unit_ei, unit_log, unit_bald."""
    m, v, wt = np.asarray(m, np.float64), np.asarray(v, np.float64), np.asarray(wt, np.float64)[:, None]
    mean = (wt * m).sum(0)
    dev = m - mean
    var = (wt * v).sum(0) + (wt * dev * dev).sum(0)
    vc = np.maximum(v, CLAMP)
    varc = (wt * vc).sum(0) + (wt * dev * dev).sum(0)
    out = dict(mean=mean, var=var, smean=mean if maximize else -mean)
    out["bald"] = 0.5 * (np.log(varc) - (wt * np.log(vc)).sum(0))
    out["unit_mean"] = (wt * np.abs(m)).sum(0)
    out["unit_var"] = var + 2.0 * (wt * np.abs(dev)).sum(0) * out["unit_mean"]
    unit_varc = varc + 2.0 * (wt * np.abs(dev)).sum(0) * out["unit_mean"]
    out["unit_bald"] = 1.0 + np.abs(np.log(varc)) + (wt * np.abs(np.log(vc))).sum(0) + unit_varc / varc
    if e is not None:
        e = np.asarray(e, np.float64)
        if log:
            with np.errstate(divide="ignore", invalid="ignore"):
                mx = e.max(0)
                s = np.where(np.isneginf(e), 0.0, wt * np.exp(e - np.where(np.isneginf(mx), 0.0, mx))).sum(0)
                out["log_ei"] = np.where(s == 0.0, -np.inf, mx + np.log(s))
            out["unit_log"] = 1.0 + np.abs(out["log_ei"])
        else:
            out["ei"] = (wt * e).sum(0)
            out["unit_ei"] = out["ei"]
    return out


def by_monte_carlo(m, v, wt, n=400000, seed=0):
    """(mean, its standard error, variance, its standard error) of draws from the Gaussian mixture at one row: m, v, wt [n]."""
    g = np.random.default_rng(seed)
    i = g.choice(len(wt), size=n, p=np.asarray(wt) / np.sum(wt))
    y = np.asarray(m)[i] + np.sqrt(np.asarray(v)[i]) * g.standard_normal(n)
    mu, s2 = y.mean(), y.var(ddof=1)
    c4 = ((y - mu) ** 4).mean()
    return mu, np.sqrt(s2 / n), s2, np.sqrt(max(c4 - s2 * s2, 0.0) / n)


def topk_of(score, k, excluded=()):
    """adkf_predict_pool's selection on a float32 score row: larger first, ties by ascending row; NaN and excluded rows never."""
    score = np.asarray(score, np.float32)
    ok = ~np.isnan(score)
    ok[list(excluded)] = False
    rows = sorted(np.nonzero(ok)[0].tolist(), key=lambda r: (-score[r], r))[:k]
    idx = np.full(k, -1, np.int64)
    val = np.full(k, -np.inf, np.float32)
    idx[:len(rows)] = rows
    val[:len(rows)] = score[rows]
    return idx, val


def problem(case):
    """A GPU case on the host: dict(kernel, ard, Zs [G M, ns, d], ys, n_s [G M], X [rows, d], phi [G M, h], members [G, M] (int32),
    weights [G, M] or None, best_f [G M]).  jes_ref.problem(n_s, d, rows, 1500 + case) replicated M times, task g in the tasks
    g M .. g M + M - 1, under phi + spread randn(G M, 3); the ARD case expands the lengthscale per dimension.  Case 2 has one -1
    entry, one zero weight and unequal weights.  best_f: the group's smallest support label, for minimisation."""
    kernel, n_s, d, rows, M, spread = CASES[case]
    G = len(n_s)
    Zs, ys, X, phi = J.problem(n_s, d, rows, 1500 + case)
    rep = lambda t: t.repeat_interleave(M, 0).contiguous()
    phi = rep(phi) + spread * torch.randn(G * M, 3, generator=torch.Generator().manual_seed(77 + case))
    if CASE_ARD[case]:
        phi = torch.cat([phi[:, :2], phi[:, 2:3].expand(G * M, d)], 1)
    members = np.arange(G * M, dtype=np.int32).reshape(G, M)
    weights = None
    if case == 2:
        members[1, 3] = -1
        weights = np.ones((G, M), np.float32)
        weights[0] = [0.5, 2.0, 1.0, 0.25, 3.0]
        weights[2, 1] = 0.0
        weights[2, 4] = 1.75
    best = np.array([float(ys[g, :n_s[g]].min()) for g in range(G)], np.float32).repeat(M)
    return dict(kernel=kernel, ard=CASE_ARD[case], Zs=rep(Zs), ys=rep(ys), n_s=np.repeat(np.array(n_s, np.int32), M), X=X, phi=phi.float().contiguous(),
                members=members, weights=weights, best_f=best, G=G, M=M, rows=rows)
