"""The float64 reference of adkf_believer_pool and the four assertions every comparison against it makes.

The reference takes oracle.gp_oracle.predict's mean and joint covariance over the pool, removes the noise from the diagonal, and
downdates that latent covariance pick by pick, S <- S - S[:, p] S[p, :] / (S[p, p] + noise).  It is CONDITIONED ON GIVEN PICKS: a
greedy argmax sequence is not stable under rounding, so no whole sequence is compared; at every step the scores of the call are
compared with the reference scores given the call's own earlier picks."""
import math

import numpy as np
import torch

from test_log_ei_cpu import log_ei_ref

MAXIMIZE, LOG_EI = 2, 16
TOL = 1e-4   # tests/test_gpu_predict_pool.py's


def ei_ref(mean, var_latent, best, maximize):
    s = np.sqrt(np.maximum(var_latent, 1e-12))
    u = ((mean - best) if maximize else (best - mean)) / s
    cdf = np.array([0.5 * math.erfc(-x / math.sqrt(2.0)) for x in u])
    return s * (u * cdf + np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi))


def posterior(Zs, ys, X, phi_t, kind):
    """(mean [rows], latent covariance [rows, rows], noise, outputscale) of one task over the pool, float64."""
    from oracle import gp_oracle as O

    pt = torch.as_tensor(phi_t).double()
    m, cov = O.predict(torch.as_tensor(Zs).double(), torch.as_tensor(ys).double(), torch.as_tensor(X).double(), pt, kind)
    noise, os_, _ = O.transform_phi(pt)
    S = cov.numpy().copy()
    S[np.diag_indices_from(S)] -= float(noise)
    return m.numpy(), S, float(noise), float(os_)


def believer_ref(post, best, flags, picks):
    """Per step j: (score_j [rows], delta_j [rows], latent variance [rows], incumbent) given picks[0 .. j - 1]; stops changing the
    state at the first pick < 0.  delta is the bound a float32 score is held to: 1e-4 max(1, max |score_j|) for EI (the bound and
    norm of tests/test_gpu_predict_pool.py), (1 + u^2) 2e-4 + 1e-4 per row for log EI (tests/test_gpu_log_ei.py's)."""
    m, S, noise, _ = post
    S = S.copy()
    best = float(best)
    mx = bool(flags & MAXIMIZE)
    steps = []
    for p in picks:
        v = S.diagonal().copy()
        if flags & LOG_EI:
            score, u, _ = log_ei_ref(m, v, best, mx)
            delta = (1.0 + u * u) * 2 * TOL + 1e-4
        else:
            score = ei_ref(m, v, best, mx)
            delta = np.full(score.shape, TOL * max(1.0, np.abs(score).max()))
        steps.append((score, delta, v, best))
        if p >= 0:
            S = S - np.outer(S[:, p], S[p, :]) / (S[p, p] + noise)
            best = max(best, m[p]) if mx else min(best, m[p])
    return steps


def check_task(post, best, flags, sel_idx, sel_val, sel_mean, sel_var, trace, excluded=(), tag=""):
    """Assertions 1-4 on one task: sel_* [q], trace [q, rows] or None.  Returns the worst error / bound seen."""
    m, _, _, os_ = post
    rows = m.shape[0]
    picks = [int(p) for p in sel_idx]
    steps = believer_ref(post, best, flags, picks)
    worst = 0.0
    taken = set(int(e) for e in excluded)
    for j, (s64, delta, v, _) in enumerate(steps):
        p = picks[j]
        if trace is not None:                                           # 1
            err = np.abs(trace[j].astype(np.float64) - s64) / delta
            worst = max(worst, float(err.max()))
            assert err.max() <= 1.0, (tag, j, "trace", float(err.max()), int(err.argmax()))
        ok = np.ones(rows, bool)
        ok[list(taken)] = False
        if p < 0:
            assert not ok.any() or np.isnan(s64[ok]).all(), (tag, j, "a step without a pick although rows are eligible")
            assert np.isneginf(sel_val[j]) and sel_mean[j] == 0 and sel_var[j] == 0, (tag, j)
            continue
        assert ok[p], (tag, j, p, "an excluded or repeated pick")
        assert abs(float(sel_val[j]) - s64[p]) <= delta[p], (tag, j, "sel_val", float(sel_val[j]), s64[p], delta[p])   # 2
        top = int(np.argmax(np.where(ok, s64, -np.inf)))
        assert s64[p] >= s64[top] - (delta[p] + delta[top]), (tag, j, "selection", p, s64[p], top, s64[top], delta[p])   # 3
        assert abs(float(sel_mean[j]) - m[p]) <= TOL * max(1.0, np.abs(m).max()), (tag, j, "sel_mean")           # 4
        assert abs(float(sel_var[j]) - v[p]) <= TOL * os_, (tag, j, "sel_var", float(sel_var[j]), v[p])
        taken.add(p)
    return worst
