"""The float64 reference of adkf_liar_pool and the assertions every comparison against it makes.

As in believer_ref.py the reference is CONDITIONED ON THE CALL'S OWN EARLIER PICKS: a greedy argmax sequence is not stable under
rounding, so no whole sequence is compared.  Unlike the kernels it uses no rank-one recursion: at step j the posterior is REBUILT by
oracle.gp_oracle.predict on the support set with the earlier picks' pool rows and the values they were conditioned on (sel_lie)
appended as labelled points at the same phi - reference and kernel share no algebra.  EI / log EI are believer_ref's.

Bounds (derived from ones the project already holds).  The pick panel c0 is held to TOL * os (tests/test_gpu_kg_pool.py), and the
conditioned mean is m_0 + c0(x, .) . beta with beta = (C_pp + noise I)^-1 (y - m_0(p)), so with L1_j = os * ||beta_(<j)||_1
    |dm_j| <= e_j = TOL * (max(1, max |m_j|) + L1_j)
    EI:      delta = TOL * max(1, max |score_j|) + TOL * L1_j
    log EI:  delta = (1 + u^2) * 2e-4 + 1e-4 + (1 + |u|) * TOL * L1_j / s
sel_var is held to TOL * os, sel_mean to e_j, sel_lie and inc exactly to the rule.  L1_j is a worst case and is capped: every
comparison asserts, from the reference alone, L1 <= L1_CAP."""
import numpy as np
import torch

from believer_ref import LOG_EI, MAXIMIZE, TOL, ei_ref, posterior
from test_log_ei_cpu import log_ei_ref

L1_CAP = 50.0
RAW_ONE = float(np.log(np.expm1(1.0)))   # softplus^-1(1)


def isotropic(Zs, ys, X, phi_t, ard):
    """(Zs, ys, X, phi [3]) in float64 of one task; ARD: the features over l at unit lengthscale (mu cancels in every distance)."""
    p = np.asarray(phi_t, np.float64)
    Zs, ys, X = np.asarray(Zs, np.float64), np.asarray(ys, np.float64), np.asarray(X, np.float64)
    if ard:
        l = np.logaddexp(0.0, p[2:])
        return Zs / l, ys, X / l, np.array([p[0], p[1], RAW_ONE])
    return Zs, ys, X, p[:3]


def expected_values(sel_idx, sel_mean, best, maximize, lie, labels):
    """(sel_lie [q], inc [q + 1]) by the rule, in float32: the first finite of the pick's label, the lie and the reported mean."""
    q = len(sel_idx)
    y = np.zeros(q, np.float32)
    inc = np.empty(q + 1, np.float32)
    inc[0] = np.float32(best)
    for j, p in enumerate(int(p) for p in sel_idx):
        if p >= 0:
            v = np.float32(labels[p]) if labels is not None else np.float32(np.nan)
            if not np.isfinite(v) and lie is not None:
                v = np.float32(lie)
            if not np.isfinite(v):
                v = np.float32(sel_mean[j])
            y[j] = v
            inc[j + 1] = max(inc[j], v) if maximize else min(inc[j], v)
        else:
            inc[j + 1] = inc[j]
    return y, inc


def liar_steps(task, kind, flags, picks, values, inc):
    """Per step j: (score_j, delta_j, m_j, v_j, e_j, L1_j) given picks[:j] conditioned on values[:j] and the incumbent inc[j]."""
    from oracle import gp_oracle as O

    Zs, ys, X, phi = task
    m0, S0, noise, os_ = posterior(Zs, ys, X, phi, kind)
    pt = torch.as_tensor(phi).double()
    mx = bool(flags & MAXIMIZE)
    steps, done = [], []
    for j, p in enumerate(picks):
        if done:
            Za, ya = np.concatenate([Zs, X[done]]), np.concatenate([ys, np.asarray(values[:len(done)], np.float64)])
            m, cov = O.predict(torch.as_tensor(Za), torch.as_tensor(ya), torch.as_tensor(X), pt, kind)
            m, v = m.numpy(), cov.diagonal().numpy() - noise
            Cpp = S0[np.ix_(done, done)] + noise * np.eye(len(done))
            beta = np.linalg.solve(Cpp, np.asarray(values[:len(done)], np.float64) - m0[done])
            l1 = os_ * float(np.abs(beta).sum())
        else:
            m, v, l1 = m0, S0.diagonal().copy(), 0.0
        best = float(inc[j])
        if flags & LOG_EI:
            score, u, _ = log_ei_ref(m, v, best, mx)
            delta = (1.0 + u * u) * 2 * TOL + 1e-4 + (1.0 + np.abs(u)) * TOL * l1 / np.sqrt(np.maximum(v, 1e-12))
        else:
            score = ei_ref(m, v, best, mx)
            delta = np.full(score.shape, TOL * max(1.0, np.abs(score).max()) + TOL * l1)
        steps.append((score, delta, m, v, TOL * (max(1.0, np.abs(m).max()) + l1), l1))
        if p >= 0 and p not in done:
            done.append(p)
    return steps, os_


def check_task(task, kind, best, flags, out, lie=None, labels=None, excluded=(), tag=""):
    """out: (sel_idx, sel_val, sel_mean, sel_var, sel_lie, inc, trace) of one task, trace [q, rows] or None.  Returns (the worst
    error / bound seen, the largest L1)."""
    sel_idx, sel_val, sel_mean, sel_var, sel_lie, inc, trace = out
    rows = task[2].shape[0]
    picks = [int(p) for p in sel_idx]
    y, inc_ref = expected_values(sel_idx, sel_mean, best, bool(flags & MAXIMIZE), lie, labels)
    assert np.array_equal(np.asarray(sel_lie, np.float32).view(np.int32), y.view(np.int32)), (tag, "sel_lie", sel_lie, y)
    assert np.array_equal(np.asarray(inc, np.float32).view(np.int32), inc_ref.view(np.int32)), (tag, "inc", inc, inc_ref)
    steps, os_ = liar_steps(task, kind, flags, picks, y, inc_ref)
    worst, l1_max = 0.0, 0.0
    taken = set(int(e) for e in excluded)
    for j, (s64, delta, m, v, e, l1) in enumerate(steps):
        p = picks[j]
        l1_max = max(l1_max, l1)
        assert l1 <= L1_CAP, (tag, j, "os * ||beta||_1 above the cap: the case is not one this bound covers", l1)
        if trace is not None:
            err = np.abs(trace[j].astype(np.float64) - s64) / delta
            worst = max(worst, float(err.max()))
            assert err.max() <= 1.0, (tag, j, "trace", float(err.max()), int(err.argmax()))
        ok = np.ones(rows, bool)
        ok[list(taken)] = False
        if p < 0:
            assert not ok.any() or np.isnan(s64[ok]).all(), (tag, j, "a step without a pick although rows are eligible")
            assert np.isneginf(sel_val[j]) and sel_mean[j] == 0 and sel_var[j] == 0 and sel_lie[j] == 0, (tag, j)
            continue
        assert ok[p], (tag, j, p, "an excluded or repeated pick")
        assert abs(float(sel_val[j]) - s64[p]) <= delta[p], (tag, j, "sel_val", float(sel_val[j]), s64[p], delta[p])
        top = int(np.argmax(np.where(ok, s64, -np.inf)))
        assert s64[p] >= s64[top] - (delta[p] + delta[top]), (tag, j, "selection", p, s64[p], top, s64[top], delta[p])
        worst = max(worst, abs(float(sel_mean[j]) - m[p]) / e, abs(float(sel_var[j]) - v[p]) / (TOL * os_))
        assert abs(float(sel_mean[j]) - m[p]) <= e, (tag, j, "sel_mean", float(sel_mean[j]), m[p], e)
        assert abs(float(sel_var[j]) - v[p]) <= TOL * os_, (tag, j, "sel_var", float(sel_var[j]), v[p])
        taken.add(p)
    return worst, l1_max
