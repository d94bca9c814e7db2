"""The float64 reference of adkf_ipv_pool (target-variance batch selection) and the assertions every comparison against it makes.

As believer_ref.py: the reference starts from believer_ref.posterior - oracle.gp_oracle.predict's joint covariance over the pool
with the noise taken off the diagonal - and downdates that latent covariance pick by pick, S <- S - S[:, p] S[p, :] / (S[p, p] +
noise).  It is CONDITIONED ON GIVEN PICKS: a greedy argmax sequence is not stable under rounding, so no whole sequence is compared;
at every step the scores of the call are compared with the reference scores given the call's own earlier picks.

Per step j, with r_m the valid targets and wt_m their weights:
    score_j(x) = sum_m wt_m S_j[x, r_m]^2 / (max(S_j[x, x], 1e-12) + noise)
    tvar_j     = sum_m wt_m S_j[r_m, r_m]
    delta_j(x) = TOL os (2 sum_m wt_m |S_j[x, r_m]| + score_j(x)) / (S_j[x, x] + noise)
delta is the first-order effect on the score of the project's posterior bound, TOL os on every variance and covariance
(believer_ref.TOL, assertion 4 of believer_ref.check_task): d score = (2 sum wt cov dcov - score dv) / (v + noise)."""
import numpy as np

from believer_ref import TOL, posterior  # noqa: F401  (posterior: re-exported for the tests)


def valid_targets(tgt, w, rows):
    """The entries adkf_ipv_pool keeps: inside [0, rows), no earlier entry of the list with the same index, a weight > 0 (NaN fails).
    Returns (indices, weights) in list order."""
    tgt = [int(i) for i in tgt]
    w = [1.0] * len(tgt) if w is None else [float(np.float32(x)) for x in w]
    idx, wt = [], []
    for m, (p, x) in enumerate(zip(tgt, w)):
        if 0 <= p < rows and x > 0 and p not in tgt[:m]:
            idx.append(p); wt.append(x)
    return np.array(idx, np.int64), np.array(wt, np.float64)


def ipv_ref(post, tgt, w, picks):
    """(steps, tvar): steps[j] = (score_j [rows], delta_j [rows]) given picks[0 .. j - 1], tvar [len(picks) + 1]; the state stops
    changing at the first pick < 0.  tgt, w: the valid targets (valid_targets)."""
    _, S, noise, os_ = post
    S = S.copy()
    steps, tvar = [], []
    for p in list(picks) + [-1]:
        v = S.diagonal().copy()
        C = S[:, tgt]                                            # [rows, M]
        den = np.maximum(v, 1e-12) + noise
        score = (C * C * w).sum(1) / den
        delta = TOL * os_ * (2.0 * (np.abs(C) * w).sum(1) + score) / (v + noise)
        steps.append((score, delta))
        tvar.append(float((w * v[tgt]).sum()))
        if p >= 0:
            S = S - np.outer(S[:, p], S[p, :]) / (S[p, p] + noise)
    return steps[:-1], np.array(tvar)


def check_task(post, tgt, w, sel_idx, sel_val, tvar, trace, excluded=(), tag=""):
    """One task: sel_* [q], tvar [q + 1] or None, trace [q, rows] or None; tgt, w: the caller's entries as passed (None: weight 1).
    (1) the trace is within delta; (2) sel_val is within delta; (3) the pick is within delta[p] + delta[top] of the reference's best
    eligible row; (4) no excluded or repeated pick; and |tvar_j - ref| <= TOL os sum_m wt_m for every j.  A task without a valid
    target must report -1 / -inf and zeros.  Returns the worst error / bound seen (scores and tvar)."""
    rows = post[0].shape[0]
    os_ = post[3]
    idx, wt = valid_targets(tgt, w, rows)
    picks = [int(p) for p in sel_idx]
    if idx.size == 0:
        assert all(p == -1 for p in picks) and np.isneginf(sel_val).all(), (tag, "no valid target, yet a pick")
        assert tvar is None or (np.asarray(tvar) == 0).all(), (tag, "no valid target: tvar")
        assert trace is None or (np.asarray(trace) == 0).all(), (tag, "no valid target: trace")
        return 0.0
    steps, tv = ipv_ref(post, idx, wt, picks)
    worst = 0.0
    if tvar is not None:
        bound = TOL * os_ * wt.sum()
        err = np.abs(np.asarray(tvar, np.float64) - tv) / bound
        worst = max(worst, float(err.max()))
        assert err.max() <= 1.0, (tag, "tvar", float(err.max()), int(err.argmax()), np.asarray(tvar).tolist(), tv.tolist())
    taken = set(int(e) for e in excluded)
    for j, (s64, delta) in enumerate(steps):
        p = picks[j]
        if trace is not None:                                           # 1
            err = np.abs(trace[j].astype(np.float64) - s64) / delta
            worst = max(worst, float(err.max()))
            assert err.max() <= 1.0, (tag, j, "trace", float(err.max()), int(err.argmax()))
        ok = np.ones(rows, bool)
        ok[list(taken)] = False
        if p < 0:
            assert not ok.any() or np.isnan(s64[ok]).all(), (tag, j, "a step without a pick although rows are eligible")
            assert np.isneginf(sel_val[j]), (tag, j)
            continue
        assert ok[p], (tag, j, p, "an excluded or repeated pick")                                                    # 4
        err = abs(float(sel_val[j]) - s64[p]) / delta[p]
        worst = max(worst, err)
        assert err <= 1.0, (tag, j, "sel_val", float(sel_val[j]), s64[p], delta[p])                                  # 2
        top = int(np.argmax(np.where(ok, s64, -np.inf)))
        assert s64[p] >= s64[top] - (delta[p] + delta[top]), (tag, j, "selection", p, s64[p], top, s64[top], delta[p])   # 3
        taken.add(p)
    return worst
