"""The float64 restatement of adkf_qei_pool (include/adkf_gp.h) and the five assertions every comparison against it makes.

The paths are test_thompson_pool_cpu.paths_ref's (test_thompson_pool_ard_cpu.ard_paths_ref's for ARD tasks), on the pool rows and,
for the noisy incumbent, on the task's own support rows.  The reference is CONDITIONED ON GIVEN PICKS, the scheme of believer_ref: a
greedy argmax sequence is not stable under rounding, so no whole sequence is compared; at every step the scores of the call are
compared with the reference scores given the call's own earlier picks.

The bound.  A score is 1-Lipschitz in each path value and in each incumbent (a mean of clipped differences), an incumbent is
1-Lipschitz in the path values it is a minimum of, and the project holds float32 paths to 1e-4 max(1, |paths_ref|max)
(tests/test_gpu_thompson_pool.py): a path value and an incumbent each move a score by at most that, hence 2e-4 of the scale; the sum
of S float32 terms adds S 2^-24 of the score.
    delta = 2 * 1e-4 * max(1, |paths_ref|max) + S * 2^-24 * score_ref
and an incumbent is held to half of the first term."""
import numpy as np

MAXIMIZE = 2
TOL = 1e-4   # tests/test_gpu_thompson_pool.py's


def task_paths(zs, ys, phi_t, kind, X, omega, phase, w_t, eps_t, ard=False):
    """(paths [S, rows], sup_paths [S, n]) of one task in float64."""
    from test_thompson_pool_ard_cpu import ard_paths_ref
    from test_thompson_pool_cpu import paths_ref

    f = ard_paths_ref if ard else paths_ref
    both = f(zs, ys, phi_t, kind, np.concatenate([np.asarray(X, np.float64), np.asarray(zs, np.float64)]), omega, phase, w_t, eps_t)
    rows = np.asarray(X).shape[0]
    return both[:, :rows], both[:, rows:]


def incumbent0(paths, sup_paths, best_f, maximize):
    """b^0 [S]: the best value of each path over the support rows, or best_f for every path."""
    S = paths.shape[0]
    if best_f is not None:
        return np.full(S, float(best_f))
    return sup_paths.max(1) if maximize else sup_paths.min(1)


def qei_ref(paths, sup_paths, best_f, maximize, picks):
    """Per step j: (score_j [rows], b^j [S]) given picks[0 .. j - 1], then the final incumbents; the state stops changing at the
    first pick < 0."""
    b = incumbent0(paths, sup_paths, best_f, maximize).astype(np.float64)
    steps = []
    for p in picks:
        imp = (paths - b[:, None]) if maximize else (b[:, None] - paths)
        steps.append((np.maximum(imp, 0.0).mean(0), b.copy()))
        if p >= 0:
            b = np.maximum(b, paths[:, p]) if maximize else np.minimum(b, paths[:, p])
    return steps, b


def check_task(paths, sup_paths, best_f, maximize, sel_idx, sel_val, trace, inc, excluded=(), tag=""):
    """Assertions 1-5 on one task: sel_* [q], trace [q, rows] or None, inc [q + 1, S] or None.  Returns the worst error / bound."""
    S, rows = paths.shape
    picks = [int(p) for p in sel_idx]
    steps, b_end = qei_ref(paths, sup_paths, best_f, maximize, picks)
    delta0 = 2 * TOL * max(1.0, float(np.abs(paths).max()))
    worst = 0.0
    taken = set(int(e) for e in excluded if 0 <= int(e) < rows)
    ended = False
    for j, (s64, b64) in enumerate(steps):
        p = picks[j]
        delta = delta0 + S * 2.0 ** -24 * s64
        ok = np.ones(rows, bool)
        ok[list(taken)] = False
        if j == 0:   # the test must not pass vacuously
            assert ok.any() and (s64[ok] > 10 * delta[ok]).any(), (tag, "step 0: the reference maximum is within 10 delta of zero", float(s64.max()), delta0)
        if trace is not None:                                                                   # 1
            err = np.abs(trace[j].astype(np.float64) - s64) / delta
            worst = max(worst, float(err.max()))
            assert err.max() <= 1.0, (tag, j, "trace", float(err.max()), int(err.argmax()))
        if inc is not None:                                                                     # 4
            err = np.abs(inc[j].astype(np.float64) - b64).max() / (delta0 / 2)
            worst = max(worst, float(err))
            assert err <= 1.0, (tag, j, "inc", float(err))
        if p < 0:                                                                               # 5: the no-pick tail
            assert not ok.any(), (tag, j, "a step without a pick although rows are eligible")
            assert np.isneginf(sel_val[j]), (tag, j)
            ended = True
            continue
        assert not ended, (tag, j, "a pick after a step without one")
        assert 0 <= p < rows and ok[p], (tag, j, "the pick is excluded or was picked before", p)   # 5
        err = abs(float(sel_val[j]) - s64[p]) / delta[p]                                        # 2
        worst = max(worst, err)
        assert err <= 1.0, (tag, j, "sel_val", err)
        top = int(np.argmax(np.where(ok, s64, -np.inf)))                                        # 3
        assert s64[p] >= s64[top] - delta[p] - delta[top], (tag, j, "the pick is not the maximum", s64[p], s64[top])
        taken.add(p)
    if inc is not None:
        err = np.abs(inc[len(picks)].astype(np.float64) - b_end).max() / (delta0 / 2)
        worst = max(worst, float(err))
        assert err <= 1.0, (tag, "inc after the last step", float(err))
    return worst
