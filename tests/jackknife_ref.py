"""The float64 reference of adkf_jackknife_pool (leave-one-out checks and jackknife+ intervals) and the assertions every comparison
against it makes.

As believer_ref.posterior, the reference is built from oracle.gp_oracle quantities: A = K_ss + noise I from kernel_matrix and
transform_phi, B = A^-1, alpha = B y, and per pool row c = k B, m = c . y, v = os - c . k.  Then, with phi fixed,
    g_i = alpha_i / B_ii,   loo_mean_i = y_i - g_i,   loo_var_i = 1 / B_ii,   loo_lpd = sum_i [-log(2 pi / B_ii) / 2 - g_i^2 B_ii / 2]
    mu_-i(x) = m(x) - c_i(x) g_i,    v_-i(x) = v(x) + c_i(x)^2 / B_ii
    plain:  a_i = mu_-i - |g_i|,  b_i = mu_-i + |g_i|
    scaled: s_i = |g_i| sqrt(B_ii), sd_i = sqrt(max(v_-i, 1e-12) + noise), a_i = mu_-i - s_i sd_i, b_i = mu_-i + s_i sd_i
    lo = the k-th smallest a, hi = the k-th largest b, k = floor(float64(float32(alpha)) (n + 1)); k = 0: -inf / +inf.

The bounds are first-order effects of the project's posterior bounds (believer_ref.TOL = 1e-4): TOL max(1, |.|max) on every mean and
TOL os on every variance; no new constant.  Order statistics are 1-Lipschitz in the sup norm of their inputs, so an endpoint is off
by at most the worst fold value.  With Mx = max(1, max |y|, max |mu_-i(x)|):
    plain       delta    = 2 TOL Mx   (the leave-one-out prediction at x and the leave-one-out residual are each a prediction)
    scaled      delta(x) = max_i [ TOL Mx + sd_i (sqrt(B_ii) TOL Mx + s_i TOL os B_ii / 2) + s_i TOL os / (2 sd_i) ]
    loo_mean    TOL Mx,     loo_var   TOL os,     loo_lpd   sum_i [ |g_i| B_ii TOL Mx + |g_i^2 B_ii^2 - B_ii| TOL os / 2 ]."""
import numpy as np
import torch

from believer_ref import TOL

RAW_ONE = float(np.log(np.expm1(1.0)))


def state(Zs, ys, X, phi_t, kind):
    """The float64 quantities of one task over the pool X [rows, d] (rows may be 0)."""
    from oracle import gp_oracle as O

    pt = torch.as_tensor(np.asarray(phi_t, np.float64))
    Z = torch.as_tensor(np.asarray(Zs, np.float64))
    y = np.asarray(ys, np.float64)
    Xq = torch.as_tensor(np.asarray(X, np.float64)).reshape(-1, Z.shape[1])
    noise, os_, ls = O.transform_phi(pt)
    n = Z.shape[0]
    A = (O.kernel_matrix(Z, Z, os_, ls, kind) + noise * torch.eye(n, dtype=torch.float64)).numpy()
    K = O.kernel_matrix(Xq, Z, os_, ls, kind).numpy()
    B = np.linalg.inv(A)
    B = 0.5 * (B + B.T)
    alpha = B @ y
    C = K @ B
    bii = B.diagonal().copy()
    return dict(n=n, y=y, B=B, bii=bii, alpha=alpha, g=alpha / bii, C=C, K=K, m=C @ y, v=float(os_) - (C * K).sum(1), noise=float(noise),
                os=float(os_))


def ard_state(Zs, ys, X, phi_t, kind):
    """state() of an ARD task: the isotropic state at unit lengthscale on the features over l (the centring cancels)."""
    p = np.asarray(phi_t, np.float64)
    l = np.logaddexp(0.0, p[2:])
    return state(np.asarray(Zs, np.float64) / l, ys, np.asarray(X, np.float64) / l, np.array([p[0], p[1], RAW_ONE]), kind)


def rank(alpha, n):
    """The rank of a level: from the float32 bits of alpha, exactly."""
    a = np.float32(alpha)
    if not (a > 0 and a < 1) or n <= 0:
        return 0
    return int(np.floor(np.float64(a) * np.float64(n + 1)))


def folds(st, scaled):
    """(mu [rows, n], a, b, s [n], sd [rows, n]) - s and sd are None in the plain form."""
    mu = st["m"][:, None] - st["C"] * st["g"][None, :]
    if not scaled:
        w = np.abs(st["g"])[None, :]
        return mu, mu - w, mu + w, None, None
    s = np.abs(st["g"]) * np.sqrt(st["bii"])
    sd = np.sqrt(np.maximum(st["v"][:, None] + st["C"] ** 2 / st["bii"][None, :], 1e-12) + st["noise"])
    return mu, mu - s[None, :] * sd, mu + s[None, :] * sd, s, sd


def loo_ref(st):
    """(loo_mean, loo_var, loo_lpd) and, given Mx, their bounds through loo_bounds."""
    g, bii = st["g"], st["bii"]
    return st["y"] - g, 1.0 / bii, float(np.sum(-0.5 * np.log(2.0 * np.pi / bii) - 0.5 * g * g * bii))


def scale_of(st, mu):
    return max(1.0, float(np.abs(st["y"]).max()), float(np.abs(mu).max()) if mu.size else 0.0)


def loo_bounds(st, Mx):
    g, bii = st["g"], st["bii"]
    return TOL * Mx, TOL * st["os"], float(np.sum(np.abs(g) * bii * TOL * Mx + 0.5 * np.abs(g * g * bii * bii - bii) * TOL * st["os"]))


def jackknife_ref(st, alphas, scaled):
    """(lo [L, rows], hi [L, rows], delta [rows], ranks [L], Mx)."""
    mu, a, b, s, sd = folds(st, scaled)
    rows, n = mu.shape
    Mx = scale_of(st, mu)
    if scaled:
        bii = st["bii"][None, :]
        per = TOL * Mx + sd * (np.sqrt(bii) * TOL * Mx + s[None, :] * TOL * st["os"] * bii / 2.0) + s[None, :] * TOL * st["os"] / (2.0 * sd)
        delta = per.max(1) if rows else np.zeros(0)
    else:
        delta = np.full(rows, 2.0 * TOL * Mx)
    sa, sb = np.sort(a, 1), -np.sort(-b, 1)
    ranks = [rank(al, n) for al in alphas]
    lo = np.stack([sa[:, k - 1] if k > 0 else np.full(rows, -np.inf) for k in ranks])
    hi = np.stack([sb[:, k - 1] if k > 0 else np.full(rows, np.inf) for k in ranks])
    return lo, hi, delta, ranks, Mx


def check_task(st, alphas, scaled, maximize, lo, hi, loo=None, top_idx=None, top_val=None, excluded=(), tag=""):
    """One task: lo, hi [L, rows] or None; loo = (loo_mean [ns], loo_var [ns], loo_lpd) or None; top_idx, top_val [k] or None.
    (1) every finite endpoint within delta, the infinite ones exactly; (2) the leave-one-out outputs within their bounds, 0 beyond n;
    (3) the selection: top_val within delta of the reference score of its row, the pick's reference score within delta[p] + delta[top]
    of the best eligible one (believer_ref's assertion 3), no excluded, repeated or infinite-score pick, and as many picks as there
    are eligible rows, up to k.  Returns the worst error / bound seen."""
    rlo, rhi, delta, ranks, Mx = jackknife_ref(st, alphas, scaled)
    rows, n = rlo.shape[1], st["n"]
    worst = 0.0
    for name, got, ref in (("lo", lo, rlo), ("hi", hi, rhi)):
        if got is None:
            continue
        got = np.asarray(got, np.float64)
        assert got.shape == ref.shape, (tag, name, got.shape, ref.shape)
        for l, k in enumerate(ranks):
            if k == 0:
                assert (got[l] == ref[l]).all(), (tag, name, l, "a level without a rank must give the infinity")
                continue
            if rows == 0:
                continue
            err = np.abs(got[l] - ref[l]) / delta
            worst = max(worst, float(err.max()))
            assert err.max() <= 1.0, (tag, name, l, k, float(err.max()), int(err.argmax()), got[l][err.argmax()], ref[l][err.argmax()])
    if loo is not None:
        rm, rv, rl = loo_ref(st)
        bm, bv, bl = loo_bounds(st, Mx)
        gm, gv, gl = np.asarray(loo[0], np.float64), np.asarray(loo[1], np.float64), float(loo[2])
        assert (gm[n:] == 0).all() and (gv[n:] == 0).all(), (tag, "slots beyond n hold 0")
        for name, e in (("loo_mean", np.abs(gm[:n] - rm).max() / bm), ("loo_var", np.abs(gv[:n] - rv).max() / bv), ("loo_lpd", abs(gl - rl) / bl)):
            worst = max(worst, float(e))
            assert e <= 1.0, (tag, name, float(e))
    if top_idx is not None:
        picks = [int(p) for p in top_idx]
        score = rlo[0] if maximize else -rhi[0]
        ok = np.isfinite(score)
        ok[[int(e) for e in excluded]] = False
        want = min(len(picks), int(ok.sum()))
        got = [p for p in picks if p >= 0]
        assert len(got) == want and picks[:want] == got and len(set(got)) == len(got), (tag, "selection", picks, want)
        assert np.isneginf(np.asarray(top_val)[want:]).all(), (tag, "the tail of top_val")
        left = ok.copy()
        for j, p in enumerate(got):
            assert ok[p], (tag, j, p, "an excluded pick, or one without a finite score")
            err = abs(float(top_val[j]) - score[p]) / delta[p]
            worst = max(worst, err)
            assert err <= 1.0, (tag, j, "top_val", float(top_val[j]), score[p], delta[p])
            top = int(np.argmax(np.where(left, score, -np.inf)))
            assert score[p] >= score[top] - (delta[p] + delta[top]), (tag, j, "selection", p, score[p], top, score[top])
            left[p] = False
    return worst
