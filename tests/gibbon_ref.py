"""The float64 reference of adkf_gibbon_pool (GIBBON, Moss et al. 2021) and what every comparison against it asserts.  Helpers for
the tests; not a test module.

The posterior is believer_ref.posterior's (the oracle's mean and latent covariance over the pool, and the noise); h(gamma) =
tau (gamma + tau), tau = phi / Phi, comes from mpmath at 50 digits - gamma + tau cancels to ~1 / |gamma| of its terms on the left, which
50 digits cover anywhere a float32 gamma can reach in the tests.  As believer_ref, the reference is CONDITIONED ON GIVEN PICKS,
S <- S - S[:, p] S[p, :] / (S[p, p] + noise): a greedy argmax sequence is not stable under rounding, so only per-step scores are
compared, each step given the call's own earlier picks.

The bound delta a float32 score is held to, per row, has two parts:
  derived     the project's posterior bounds |dm| <= 1e-4 max(1, max |m|) and |dv| <= 1e-4 os, the latter for v_0 and v_j alike,
              pushed through the float64 score by evaluating it at the eight corners of the perturbed inputs (a fast float64 h serves
              both ends of each difference) and taking the largest deviation;
  evaluation  EVAL_C eps32 mean_s (1 + gamma_s^2): the float32 evaluation of the S terms and the logarithm of the variance ratio from
              the call's own float32 mean and variances.  EVAL_C is four times the largest ratio measured on the MI355X at the call's
              own posterior (tests/test_gpu_gibbon_pool.py::test_the_epilogue_alone prints it), rounded up to a power of two."""
import math
from unittest import mock

import mpmath as mp
import numpy as np

import believer_ref as B

MAXIMIZE = 2
TOL = B.TOL
EPS32 = float(np.finfo(np.float32).eps)
EVAL_C = 32.0   # measured: 5.63 (matern, ns = 200, -12 < gamma <= -1; rbf, ns = 32: 5.49); 4 x 5.63 = 22.5 -> 32
CLAMP = 1e-12


def h_ref(gamma):
    """h(gamma) as a float from 50 digits; NaN for a NaN or infinite gamma."""
    gamma = float(gamma)
    if not math.isfinite(gamma):
        return float("nan")
    with mp.workdps(50):
        x = mp.mpf(gamma)
        tau = mp.npdf(x) / mp.ncdf(x)
        return float(tau * (x + tau))


def _h64(g):
    """h in float64 for the perturbed evaluations: as written down to gamma = -8, through Mills' ratio below (h = -U / M^2)."""
    if not math.isfinite(g):
        return float("nan")
    if g > -8.0:
        pdf = math.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
        tau = pdf / (1.0 - 0.5 * math.erfc(g / math.sqrt(2.0))) if g > 0.0 else pdf / (0.5 * math.erfc(-g / math.sqrt(2.0)))
        return tau * (g + tau)
    w = 1.0 / (g * g)
    U = term = -1.0
    for k in range(1, 64):
        nxt = -term * (2 * k + 1) * w
        if abs(nxt) >= abs(term):
            break
        term = nxt
        U += term
    M = 1.0 + w * U
    return -U / (M * M)


_h64v = np.vectorize(_h64, otypes=[np.float64])
_hrefv = np.vectorize(h_ref, otypes=[np.float64])


def gamma_of(mean, v0, ystar_t, maximize, clamp=CLAMP):
    """gamma [rows, S] = +-(ystar_t[s] - mean) / sqrt(max(v0, clamp))."""
    sigma = np.sqrt(np.maximum(np.asarray(v0, np.float64), clamp))
    diff = np.asarray(ystar_t, np.float64)[None, :] - np.asarray(mean, np.float64)[:, None]
    return (diff if maximize else -diff) / sigma[:, None]


_a_cache = {}


def a_ref(mean, v0, noise, ystar_t, maximize, h=_hrefv, clamp=CLAMP):
    """(a [rows], gamma [rows, S]): the single-point score -(1 / 2S) sum_s log1p(-rho2 h(gamma_s)).  The mpmath values are kept per
    input, so that the comparisons of one problem (device, twin, every step) share them."""
    mean, v0, ystar_t = (np.ascontiguousarray(x, np.float64) for x in (mean, v0, ystar_t))
    key = (mean.tobytes(), v0.tobytes(), float(noise), ystar_t.tobytes(), bool(maximize), clamp) if h is _hrefv else None
    if key not in _a_cache:
        vc = np.maximum(v0, clamp)
        gamma = gamma_of(mean, v0, ystar_t, maximize, clamp)
        rho2 = vc / (vc + noise)
        out = -0.5 * np.log1p(-rho2[:, None] * h(gamma)).mean(axis=1), gamma
        if key is None:
            return out
        _a_cache[key] = out
    return _a_cache[key]


def log_ratio(v0, vj, noise):
    return 0.5 * np.log((np.maximum(vj, CLAMP) + noise) / (np.maximum(v0, CLAMP) + noise))


def gamma_weight(gamma):
    """mean_s (1 + gamma_s^2) per row: what the float32 error of the S terms scales with."""
    return (1.0 + np.asarray(gamma, np.float64) ** 2).mean(axis=1)


def gibbon_steps(post, ystar_t, maximize, picks):
    """Per step j: (score_j [rows], delta_j [rows], latent variance v_j [rows], None) given picks[0 .. j - 1] - believer_ref's
    tuples; the state stops changing at the first pick < 0."""
    m, S, noise, os_ = post
    S = S.copy()
    v0 = S.diagonal().copy()
    a, gamma = a_ref(m, v0, noise, ystar_t, maximize)
    evaluation = EVAL_C * EPS32 * gamma_weight(gamma)
    dm, dv = TOL * max(1.0, np.abs(m).max()), TOL * os_
    a_mid = a_ref(m, v0, noise, ystar_t, maximize, h=_h64v)[0]
    a_dev = {(sm, s0): a_ref(m + sm * dm, v0 + s0 * dv, noise, ystar_t, maximize, h=_h64v)[0] - a_mid for sm in (-1, 1) for s0 in (-1, 1)}
    steps = []
    for p in picks:
        v = S.diagonal().copy()
        score = a + log_ratio(v0, v, noise)
        l_mid = log_ratio(v0, v, noise)
        derived = np.zeros_like(a)
        for (sm, s0), da in a_dev.items():
            for sj in (-1, 1):
                derived = np.fmax(derived, np.abs(da + log_ratio(v0 + s0 * dv, v + sj * dv, noise) - l_mid))
        steps.append((score, derived + evaluation, v, None))
        if p >= 0:
            S = S - np.outer(S[:, p], S[p, :]) / (S[p, p] + noise)
    return steps


def check_task(post, ystar_t, maximize, sel_idx, sel_val, sel_mean, sel_var, trace, excluded=(), tag=""):
    """believer_ref.check_task's assertions 1-4 (trace, sel_val, selection within delta[p] + delta[top], sel_mean / sel_var) with the
    scores and bounds of this module.  Returns the worst trace error / bound seen."""
    steps = gibbon_steps(post, ystar_t, maximize, [int(p) for p in sel_idx])
    with mock.patch.object(B, "believer_ref", lambda *_: steps):
        return B.check_task(post, 0.0, MAXIMIZE if maximize else 0, sel_idx, sel_val, sel_mean, sel_var, trace, excluded=excluded, tag=tag)


def ystar_above(post, S, maximize):
    """The reference inputs: ystar_s = max_x m(x) + c_s sqrt(os), c_s spread over [0.05, 2]; mirrored for minimisation."""
    m, _, _, os_ = post
    c = np.linspace(0.05, 2.0, S) if S > 1 else np.array([0.5])
    return ((m.max() + c * math.sqrt(os_)) if maximize else (m.min() - c * math.sqrt(os_))).astype(np.float32)


def ystar_below(post, S, maximize):
    """The second set: ystar BELOW the pool's means (above, for minimisation) by 1.5 to 14 prior deviations, so that every gamma is
    <= -1 and those of the far samples <= -12: the left branch of pm_gibbon_term and its series (one sample: 3 deviations)."""
    m, _, _, os_ = post
    c = np.linspace(1.5, 14.0, S) if S > 1 else np.array([3.0])
    return ((m.min() - c * math.sqrt(os_)) if maximize else (m.max() + c * math.sqrt(os_))).astype(np.float32)
