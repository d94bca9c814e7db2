"""The reference of max-value entropy search (adkf_mes_pool): g(gamma) = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma) with
mpmath at 50 digits - enough for the cancellation of its two terms (each ~gamma^2 / 2) anywhere a float32 gamma can reach in the
tests - and the score of a pool from a posterior mean and latent variance.  Helpers for the tests; not a test module."""
import math

import mpmath as mp
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def mes_term_ref(gamma):
    """g(gamma) as a float; NaN for a NaN or infinite gamma."""
    gamma = float(gamma)
    if not math.isfinite(gamma):
        return float("nan")
    with mp.workdps(50):
        x = mp.mpf(gamma)
        cdf = mp.ncdf(x)
        return float(x * mp.npdf(x) / (2 * cdf) - mp.log(cdf))


def mes_ref(mean, var_latent, ystar_t, maximize, clamp=1e-12):
    """(score [rows], gamma [rows, S]) in float64: score = mean_s g(gamma_s), gamma_s = +-(ystar_t[s] - mean) / sigma,
    sigma = sqrt(max(var_latent, clamp))."""
    mean, var = np.asarray(mean, np.float64), np.asarray(var_latent, np.float64)
    ystar_t = np.asarray(ystar_t, np.float64)
    sigma = np.sqrt(np.maximum(var, clamp))
    diff = ystar_t[None, :] - mean[:, None]
    gamma = (diff if maximize else -diff) / sigma[:, None]
    g = np.array([[mes_term_ref(x) for x in row] for row in gamma], np.float64).reshape(gamma.shape)
    return g.mean(axis=1), gamma


def gamma_weight(gamma):
    """mean_s (1 + gamma_s^2) per row: what the float32 error of a score scales with."""
    return (1.0 + np.asarray(gamma, np.float64) ** 2).mean(axis=1)
