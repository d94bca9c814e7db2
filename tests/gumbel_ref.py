"""Float64 reference of Gumbel max-value sampling (adkf_gumbel_pool; Wang & Jegelka 2017, section 3.1): the quartiles of
Pr[max_i h_i < z] = prod_i Phi((z - mu_i) / sigma_i) by bisection to convergence, the Gumbel fitted to them, and its draws."""
import numpy as np
from scipy.special import log_ndtr, ndtri

LOG_Q = (np.log(0.25), np.log(0.5), np.log(0.75))
DENOM = np.log(np.log(4.0)) - np.log(np.log(4.0 / 3.0))
LOGLOG2 = np.log(np.log(2.0))
U_MIN = 2.0 ** -24


def kappa(rows):
    return max(1.0, float(ndtri(1.0 - 0.25 / rows)))


def bracket(mu, sigma):
    """[lo, hi] that holds the three quartiles: log P(lo) <= log Phi(-1) < log 0.25, 1 - P(hi) <= rows (1 - Phi(kappa)) <= 0.25"""
    mu, sigma = np.asarray(mu, np.float64), np.asarray(sigma, np.float64)
    return float((mu - sigma).max()), float((mu + kappa(mu.size) * sigma).max())


def log_prob(z, mu, sigma):
    return float(log_ndtr((z - np.asarray(mu, np.float64)) / np.asarray(sigma, np.float64)).sum())


def quartiles_exact(mu, sigma):
    """(q25, q50, q75) of the maximum of independent N(mu_i, sigma_i^2): bisection on sum log_ndtr inside the bracket, to 1e-13"""
    mu, sigma = np.asarray(mu, np.float64), np.asarray(sigma, np.float64)
    lo0, hi0 = bracket(mu, sigma)
    out = []
    for lq in LOG_Q:
        lo, hi = lo0, hi0
        assert log_prob(lo, mu, sigma) <= lq <= log_prob(hi, mu, sigma) + 1e-12, (lo, hi, lq)
        while hi - lo > 1e-13 * max(1.0, abs(lo), abs(hi)):
            mid = 0.5 * (lo + hi)
            if log_prob(mid, mu, sigma) < lq:
                lo = mid
            else:
                hi = mid
        out.append(0.5 * (lo + hi))
    return np.array(out)


def gumbel_fit(q):
    """(a, b) of the Gumbel exp(-exp(-(z - a) / b)) through the quartiles q = (q25, q50, q75)"""
    b = (q[2] - q[0]) / DENOM
    return q[1] + b * LOGLOG2, b


def samples(a, b, u):
    u = np.clip(np.asarray(u, np.float64), U_MIN, 1.0 - U_MIN)
    return a - b * np.log(-np.log(u))
