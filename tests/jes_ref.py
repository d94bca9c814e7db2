"""The float64 reference of adkf_jes_pool (joint entropy search, Hvarfner, Hutter and Nardi 2022, the lower bound at q = 1) and the
bound every comparison against it asserts.  Helpers for the tests; not a test module.

The posterior is believer_ref.posterior's / ard_posterior's (the oracle's mean and full latent covariance over the pool, and the
noise); h(gamma) = tau (gamma + tau), tau = phi / Phi, is gibbon_ref.h_ref's 50-digit value.  score_of evaluates the definition of
include/adkf_gp.h from ANY set of inputs - the float64 posterior (the reference), the call's own float32 numbers (the evaluation
check), or perturbed ones (the derived bound):
    d_s = max(v(x*_s), 1e-12) + cond_noise,   v_s = max(v - c_s^2 / d_s, 1e-12),   m_s = m + c_s (f*_s - m(x*_s)) / d_s,
    term_s = log((max(v, 1e-12) + noise) / (v_s + noise)) - log1p(-v_s / (v_s + noise) h(gamma_s)),   score = mean_valid(term_s) / 2.

The bound delta a float32 score is held to, per row, has two parts, as gibbon_ref's:
  derived     the project's posterior bounds |dm| <= 1e-4 max(1, max |m|) on m(x) and m(x*_s), |dv| <= 1e-4 os on v(x) and v(x*_s) and
              |dc| <= 1e-4 os on c_s (believer_ref's and kg_ref's), pushed through the float64 score by evaluating it at the 32 corners
              of the perturbed inputs (a fast float64 h serves both ends of each difference) and taking the largest deviation;
  evaluation  EVAL_C eps32 mean_s (1 + gamma_s^2): the float32 evaluation of the S terms from the call's own float32 mean, variance,
              covariances, opt_mean and opt_var.  EVAL_C is four times the largest ratio measured on the MI355X at the call's own
              numbers (tests/test_gpu_jes_pool.py::test_the_epilogue_alone prints it), rounded up to a power of two."""
import itertools
import math

import mpmath as mp
import numpy as np
import torch

import believer_ref as B
import gibbon_ref as G
from kg_ref import topk_of  # noqa: F401  (prediction's unique order on float32 scores)

MAXIMIZE = 2
TOL = B.TOL
EPS32 = G.EPS32
CLAMP = 1e-12
CLAMP32 = float(np.float32(1e-12))
EVAL_C = 16.0   # measured: 2.049 (a float64 task of the ill-conditioned batch; test_the_epilogue_alone: 1.588, rbf, ns = 32, S = 5); 4 x 2.049 = 8.2 -> 16


def h64(g):
    """h in float64 over an array, for the perturbed evaluations: tau from erfcx on the left (no underflow), from the complement of the
    tail on the right.  NaN for a NaN or infinite gamma."""
    g = torch.as_tensor(np.asarray(g, np.float64))
    left = torch.clamp(g, max=0.0)
    tau_l = math.sqrt(2.0 / math.pi) / torch.special.erfcx(-left / math.sqrt(2.0))
    right = torch.clamp(g, min=0.0)
    tau_r = torch.exp(-0.5 * right * right) / math.sqrt(2.0 * math.pi) / (1.0 - 0.5 * torch.special.erfc(right / math.sqrt(2.0)))
    tau = torch.where(g <= 0.0, tau_l, tau_r)
    h = torch.clamp(tau * (g + tau), 0.0, 1.0)
    h = torch.where(torch.isfinite(g), h, torch.full_like(h, float("nan")))
    return h.numpy()


def valid_samples(opt_idx_t, rows):
    """The samples of one task as the entry keeps them: the pool row, or -1 for one outside [0, rows).  Repetitions stay."""
    return [int(p) if 0 <= int(p) < rows else -1 for p in opt_idx_t]


def score_of(m, v, C, om, ov, fv, valid, noise, cond_noise, maximize, h=G._hrefv, clamp=CLAMP):
    """(score [rows], gamma [rows, S_eff]) from mean m [rows], latent variance v [rows], covariances C [rows, S], and per sample the
    mean om [S] and latent variance ov [S] at its location, its value fv [S] and whether it counts, valid [S].  No valid sample, or a
    non-finite value on a valid one: NaN everywhere.  A row whose own m or v is NaN: NaN."""
    m, v, C, om, ov, fv = (np.asarray(x, np.float64) for x in (m, v, C, om, ov, fv))
    keep = [s for s in range(len(fv)) if valid[s]]
    if not keep or not np.isfinite(fv[keep]).all():
        return np.full(m.shape, np.nan), np.full((len(m), len(keep)), np.nan)
    c, f = C[:, keep], fv[keep]
    d = np.maximum(ov[keep], clamp) + cond_noise
    vc = np.maximum(v, clamp)[:, None]
    vs = np.maximum(v[:, None] - c * c / d, clamp)
    ms = m[:, None] + c * ((f - om[keep]) / d)
    gamma = ((f - ms) if maximize else (ms - f)) / np.sqrt(vs)
    term = np.log((vc + noise) / (vs + noise)) - np.log1p(-(vs / (vs + noise)) * h(gamma))
    score = 0.5 * term.mean(axis=1)
    score[np.isnan(m) | np.isnan(v)] = np.nan
    return score, gamma


_ref_cache = {}


def jes_task(post, opt_idx_t, opt_val_t, cond_noise, maximize, fast=False):
    """The float64 reference of one task over the whole pool from its float64 posterior post = (m, S, noise, os):
    (score [rows], delta [rows], gamma [rows, S_eff], valid).  Kept per input: the comparisons of one problem share the mpmath values.
    fast: h64 in the place of the 50-digit h (for a look at delta alone)."""
    m, S, noise, os_ = post
    rows = len(m)
    valid = valid_samples(opt_idx_t, rows)
    fv = np.asarray(opt_val_t, np.float64)
    key = (m.tobytes(), S.diagonal().tobytes(), tuple(valid), fv.tobytes(), float(cond_noise), bool(maximize), float(noise), bool(fast))
    if key in _ref_cache:
        return _ref_cache[key]
    v = S.diagonal().copy()
    ok = [p >= 0 for p in valid]
    C = np.stack([S[:, p] if p >= 0 else np.zeros(rows) for p in valid], axis=1)
    om = np.array([m[p] if p >= 0 else 0.0 for p in valid])
    ov = np.array([v[p] if p >= 0 else 0.0 for p in valid])
    score, gamma = score_of(m, v, C, om, ov, fv, ok, noise, cond_noise, maximize, h=h64 if fast else G._hrefv)
    if not np.isfinite(score).any():
        out = (score, np.zeros(rows), gamma, valid)
        _ref_cache[key] = out
        return out
    evaluation = EVAL_C * EPS32 * G.gamma_weight(gamma)
    dm, dv, dc = TOL * max(1.0, float(np.abs(m).max())), TOL * os_, TOL * os_
    mid = score_of(m, v, C, om, ov, fv, ok, noise, cond_noise, maximize, h=h64)[0]
    derived = np.zeros(rows)
    for s1, s2, s3, s4, s5 in itertools.product((-1, 1), repeat=5):
        dev = score_of(m + s1 * dm, v + s2 * dv, C + s3 * dc, om + s4 * dm, ov + s5 * dv, fv, ok, noise, cond_noise, maximize, h=h64)[0]
        derived = np.fmax(derived, np.abs(dev - mid))
    out = (score, derived + evaluation, gamma, valid)
    _ref_cache[key] = out
    return out


def term_by_quadrature(m, v, c, om, ov, f, noise, cond_noise, maximize):
    """term_s of one row and one sample from the definition, by brute force in mpmath: the latent value at x given f(x*_s) = f*_s under
    the noise variance cond_noise is N(m_s, v_s); its density truncated at the sampled optimum (f <= f*_s for a maximum, >= for a
    minimum) has variance V by 1-D quadrature, the observation there V + noise, and the term is log((max(v, 1e-12) + noise) / (V + noise)):
    twice the difference of the entropies of two Gaussians with those variances."""
    with mp.workdps(25):
        m, v, c, om, ov, f, noise, cond_noise = (mp.mpf(float(x)) for x in (m, v, c, om, ov, f, noise, cond_noise))
        d = max(ov, mp.mpf(CLAMP)) + cond_noise
        vs = max(v - c * c / d, mp.mpf(CLAMP))
        ms = m + c * (f - om) / d
        sd = mp.sqrt(vs)
        dens = lambda x: mp.npdf(x, ms, sd)
        lo, hi = (ms - 40 * sd, f) if maximize else (f, ms + 40 * sd)
        if lo >= hi:   # the truncation point is more than 40 deviations out on the empty side
            lo, hi = (f - 40 * sd, f) if maximize else (f, f + 40 * sd)
        pts = [lo, hi] if not (lo < ms < hi) else [lo, ms, hi]
        z = mp.quad(dens, pts)
        e1 = mp.quad(lambda x: x * dens(x), pts) / z
        V = mp.quad(lambda x: (x - e1) ** 2 * dens(x), pts) / z
        return float(mp.log((max(v, mp.mpf(CLAMP)) + noise) / (V + noise)))


def samples_for(post, S, rows, maximize, seed, messy=False):
    """Optimum samples of one task for the tests: locations among the rows of best float64 posterior mean in the call's sense and a few
    random rows, values f*_s = m(x*_s) + c_s sqrt(v(x*_s) + 0.05 os) beyond the mean there (mirrored for minimisation), c_s spread over
    [0.2, 2.5].  messy: a -1, a row outside the pool and a repetition (with another value) among them when there is room."""
    m, Sg, _, os_ = post
    g = np.random.default_rng(seed)
    order = np.argsort(-m if maximize else m, kind="stable")[:S].tolist()
    order += g.integers(0, rows, S - len(order)).tolist()
    for j in range(2, S, 3):
        order[j] = int(g.integers(0, rows))
    c = np.linspace(0.2, 2.5, S) if S > 1 else np.array([1.0])
    idx = np.array(order, np.int64)
    v = np.maximum(Sg.diagonal()[idx], 0.0)
    val = m[idx] + (1.0 if maximize else -1.0) * c * np.sqrt(v + 0.05 * os_)
    if messy and S >= 5:
        idx[1] = -1
        idx[3] = rows + 7
        idx[4] = idx[0]
    return idx, val.astype(np.float32)


def distinct_samples(post, S, rows, maximize, seed):
    """samples_for on duplicate-free locations (S <= rows): what kg_pool(ref_idx=opt_idx) reports the covariances of."""
    m, Sg, _, os_ = post
    g = np.random.default_rng(seed)
    best = np.argsort(-m if maximize else m, kind="stable")[:max(1, S // 2)].tolist()
    rest = [int(r) for r in g.permutation(rows) if int(r) not in set(best)]
    idx = np.array((best + rest)[:S], np.int64)
    c = np.linspace(0.2, 2.5, S) if S > 1 else np.array([1.0])
    v = np.maximum(Sg.diagonal()[idx], 0.0)
    val = m[idx] + (1.0 if maximize else -1.0) * c * np.sqrt(v + 0.05 * os_)
    return idx, val.astype(np.float32)


# ---- the problems of tests/test_gpu_jes_pool.py::test_against_the_reference, built on the host so that tests/test_jes_pool_cpu.py can
# look at their bounds first: (kernel, n_s, d, rows, S, maximize) - ns in {1, 32, 200} (200: the refined kind) with one ragged case, d in
# {3, 16}, rows in {1, 63, 65, 200} (a partial tile, one past the tile edge, several tiles), S in {1, 5, 64}, both senses
CASES = [
    ("rbf", [32, 29, 21], 3, 200, 5, True),
    ("matern", [32, 32], 16, 65, 64, False),
    ("rbf", [200, 197], 16, 63, 5, False),
    ("matern", [200, 133], 16, 200, 1, True),
    ("matern", [1, 1], 3, 65, 5, True),
    ("rbf", [1, 1], 16, 1, 1, False),
    ("matern", [32, 29], 16, 1, 64, True),
    ("rbf", [200, 197], 16, 65, 64, True),
]


def problem(n_s, d, rows, seed):
    """A support-only problem with phi GIVEN, not fitted, on the host: (Zs [T, ns, d], ys [T, ns], X [rows, d], phi [T, 3]) float32.
    Features and pool are draws of one linear map of standard normals, y = sin(sum of the first features) + noise; raw noise from -1
    to -3 (noise >= 0.048 >= 1e-2 os), raw outputscale from 0.3 to 0 and the median distance of the task's support rows as its
    lengthscale (1 for a single row)."""
    T, ns = len(n_s), max(n_s)
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(d, d, generator=g) / math.sqrt(d)
    Zs = (torch.randn(T, ns, d, generator=g) @ W).float()
    ys = (torch.sin(Zs[..., :min(d, 4)].sum(-1)) + 0.1 * torch.randn(T, ns, generator=g)).float()
    X = (torch.randn(rows, d, generator=g) @ W).float()
    phi = torch.empty(T, 3)
    phi[:, 0] = torch.linspace(-1.0, -3.0, T)
    phi[:, 1] = torch.linspace(0.3, 0.0, T)
    for t, n in enumerate(n_s):
        ls = float(torch.pdist(Zs[t, :n].double()).median()) if n > 1 else 1.0
        phi[t, 2] = math.log(math.expm1(ls))
    return Zs, ys, X, phi.float()
