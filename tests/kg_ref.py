"""The float64 / mpmath reference of adkf_kg_pool: the knowledge gradient for correlated beliefs of a set of lines.

kg_lines is Frazier's sorted algorithm (Frazier, Powell and Dayanik 2009, algorithm 1): the lines by ascending slope, equal slopes
reduced to their largest intercept, the upper envelope by a stack, then the sum over consecutive survivors of
(b_next - b_cur) h(-|c|), h(u) = phi(u) + u Phi(u), c the abscissa where the two cross.  h and log h come from math.erfc where float64
holds them (u > -8) and from mpmath below, so that neither cancels nor underflows; the sum of the logarithms is a log-sum-exp.  The
value is returned with what the evaluation bounds of the device tests are built from:
    plain   |got - ref| <= EVAL_C * eps32 * unit,       unit = max_l |a_l - a*| + max_l |b_l|  (an absolute scale of the line set)
    log     |got - ref| <= EVAL_C_LOG * eps32 * unit,   unit = 1 + c_max^2,  c_max the largest |c| among the terms kept
EVAL_C and EVAL_C_LOG are four times the largest ratio |got - ref| / (eps32 unit) measured on the MI355X against this reference
(tests/test_gpu_kg_pool.py::test_the_envelope_alone prints it), rounded up to a power of two.  The margin of four covers shapes and
seeds that were not measured; the constants are never taken from the device code's output on another run."""
import math

import mpmath as mp
import numpy as np

import believer_ref as B

MAXIMIZE, LOG = 2, 16
TOL = B.TOL
EPS32 = float(np.finfo(np.float32).eps)
CLAMP32 = float(np.float32(1e-12))
EVAL_C = 4.0        # measured: 0.549 (matern, ns = 200, refined; rbf, ns = 32, plain: 0.375); 4 x 0.549 = 2.2 -> 4
EVAL_C_LOG = 16.0   # measured: 3.127 (rbf, ns = 32; matern, ns = 200: 3.033; a float64 task: 1.93); 4 x 3.127 = 12.5 -> 16

mp.mp.dps = 40


def log_h(u):
    """log(phi(u) + u Phi(u)) for u <= 0 (any real u works)."""
    u = float(u)
    if u == -math.inf:
        return -math.inf
    if u > -8.0:
        return math.log(math.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi) + u * 0.5 * math.erfc(-u / math.sqrt(2.0)))
    x = mp.mpf(u)
    return float(mp.log(mp.npdf(x) + x * mp.ncdf(x)))


def kg_lines(a, b, log=False):
    """(value, unit, info) of the lines a_l + b_l Z: value = KG (log: log KG, -inf for one surviving line), unit as in the module's
    docstring for the same form, info = dict(active=[indices in ascending slope], c=[crossings], terms=[log terms])."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    order = sorted(range(len(a)), key=lambda i: (b[i], -a[i], i))
    hull, start = [], []
    for i in order:
        if hull and b[hull[-1]] == b[i]:
            continue   # an equal slope with a smaller or equal intercept
        z = -math.inf
        while hull:
            z = (a[hull[-1]] - a[i]) / (b[i] - b[hull[-1]])
            if z > start[-1]:
                break
            hull.pop(); start.pop()
            z = -math.inf
        hull.append(i); start.append(z if len(hull) > 1 else -math.inf)
    cs = [start[k + 1] for k in range(len(hull) - 1)]
    terms = [math.log(b[hull[k + 1]] - b[hull[k]]) + log_h(-abs(cs[k])) for k in range(len(hull) - 1)]
    info = dict(active=hull, c=cs, terms=terms)
    unit_plain = float(np.abs(a - a.max()).max() + np.abs(b).max())
    if not terms or max(terms) == -math.inf:
        return (-math.inf if log else 0.0), (1.0 if log else unit_plain), info
    if log:
        mx = max(terms)
        val = mx + math.log(sum(math.exp(t - mx) for t in terms))
        keep = [abs(c) for c, t in zip(cs, terms) if t > -math.inf]
        return val, 1.0 + max(keep) ** 2, info
    val = float(sum(mp.e ** mp.mpf(t) for t in terms))
    return val, unit_plain, info


def kg_quad(a, b):
    """E[max_l (a_l + b_l Z)] - max_l a_l by direct quadrature in mpmath (the check of kg_lines; small line sets only)."""
    a = [mp.mpf(float(x)) for x in a]
    b = [mp.mpf(float(x)) for x in b]
    amax = max(a)
    f = lambda z: (max(ai + bi * z for ai, bi in zip(a, b)) - amax) * mp.npdf(z)
    # the integrand has kinks where lines cross: split there
    pts = {mp.mpf(-40), mp.mpf(40)}
    for i in range(len(a)):
        for j in range(i):
            if b[i] != b[j]:
                z = (a[j] - a[i]) / (b[i] - b[j])
                if -40 < z < 40:
                    pts.add(z)
    return float(mp.quad(f, sorted(pts)))


def lines_of_row(mean_r, var_r, cov_r, ref_mean, ref_rows, r, noise, maximize, clamp=CLAMP32):
    """The lines of pool row r as the entry defines them, in float64 from the given numbers: (a [L], b [L]), the own line last.
    ref_rows[j] < 0: a skipped entry; the entry equal to r is skipped for this row."""
    sgn = 1.0 if maximize else -1.0
    vc = max(float(var_r), clamp)
    s = math.sqrt(vc + float(noise))
    a, b = [], []
    for j, p in enumerate(ref_rows):
        if p >= 0 and p != r:
            a.append(sgn * float(ref_mean[j])); b.append(float(cov_r[j]) / s)
    a.append(sgn * float(mean_r)); b.append(vc / s)
    return np.array(a), np.array(b)


def valid_refs(ref_idx_t, rows):
    """The entries of one task as the entry keeps them: the pool row, or -1 for one outside [0, rows) or a repetition."""
    out, seen = [], set()
    for p in (int(x) for x in ref_idx_t):
        ok = 0 <= p < rows and p not in seen
        out.append(p if ok else -1)
        if ok:
            seen.add(p)
    return out


def kg_task(post, ref_idx_t, maximize, log=False):
    """The float64 reference of one task over the whole pool from its float64 posterior post = (m, S, noise, os):
    (score [rows], unit [rows], refs)."""
    m, S, noise, _ = post
    rows = len(m)
    refs = valid_refs(ref_idx_t, rows)
    rm = [m[p] if p >= 0 else 0.0 for p in refs]
    score, unit = np.empty(rows), np.empty(rows)
    for r in range(rows):
        a, b = lines_of_row(m[r], S[r, r], [S[r, p] if p >= 0 else 0.0 for p in refs], rm, refs, r, noise, maximize, clamp=1e-12)
        score[r], unit[r], _ = kg_lines(a, b, log)
    return score, unit, refs


def topk_of(score, k, excluded=()):
    """(idx [k], val [k]) of the unique order on float32 scores: larger first, ties by ascending row, NaN never, -1 / -inf tail."""
    s = np.asarray(score, np.float32)
    ex = set(excluded)
    cand = [r for r in range(len(s)) if s[r] == s[r] and r not in ex]
    cand.sort(key=lambda r: (-float(s[r]), r))
    idx = cand[:k] + [-1] * (k - len(cand[:k]))
    val = [s[r] if r >= 0 else np.float32(-np.inf) for r in idx]
    return np.array(idx, np.int64), np.array(val, np.float32)
