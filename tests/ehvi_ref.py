"""Float64 reference of adkf_ehvi_pool (include/adkf_gp.h): the staircase, the exact two-objective expected hypervolume improvement,
the feasibility weight, their log form, and the bound a float32 score is held to.  Everything minimises: callers negate the mean, the
front column and the reference coordinate of a maximised objective (``to_min``)."""
import math

import numpy as np
from scipy import special as sp

EPS32 = 2.0 ** -24

# The float32 score against the float64 score at the call's own float32 m and v (tests/test_gpu_ehvi_pool.py): each constant is 4
# times the largest ratio that test prints on the MI355X, rounded up to a power of two; the factor 4 is for shapes and seeds the test
# does not visit.  Largest ratios printed per case - label fronts (P, C) = (7, 0), (64, 2), (1, 1), which clean down to 1 to 7 steps,
# then anti-chains whose staircases keep all 64 (C = 2) and all 33 (C = 0) points: linear 0.806, 1.027, 0.664, 0.172, 0.098; log
# 4.093, 3.572, 4.153, 4.014, 3.761.  The log maxima all come from the reference point moved by 25 (pm_log_ei's deep tail); on the
# groups as they are the log ratios stay below 1.2 and with the reference moved by MID_SHIFT below 0.02.  See DESIGN.md.
EVAL_C = 8.0
EVAL_C_LOG = 32.0


def to_min(x, maximize):
    return -np.asarray(x, np.float64) if maximize else np.asarray(x, np.float64)


def staircase(front, ref, maximize=(False, False)):
    """The cleaning rule, point by point: (a [P], b [P]) in the minimisation sense, a ascending and b strictly descending."""
    F = np.asarray(front, np.float64).reshape(-1, 2) * np.array([-1.0 if m else 1.0 for m in maximize])
    r = np.asarray(ref, np.float64) * np.array([-1.0 if m else 1.0 for m in maximize])
    ok = [i for i in range(len(F)) if not np.isnan(F[i]).any() and F[i, 0] < r[0] and F[i, 1] < r[1]]
    keep = []
    for i in ok:
        dominated = False
        for j in ok:
            if j != i and F[j, 0] <= F[i, 0] and F[j, 1] <= F[i, 1] and (F[j, 0] < F[i, 0] or F[j, 1] < F[i, 1] or j < i):
                dominated = True
        if not dominated:
            keep.append(i)
    keep.sort(key=lambda i: F[i, 0])
    S = F[keep].reshape(-1, 2)
    assert (np.diff(S[:, 0]) > 0).all() and (np.diff(S[:, 1]) < 0).all()
    return S[:, 0].copy(), S[:, 1].copy()


def _z(m, s, c):
    with np.errstate(invalid="ignore"):
        return (c - m) / s


def psi(m, s, c):
    """E[(c - y)+], y ~ N(m, s^2); psi(-inf) = 0."""
    if np.isneginf(c):
        return np.zeros_like(np.asarray(m, np.float64))
    z = _z(m, s, c)
    return s * (z * sp.ndtr(z) + np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))


def edge_err(m, s, c):
    """e(c) = s (|z| Phi(z) + phi(z)) (1 + z^2): the rounding of z, of exp(-z^2 / 2) and the cancellation of z Phi + phi; e(-inf) = 0."""
    if np.isneginf(c):
        return np.zeros_like(np.asarray(m, np.float64))
    z = _z(m, s, c)
    return s * (np.abs(z) * sp.ndtr(z) + np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)) * (1.0 + z * z)


def sigma(v):
    return np.sqrt(np.maximum(np.asarray(v, np.float64), 1e-12))


def ehvi(m1, v1, m2, v2, a, b, r1, r2):
    """(EHVI, unit_obj) per row: two objectives over the staircase (a, b) and the reference point (r1, r2), all minimised."""
    m1, m2 = np.asarray(m1, np.float64), np.asarray(m2, np.float64)
    s1, s2 = sigma(v1), sigma(v2)
    P = len(a)
    edges = [-np.inf] + list(a) + [r1]
    second = [r2] + list(b)
    val = np.zeros_like(m1)
    unit = np.zeros_like(m1)
    for i in range(P + 1):
        lo, hi, f2 = psi(m1, s1, edges[i]), psi(m1, s1, edges[i + 1]), psi(m2, s2, second[i])
        val += (hi - lo) * f2
        unit += (edge_err(m1, s1, edges[i + 1]) + edge_err(m1, s1, edges[i])) * f2 + (hi - lo) * edge_err(m2, s2, second[i])
    return val, unit


def ei(m1, v1, r1):
    """(EHVI, unit_obj) of a single objective: psi_1(r1) and e_1(r1)."""
    m1 = np.asarray(m1, np.float64)
    return psi(m1, sigma(v1), r1), edge_err(m1, sigma(v1), r1)


def feasibility(cons):
    """cons: a list of (m, v, thr, geq).  Returns (PoF, log PoF, sum_c (1 + z_c^2)) per row."""
    pof, lp, zz = 1.0, 0.0, 0.0
    for m, v, thr, geq in cons:
        m = np.asarray(m, np.float64)
        z = ((m - thr) if geq else (thr - m)) / sigma(v)
        pof = pof * sp.ndtr(z)
        lp = lp + sp.log_ndtr(z)
        zz = zz + 1.0 + z * z
    return pof, lp, zz


def _mp_log_ehvi(m1, s1, m2, s2, a, b, r1, r2):
    """log EHVI of one row in 60 digits: where float64 underflows."""
    import mpmath as mp

    with mp.workdps(60):
        def f(m, s, c):
            if c == -np.inf:
                return mp.mpf(0)
            z = (mp.mpf(float(c)) - mp.mpf(float(m))) / mp.mpf(float(s))
            return mp.mpf(float(s)) * (z * mp.ncdf(z) + mp.npdf(z))
        edges = [-np.inf] + list(a) + [r1]
        second = [r2] + list(b)
        tot = mp.mpf(0)
        for i in range(len(a) + 1):
            w = f(m1, s1, edges[i + 1]) - f(m1, s1, edges[i])
            tot += w * (f(m2, s2, second[i]) if m2 is not None else 1)
        return float(mp.log(tot)) if tot > 0 else -np.inf


def log_ehvi(m1, v1, m2, v2, a, b, r1, r2, val):
    """log of ``val`` (ehvi's or ei's first result), row by row in multiprecision where float64 has lost it (below 1e-280)."""
    with np.errstate(divide="ignore"):
        out = np.log(np.maximum(val, 0.0))
    s1 = sigma(v1)
    s2 = sigma(v2) if v2 is not None else None
    for r in np.nonzero(~(val > 1e-280) & ~np.isnan(val))[0]:
        out[r] = _mp_log_ehvi(m1[r], s1[r], None if m2 is None else m2[r], None if s2 is None else s2[r], a, b, r1, r2)
    return out


def group_ref(m1, v1, m2, v2, a, b, r1, r2, cons=()):
    """The float64 scores of a group and the bound units.  m2 None: one objective.  Returns dict(lin, log, EHVI, PoF, unit, zz):
    ``lin = EHVI PoF``, ``log = log EHVI + log PoF``, ``unit = unit_obj``, ``zz = sum_c (1 + z_c^2)``."""
    if m2 is None:
        val, unit = ei(m1, v1, r1)
        lval = log_ehvi(np.asarray(m1, np.float64), v1, None, None, (), (), r1, None, val)
    else:
        val, unit = ehvi(m1, v1, m2, v2, a, b, r1, r2)
        lval = log_ehvi(np.asarray(m1, np.float64), v1, np.asarray(m2, np.float64), v2, a, b, r1, r2, val)
    pof, lp, zz = feasibility(cons)
    return dict(lin=val * pof, log=lval + lp, EHVI=val, PoF=pof * np.ones_like(val), unit=unit, zz=zz * np.ones_like(val))


def bound_linear(g):
    return EPS32 * g["PoF"] * (g["unit"] + g["EHVI"] * g["zz"])


def bound_log(g):
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(g["EHVI"] > 0, g["unit"] / g["EHVI"], 0.0)
    return EPS32 * (rel + g["zz"] + 1.0 + np.abs(g["log"]))


def by_quadrature(m1, s1, m2, s2, a, b, r1, r2):
    """One row by one-dimensional quadrature of the normal CDFs: sum_i [int_{a_i}^{a_(i+1)} Phi_1] [int_{-inf}^{b_i} Phi_2], which
    does not use the closed form of psi."""
    from scipy import integrate

    c1 = lambda y: sp.ndtr((y - m1) / s1)
    c2 = lambda y: sp.ndtr((y - m2) / s2)
    edges = [m1 - 40.0 * s1] + list(a) + [r1]
    second = [r2] + list(b)
    tot = 0.0
    for i in range(len(a) + 1):
        lo = min(edges[i], edges[i + 1])
        w = integrate.quad(c1, lo, edges[i + 1], epsabs=1e-13, epsrel=1e-12, limit=200)[0]
        f = integrate.quad(c2, min(m2 - 40.0 * s2, second[i]), second[i], epsabs=1e-13, epsrel=1e-12, limit=200)[0]
        tot += w * f
    return tot


def by_monte_carlo(m1, s1, m2, s2, a, b, r1, r2, n=400000, seed=0):
    """(mean, standard error) of the hypervolume improvement of one sample (y1, y2) over the staircase, by its definition: the area
    of [y, r] minus the part of it the staircase already dominates."""
    g = np.random.default_rng(seed)
    y1, y2 = m1 + s1 * g.standard_normal(n), m2 + s2 * g.standard_normal(n)
    inside = (y1 < r1) & (y2 < r2)
    area = np.where(inside, (r1 - y1) * (r2 - y2), 0.0)
    # the dominated part: the staircase's cells to the upper right of y
    edges = list(a) + [r1]
    dom = np.zeros(n)
    for i in range(len(a)):
        wx = np.clip(edges[i + 1] - np.maximum(edges[i], y1), 0.0, None)
        wy = np.clip(r2 - np.maximum(b[i], y2), 0.0, None)
        dom += wx * wy
    h = np.where(inside, area - dom, 0.0)
    return h.mean(), h.std(ddof=1) / math.sqrt(n)


def make_groups(ys, n_s, P, C, seed, two=True, chain=False):
    """One group per task t of a batch with labels ys [T, ns] (n_s valid each): objectives (t, t + 1 mod T) with mixed senses, the
    front from the two tasks' own support labels (label pairs first, jittered copies of them up to P points), ref their worst value
    plus 0.1 of their range, C constraint tasks (t + 1 + c mod T) with thresholds near the median label, senses alternating.
    Label fronts clean down to a handful of points; ``chain``: the front is an anti-chain of P points instead, spread over the label
    range from (best, worst) to (worst, best) and shuffled - every one of them survives, so the staircase has P steps.
    Returns a dict of host arrays in the layout of adkf_ehvi_pool."""
    g = np.random.default_rng(seed)
    ys = np.asarray(ys, np.float64)
    T = len(n_s)
    obj = np.array([[t, (t + 1) % T if two else -1] for t in range(T)], np.int32)
    obj_max = np.array([[t % 2, (t // 2 + 1) % 2] for t in range(T)], np.int32)
    ref = np.zeros((T, 2), np.float32)
    front = np.zeros((T, P, 2), np.float32) if P > 0 else None
    for t in range(T):
        t1, t2 = t, (t + 1) % T
        n = int(min(n_s[t1], n_s[t2]))
        pts = np.stack([ys[t1, :n], ys[t2, :n]], 1)
        for c in range(2):
            lo, hi = pts[:, c].min(), pts[:, c].max()
            ref[t, c] = lo - 0.1 * (hi - lo) if obj_max[t, c] else hi + 0.1 * (hi - lo)
        if P > 0 and chain:
            u = (np.arange(P) + 0.5) / P
            for c, w in ((0, u), (1, 1.0 - u)):
                lo, hi = pts[:, c].min(), pts[:, c].max()
                best, worst = (hi, lo) if obj_max[t, c] else (lo, hi)
                front[t, :, c] = best + w * (worst - best)
            front[t] = front[t, g.permutation(P)]
        elif P > 0:
            extra = pts[g.integers(n, size=max(P - n, 0))] + 0.05 * g.normal(size=(max(P - n, 0), 2))
            front[t] = np.concatenate([pts[:min(P, n)], extra])[:P]
    out = dict(G=T, P=P, C=C, obj=obj, obj_max=obj_max, ref=ref, front=front, front_n=np.full(T, P, np.int32), con=None, con_thr=None,
               con_geq=None)
    if C > 0:
        out["con"] = np.array([[(t + 1 + c) % T for c in range(C)] for t in range(T)], np.int32)
        out["con_thr"] = np.array([[np.median(ys[(t + 1 + c) % T, :n_s[(t + 1 + c) % T]]) + 0.3 * g.normal() for c in range(C)]
                                   for t in range(T)], np.float32)
        out["con_geq"] = np.array([[(t + c) % 2 for c in range(C)] for t in range(T)], np.int32)
    return out


def score_ref(m, v, grp, g):
    """group_ref of group g of ``grp`` (make_groups' layout) at the means m [T, rows] and latent variances v [T, rows]."""
    t1, t2 = int(grp["obj"][g, 0]), int(grp["obj"][g, 1])
    mx = grp["obj_max"][g] if grp["obj_max"] is not None else (0, 0)
    cons = []
    for c in range(grp["C"]):
        t = int(grp["con"][g, c])
        if t >= 0:
            cons.append((m[t], v[t], float(grp["con_thr"][g, c]), bool(grp["con_geq"][g, c])))
    r1 = float(to_min(grp["ref"][g, 0], mx[0]))
    if t2 < 0:
        return group_ref(to_min(m[t1], mx[0]), v[t1], None, None, (), (), r1, None, cons)
    r2 = float(to_min(grp["ref"][g, 1], mx[1]))
    n = int(grp["front_n"][g]) if grp["P"] > 0 else 0
    a, b = staircase(grp["front"][g, :n] if n > 0 else np.zeros((0, 2)), grp["ref"][g], mx)
    return group_ref(to_min(m[t1], mx[0]), v[t1], to_min(m[t2], mx[1]), v[t2], a, b, r1, r2, cons)


def topk_of(score, k, excluded=()):
    """adkf_predict_pool's selection on a float32 score row: larger first, ties by ascending row; NaN and excluded rows never."""
    score = np.asarray(score, np.float32)
    ok = ~np.isnan(score)
    ok[np.asarray(list(excluded), np.int64)] = False
    cand = np.nonzero(ok)[0]
    order = cand[np.argsort(-score[cand].astype(np.float64), kind="stable")][:k]
    idx = np.full(k, -1, np.int64)
    val = np.full(k, -np.inf, np.float32)
    idx[:order.size] = order
    val[:order.size] = score[order]
    return idx, val
