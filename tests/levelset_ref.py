"""The float64 reference of adkf_levelset_pool and the assertions every comparison against it makes.

As believer_ref.py: believer_ref.posterior's mean and latent covariance over the pool, downdated pick by pick, S <- S - S[:, p] S[p, :] /
(S[p, p] + noise), the mean held fixed.  It is CONDITIONED ON THE CALL'S OWN EARLIER PICKS and never compares a whole greedy sequence.
Per step: the float64 score of the chosen kind, the float64 straddle, the classes and hits (scipy's log_ndtr / ndtr in float64).

The bound of a trace entry is built from the project's existing bounds, not tuned on the device: a mean is held to dm = TOL max(1,
max |m|) and a latent variance to dv = TOL os (TOL = 1e-4, tests/test_gpu_predict_pool.py's), so a deviation sigma = sqrt(max(v,
1e-12)) to dsigma = min(dv / (2 sigma_ref), sqrt(dv)) (the derivative of the root, and |sqrt a - sqrt b| <= sqrt |a - b| where that
derivative explodes).  STRADDLE and BOUND are 1-Lipschitz in m and beta-Lipschitz in sigma: dm + beta dsigma.  PROB is the same
through d log Phi / dz = phi / Phi: (phi / Phi)(z) (dm + |z| dsigma) / sigma, plus the evaluation term: 4 x the error that a plain
numpy-float32 evaluation of the same three-piece formula shows against float64 on the same rows, per range of z, in units of
eps32 (1 + z^2) (prob_yardstick)."""
import numpy as np
from scipy.special import log_ndtr, ndtr, ndtri

import believer_ref as B

TOL = B.TOL
STRADDLE, PROB, BOUND = 0, 1, 2
MAXIMIZE = 2
EPS32 = 2.0 ** -24   # the unit roundoff of float32: half an ulp, relative
RANGES = ((0.0, np.inf), (-1.0, 0.0), (-16.0, -1.0), (-np.inf, -16.0))   # lo < z <= hi: z > 0, -1 < z <= 0, -16 < z <= -1, z <= -16


def log_cdf_f32(z):
    """log Phi(z) by the device's three pieces (csrc/levelset_stream.h: ls_log_cdf) in plain numpy float32: every operation rounded."""
    from scipy.special import erfc, erfcx
    z = np.asarray(z, np.float32)
    f, h, c = np.float32, np.float32(0.5), np.float32(0.70710678118654752)
    with np.errstate(all="ignore"):
        right = np.log1p(-h * erfc(np.maximum(z, f(0)) * c).astype(np.float32)).astype(np.float32)
        mid = np.log(h * erfc(-np.clip(z, f(-1), f(0)) * c).astype(np.float32)).astype(np.float32)
        a = -np.minimum(z, f(-1))
        left = (np.log(h * erfcx(a * c).astype(np.float32)).astype(np.float32) - h * a * a).astype(np.float32)
    return np.where(z > 0, right, np.where(z > -1, mid, left)).astype(np.float32)


def prob_f32(mean, var, tau, maximize):
    """The PROB score of a row in plain numpy float32 from its float32 mean and latent variance, as the device forms it: the root of
    the clamped variance, the difference, the quotient, then log_cdf_f32.  Returns (score, z), both float32."""
    mean, var, tau = np.asarray(mean, np.float32), np.asarray(var, np.float32), np.float32(tau)
    sg = np.sqrt(np.maximum(var, np.float32(1e-12)), dtype=np.float32)
    dm = (mean - tau).astype(np.float32)
    z = ((dm if maximize else -dm) / sg).astype(np.float32)
    return log_cdf_f32(z), z


def range_of(z):
    z = np.asarray(z, np.float64)
    return np.where(z > 0, 0, np.where(z > -1, 1, np.where(z > -16, 2, 3)))


def prob_units(got, z32):
    """|got - log Phi(z32)| of float32 results at float32 arguments, in units of eps32 (1 + z^2)."""
    z = np.asarray(z32, np.float32).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - log_ndtr(z)) / (EPS32 * (1.0 + z * z))


def prob_yardstick(z):
    """Per range of z, the worst error of log_cdf_f32 on these rows in units of eps32 (1 + z^2): [4], 0 for a range without rows."""
    z32 = np.asarray(z, np.float32).ravel()
    u, r = prob_units(log_cdf_f32(z32), z32), range_of(z32)
    return np.array([u[r == k].max() if (r == k).any() else 0.0 for k in range(4)])


def phi_over_Phi(z):
    """phi(z) / Phi(z) without underflow."""
    return np.exp(-0.5 * z * z - 0.5 * np.log(2.0 * np.pi) - log_ndtr(z))


def rows_ref(m, v, tau, beta, kind, maximize):
    """score, straddle, class, z and sigma of every row, float64."""
    sg = np.sqrt(np.maximum(v, 1e-12))
    dm = m - tau
    sd = dm if maximize else -dm
    z = sd / sg
    straddle = beta * sg - np.abs(dm)
    if kind == STRADDLE:
        score = straddle
    elif kind == PROB:
        score = log_ndtr(z)
    else:
        score = (m if maximize else -m) + beta * sg
    cls = np.where(straddle > 0, 2, np.where(sd > 0, 0, 1)).astype(np.int8)
    return score, straddle, cls, z, sg


def straddle_f32(mean, var, tau, beta):
    """The straddle as the tile walk forms it, in numpy float32 from float32 mean and latent variance: fmaf(beta, sigma, -|m - tau|),
    the fused product taken in float64 (exact for float32 factors) and rounded once."""
    mean, var = np.asarray(mean, np.float32), np.asarray(var, np.float32)
    sg = np.sqrt(np.maximum(var, np.float32(1e-12)), dtype=np.float32)
    dm = np.abs(mean - np.float32(tau), dtype=np.float32)
    return (np.float64(np.float32(beta)) * sg.astype(np.float64) - dm.astype(np.float64)).astype(np.float32)


def levelset_steps(post, tau, beta, kind, maximize, picks):
    """Per step j a dict(score, straddle, cls, z, sigma, v, delta, delta_straddle, hits, dhits) given picks[0 .. j - 1]; the state stops
    changing at the first pick < 0.  delta: the bound of a float32 score of the kind; delta_straddle: that of the straddle, which
    decides the class; dhits: the bound of hits, the same propagation through d Phi / dz = phi plus the fixed-point rounding and
    the float32 Phi terms (16 ulps of erfcf, the rounding of its argument, the final conversion)."""
    m, S, noise, os_ = post
    S = S.copy()
    tau, beta = float(tau), float(beta)
    dmean, dv = TOL * max(1.0, np.abs(m).max()), TOL * os_
    steps = []
    for p in picks:
        v = S.diagonal().copy()
        score, straddle, cls, z, sg = rows_ref(m, v, tau, beta, kind, maximize)
        dsg = np.minimum(dv / (2.0 * sg), np.sqrt(dv))
        d_lin = dmean + beta * dsg
        dz = (dmean + np.abs(z) * dsg) / sg
        if kind == PROB:
            delta = phi_over_Phi(z) * dz + 4.0 * prob_yardstick(z)[range_of(z)] * EPS32 * (1.0 + z * z)
        else:
            delta = d_lin
        Phi = ndtr(z)
        pdf = np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
        dhits = (np.minimum(pdf * dz, 1.0) + 32 * EPS32 * Phi + 2 * EPS32 * pdf * np.abs(z)).sum() + len(m) * 2.0 ** -32 + 2 * EPS32 * Phi.sum()
        steps.append(dict(score=score, straddle=straddle, cls=cls, z=z, sigma=sg, v=v, delta=delta, delta_straddle=d_lin,
                          hits=Phi.sum(), dhits=dhits))
        if p >= 0:
            S = S - np.outer(S[:, p], S[p, :]) / (S[p, p] + noise)
    return steps


def new_tally():
    """Band rows against rows compared, over a whole test (assert_tally)."""
    return dict(band=0, rows=0)


def assert_tally(tally, cap=0.02):
    assert tally["rows"] > 0 and tally["band"] <= cap * tally["rows"], tally


def check_task(post, tau, beta, kind, maximize, sel_idx, sel_val, sel_mean, sel_var, trace, counts=None, hits=None, excluded=(), tally=None, tag=""):
    """The believer's four assertions on one task (trace, sel_val, near-argmax selection, sel_mean / sel_var) and a fifth: counts[j, c]
    lies between the number of reference rows in class c outside the band |straddle_ref| <= bound and that number plus the band's
    size, and the three counts sum to rows.  hits is held to the propagated bound of levelset_steps.  sel_* [q], trace [q, rows] or
    None, counts [q, 3] or None, hits [q] or None.  Returns the worst trace error / bound seen."""
    m, _, _, os_ = post
    rows = m.shape[0]
    picks = [int(p) for p in sel_idx]
    steps = levelset_steps(post, tau, beta, kind, maximize, picks)
    worst = 0.0
    taken = set(int(e) for e in excluded)
    for j, st in enumerate(steps):
        s64, delta, v, p = st["score"], st["delta"], st["v"], picks[j]
        if trace is not None:                                           # 1
            err = np.abs(trace[j].astype(np.float64) - s64) / delta
            worst = max(worst, float(err.max()))
            assert err.max() <= 1.0, (tag, j, "trace", float(err.max()), int(err.argmax()))
        if counts is not None:                                          # 5
            band = np.abs(st["straddle"]) <= st["delta_straddle"]
            if tally is not None:
                tally["band"] += int(band.sum()); tally["rows"] += rows
            assert int(counts[j].sum()) == rows, (tag, j, "counts do not sum to rows", counts[j].tolist())
            for c in range(3):
                lo = int(((st["cls"] == c) & ~band).sum())
                assert lo <= int(counts[j, c]) <= lo + int(band.sum()), (tag, j, "counts", c, int(counts[j, c]), lo, int(band.sum()))
        if hits is not None:
            assert abs(float(hits[j]) - st["hits"]) <= st["dhits"], (tag, j, "hits", float(hits[j]), st["hits"], st["dhits"])
        ok = np.ones(rows, bool)
        ok[list(taken)] = False
        if p < 0:
            assert not ok.any() or np.isnan(s64[ok]).all(), (tag, j, "a step without a pick although rows are eligible")
            assert np.isneginf(sel_val[j]) and sel_mean[j] == 0 and sel_var[j] == 0, (tag, j)
            continue
        assert ok[p], (tag, j, p, "an excluded or repeated pick")
        assert abs(float(sel_val[j]) - s64[p]) <= delta[p], (tag, j, "sel_val", float(sel_val[j]), s64[p], delta[p])   # 2
        top = int(np.argmax(np.where(ok, s64, -np.inf)))
        assert s64[p] >= s64[top] - (delta[p] + delta[top]), (tag, j, "selection", p, s64[p], top, s64[top], delta[p])   # 3
        assert abs(float(sel_mean[j]) - m[p]) <= TOL * max(1.0, np.abs(m).max()), (tag, j, "sel_mean")           # 4
        assert abs(float(sel_var[j]) - v[p]) <= TOL * os_, (tag, j, "sel_var", float(sel_var[j]), v[p])
        taken.add(p)
    return worst


def hits_from_trace_bound(trace_j):
    """What |hits_j - sum_r exp(trace_j[r])| of a PROB call is held to, derived, not fitted.  hits_j is the 2^-31 fixed-point sum of
    the float32 terms Phi32_r = 0.5 erfcf(-z_r / sqrt 2); trace_j[r] is the float32 log Phi(z_r) of the same float32 z_r.  Counted:
      the fixed point      each term rounded to a multiple of 2^-31: rows 2^-32;
      Phi32                the product z / sqrt 2 (one rounding of the argument: |d Phi| <= phi(z) |z| eps32), erfcf (OpenCL's table allows
                           16 ulps = 32 eps32 relative), the halving (exact);
      exp(trace)           trace carries the absolute error of the float32 evaluation of log Phi at the given z, which is the relative
                           error of its exponential: a^2 / 2 (one rounding, eps32 z^2 / 2), the final difference (one rounding of a
                           value <= 1 + z^2), erfcf / erfcxf (16 ulps: 32 eps32 relative, absolute in the logarithm) and logf / log1pf
                           (4 ulps of a value <= 1 + z^2: 8 eps32 (1 + z^2)): 42 eps32 (1 + z^2) at most;
      the conversion       u64 to double (exact below 2^53) to float: eps32 relative to the sum.
    z is recovered from trace itself (ndtri), which is accurate enough for a bound: on the right, where exp(trace) -> 1, the term
    Phi (1 + z^2) is replaced by the error of the tail, which is below 42 eps32 as well."""
    t = np.asarray(trace_j, np.float64)
    Phi = np.exp(t)
    z = ndtri(np.clip(Phi, 1e-300, 1.0 - 1e-16))
    z = np.where(Phi < 1e-300, -np.sqrt(np.maximum(-2.0 * t, 0.0)), z)   # (far on the left log Phi ~ -z^2 / 2)
    pdf = np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
    rel = np.where(z > 0, 42.0, 42.0 * (1.0 + z * z))
    with np.errstate(all="ignore"):
        per_row = np.nan_to_num(EPS32 * (pdf * np.abs(z) + 32.0 * Phi + rel * Phi), nan=0.0)   # (Phi = 0 far on the left: 0 * inf)
    return t.size * 2.0 ** -32 + per_row.sum() + EPS32 * Phi.sum()
