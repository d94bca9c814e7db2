"""GPU: knowledge-gradient selection over a shared pool (adkf_kg_pool / gp_ops.kg_pool) - the envelope alone against the
float64 / mpmath reference of kg_ref.py at the call's own float32 mean, variance, cov and ref_mean; cov and ref_mean against the
float64 posterior; the plain score end to end with a bound derived from the posterior bounds; every task kind (plain, two panels,
refined, global slots, float64, ARD, M = 1 and 64, tiny pools, more tasks than workgroups); the bitwise properties of the call; log KG
against KG and on the underflow case it exists for; the batched BO loop."""
import math

import numpy as np
import pytest
import torch

import believer_ref as B
import kg_ref as R
import test_gpu_believer_pool as BV
import test_gpu_believer_pool_ard as BVA
import test_gpu_log_ei as L
import test_gpu_predict_marginal as M_
import test_gpu_predict_pool as P
from test_believer_pool_ard_cpu import ard_posterior

pytestmark = pytest.mark.gpu

EPS32 = R.EPS32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, c):
    return torch.equal(_bits(a), _bits(c))


def _noise32(phi, T):
    from oracle import gp_oracle as O

    return [float(np.float32(float(O.transform_phi(phi[t].double().cpu())[0]))) for t in range(T)]


def _ref_at_inputs(mean_t, var_t, cov_t, rmean_t, refs, noise, maximize, log):
    """The reference of one task evaluated at the call's own float32 numbers: (ref [rows], unit [rows])."""
    rows = len(mean_t)
    ref, unit = np.empty(rows), np.empty(rows)
    for r in range(rows):
        a, b = R.lines_of_row(mean_t[r], var_t[r], cov_t[r], rmean_t, refs, r, noise, maximize)
        ref[r], unit[r], _ = R.kg_lines(a, b, log)
    return ref, unit


def _eval_check(got, ref, unit, const, tag):
    """|got - ref| <= const eps32 unit on every finite row, -inf exactly where the reference is; returns the largest ratio."""
    got = got.astype(np.float64)
    inf = np.isneginf(ref)
    assert np.array_equal(inf, np.isneginf(got)), (tag, "the rows with one surviving line")
    assert np.isfinite(got[~inf]).all(), tag
    ratio = np.abs(got[~inf] - ref[~inf]) / (EPS32 * unit[~inf])
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{tag}: worst |got - ref| / (eps32 unit) = {worst:.3f} over {ratio.size} rows")
    assert worst <= const, (tag, worst)
    return worst


@pytest.mark.parametrize("kernel,ns,d", L.SHAPES)
def test_the_envelope_alone(dev, kernel, ns, d):
    """score against the reference at the call's OWN float32 mean and latent variance (predict_pool(latent=True) on the same batch:
    the same tile arithmetic), cov, ref_mean and noise, every row compared:
        KG      |got - ref| <= EVAL_C eps32 (max_l |a_l - a*| + max_l |b_l|)
        log KG  |got - ref| <= EVAL_C_LOG eps32 (1 + c_max^2)
    The constants are 4 x the largest ratio this test has printed on the MI355X, rounded up to a power of two (kg_ref.py).  The pool
    holds task 0's support rows: small variances, steep crossings."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    T, ROWS = L.T, L.ROWS
    pp = gp_ops.predict_pool(b, phi, Xc, latent=True)
    gp_ops.check_info(pp["info"])
    mean, var = pp["mean"].cpu().numpy(), pp["var"].cpu().numpy()
    noise = _noise32(phi, T)
    compared = 0
    worst = {False: 0.0, True: 0.0}
    for maximize in (False, True):
        first = gp_ops.kg_pool(b, phi, Xc, n_refs=16, maximize=maximize, want_cov=True)
        gp_ops.check_info(first["info"])
        ref_idx = first["ref_idx"]
        for log in (False, True):
            out = first if not log else gp_ops.kg_pool(b, phi, Xc, ref_idx=ref_idx, maximize=maximize, log=True, want_cov=True)
            assert _same(out["cov"], first["cov"]) and _same(out["ref_mean"], first["ref_mean"])
            got, cov, rmean = out["score"].cpu().numpy(), out["cov"].cpu().numpy(), out["ref_mean"].cpu().numpy()
            for t in range(T):
                refs = R.valid_refs(ref_idx[t].tolist(), ROWS)
                assert min(refs) >= 0
                ref, unit = _ref_at_inputs(mean[t], var[t], cov[t], rmean[t], refs, noise[t], maximize, log)
                w = _eval_check(got[t], ref, unit, R.EVAL_C_LOG if log else R.EVAL_C, (kernel, "max" if maximize else "min", "log" if log else "plain", t))
                worst[log] = max(worst[log], w)
                compared += ref.size
                if not log:
                    assert (got[t] >= 0).all()
    print(f"{kernel} ns {ns}: worst ratio plain {worst[False]:.3f} (EVAL_C {R.EVAL_C}), log {worst[True]:.3f} (EVAL_C_LOG {R.EVAL_C_LOG})")
    assert compared == 4 * T * ROWS   # no row was left out


_posts = {}


def _post_of(b, phi, Zs, ys, n_s, X, ard=False):
    """The float64 posterior of every task over the pool, once per problem (the problems are shared and left unchanged)."""
    key = (b.kernel, tuple(n_s), tuple(X.shape), ard, float(X.double().sum()), float(phi.double().sum()), float(ys.double().sum()))
    if key not in _posts:
        Xh, ph = X.cpu().numpy(), phi.cpu().numpy()
        _posts[key] = [(ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], Xh, ph[t], b.kernel) if ard else
                        B.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], Xh, ph[t], b.kernel)) for t in range(len(n_s))]
    return _posts[key]


def _refs_for(posts, M, rows, maximize, seed):
    """Reference rows per task: the rows of best float64 posterior mean in the call's sense, every third one replaced by a random row, a
    -1 and a repetition among them when there is room."""
    g = np.random.default_rng(seed)
    out = []
    for m, _, _, _ in posts:
        order = np.argsort(-m if maximize else m, kind="stable")[:M].tolist()
        order += g.integers(0, rows, M - len(order)).tolist()
        for j in range(2, M, 3):
            order[j] = int(g.integers(0, rows))
        if M >= 6:
            order[4] = -1
            order[5] = order[0]
        out.append(order)
    return np.array(out, np.int64)


def _check_against_posterior(out, posts, ref_idx, maximize, tag, tasks=None):
    """Tests 2 and 3 of the issue on the tasks given (all by default): cov and ref_mean within the project's posterior bounds,
    |dcov| <= TOL os and |dm| <= TOL max(1, max |m|); the plain score within
        2 dm + sqrt(2 / pi) max_l db_l + EVAL_C eps32 unit,   db_l <= (TOL os / s) (1 + max_l |b_l| / (2 s)),
    because E[max_l (a_l + b_l Z)] is 1-Lipschitz in a and E|Z|-Lipschitz in b (sup norms), max_l a_l is 1-Lipschitz in a, and
    b = cov / s with s = sqrt(vc + noise), |dcov|, |dv| <= TOL os, |ds| <= |dv| / (2 s)."""
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    score, cov, rmean = out["score"].cpu().numpy(), out["cov"].cpu().numpy(), out["ref_mean"].cpu().numpy()
    worst = 0.0
    for t in (range(len(posts)) if tasks is None else tasks):
        m, S, noise, os_ = posts[t]
        rows = len(m)
        refs = R.valid_refs(ref_idx[t].tolist(), rows)
        dm = B.TOL * max(1.0, float(np.abs(m).max()))
        for j, p in enumerate(refs):
            if p < 0:
                assert (cov[t, :, j] == 0).all() and rmean[t, j] == 0, (tag, t, j)
            else:
                assert np.abs(cov[t, :, j] - S[:, p]).max() <= B.TOL * os_, (tag, t, j, float(np.abs(cov[t, :, j] - S[:, p]).max()))
                assert abs(rmean[t, j] - m[p]) <= dm, (tag, t, j)
        rm = [m[p] if p >= 0 else 0.0 for p in refs]
        for r in range(rows):
            a, bl = R.lines_of_row(m[r], S[r, r], [S[r, p] if p >= 0 else 0.0 for p in refs], rm, refs, r, noise, maximize, clamp=1e-12)
            ref, unit, _ = R.kg_lines(a, bl)
            s = math.sqrt(max(S[r, r], 1e-12) + noise)
            db = (B.TOL * os_ / s) * (1.0 + float(np.abs(bl).max()) / (2.0 * s))
            bound = 2.0 * dm + math.sqrt(2.0 / math.pi) * db + R.EVAL_C * EPS32 * unit
            err = abs(float(score[t, r]) - ref)
            worst = max(worst, err / bound)
            assert err <= bound, (tag, t, r, err, bound)
        assert (score[t] >= 0).all(), (tag, t)
    print(f"{tag}: worst end-to-end error / bound {worst:.3f}")


CASES = [  # (kernel, n_s, d, rows, M): the shapes of test_gpu_gibbon_pool.CASES
    ("matern", [48, 45, 31], 16, 300, 16),       # plain, one panel
    ("rbf", [128, 125, 85], 64, 37, 7),          # two panels, one partial tile: rows < 64
    ("rbf", [200, 197, 133], 64, 333, 32),       # refined, LDS tiles
    ("matern", [1024, 700], 12, 130, 8),         # global slots
    ("rbf", [32, 29, 21], 8, 200, 64),           # the full reference panel
    ("matern", [48, 45, 31], 16, 300, 1),        # one reference row
]


@pytest.mark.parametrize("kernel,n_s,d,rows,M", CASES)
def test_against_the_posterior(dev, kernel, n_s, d, rows, M):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    for maximize in ((False, True) if max(n_s) <= 200 else (False,)):
        ref_idx = _refs_for(posts, M, rows, maximize, 7 + M)
        out = gp_ops.kg_pool(b, phi, X, ref_idx=torch.from_numpy(ref_idx).to(dev), maximize=maximize, want_cov=True)
        _check_against_posterior(out, posts, ref_idx, maximize, (kernel, max(n_s), M, maximize))
        if M == 1:   # the reference row itself has its own line only
            lg = gp_ops.kg_pool(b, phi, X, ref_idx=torch.from_numpy(ref_idx).to(dev), maximize=maximize, log=True)["score"].cpu().numpy()
            for t in range(b.T):
                assert out["score"][t, ref_idx[t, 0]] == 0 and np.isneginf(lg[t, ref_idx[t, 0]]) and np.isfinite(np.delete(lg[t], ref_idx[t, 0])).all()


def test_ard(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, M = "matern", [48, 45, 31], 12, 300, 16
    b, phi, Zs, ys, n_s, X, _ = BVA._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    posts = _post_of(b, phi, Zs, ys, n_s, X, ard=True)
    for maximize in (False, True):
        ref_idx = _refs_for(posts, M, rows, maximize, 3)
        out = gp_ops.kg_pool(b, phi, X, ref_idx=torch.from_numpy(ref_idx).to(dev), maximize=maximize, want_cov=True)
        _check_against_posterior(out, posts, ref_idx, maximize, ("ard", maximize))


def _ill(dev):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, _ = P._ill_batch(dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.cat([P._pool(130, 2, 3), b.Z_s[1, :5].cpu()]).to(dev)
    return b, phi, Zs, ys, n_s, X


def _kinds(b):
    """Which walk each task of a fitted batch takes (0 plain, 1 refined, 2 float64), from its scalars, as _ill_batch asserts it."""
    torch.cuda.synchronize()
    return [M_._path(sc) for sc in M_._scalars(b)]


def test_a_float64_task_beside_float32_ones(dev):
    """test_gpu_predict_pool._ill_batch: task 1 takes the float64 walk (asserted there from the fitted scalars; the kinds are printed).
    cov and ref_mean of EVERY task against the float64 posterior and the plain score of every task end to end, the flagged ones
    included (k_kg_refs' float64 solve, W64 and bv64_c0 have no other independent reference); then the envelope of every flagged
    task against the reference at the call's own numbers, as test_the_envelope_alone, in both forms."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X = _ill(dev)
    kinds = _kinds(b)
    rows = X.shape[0]
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    pp = gp_ops.predict_pool(b, phi, X, latent=True)
    mean, var = pp["mean"].cpu().numpy(), pp["var"].cpu().numpy()
    noise = _noise32(phi, b.T)
    for maximize in (False, True):
        ref_idx = _refs_for(posts, 9, rows, maximize, 21)
        ri = torch.from_numpy(ref_idx).to(dev)
        out = gp_ops.kg_pool(b, phi, X, ref_idx=ri, maximize=maximize, want_cov=True)
        _check_against_posterior(out, posts, ref_idx, maximize, ("mixed", maximize))
        lg = gp_ops.kg_pool(b, phi, X, ref_idx=ri, maximize=maximize, log=True, want_cov=True)
        cov, rmean = out["cov"].cpu().numpy(), out["ref_mean"].cpu().numpy()
        flagged = [t for t, kd in enumerate(kinds) if kd == 2]
        assert 1 in flagged
        for t in flagged:
            refs = R.valid_refs(ref_idx[t].tolist(), rows)
            for log, o in ((False, out), (True, lg)):
                ref, unit = _ref_at_inputs(mean[t], var[t], cov[t], rmean[t], refs, noise[t], maximize, log)
                _eval_check(o["score"][t].cpu().numpy(), ref, unit, R.EVAL_C_LOG if log else R.EVAL_C, ("float64 task", t, maximize, log))
    b.flags = 0


def test_tiny_pools(dev):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, "matern", [48, 45, 31], 16, 300, 548)
    X5 = X[:5].contiguous()
    posts = _post_of(b, phi, Zs, ys, n_s, X5)
    ref_idx = np.array([[0, 2, 4, 9]] * b.T, np.int64)   # 9: outside this pool, skipped
    out = gp_ops.kg_pool(b, phi, X5, ref_idx=torch.from_numpy(ref_idx).to(dev), want_cov=True, topk=8)
    _check_against_posterior(out, posts, ref_idx, False, "rows = 5")
    assert bool((out["top_idx"][:, 5:] == -1).all()) and bool(torch.isneginf(out["top_val"][:, 5:]).all()) and bool((out["top_idx"][:, :5] >= 0).all())
    # one row: it can only refer to itself, so it has its own line only
    one = gp_ops.kg_pool(b, phi, X[:1].contiguous(), ref_idx=torch.zeros(b.T, 3, dtype=torch.int64, device=dev), want_cov=True, topk=2)
    assert bool((one["score"] == 0).all()) and bool((one["top_idx"] == torch.tensor([0, -1], device=dev)).all())
    assert bool((one["cov"][:, 0, 0] > 0).all()) and bool((one["cov"][:, 0, 1:] == 0).all())
    lg = gp_ops.kg_pool(b, phi, X[:1].contiguous(), ref_idx=torch.zeros(b.T, 3, dtype=torch.int64, device=dev), log=True, topk=1)
    assert bool(torch.isneginf(lg["score"]).all()) and bool((lg["top_idx"] == 0).all()) and bool(torch.isneginf(lg["top_val"]).all())
    # no row
    none = gp_ops.kg_pool(b, phi, X[:0].contiguous(), ref_idx=torch.zeros(b.T, 3, dtype=torch.int64, device=dev), topk=2, want_cov=True)
    assert none["score"].shape == (b.T, 0) and bool((none["top_idx"] == -1).all()) and bool((none["ref_mean"] == 0).all())


def test_more_tasks_than_workgroups(dev):
    """T = 300 tiny tasks over two tiles, one partial: the score of every task end to end, and three tasks alone are the tasks in the batch."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, M = 300, 8, 4, 70, 3
    g = torch.Generator().manual_seed(77)
    Zs, ys, _ = M_._features(T, ns, [0] * T, d, 77, True)
    n_s = [int(x) for x in torch.randint(3, ns + 1, (T,), generator=g)]
    n_s[0] = ns
    b = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.empty(T, 4, device=dev), "matern", n_s=torch.tensor(n_s, dtype=torch.int32))
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    phi = phi0.clone()
    phi[:, 0] = torch.linspace(-1.0, -3.0, T, device=dev)
    phi[:, 1] = 0.3
    X = P._pool(rows, d, 78).to(dev)
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    ref_idx = _refs_for(posts, M, rows, False, 5)
    ri = torch.from_numpy(ref_idx).to(dev)
    out = gp_ops.kg_pool(b, phi, X, ref_idx=ri, want_cov=True, topk=4)
    _check_against_posterior(out, posts, ref_idx, False, "T300")
    for t in (0, 151, 299):
        b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), "matern",
                            n_s=torch.tensor([n_s[t]], dtype=torch.int32))
        o1 = gp_ops.kg_pool(b1, phi[t:t + 1].contiguous(), X, ref_idx=ri[t:t + 1].contiguous(), want_cov=True, topk=4)
        for name in ("score", "cov", "ref_mean", "top_val"):
            assert _same(o1[name][0], out[name][t]), (name, t)
        assert torch.equal(o1["top_idx"][0], out["top_idx"][t])


def test_bitwise_properties(dev):
    """Two runs are equal; a task alone is the task in a batch; top_idx / top_val are the sort of score under the unique order with the
    exclusions applied; the score of a row does not depend on k; KG >= 0 - on the plain and refined float32 walks, and on the float64
    walk beside them.  A NaN score is never selected: test_a_nan_score_is_never_selected."""
    from adkf_ift_amd import gp_ops

    for kernel, n_s, d, rows, M in (CASES[0], CASES[2]):
        b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
        posts = _post_of(b, phi, Zs, ys, n_s, X)
        ri = torch.from_numpy(_refs_for(posts, M, rows, True, 7 + M)).to(dev)
        lists = [[0, 7], [], [3]]
        for log in (False, True):
            kw = dict(ref_idx=ri, maximize=True, log=log, want_cov=True)
            first = gp_ops.kg_pool(b, phi, X, topk=8, exclude=lists, **kw)
            again = gp_ops.kg_pool(b, phi, X, topk=8, exclude=lists, **kw)
            for name in ("score", "cov", "ref_mean", "top_val"):
                assert _same(first[name], again[name]), name
            assert torch.equal(first["top_idx"], again["top_idx"])
            for k in (0, 1, 64):
                other = gp_ops.kg_pool(b, phi, X, topk=k, exclude=lists, **kw)
                assert _same(other["score"], first["score"]) and _same(other["cov"], first["cov"]), k
            blind = gp_ops.kg_pool(b, phi, X, topk=8, exclude=lists, ref_idx=ri, maximize=True, log=log, want_score=False)
            assert blind["score"] is None and torch.equal(blind["top_idx"], first["top_idx"]) and _same(blind["top_val"], first["top_val"])
            score = first["score"].cpu().numpy()
            if not log:
                assert (score >= 0).all()
            for t in range(b.T):
                wi, wv = R.topk_of(score[t], 8, lists[t])
                assert np.array_equal(first["top_idx"][t].cpu().numpy(), wi) and np.array_equal(first["top_val"][t].cpu().numpy().view(np.int32), wv.view(np.int32))
                b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), kernel,
                                    n_s=torch.tensor([n_s[t]], dtype=torch.int32))
                o1 = gp_ops.kg_pool(b1, phi[t:t + 1].contiguous(), X, topk=8, exclude=[lists[t]], ref_idx=ri[t:t + 1].contiguous(), maximize=True,
                                    log=log, want_cov=True)
                for name in ("score", "cov", "ref_mean", "top_val"):
                    assert _same(o1[name][0], first[name][t]), (name, t, log)
                assert torch.equal(o1["top_idx"][0], first["top_idx"][t])
    b, phi, Zs, ys, n_s, X = _ill(dev)                       # the float64 walk (task 1) beside float32 ones
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    ri = torch.from_numpy(_refs_for(posts, 9, X.shape[0], False, 21)).to(dev)
    for log in (False, True):
        first = gp_ops.kg_pool(b, phi, X, ref_idx=ri, log=log, topk=8, want_cov=True)
        again = gp_ops.kg_pool(b, phi, X, ref_idx=ri, log=log, topk=8, want_cov=True)
        for name in ("score", "cov", "ref_mean", "top_val"):
            assert _same(first[name], again[name]), name
        score = first["score"].cpu().numpy()
        for t in range(b.T):
            wi, wv = R.topk_of(score[t], 8)
            assert np.array_equal(first["top_idx"][t].cpu().numpy(), wi), (t, log)
        if not log:
            assert (score >= 0).all()
    b1 = gp_ops.GPBatch(b.Z_s[1:2].contiguous(), b.y_s[1:2].contiguous(), b.priors[1:2].contiguous(), b.kernel,
                        n_s=torch.tensor([n_s[1]], dtype=torch.int32))
    o1 = gp_ops.kg_pool(b1, phi[1:2].contiguous(), X, ref_idx=ri[1:2].contiguous(), topk=8, want_cov=True)
    b.flags = 0
    full = gp_ops.kg_pool(b, phi, X, ref_idx=ri, topk=8, want_cov=True)   # (both evaluate at phi: no state of a fit is reused)
    for name in ("score", "cov", "ref_mean", "top_val"):
        assert _same(o1[name][0], full[name][1]), name
    assert torch.equal(o1["top_idx"][0], full["top_idx"][1])


def test_a_nan_score_is_never_selected(dev):
    """A pool row whose mean or variance is NaN scores NaN (not the finite score its lines would give once fmaxf / fminf have dropped
    the NaN ones) and is never selected; every other row keeps its bits.  Tile walk: an infinite feature under Matern - the squared
    distance to the support rows on the far side is +inf, which the clamp of the distance keeps, and kappa = inf * 0 = NaN.  Float64
    walk: a NaN feature, which nothing absorbs there (the float32 tile would: fmaxf(NaN, 0) = 0)."""
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, M = CASES[0]
    assert kernel == "matern"
    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    ri = torch.from_numpy(_refs_for(posts, M, rows, True, 7 + M)).to(dev)
    bad = next(r for r in range(70, rows) if r not in set(ri.flatten().tolist()))   # in the second tile, not a reference row
    keep = [r for r in range(rows) if r != bad]
    Xn = X.clone()
    Xn[bad, 0] = float("inf")
    for log in (False, True):
        full = gp_ops.kg_pool(b, phi, X, topk=64, ref_idx=ri, maximize=True, log=log)
        nan = gp_ops.kg_pool(b, phi, Xn, topk=64, ref_idx=ri, maximize=True, log=log)
        gp_ops.check_info(nan["info"])
        assert bool(torch.isnan(nan["score"][:, bad]).all()), nan["score"][:, bad]
        assert not bool((nan["top_idx"] == bad).any()) and bool((nan["top_idx"] >= 0).all())
        assert _same(nan["score"][:, keep], full["score"][:, keep])
    b, phi, Zs, ys, n_s, X = _ill(dev)
    flagged = [t for t, kd in enumerate(_kinds(b)) if kd == 2]
    assert 1 in flagged
    rows = X.shape[0]
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    ri = torch.from_numpy(_refs_for(posts, 9, rows, False, 21)).to(dev)
    bad = next(r for r in range(rows) if r not in set(ri.flatten().tolist()))
    keep = [r for r in range(rows) if r != bad]
    Xn = X.clone()
    Xn[bad, 1] = float("nan")
    for log in (False, True):
        full = gp_ops.kg_pool(b, phi, X, topk=64, ref_idx=ri, log=log)
        nan = gp_ops.kg_pool(b, phi, Xn, topk=64, ref_idx=ri, log=log)
        gp_ops.check_info(nan["info"])
        assert bool(torch.isnan(nan["score"][flagged, bad]).all()), nan["score"][:, bad]
        assert not bool((nan["top_idx"][flagged] == bad).any()) and bool((nan["top_idx"][flagged] >= 0).all())
        assert _same(nan["score"][:, keep], full["score"][:, keep])
    b.flags = 0


def test_log_against_plain(dev):
    """exp(log KG) against KG from the same inputs on every row of a normal case, within the two evaluation bounds (the triangle
    inequality through the reference value K): |exp(l) - k| <= EVAL_C eps32 unit_plain + K expm1(EVAL_C_LOG eps32 unit_log)."""
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, M = CASES[0]
    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    pp = gp_ops.predict_pool(b, phi, X, latent=True)
    mean, var = pp["mean"].cpu().numpy(), pp["var"].cpu().numpy()
    noise = _noise32(phi, b.T)
    for maximize in (False, True):
        ref_idx = _refs_for(posts, M, rows, maximize, 7 + M)
        ri = torch.from_numpy(ref_idx).to(dev)
        plain = gp_ops.kg_pool(b, phi, X, ref_idx=ri, maximize=maximize, want_cov=True)
        lg = gp_ops.kg_pool(b, phi, X, ref_idx=ri, maximize=maximize, log=True)
        k, l = plain["score"].cpu().numpy().astype(np.float64), lg["score"].cpu().numpy().astype(np.float64)
        cov, rmean = plain["cov"].cpu().numpy(), plain["ref_mean"].cpu().numpy()
        for t in range(b.T):
            refs = R.valid_refs(ref_idx[t].tolist(), rows)
            K, up = _ref_at_inputs(mean[t], var[t], cov[t], rmean[t], refs, noise[t], maximize, False)
            _, ul = _ref_at_inputs(mean[t], var[t], cov[t], rmean[t], refs, noise[t], maximize, True)
            assert np.isfinite(l[t]).all() and (k[t] > 0).all()
            bound = R.EVAL_C * EPS32 * up + K * np.expm1(R.EVAL_C_LOG * EPS32 * ul)
            ratio = float((np.abs(np.exp(l[t]) - k[t]) / bound).max())
            print(f"log against plain, maximize {maximize} task {t}: worst |exp(l) - k| / bound {ratio:.3f}")
            assert (np.abs(np.exp(l[t]) - k[t]) <= bound).all(), (maximize, t, ratio)


def _underflow_problem(dev):
    """One task whose support holds one observation about 40 prior standard deviations below the rest (minimisation: far better), a pool
    whose row 0 is that support row, and row 0 alone as the reference set."""
    from adkf_ift_amd import gp_ops
    from oracle import gp_oracle as O

    ns, d, rows = 16, 6, 150
    Zs, ys, _ = M_._features(1, ns, [0], d, 91, True)
    med = float(torch.cdist(Zs[0].double(), Zs[0].double())[np.triu_indices(ns, 1)].median())
    ls = 0.15 * med                                              # a short lengthscale: no other pool row sees much of the outlier
    phi = torch.tensor([[-3.0, 0.3, math.log(math.expm1(ls))]], dtype=torch.float32, device=dev)
    os_ = float(O.transform_phi(phi[0].double().cpu())[1])
    ys = ys.clone()
    ys[0, 0] = float(ys[0, 1:].min()) - 40.0 * math.sqrt(os_)
    b = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.zeros(1, 4, device=dev), "rbf")
    X = P._pool(rows, d, 92)
    X[0] = Zs[0, 0]
    return b, phi, Zs, ys, X.to(dev)


def test_the_underflow_case(dev):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, X = _underflow_problem(dev)
    rows = X.shape[0]
    post = B.posterior(Zs[0], ys[0], X.cpu().numpy(), phi[0].cpu().numpy(), b.kernel)
    # on the CPU, with the reference alone: KG is below the smallest float32 denormal on every row
    lref, _, _ = R.kg_task(post, [0], False, log=True)
    assert np.isneginf(lref[0]) and (lref[1:] < math.log(1.4e-45) - 5.0).all() and np.isfinite(lref[1:]).all(), float(lref[1:].max())
    ri = torch.zeros(1, 1, dtype=torch.int64, device=dev)
    plain = gp_ops.kg_pool(b, phi, X, ref_idx=ri, want_cov=True)
    gp_ops.check_info(plain["info"])
    assert bool((plain["score"] == 0).all())
    k = 32
    lg = gp_ops.kg_pool(b, phi, X, ref_idx=ri, log=True, topk=k)
    l = lg["score"][0].cpu().numpy()
    assert np.isneginf(l[0]) and np.isfinite(l[1:]).all()
    # the order of the selection against the reference at the call's own numbers
    pp = gp_ops.predict_pool(b, phi, X, latent=True)
    mean, var = pp["mean"][0].cpu().numpy(), pp["var"][0].cpu().numpy()
    ref, unit = _ref_at_inputs(mean, var, plain["cov"][0].cpu().numpy(), plain["ref_mean"][0].cpu().numpy(), [0], _noise32(phi, 1)[0], False, True)
    _eval_check(l, ref, unit, R.EVAL_C_LOG, "underflow, log")
    got = lg["top_idx"][0].tolist()
    order = sorted(range(1, rows), key=lambda r: (-ref[r], r))
    bound = R.EVAL_C_LOG * EPS32 * unit
    clear = [ref[order[i]] - ref[order[i + 1]] > 2 * max(bound[order[i]], bound[order[i + 1]]) for i in range(k)]   # gap below place i
    settled = 0
    for i in range(k):
        if (i == 0 or clear[i - 1]) and clear[i]:
            assert got[i] == order[i], (i, got[i], order[i])
            settled += 1
    print(f"underflow case: {settled} of {k} places settled by the bound; log KG in [{ref[1:].min():.1f}, {ref[1:].max():.1f}]")
    assert settled > k // 2 and 0 not in got


def test_bo_loop(dev, monkeypatch):
    """The toy pool of the other loops' tests: records of the right length that never repeat an index, two runs are equal, a replicate
    alone is the replicate in a batch of four, and an iteration makes one mean top-n_refs call and one kg_pool call."""
    from adkf_ift_amd import bayes_opt as BO
    from adkf_ift_amd import gp_ops

    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=3, num_bo_iters=3, kernel_type="matern", device=dev, init_from=5000, noise_init=0.01,
              noise_prior=True, n_refs=16)
    calls = {"kg": 0, "pool": 0}
    kg_pool, predict_pool = gp_ops.kg_pool, gp_ops.predict_pool

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(gp_ops, "kg_pool", counted("kg", kg_pool))
    monkeypatch.setattr(gp_ops, "predict_pool", counted("pool", predict_pool))
    Rn = 4
    rngs = lambda n=Rn: [np.random.default_rng(s) for s in range(n)]
    recs = BO.run_gp_kg_bo_batched(X, y, rngs=rngs(), **kw)
    assert calls == {"kg": 3, "pool": 3}
    assert len(recs) == Rn
    for r in range(Rn):
        assert len(recs[r]) == 1 + 3 * 3 and len(set(recs[r][1:])) == 9 and all(0 <= i < 10000 for i in recs[r]), recs[r]
    assert recs == BO.run_gp_kg_bo_batched(X, y, rngs=rngs(), **kw)
    for r in (0, 3):
        alone = BO.run_gp_kg_bo_batched(X, y, rngs=[np.random.default_rng(r)], **kw)
        assert alone[0] == recs[r], (r, "the batch couples replicates")
    ard = BO.run_gp_kg_bo_batched(X, y, rngs=rngs(2), ard=True, **kw)
    for rec in ard:
        assert len(rec) == 1 + 3 * 3 and len(set(rec[1:])) == 9, rec
