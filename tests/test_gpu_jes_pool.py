"""GPU: joint entropy search over a shared pool (adkf_jes_pool / gp_ops.jes_pool) - the epilogue alone against the float64 score at the
call's own float32 mean, variance, cov, opt_mean and opt_var; the score end to end against the float64 reference of jes_ref.py within
its per-row bound, every row compared; every task kind (plain, refined, float64, ARD, one support row, tiny pools, more tasks than
workgroups); the bitwise properties of the call, GIBBON's a(x) at a huge cond_noise among them; NaN handling; the batched BO loop."""
import numpy as np
import pytest
import torch

import believer_ref as B
import gibbon_ref as G
import jes_ref as R
import test_gpu_believer_pool as BV
import test_gpu_believer_pool_ard as BVA
import test_gpu_kg_pool as KG
import test_gpu_predict_marginal as M_
import test_gpu_predict_pool as P
from test_believer_pool_ard_cpu import ard_posterior

pytestmark = pytest.mark.gpu

EPS32 = R.EPS32
CN = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, c):
    return torch.equal(_bits(a), _bits(c))


_built = {}


def _built_problem(dev, kernel, n_s, d, rows, seed):
    """jes_ref.problem on the device, once per shape, shared and left unchanged: (b, phi, Zs, ys, n_s, X)."""
    from adkf_ift_amd import gp_ops

    key = (kernel, tuple(n_s), d, rows, seed)
    if key not in _built:
        Zs, ys, X, phi = R.problem(n_s, d, rows, seed)
        T = len(n_s)
        b = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.zeros(T, 4, device=dev), kernel, n_s=torch.tensor(n_s, dtype=torch.int32))
        _built[key] = (b, phi.to(dev), Zs, ys, list(n_s), X.to(dev))
    return _built[key]


def _samples(posts, S, rows, maximize, seed, dev, messy=True, distinct=False):
    make = R.distinct_samples if distinct else (lambda *a: R.samples_for(*a, messy=messy))
    pairs = [make(posts[t], S, rows, maximize, seed + t) for t in range(len(posts))]
    idx, val = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return idx, val, torch.from_numpy(idx).to(dev), torch.from_numpy(val).to(dev)


def _check_against_reference(out, posts, idx, val, cond_noise, maximize, tag, tasks=None, cap=True):
    """score within delta on EVERY row of the tasks given (all by default), opt_mean and opt_var within the project's posterior bounds,
    score >= 0, and (cap) the bound is informative: the median over the rows of delta / max(score_ref, 1e-3) is below 0.5."""
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    score, omean, ovar = out["score"].cpu().numpy(), out["opt_mean"].cpu().numpy(), out["opt_var"].cpu().numpy()
    worst, compared = 0.0, 0
    for t in (range(len(posts)) if tasks is None else tasks):
        m, S, noise, os_ = posts[t]
        assert noise >= 1e-2 * os_ or not cap
        ref, delta, _, valid = R.jes_task(posts[t], idx[t], val[t], cond_noise, maximize)
        err = np.abs(score[t].astype(np.float64) - ref)
        print(f"{tag} task {t}: worst error / delta {float((err / delta).max()):.3f}, median delta / max(score, 1e-3) "
              f"{float(np.median(delta / np.maximum(ref, 1e-3))):.4f}")
        assert (err <= delta).all(), (tag, t, int(np.argmax(err / delta)), float((err / delta).max()))
        worst = max(worst, float((err / delta).max()))
        compared += ref.size
        if cap:
            assert float(np.median(delta / np.maximum(ref, 1e-3))) < 0.5, (tag, t, "a vacuous bound")
        assert (score[t] >= 0).all(), (tag, t)
        dm = B.TOL * max(1.0, float(np.abs(m).max()))
        for j, p in enumerate(valid):
            if p < 0:
                assert omean[t, j] == 0 and ovar[t, j] == 0, (tag, t, j)
            else:
                assert abs(omean[t, j] - m[p]) <= dm and abs(ovar[t, j] - S[p, p]) <= B.TOL * os_, (tag, t, j)
    return worst, compared


# ---- the epilogue alone
EPI_CASES = [("rbf", [32, 29, 21], 16, 200, 5), ("matern", [200, 133], 16, 130, 64), ("matern", [32, 32], 3, 65, 1)]


def _ref_at_inputs(mean_t, var_t, cov_t, omean_t, ovar_t, val_t, noise, cond_noise, maximize):
    """The float64 score of one task at the call's own float32 numbers (every sample valid): (ref [rows], unit [rows])."""
    ok = [True] * len(val_t)
    ref, gamma = R.score_of(mean_t, var_t, cov_t, omean_t, ovar_t, val_t, ok, noise, cond_noise, maximize, h=R.h64, clamp=R.CLAMP32)
    return ref, G.gamma_weight(gamma)


@pytest.mark.parametrize("kernel,n_s,d,rows,S", EPI_CASES)
def test_the_epilogue_alone(dev, kernel, n_s, d, rows, S):
    """score against the float64 score evaluated at the call's OWN float32 mean and latent variance (predict_pool(latent=True) on the
    same batch: the same tile arithmetic), cov (kg_pool(ref_idx=opt_idx, want_cov=True) on duplicate-free opt_idx: the same panel),
    opt_mean, opt_var, noise and cond_noise, every row compared:  |got - ref| <= EVAL_C eps32 mean_s (1 + gamma_s^2).
    EVAL_C is 4 x the largest ratio this test has printed on the MI355X, rounded up to a power of two (jes_ref.py)."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X = _built_problem(dev, kernel, n_s, d, rows, 700 + max(n_s) + S)
    posts = KG._post_of(b, phi, Zs, ys, n_s, X)
    pp = gp_ops.predict_pool(b, phi, X, latent=True)
    gp_ops.check_info(pp["info"])
    mean, var = pp["mean"].cpu().numpy(), pp["var"].cpu().numpy()
    noise = KG._noise32(phi, b.T)
    cn32 = float(np.float32(CN))
    worst, compared = 0.0, 0
    for maximize in (False, True):
        idx, val, di, dv = _samples(posts, S, rows, maximize, 41, dev, distinct=True)
        out = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, cond_noise=CN, maximize=maximize)
        kg = gp_ops.kg_pool(b, phi, X, ref_idx=di, maximize=maximize, want_cov=True)
        gp_ops.check_info(out["info"])
        assert _same(out["opt_mean"], kg["ref_mean"])
        got, cov = out["score"].cpu().numpy().astype(np.float64), kg["cov"].cpu().numpy()
        omean, ovar = out["opt_mean"].cpu().numpy(), out["opt_var"].cpu().numpy()
        for t in range(b.T):
            ref, unit = _ref_at_inputs(mean[t], var[t], cov[t], omean[t], ovar[t], val[t], noise[t], cn32, maximize)
            ratio = np.abs(got[t] - ref) / (EPS32 * unit)
            print(f"{kernel} ns {n_s[t]} S {S} {'max' if maximize else 'min'} task {t}: worst |got - ref| / (eps32 unit) = {float(ratio.max()):.3f} "
                  f"(row {int(ratio.argmax())}) over {ratio.size} rows")
            worst = max(worst, float(ratio.max()))
            compared += ratio.size
            assert (got[t] >= 0).all()
    print(f"{kernel} ns {max(n_s)} S {S}: worst ratio {worst:.3f} (EVAL_C {R.EVAL_C})")
    assert compared == 2 * b.T * rows   # no row was left out
    assert worst <= R.EVAL_C, worst


# ---- end to end
@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_against_the_reference(dev, case):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, S, maximize = R.CASES[case]
    b, phi, Zs, ys, n_s, X = _built_problem(dev, kernel, n_s, d, rows, 900 + case)
    posts = KG._post_of(b, phi, Zs, ys, n_s, X)
    idx, val, di, dv = _samples(posts, S, rows, maximize, 31, dev)
    out = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, cond_noise=CN, maximize=maximize)
    _, compared = _check_against_reference(out, posts, idx, val, CN, maximize, (case, kernel, max(n_s), S, maximize))
    assert compared == b.T * rows


def test_ard(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, S = "matern", [48, 45, 31], 12, 130, 5
    b, phi, Zs, ys, n_s, X, _ = BVA._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    posts = KG._post_of(b, phi, Zs, ys, n_s, X, ard=True)
    for maximize in (False, True):
        idx, val, di, dv = _samples(posts, S, rows, maximize, 3, dev)
        out = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, cond_noise=CN, maximize=maximize)
        _check_against_reference(out, posts, idx, val, CN, maximize, ("ard", maximize))


def test_global_row_tile_slots(dev):
    """1024 support points: the row tiles do not fit the LDS and move to the global slots.  The problem is the believer's and the
    knowledge gradient's at this size (test_gpu_believer_pool._explicit), on which prediction's own mean and variance meet the
    posterior bounds the derived part of delta starts from - asserted here first: at a thousand points that is a property of the
    problem, not of the shape (on jes_ref.problem(950) at these sizes, with the median distance as the lengthscale, predict_pool's
    mean is off by 1.4e-3 and its variance by 2.0e-3 for the 700-point task, ten and thirty times those bounds)."""
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, S = "matern", [1024, 700], 12, 130, 5
    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    posts = KG._post_of(b, phi, Zs, ys, n_s, X)
    pp = gp_ops.predict_pool(b, phi, X, latent=True)
    for t, (m, Sg, _, os_) in enumerate(posts):
        assert np.abs(pp["mean"][t].cpu().numpy() - m).max() <= B.TOL * max(1.0, float(np.abs(m).max())), t
        assert np.abs(pp["var"][t].cpu().numpy() - Sg.diagonal()).max() <= B.TOL * os_, t
    idx, val, di, dv = _samples(posts, S, rows, False, 31, dev)
    out = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, cond_noise=CN, topk=4, want_score=True)
    _, compared = _check_against_reference(out, posts, idx, val, CN, False, ("slots", 1024))
    assert compared == b.T * rows
    score = out["score"].cpu().numpy()
    for t in range(b.T):
        wi, _ = R.topk_of(score[t], 4)
        assert np.array_equal(out["top_idx"][t].cpu().numpy(), wi), t


def test_a_float64_task_beside_float32_ones(dev):
    """test_gpu_kg_pool._ill's problem: task 1 takes the float64 walk (asserted from the fitted scalars; the kinds are printed).  The
    score of EVERY task end to end (the fitted noise is small there, so the cap on the bound is not asserted), then the epilogue of every
    flagged task against the float64 score at the call's own numbers, as test_the_epilogue_alone."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X = KG._ill(dev)
    kinds = KG._kinds(b)
    print("kinds:", kinds)
    flagged = [t for t, kd in enumerate(kinds) if kd == 2]
    assert 1 in flagged and min(kinds) < 2
    rows = X.shape[0]
    posts = KG._post_of(b, phi, Zs, ys, n_s, X)
    pp = gp_ops.predict_pool(b, phi, X, latent=True)
    mean, var = pp["mean"].cpu().numpy(), pp["var"].cpu().numpy()
    noise = KG._noise32(phi, b.T)
    cn = 1e-3
    for maximize in (False, True):
        idx, val, di, dv = _samples(posts, 9, rows, maximize, 21, dev, distinct=True)
        out = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, cond_noise=cn, maximize=maximize)
        _check_against_reference(out, posts, idx, val, cn, maximize, ("mixed", maximize), cap=False)
        kg = gp_ops.kg_pool(b, phi, X, ref_idx=di, maximize=maximize, want_cov=True)
        assert _same(out["opt_mean"], kg["ref_mean"])
        got, cov = out["score"].cpu().numpy().astype(np.float64), kg["cov"].cpu().numpy()
        omean, ovar = out["opt_mean"].cpu().numpy(), out["opt_var"].cpu().numpy()
        for t in flagged:
            ref, unit = _ref_at_inputs(mean[t], var[t], cov[t], omean[t], ovar[t], val[t], noise[t], float(np.float32(cn)), maximize)
            ratio = float((np.abs(got[t] - ref) / (EPS32 * unit)).max())
            print(f"float64 task {t} {'max' if maximize else 'min'}: worst |got - ref| / (eps32 unit) = {ratio:.3f}")
            assert ratio <= R.EVAL_C, (t, maximize, ratio)
    b.flags = 0


def test_tiny_pools(dev):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X = _built_problem(dev, "matern", [32, 29], 16, 65, 906)
    X5 = X[:5].contiguous()
    posts = KG._post_of(b, phi, Zs, ys, n_s, X5)
    idx = np.array([[0, 2, 4, 9]] * b.T, np.int64)   # 9: outside this pool, skipped
    val = np.stack([posts[t][0].max() + np.array([0.1, 0.5, 1.0, 2.0]) for t in range(b.T)]).astype(np.float32)
    out = gp_ops.jes_pool(b, phi, X5, opt_idx=torch.from_numpy(idx).to(dev), opt_val=torch.from_numpy(val).to(dev), maximize=True, topk=8,
                          want_score=True)
    _check_against_reference(out, posts, idx, val, CN, True, "rows = 5")
    assert bool((out["top_idx"][:, 5:] == -1).all()) and bool(torch.isneginf(out["top_val"][:, 5:]).all()) and bool((out["top_idx"][:, :5] >= 0).all())
    # no row: no sample is valid
    zi, zv = torch.zeros(b.T, 3, dtype=torch.int64, device=dev), torch.zeros(b.T, 3, device=dev)
    none = gp_ops.jes_pool(b, phi, X[:0].contiguous(), opt_idx=zi, opt_val=zv, topk=2, want_score=True)
    assert none["score"].shape == (b.T, 0) and bool((none["top_idx"] == -1).all()) and bool((none["opt_mean"] == 0).all())


def test_more_tasks_than_workgroups(dev):
    """T = 300 tiny tasks over two tiles, one partial: the score of every task end to end, and three tasks alone are the tasks in the batch."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, S = 300, 8, 4, 70, 3
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
    posts = KG._post_of(b, phi, Zs, ys, n_s, X)
    idx, val, di, dv = _samples(posts, S, rows, False, 5, dev, messy=False)
    out = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, topk=4, want_score=True)
    _check_against_reference(out, posts, idx, val, CN, False, "T300")
    for t in (0, 151, 299):
        b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), "matern",
                            n_s=torch.tensor([n_s[t]], dtype=torch.int32))
        o1 = gp_ops.jes_pool(b1, phi[t:t + 1].contiguous(), X, opt_idx=di[t:t + 1].contiguous(), opt_val=dv[t:t + 1].contiguous(), topk=4,
                             want_score=True)
        for name in ("score", "opt_mean", "opt_var", "top_val"):
            assert _same(o1[name][0], out[name][t]), (name, t)
        assert torch.equal(o1["top_idx"][0], out["top_idx"][t])


# ---- bitwise properties
def test_bitwise_properties(dev):
    """Two runs are equal; a task alone is the task in a batch; a permutation of the tasks permutes the results; top_idx / top_val are
    the sort of score under the unique order with the exclusions applied; the score does not depend on k; score >= 0; opt_mean is
    kg_pool's ref_mean on duplicate-free samples - on the plain and refined float32 walks, and on the float64 walk beside them."""
    from adkf_ift_amd import gp_ops

    for case in (0, 7):
        kernel, n_s, d, rows, S, maximize = R.CASES[case]
        b, phi, Zs, ys, n_s, X = _built_problem(dev, kernel, n_s, d, rows, 900 + case)
        posts = KG._post_of(b, phi, Zs, ys, n_s, X)
        _, _, di, dv = _samples(posts, S, rows, maximize, 31, dev)
        lists = [[0, 7], [3]] + [[]] * (b.T - 2)
        kw = dict(opt_idx=di, opt_val=dv, cond_noise=CN, maximize=maximize, want_score=True)
        first = gp_ops.jes_pool(b, phi, X, topk=8, exclude=lists, **kw)
        again = gp_ops.jes_pool(b, phi, X, topk=8, exclude=lists, **kw)
        for name in ("score", "opt_mean", "opt_var", "top_val"):
            assert _same(first[name], again[name]), name
        assert torch.equal(first["top_idx"], again["top_idx"])
        for k in (0, 1, 64):
            other = gp_ops.jes_pool(b, phi, X, topk=k, exclude=lists, **kw)
            assert _same(other["score"], first["score"]) and _same(other["opt_var"], first["opt_var"]), k
        blind = gp_ops.jes_pool(b, phi, X, topk=8, exclude=lists, opt_idx=di, opt_val=dv, cond_noise=CN, maximize=maximize, want_score=False)
        assert blind["score"] is None and torch.equal(blind["top_idx"], first["top_idx"]) and _same(blind["top_val"], first["top_val"])
        score = first["score"].cpu().numpy()
        assert (score >= 0).all()
        for t in range(b.T):
            wi, wv = R.topk_of(score[t], 8, lists[t])
            assert np.array_equal(first["top_idx"][t].cpu().numpy(), wi) and np.array_equal(first["top_val"][t].cpu().numpy().view(np.int32), wv.view(np.int32))
            b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), kernel,
                                n_s=torch.tensor([n_s[t]], dtype=torch.int32))
            o1 = gp_ops.jes_pool(b1, phi[t:t + 1].contiguous(), X, topk=8, exclude=[lists[t]], opt_idx=di[t:t + 1].contiguous(),
                                 opt_val=dv[t:t + 1].contiguous(), cond_noise=CN, maximize=maximize, want_score=True)
            for name in ("score", "opt_mean", "opt_var", "top_val"):
                assert _same(o1[name][0], first[name][t]), (name, t)
            assert torch.equal(o1["top_idx"][0], first["top_idx"][t])
        perm = list(range(b.T))[::-1]
        bp = gp_ops.GPBatch(b.Z_s[perm].contiguous(), b.y_s[perm].contiguous(), b.priors[perm].contiguous(), kernel,
                            n_s=torch.tensor([n_s[t] for t in perm], dtype=torch.int32))
        op = gp_ops.jes_pool(bp, phi[perm].contiguous(), X, topk=8, exclude=[lists[t] for t in perm], opt_idx=di[perm].contiguous(),
                             opt_val=dv[perm].contiguous(), cond_noise=CN, maximize=maximize, want_score=True)
        for name in ("score", "opt_mean", "opt_var", "top_val"):
            assert _same(op[name], first[name][perm]), (name, "permuted")
        assert torch.equal(op["top_idx"], first["top_idx"][perm])
        # opt_mean is kg_pool's ref_mean, bit for bit, on duplicate-free samples
        _, _, qi, qv = _samples(posts, S, rows, maximize, 41, dev, distinct=True)
        assert _same(gp_ops.jes_pool(b, phi, X, opt_idx=qi, opt_val=qv, maximize=maximize)["opt_mean"],
                     gp_ops.kg_pool(b, phi, X, ref_idx=qi, maximize=maximize, want_score=False, topk=1)["ref_mean"])
    b, phi, Zs, ys, n_s, X = KG._ill(dev)                       # the float64 walk (task 1) beside float32 ones
    posts = KG._post_of(b, phi, Zs, ys, n_s, X)
    _, _, di, dv = _samples(posts, 9, X.shape[0], False, 21, dev, distinct=True)
    first = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, cond_noise=1e-3, topk=8, want_score=True)
    again = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, cond_noise=1e-3, topk=8, want_score=True)
    for name in ("score", "opt_mean", "opt_var", "top_val"):
        assert _same(first[name], again[name]), name
    assert _same(first["opt_mean"], gp_ops.kg_pool(b, phi, X, ref_idx=di, want_score=False, topk=1)["ref_mean"])
    score = first["score"].cpu().numpy()
    assert (score >= 0).all()
    for t in range(b.T):
        wi, _ = R.topk_of(score[t], 8)
        assert np.array_equal(first["top_idx"][t].cpu().numpy(), wi), t
    b1 = gp_ops.GPBatch(b.Z_s[1:2].contiguous(), b.y_s[1:2].contiguous(), b.priors[1:2].contiguous(), b.kernel,
                        n_s=torch.tensor([n_s[1]], dtype=torch.int32))
    o1 = gp_ops.jes_pool(b1, phi[1:2].contiguous(), X, opt_idx=di[1:2].contiguous(), opt_val=dv[1:2].contiguous(), cond_noise=1e-3, topk=8,
                         want_score=True)
    b.flags = 0
    full = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, cond_noise=1e-3, topk=8, want_score=True)   # (both evaluate at phi: no state of a fit is reused)
    for name in ("score", "opt_mean", "opt_var", "top_val"):
        assert _same(o1[name][0], full[name][1]), name
    assert torch.equal(o1["top_idx"][0], full["top_idx"][1])


def test_a_huge_cond_noise_gives_gibbon(dev):
    """cond_noise = 1e30 with every sample valid: c^2 / d_s and the shift of the mean round away, and the score is
    gibbon_pool(q = 1, want_trace=True)["trace"][:, 0] for ystar = opt_val, bit for bit - float32 tasks (plain and refined) and the
    float64 task of the ill-conditioned batch."""
    from adkf_ift_amd import gp_ops

    for case in (0, 1, 7):
        kernel, n_s, d, rows, S, maximize = R.CASES[case]
        b, phi, Zs, ys, n_s, X = _built_problem(dev, kernel, n_s, d, rows, 900 + case)
        posts = KG._post_of(b, phi, Zs, ys, n_s, X)
        _, _, di, dv = _samples(posts, S, rows, maximize, 31, dev, messy=False)
        assert bool(((di >= 0) & (di < rows)).all())
        jes = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, cond_noise=1e30, maximize=maximize)
        gib = gp_ops.gibbon_pool(b, phi, X, ystar=dv, q=1, maximize=maximize, want_trace=True)
        gp_ops.check_info(jes["info"])
        assert _same(jes["score"], gib["trace"][:, 0]), (case, float((jes["score"] - gib["trace"][:, 0]).abs().max()))
        assert bool((jes["score"] > 0).any())
    b, phi, Zs, ys, n_s, X = KG._ill(dev)
    kinds = KG._kinds(b)
    assert kinds[1] == 2
    posts = KG._post_of(b, phi, Zs, ys, n_s, X)
    for maximize in (False, True):
        _, _, di, dv = _samples(posts, 9, X.shape[0], maximize, 21, dev, messy=False)
        jes = gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=dv, cond_noise=1e30, maximize=maximize)
        gib = gp_ops.gibbon_pool(b, phi, X, ystar=dv, q=1, maximize=maximize, want_trace=True)
        assert _same(jes["score"], gib["trace"][:, 0]), ("mixed", maximize, kinds)
    b.flags = 0


# ---- NaN handling
def test_nan_handling(dev):
    """A pool row with a non-finite feature (no sampled location) scores NaN and is never selected, and every other row keeps its bits
    (tile walk: an infinite feature under Matern, as test_gpu_kg_pool; float64 walk: a NaN feature).  A non-finite opt_val on a valid
    entry makes that task NaN and leaves the others untouched; all -1 gives NaN and a -1 / -inf selection."""
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, S, maximize = R.CASES[1]
    assert kernel == "matern"
    b, phi, Zs, ys, n_s, X = _built_problem(dev, kernel, n_s, d, rows, 901)
    posts = KG._post_of(b, phi, Zs, ys, n_s, X)
    _, _, di, dv = _samples(posts, S, rows, maximize, 31, dev)
    used = set(di.flatten().tolist())
    bad = next(r for r in range(rows - 1, -1, -1) if r not in used)   # towards the end of the pool: the second tile when there is one
    keep = [r for r in range(rows) if r != bad]
    Xn = X.clone()
    Xn[bad, 0] = float("inf")
    full = gp_ops.jes_pool(b, phi, X, topk=64, opt_idx=di, opt_val=dv, maximize=maximize, want_score=True)
    nan = gp_ops.jes_pool(b, phi, Xn, topk=64, opt_idx=di, opt_val=dv, maximize=maximize, want_score=True)
    gp_ops.check_info(nan["info"])
    assert bool(torch.isnan(nan["score"][:, bad]).all()), nan["score"][:, bad]
    assert not bool((nan["top_idx"] == bad).any()) and bool((nan["top_idx"] >= 0).all())
    assert _same(nan["score"][:, keep], full["score"][:, keep])
    # a non-finite value: that task only
    for badv in (float("nan"), float("inf"), float("-inf")):
        v2 = dv.clone()
        valid_s = next(s for s in range(S) if 0 <= int(di[1, s]) < rows)
        v2[1, valid_s] = badv
        o2 = gp_ops.jes_pool(b, phi, X, topk=4, opt_idx=di, opt_val=v2, maximize=maximize, want_score=True)
        assert bool(torch.isnan(o2["score"][1]).all()) and bool((o2["top_idx"][1] == -1).all()) and bool(torch.isneginf(o2["top_val"][1]).all())
        assert _same(o2["score"][0], full["score"][0]) and torch.equal(o2["top_idx"][0], full["top_idx"][0, :4])
    # a non-finite value on a skipped entry is not read
    skipped_s = next(s for s in range(S) if not 0 <= int(di[0, s]) < rows)
    v3 = dv.clone()
    v3[0, skipped_s] = float("nan")
    assert _same(gp_ops.jes_pool(b, phi, X, opt_idx=di, opt_val=v3, maximize=maximize)["score"], full["score"])
    # no valid sample at all in task 0
    i4 = di.clone()
    i4[0] = -1
    o4 = gp_ops.jes_pool(b, phi, X, topk=4, opt_idx=i4, opt_val=dv, maximize=maximize, want_score=True)
    assert bool(torch.isnan(o4["score"][0]).all()) and bool((o4["top_idx"][0] == -1).all()) and bool(torch.isneginf(o4["top_val"][0]).all())
    assert bool((o4["opt_mean"][0] == 0).all()) and bool((o4["opt_var"][0] == 0).all()) and _same(o4["score"][1], full["score"][1])
    # the float64 walk
    b, phi, Zs, ys, n_s, X = KG._ill(dev)
    flagged = [t for t, kd in enumerate(KG._kinds(b)) if kd == 2]
    assert 1 in flagged
    rows = X.shape[0]
    posts = KG._post_of(b, phi, Zs, ys, n_s, X)
    _, _, di, dv = _samples(posts, 9, rows, False, 21, dev, distinct=True)
    bad = next(r for r in range(rows) if r not in set(di.flatten().tolist()))
    keep = [r for r in range(rows) if r != bad]
    Xn = X.clone()
    Xn[bad, 1] = float("nan")
    full = gp_ops.jes_pool(b, phi, X, topk=64, opt_idx=di, opt_val=dv, cond_noise=1e-3, want_score=True)
    nan = gp_ops.jes_pool(b, phi, Xn, topk=64, opt_idx=di, opt_val=dv, cond_noise=1e-3, want_score=True)
    gp_ops.check_info(nan["info"])
    assert bool(torch.isnan(nan["score"][flagged, bad]).all()), nan["score"][:, bad]
    assert not bool((nan["top_idx"][flagged] == bad).any()) and bool((nan["top_idx"][flagged] >= 0).all())
    assert _same(nan["score"][:, keep], full["score"][:, keep])
    v2 = dv.clone()
    v2[1, 0] = float("inf")
    o2 = gp_ops.jes_pool(b, phi, X, topk=4, opt_idx=di, opt_val=v2, cond_noise=1e-3, want_score=True)
    assert bool(torch.isnan(o2["score"][1]).all()) and bool((o2["top_idx"][1] == -1).all()) and _same(o2["score"][0], full["score"][0])
    b.flags = 0


# ---- the BO loop
def test_bo_loop(dev, monkeypatch):
    """A toy pool of 150 rows, 3 replicates, 3 iterations: records of the right length that never repeat an index, two runs are equal,
    a replicate alone is the replicate in the batch, and an iteration makes one optimum_samples call and one jes_pool call."""
    from adkf_ift_amd import bayes_opt as BO
    from adkf_ift_amd import gp_ops

    g = torch.Generator().manual_seed(3)
    X = torch.randn(150, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=3, num_bo_iters=3, kernel_type="matern", device=dev, init_from=75, noise_init=0.01,
              noise_prior=True, n_features=256, n_opt_samples=8)
    calls = {"jes": 0, "opt": 0}
    jes_pool, optimum_samples = gp_ops.jes_pool, gp_ops.optimum_samples

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(gp_ops, "jes_pool", counted("jes", jes_pool))
    monkeypatch.setattr(gp_ops, "optimum_samples", counted("opt", optimum_samples))
    Rn = 3
    rngs = lambda n=Rn: [np.random.default_rng(s) for s in range(n)]
    recs = BO.run_gp_jes_bo_batched(X, y, rngs=rngs(), **kw)
    assert calls == {"jes": 3, "opt": 3}
    assert len(recs) == Rn
    for r in range(Rn):
        assert len(recs[r]) == 1 + 3 * 3 and len(set(recs[r][1:])) == 9 and all(0 <= i < 150 for i in recs[r]), recs[r]
    assert recs == BO.run_gp_jes_bo_batched(X, y, rngs=rngs(), **kw)
    for r in (0, 2):
        alone = BO.run_gp_jes_bo_batched(X, y, rngs=[np.random.default_rng(r)], **kw)
        assert alone[0] == recs[r], (r, "the batch couples replicates")
    ard = BO.run_gp_jes_bo_batched(X, y, rngs=rngs(2), ard=True, **kw)
    for rec in ard:
        assert len(rec) == 1 + 3 * 3 and len(set(rec[1:])) == 9, rec
    # optimum_samples is max_value_samples with the rows kept
    b, phi, Zs, ys, n_s, Xp = _built_problem(dev, "rbf", [32, 29, 21], 3, 200, 900)
    omega, phase = gp_ops.rff_basis("rbf", 3, 128, generator=torch.Generator().manual_seed(0), device=dev)
    os_ = gp_ops.optimum_samples(b, phi, Xp, omega=omega, phase=phase, n_samples=4, generator=torch.Generator().manual_seed(5))
    mv = gp_ops.max_value_samples(b, phi, Xp, omega=omega, phase=phase, n_samples=4, w=os_["w"], eps=os_["eps"])
    assert _same(os_["opt_val"], mv["ystar"]) and bool(((os_["opt_idx"] >= 0) & (os_["opt_idx"] < 200)).all())
