"""GPU: log EI (ADKF_PM_LOG_EI / log_ei=True) - the new epilogue alone against an mpmath reference at the call's own mean and
variance, end to end against the float64 oracle, the structure it inherits (pool = packed, the selection, nothing changed
without the flag, exp(log EI) = EI), the underflow case it exists for, and the BO loops under acquisition="log_ei"."""
import numpy as np
import pytest
import torch

import test_gpu_predict_marginal as M
import test_gpu_predict_marginal_ard as MA
import test_gpu_predict_pool as P
from test_log_ei_cpu import EPS32, log_ei_ref
from test_predict_pool_cpu import select_ref

pytestmark = pytest.mark.gpu

SHAPES = [("rbf", 32, 16), ("matern", 200, 64)]   # test_gpu_predict_pool.test_against_the_oracle's: plain and refined
T, ROWS = 4, 777
POOL_SEED = 8          # _pool(ROWS, d, 8), as test_against_the_oracle; test_the_underflow_case_is_fixed states what it needs of it
CLAMP32 = float(np.float32(1e-12))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


_cases = {}


def _case(dev, kernel, ns, d):
    """One fitted batch per shape, shared by the tests and left unchanged: (b, phi, Zs, ys, n_s, X, Xc, best, post) with X the pool,
    Xc the pool whose first n_s[0] rows are task 0's support rows, best [T] the medians of y, post[t] the float64 oracle's
    (mean, latent variance) on X."""
    from adkf_ift_amd import gp_ops

    key = (kernel, ns, d)
    if key not in _cases:
        n_s = [ns, ns - 3, (2 * ns) // 3, ns // 4]
        Zs, ys, _ = M._features(T, ns, [0] * T, d, 55 + ns, True)
        b, phi = M._fit(dev, Zs, ys, n_s, kernel, True)
        b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
        X = P._pool(ROWS, d, POOL_SEED)
        Xc = X.clone()
        Xc[:n_s[0]] = Zs[0, :n_s[0]]
        best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(T)])
        kind = gp_ops.kernel_id(kernel)
        post = []
        for t in range(T):
            m_ref, v_ref, noise = M._oracle_diag(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], kind)
            post.append((m_ref, v_ref - noise))
        _cases[key] = (b, phi, Zs, ys, n_s, X.to(dev), Xc.to(dev), best, post)
    return _cases[key]


RANGES = (("u > -1", -1.0, np.inf), ("-12 < u <= -1", -12.0, -1.0), ("u <= -12", -np.inf, -12.0))


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_the_epilogue_alone(dev, kernel, ns, d):
    """pm_log_ei against mpmath at the call's OWN float32 mean and latent variance (sigma and u formed in float64 from them, with
    the kernel's clamp), which leaves the GP's float32 error out:
        |got - ref| <= 32 eps32 (1 + u^2) + 4 eps32 |log sigma|.
    u carries three float32 roundings (about 3 eps32 u^2 in the tail, where d log h / du ~ -u), the evaluation adds under
    2 eps32 (1 + u^2) with an exact erfcx, and the rest is room for the device's erfcxf, logf and expf in the cancelling bracket.
    The pool holds task 0's support rows: small variances, large |u|."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = _case(dev, kernel, ns, d)
    worst = {name: 0.0 for name, _, _ in RANGES}
    count = {name: 0 for name, _, _ in RANGES}
    compared = 0
    for shift in (0.0, 8.0, 30.0):
        bf = (best - shift).float()
        out = gp_ops.predict_pool(b, phi, Xc, latent=True, best_f=bf.to(dev), log_ei=True)
        gp_ops.check_info(out["info"])
        mean, var, lei = (out[n].cpu().numpy() for n in ("mean", "var", "ei"))
        assert np.isfinite(lei).all() and lei.shape == (T, ROWS)
        for t in range(T):
            ref, u, ls = log_ei_ref(mean[t], var[t], float(bf[t]), False, clamp=CLAMP32)
            err = np.abs(lei[t].astype(np.float64) - ref)
            unit = EPS32 * (1.0 + u * u)
            for name, lo, hi in RANGES:
                sel = (u > lo) & (u <= hi)
                if sel.any():
                    worst[name] = max(worst[name], float((err[sel] / unit[sel]).max()))
                    count[name] += int(sel.sum())
            bound = 32 * unit + 4 * EPS32 * np.abs(ls)
            print(f"{kernel} shift {shift} task {t}: u in [{u.min():.4g}, {u.max():.4g}], min var {var[t].min():.3g}, "
                  f"worst err / bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (shift, t, float((err / bound).max()), u[(err / bound).argmax()])
            compared += ref.size
    print(f"{kernel}: worst |got - ref| / (eps32 (1 + u^2)) per range {worst}, rows per range {count}")
    assert compared == 3 * T * ROWS                      # no row was left out
    assert all(count[name] > 0 for name in count), count   # and every range of the evaluation was reached


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_against_the_oracle(dev, kernel, ns, d):
    """End to end, best_f lowered by 8: |got - ref| <= (1 + u^2) 2 TOL + 1e-4 with ref and u from the float64 oracle's mean and
    latent variance and TOL what test_gpu_predict_pool holds mean and var to (a relative error TOL in the mean and TOL / 2 in
    sigma move u by about 2 TOL |u| here, and log h by |u| times that).  On the pool of test_against_the_oracle, whose rows keep
    the variance far from cancellation so that TOL is a per-row statement.  The bound is not vacuous: it stays under a tenth of
    the spread of each task's scores."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = _case(dev, kernel, ns, d)
    bf = (best - 8.0).float()
    out = gp_ops.predict_pool(b, phi, X, latent=True, best_f=bf.to(dev), log_ei=True, want_mean=False, want_var=False)
    lei = out["ei"].cpu().numpy()
    for t in range(T):
        ref, u, _ = log_ei_ref(post[t][0], post[t][1], float(bf[t]))
        bound = (1.0 + u * u) * 2 * P.TOL + 1e-4
        err = np.abs(lei[t].astype(np.float64) - ref)
        print(f"{kernel} task {t}: u in [{u.min():.4g}, {u.max():.4g}], worst err / bound {float((err / bound).max()):.3f}, "
              f"largest bound {bound.max():.3g}, spread of the scores {ref.max() - ref.min():.3g}")
        assert bound.max() < 0.1 * (ref.max() - ref.min()), "shift 8 makes the bound vacuous here"
        assert (err <= bound).all(), (t, float((err / bound).max()))


def _pool_equals_packed(b, phi, X, best, tag):
    from adkf_ift_amd import gp_ops

    rows = X.shape[0]
    for latent, maximize in ((False, False), (True, True)):
        out = gp_ops.predict_pool(b, phi, X, latent=latent, best_f=best, maximize=maximize, log_ei=True)
        plain = gp_ops.predict_pool(b, phi, X, latent=latent, best_f=best, maximize=maximize)
        gp_ops.check_info(out["info"])
        assert torch.equal(out["mean"], plain["mean"]) and torch.equal(out["var"], plain["var"]), tag
        assert not torch.equal(out["ei"], plain["ei"]), tag
        for t in range(b.T):
            q_off = torch.tensor([0] * (t + 1) + [rows] * (b.T - t), dtype=torch.int64, device=X.device)
            mean, var, lei, _ = gp_ops.predict_marginal(b, phi, X, q_off, latent=latent, best_f=best, maximize=maximize, log_ei=True)
            assert torch.equal(out["ei"][t], lei), (tag, t)
            assert torch.equal(out["mean"][t], mean) and torch.equal(out["var"][t], var), (tag, t)
            assert bool(torch.isfinite(lei).all()) and bool((lei != 0).any())


def test_pool_equals_packed(dev):
    """Bit for bit under the flag, on every kind of task: plain, refined, float64, ARD."""
    from adkf_ift_amd import gp_ops

    best = torch.tensor([0.1, -0.2, 0.3, 0.0], device=dev)
    for kernel, ns, d in SHAPES:
        b, phi, _, _, _, X, Xc, _, _ = _case(dev, kernel, ns, d)
        _pool_equals_packed(b, phi, Xc[:333], best - 3.0, (kernel, ns))
    b, phi, *_ = P._ill_batch(dev)
    X = torch.cat([P._pool(200, 2, 3), b.Z_s[1, :5].cpu()]).to(dev)
    _pool_equals_packed(b, phi, X, best, "float64")
    n_s = [32, 25, 17, 9]
    Zs, ys, _ = M._features(4, 32, [0] * 4, 12, 31, True)
    b, phi = MA._fit_ard(dev, Zs, ys, n_s, "matern", True)
    b.flags = gp_ops.REUSE_INNER
    X = P._pool(203, 12, 5).to(dev)
    _pool_equals_packed(b, phi, X, best - 3.0, "ard")
    gp_ops.predict_pool(b, phi, X, best_f=best, log_ei=True, want_ei=False, topk=4)                          # the selection reads it
    with pytest.raises(ValueError, match="log_ei"):
        gp_ops.predict_marginal(b, phi, X, torch.zeros(5, dtype=torch.int64, device=dev), log_ei=True)        # no best_f
    with pytest.raises(ValueError, match="log_ei"):
        gp_ops.predict_pool(b, phi, X, best_f=best, log_ei=True, want_ei=False)                              # nothing reads it
    with pytest.raises(ValueError, match="log_ei"):
        gp_ops.predict_pool(b, phi, X, best_f=best, log_ei=True, want_ei=False, topk=4, score="mean")


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_selection_and_the_unflagged_call(dev, kernel, ns, d):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = _case(dev, kernel, ns, d)
    lists = [[0, 1, 5, 700], [], list(range(0, ROWS, 2)), [776]]
    for shift in (0.0, 30.0):
        bf = (best - shift).float().to(dev)
        out = gp_ops.predict_pool(b, phi, Xc, latent=True, best_f=bf, log_ei=True, topk=8, exclude=lists)
        lei, ti, tv = out["ei"].cpu().numpy(), out["top_idx"].cpu().numpy(), out["top_val"].cpu().numpy()
        for t in range(T):
            idx, val = select_ref(lei[t], 8, lists[t])
            assert np.array_equal(ti[t], idx), (shift, t, ti[t], idx)
            assert np.array_equal(tv[t].view(np.int32), val.view(np.int32)), (shift, t)
        only = gp_ops.predict_pool(b, phi, Xc, latent=True, best_f=bf, log_ei=True, want_mean=False, want_var=False, want_ei=False,
                                   topk=8, exclude=lists)
        assert only["ei"] is None and torch.equal(only["top_idx"], out["top_idx"]) and torch.equal(only["top_val"], out["top_val"])
    # without the flag: the explicit False and the default arguments are the same call
    bf = best.to(dev)
    a = gp_ops.predict_pool(b, phi, Xc, latent=True, best_f=bf, topk=8, exclude=lists, log_ei=False)
    c = gp_ops.predict_pool(b, phi, Xc, latent=True, best_f=bf, topk=8, exclude=lists)
    for name in ("mean", "var", "ei", "top_idx", "top_val"):
        assert torch.equal(a[name], c[name]), name
    q_off = torch.tensor([0, ROWS, ROWS, ROWS, ROWS], dtype=torch.int64, device=dev)
    pa = gp_ops.predict_marginal(b, phi, Xc, q_off, latent=True, best_f=bf, log_ei=False)
    pc = gp_ops.predict_marginal(b, phi, Xc, q_off, latent=True, best_f=bf)
    assert all(torch.equal(x, y) for x, y in zip(pa[:3], pc[:3])) and torch.equal(pc[2], c["ei"][0])
    # consistency with EI where EI is accurate: |exp(log EI) - EI| <= 32 eps32 (1 + u^2) EI for u >= -8
    lg = gp_ops.predict_pool(b, phi, Xc, latent=True, best_f=bf, log_ei=True)
    mean, var, lei, ei = (x.cpu().numpy().astype(np.float64) for x in (lg["mean"], lg["var"], lg["ei"], c["ei"]))
    u = (best.numpy().astype(np.float64)[:, None] - mean) / np.sqrt(np.maximum(var, CLAMP32))
    sel = u >= -8.0
    ratio = np.abs(np.exp(lei[sel]) - ei[sel]) / (EPS32 * (1.0 + u[sel] ** 2) * ei[sel])
    print(f"{kernel}: exp(log EI) vs EI on {int(sel.sum())} rows with u >= -8 (min {u[sel].min():.3g}): worst ratio {ratio.max():.3f} of 32")
    assert sel.sum() > ROWS and (ei[sel] > 0).all() and ratio.max() <= 32.0


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_the_underflow_case_is_fixed(dev, kernel, ns, d):
    """best_f lowered by 30: float32 EI is <= 0 on every row, so the EI call returns the first k eligible row indices; the log-EI
    call returns the oracle's best row for every task whose oracle scores separate the best from the second best by more than
    the bound of test_against_the_oracle (at either row).  At least 3 of the 4 tasks must qualify, which holds for pool seed 8
    (POOL_SEED) by the oracle alone."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = _case(dev, kernel, ns, d)
    bf = (best - 30.0).float()
    lists = [[0, 2], [], [1], [0, 1, 2, 3]]
    plain = gp_ops.predict_pool(b, phi, X, latent=True, best_f=bf.to(dev), topk=8, exclude=lists)
    assert bool((plain["ei"] <= 0).all()), "the premise: EI has underflowed on the whole pool"
    for t in range(T):
        idx, _ = select_ref(plain["ei"][t].cpu().numpy(), 8, lists[t])
        assert np.array_equal(plain["top_idx"][t].cpu().numpy(), idx)
        if bool((plain["ei"][t] == 0).all()):
            assert idx.tolist() == [i for i in range(8 + len(lists[t])) if i not in lists[t]][:8]
    out = gp_ops.predict_pool(b, phi, X, latent=True, best_f=bf.to(dev), log_ei=True, want_mean=False, want_var=False, want_ei=False,
                              topk=8, exclude=lists)
    top = out["top_idx"].cpu().numpy()
    assert bool(torch.isfinite(out["top_val"]).all()) and bool((out["top_val"][:, :-1] > out["top_val"][:, 1:]).all())
    qualified = 0
    for t in range(T):
        ref, u, _ = log_ei_ref(post[t][0], post[t][1], float(bf[t]))
        bound = (1.0 + u * u) * 2 * P.TOL + 1e-4
        ref_x = ref.copy()
        ref_x[lists[t]] = -np.inf
        first, second = np.argsort(-ref_x)[:2]
        gap = ref_x[first] - ref_x[second]
        print(f"{kernel} task {t}: oracle best {first} ({ref_x[first]:.4f}), second {second} ({ref_x[second]:.4f}), gap {gap:.4g}, "
              f"bounds {bound[first]:.3g} + {bound[second]:.3g}, device pick {top[t, 0]}")
        if gap > max(bound[first], bound[second]):
            qualified += 1
            assert top[t, 0] == first, (t, top[t, 0], first)
    assert qualified >= 3, qualified


def test_bo_loops(dev):
    """test_gpu_predict_pool.test_batched_bo_loop's problem, smaller.  Under "log_ei": batched = alone = sequential streaming, six
    distinct picks, and no generator is touched after the initial choice (no random fallback).  Under "ei": the records of the call
    without the argument."""
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(3)
    X = torch.randn(2000, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=2, num_bo_iters=3, kernel_type="matern", device=dev, init_from=1000, noise_init=0.01,
              noise_prior=True)
    R = 3

    def fresh(seed):   # the state after the one initial choice
        rng = np.random.default_rng(seed)
        rng.choice(np.arange(1000, 2000), size=6, replace=False)
        return rng.bit_generator.state

    rngs = [np.random.default_rng(s) for s in range(R)]
    recs = BO.run_gp_ei_bo_batched(X, y, rngs=rngs, acquisition="log_ei", **kw)
    assert len(recs) == R
    for r in range(R):
        assert len(recs[r]) == 1 + 3 * 2 and len(set(recs[r][1:])) == 6
        assert rngs[r].bit_generator.state == fresh(r), (r, "the batched loop fell back to random picks")
        rng = np.random.default_rng(r)
        alone = BO.run_gp_ei_bo_batched(X, y, rngs=[rng], acquisition="log_ei", **kw)
        assert alone[0] == recs[r], (r, "the batch couples replicates")
        assert rng.bit_generator.state == fresh(r)
        rng = np.random.default_rng(r)
        seq = BO.run_gp_ei_bo(X, y, rng=rng, streaming=True, acquisition="log_ei", **kw)
        assert seq == recs[r], (r, "batched vs sequential")
        assert rng.bit_generator.state == fresh(r)
    # the non-streaming sequential path ranks with the host function: a valid record with no fallback either
    rng = np.random.default_rng(0)
    host = BO.run_gp_ei_bo(X, y, rng=rng, streaming=False, acquisition="log_ei", **kw)
    assert len(host) == 7 and len(set(host[1:])) == 6 and rng.bit_generator.state == fresh(0)
    # "ei": what the call without the argument does
    ei_recs = BO.run_gp_ei_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(R)], acquisition="ei", **kw)
    assert ei_recs == BO.run_gp_ei_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(R)], **kw)
    assert BO.run_gp_ei_bo(X, y, rng=np.random.default_rng(1), streaming=True, acquisition="ei", **kw) == \
        BO.run_gp_ei_bo(X, y, rng=np.random.default_rng(1), streaming=True, **kw) == ei_recs[1]
