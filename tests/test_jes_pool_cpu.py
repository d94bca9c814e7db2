"""CPU: adkf_jes_pool without a GPU - the reference of jes_ref.py against brute-force quadrature and on known answers; the entry is
exported, refuses cleanly with no device and checks every argument before any launch; gp_ops.jes_pool's and the BO loop's argument
handling; the CPU twin against the reference (isotropic and ARD, RBF and Matern, both senses, S = 1, 5 and 64, with repeated and
skipped samples) and the semantics of the call on the twin: S_eff = 0, non-finite values, exclusions and the order of the selection,
skipped tasks, score >= 0."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import believer_ref as B
import gibbon_ref as G
import jes_ref as R
from adkf_ift_amd import _lib
from test_believer_pool_ard_cpu import ard_posterior
from test_predict_pool_cpu import _problem, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE, LOG = 1, 2, 16
EPS32 = R.EPS32


# ---- the reference checks itself
def _toy(seed, rows=5):
    """A small positive-definite latent covariance with its mean: a posterior tuple (m, Sigma, noise, os)."""
    g = np.random.default_rng(seed)
    A = g.normal(size=(rows, rows + 3))
    Sg = A @ A.T / (rows + 3)
    return g.normal(size=rows), Sg, 0.05, float(Sg.diagonal().max())


def test_the_reference_against_quadrature():
    """Every term of a handful of rows and samples against the variance of the truncated, conditioned predictive density by 1-D
    quadrature: the definition itself, with no h and no log1p in it."""
    compared = 0
    for seed, maximize, cn in ((1, True, 1e-6), (2, False, 1e-6), (3, True, 0.3), (4, False, 0.0)):
        post = _toy(seed)
        m, Sg, noise, _ = post
        idx = np.array([0, 3, 3, 4], np.int64)
        val = (m[idx] + (1 if maximize else -1) * np.array([0.1, 0.8, 2.0, -0.3])).astype(np.float32)   # one sample on the "wrong" side
        for s in range(len(idx)):
            one, _, _, _ = R.jes_task(post, idx[s:s + 1], val[s:s + 1], cn, maximize)
            for r in (0, 2, 4):   # two sampled locations and a row beside them
                p = int(idx[s])
                quad = R.term_by_quadrature(m[r], Sg[r, r], Sg[r, p], m[p], Sg[p, p], val[s], noise, cn, maximize)
                assert abs(2.0 * one[r] - quad) <= 1e-10 * max(1.0, abs(quad)), (seed, s, r, 2.0 * one[r], quad)
                compared += 1
        # the score of all samples is the mean of the single-sample scores
        allv, _, _, _ = R.jes_task(post, idx, val, cn, maximize)
        singles = np.mean([R.jes_task(post, idx[s:s + 1], val[s:s + 1], cn, maximize)[0] for s in range(len(idx))], axis=0)
        assert np.abs(allv - singles).max() <= 1e-14 and (allv >= 0).all()
    assert compared == 4 * 4 * 3


def test_the_reference_on_known_answers():
    # a row uncorrelated with every x*_s: GIBBON's a(x) on opt_val
    m, Sg, noise, os_ = _toy(7, rows=8)
    Sg[0, 1:] = 0.0
    Sg[1:, 0] = 0.0
    post = (m, Sg, noise, os_)
    idx, val = np.array([2, 5, 5], np.int64), (m.max() + np.array([0.2, 0.9, 1.7])).astype(np.float32)
    for maximize in (True, False):
        v = val if maximize else (m.min() - np.array([0.2, 0.9, 1.7])).astype(np.float32)
        score, _, _, _ = R.jes_task(post, idx, v, 1e-6, maximize)
        a, _ = G.a_ref(m, Sg.diagonal().copy(), noise, v, maximize)
        assert abs(score[0] - a[0]) <= 1e-15 * max(1.0, a[0]) and a[0] > 0
        # and for every row once the conditioning is switched off by a huge cond_noise
        big, _, _, _ = R.jes_task(post, idx, v, 1e30, maximize)
        assert np.abs(big - a).max() <= 1e-15 * max(1.0, a.max())
    # S = 1, x = x*_s, cond_noise = 0: v_s is at the clamp, and the term is log((v + noise) / (1e-12 + noise)) to rounding
    for r in (1, 4):
        one, _, gamma, _ = R.jes_task(post, np.array([r], np.int64), np.array([m[r] + 0.4], np.float32), 0.0, True)
        want = 0.5 * np.log((Sg[r, r] + noise) / (1e-12 + noise))
        assert abs(one[r] - want) <= 1e-10, (r, one[r], want)
    # skipped samples do not count, a repeated one counts twice
    full, _, _, valid = R.jes_task(post, np.array([2, -1, 5, 99, 5], np.int64), np.array([1.0, 7.0, 1.5, -3.0, 1.5], np.float32), 1e-6, True)
    same, _, _, _ = R.jes_task(post, np.array([2, 5, 5], np.int64), np.array([1.0, 1.5, 1.5], np.float32), 1e-6, True)
    assert valid == [2, -1, 5, -1, 5] and np.array_equal(full, same)
    # no valid sample, or a non-finite value on a valid one: NaN
    assert np.isnan(R.jes_task(post, np.array([-1, 8], np.int64), np.array([1.0, 1.0], np.float32), 1e-6, True)[0]).all()
    assert np.isnan(R.jes_task(post, np.array([2, 3], np.int64), np.array([1.0, np.inf], np.float32), 1e-6, True)[0]).all()
    assert np.isfinite(R.jes_task(post, np.array([2, -1], np.int64), np.array([1.0, np.nan], np.float32), 1e-6, True)[0]).all()
    # the fast h of the derived bound against the 50-digit one
    g = np.concatenate([np.linspace(-30, 8, 77), [-1.0, 0.0, 1e-3, -1e-3]])
    assert np.abs(R.h64(g) - G._hrefv(g)).max() <= 1e-12


# ---- the entry of the device library
def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, S=4, k=3, ard=False, flags=0, x=True, idx=True, val=True, cond_noise=1e-6,
               outs=(True, False, False), top=(True, True), excl=(False, False), info=True, ws=True, ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    Sm, kk = min(max(S, 1), 64), min(max(k, 0), 64)
    idx_t, val_t = torch.zeros(T, Sm, dtype=torch.int64), torch.zeros(T, Sm)
    score, omean, ovar = torch.zeros(T * max(rows, 1)), torch.zeros(T * Sm), torch.zeros(T * Sm)
    inf = torch.zeros(T, dtype=torch.int32)
    top_idx, top_val = torch.zeros(T * max(kk, 1), dtype=torch.int64), torch.zeros(T * max(kk, 1))
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_jes_pool_scratch_bytes(T, ns, d, Sm, kk)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_jes_pool(C.byref(b), p(phi), flags, p(X), rows, p(idx_t) if idx else None, p(val_t) if val else None, S, cond_noise,
                             p(e_idx) if excl[0] else None, p(e_off) if excl[1] else None, p(score) if outs[0] else None,
                             p(omean) if outs[1] else None, p(ovar) if outs[2] else None, k, p(top_idx) if top[0] else None,
                             p(top_val) if top[1] else None, p(inf) if info else None, p(wsb) if ws else None, nb - ws_short,
                             C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_the_entry_is_exported(lib):
    assert "adkf_jes_pool" in _lib.SIGNATURES and "adkf_jes_pool_scratch_bytes" in _lib.SIGNATURES
    fn = lib.adkf_jes_pool   # a library without the entry point fails here
    assert fn.restype is C.c_int and len(fn.argtypes) == 23 and fn.argtypes[8] is C.c_float


def test_the_scratch_size(lib):
    f = lib.adkf_jes_pool_scratch_bytes
    base = f(3, 16, 8, 4, 0)
    # the knowledge gradient's reference state for M = S, three more [T, S] arrays and a scale per task (each padded to the arena's 256 bytes)
    kg = lib.adkf_kg_pool_scratch_bytes(3, 16, 8, 4, 0)
    assert base >= kg + 4 * (3 * 3 * 4 + 3) and base - kg <= 4 * (3 * 3 * 4 + 3) + 4 * 256 and base % 8 == 0
    assert 0 <= f(3, 16, 8, 4, 5) - base - lib.adkf_predict_pool_scratch_bytes(3, 5) < 512   # prediction's lists behind the state
    # monotone in every argument; rows is not an argument
    assert f(3, 16, 8, 8, 0) > base and f(3, 32, 8, 4, 0) > base and f(3, 16, 16, 4, 0) > base and f(4, 16, 8, 4, 0) > base
    assert f(3, 16, 8, 4, 64) > f(3, 16, 8, 4, 5) > base
    assert all(f(3, 16, 8, S + 1, 2) >= f(3, 16, 8, S, 2) for S in range(1, 64)) and f(3, 16, 8, 64, 2) > f(3, 16, 8, 1, 2)
    for bad in ((0, 16, 8, 4, 0), (3, 0, 8, 4, 0), (3, 16, 0, 4, 0), (3, 16, 8, 0, 0), (3, 16, 8, 65, 0), (3, 16, 8, 4, -1), (3, 16, 8, 4, 65)):
        assert f(*bad) == 0, bad


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0, x=False) == LAUNCH
    assert _host_call(lib, ard=True, d=12, rows=7, S=1, k=0, cond_noise=0.0) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, S=64, k=64, outs=(True, True, True), excl=(True, True), flags=MAXIMIZE, cond_noise=1e30) == LAUNCH
    assert _host_call(lib, k=0, outs=(False, True, False), top=(False, False)) == LAUNCH
    assert _host_call(lib, k=0, outs=(False, False, True), top=(False, False)) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    assert _host_call(lib, idx=False) == BADARG
    assert _host_call(lib, val=False) == BADARG
    for cn in (-1e-6, -1.0, float("nan"), float("inf"), -float("inf")):
        assert _host_call(lib, cond_noise=cn) == BADARG, cn
    assert _host_call(lib, info=False) == BADARG
    assert _host_call(lib, ws=False) == BADARG
    assert _host_call(lib, excl=(True, False)) == BADARG                       # excl_idx without excl_off
    assert _host_call(lib, k=-1) == BADARG
    assert _host_call(lib, top=(False, True)) == BADARG
    assert _host_call(lib, top=(True, False)) == BADARG
    assert _host_call(lib, k=0, outs=(False, False, False)) == BADARG          # no output at all
    assert _host_call(lib, scratch_off=4) == BADARG                            # a misaligned scratch
    for bit in (LATENT, 4, 8, LOG, 32):
        assert _host_call(lib, flags=bit) == BADARG                            # flag bits other than MAXIMIZE
        assert _host_call(lib, flags=bit | MAXIMIZE) == BADARG
    for S in (0, -2, 65):
        assert _host_call(lib, S=S) == SIZE
    assert _host_call(lib, k=65) == SIZE
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, ard=True, ws_short=1) == WORKSPACE
    assert _host_call(lib, scratch_short=1) == WORKSPACE


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False, T=3, d=5)
    idx, val = torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, 4)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.jes_pool(types.SimpleNamespace(nq=3, ard=False, T=3, d=5), None, None, opt_idx=idx, opt_val=val)
    for k in (-1, 65):
        with pytest.raises(ValueError, match="topk must be"):
            gp_ops.jes_pool(iso, None, None, opt_idx=idx, opt_val=val, topk=k)
    for bad in (torch.zeros(3, 4), torch.zeros(4, dtype=torch.int64), torch.zeros(4, 4, dtype=torch.int64), [[1, 2]] * 3):
        with pytest.raises(ValueError, match="opt_idx must be"):
            gp_ops.jes_pool(iso, None, None, opt_idx=bad, opt_val=val)
    for S in (0, 65):
        with pytest.raises(ValueError, match="optimum samples S must be"):
            gp_ops.jes_pool(iso, None, None, opt_idx=torch.zeros(3, S, dtype=torch.int64), opt_val=torch.zeros(3, S))
    for bad in (torch.zeros(3, 5), torch.zeros(4), [[0.0] * 4] * 3):
        with pytest.raises(ValueError, match="opt_val must be"):
            gp_ops.jes_pool(iso, None, None, opt_idx=idx, opt_val=bad)
    for cn in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cond_noise must be"):
            gp_ops.jes_pool(iso, None, None, opt_idx=idx, opt_val=val, cond_noise=cn)


def test_the_bo_loop_checks_its_arguments():
    from adkf_ift_amd import bayes_opt as BO

    X, y = torch.randn(20, 3), torch.randn(20)
    for q in (0, 65):
        with pytest.raises(ValueError, match="query_batch_size must be"):
            BO.run_gp_jes_bo_batched(X, y, 4, q, 1, "matern", "cpu", 10, 0.01, True, rngs=[np.random.default_rng(0)])
    for n in (0, 65):
        with pytest.raises(ValueError, match="n_opt_samples must be"):
            BO.run_gp_jes_bo_batched(X, y, 4, 2, 1, "matern", "cpu", 10, 0.01, True, rngs=[np.random.default_rng(0)], n_opt_samples=n)
    for cn in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cond_noise must be"):
            BO.run_gp_jes_bo_batched(X, y, 4, 2, 1, "matern", "cpu", 10, 0.01, True, rngs=[np.random.default_rng(0)], cond_noise=cn)


# ---- the twin
def _jes_twin():
    cpu_twin, _ = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_jes_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_jes_pool"]
    sb = tw.adkf_jes_pool_scratch_bytes
    sb.restype, sb.argtypes = _lib.SIGNATURES["adkf_jes_pool_scratch_bytes"]
    assert sb(3, 16, 8, 4, 5) == 0
    return fn


def jes_call(fn, b, phi, flags, X, opt_idx, opt_val, cond_noise=1e-6, k=0, excl=None, want=(True, True, True), ok=True):
    """The twin's adkf_jes_pool on host arrays: (score, opt_mean, opt_var, top_idx, top_val, info)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    opt_idx = np.ascontiguousarray(opt_idx, np.int64)
    opt_val = np.ascontiguousarray(opt_val, np.float32)
    S = opt_idx.shape[1]
    score = np.full((T, rows), -7.0, np.float32) if want[0] else None
    omean = np.full((T, S), np.nan, np.float32) if want[1] else None
    ovar = np.full((T, S), np.nan, np.float32) if want[2] else None
    info = np.empty(T, np.int32)
    top_idx = np.full((T, max(k, 1)), -7, np.int64)
    top_val = np.full((T, max(k, 1)), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(opt_idx), pp(opt_val), S, cond_noise, pp(e_idx), pp(e_off), pp(score), pp(omean),
            pp(ovar), k, pp(top_idx) if k else None, pp(top_val) if k else None, pp(info), None, 0, None, 0, None)
    assert rc == 0
    if ok:
        assert (info == 0).all()
    return score, omean, ovar, top_idx, top_val, info


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _posts(b, Zs, ys, n_s, X, phi, kind, ard):
    return [(ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], X, phi[t], kind) if ard else
             B.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], kind)) for t in range(b.T)]


def check_twin_task(post, idx_t, val_t, cond_noise, maximize, score, omean, ovar, tag):
    """The twin rounds a float64 evaluation to float32 at the boundary; its posterior and the oracle's differ by float64 rounding
    through a solve of condition (os + noise) / noise <= 1e3, and the cancellation of v - c^2 / d at a sampled location amplifies that
    by at most os / noise in the logarithm: 1e-8 is generous.  So |score - ref| <= 2 eps32 |ref| + 1e-8, and
    |opt_mean - m| <= 2 eps32 |m| + 1e-9, |opt_var - v| <= 2 eps32 |v| + 1e-9 os."""
    m, S, _, os_ = post
    ref, delta, _, valid = R.jes_task(post, idx_t, val_t, cond_noise, maximize)
    err = np.abs(score.astype(np.float64) - ref)
    assert (err <= 2 * EPS32 * np.abs(ref) + 1e-8).all(), (tag, float(err.max()))
    for j, p in enumerate(valid):
        if p < 0:
            assert omean[j] == 0 and ovar[j] == 0, (tag, j)
        else:
            assert abs(omean[j] - m[p]) <= 2 * EPS32 * abs(m[p]) + 1e-9, (tag, j)
            assert abs(ovar[j] - S[p, p]) <= 2 * EPS32 * abs(S[p, p]) + 1e-9 * os_, (tag, j)
    return ref, delta


CASES = [(0, False, 1), (1, False, 5), (0, True, 5), (1, True, 64), (0, False, 64)]   # (kind, ARD, S)


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("kind,ard,S", CASES)
def test_cpu_twin_against_the_reference(kind, ard, S, maximize):
    """Also the check the GPU test relies on: on these problems the derived bound is informative - the median over the rows of
    delta / max(score, 1e-3) is below 0.5."""
    fn = _jes_twin()
    rows = 40
    b, Zs, ys, n_s, X, phi, _ = _problem(kind, ard, 60 + kind + 2 * ard, rows=rows)
    posts = _posts(b, Zs, ys, n_s, X, phi, kind, ard)
    for messy, cns in ((False, (1e-6,)), (True, (0.0, 0.05))) if S < 64 else ((True, (1e-6,)),):
        pairs = [R.samples_for(posts[t], S, rows, maximize, 11 + t, messy=messy) for t in range(b.T)]
        idx, val = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        for cn in cns:
            score, omean, ovar, _, _, _ = jes_call(fn, b, phi, MAXIMIZE if maximize else 0, X, idx, val, cond_noise=cn)
            for t in range(b.T):
                ref, delta = check_twin_task(posts[t], idx[t], val[t], cn, maximize, score[t], omean[t], ovar[t], (kind, ard, S, maximize, messy, cn, t))
                assert (score[t] >= 0).all()
                med = float(np.median(delta / np.maximum(ref, 1e-3)))
                assert med < 0.5, ("a vacuous bound", kind, ard, S, maximize, t, med)


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_the_gpu_problems_have_an_informative_bound(case):
    """Before tests/test_gpu_jes_pool.py relies on it: on each of its reference problems, with its samples, the median over the rows of
    delta / max(score, 1e-3) is below 0.5 and noise >= 1e-2 os; the twin agrees with the reference there."""
    fn = _jes_twin()
    from oracle import cpu_twin

    kernel, n_s, d, rows, S, maximize = R.CASES[case]
    kind = {"rbf": 0, "matern": 1}[kernel]
    Zs, ys, X, phi = R.problem(n_s, d, rows, 900 + case)
    b = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((len(n_s), 4), np.float32), kind, n_s=np.array(n_s, np.int32))
    Xh, ph = np.ascontiguousarray(X.numpy()), phi.numpy()
    posts = _posts(b, Zs, ys, n_s, Xh, ph, kind, False)
    pairs = [R.samples_for(posts[t], S, rows, maximize, 31 + t, messy=True) for t in range(b.T)]
    idx, val = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    score, _, _, _, _, _ = jes_call(fn, b, ph, MAXIMIZE if maximize else 0, Xh, idx, val)
    for t in range(b.T):
        assert posts[t][2] >= 1e-2 * posts[t][3]
        ref, delta, _, _ = R.jes_task(posts[t], idx[t], val[t], 1e-6, maximize, fast=True)
        med = float(np.median(delta / np.maximum(ref, 1e-3)))
        print(f"case {case} task {t}: median delta / max(score, 1e-3) = {med:.4f}, score in [{ref.min():.4g}, {ref.max():.4g}]")
        assert med < 0.5, (case, t, med)
        assert (np.abs(score[t] - ref) <= 2 * EPS32 * np.abs(ref) + 1e-8).all() and (score[t] >= 0).all()


def test_no_valid_sample_and_non_finite_values():
    fn = _jes_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(1, False, 44, rows=12)
    posts = _posts(b, Zs, ys, n_s, X, phi, 1, False)
    idx = np.array([[3, 7, 3, 0], [-1, 12, -5, 400], [5, -1, 11, 2]], np.int64)
    val = np.array([[0.5, 0.7, 0.9, 1.1], [0.5, np.nan, np.inf, 0.2], [0.3, np.nan, 0.8, 1.0]], np.float32)   # a NaN on a skipped entry is not read
    score, omean, ovar, top_idx, top_val, _ = jes_call(fn, b, phi, MAXIMIZE, X, idx, val, k=4)
    assert np.isnan(score[1]).all() and (top_idx[1] == -1).all() and np.isneginf(top_val[1]).all() and (omean[1] == 0).all() and (ovar[1] == 0).all()
    for t in (0, 2):
        check_twin_task(posts[t], idx[t], val[t], 1e-6, True, score[t], omean[t], ovar[t], ("S_eff", t))
        assert (top_idx[t] >= 0).all()
    for badv in (np.nan, np.inf, -np.inf):
        v2 = val.copy()
        v2[2, 2] = badv
        s2, _, _, ti2, tv2, _ = jes_call(fn, b, phi, MAXIMIZE, X, idx, v2, k=4)
        assert np.isnan(s2[2]).all() and (ti2[2] == -1).all() and np.isneginf(tv2[2]).all()
        assert np.array_equal(_bits(s2[0]), _bits(score[0])) and np.array_equal(ti2[0], top_idx[0])   # that task only


def test_exclusions_the_order_and_a_skipped_task():
    fn = _jes_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(1, False, 46, rows=70)
    X[10] = X[3]; X[41] = X[3]          # exact duplicate rows: equal scores, ascending index
    posts = _posts(b, Zs, ys, n_s, X, phi, 1, False)
    pairs = [R.samples_for(posts[t], 6, 70, False, 3 + t, messy=True) for t in range(b.T)]
    idx, val = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    lists = [[5, 6, 17], [], sorted(set(range(70)) - {3, 10, 41, 50})]
    excl = (np.array([i for l in lists for i in l], np.int64), np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64))
    k = 8
    score, _, _, top_idx, top_val, _ = jes_call(fn, b, phi, 0, X, idx, val, k=k, excl=excl)
    for t in range(b.T):
        wi, wv = R.topk_of(score[t], k, lists[t])
        assert np.array_equal(top_idx[t], wi) and np.array_equal(_bits(top_val[t]), _bits(wv)), t
        assert _bits(score[t, 3]) == _bits(score[t, 10]) == _bits(score[t, 41])
    assert (top_idx[2, 4:] == -1).all() and np.isneginf(top_val[2, 4:]).all()
    # score == NULL: the same selection
    _, _, _, ti2, tv2, _ = jes_call(fn, b, phi, 0, X, idx, val, k=k, excl=excl, want=(False, False, False))
    assert np.array_equal(ti2, top_idx) and np.array_equal(_bits(tv2), _bits(top_val))
    full = jes_call(fn, b, phi, 0, X, idx, val, k=4)
    b.n_s[1] = 0                        # a skipped task: zero slices, -1 / -inf; the others do not see it
    score, omean, ovar, top_idx, top_val, info = jes_call(fn, b, phi, 0, X, idx, val, k=4)
    assert (score[1] == 0).all() and (omean[1] == 0).all() and (ovar[1] == 0).all() and (top_idx[1] == -1).all() and np.isneginf(top_val[1]).all()
    for t in (0, 2):
        assert np.array_equal(_bits(score[t]), _bits(full[0][t])) and np.array_equal(top_idx[t], full[3][t])
    # a NaN pool row that is no sampled location scores NaN, is never selected, and its neighbours keep their bits
    b.n_s[1] = 7
    bad = next(r for r in range(70) if r not in set(idx.flatten().tolist()))
    Xn = X.copy()
    Xn[bad] = np.nan
    sn, _, _, tin, _, _ = jes_call(fn, b, phi, 0, Xn, idx, val, k=64)
    s0 = jes_call(fn, b, phi, 0, X, idx, val)[0]
    assert np.isnan(sn[:, bad]).all() and not (tin == bad).any() and np.array_equal(_bits(np.delete(sn, bad, axis=1)), _bits(np.delete(s0, bad, axis=1)))
    # an empty pool: no sample is valid
    e0, m0, v0, ti0, tv0, _ = jes_call(fn, b, phi, 0, X[:0], idx, val, k=3)
    assert e0.shape == (b.T, 0) and (m0 == 0).all() and (v0 == 0).all() and (ti0 == -1).all() and np.isneginf(tv0).all()
