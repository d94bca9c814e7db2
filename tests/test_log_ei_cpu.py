"""CPU: log EI (ADKF_PM_LOG_EI) without a GPU - the argument checks of the HIP library with no device, the CPU twin against
the float64 oracle fed to an mpmath log h(u), the selection on the twin where float32 EI is 0 on every row, and
bayes_opt.log_expected_improvement against mpmath.  ``log_h_ref`` / ``log_ei_ref`` are the one reference of log EI; the GPU tests
import them from here."""
import ctypes as C
import math

import mpmath
import numpy as np
import pytest
import torch

from adkf_ift_amd import _lib
from test_predict_pool_cpu import _call, _host_call, _problem, _twin, lib, select_ref  # noqa: F401  (lib: the fixture)

BADARG, LAUNCH = -1, -4
ARD = 4
LATENT, MAXIMIZE, SCORE_MEAN, LOG_EI = 1, 2, 4, 16
EPS32 = float(np.finfo(np.float32).eps)
SHIFTS = (0.0, 8.0, 30.0, 300.0)


def log_h_ref(u):
    """log(phi(u) + u Phi(u)) at 50 digits, elementwise over a float64 array; rounded to float64."""
    u = np.asarray(u, np.float64)
    out = np.empty(u.shape, np.float64)
    with mpmath.workdps(50):
        for i, x in np.ndenumerate(u):
            x = mpmath.mpf(float(x))
            out[i] = float(mpmath.log(mpmath.npdf(x) + x * mpmath.ncdf(x)))
    return out


def log_ei_ref(mean, var_latent, best, maximize=False, clamp=1e-12):
    """(log sigma + log h(u), u, log sigma) with sigma = sqrt(max(var_latent, clamp)) and u = +-(best - mean) / sigma formed in
    float64 from the arrays given."""
    mean, var_latent = np.asarray(mean, np.float64), np.asarray(var_latent, np.float64)
    sigma = np.sqrt(np.maximum(var_latent, clamp))
    u = ((mean - best) if maximize else (best - mean)) / sigma
    return np.log(sigma) + log_h_ref(u), u, np.log(sigma)


def test_the_reference_itself():
    """Known values: h(0) = phi(0); the issue's EI(u = -14) = 5.5e-46 and EI(u = -15) = 2.4e-52 at sigma = 1; h(u) -> u for large u."""
    assert abs(log_h_ref(0.0) - math.log(1.0 / math.sqrt(2.0 * math.pi))) < 1e-15
    assert abs(math.exp(float(log_h_ref(-14.0))) / 5.5e-46 - 1.0) < 0.02
    assert abs(math.exp(float(log_h_ref(-15.0))) / 2.4e-52 - 1.0) < 0.02
    assert abs(log_h_ref(50.0) - math.log(50.0)) < 1e-15


def _packed_host_call(lib, entry, flags, ei=True, best=True, T=3, ns=16, d=8, rows=10):
    """adkf_predict_marginal(_ard) on host memory (nothing is dereferenced before the first launch)."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ard = entry.endswith("_ard")
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq, q_off = torch.zeros(rows, d), torch.zeros(T + 1, dtype=torch.int64)
    out = [torch.zeros(rows) for _ in range(3)]
    info, bf = torch.zeros(T, dtype=torch.int32), torch.zeros(T)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    ws = torch.zeros(nb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, 0, d, 0, ARD if ard else 0
    b.n_s = b.n_q = b.Z_q = b.y_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    return getattr(lib, entry)(C.byref(b), p(phi), flags, p(Zq), p(q_off), rows, p(bf) if best else None, p(out[0]), p(out[1]),
                               p(out[2]) if ei else None, p(info), p(ws), nb, None)


def test_flag_checks_come_before_any_launch(lib):
    import test_thompson_pool_ard_cpu as TA
    import test_thompson_pool_cpu as TS

    assert _lib.PM_LOG_EI == LOG_EI
    for entry in ("adkf_predict_marginal", "adkf_predict_marginal_ard"):
        assert _packed_host_call(lib, entry, LOG_EI, ei=False) == BADARG                  # the flag without ei
        assert _packed_host_call(lib, entry, LOG_EI | LATENT, ei=False) == BADARG
        assert _packed_host_call(lib, entry, LOG_EI, ei=True, best=False) == BADARG       # ei without best_f, as before
        assert _packed_host_call(lib, entry, 8) == BADARG                                 # bit 8 stays unknown
        assert _packed_host_call(lib, entry, 8 | LOG_EI) == BADARG
        assert _packed_host_call(lib, entry, 32 | LOG_EI) == BADARG
    # the pool call: the flag with ei == NULL and no selection that ranks by EI
    assert _host_call(lib, flags=LOG_EI) == BADARG                                        # k == 0
    assert _host_call(lib, flags=LOG_EI, best=True) == BADARG
    assert _host_call(lib, flags=LOG_EI | SCORE_MEAN, k=4) == BADARG                      # ranking by the mean
    assert _host_call(lib, flags=LOG_EI | SCORE_MEAN | MAXIMIZE, k=4, best=True) == BADARG
    assert _host_call(lib, flags=LOG_EI, k=4, best=False) == BADARG                       # ranking by log EI without best_f
    assert _host_call(lib, flags=LOG_EI, ei=True, best=False) == BADARG
    assert _host_call(lib, flags=8) == BADARG and _host_call(lib, flags=8 | LOG_EI, ei=True, best=True) == BADARG
    # both Thompson entries keep rejecting every bit but MAXIMIZE
    assert TS._host_call(lib, flags=LOG_EI) == BADARG and TS._host_call(lib, flags=LOG_EI | MAXIMIZE) == BADARG
    assert TA._host_call(lib, flags=LOG_EI) == BADARG and TA._host_call(lib, flags=LOG_EI | MAXIMIZE) == BADARG


def test_valid_flag_sets_reach_the_launch(lib):
    """Without a device a call that passes every check fails at its first launch: ADKF_E_LAUNCH."""
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    for entry in ("adkf_predict_marginal", "adkf_predict_marginal_ard"):
        assert _packed_host_call(lib, entry, LOG_EI) == LAUNCH
        assert _packed_host_call(lib, entry, LOG_EI | LATENT | MAXIMIZE) == LAUNCH
    assert _host_call(lib, flags=LOG_EI, ei=True, best=True) == LAUNCH                                     # per row only
    assert _host_call(lib, flags=LOG_EI, k=4, best=True, mean=False, var=False) == LAUNCH                  # the selection only
    assert _host_call(lib, flags=LOG_EI | SCORE_MEAN, ei=True, k=4, best=True) == LAUNCH                   # ei reads it
    assert _host_call(lib, flags=LOG_EI | LATENT | MAXIMIZE, ard=True, d=12, ei=True, k=64, best=True) == LAUNCH


def _oracle_mean_vl(Zs, ys, n_s, X, phi, kind, t):
    """The float64 oracle's mean and latent variance of the pool rows for task t (phi[t] of 2 + d entries: one lengthscale each)."""
    from oracle import gp_oracle as O

    n = n_s[t]
    pt = torch.from_numpy(phi[t]).double()
    m_ref, cov = O.predict(Zs[t, :n].double(), ys[t, :n].double(), torch.from_numpy(X).double(), pt, kind)
    return m_ref.numpy(), cov.diagonal().numpy() - float(O.transform_phi(pt)[0])


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_twin_against_the_oracle(kind, ard):
    """|got - ref| <= 8 eps32 max(1, |ref|): the twin works in double, what is left is the rounding of its float output."""
    _, fn = _twin()
    b, Zs, ys, n_s, X, phi, best0 = _problem(kind, ard, 30 + kind + 2 * ard)
    seen = []
    for shift in SHIFTS:
        best = (best0 - np.float32(shift)).astype(np.float32)
        post = [_oracle_mean_vl(Zs, ys, n_s, X, phi, kind, t) for t in range(b.T)]
        for flags in (LOG_EI, LOG_EI | MAXIMIZE, LOG_EI | LATENT):
            mean, var, lei, _, _ = _call(fn, b, phi, flags, X, best)
            for t in range(b.T):
                ref, u, _ = log_ei_ref(post[t][0], post[t][1], float(best[t]), bool(flags & MAXIMIZE))
                assert np.isfinite(lei[t]).all() and np.isfinite(ref).all()
                err = np.abs(lei[t].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
                assert err.max() <= 8 * EPS32, (shift, flags, t, err.max() / EPS32, u[err.argmax()])
                if not flags & MAXIMIZE:
                    seen.append((shift, u.min(), u.max()))
        if shift == 30.0:   # the premise of the feature: float32 EI is no longer positive anywhere
            _, _, ei, _, _ = _call(fn, b, phi, 0, X, best)
            assert (ei <= 0).all()
    # the shifts reach all three ranges of the evaluation: around 0, the cancelling bracket, the asymptotic series
    lo = {s: min(a for q, a, _ in seen if q == s) for s in SHIFTS}
    hi = {s: max(c for q, _, c in seen if q == s) for s in SHIFTS}
    assert hi[0.0] > 0 and lo[0.0] > -12 and lo[8.0] < -8 and hi[8.0] < -1 and hi[30.0] < -12 and hi[300.0] < -100, (lo, hi)


@pytest.mark.parametrize("ard", [False, True])
def test_packed_twin_equals_pool_twin(ard):
    """adkf_predict_marginal(_ard) of the twin under the flag: the pool call's values, bit for bit."""
    cpu_twin, fn = _twin()
    b, Zs, ys, n_s, X, phi, best0 = _problem(1, ard, 50 + ard)
    best = (best0 - np.float32(8.0)).astype(np.float32)
    _, _, lei, _, _ = _call(fn, b, phi, LOG_EI | LATENT, X, best)
    packed = getattr(cpu_twin.load(), "adkf_predict_marginal_ard" if ard else "adkf_predict_marginal")
    pp = lambda a: a.ctypes.data_as(C.c_void_p)
    rows = X.shape[0]
    for t in range(b.T):
        q_off = np.array([0] * (t + 1) + [rows] * (b.T - t), np.int64)
        mean, var, ei = (np.full(rows, np.nan, np.float32) for _ in range(3))
        info = np.empty(b.T, np.int32)
        assert packed(C.byref(b.c), pp(phi), LOG_EI | LATENT, pp(X), pp(q_off), rows, pp(best), pp(mean), pp(var), pp(ei), pp(info),
                      None, 0, None) == 0
        assert np.array_equal(ei.view(np.int32), lei[t].view(np.int32)), t
        assert packed(C.byref(b.c), pp(phi), LOG_EI, pp(X), pp(q_off), rows, pp(best), pp(mean), pp(var), None, pp(info), None, 0,
                      None) == BADARG
    assert fn(C.byref(b.c), pp(phi), LOG_EI | SCORE_MEAN, pp(X), rows, pp(best), None, None, pp(mean), None, None, 0, None, None,
              pp(info), None, 0, None, 0, None) == BADARG


@pytest.mark.parametrize("ard", [False, True])
def test_selection_on_the_twin(ard):
    _, fn = _twin()
    b, Zs, ys, n_s, X, phi, best0 = _problem(1, ard, 40 + ard, rows=70)
    lists = [[0, 5, 6], [], sorted(set(range(70)) - {3, 10, 41, 50, 51, 60, 66})]
    e_idx = np.array([i for l in lists for i in l], np.int64)
    e_off = np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64)
    k = 5
    for shift in (0.0, 30.0):
        best = (best0 - np.float32(shift)).astype(np.float32)
        for flags in (LOG_EI | LATENT, LOG_EI | LATENT | MAXIMIZE, LOG_EI):
            _, _, lei, top_idx, top_val = _call(fn, b, phi, flags, X, best, k=k, excl=(e_idx, e_off))
            for t in range(b.T):
                idx, val = select_ref(lei[t], k, lists[t])
                assert np.array_equal(top_idx[t], idx), (shift, flags, t)
                assert np.array_equal(top_val[t].view(np.int32), val.view(np.int32)), (shift, flags, t)
            _, _, _, ti2, tv2 = _call(fn, b, phi, flags, X, best, k=k, excl=(e_idx, e_off), per_row=False)   # selection only
            assert np.array_equal(ti2, top_idx) and np.array_equal(tv2.view(np.int32), top_val.view(np.int32))
        if shift == 30.0:
            _, _, _, _, ei_val = _call(fn, b, phi, LATENT, X, best, k=k, excl=(e_idx, e_off))
            assert (ei_val <= 0).all()                       # ranked by EI: nothing left to rank
            _, _, _, top_idx, top_val = _call(fn, b, phi, LOG_EI | LATENT, X, best, k=k, excl=(e_idx, e_off))
            assert np.isfinite(top_val).all() and (np.diff(top_val, axis=1) < 0).all()   # ranked by log EI: five distinct scores
            assert all(len(set(r)) == k and min(r) >= 0 for r in top_idx.tolist())


def _u_grid():
    return np.concatenate([np.linspace(6.0, -1.0, 57), -np.linspace(1.0, 40.0, 157), -np.logspace(math.log10(40.0), 6.0, 60)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("maximize", [False, True])
def test_host_function_against_mpmath(dtype, maximize):
    """bayes_opt.log_expected_improvement: |got - ref| <= 8 eps(dtype) max(1, |ref|), ref from the inputs as the dtype holds them."""
    from adkf_ift_amd.bayes_opt import log_expected_improvement

    eps = float(torch.finfo(dtype).eps)
    u = _u_grid()
    best = 0.25
    for sigma in (1e-6, 1e-3, 1.0):
        var = torch.full((u.size,), sigma * sigma, dtype=dtype)
        mean = torch.from_numpy(best + (u if maximize else -u) * sigma).to(dtype)
        got = log_expected_improvement(mean, var, best, maximize=maximize)
        assert got.dtype == dtype and got.shape == mean.shape
        ref, uu, _ = log_ei_ref(mean.double().numpy(), var.double().numpy(), best, maximize, clamp=0.0)
        assert uu.min() < -0.9e6 and uu.max() > 5.9
        err = np.abs(got.double().numpy() - ref) / np.maximum(1.0, np.abs(ref))
        assert np.isfinite(got.numpy()).all() and err.max() <= 8 * eps, (sigma, err.max() / eps, uu[err.argmax()])


def test_host_function_matches_expected_improvement():
    from adkf_ift_amd.bayes_opt import expected_improvement, log_expected_improvement

    u = torch.linspace(-5.0, 6.0, 441, dtype=torch.float64)
    for sigma in (1e-3, 1.0):
        for maximize in (False, True):
            mean, var = (u if maximize else -u) * sigma + 0.5, torch.full_like(u, sigma * sigma)
            ei = expected_improvement(mean, var, 0.5, maximize=maximize)
            lei = log_expected_improvement(mean, var, 0.5, maximize=maximize)
            assert bool(((lei.exp() - ei).abs() <= 1e-5 * ei).all())
    nan = log_expected_improvement(torch.tensor([float("nan"), 0.0]), torch.ones(2), 0.0)
    assert bool(torch.isnan(nan[0])) and bool(torch.isfinite(nan[1]))


def test_an_unknown_acquisition_is_refused_first():
    """Before anything touches a device or a generator."""
    from adkf_ift_amd import bayes_opt as BO

    X, y = torch.zeros(8, 2), torch.zeros(8)
    kw = dict(num_init_points=2, query_batch_size=1, num_bo_iters=1, kernel_type="matern", device="cpu", init_from=0, noise_init=0.01,
              noise_prior=True)
    rng = np.random.default_rng(0)
    state = rng.bit_generator.state
    with pytest.raises(ValueError, match="acquisition"):
        BO.run_gp_ei_bo(X, y, rng=rng, acquisition="nope", **kw)
    with pytest.raises(ValueError, match="acquisition"):
        BO.run_gp_ei_bo_batched(X, y, rngs=[rng], acquisition="nope", **kw)
    assert rng.bit_generator.state == state
