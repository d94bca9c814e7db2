"""CPU: adkf_gumbel_pool without a GPU - clean refusal with no device, every argument check before any launch, the CPU twin (the same
scheme: probes, clamp and fixed point) on known answers and against the exact quartiles of gumbel_ref.py at the twin's own float32
mean and variance, the structure of the call, and the argument handling of gp_ops.gumbel_pool and of the BO loop's max_value."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
from scipy.special import ndtri

import gumbel_ref as G
from adkf_ift_amd import _lib
from test_predict_pool_cpu import _call, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE = 1, 2
EPS32 = 2.0 ** -24
# The scheme's own error: linear interpolation of log Pr in a cell of the second pass.  The float64 prototype of the two-pass scheme
# stays within 1.1e-4 b of the quartiles found by bisection (rows 1 ... 1e5); four times that for other shapes.  The twin's probes and
# its outputs are float32: 4 eps32 of the largest |quartile| on top (a probe, the interpolated value, the output).
SCHEME = 4 * 1.1e-4


def _tol(q_ref, b_ref):
    return SCHEME * b_ref + 4 * EPS32 * np.abs(q_ref).max()


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, S=5, ard=False, flags=0, x=True, u=True, ystar=True, quant=True, gumbel=True,
               info=True, ws=True, ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(min(rows, 16), 1), d) if x else None
    Sk = min(max(S, 1), 64)
    u_t, ystar_t, quant_t, gumbel_t = torch.full((T, Sk), 0.5), torch.zeros(T, Sk), torch.zeros(T, 3), torch.zeros(T, 2)
    inf = torch.zeros(T, dtype=torch.int32)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_gumbel_pool_scratch_bytes(T)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_gumbel_pool(C.byref(b), p(phi), flags, p(X), rows, p(u_t) if u else None, S, p(ystar_t) if ystar else None,
                                p(quant_t) if quant else None, p(gumbel_t) if gumbel else None, p(inf) if info else None,
                                p(wsb) if ws else None, nb - ws_short, C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_scratch_bytes_depend_on_T_only(lib):
    f = lib.adkf_gumbel_pool_scratch_bytes
    assert f(0) == 0 and f(-1) == 0
    assert 0 < f(1) < f(16) < f(5000) and f(5000) <= 5000 * 1024     # sums, probes and two maxima per task
    assert f(16) % 8 == 0


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, rows=0, x=False, quant=False, gumbel=False) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, S=64, flags=MAXIMIZE) == LAUNCH
    assert _host_call(lib, ard=True, d=12, rows=7, S=1, quant=False) == LAUNCH
    assert _host_call(lib, rows=1 << 27) == LAUNCH                              # the largest pool whose sums cannot wrap


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    for bit in (LATENT, 4, 8, 16, 32):
        assert _host_call(lib, flags=bit) == BADARG                            # flag bits other than MAXIMIZE
        assert _host_call(lib, flags=bit | MAXIMIZE) == BADARG
    assert _host_call(lib, u=False) == BADARG
    assert _host_call(lib, ystar=False) == BADARG
    assert _host_call(lib, info=False) == BADARG
    assert _host_call(lib, ws=False) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    assert _host_call(lib, scratch_off=4) == BADARG                            # a misaligned scratch
    for S in (0, -1, 65):
        assert _host_call(lib, S=S) == SIZE
    assert _host_call(lib, rows=(1 << 27) + 1) == SIZE                         # the fixed-point sums could wrap
    assert _host_call(lib, scratch_short=1) == WORKSPACE
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, ard=True, ws_short=1) == WORKSPACE


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False, T=3, d=5)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.gumbel_pool(types.SimpleNamespace(nq=3, ard=False, T=3, d=5), None, None, n_samples=4)
    with pytest.raises(ValueError, match="n_samples or u"):
        gp_ops.gumbel_pool(iso, None, None)
    for S in (0, 65):
        with pytest.raises(ValueError, match="n_samples must be"):
            gp_ops.gumbel_pool(iso, None, None, n_samples=S)
        with pytest.raises(ValueError, match="number of samples"):
            gp_ops.gumbel_pool(iso, None, None, u=torch.zeros(3, S))
    for bad in (0.5, torch.zeros(4), torch.zeros(4, 4), torch.zeros(3, 4, 1)):
        with pytest.raises(ValueError, match="u must be"):
            gp_ops.gumbel_pool(iso, None, None, u=bad)
    with pytest.raises(ValueError, match="does not match"):
        gp_ops.gumbel_pool(iso, None, None, u=torch.zeros(3, 4), n_samples=5)


def test_an_unknown_max_value_is_refused_first():
    """Before anything touches a device or a generator."""
    from adkf_ift_amd import bayes_opt as BO

    X, y = torch.zeros(8, 2), torch.zeros(8)
    kw = dict(num_init_points=2, query_batch_size=1, num_bo_iters=1, kernel_type="matern", device="cpu", init_from=0, noise_init=0.01,
              noise_prior=True)
    rng = np.random.default_rng(0)
    state = rng.bit_generator.state
    with pytest.raises(ValueError, match="max_value"):
        BO.run_gp_mes_bo_batched(X, y, rngs=[rng], max_value="nope", **kw)
    assert rng.bit_generator.state == state


# ---- the twin
def _gumbel_twin():
    cpu_twin, pool_fn = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_gumbel_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_gumbel_pool"]
    assert tw.adkf_gumbel_pool_scratch_bytes(7) == 0
    return fn, pool_fn


def _problem(T, d, rows, seed, ard=False, kind=1):
    """A ragged batch (the middle task of three is empty) and a pool"""
    from oracle import cpu_twin

    ns = 12
    n_s = np.array([12, 0, 9][:T] if T == 3 else [10], np.int32)
    g = torch.Generator().manual_seed(seed)
    Zs = torch.randn(T, ns, d, generator=g) + 0.7
    ys = torch.randn(T, ns, generator=g)
    X = torch.randn(rows, d, generator=g) + 0.7
    base = torch.tensor([[-2.0, 0.3], [-1.0, 0.0], [-3.0, 0.5]])[:T]
    raw_ls = (1.0 + torch.rand(T, d if ard else 1, generator=g))
    phi = torch.cat([base, raw_ls], 1).numpy().astype(np.float32)
    b = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((T, 4), np.float32), kind, n_s=n_s)
    if ard:
        b.c.flags = ARD
    return b, n_s, np.ascontiguousarray(X.numpy(), np.float32), phi


def gumbel_call(fn, b, phi, flags, X, u, outputs=True):
    """The twin's adkf_gumbel_pool on host arrays: (ystar, quant, gumbel)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    u = np.ascontiguousarray(u, np.float32)
    ystar = np.full(u.shape, np.nan, np.float32)
    quant = np.full((T, 3), np.nan, np.float32) if outputs else None
    gumbel = np.full((T, 2), np.nan, np.float32) if outputs else None
    info = np.empty(T, np.int32)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(u), u.shape[1], pp(ystar), pp(quant), pp(gumbel), pp(info), None, 0, None, 0, None)
    assert rc == 0 and (info == 0).all()
    return ystar, quant, gumbel


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _own_posterior(pool_fn, b, phi, X, maximize):
    """mu (in the score's sense) and sigma from the twin's own float32 latent mean and variance"""
    mean, var, _, _, _ = _call(pool_fn, b, phi, LATENT, X, np.zeros(b.T, np.float32))
    mu = mean.astype(np.float64) if maximize else -mean.astype(np.float64)
    return mu, np.sqrt(np.maximum(var, np.float32(1e-12))).astype(np.float64)


def _check_task(quant, gumbel, mu, sigma, tag):
    q_ref = G.quartiles_exact(mu, sigma)
    a_ref, b_ref = G.gumbel_fit(q_ref)
    tol = _tol(q_ref, b_ref)
    err = np.abs(quant.astype(np.float64) - q_ref).max()
    print(f"{tag}: rows {mu.size}, b {b_ref:.4g}, quartile error {err / b_ref:.3g} b (bound {tol / b_ref:.3g} b)")
    assert err <= tol, (tag, err / b_ref)
    assert abs(gumbel[1] - b_ref) <= 2 * tol / G.DENOM + 2 * EPS32 * b_ref and abs(gumbel[0] - a_ref) <= 2 * tol
    return err / b_ref


def test_the_reference_itself():
    g = np.random.default_rng(0)
    for rows in (1, 7, 1000):
        mu, sigma = g.standard_normal(rows), g.uniform(0.01, 0.9, rows)
        q = G.quartiles_exact(mu, sigma)
        for lq, z in zip(G.LOG_Q, q):
            assert abs(G.log_prob(z, mu, sigma) - lq) < 1e-9
        a, b = G.gumbel_fit(q)
        # two parameters: the fitted Gumbel has the same median and the same interquartile range
        assert abs(G.samples(a, b, 0.5) - q[1]) < 1e-12 * max(1.0, abs(q[1]))
        assert abs((G.samples(a, b, 0.75) - G.samples(a, b, 0.25)) - (q[2] - q[0])) < 1e-12 * max(1.0, q[2] - q[0])
    q = G.quartiles_exact([2.0], [0.5])
    assert np.allclose(q, 2.0 + 0.5 * ndtri([0.25, 0.5, 0.75]), atol=1e-12)
    assert np.isfinite(G.samples(0.0, 1.0, [0.0, 1.0])).all()


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("rows", [1, 64, 65])
def test_known_answers(rows, maximize):
    """rows identical pool rows: Pr = Phi((z - mu) / sigma)^rows, so q = mu + sigma Phi^-1(p^(1 / rows)); rows = 1: mu -+ 0.67449 sigma, mu"""
    fn, pool_fn = _gumbel_twin()
    b, n_s, X, phi = _problem(3, 5, 1, 11)
    X = np.ascontiguousarray(np.repeat(X, rows, 0))
    flags = MAXIMIZE if maximize else 0
    mu, sigma = _own_posterior(pool_fn, b, phi, X, maximize)
    ystar, quant, gumbel = gumbel_call(fn, b, phi, flags, X, np.full((3, 2), 0.5, np.float32))
    for t in (0, 2):
        assert (mu[t] == mu[t, 0]).all() and (sigma[t] == sigma[t, 0]).all()
        q_ref = mu[t, 0] + sigma[t, 0] * ndtri(np.array([0.25, 0.5, 0.75]) ** (1.0 / rows))
        a_ref, b_ref = G.gumbel_fit(q_ref)
        err = np.abs(quant[t] - q_ref).max()
        assert err <= _tol(q_ref, b_ref), (t, err / b_ref)
        if rows == 1:
            assert abs(quant[t, 1] - mu[t, 0]) <= _tol(q_ref, b_ref) and abs((quant[t, 2] - quant[t, 0]) / sigma[t, 0] - 2 * 0.6744897501960817) <= 3 * SCHEME
        # u = 1 / 2 draws the median; ystar is in f's sense
        med = quant[t, 1] if maximize else -quant[t, 1]
        assert np.abs(ystar[t] - med).max() <= 4 * EPS32 * (abs(gumbel[t, 0]) + gumbel[t, 1])


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("T,d", [(1, 5), (3, 8), (3, 5)])
def test_against_the_exact_quartiles(T, d, maximize):
    fn, pool_fn = _gumbel_twin()
    worst = 0.0
    for rows in (1, 2, 63, 64, 65, 130, 1000):
        ard = rows in (63, 130) and T == 3
        b, n_s, X, phi = _problem(T, d, rows, 100 + rows + d, ard=ard)
        mu, sigma = _own_posterior(pool_fn, b, phi, X, maximize)
        u = np.random.default_rng(rows).uniform(size=(T, 6)).astype(np.float32)
        ystar, quant, gumbel = gumbel_call(fn, b, phi, MAXIMIZE if maximize else 0, X, u)
        for t in range(T):
            if n_s[t] == 0:   # skipped: -inf, and the sample that makes adkf_mes_pool's scores NaN
                assert np.isneginf(quant[t]).all() and np.isneginf(gumbel[t]).all()
                assert (np.isneginf(ystar[t]) if maximize else np.isposinf(ystar[t])).all()
                continue
            worst = max(worst, _check_task(quant[t], gumbel[t], mu[t], sigma[t], f"T {T} d {d} rows {rows} ard {ard} task {t}"))
            assert quant[t, 0] <= quant[t, 1] <= quant[t, 2] and gumbel[t, 1] >= 0
            ref = G.samples(float(gumbel[t, 0]), float(gumbel[t, 1]), u[t])
            ref = ref if maximize else -ref
            assert np.abs(ystar[t] - ref).max() <= 8 * EPS32 * (abs(gumbel[t, 0]) + gumbel[t, 1] * np.abs(np.log(-np.log(u[t]))).max())
    print(f"T {T} d {d} maximize {maximize}: worst quartile error {worst:.3g} b")


def test_structure():
    fn, pool_fn = _gumbel_twin()
    b, n_s, X, phi = _problem(3, 5, 130, 21)
    u = np.random.default_rng(1).uniform(size=(3, 7)).astype(np.float32)
    u[0, 0], u[0, 1], u[2, 0], u[2, 1] = 0.0, 1.0, -3.0, 7.0          # clamped to [2^-24, 1 - 2^-24]: finite
    full = gumbel_call(fn, b, phi, 0, X, u)
    for t in (0, 2):
        assert np.isfinite(full[0][t]).all() and np.isfinite(full[1][t]).all() and np.isfinite(full[2][t]).all()
        a_, b_ = float(full[2][t, 0]), float(full[2][t, 1])
        ends = -G.samples(a_, b_, [0.0, 1.0])
        assert np.abs(full[0][t, :2] - ends).max() <= 8 * EPS32 * (abs(a_) + b_ * 17.0)      # |log(-log 2^-24)| < 17
    # quant and gumbel are optional: the same samples
    only = gumbel_call(fn, b, phi, 0, X, u, outputs=False)
    assert only[1] is None and np.array_equal(_bits(only[0]), _bits(full[0]))
    # a permutation of the pool's rows, and the pool split as [A; B] and [B; A]: the same bits
    perm = np.random.default_rng(2).permutation(130)
    for Xp in (X[perm], np.concatenate([X[70:], X[:70]])):
        out = gumbel_call(fn, b, phi, 0, np.ascontiguousarray(Xp), u)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(out, full))
    # a task alone and inside the batch: the same bits
    from oracle import cpu_twin
    for t in (0, 2):
        b1 = cpu_twin.CpuBatch(b.Z_s[t:t + 1], b.y_s[t:t + 1], b.priors[t:t + 1], 1, n_s=n_s[t:t + 1])
        o1 = gumbel_call(fn, b1, phi[t:t + 1], 0, X, u[t:t + 1])
        assert all(np.array_equal(_bits(x[0]), _bits(y[t])) for x, y in zip(o1, full))
    # an empty pool
    ystar, quant, gumbel = gumbel_call(fn, b, phi, MAXIMIZE, X[:0], u)
    assert np.isneginf(ystar).all() and np.isneginf(quant).all() and np.isneginf(gumbel).all()
    ystar, _, _ = gumbel_call(fn, b, phi, 0, X[:0], u)
    assert np.isposinf(ystar).all()


def test_pool_rows_on_support_rows_and_b_equal_to_zero():
    fn, pool_fn = _gumbel_twin()
    b, n_s, X, phi = _problem(3, 5, 40, 31)
    # pool rows that coincide with support rows of task 0: small sigma there, gamma far out on both sides, clamped terms
    X[:12] = b.Z_s[0]
    mu, sigma = _own_posterior(pool_fn, b, phi, X, False)
    u = np.full((3, 3), 0.3, np.float32)
    ystar, quant, gumbel = gumbel_call(fn, b, phi, 0, X, u)
    for t in (0, 2):
        _check_task(quant[t], gumbel[t], mu[t], sigma[t], f"coincident task {t}")
    # one pool row equal to a support row
    X1 = np.ascontiguousarray(b.Z_s[0, 3:4])
    mu, sigma = _own_posterior(pool_fn, b, phi, X1, True)
    ystar, quant, gumbel = gumbel_call(fn, b, phi, MAXIMIZE, X1, u)
    _check_task(quant[0], gumbel[0], mu[0], sigma[0], "one support row")
    # labels so large that lo and hi are one float32: the window is a point, b == 0 and every sample is a
    b.y_s[...] = b.y_s * 1e-3 + 3e8
    ystar, quant, gumbel = gumbel_call(fn, b, phi, MAXIMIZE, X1, u)
    for t in (0, 2):
        assert gumbel[t, 1] == 0 and quant[t, 0] == quant[t, 1] == quant[t, 2] == gumbel[t, 0] and np.isfinite(gumbel[t, 0])
        assert (ystar[t] == gumbel[t, 0]).all()
