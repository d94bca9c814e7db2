"""CPU: adkf_jackknife_pool (leave-one-out checks and jackknife+ intervals) without a GPU - the closed forms of jackknife_ref.py
against actually deleting each point, the CPU twin against the reference (jackknife_ref.check_task), the ranks as a function of the
float32 bits of the levels, the coverage the definition promises on exchangeable tasks, every argument check of the library before
any launch, the scratch size, and the argument handling of gp_ops.jackknife_pool."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import jackknife_ref as R
from adkf_ift_amd import _lib
from test_ipv_pool_cpu import _pack, host_problem
from test_predict_pool_cpu import _problem, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
MAXIMIZE, SCALED, ARD = 2, 64, 4


# ---- the reference itself
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [12, 40])
def test_closed_forms_against_deleting_the_point(kind, n):
    """g_i, 1 / B_ii, mu_-i(x) and v_-i(x) of the reference against oracle.gp_oracle.predict on the support set without point i, at
    the pool rows and at z_i itself: 1e-10."""
    from oracle import gp_oracle as O

    g = torch.Generator().manual_seed(300 + 10 * kind + n)
    d, rows = 5, 9
    Zs = torch.randn(n, d, generator=g, dtype=torch.float64)
    ys = torch.randn(n, generator=g, dtype=torch.float64)
    X = torch.randn(rows, d, generator=g, dtype=torch.float64)
    phi = torch.tensor([-1.5, 0.4, 0.9], dtype=torch.float64)
    st = R.state(Zs, ys, X, phi, kind)
    mu, _, _, _, _ = R.folds(st, False)
    loo_mean, loo_var, _ = R.loo_ref(st)
    worst = 0.0
    for i in range(n):
        keep = [j for j in range(n) if j != i]
        m, cov = O.predict(Zs[keep], ys[keep], torch.cat([X, Zs[i:i + 1]]), phi, kind)
        m, var = m.numpy(), cov.diagonal().numpy()            # (var: observed, noise included)
        errs = (np.abs(mu[:, i] - m[:rows]).max(),
                np.abs(st["v"] + st["C"][:, i] ** 2 / st["bii"][i] - (var[:rows] - st["noise"])).max(),
                abs(st["g"][i] - (float(ys[i]) - m[rows])), abs(loo_mean[i] - m[rows]), abs(loo_var[i] - var[rows]))
        worst = max(worst, max(errs))
        assert max(errs) <= 1e-10, (kind, n, i, errs)
    print(f"kind {kind} n {n}: worst |closed form - deletion| {worst:.2e}")


def test_ranks_come_from_the_float32_bits():
    assert R.rank(0.7, 9) == 6            # 0.7f = 0.699999988: 6.99999988, not 7
    assert R.rank(0.25, 3) == 1 and R.rank(0.1, 3) == 0 and R.rank(0.1, 19) == 2 and R.rank(0.5, 9) == 5
    for bad in (0.0, -0.1, 1.0, 1.5, float("nan")):
        assert R.rank(bad, 50) == 0


# ---- the twin
def _jk_twin():
    cpu_twin, _ = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_jackknife_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_jackknife_pool"]
    assert tw.adkf_jackknife_pool_scratch_bytes(4, 8, 2, 8) == 0
    return fn


def jk_call(fn, b, phi, X, alphas, flags=0, k=0, excl=None, want=(True, True, True), expect_info=True):
    """The twin's adkf_jackknife_pool on host arrays: dict(lo, hi, loo_mean, loo_var, loo_lpd, top_idx, top_val, info)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows, ns = b.T, X.shape[0], b.c.ns_max
    al = np.ascontiguousarray(alphas, np.float32)
    L = al.shape[0]
    lo = np.full((T, L, rows), np.nan, np.float32) if want[0] else None
    hi = np.full((T, L, rows), np.nan, np.float32) if want[1] else None
    lm, lv, ll = ((np.full((T, ns), np.nan, np.float32), np.full((T, ns), np.nan, np.float32), np.full(T, np.nan, np.float32))
                  if want[2] else (None, None, None))
    info = np.empty(T, np.int32)
    top_idx = np.full((T, max(k, 1)), -7, np.int64)
    top_val = np.full((T, max(k, 1)), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(al), L, pp(e_idx), pp(e_off), pp(lo), pp(hi), pp(lm), pp(lv), pp(ll), k,
            pp(top_idx) if k else None, pp(top_val) if k else None, pp(info), None, 0, None, 0, None)
    assert rc == 0
    if expect_info:
        assert (info == 0).all()
    return dict(lo=lo, hi=hi, loo_mean=lm, loo_var=lv, loo_lpd=ll, top_idx=top_idx if k else None, top_val=top_val if k else None, info=info)


def check_call(out, states, alphas, scaled, maximize, lists=None, tag=""):
    """jackknife_ref.check_task on every task of a call (host arrays); returns the worst error / bound."""
    worst = 0.0
    for t, st in enumerate(states):
        loo = None if out["loo_mean"] is None else (out["loo_mean"][t], out["loo_var"][t], out["loo_lpd"][t])
        w = R.check_task(st, alphas, scaled, maximize, None if out["lo"] is None else out["lo"][t], None if out["hi"] is None else out["hi"][t],
                         loo, None if out["top_idx"] is None else out["top_idx"][t], None if out["top_val"] is None else out["top_val"][t],
                         excluded=lists[t] if lists else (), tag=(tag, t))
        worst = max(worst, w)
    return worst


LEVELS = (0.1, 0.25)
TWIN_SHAPES = [("matern", [48, 45, 31], 16, 60), ("rbf", [128, 125, 85], 64, 37), ("matern", [256, 19, 3], 12, 70)]
_states = {}


def states_of(kernel, n_s, d, rows, seed):
    key = (kernel, tuple(n_s), d, rows, seed)
    if key not in _states:
        hb, Zs, ys, n_s, X, phi, kind = host_problem(kernel, n_s, d, rows, seed)
        _states[key] = [R.state(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], kind) for t in range(hb.T)]
    return _states[key]


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("kernel,n_s,d,rows", TWIN_SHAPES)
def test_cpu_twin_against_the_reference(kernel, n_s, d, rows, scaled):
    fn = _jk_twin()
    seed = 500 + max(n_s)
    hb, Zs, ys, n_s, X, phi, kind = host_problem(kernel, n_s, d, rows, seed)
    states = states_of(kernel, n_s, d, rows, seed)
    lists = [[0, 7], [], [3]]
    for maximize in (False, True):
        out = jk_call(fn, hb, phi, X, LEVELS, (SCALED if scaled else 0) | (MAXIMIZE if maximize else 0), k=8, excl=_pack(lists))
        worst = check_call(out, states, LEVELS, scaled, maximize, lists, tag=(kernel, scaled, maximize))
        print(f"{kernel} {n_s} scaled={scaled} maximize={maximize}: worst error / bound {worst:.2e}")
        for t, n in enumerate(n_s):
            if R.rank(LEVELS[0], n) == 0:   # n = 3: no rank at 0.1 - the infinities, and such rows are never selected
                assert np.isneginf(out["lo"][t, 0]).all() and np.isposinf(out["hi"][t, 0]).all()
                assert (out["top_idx"][t] == -1).all() and np.isneginf(out["top_val"][t]).all()
                assert R.rank(LEVELS[1], n) == 1 and np.isfinite(out["lo"][t, 1]).all()   # at 0.25: the min / max
            else:
                assert (out["top_idx"][t] >= 0).all()
                assert (out["lo"][t, 0] <= out["lo"][t, 1]).all() and (out["hi"][t, 0] >= out["hi"][t, 1]).all()
                assert (out["lo"][t] <= out["hi"][t]).all()


def test_the_twin_agrees_with_the_reference_on_the_ranks():
    """Every (alpha, n) of a small grid - 0.7f with n = 9 is rank 6, not 7 - and levels without a rank."""
    fn = _jk_twin()
    n_s = [9, 4, 19, 10]
    seed = 733
    hb, Zs, ys, n_s, X, phi, kind = host_problem("matern", n_s, 6, 11, seed)
    states = states_of("matern", n_s, 6, 11, seed)
    alphas = (0.7, 0.1, 0.3, 0.5, 0.9, 0.05, float("nan"), 1.0)
    out = jk_call(fn, hb, phi, X, alphas)
    for t, st in enumerate(states):
        lo, hi, _, ranks, _ = R.jackknife_ref(st, alphas, False)
        assert ranks == [R.rank(a, n_s[t]) for a in alphas]
        mu, a, b, _, _ = R.folds(st, False)
        for l, k in enumerate(ranks):
            if k == 0:
                assert np.isneginf(out["lo"][t, l]).all() and np.isposinf(out["hi"][t, l]).all()
                continue
            # (both sides are float64 rounded once: 1e-5 is a few float32 roundings of values of order 1 to 10)
            assert np.abs(out["lo"][t, l] - lo[l]).max() <= 1e-5 and np.abs(out["hi"][t, l] - hi[l]).max() <= 1e-5, (t, l, k)
            if k < n_s[t]:   # and it is not the neighbouring rank: over 11 rows the two order statistics are well apart somewhere
                assert np.abs(out["lo"][t, l] - np.sort(a, 1)[:, k]).max() > 1e-3 and np.abs(out["hi"][t, l] + np.sort(-b, 1)[:, k]).max() > 1e-3
    assert R.rank(alphas[0], 9) == 6 and R.jackknife_ref(states[0], alphas, False)[3][0] == 6


def test_skipped_tasks_small_pools_and_null_outputs():
    fn = _jk_twin()
    seed = 548
    hb, Zs, ys, n_s, X, phi, kind = host_problem(*TWIN_SHAPES[0], seed)
    states = states_of(*TWIN_SHAPES[0], seed)
    full = jk_call(fn, hb, phi, X, LEVELS, k=4)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)
    # rows = 0: the leave-one-out diagnostic alone, the same bits
    none = jk_call(fn, hb, phi, X[:0], LEVELS, k=4)
    assert none["lo"].shape == (hb.T, 2, 0) and (none["top_idx"] == -1).all() and np.isneginf(none["top_val"]).all()
    for name in ("loo_mean", "loo_var", "loo_lpd"):
        assert np.array_equal(bits(none[name]), bits(full[name])), name
    # null outputs: the same selection
    sel = jk_call(fn, hb, phi, X, LEVELS, k=4, want=(False, False, False))
    assert np.array_equal(sel["top_idx"], full["top_idx"]) and np.array_equal(bits(sel["top_val"]), bits(full["top_val"]))
    # rows < k and every row excluded
    few = jk_call(fn, hb, phi, X[:3], LEVELS, k=8)
    assert (few["top_idx"][:, :3] >= 0).all() and (few["top_idx"][:, 3:] == -1).all() and np.isneginf(few["top_val"][:, 3:]).all()
    gone = jk_call(fn, hb, phi, X[:3], LEVELS, k=2, excl=_pack([[0, 1, 2]] * hb.T))
    assert (gone["top_idx"] == -1).all() and np.isneginf(gone["top_val"]).all()
    # a task with n_s == 0 is skipped; the others are what they are without it
    keep = hb.n_s[1]
    hb.n_s[1] = 0
    try:
        out = jk_call(fn, hb, phi, X, LEVELS, k=4)
    finally:
        hb.n_s[1] = keep
    for name in ("lo", "hi", "loo_mean", "loo_var", "loo_lpd"):
        assert (out[name][1] == 0).all(), name
        for t in (0, 2):
            assert np.array_equal(bits(out[name][t]), bits(full[name][t])), (name, t)
    assert (out["top_idx"][1] == -1).all() and np.isneginf(out["top_val"][1]).all()
    check_call(full, states, LEVELS, False, False)


def test_cpu_twin_on_an_ard_batch():
    fn = _jk_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(1, True, 63, rows=40)
    states = [R.ard_state(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], X, phi[t], 1) for t in range(b.T)]
    for scaled in (False, True):
        out = jk_call(fn, b, phi, X, (0.2, 0.4), (SCALED if scaled else 0) | MAXIMIZE, k=5)
        check_call(out, states, (0.2, 0.4), scaled, True, tag=("ard", scaled))


# ---- the definition
@pytest.mark.parametrize("scaled", [False, True])
def test_coverage_of_the_definition(scaled):
    """400 exchangeable tasks from a Matern GP prior, n = 19 and one held-out point each, alpha = 0.1, the fit's lengthscale off by
    1.5: the interval of the reference covers the held-out label at least 80 % of the time, the theorem's floor 1 - 2 alpha.  (About
    0.90 is what one sees; the binomial deviation is 0.015, so this guards the direction of the ranks, it does not measure.)"""
    from oracle import gp_oracle as O

    g = torch.Generator().manual_seed(2021)
    n, d, tasks = 19, 3, 400
    true_phi = torch.tensor([float(O.inv_softplus(torch.tensor(0.05))), RAW(1.0), RAW(1.0)], dtype=torch.float64)
    fit_phi = torch.tensor([float(O.inv_softplus(torch.tensor(0.05))), RAW(1.0), RAW(1.5)], dtype=torch.float64)
    noise, os_, ls = O.transform_phi(true_phi)
    hit = 0
    for _ in range(tasks):
        Z = torch.randn(n + 1, d, generator=g, dtype=torch.float64)
        A = O.kernel_matrix(Z, Z, os_, ls, 1) + noise * torch.eye(n + 1, dtype=torch.float64)
        y = torch.linalg.cholesky(A) @ torch.randn(n + 1, generator=g, dtype=torch.float64)
        st = R.state(Z[:n], y[:n], Z[n:], fit_phi, 1)
        lo, hi, _, ranks, _ = R.jackknife_ref(st, (0.1,), scaled)
        assert ranks == [2]
        hit += int(lo[0, 0] <= float(y[n]) <= hi[0, 0])
    print(f"scaled={scaled}: coverage {hit / tasks:.3f} of {tasks} tasks")
    assert hit / tasks >= 0.80


def RAW(x):
    return float(np.log(np.expm1(x)))


# ---- the library's argument checks
def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, L=2, k=0, ard=False, flags=0, x=True, alpha=True, lo=True, hi=True, loo=True, top=(True, True),
               excl=(False, False), info=True, ws=True, ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    LL, kk = min(max(L, 1), 8), min(max(k, 1), 64)
    al = torch.full((LL,), 0.1)
    olo, ohi = torch.zeros(T * LL * max(rows, 1)), torch.zeros(T * LL * max(rows, 1))
    lm, lv, ll = torch.zeros(T * ns), torch.zeros(T * ns), torch.zeros(T)
    inf = torch.zeros(T, dtype=torch.int32)
    top_idx, top_val = torch.zeros(T * kk, dtype=torch.int64), torch.zeros(T * kk)
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_jackknife_pool_scratch_bytes(T, ns, L, k)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_jackknife_pool(C.byref(b), p(phi), flags, p(X), rows, p(al) if alpha else None, L, p(e_idx) if excl[0] else None,
                                   p(e_off) if excl[1] else None, p(olo) if lo else None, p(ohi) if hi else None, p(lm) if loo else None,
                                   p(lv) if loo else None, p(ll) if loo else None, k, p(top_idx) if top[0] else None,
                                   p(top_val) if top[1] else None, p(inf) if info else None, p(wsb) if ws else None, nb - ws_short,
                                   C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_scratch_bytes(lib):
    f = lib.adkf_jackknife_pool_scratch_bytes
    assert f(16, 128, 1, 0) > 0 and f(16, 128, 1, 0) == f(16, 128, 8, 0)            # not a function of L
    assert f(16, 128, 1, 0) < f(32, 128, 1, 0) and f(16, 128, 1, 0) < f(16, 256, 1, 0) and f(16, 128, 1, 0) < f(16, 128, 1, 8)
    for bad in ((0, 128, 1, 0), (-1, 128, 1, 0), (16, 0, 1, 0), (16, -5, 1, 0), (16, 128, 0, 0), (16, 128, -1, 0), (16, 128, 1, -1),
                (16, 257, 1, 0), (16, 128, 9, 0), (16, 128, 1, 65)):
        assert f(*bad) == 0, bad
    assert _lib.JK_POINTS_MAX == 256 and _lib.JK_LEVELS_MAX == 8 and _lib.PM_JK_SCALED == 64


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0, x=False, lo=False, hi=False) == LAUNCH
    assert _host_call(lib, ard=True, ns=256, L=8, k=64, flags=MAXIMIZE | SCALED, excl=(True, True)) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, ns=257) == SIZE
    assert _host_call(lib, L=0) == SIZE and _host_call(lib, L=9) == SIZE and _host_call(lib, L=-3) == SIZE
    assert _host_call(lib, k=65) == SIZE
    for bit in (1, 4, 8, 16, 32, 128):
        assert _host_call(lib, flags=bit) == BADARG                            # a flag bit other than MAXIMIZE | JK_SCALED
    assert _host_call(lib, alpha=False) == BADARG
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    assert _host_call(lib, info=False) == BADARG
    assert _host_call(lib, ws=False) == BADARG
    assert _host_call(lib, k=2, excl=(True, False)) == BADARG                  # excl_idx without excl_off
    assert _host_call(lib, k=-1) == BADARG
    assert _host_call(lib, k=4, top=(False, True)) == BADARG and _host_call(lib, k=4, top=(True, False)) == BADARG
    assert _host_call(lib, lo=False, hi=False, loo=False) == BADARG            # no output at all
    assert _host_call(lib, k=4, scratch_off=4) == BADARG                       # a misaligned scratch
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, scratch_short=1) == WORKSPACE


# ---- Python
def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    b = types.SimpleNamespace(nq=0, ard=False, T=2, ns=16)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.jackknife_pool(types.SimpleNamespace(nq=3, ard=False, T=2, ns=16), None, None)
    with pytest.raises(ValueError, match="topk"):
        gp_ops.jackknife_pool(b, None, None, topk=65)
    with pytest.raises(ValueError, match="held-out"):
        gp_ops.jackknife_pool(types.SimpleNamespace(nq=0, ard=False, T=2, ns=257), None, None)
    for bad in ((), (0.1,) * 9):
        with pytest.raises(ValueError, match="levels"):
            gp_ops.jackknife_pool(b, None, None, alpha=bad)
