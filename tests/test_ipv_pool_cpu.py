"""CPU: adkf_ipv_pool (target-variance batch selection) without a GPU - the float64 reference of ipv_ref.py against a refit and
its telescoping identity, the CPU twin against the reference (ipv_ref.check_task), the semantics of skipped entries and of a task
without targets on the twin, every argument check of the library before any launch, the scratch size, and the argument handling of
gp_ops.ipv_pool and bayes_opt.run_gp_ipv_al_batched."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import ipv_ref as R
from adkf_ift_amd import _lib
from test_gpu_predict_marginal import _features
from test_gpu_predict_pool import _pool
from test_predict_pool_cpu import _problem, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _pack(lists):
    return (np.array([i for l in lists for i in l], np.int64), np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64))


# ---- the reference itself
def test_the_reference_against_a_refit():
    """tvar_0 - score_0(x) is the summed latent variance at the targets once x has joined the support set (any label: the variance
    does not depend on it), from oracle.gp_oracle.predict on the enlarged task."""
    from oracle import gp_oracle as O

    for kind, seed in ((0, 60), (1, 61)):
        b, Zs, ys, n_s, X, phi, _ = _problem(kind, False, seed, rows=23)
        tgt = np.array([2, 9, 14, 20])
        for t in (0, 1):
            n = n_s[t]
            post = R.posterior(Zs[t, :n], ys[t, :n], X, phi[t], kind)
            steps, tvar = R.ipv_ref(post, tgt, np.ones(4), [-1])
            for x in (0, 9, 17):   # (9 is a target)
                Z1 = torch.cat([Zs[t, :n].double(), torch.as_tensor(X[x:x + 1]).double()])
                y1 = torch.cat([ys[t, :n].double(), torch.tensor([0.37], dtype=torch.float64)])
                _, cov = O.predict(Z1, y1, torch.as_tensor(X[tgt]).double(), torch.as_tensor(phi[t]).double(), kind)
                after = float((cov.diagonal() - post[2]).sum())
                assert abs((tvar[0] - steps[0][0][x]) - after) <= 1e-9, (kind, t, x, tvar[0] - steps[0][0][x], after)


def test_the_reference_telescopes():
    """tvar_j - tvar_(j+1) = score_j(p_j) along a whole chain, weights included."""
    b, Zs, ys, n_s, X, phi, _ = _problem(1, False, 62, rows=40)
    tgt, w = np.array([1, 5, 8, 13, 21, 34]), np.array([1.0, 0.5, 2.0, 0.25, 1.5, 1.0])
    for t in range(3):
        post = R.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], 1)
        picks = [7, 5, 30, 0, 39, 21, 2, 11]
        steps, tvar = R.ipv_ref(post, tgt, w, picks)
        for j, p in enumerate(picks):
            assert abs((tvar[j] - tvar[j + 1]) - steps[j][0][p]) <= 1e-12, (t, j)
            assert (steps[j][0] >= 0).all()
        assert (np.diff(tvar) < 0).all()


# ---- the twin
def _ipv_twin():
    cpu_twin, _ = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_ipv_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_ipv_pool"]
    assert tw.adkf_ipv_pool_scratch_bytes(4, 8, 3, 8, 8) == 0
    return fn


def ipv_call(fn, b, phi, X, tgt, w, q, excl=None, want_trace=True, expect_info=True):
    """The twin's adkf_ipv_pool on host arrays: (sel_idx, sel_val, tvar, trace, info)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    tgt = np.ascontiguousarray(tgt, np.int64)
    w = None if w is None else np.ascontiguousarray(w, np.float32)
    trace = np.full((T, q, rows), np.nan, np.float32) if want_trace else None
    info = np.empty(T, np.int32)
    sel_idx = np.full((T, q), -7, np.int64)
    sel_val = np.full((T, q), np.nan, np.float32)
    tvar = np.full((T, q + 1), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), 0, pp(X), rows, pp(tgt), pp(w), tgt.shape[1], pp(e_idx), pp(e_off), q, pp(trace), pp(sel_idx), pp(sel_val),
            pp(tvar), pp(info), None, 0, None, 0, None)
    assert rc == 0
    if expect_info:
        assert (info == 0).all()
    return sel_idx, sel_val, tvar, trace, info


_problems = {}


def host_problem(kernel, n_s, d, rows, seed):
    """The support sets and pool of tests/test_gpu_believer_pool._explicit on the host, phi GIVEN: raw noise from -1 to -3, raw
    outputscale from 0.3 to 0, the lengthscale the median distance of the support set.  (hb, Zs, ys, n_s, X, phi), shared and left
    unchanged."""
    from oracle import cpu_twin

    key = (kernel, tuple(n_s), d, rows, seed)
    if key not in _problems:
        T, ns = len(n_s), max(n_s)
        Zs, ys, _ = _features(T, ns, [0] * T, d, seed, True)
        X = np.ascontiguousarray(_pool(rows, d, seed + 1).numpy())
        phi = np.zeros((T, 3), np.float32)
        phi[:, 0] = np.linspace(-1.0, -3.0, T)
        phi[:, 1] = np.linspace(0.3, 0.0, T)
        for t in range(T):
            med = float(torch.pdist(Zs[t, :n_s[t]].double()).median())
            phi[t, 2] = np.log(np.expm1(med))
        kind = {"rbf": 0, "matern": 1}[kernel]
        hb = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((T, 4), np.float32), kind, n_s=np.array(n_s, np.int32))
        _problems[key] = (hb, Zs, ys, list(n_s), X, phi, kind)
    return _problems[key]


def targets_of(T, rows, M, seed):
    """M distinct pool rows per task and non-uniform weights in [0.25, 2]."""
    g = np.random.default_rng(seed)
    tgt = np.stack([g.choice(rows, size=M, replace=False) for _ in range(T)]).astype(np.int64)
    w = (0.25 + 1.75 * g.random((T, M))).astype(np.float32)
    return tgt, w


TWIN_SHAPES = [("matern", [48, 45, 31], 16, 300, 8, 8), ("rbf", [200, 197, 133], 64, 333, 5, 6)]


@pytest.mark.parametrize("exclude_targets", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kernel,n_s,d,rows,M,q", TWIN_SHAPES)
def test_cpu_twin_against_the_reference(kernel, n_s, d, rows, M, q, weighted, exclude_targets):
    fn = _ipv_twin()
    hb, Zs, ys, n_s, X, phi, kind = host_problem(kernel, n_s, d, rows, 500 + max(n_s))
    tgt, w = targets_of(hb.T, rows, M, 7)
    w = w if weighted else None
    lists = [sorted(tgt[t].tolist()) for t in range(hb.T)] if exclude_targets else None
    sel_idx, sel_val, tvar, trace, _ = ipv_call(fn, hb, phi, X, tgt, w, q, excl=_pack(lists) if lists else None)
    for t in range(hb.T):
        post = R.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], kind)
        worst = R.check_task(post, tgt[t], None if w is None else w[t], sel_idx[t], sel_val[t], tvar[t], trace[t],
                             excluded=lists[t] if lists else (), tag=(kernel, weighted, exclude_targets, t))
        print(f"{kernel} {max(n_s)} weighted={weighted} exclude={exclude_targets} task {t}: picks {sel_idx[t].tolist()}, worst error / bound {worst:.2e}")
        assert len(set(sel_idx[t].tolist())) == q and (sel_idx[t] >= 0).all()
        if exclude_targets:
            assert not set(sel_idx[t].tolist()) & set(tgt[t].tolist())
        assert (np.diff(tvar[t].astype(np.float64)) < 0).all()


def test_skipped_entries_change_no_bit():
    fn = _ipv_twin()
    hb, Zs, ys, n_s, X, phi, kind = host_problem(*TWIN_SHAPES[0][:4], 548)
    rows, q = X.shape[0], 6
    tgt, w = targets_of(hb.T, rows, 5, 11)
    base = ipv_call(fn, hb, phi, X, tgt, w, q)
    # -1, >= rows, a repeat (with another weight) and a weight of 0, NaN and below 0, between and behind the entries
    col = lambda v: np.full((hb.T, 1), v)
    tgt2 = np.concatenate([tgt[:, :2], col(-1), tgt[:, 2:4], col(rows), tgt[:, :1], tgt[:, 4:], col(17), col(18), col(19)], 1).astype(np.int64)
    w2 = np.concatenate([w[:, :2], col(1.0), w[:, 2:4], col(1.0), col(3.0), w[:, 4:], col(0.0), col(np.nan), col(-1.0)], 1).astype(np.float32)
    assert not (tgt == 17).any() and not (tgt == 18).any() and not (tgt == 19).any()
    more = ipv_call(fn, hb, phi, X, tgt2, w2, q)
    assert np.array_equal(base[0], more[0])
    for a, c in zip(base[1:4], more[1:4]):
        assert np.array_equal(_bits(a), _bits(c))
    # weights == NULL is a weight of 1
    ones = ipv_call(fn, hb, phi, X, tgt, np.ones_like(w), q)
    none = ipv_call(fn, hb, phi, X, tgt, None, q)
    assert np.array_equal(ones[0], none[0]) and np.array_equal(_bits(ones[3]), _bits(none[3]))
    # trace == NULL: the same selection
    again = ipv_call(fn, hb, phi, X, tgt, w, q, want_trace=False)
    assert again[3] is None and np.array_equal(again[0], base[0]) and np.array_equal(_bits(again[1]), _bits(base[1]))
    assert np.array_equal(_bits(again[2]), _bits(base[2]))


def test_tasks_without_targets_small_pools_and_skipped_tasks():
    fn = _ipv_twin()
    hb, Zs, ys, n_s, X, phi, kind = host_problem(*TWIN_SHAPES[0][:4], 548)
    rows, q = X.shape[0], 4
    tgt, w = targets_of(hb.T, rows, 3, 12)
    full = ipv_call(fn, hb, phi, X, tgt, w, q)
    tgt1, w1 = tgt.copy(), w.copy()
    tgt1[1] = [-1, rows, rows + 5]          # task 1: no valid entry
    w1[2] = [0.0, np.nan, -2.0]             # task 2: no valid weight
    sel_idx, sel_val, tvar, trace, _ = ipv_call(fn, hb, phi, X, tgt1, w1, q)
    for t in (1, 2):
        assert (sel_idx[t] == -1).all() and np.isneginf(sel_val[t]).all() and (tvar[t] == 0).all() and (trace[t] == 0).all()
    assert np.array_equal(sel_idx[0], full[0][0]) and np.array_equal(_bits(trace[0]), _bits(full[3][0]))
    # a pool of 5 rows with q = 8: five picks, then the -1 / -inf tail with tvar repeated; every row excluded; no rows
    t5 = np.array([[0, 3, 4]] * hb.T, np.int64)
    sel_idx, sel_val, tvar, trace, _ = ipv_call(fn, hb, phi, X[:5], t5, None, 8)
    for t in range(hb.T):
        assert sorted(sel_idx[t, :5].tolist()) == list(range(5)) and (sel_idx[t, 5:] == -1).all() and np.isneginf(sel_val[t, 5:]).all()
        assert (_bits(tvar[t, 5:]) == _bits(tvar[t, 5])).all() and tvar[t, 5] > 0
        post = R.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], X[:5], phi[t], kind)
        R.check_task(post, t5[t], None, sel_idx[t], sel_val[t], tvar[t], trace[t], tag=("small", t))
    sel_idx, sel_val, tvar, _, _ = ipv_call(fn, hb, phi, X[:5], t5, None, 3, excl=_pack([list(range(5))] * hb.T))
    assert (sel_idx == -1).all() and np.isneginf(sel_val).all() and (tvar > 0).all() and (_bits(tvar) == _bits(tvar[:, :1])).all()
    sel_idx, sel_val, tvar, _, _ = ipv_call(fn, hb, phi, X[:0], t5, None, 3)
    assert (sel_idx == -1).all() and np.isneginf(sel_val).all() and (tvar == 0).all()
    # a task with n_s == 0 is skipped; the others are what they are without it
    keep = hb.n_s[1]
    hb.n_s[1] = 0
    try:
        sel_idx, sel_val, tvar, trace, _ = ipv_call(fn, hb, phi, X, tgt, w, q)
    finally:
        hb.n_s[1] = keep
    assert (sel_idx[1] == -1).all() and np.isneginf(sel_val[1]).all() and (tvar[1] == 0).all() and (trace[1] == 0).all()
    for t in (0, 2):
        assert np.array_equal(sel_idx[t], full[0][t]) and np.array_equal(_bits(trace[t]), _bits(full[3][t]))


def test_cpu_twin_on_an_ard_batch():
    from test_believer_pool_ard_cpu import ard_posterior

    fn = _ipv_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(1, True, 63, rows=70)
    tgt, w = targets_of(b.T, 70, 4, 13)
    sel_idx, sel_val, tvar, trace, _ = ipv_call(fn, b, phi, X, tgt, w, 6)
    for t in range(b.T):
        post = ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], X, phi[t], 1)
        R.check_task(post, tgt[t], w[t], sel_idx[t], sel_val[t], tvar[t], trace[t], tag=("ard", t))


# ---- the library's argument checks
def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, M=4, q=4, ard=False, flags=0, x=True, tgt=True, w=True, sel=(True, True), trace=False,
               tvar=True, excl=(False, False), info=True, ws=True, ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    qq, MM = min(max(q, 1), 64), min(max(M, 1), 64)
    tr = torch.zeros(T * qq * max(rows, 1))
    inf = torch.zeros(T, dtype=torch.int32)
    sel_idx, sel_val, tv = torch.zeros(T * qq, dtype=torch.int64), torch.zeros(T * qq), torch.zeros(T * (qq + 1))
    ti, tw = torch.zeros(T * MM, dtype=torch.int64), torch.ones(T * MM)
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_ipv_pool_scratch_bytes(T, ns, d, M, q)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_ipv_pool(C.byref(b), p(phi), flags, p(X), rows, p(ti) if tgt else None, p(tw) if w else None, M,
                             p(e_idx) if excl[0] else None, p(e_off) if excl[1] else None, q, p(tr) if trace else None,
                             p(sel_idx) if sel[0] else None, p(sel_val) if sel[1] else None, p(tv) if tvar else None,
                             p(inf) if info else None, p(wsb) if ws else None, nb - ws_short,
                             C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_scratch_bytes_depend_on_their_five_arguments_only(lib):
    f = lib.adkf_ipv_pool_scratch_bytes
    assert f(16, 128, 256, 8, 8) > 0 and f(16, 128, 256, 8, 8) == f(16, 128, 256, 8, 8)
    assert f(16, 128, 256, 8, 8) < f(32, 128, 256, 8, 8) and f(16, 128, 256, 8, 8) < f(16, 256, 256, 8, 8)
    assert f(16, 128, 256, 8, 8) < f(16, 128, 512, 8, 8)
    assert f(16, 128, 256, 1, 8) < f(16, 128, 256, 8, 8) < f(16, 128, 256, 56, 8)
    assert f(16, 128, 256, 8, 1) < f(16, 128, 256, 8, 8) < f(16, 128, 256, 8, 56)
    assert f(0, 128, 256, 8, 8) == 0 and f(16, 128, 256, 0, 8) == 0 and f(16, 128, 256, 8, 0) == 0
    assert f(16, 128, 256, 32, 32) > 0 and f(16, 128, 256, 33, 32) == 0 and f(16, 128, 256, 1, 64) == 0
    assert _lib.IPV_ENTRIES_MAX == 64


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0, x=False, w=False, tvar=False) == LAUNCH
    assert _host_call(lib, ard=True, ns=200, M=32, q=32, trace=True, excl=(True, True)) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    assert _host_call(lib, tgt=False) == BADARG
    assert _host_call(lib, sel=(False, True)) == BADARG
    assert _host_call(lib, sel=(True, False)) == BADARG
    assert _host_call(lib, info=False) == BADARG
    assert _host_call(lib, ws=False) == BADARG
    assert _host_call(lib, excl=(True, False)) == BADARG                       # excl_idx without excl_off
    for M, q in ((0, 4), (-2, 4), (4, 0), (4, -1)):
        assert _host_call(lib, M=M, q=q) == BADARG
    assert _host_call(lib, scratch_off=4) == BADARG                            # a misaligned scratch
    for bit in (1, 2, 4, 8, 16, 32):
        assert _host_call(lib, flags=bit) == BADARG                            # any flag bit
    for M, q in ((33, 32), (1, 64), (64, 1), (64, 64)):
        assert _host_call(lib, M=M, q=q) == SIZE                               # M + q = 65 and beyond
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, scratch_short=1) == WORKSPACE


# ---- Python
def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    b = types.SimpleNamespace(nq=0, ard=False, T=2)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.ipv_pool(types.SimpleNamespace(nq=3, ard=False, T=2), None, None, targets=[[1], [2]], q=4)
    for q in (0, -1, 64):
        with pytest.raises(ValueError, match="q must be"):
            gp_ops.ipv_pool(b, None, None, targets=[[1], [2]], q=q)
    for bad in ([[1, 2, 3]], [1, 2], [[0.5], [1.5]], "targets", [[], []]):
        with pytest.raises(ValueError):
            gp_ops.ipv_pool(b, None, None, targets=bad, q=4)
    with pytest.raises(ValueError, match="M \\+ q"):
        gp_ops.ipv_pool(b, None, None, targets=torch.zeros(2, 33, dtype=torch.int64), q=32)
    with pytest.raises(ValueError, match="weights"):
        gp_ops.ipv_pool(b, None, None, targets=[[1, 2], [2, 3]], weights=torch.ones(2, 3), q=4)


def test_the_loop_checks_its_arguments():
    from adkf_ift_amd import bayes_opt as BO

    X, y = torch.randn(50, 3), torch.randn(50)
    kw = dict(num_init_points=4, num_rounds=1, kernel_type="matern", device="cpu", init_from=0, noise_init=0.01, noise_prior=True,
              rngs=[np.random.default_rng(0)])
    for bad in ([], [50], [-1], [0.5]):
        with pytest.raises(ValueError, match="target_idx"):
            BO.run_gp_ipv_al_batched(X, y, bad, query_batch_size=2, **kw)
    X2, y2 = torch.randn(100, 3), torch.randn(100)
    with pytest.raises(ValueError, match="distinct targets"):
        BO.run_gp_ipv_al_batched(X2, y2, list(range(64)), query_batch_size=1, **kw)
    for qb in (0, 62):   # (three distinct targets: at most 61)
        with pytest.raises(ValueError, match="query_batch_size"):
            BO.run_gp_ipv_al_batched(X, y, [1, 2, 3, 3], query_batch_size=qb, **kw)
    with pytest.raises(ValueError, match="num_rounds"):
        BO.run_gp_ipv_al_batched(X, y, [1, 2], query_batch_size=2, **{**kw, "num_rounds": -1})
