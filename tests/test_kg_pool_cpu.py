"""CPU: adkf_kg_pool without a GPU - the reference of kg_ref.py against quadrature, known answers and exactly degenerate line sets;
the entry is exported, refuses cleanly with no device and checks every argument before any launch; gp_ops.kg_pool's and the BO
loop's argument handling; the CPU twin against the reference (isotropic and ARD, both senses, KG and log KG) and the semantics of
the call on the twin: skipped and repeated reference entries, M > rows, rows that are reference rows, exclusions and the order of
the selection, skipped tasks."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import believer_ref as B
import kg_ref as R
from adkf_ift_amd import _lib
from test_believer_pool_ard_cpu import ard_posterior
from test_predict_pool_cpu import _problem, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE, LOG = 1, 2, 16
EPS32 = R.EPS32


# ---- the reference checks itself
def test_the_reference_against_quadrature():
    g = np.random.default_rng(11)
    for n in (2, 3, 5, 9, 17):
        for scale in (0.1, 1.0, 5.0):
            a, b = g.normal(size=n) * scale, g.normal(size=n)
            val, unit, info = R.kg_lines(a, b)
            quad = R.kg_quad(a, b)
            assert abs(val - quad) <= 1e-12 * max(unit, 1.0), (n, scale, val, quad)
            lval, lunit, _ = R.kg_lines(a, b, log=True)
            assert abs(lval - math.log(quad)) <= 1e-10 * lunit, (n, scale)
            assert val >= 0 and len(info["active"]) >= 2 and info["c"] == sorted(info["c"])


def test_the_reference_on_known_answers():
    assert R.kg_lines([0.7], [1.3])[0] == 0.0 and R.kg_lines([0.7], [1.3], log=True)[0] == -math.inf
    assert abs(R.kg_lines([0.0, 0.0], [0.0, 1.0])[0] - 1.0 / math.sqrt(2.0 * math.pi)) < 1e-16
    h = lambda u: math.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi) + u * 0.5 * math.erfc(-u / math.sqrt(2.0))
    for a, b in (((0.3, -0.2), (0.5, 1.5)), ((1.0, 2.5), (2.0, -1.0)), ((0.0, -3.0), (0.1, 0.9))):
        da, db = abs(a[0] - a[1]), abs(b[0] - b[1])
        want = db * h(-da / db)   # EI's formula: sigma = |db|, u = -|da| / |db|
        assert abs(R.kg_lines(a, b)[0] - want) <= 1e-15 * max(1.0, want)
        assert abs(R.kg_lines(a, b, log=True)[0] - math.log(want)) <= 1e-13 * (1 + (da / db) ** 2)
    # far in the tail the logarithm stays finite where float64 KG is 0
    lv = R.kg_lines([0.0, -60.0], [0.0, 1.0], log=True)[0]
    assert R.kg_lines([0.0, -60.0], [0.0, 1.0])[0] == 0.0 and -1850 < lv < -1800


def test_the_reference_on_degenerate_sets():
    base = R.kg_lines([0.25, -0.5, 1.0], [-1.0, 0.5, 2.0])
    dup = R.kg_lines([0.25, -0.5, 1.0, -0.5, 0.25, 1.0], [-1.0, 0.5, 2.0, 0.5, -1.0, 2.0])   # every line twice
    assert dup[0] == base[0] and len(dup[2]["active"]) == len(base[2]["active"])
    # three lines through the point (z, y) = (0.5, 1): the middle one has an empty interval; with or without it, the same value
    three = R.kg_lines([1.5, 1.0, 0.0], [-1.0, 0.0, 2.0])
    two = R.kg_lines([1.5, 0.0], [-1.0, 2.0])
    assert abs(three[0] - two[0]) <= 1e-15 and abs(R.kg_quad([1.5, 1.0, 0.0], [-1.0, 0.0, 2.0]) - two[0]) <= 1e-12
    # all slopes equal: one survivor
    assert R.kg_lines([0.1, 0.9, -2.0], [0.5, 0.5, 0.5])[0] == 0.0
    assert R.kg_lines([0.1, 0.9, -2.0], [0.5, 0.5, 0.5], log=True)[0] == -math.inf


# ---- the entry of the device library
def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, M=4, k=3, ard=False, flags=0, x=True, ref=True, outs=(True, False, False), top=(True, True),
               excl=(False, False), info=True, ws=True, ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    Mm, kk = min(max(M, 1), 64), min(max(k, 0), 64)
    ref_t = torch.zeros(T, Mm, dtype=torch.int64)
    score, cov, rmean = torch.zeros(T * max(rows, 1)), torch.zeros(T * max(rows, 1) * Mm), torch.zeros(T * Mm)
    inf = torch.zeros(T, dtype=torch.int32)
    top_idx, top_val = torch.zeros(T * max(kk, 1), dtype=torch.int64), torch.zeros(T * max(kk, 1))
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_kg_pool_scratch_bytes(T, ns, d, Mm, kk)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_kg_pool(C.byref(b), p(phi), flags, p(X), rows, p(ref_t) if ref else None, M, p(e_idx) if excl[0] else None,
                            p(e_off) if excl[1] else None, p(score) if outs[0] else None, p(cov) if outs[1] else None,
                            p(rmean) if outs[2] else None, k, p(top_idx) if top[0] else None, p(top_val) if top[1] else None,
                            p(inf) if info else None, p(wsb) if ws else None, nb - ws_short,
                            C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_the_entry_is_exported(lib):
    assert "adkf_kg_pool" in _lib.SIGNATURES and "adkf_kg_pool_scratch_bytes" in _lib.SIGNATURES
    fn = lib.adkf_kg_pool   # a library without the entry point fails here
    assert fn.restype is C.c_int and len(fn.argtypes) == 21
    assert _lib.KG_REFS_MAX == 64


def test_the_scratch_size(lib):
    f = lib.adkf_kg_pool_scratch_bytes
    base = f(3, 16, 8, 4, 0)
    assert base >= 4 * 3 * 4 * (16 + 8 + 1) + 8 * 3 * 4 and base % 8 == 0
    assert 0 <= f(3, 16, 8, 4, 5) - base - lib.adkf_predict_pool_scratch_bytes(3, 5) < 128   # prediction's lists behind the state (+ the arena's alignment)
    assert f(3, 16, 8, 8, 0) > base and f(3, 32, 8, 4, 0) > base and f(3, 16, 16, 4, 0) > base
    for bad in ((0, 16, 8, 4, 0), (3, 0, 8, 4, 0), (3, 16, 0, 4, 0), (3, 16, 8, 0, 0), (3, 16, 8, 65, 0), (3, 16, 8, 4, -1), (3, 16, 8, 4, 65)):
        assert f(*bad) == 0, bad


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0, x=False) == LAUNCH
    assert _host_call(lib, ard=True, d=12, rows=7, M=1, k=0, flags=LOG) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, M=64, k=64, outs=(True, True, True), excl=(True, True), flags=MAXIMIZE | LOG) == LAUNCH
    assert _host_call(lib, k=0, outs=(False, True, False), top=(False, False)) == LAUNCH
    assert _host_call(lib, k=0, outs=(False, False, True), top=(False, False)) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    assert _host_call(lib, ref=False) == BADARG
    assert _host_call(lib, info=False) == BADARG
    assert _host_call(lib, ws=False) == BADARG
    assert _host_call(lib, excl=(True, False)) == BADARG                       # excl_idx without excl_off
    assert _host_call(lib, k=-1) == BADARG
    assert _host_call(lib, top=(False, True)) == BADARG
    assert _host_call(lib, top=(True, False)) == BADARG
    assert _host_call(lib, k=0, outs=(False, False, False)) == BADARG          # no output at all
    assert _host_call(lib, scratch_off=4) == BADARG                            # a misaligned scratch
    for bit in (LATENT, 4, 8, 32):
        assert _host_call(lib, flags=bit) == BADARG                            # flag bits other than MAXIMIZE | LOG_EI
        assert _host_call(lib, flags=bit | MAXIMIZE | LOG) == BADARG
    for M in (0, -2, 65):
        assert _host_call(lib, M=M) == SIZE
    assert _host_call(lib, k=65) == SIZE
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, ard=True, ws_short=1) == WORKSPACE
    assert _host_call(lib, scratch_short=1) == WORKSPACE


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False, T=3, d=5)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.kg_pool(types.SimpleNamespace(nq=3, ard=False, T=3, d=5), None, None)
    for k in (-1, 65):
        with pytest.raises(ValueError, match="topk must be"):
            gp_ops.kg_pool(iso, None, None, topk=k)
    for n in (0, 65):
        with pytest.raises(ValueError, match="n_refs must be"):
            gp_ops.kg_pool(iso, None, None, n_refs=n)
    for bad in (torch.zeros(3, 4), torch.zeros(4, dtype=torch.int64), torch.zeros(4, 4, dtype=torch.int64), [[1, 2]] * 3):
        with pytest.raises(ValueError, match="ref_idx must be"):
            gp_ops.kg_pool(iso, None, None, ref_idx=bad)
    for M in (0, 65):
        with pytest.raises(ValueError, match="reference rows M must be"):
            gp_ops.kg_pool(iso, None, None, ref_idx=torch.zeros(3, M, dtype=torch.int64))


def test_the_bo_loop_checks_its_arguments():
    from adkf_ift_amd import bayes_opt as BO

    X, y = torch.randn(20, 3), torch.randn(20)
    for q in (0, 65):
        with pytest.raises(ValueError, match="query_batch_size must be"):
            BO.run_gp_kg_bo_batched(X, y, 4, q, 1, "matern", "cpu", 10, 0.01, True, rngs=[np.random.default_rng(0)])
    for n in (0, 65):
        with pytest.raises(ValueError, match="n_refs must be"):
            BO.run_gp_kg_bo_batched(X, y, 4, 2, 1, "matern", "cpu", 10, 0.01, True, rngs=[np.random.default_rng(0)], n_refs=n)


# ---- the twin
def _kg_twin():
    cpu_twin, _ = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_kg_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_kg_pool"]
    return fn


def kg_call(fn, b, phi, flags, X, ref_idx, k=0, excl=None, want=(True, True, True), ok=True):
    """The twin's adkf_kg_pool on host arrays: (score, cov, ref_mean, top_idx, top_val, info)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    ref_idx = np.ascontiguousarray(ref_idx, np.int64)
    M = ref_idx.shape[1]
    score = np.full((T, rows), np.nan, np.float32) if want[0] else None
    cov = np.full((T, rows, M), np.nan, np.float32) if want[1] else None
    rmean = np.full((T, M), np.nan, np.float32) if want[2] else None
    info = np.empty(T, np.int32)
    top_idx = np.full((T, max(k, 1)), -7, np.int64)
    top_val = np.full((T, max(k, 1)), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(ref_idx), M, pp(e_idx), pp(e_off), pp(score), pp(cov), pp(rmean), k,
            pp(top_idx) if k else None, pp(top_val) if k else None, pp(info), None, 0, None, 0, None)
    assert rc == 0
    if ok:
        assert (info == 0).all()
    return score, cov, rmean, top_idx, top_val, info


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _posts(b, Zs, ys, n_s, X, phi, kind, ard):
    return [(ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], X, phi[t], kind) if ard else
             B.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], kind)) for t in range(b.T)]


def check_twin_task(post, ref_idx_t, maximize, log, score, cov, rmean, tag):
    """The twin rounds a float64 evaluation to float32 at the boundary; its posterior and the oracle's differ by float64 rounding
    through a solve of condition (os + noise) / noise <= 1e3: 1e-9 of the scale is generous.  So
        |score - ref| <= 2 eps32 |ref| + 1e-9 unit,   |cov - S| <= 2 eps32 |S| + 1e-9 os,   |ref_mean - m| <= 2 eps32 |m| + 1e-9."""
    m, S, noise, os_ = post
    ref, unit, refs = R.kg_task(post, ref_idx_t, maximize, log)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isneginf(ref), np.isneginf(score)), tag
    err = np.abs(score[fin].astype(np.float64) - ref[fin])
    assert (err <= 2 * EPS32 * np.abs(ref[fin]) + 1e-9 * unit[fin]).all(), (tag, float((err / unit[fin]).max()))
    for j, p in enumerate(refs):
        if p < 0:
            assert (cov[:, j] == 0).all() and rmean[j] == 0, (tag, j)
        else:
            assert (np.abs(cov[:, j] - S[:, p]) <= 2 * EPS32 * np.abs(S[:, p]) + 1e-9 * os_).all(), (tag, j)
            assert abs(rmean[j] - m[p]) <= 2 * EPS32 * abs(m[p]) + 1e-9, (tag, j)
    return ref


CASES = [(0, False, 1), (1, False, 5), (0, True, 8), (1, True, 5), (1, False, 64)]   # (kind, ARD, M)


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("kind,ard,M", CASES)
def test_cpu_twin_against_the_reference(kind, ard, M, maximize):
    fn = _kg_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(kind, ard, 60 + kind + 2 * ard, rows=40)
    g = np.random.default_rng(5 + M)
    ref_idx = np.stack([g.permutation(40)[:M] if M <= 40 else g.integers(0, 40, M) for _ in range(b.T)]).astype(np.int64)
    posts = _posts(b, Zs, ys, n_s, X, phi, kind, ard)
    for log in (False, True):
        flags = (MAXIMIZE if maximize else 0) | (LOG if log else 0)
        score, cov, rmean, _, _, _ = kg_call(fn, b, phi, flags, X, ref_idx)
        for t in range(b.T):
            ref = check_twin_task(posts[t], ref_idx[t], maximize, log, score[t], cov[t], rmean[t], (kind, ard, M, maximize, log, t))
            if not log:
                assert (score[t] >= 0).all()
            if M == 1:   # a row that is the only reference entry has no other line than its own
                assert (score[t, ref_idx[t, 0]] == (-np.inf if log else 0.0)) and np.isfinite(np.delete(ref, ref_idx[t, 0])).all()


def test_skipped_and_repeated_entries_and_more_entries_than_rows():
    fn = _kg_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(1, False, 44, rows=12)
    posts = _posts(b, Zs, ys, n_s, X, phi, 1, False)
    messy = np.array([[3, -1, 3, 12, 7, 400, 7, 0], [-1, -1, 5, 5, 5, -9, 11, 11], [-1, 12, 13, -2, -1, -1, -1, -1]], np.int64)
    clean = np.array([[3, 7, 0], [5, 11, -1], [-1, -1, -1]], np.int64)
    for flags in (0, MAXIMIZE | LOG):
        sm, cm, rm, _, _, _ = kg_call(fn, b, phi, flags, X, messy)
        sc, cc, rc, _, _, _ = kg_call(fn, b, phi, flags, X, clean)
        assert np.array_equal(_bits(sm), _bits(sc))                    # the same reference sets: the same bits
        for t in range(b.T):
            check_twin_task(posts[t], messy[t], bool(flags & MAXIMIZE), bool(flags & LOG), sm[t], cm[t], rm[t], ("messy", flags, t))
        assert np.array_equal(_bits(cm[0][:, [0, 4, 7]]), _bits(cc[0])) and (cm[0][:, [1, 2, 3, 5, 6]] == 0).all()
        # task 2 has no valid entry: every row has its own line only
        assert (sm[2] == (-np.inf if flags & LOG else 0.0)).all() and (cm[2] == 0).all() and (rm[2] == 0).all()
    # M = 40 > rows = 12, every row of the pool a reference row (repeated): defined, and equal to the 12 distinct entries
    big = np.tile(np.arange(12, dtype=np.int64), 4)[None].repeat(b.T, 0)[:, :40]
    sb_, _, _, _, _, _ = kg_call(fn, b, phi, 0, X, big)
    s12, _, _, _, _, _ = kg_call(fn, b, phi, 0, X, np.arange(12, dtype=np.int64)[None].repeat(b.T, 0))
    assert np.array_equal(_bits(sb_), _bits(s12)) and (sb_ > 0).all()


def test_rows_that_are_reference_rows():
    """A row's own entry is skipped for that row, by index: its score is the score with that entry removed from the set; cov keeps
    v(x) in that column."""
    fn = _kg_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(0, False, 45, rows=30)
    posts = _posts(b, Zs, ys, n_s, X, phi, 0, False)
    ref_idx = np.array([[4, 9, 17, 22]] * b.T, np.int64)
    for flags in (MAXIMIZE, LOG):
        score, cov, _, _, _, _ = kg_call(fn, b, phi, flags, X, ref_idx)
        for j, p in enumerate(ref_idx[0]):
            less = np.delete(ref_idx, j, axis=1)
            s2, _, _, _, _, _ = kg_call(fn, b, phi, flags, X, less)
            assert np.array_equal(_bits(score[:, p]), _bits(s2[:, p])), (flags, p)
            for t in range(b.T):
                v = posts[t][1][p, p]
                assert abs(cov[t, p, j] - v) <= 2 * EPS32 * v + 1e-9 * posts[t][3]
        # an exact duplicate ROW of a reference row is another index: it keeps the entry (two coincident lines, one survives)
        X2 = X.copy()
        X2[5] = X2[4]
        s3, _, _, _, _, _ = kg_call(fn, b, phi, flags, X2, ref_idx)
        assert np.isfinite(s3[:, 5]).all()


def test_exclusions_the_order_and_a_skipped_task():
    fn = _kg_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(1, False, 46, rows=70)
    X[10] = X[3]; X[41] = X[3]          # exact duplicate rows: equal scores, ascending index
    ref_idx = np.array([[0, 20, 33, 60, 69, 8]] * b.T, np.int64)
    lists = [[5, 6, 17], [], sorted(set(range(70)) - {3, 10, 41, 50})]
    excl = (np.array([i for l in lists for i in l], np.int64), np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64))
    for flags in (0, MAXIMIZE, LOG):
        k = 8
        score, _, _, top_idx, top_val, _ = kg_call(fn, b, phi, flags, X, ref_idx, k=k, excl=excl)
        for t in range(b.T):
            wi, wv = R.topk_of(score[t], k, lists[t])
            assert np.array_equal(top_idx[t], wi) and np.array_equal(_bits(top_val[t]), _bits(wv)), (flags, t)
            assert _bits(score[t, 3]) == _bits(score[t, 10]) == _bits(score[t, 41])
        assert top_idx[2].tolist()[:4] == sorted(top_idx[2].tolist()[:4], key=lambda r: (-score[2, r], r)) and (top_idx[2, 4:] == -1).all()
        assert np.isneginf(top_val[2, 4:]).all()
        # score == NULL: the same selection
        _, _, _, ti2, tv2, _ = kg_call(fn, b, phi, flags, X, ref_idx, k=k, excl=excl, want=(False, False, False))
        assert np.array_equal(ti2, top_idx) and np.array_equal(_bits(tv2), _bits(top_val))
    full = kg_call(fn, b, phi, 0, X, ref_idx, k=4)
    b.n_s[1] = 0                        # a skipped task: zero slices, -1 / -inf; the others do not see it
    score, cov, rmean, top_idx, top_val, info = kg_call(fn, b, phi, 0, X, ref_idx, k=4)
    assert (score[1] == 0).all() and (cov[1] == 0).all() and (rmean[1] == 0).all() and (top_idx[1] == -1).all() and np.isneginf(top_val[1]).all()
    for t in (0, 2):
        assert np.array_equal(_bits(score[t]), _bits(full[0][t])) and np.array_equal(top_idx[t], full[3][t])
    # a NaN score is never selected: a NaN pool row (not a reference row) has NaN mean and variance on the twin
    b.n_s[1] = 7
    Xn = X.copy()
    Xn[15] = np.nan
    sn, _, _, tin, tvn, _ = kg_call(fn, b, phi, LOG, Xn, ref_idx, k=64)
    assert np.isnan(sn[:, 15]).all() and not (tin == 15).any() and (np.delete(sn, 15, axis=1) == np.delete(kg_call(fn, b, phi, LOG, X, ref_idx)[0], 15, axis=1)).all()
    # an empty pool
    s0, c0, r0, ti0, tv0, _ = kg_call(fn, b, phi, 0, X[:0], ref_idx, k=3)
    assert s0.shape == (b.T, 0) and (r0 == 0).all() and (ti0 == -1).all() and np.isneginf(tv0).all()
