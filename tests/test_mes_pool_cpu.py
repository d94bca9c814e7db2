"""CPU: adkf_mes_pool without a GPU - clean refusal with no device, every argument check before any launch, the CPU twin against
the mpmath reference of mes_ref.py on the float64 oracle's posterior (isotropic and ARD batches, both signs, all three branches of
g), the semantics of the call on the twin, and the argument handling of gp_ops.mes_pool / gp_ops.max_value_samples."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import mes_ref as R
from adkf_ift_amd import _lib
from test_predict_pool_cpu import _call, _problem, _twin, lib, select_ref  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE = 1, 2
TOL = 1e-4   # what the twin's mean and variance are held to against the oracle (test_predict_pool_cpu: phi crosses as float32)


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, S=5, ard=False, flags=0, x=True, ystar=True, score=True, k=0, top=(True, True),
               excl=(False, False), info=True, ws=True, ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    ystar_t = torch.zeros(T, min(max(S, 1), 64))
    out = torch.zeros(T * max(rows, 1))
    inf = torch.zeros(T, dtype=torch.int32)
    kk = min(max(k, 1), 64)
    top_idx, top_val = torch.zeros(T * kk, dtype=torch.int64), torch.zeros(T * kk)
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_predict_pool_scratch_bytes(T, k)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_mes_pool(C.byref(b), p(phi), flags, p(X), rows, p(ystar_t) if ystar else None, S, p(e_idx) if excl[0] else None,
                             p(e_off) if excl[1] else None, p(out) if score else None, k, p(top_idx) if top[0] else None,
                             p(top_val) if top[1] else None, p(inf) if info else None, p(wsb) if ws else None, nb - ws_short,
                             C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, rows=0, x=False, k=64, score=False) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, S=64, k=64, excl=(True, True), flags=MAXIMIZE) == LAUNCH
    assert _host_call(lib, ard=True, d=12, rows=7, k=3, S=1, score=False) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, info=False) == BADARG
    assert _host_call(lib, ws=False) == BADARG
    for bit in (LATENT, 4, 8, 16, 32):
        assert _host_call(lib, flags=bit) == BADARG                            # flag bits other than MAXIMIZE
        assert _host_call(lib, flags=bit | MAXIMIZE) == BADARG
    assert _host_call(lib, ystar=False) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    assert _host_call(lib, k=2, excl=(True, False)) == BADARG                  # excl_idx without excl_off
    assert _host_call(lib, k=-1) == BADARG
    assert _host_call(lib, k=4, top=(False, True)) == BADARG
    assert _host_call(lib, k=4, top=(True, False)) == BADARG
    assert _host_call(lib, k=0, score=False) == BADARG                         # nothing asked for
    assert _host_call(lib, k=4, scratch_off=4) == BADARG                       # a misaligned scratch
    for S in (0, -1, 65):
        assert _host_call(lib, S=S) == SIZE
    assert _host_call(lib, k=65) == SIZE
    assert _host_call(lib, k=8, scratch_short=1) == WORKSPACE
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, ard=True, ws_short=1) == WORKSPACE


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False, T=3, d=5)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.mes_pool(types.SimpleNamespace(nq=3, ard=False, T=3, d=5), None, None, ystar=torch.zeros(3, 4))
    for topk in (-1, 65):
        with pytest.raises(ValueError, match="topk must be"):
            gp_ops.mes_pool(iso, None, None, ystar=torch.zeros(3, 4), topk=topk)
    with pytest.raises(ValueError, match="no output"):
        gp_ops.mes_pool(iso, None, None, ystar=torch.zeros(3, 4), topk=0, want_score=False)
    for bad in (None, torch.zeros(4), torch.zeros(4, 4), torch.zeros(3, 4, 1)):
        with pytest.raises(ValueError, match="ystar must be"):
            gp_ops.mes_pool(iso, None, None, ystar=bad)
    for S in (0, 65):
        with pytest.raises(ValueError, match="max-value samples"):
            gp_ops.mes_pool(iso, None, None, ystar=torch.zeros(3, S), topk=2)
    # max_value_samples is one Thompson call of the batch's kind: its checks are that call's
    for b in (iso, types.SimpleNamespace(nq=0, ard=True, T=3, d=5)):
        for S in (0, 65):
            with pytest.raises(ValueError, match="n_samples must be"):
                gp_ops.max_value_samples(b, None, None, omega=None, phase=None, n_samples=S)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.max_value_samples(types.SimpleNamespace(nq=2, ard=False, T=3, d=5), None, None, omega=None, phase=None, n_samples=4)


# ---- the twin
def _mes_twin():
    cpu_twin, _ = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_mes_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_mes_pool"]
    return fn


def mes_call(fn, b, phi, flags, X, ystar, k=0, excl=None, want_score=True):
    """The twin's adkf_mes_pool on host arrays: (score, top_idx, top_val)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    ystar = np.ascontiguousarray(ystar, np.float32)
    score = np.full((T, rows), np.nan, np.float32) if want_score else None
    info = np.empty(T, np.int32)
    top_idx = np.full((T, max(k, 1)), -7, np.int64)
    top_val = np.full((T, max(k, 1)), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(ystar), ystar.shape[1], pp(e_idx), pp(e_off), pp(score), k,
            pp(top_idx) if k else None, pp(top_val) if k else None, pp(info), None, 0, None, 0, None)
    assert rc == 0 and (info == 0).all()
    return score, top_idx, top_val


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_the_reference_itself():
    """g > 0, strictly decreasing, its two asymptotes, and the left-tail form of the issue against the definition."""
    xs = np.linspace(-40.0, 12.0, 105)
    g = np.array([R.mes_term_ref(x) for x in xs])
    assert (g > 0).all() and (np.diff(g) < 0).all()
    assert abs(R.mes_term_ref(0.0) - np.log(2.0)) < 1e-15
    a = 30.0   # the two terms, each ~a^2 / 2, cancel to log(a sqrt(2 pi)) - 1 / 2 + O(a^-2)
    assert abs(R.mes_term_ref(-a) - (np.log(a * np.sqrt(2 * np.pi)) - 0.5)) < 3.0 / (a * a)
    assert np.isnan(R.mes_term_ref(np.nan)) and np.isnan(R.mes_term_ref(np.inf)) and np.isnan(R.mes_term_ref(-np.inf))


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_twin_against_the_reference(kind, ard, maximize):
    from oracle import gp_oracle as O

    fn = _mes_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(kind, ard, 30 + kind + 2 * ard)
    Xd = torch.from_numpy(X).double()
    S = 5
    post = []
    for t in range(b.T):
        n = n_s[t]
        pt = torch.from_numpy(phi[t]).double()
        m_ref, cov = O.predict(Zs[t, :n].double(), ys[t, :n].double(), Xd, pt, kind)
        tr = O.transform_phi(pt)
        post.append((m_ref.numpy(), cov.diagonal().numpy() - float(tr[0]), float(tr[1])))
    seen = np.zeros(3, int)   # gamma > 0, -1 < gamma <= 0, gamma <= -1
    worst = 0.0
    for shift in (-3.0, 0.0, 2.0):
        jitter = np.linspace(-0.2, 0.2, S)
        ystar = np.empty((b.T, S), np.float32)
        for t, (m, v, os) in enumerate(post):
            ystar[t] = (m.max() + shift * np.sqrt(os) + jitter) if maximize else (m.min() - shift * np.sqrt(os) + jitter)
        score, _, _ = mes_call(fn, b, phi, MAXIMIZE if maximize else 0, X, ystar)
        for t, (m, v, os) in enumerate(post):
            ref, gamma = R.mes_ref(m, v, ystar[t], maximize)
            seen += [(gamma > 0).sum(), ((gamma > -1) & (gamma <= 0)).sum(), (gamma <= -1).sum()]
            dm, dv = TOL * np.abs(m).max(), TOL * np.abs(v).max()
            bound = 0.4 * dm / np.sqrt(v) + dv / (2 * v) + 1e-6
            err = np.abs(score[t] - ref)
            worst = max(worst, (err / bound).max())
            assert (err <= bound).all(), (shift, t, (err / bound).max())
            assert (score[t] > 0).all()
    print(f"kind {kind} ard {ard} maximize {maximize}: gammas per branch {seen.tolist()}, worst error / bound {worst:.2e}")
    assert (seen > 0).all(), seen


@pytest.mark.parametrize("ard", [False, True])
def test_selection_semantics_on_the_twin(ard):
    fn = _mes_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(1, ard, 40 + ard, rows=70)
    X[10] = X[3]; X[41] = X[3]; X[69] = X[20]          # exact duplicate rows: bit-equal scores
    g = np.random.default_rng(5)
    ystar = (-1.5 + 0.5 * g.standard_normal((b.T, 5))).astype(np.float32)
    lists = [[5, 6, 17], [], sorted(set(range(70)) - {3, 10, 41, 50})]
    excl = (np.array([i for l in lists for i in l], np.int64), np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64))
    for flags, k in ((0, 1), (0, 7), (MAXIMIZE, 64), (0, 64)):
        ys_f = -ystar if flags & MAXIMIZE else ystar
        score, top_idx, top_val = mes_call(fn, b, phi, flags, X, ys_f, k=k, excl=excl)
        for t in range(b.T):
            idx, val = select_ref(score[t], k, lists[t])
            assert np.array_equal(top_idx[t], idx), (flags, k, t)
            assert np.array_equal(_bits(top_val[t]), _bits(val)), (flags, k, t)
            assert _bits(score[t, 3]) == _bits(score[t, 10]) == _bits(score[t, 41])
        if k == 64:   # task 2 has four eligible rows: duplicates in index order, then the -1 / -inf tail
            assert (top_idx[2, 4:] == -1).all() and np.isneginf(top_val[2, 4:]).all() and (top_idx[2, :4] >= 0).all()
            got = top_idx[2, :4].tolist()
            assert got.index(3) < got.index(10) < got.index(41)
        # score == NULL: the same selection, bit for bit
        none, ti2, tv2 = mes_call(fn, b, phi, flags, X, ys_f, k=k, excl=excl, want_score=False)
        assert none is None and np.array_equal(ti2, top_idx) and np.array_equal(_bits(tv2), _bits(top_val))
    # no exclusion list, a pool smaller than k, and an empty pool
    score, top_idx, top_val = mes_call(fn, b, phi, 0, X[:9], ystar, k=16)
    for t in range(b.T):
        idx, val = select_ref(score[t], 16)
        assert np.array_equal(top_idx[t], idx) and np.array_equal(_bits(top_val[t]), _bits(val)) and (top_idx[t, 9:] == -1).all()
    score, top_idx, top_val = mes_call(fn, b, phi, 0, X[:0], ystar, k=3)
    assert score.shape == (b.T, 0) and (top_idx == -1).all() and np.isneginf(top_val).all()


def test_one_sample_orders_the_rows_by_gamma():
    """g is strictly decreasing: with S = 1 the scores sort as -gamma does (gamma from the twin's own float32 mean and variance)."""
    _, pool_fn = _twin()
    fn = _mes_twin()
    for maximize in (False, True):
        flags = MAXIMIZE if maximize else 0
        b, Zs, ys, n_s, X, phi, best = _problem(1, False, 44, rows=70)
        mean, var, _, _, _ = _call(pool_fn, b, phi, LATENT | flags, X, best)
        ystar = np.array([[mean[t].max() if maximize else mean[t].min()] for t in range(b.T)], np.float32)
        score, _, _ = mes_call(fn, b, phi, flags, X, ystar)
        for t in range(b.T):
            gamma = R.mes_ref(mean[t], var[t], ystar[t], maximize)[1][:, 0]
            order = np.argsort(gamma, kind="stable")
            keep = [order[0]]
            for i in order[1:]:
                if gamma[i] - gamma[keep[-1]] > 1e-6:
                    keep.append(i)
            assert len(keep) >= 60
            assert (np.diff(score[t][keep].astype(np.float64)) < 0).all(), (maximize, t)


def test_a_nan_sample_and_a_skipped_task():
    fn = _mes_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(0, False, 41, rows=70)
    ystar = np.full((b.T, 4), -1.0, np.float32) + np.arange(4, dtype=np.float32) * 0.25
    full = mes_call(fn, b, phi, 0, X, ystar, k=5)
    for bad in (np.nan, np.inf, -np.inf):
        ys2 = ystar.copy()
        ys2[1, 2] = bad
        score, top_idx, top_val = mes_call(fn, b, phi, 0, X, ys2, k=5)
        assert np.isnan(score[1]).all() and (top_idx[1] == -1).all() and np.isneginf(top_val[1]).all()
        for t in (0, 2):
            assert np.array_equal(_bits(score[t]), _bits(full[0][t])) and np.array_equal(top_idx[t], full[1][t])
            assert np.array_equal(_bits(top_val[t]), _bits(full[2][t]))
    # a task with n_s == 0 is skipped: zeros and -1 / -inf; the others are what they are without it
    b.n_s[1] = 0
    score, top_idx, top_val = mes_call(fn, b, phi, 0, X, ystar, k=5)
    assert (score[1] == 0).all() and (top_idx[1] == -1).all() and np.isneginf(top_val[1]).all()
    for t in (0, 2):
        assert np.array_equal(_bits(score[t]), _bits(full[0][t])) and np.array_equal(top_idx[t], full[1][t])
