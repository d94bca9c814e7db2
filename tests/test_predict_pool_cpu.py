"""CPU: adkf_predict_pool without a GPU - clean refusal with no device, every argument check before any launch, the CPU twin
against the float64 oracle (isotropic and ARD batches), the selection semantics on the twin, and gp_ops.pack_exclude."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from adkf_ift_amd import _lib

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE, SCORE_MEAN = 1, 2, 4


def _rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.fixture(scope="module")
def lib():
    try:
        return _lib.load()
    except (RuntimeError, OSError) as e:
        pytest.fail(f"libadkf_gp.so must be built (build() compiles it without a GPU): {e}")


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, ard=False, flags=0, x=True, mean=True, var=True, ei=False, best=False, k=0,
               top=(True, True), excl=(False, False), ws_short=0, scratch_short=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    out = [torch.zeros(T * max(rows, 1)) for _ in range(3)]
    info, bf = torch.zeros(T, dtype=torch.int32), torch.zeros(T)
    kk = max(k, 1)
    top_idx, top_val = torch.zeros(T * kk, dtype=torch.int64), torch.zeros(T * kk)
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    ws = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_predict_pool_scratch_bytes(T, k)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_predict_pool(C.byref(b), p(phi), flags, p(X), rows, p(bf) if best else None, p(e_idx) if excl[0] else None,
                                 p(e_off) if excl[1] else None, p(out[0]) if mean else None, p(out[1]) if var else None,
                                 p(out[2]) if ei else None, k, p(top_idx) if top[0] else None, p(top_val) if top[1] else None, p(info),
                                 p(ws), nb - ws_short, p(scratch), sb - scratch_short, None)


def test_scratch_bytes_depend_on_T_and_k_only(lib):
    f = lib.adkf_predict_pool_scratch_bytes
    assert f(16, 0) == 0 and f(1, 0) == 0
    assert 0 < f(16, 64) <= 4 << 20 and 0 < f(1, 64) <= 4 << 20 and 0 < f(10000, 64) <= 10000 * 64 * 12
    assert f(16, 1) < f(16, 64)


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, rows=0, k=64, best=True, mean=False, var=False) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, ei=True, best=True, k=64, excl=(True, True)) == LAUNCH
    assert _host_call(lib, ard=True, d=12, rows=7, k=3, flags=SCORE_MEAN | MAXIMIZE) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    assert _host_call(lib, ei=True, best=False) == BADARG                      # ei without best_f
    assert _host_call(lib, k=4, best=False) == BADARG                          # ranking by EI without best_f
    assert _host_call(lib, k=-1) == BADARG
    assert _host_call(lib, k=4, best=True, top=(False, True)) == BADARG
    assert _host_call(lib, k=4, best=True, top=(True, False)) == BADARG
    assert _host_call(lib, mean=False, var=False, ei=False, k=0) == BADARG     # no output at all
    assert _host_call(lib, k=2, best=True, excl=(True, False)) == BADARG       # excl_idx without excl_off
    assert _host_call(lib, flags=8) == BADARG                                  # an unknown flag bit
    assert _host_call(lib, k=65, best=True) == SIZE
    assert _host_call(lib, k=8, best=True, scratch_short=1) == WORKSPACE
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, ard=True, ws_short=1) == WORKSPACE


def test_pack_exclude():
    from adkf_ift_amd import gp_ops

    idx, off = gp_ops.pack_exclude([[5, 1, 5, 99, -2, 3], [], None, torch.tensor([7, 0])], 4, 10)
    assert idx.dtype == torch.int64 and off.dtype == torch.int64 and off.shape == (5,)
    assert off.tolist() == [0, 3, 3, 3, 5] and idx.tolist() == [1, 3, 5, 0, 7]
    idx, off = gp_ops.pack_exclude(None, 3, 10)
    assert idx.numel() == 0 and idx.dtype == torch.int64 and off.tolist() == [0, 0, 0, 0]
    # an (excl_idx, excl_off) pair is normalised in the same way
    idx, off = gp_ops.pack_exclude((torch.tensor([4, 2, 2, 11, 6]), torch.tensor([0, 4, 5])), 2, 10)
    assert off.tolist() == [0, 2, 3] and idx.tolist() == [2, 4, 6]
    with pytest.raises(ValueError):
        gp_ops.pack_exclude([[1]], 2, 10)


def _twin():
    import os
    import shutil
    import subprocess

    from oracle import cpu_twin
    if not os.path.exists(cpu_twin.LIB) and shutil.which("g++") is None:   # no host compiler: the twin is checker-only
        pytest.skip("CPU twin not built and no g++ to build it")
    try:
        tw = cpu_twin.load()
    except subprocess.CalledProcessError as e:   # the compiler is there but cannot build it (e.g. no OpenMP)
        pytest.skip(f"CPU twin could not be built: {e}")
    fn = tw.adkf_predict_pool   # a twin library without the entry point fails here
    sb = tw.adkf_predict_pool_scratch_bytes
    assert sb(4, 8) == 0
    return cpu_twin, fn


def _problem(kind, ard, seed, rows=23):
    from oracle import cpu_twin

    T, ns, d = 3, 12, 5
    n_s = np.array([12, 7, 10], np.int32)
    g = torch.Generator().manual_seed(seed)
    Zs = torch.randn(T, ns, d, generator=g) * torch.tensor([1.0, 0.5, 2.0, 1.5, 0.8]) + 0.7
    ys = torch.randn(T, ns, generator=g)
    X = torch.randn(rows, d, generator=g) + 0.7
    base = torch.tensor([[-2.0, 0.3], [-1.0, 0.0], [-3.0, 0.5]])
    if ard:
        raw_ls = torch.tensor([[0.8, 1.6, 0.2, 1.1, 2.0], [1.2, 0.4, 0.9, 0.6, 1.4], [0.5, 0.5, 1.8, 0.3, 1.0]])
    else:
        raw_ls = torch.tensor([[0.8], [1.2], [0.5]])
    phi = torch.cat([base, raw_ls], 1).numpy().astype(np.float32)
    b = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((T, 4), np.float32), kind, n_s=n_s)
    if ard:
        b.c.flags = ARD
    best = np.array([0.2, -0.1, -0.4], np.float32)
    return b, Zs, ys, n_s, np.ascontiguousarray(X.numpy(), np.float32), phi, best


def _call(fn, b, phi, flags, X, best, k=0, excl=None, per_row=True):
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    mean, var, ei = (np.full((T, rows), np.nan, np.float32) for _ in range(3)) if per_row else (None, None, None)
    info = np.empty(T, np.int32)
    top_idx = np.full((T, max(k, 1)), -7, np.int64)
    top_val = np.full((T, max(k, 1)), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(best), pp(e_idx), pp(e_off), pp(mean), pp(var), pp(ei), k, pp(top_idx) if k else None,
            pp(top_val) if k else None, pp(info), None, 0, None, 0, None)
    assert rc == 0 and (info == 0).all()
    return mean, var, ei, top_idx, top_val


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_twin_against_the_oracle(kind, ard):
    from oracle import gp_oracle as O

    _, fn = _twin()
    b, Zs, ys, n_s, X, phi, best = _problem(kind, ard, 30 + kind + 2 * ard)
    Xd = torch.from_numpy(X).double()
    for flags in (0, LATENT, MAXIMIZE, LATENT | MAXIMIZE):
        mean, var, ei, _, _ = _call(fn, b, phi, flags, X, best)
        for t in range(b.T):
            n = n_s[t]
            pt = torch.from_numpy(phi[t]).double()
            m_ref, cov = O.predict(Zs[t, :n].double(), ys[t, :n].double(), Xd, pt, kind)
            noise = float(O.transform_phi(pt)[0])
            v_ref = cov.diagonal().numpy() - (noise if flags & LATENT else 0.0)
            assert _rel(mean[t], m_ref.numpy()) <= 1e-4
            assert _rel(var[t], v_ref) <= 1e-4
            s = np.sqrt(np.maximum(cov.diagonal().numpy() - noise, 1e-12))
            u = ((m_ref.numpy() - best[t]) if flags & MAXIMIZE else (best[t] - m_ref.numpy())) / s
            cdf = np.array([0.5 * math.erfc(-x / math.sqrt(2.0)) for x in u])
            e_ref = s * (u * cdf + np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi))
            assert _rel(ei[t], e_ref) <= 1e-4


def select_ref(score, k, excluded=()):
    """The ordering rule restated: stable sort by descending score, then by index; NaN and excluded rows are not eligible."""
    score = np.asarray(score, np.float32)
    ok = np.ones(score.shape[0], bool)
    ok[np.asarray(list(excluded), np.int64)] = False
    ok &= ~np.isnan(score)
    cand = np.nonzero(ok)[0]
    order = cand[np.argsort(-score[cand].astype(np.float64), kind="stable")][:k]   # (cand ascending: ties keep the lower index)
    idx = np.full(k, -1, np.int64)
    val = np.full(k, -np.inf, np.float32)
    idx[:order.size] = order
    val[:order.size] = score[order]
    return idx, val


@pytest.mark.parametrize("ard", [False, True])
def test_selection_semantics_on_the_twin(ard):
    _, fn = _twin()
    b, Zs, ys, n_s, X, phi, best = _problem(1, ard, 40 + ard, rows=70)
    X[10] = X[3]; X[41] = X[3]; X[69] = X[20]          # exact duplicate rows: bit-equal scores
    # choose the exclusions from a first look at the scores: task 0 may not take its best row, task 1 has none, task 2 nearly all
    _, _, ei0, _, _ = _call(fn, b, phi, LATENT, X, best)
    lists = [sorted({int(np.argmax(ei0[0])), 5, 6}), [], sorted(set(range(70)) - {3, 10, 41, 50})]
    e_idx = np.array([i for l in lists for i in l], np.int64)
    e_off = np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64)
    for flags, k in ((LATENT, 1), (LATENT, 7), (LATENT | MAXIMIZE, 64), (SCORE_MEAN, 5), (SCORE_MEAN | MAXIMIZE, 64), (0, 64)):
        mean, var, ei, top_idx, top_val = _call(fn, b, phi, flags, X, best, k=k, excl=(e_idx, e_off))
        for t in range(b.T):
            score = (mean[t] if flags & MAXIMIZE else -mean[t]) if flags & SCORE_MEAN else ei[t]
            idx, val = select_ref(score, k, lists[t])
            assert np.array_equal(top_idx[t], idx), (flags, k, t)
            assert np.array_equal(top_val[t].view(np.int32), val.view(np.int32)), (flags, k, t)
            assert not set(top_idx[t].tolist()) & set(lists[t])
        if k == 64:   # task 2 has four eligible rows: duplicates in index order, then the -1 / -inf tail
            assert (top_idx[2, 4:] == -1).all() and np.isneginf(top_val[2, 4:]).all() and (top_idx[2, :4] >= 0).all()
            got = top_idx[2, :4].tolist()
            assert got.index(3) < got.index(10) < got.index(41)
        # nothing per row requested: the same selection, bit for bit
        _, _, _, ti2, tv2 = _call(fn, b, phi, flags, X, best, k=k, excl=(e_idx, e_off), per_row=False)
        assert np.array_equal(ti2, top_idx) and np.array_equal(tv2.view(np.int32), top_val.view(np.int32))
    # no exclusion list at all, and a pool smaller than k
    mean, var, ei, top_idx, top_val = _call(fn, b, phi, LATENT, X[:9], best, k=16)
    for t in range(b.T):
        idx, val = select_ref(ei[t], 16)
        assert np.array_equal(top_idx[t], idx) and np.array_equal(top_val[t].view(np.int32), val.view(np.int32))
        assert (top_idx[t, 9:] == -1).all()
