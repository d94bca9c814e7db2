"""CPU: adkf_believer_pool_ard without a GPU - the export and its signature, clean refusal with no device, every argument check of
the isotropic entry made on the ARD one before any launch, the CPU twin against the float64 reference of believer_ref.py
(assertions 1-4), the semantics of the batch on the twin, and gp_ops.believer_pool_ard's argument handling.

The reference needs no ARD code: an ARD GP with lengthscales l is the isotropic GP at unit lengthscale on Z / l, so believer_ref's
posterior is called on the features divided by l = softplus(phi[2:]) (float64, from the float32 phi) with the raw lengthscale
softplus^-1(1)."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import believer_ref as R
from adkf_ift_amd import _lib
from test_believer_pool_cpu import _bits
from test_predict_pool_cpu import _call, _problem, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE, LOG_EI = 1, 2, 16
RAW_ONE = math.log(math.expm1(1.0))   # softplus^-1(1)


def ard_posterior(Zs, ys, X, phi_t, kind):
    """believer_ref.posterior of an ARD task: the isotropic posterior at unit lengthscale on the features over l."""
    p = np.asarray(phi_t, np.float64)
    l = np.logaddexp(0.0, p[2:])
    return R.posterior(np.asarray(Zs, np.float64) / l, ys, np.asarray(X, np.float64) / l, np.array([p[0], p[1], RAW_ONE]), kind)


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, q=4, ard=True, flags=0, x=True, best=True, sel=(True, True), extra=True, trace=False,
               excl=(False, False), info=True, ws=True, ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    qq = min(max(q, 1), 64)
    tr = torch.zeros(T * qq * max(rows, 1))
    inf, bf = torch.zeros(T, dtype=torch.int32), torch.zeros(T)
    sel_idx, out = torch.zeros(T * qq, dtype=torch.int64), [torch.zeros(T * qq) for _ in range(3)]
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_believer_pool_scratch_bytes(T, ns, d, q)   # (the layout does not depend on the kind of batch)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_believer_pool_ard(C.byref(b), p(phi), flags, p(X), rows, p(bf) if best else None, p(e_idx) if excl[0] else None,
                                      p(e_off) if excl[1] else None, q, p(tr) if trace else None, p(sel_idx) if sel[0] else None,
                                      p(out[0]) if sel[1] else None, p(out[1]) if extra else None, p(out[2]) if extra else None,
                                      p(inf) if info else None, p(wsb) if ws else None, nb - ws_short,
                                      C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_the_entry_is_exported_with_the_isotropic_signature(lib):
    assert hasattr(lib, "adkf_believer_pool_ard")
    assert _lib.SIGNATURES["adkf_believer_pool_ard"] == _lib.SIGNATURES["adkf_believer_pool"]


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, rows=0, x=False, extra=False) == LAUNCH
    assert _host_call(lib, ns=200, d=12, rows=5, q=64, trace=True, excl=(True, True), flags=MAXIMIZE | LOG_EI) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, ard=False) == BADARG                                # a batch that is not an ARD batch
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    assert _host_call(lib, best=False) == BADARG
    assert _host_call(lib, sel=(False, True)) == BADARG
    assert _host_call(lib, sel=(True, False)) == BADARG
    assert _host_call(lib, info=False) == BADARG
    assert _host_call(lib, ws=False) == BADARG
    assert _host_call(lib, excl=(True, False)) == BADARG                       # excl_idx without excl_off
    assert _host_call(lib, q=0) == BADARG
    assert _host_call(lib, q=-3) == BADARG
    assert _host_call(lib, scratch_off=4) == BADARG                            # a misaligned scratch
    for bit in (LATENT, 4, 8, 32):
        assert _host_call(lib, flags=bit) == BADARG                            # flag bits other than MAXIMIZE | LOG_EI
    assert _host_call(lib, q=65) == SIZE
    assert lib.adkf_workspace_bytes_ard(3, 16, 0, 8) > lib.adkf_workspace_bytes(3, 16, 0, 8)
    assert _host_call(lib, ws_short=1) == WORKSPACE                            # the bound is adkf_workspace_bytes_ard
    assert _host_call(lib, scratch_short=1) == WORKSPACE


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False)
    with pytest.raises(ValueError, match="ARD"):
        gp_ops.believer_pool_ard(iso, None, None, best_f=None, q=4)
    ard = types.SimpleNamespace(nq=0, ard=True)
    for q in (0, -1, 65):
        with pytest.raises(ValueError, match="q must be"):
            gp_ops.believer_pool_ard(ard, None, None, best_f=None, q=q)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.believer_pool_ard(types.SimpleNamespace(nq=3, ard=True), None, None, best_f=None, q=4)
    with pytest.raises(ValueError, match="ARD"):   # the isotropic entry keeps refusing ARD batches
        gp_ops.believer_pool(ard, None, None, best_f=None, q=4)


# ---- the twin
def _bv_twin():
    cpu_twin, _ = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_believer_pool_ard   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_believer_pool_ard"]
    return fn


def bv_call(fn, b, phi, flags, X, best, q, excl=None, want_trace=True):
    """The twin's adkf_believer_pool_ard on host arrays: (sel_idx, sel_val, sel_mean, sel_var, trace, info)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    trace = np.full((T, q, rows), np.nan, np.float32) if want_trace else None
    info = np.empty(T, np.int32)
    sel_idx = np.full((T, q), -7, np.int64)
    sel_val, sel_mean, sel_var = (np.full((T, q), np.nan, np.float32) for _ in range(3))
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(best), pp(e_idx), pp(e_off), q, pp(trace), pp(sel_idx), pp(sel_val), pp(sel_mean),
            pp(sel_var), pp(info), None, 0, None, 0, None)
    assert rc == 0 and (info == 0).all()
    return sel_idx, sel_val, sel_mean, sel_var, trace, info


def test_the_twin_refuses_the_other_kind_of_batch():
    fn = _bv_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(0, False, 60, rows=70)
    pp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = [np.zeros((b.T, 2), np.int64)] + [np.zeros((b.T, 2), np.float32) for _ in range(3)]
    info = np.zeros(b.T, np.int32)
    assert fn(C.byref(b.c), pp(phi), 0, pp(X), X.shape[0], pp(best), None, None, 2, None, pp(out[0]), pp(out[1]), pp(out[2]), pp(out[3]),
              pp(info), None, 0, None, 0, None) == BADARG


@pytest.mark.parametrize("flags", [0, MAXIMIZE, LOG_EI])
@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_twin_against_the_reference(kind, flags):
    fn = _bv_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(kind, True, 60 + kind, rows=70)
    q = 8
    sel_idx, sel_val, sel_mean, sel_var, trace, _ = bv_call(fn, b, phi, flags, X, best, q)
    for t in range(b.T):
        n = n_s[t]
        post = ard_posterior(Zs[t, :n].numpy(), ys[t, :n], X, phi[t], kind)
        s0 = R.believer_ref(post, best[t], flags & MAXIMIZE, [-1])[0][0]
        assert s0.max() >= 0.01, (t, s0.max(), "EI must stay far from underflow")
        worst = R.check_task(post, best[t], flags, sel_idx[t], sel_val[t], sel_mean[t], sel_var[t], trace[t], tag=(kind, flags, t))
        print(f"kind {kind} flags {flags} task {t}: picks {sel_idx[t].tolist()}, worst trace error / bound {worst:.2e}")
        assert len(set(sel_idx[t].tolist())) == q and (sel_idx[t] >= 0).all()


@pytest.mark.parametrize("flags", [0, MAXIMIZE, LOG_EI | MAXIMIZE])
def test_one_pick_is_the_pool_call(flags):
    _, pool_fn = _twin()
    fn = _bv_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(1, True, 61, rows=70)
    lists = [[5, 6], [], list(range(0, 70, 3))]
    excl = (np.array([i for l in lists for i in l], np.int64), np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64))
    sel_idx, sel_val, sel_mean, sel_var, trace, _ = bv_call(fn, b, phi, flags, X, best, 1, excl=excl)
    mean, var, ei, top_idx, top_val = _call(pool_fn, b, phi, LATENT | flags, X, best, k=1, excl=excl)
    assert np.array_equal(sel_idx, top_idx) and np.array_equal(_bits(sel_val), _bits(top_val))
    assert np.array_equal(_bits(trace[:, 0]), _bits(ei))
    for t in range(b.T):
        assert _bits(sel_mean[t, 0]) == _bits(mean[t, sel_idx[t, 0]]) and _bits(sel_var[t, 0]) == _bits(var[t, sel_idx[t, 0]])


def test_semantics_on_the_twin():
    fn = _bv_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(1, True, 40, rows=70)
    X[10] = X[3]; X[41] = X[3]          # exact duplicate rows
    lists = [[5, 6, 17], [], sorted(set(range(70)) - {3, 10, 41, 50})]
    excl = (np.array([i for l in lists for i in l], np.int64), np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64))
    for flags in (0, MAXIMIZE):
        q = 8
        sel_idx, sel_val, sel_mean, sel_var, trace, _ = bv_call(fn, b, phi, flags, X, best, q, excl=excl)
        for t in range(b.T):
            got = [p for p in sel_idx[t].tolist() if p >= 0]
            assert len(set(got)) == len(got), (t, "a pick repeats")
            assert not set(got) & set(lists[t]), (t, "an excluded row was picked")
            post = ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], X, phi[t], 1)
            R.check_task(post, best[t], flags, sel_idx[t], sel_val[t], sel_mean[t], sel_var[t], trace[t], excluded=lists[t], tag=(flags, t))
            # scores only fall: both the variance and the incumbent move against them
            steps = R.believer_ref(post, best[t], flags, sel_idx[t].tolist())
            for j in range(len(got) - 1):
                delta = steps[j][1][0]
                assert sel_val[t, j + 1] <= sel_val[t, j] + delta, (flags, t, j)
                assert (trace[t, j + 1] <= trace[t, j] + delta).all(), (flags, t, j)
        # task 2 may take 3, 10, 41 and 50 only: the duplicates in index order, then the -1 / -inf tail
        assert (sel_idx[2, 4:] == -1).all() and np.isneginf(sel_val[2, 4:]).all() and (sel_idx[2, :4] >= 0).all()
        assert (sel_mean[2, 4:] == 0).all() and (sel_var[2, 4:] == 0).all()
        got = sel_idx[2, :4].tolist()
        assert got.index(3) < got.index(10) < got.index(41)
        # exact duplicates: bit-equal scores at every step
        for t in range(b.T):
            for j in range(q):
                assert _bits(trace[t, j, 10]) == _bits(trace[t, j, 41]) == _bits(trace[t, j, 3]), (t, j)
        # trace == NULL: the same selection, bit for bit
        again = bv_call(fn, b, phi, flags, X, best, q, excl=excl, want_trace=False)
        assert again[4] is None and np.array_equal(again[0], sel_idx)
        for a, c in zip(again[1:4], (sel_val, sel_mean, sel_var)):
            assert np.array_equal(_bits(a), _bits(c))
