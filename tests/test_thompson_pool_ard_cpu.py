"""CPU: adkf_thompson_pool_ard without a GPU - the export, every argument check before any launch, clean refusal with no device,
the CPU twin against a float64 restatement on the scaled features (include/adkf_gp.h), the twin with equal lengthscales against its
isotropic entry, and the selection semantics on the twin."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from adkf_ift_amd import _lib
from test_predict_pool_cpu import select_ref
from test_thompson_pool_cpu import ARD, BADARG, LAUNCH, MAXIMIZE, SIZE, WORKSPACE, _draws, _np_basis, paths_ref

RAW_ONE = math.log(math.expm1(1.0))   # softplus^-1(1)


def _isp(x):
    return np.log(np.expm1(np.asarray(x, np.float64)))


@pytest.fixture(scope="module")
def lib():
    try:
        return _lib.load()
    except (RuntimeError, OSError) as e:
        pytest.fail(f"libadkf_gp.so must be built (build() compiles it without a GPU): {e}")


def _host_call(lib, entry="adkf_thompson_pool_ard", T=3, ns=16, nq=0, d=8, rows=10, ard=True, flags=0, x=True, S=4, m=64, missing=(),
               excl=(False, False), ws_short=0, scratch_short=0, scratch_offset=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    ss, mm = max(S, 1), max(m, 1)
    arr = dict(omega=torch.zeros(mm, d), phase=torch.zeros(mm), w=torch.zeros(T, ss, mm), eps=torch.zeros(T, ss, ns),
               sel_idx=torch.zeros(T, ss, dtype=torch.int64), sel_val=torch.zeros(T, ss), info=torch.zeros(T, dtype=torch.int32))
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    arr["ws"] = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_thompson_pool_scratch_bytes(T, ns, S, m)
    scratch = torch.zeros(sb // 4 + 64)
    g = lambda n: None if n in missing else p(arr[n])
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return getattr(lib, entry)(C.byref(b), p(phi), flags, p(X), rows, g("omega"), g("phase"), m, g("w"), g("eps"), S,
                               p(e_idx) if excl[0] else None, p(e_off) if excl[1] else None, None, g("sel_idx"), g("sel_val"), g("info"),
                               g("ws"), nb - ws_short, C.c_void_p(scratch.data_ptr() + scratch_offset), sb - scratch_short, None)


def test_the_library_exports_the_entry(lib):
    assert hasattr(lib, "adkf_thompson_pool_ard")
    assert "adkf_thompson_pool_ard" in _lib.SIGNATURES
    assert _lib.SIGNATURES["adkf_thompson_pool_ard"] == _lib.SIGNATURES["adkf_thompson_pool"]


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, S=64, m=4096, flags=MAXIMIZE, excl=(True, True)) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, ard=False) == BADARG                                # not an ARD batch
    for bit in (1, 4, 8, 16):
        assert _host_call(lib, flags=bit) == BADARG                            # any flag bit other than MAXIMIZE
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    for name in ("omega", "phase", "w", "eps", "sel_idx", "sel_val", "info", "ws"):
        assert _host_call(lib, missing=(name,)) == BADARG, name
    assert _host_call(lib, excl=(True, False)) == BADARG                       # excl_idx without excl_off
    assert _host_call(lib, S=0) == SIZE and _host_call(lib, S=65) == SIZE
    assert _host_call(lib, m=0) == SIZE and _host_call(lib, m=32) == SIZE and _host_call(lib, m=4160) == SIZE
    assert _host_call(lib, m=100) == SIZE                                      # not a multiple of 64
    assert _host_call(lib, ws_short=1) == WORKSPACE                            # the ARD workspace, one byte short
    assert _host_call(lib, scratch_short=1) == WORKSPACE
    assert _host_call(lib, scratch_offset=4) == BADARG                         # a scratch that is not 8-byte aligned


def test_the_isotropic_entry_still_refuses_ard_batches(lib):
    assert _host_call(lib, entry="adkf_thompson_pool", ard=True) == BADARG


# ---- the CPU twin

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
    return cpu_twin, tw.adkf_thompson_pool_ard, tw.adkf_thompson_pool   # a twin library without the entry point fails here


# per task and dimension, all distinct, in [0.5, 2.0]
ELL = np.array([[0.5, 0.8, 1.1, 1.4, 1.7], [2.0, 1.55, 0.65, 0.95, 1.25], [0.9, 1.9, 0.6, 1.3, 0.7]])


def _problem(kind, seed, rows=23, ell=ELL, n_s=(12, 7, 10)):
    """The data of test_thompson_pool_cpu._problem as an ARD batch with lengthscales ell [T, d]."""
    from oracle import cpu_twin

    T, ns, d = 3, 12, 5
    n_s = np.array(n_s, np.int32)
    g = torch.Generator().manual_seed(seed)
    Zs = torch.randn(T, ns, d, generator=g) * torch.tensor([1.0, 0.5, 2.0, 1.5, 0.8]) + 0.7
    ys = torch.randn(T, ns, generator=g)
    X = torch.randn(rows, d, generator=g) + 0.7
    head = np.array([[-2.0, 0.3], [-1.0, 0.0], [-3.0, 0.5]])
    phi = np.concatenate([head, _isp(ell)], 1).astype(np.float32)
    b = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((T, 4), np.float32), kind, n_s=n_s)
    b.c.flags = ARD
    return b, Zs.numpy(), ys.numpy(), n_s, np.ascontiguousarray(X.numpy(), np.float32), phi


def _call(fn, b, phi, flags, X, omega, phase, w, eps, excl=None, want_paths=True):
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows, S, m = b.T, X.shape[0], w.shape[1], omega.shape[0]
    paths = np.full((T, S, rows), np.nan, np.float32) if want_paths else None
    info = np.full(T, -9, np.int32)
    sel_idx, sel_val = np.full((T, S), -7, np.int64), np.full((T, S), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(omega), pp(phase), m, pp(w), pp(eps), S, pp(e_idx), pp(e_off), pp(paths),
            pp(sel_idx), pp(sel_val), pp(info), None, 0, None, 0, None)
    assert rc == 0 and (info == 0).all()
    return paths, sel_idx, sel_val


def ard_paths_ref(zs, ys, phi, kind, X, omega, phase, w, eps):
    """The specification for one ARD task: paths_ref on (z - mu) / l and (X - mu) / l formed in float64 from the float32 phi, at
    phi = (raw_noise, raw_outputscale, softplus^-1(1)).  (The scaled support set has mean zero, so paths_ref's own centring is a
    shift by rounding error only.)"""
    zs, X, phi = np.asarray(zs, np.float64), np.asarray(X, np.float64), np.asarray(phi, np.float64)
    ell = np.log1p(np.exp(phi[2:]))
    mu = zs.mean(0)
    return paths_ref((zs - mu) / ell, ys, np.array([phi[0], phi[1], RAW_ONE]), kind, (X - mu) / ell, omega, phase, w, eps)


@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_twin_against_the_float64_restatement(kind):
    _, fn, _ = _twin()
    b, Zs, ys, n_s, X, phi = _problem(kind, 50 + kind)
    S, m = 5, 128
    omega, phase = _np_basis(kind, b.d, m, 3 + kind)
    w, eps = _draws(b.T, S, m, b.ns, 4)
    for flags in (0, MAXIMIZE):
        paths, sel_idx, sel_val = _call(fn, b, phi, flags, X, omega, phase, w, eps)
        for t in range(b.T):
            n = n_s[t]
            ref = ard_paths_ref(Zs[t, :n], ys[t, :n], phi[t], kind, X, omega, phase, w[t], eps[t])
            err = np.abs(paths[t] - ref).max()
            print(f"kind {kind} flags {flags} task {t}: |paths - ref| max {err:.3e}, |ref| max {np.abs(ref).max():.3e}")
            assert err <= 1e-4 * max(1.0, np.abs(ref).max()), (t, err)
            for q in range(S):
                score = paths[t, q] if flags & MAXIMIZE else -paths[t, q]
                idx, val = select_ref(score, 1)
                assert sel_idx[t, q] == idx[0] and sel_val[t, q].view(np.int32) == val[0].view(np.int32)
    # the lengthscales matter: the isotropic restatement at the mean lengthscale is far off
    iso = paths_ref(Zs[0], ys[0], np.array([phi[0, 0], phi[0, 1], float(_isp(ELL[0].mean()))]), kind, X, omega, phase, w[0], eps[0])
    assert np.abs(paths[0] - iso).max() > 1e-2 * max(1.0, np.abs(iso).max())


@pytest.mark.parametrize("kind", [0, 1])
def test_equal_lengthscales_give_the_isotropic_call(kind):
    """Both entries of the twin compute in float64 and round once; the argument of the cosine and the distances are formed in a
    different order ((x - mu) / l per element against a division of the sum), which is a few float32 ulps after the rounding."""
    from oracle import cpu_twin

    _, fn_ard, fn_iso = _twin()
    ls = np.array([0.8, 1.3, 0.6])
    b, Zs, ys, n_s, X, phi = _problem(kind, 70 + kind, ell=np.repeat(ls[:, None], 5, 1))
    b_iso = cpu_twin.CpuBatch(Zs, ys, np.zeros((b.T, 4), np.float32), kind, n_s=n_s)
    phi_iso = np.ascontiguousarray(phi[:, :3])
    S, m = 5, 128
    omega, phase = _np_basis(kind, b.d, m, 5 + kind)
    w, eps = _draws(b.T, S, m, b.ns, 6)
    pa, _, _ = _call(fn_ard, b, phi, 0, X, omega, phase, w, eps)
    pi, _, _ = _call(fn_iso, b_iso, phi_iso, 0, X, omega, phase, w, eps)
    for t in range(b.T):
        err, scale = np.abs(pa[t] - pi[t]).max(), max(1.0, np.abs(pi[t]).max())
        print(f"kind {kind} task {t}: |ard - iso| max {err:.3e}, |iso| max {np.abs(pi[t]).max():.3e}")
        assert err <= 1e-6 * scale, (t, err)


def test_selection_semantics_on_the_twin():
    from oracle import cpu_twin

    _, fn, _ = _twin()
    b, Zs, ys, n_s, X, phi = _problem(1, 60, rows=70)
    X[10] = X[3]; X[41] = X[3]; X[69] = X[20]          # exact duplicate rows: bit-equal scores
    S, m = 6, 64
    omega, phase = _np_basis(1, b.d, m, 8)
    w, eps = _draws(b.T, S, m, b.ns, 9)
    # choose the exclusions from a first look: task 0 may not take the winners of its samples, task 1 excludes nothing, task 2 everything
    p0, s0, _ = _call(fn, b, phi, 0, X, omega, phase, w, eps)
    assert np.array_equal(p0[:, :, 10], p0[:, :, 3]) and np.array_equal(p0[:, :, 69], p0[:, :, 20])
    lists = [sorted(set(s0[0].tolist()) | {5}), [], list(range(70))]
    e_idx = np.array([i for l in lists for i in l], np.int64)
    e_off = np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64)
    for flags in (0, MAXIMIZE):
        paths, sel_idx, sel_val = _call(fn, b, phi, flags, X, omega, phase, w, eps, excl=(e_idx, e_off))
        for t in range(b.T):
            for q in range(S):
                idx, val = select_ref(paths[t, q] if flags & MAXIMIZE else -paths[t, q], 1, lists[t])
                assert sel_idx[t, q] == idx[0], (flags, t, q)
                assert sel_val[t, q].view(np.int32) == val[0].view(np.int32), (flags, t, q)
        assert (sel_idx[2] == -1).all() and np.isneginf(sel_val[2]).all()          # every row excluded
        assert not set(sel_idx[0].tolist()) & set(lists[0])
        # paths = NULL: the same selection, bit for bit
        _, si2, sv2 = _call(fn, b, phi, flags, X, omega, phase, w, eps, excl=(e_idx, e_off), want_paths=False)
        assert np.array_equal(si2, sel_idx) and np.array_equal(sv2.view(np.int32), sel_val.view(np.int32))
    # planted duplicates: a pool of copies of one row - every score is shared, the lowest index wins
    Xd = np.ascontiguousarray(np.repeat(X[3:4], 9, 0))
    _, si, _ = _call(fn, b, phi, 0, Xd, omega, phase, w, eps)
    assert (si == 0).all()
    ex = (np.array([0, 1, 0], np.int64), np.array([0, 2, 2, 3], np.int64))
    _, si, _ = _call(fn, b, phi, 0, Xd, omega, phase, w, eps, excl=ex)
    assert (si[0] == 2).all() and (si[1] == 0).all() and (si[2] == 1).all()
    # a task with n_s = 0: -1 / -inf and zeros
    b0 = cpu_twin.CpuBatch(Zs, ys, np.zeros((b.T, 4), np.float32), 1, n_s=np.array([12, 0, 10], np.int32))
    b0.c.flags = ARD
    paths, sel_idx, sel_val = _call(fn, b0, phi, 0, X, omega, phase, w, eps)
    assert (sel_idx[1] == -1).all() and np.isneginf(sel_val[1]).all() and (paths[1] == 0).all()
    assert (sel_idx[0] >= 0).all() and np.array_equal(paths[0], p0[0])
