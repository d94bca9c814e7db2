"""CPU: adkf_thompson_pool without a GPU - every argument check before any launch, clean refusal with no device, the CPU twin
against a float64 restatement of the specification (include/adkf_gp.h), the selection semantics on the twin, the law of
gp_ops.rff_basis, and the mean of the paths against the posterior mean."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from adkf_ift_amd import _lib
from test_predict_pool_cpu import select_ref

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD, MAXIMIZE = 4, 2


@pytest.fixture(scope="module")
def lib():
    try:
        return _lib.load()
    except (RuntimeError, OSError) as e:
        pytest.fail(f"libadkf_gp.so must be built (build() compiles it without a GPU): {e}")


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, ard=False, flags=0, x=True, S=4, m=64, missing=(), excl=(False, False), ws_short=0,
               scratch_short=0, scratch_offset=0):
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
    return lib.adkf_thompson_pool(C.byref(b), p(phi), flags, p(X), rows, g("omega"), g("phase"), m, g("w"), g("eps"), S,
                                  p(e_idx) if excl[0] else None, p(e_off) if excl[1] else None, None, g("sel_idx"), g("sel_val"), g("info"),
                                  g("ws"), nb - ws_short, C.c_void_p(scratch.data_ptr() + scratch_offset), sb - scratch_short, None)


def test_scratch_bytes_do_not_depend_on_rows(lib):
    f = lib.adkf_thompson_pool_scratch_bytes
    assert f(16, 128, 16, 1024) > 16 * 16 * 128 * 4
    assert f(16, 128, 16, 1024) < f(16, 128, 64, 1024) <= 64 << 20
    assert f(16, 128, 0, 1024) == 0 and f(16, 128, 65, 1024) == 0 and f(16, 128, 16, 100) == 0 and f(0, 128, 16, 64) == 0


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, S=64, m=4096, flags=MAXIMIZE, excl=(True, True)) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, ard=True) == BADARG                                 # ARD: out of scope
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
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, scratch_short=1) == WORKSPACE
    assert _host_call(lib, scratch_offset=4) == BADARG                         # a scratch that is not 8-byte aligned


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
    fn = tw.adkf_thompson_pool   # a twin library without the entry point fails here
    sb = tw.adkf_thompson_pool_scratch_bytes
    assert sb(4, 8, 4, 64) == 0
    return cpu_twin, fn


def _np_basis(kind, d, m, seed):
    """A basis with the laws of gp_ops.rff_basis, drawn with numpy (the twin tests do not depend on the package's generator)."""
    g = np.random.default_rng(seed)
    om = g.standard_normal((m, d))
    if kind == 1:
        om = om / np.sqrt(g.chisquare(5, (m, 1)) / 5.0)
    return om.astype(np.float32), (g.random(m) * 2 * math.pi).astype(np.float32)


def paths_ref(zs, ys, phi, kind, X, omega, phase, w, eps):
    """The specification in float64 for one task: zs [n, d], ys [n], X [rows, d], w [S, m], eps [S, >= n] -> f [S, rows]."""
    from oracle import gp_oracle as O

    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    zs, ys, X, omega, phase, w, eps, phi = (t(a) for a in (zs, ys, X, omega, phase, w, eps, phi))
    n, m = zs.shape[0], omega.shape[0]
    noise, os_, ls = O.transform_phi(phi)
    mu = zs.mean(0)
    feat = lambda x: torch.sqrt(2.0 * os_ / m) * torch.cos((x - mu) @ omega.T / ls + phase)
    A = O.kernel_matrix(zs, zs, os_, ls, kind) + noise * torch.eye(n, dtype=torch.float64)
    r = ys[:, None] - feat(zs) @ w.T - torch.sqrt(noise) * eps[:, :n].T
    v = torch.linalg.solve(A, r)
    return (feat(X) @ w.T + O.kernel_matrix(X, zs, os_, ls, kind) @ v).T.numpy()


def _problem(kind, seed, rows=23, T=3, ns=12, d=5):
    from oracle import cpu_twin

    n_s = np.array([12, 7, 10][:T], np.int32)
    g = torch.Generator().manual_seed(seed)
    Zs = torch.randn(T, ns, d, generator=g) * torch.tensor([1.0, 0.5, 2.0, 1.5, 0.8]) + 0.7
    ys = torch.randn(T, ns, generator=g)
    X = torch.randn(rows, d, generator=g) + 0.7
    phi = torch.tensor([[-2.0, 0.3, 0.8], [-1.0, 0.0, 1.2], [-3.0, 0.5, 0.5]])[:T].numpy().astype(np.float32)
    b = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((T, 4), np.float32), kind, n_s=n_s)
    return b, Zs.numpy(), ys.numpy(), n_s, np.ascontiguousarray(X.numpy(), np.float32), phi


def _draws(T, S, m, ns, seed):
    g = np.random.default_rng(seed)
    return g.standard_normal((T, S, m)).astype(np.float32), g.standard_normal((T, S, ns)).astype(np.float32)


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


@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_twin_against_the_float64_restatement(kind):
    _, fn = _twin()
    b, Zs, ys, n_s, X, phi = _problem(kind, 50 + kind)
    S, m = 5, 128
    omega, phase = _np_basis(kind, b.d, m, 3 + kind)
    w, eps = _draws(b.T, S, m, b.ns, 4)
    for flags in (0, MAXIMIZE):
        paths, sel_idx, sel_val = _call(fn, b, phi, flags, X, omega, phase, w, eps)
        for t in range(b.T):
            n = n_s[t]
            ref = paths_ref(Zs[t, :n], ys[t, :n], phi[t], kind, X, omega, phase, w[t], eps[t])
            err = np.abs(paths[t] - ref).max()
            print(f"kind {kind} flags {flags} task {t}: |paths - ref| max {err:.3e}, |ref| max {np.abs(ref).max():.3e}")
            assert err <= 1e-4 * max(1.0, np.abs(ref).max()), (t, err)
            for q in range(S):
                score = paths[t, q] if flags & MAXIMIZE else -paths[t, q]
                idx, val = select_ref(score, 1)
                assert sel_idx[t, q] == idx[0] and sel_val[t, q].view(np.int32) == val[0].view(np.int32)


def test_selection_semantics_on_the_twin():
    from oracle import cpu_twin

    _, fn = _twin()
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
    paths, sel_idx, sel_val = _call(fn, b0, phi, 0, X, omega, phase, w, eps)
    assert (sel_idx[1] == -1).all() and np.isneginf(sel_val[1]).all() and (paths[1] == 0).all()
    assert (sel_idx[0] >= 0).all() and np.array_equal(paths[0], p0[0])


@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_rff_basis_draws_the_right_law(kernel):
    """(1/m) sum_j 2 cos(w_j.x + b_j) cos(w_j.y + b_j) estimates kappa(|x - y|) at unit lengthscale; the terms lie in [-2, 2], so by
    Hoeffding the estimate is within sqrt(8 ln(2 / delta) / m) of it with probability 1 - delta (delta = 1e-9; 0.0256 at m = 2^18)."""
    from adkf_ift_amd import gp_ops

    d, m = 4, 1 << 18
    g = torch.Generator().manual_seed(11)
    omega, phase = gp_ops.rff_basis(kernel, d, m, generator=g)
    assert omega.shape == (m, d) and phase.shape == (m,) and omega.dtype == torch.float32 and phase.dtype == torch.float32
    assert float(phase.min()) >= 0.0 and float(phase.max()) < 2 * math.pi + 1e-6
    omega, phase = omega.double().cpu(), phase.double().cpu()
    bound = math.sqrt(8.0 * math.log(2.0 / 1e-9) / m)
    x = torch.tensor([0.3, -0.2, 0.5, 0.1], dtype=torch.float64)
    u = torch.tensor([0.5, 0.5, -0.5, 0.5], dtype=torch.float64)   # a unit vector
    for dist in (0.0, 0.3, 1.0, 2.0, 4.0):
        y = x + dist * u
        est = float((2.0 * torch.cos(omega @ x + phase) * torch.cos(omega @ y + phase)).mean())
        if kernel == "rbf":
            k = math.exp(-0.5 * dist * dist)
        else:
            k = (1.0 + math.sqrt(5.0) * dist + 5.0 / 3.0 * dist * dist) * math.exp(-math.sqrt(5.0) * dist)
        print(f"{kernel} |x - y| = {dist}: estimate {est:.5f}, kernel {k:.5f}, bound {bound:.4f}")
        assert abs(est - k) <= bound, (kernel, dist, est, k)
    with pytest.raises(ValueError):
        gp_ops.rff_basis("tanimoto", d, 64)
    # the same generator state gives the same basis
    a = gp_ops.rff_basis(kernel, d, 128, generator=torch.Generator().manual_seed(5))
    c = gp_ops.rff_basis(kernel, d, 128, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_the_mean_of_the_paths_is_the_posterior_mean():
    """Over standard normal w, eps the mean of f is K A^-1 y exactly, whatever m is: N = 4096 samples, per row
    |mean_hat - K A^-1 y| <= 6 std_hat / sqrt(N).  Catches a wrong sign or scale in the update term that a reference with the same
    mistake would share."""
    from oracle import cpu_twin
    from oracle import gp_oracle as O

    _, fn = _twin()
    kind, n, d, rows, m, S, calls = 1, 24, 6, 200, 4096, 64, 64
    g = torch.Generator().manual_seed(2)
    Zs = torch.randn(1, n, d, generator=g) * 0.8 + 0.2
    ys = torch.sin(Zs[..., :3].sum(-1)) + 0.1 * torch.randn(1, n, generator=g)
    X = np.ascontiguousarray((torch.randn(rows, d, generator=g) * 0.8 + 0.2).numpy(), np.float32)
    phi = np.array([[-2.5, 0.4, 1.0]], np.float32)
    b = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((1, 4), np.float32), kind)
    omega, phase = _np_basis(kind, d, m, 21)
    tot, tot2 = np.zeros(rows), np.zeros(rows)
    for c in range(calls):
        w, eps = _draws(1, S, m, n, 1000 + c)
        paths, _, _ = _call(fn, b, phi, 0, X, omega, phase, w, eps)
        p = paths[0].astype(np.float64)
        tot += p.sum(0); tot2 += (p * p).sum(0)
    N = calls * S
    mean_hat = tot / N
    std_hat = np.sqrt(np.maximum(tot2 / N - mean_hat ** 2, 0.0) * N / (N - 1))
    pt = torch.from_numpy(phi[0]).double()
    m_ref, _ = O.predict(Zs[0].double(), ys[0].double(), torch.from_numpy(X).double(), pt, kind)
    z = np.abs(mean_hat - m_ref.numpy()) / (std_hat / math.sqrt(N))
    print(f"N = {N}: max |z| over the {rows} rows = {z.max():.2f}; std_hat in [{std_hat.min():.3f}, {std_hat.max():.3f}]")
    assert N >= 4000 and std_hat.min() > 0
    assert z.max() <= 6.0, z.max()
