"""CPU: adkf_qei_pool without a GPU - every argument check before any launch, clean refusal with no device, the scratch size, the CPU
twin against the float64 restatement (tests/qei_ref.py), the identities the specification implies (monotone scores, the telescoping
sum, the unclipped score) on the twin's trace and incumbents, and the selection semantics on the twin."""
import ctypes as C

import numpy as np
import pytest
import torch

from adkf_ift_amd import _lib
from qei_ref import check_task, task_paths
from test_thompson_pool_cpu import ARD, BADARG, LAUNCH, MAXIMIZE, SIZE, WORKSPACE, _draws, _np_basis

bits = lambda a: np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def lib():
    try:
        return _lib.load()
    except (RuntimeError, OSError) as e:
        pytest.fail(f"libadkf_gp.so must be built (build() compiles it without a GPU): {e}")


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, ard=False, flags=0, x=True, S=4, m=64, q=2, best=False, missing=(), excl=(False, False),
               ws_short=0, scratch_short=0, scratch_offset=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    ss, mm, qq = max(S, 1), max(m, 1), max(q, 1)
    arr = dict(omega=torch.zeros(mm, d), phase=torch.zeros(mm), w=torch.zeros(T, ss, mm), eps=torch.zeros(T, ss, ns),
               sel_idx=torch.zeros(T, qq, dtype=torch.int64), sel_val=torch.zeros(T, qq), info=torch.zeros(T, dtype=torch.int32))
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    arr["ws"] = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_qei_pool_scratch_bytes(T, ns, S, m)
    scratch = torch.zeros(sb // 4 + 64)
    g = lambda n: None if n in missing else p(arr[n])
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_qei_pool(C.byref(b), p(phi), flags, p(X), rows, g("omega"), g("phase"), m, g("w"), g("eps"), S,
                             p(torch.zeros(T)) if best else None, p(e_idx) if excl[0] else None, p(e_off) if excl[1] else None, q, None, None,
                             g("sel_idx"), g("sel_val"), g("info"), g("ws"), nb - ws_short, C.c_void_p(scratch.data_ptr() + scratch_offset),
                             sb - scratch_short, None)


def test_the_library_exports_the_entry(lib):
    assert hasattr(lib, "adkf_qei_pool") and hasattr(lib, "adkf_qei_pool_scratch_bytes")
    assert _lib.QEI_SAMPLES_MAX == 256 and _lib.QEI_PICKS_MAX == 64


def test_scratch_bytes_do_not_depend_on_rows(lib):
    f = lib.adkf_qei_pool_scratch_bytes          # (T, ns_max, S, m): no rows among the arguments
    assert f(16, 128, 64, 1024) > 16 * 64 * 128 * 4
    assert f(16, 128, 64, 1024) < f(16, 128, 256, 1024) <= 64 << 20
    assert f(16, 128, 64, 64) == f(16, 128, 64, 4096)
    assert f(16, 128, 0, 1024) == 0 and f(16, 128, 257, 1024) == 0                       # S
    assert f(16, 128, 16, 100) == 0 and f(16, 128, 16, 32) == 0 and f(16, 128, 16, 4160) == 0   # m
    assert f(0, 128, 16, 64) == 0 and f(-1, 128, 16, 64) == 0 and f(16, 0, 16, 64) == 0  # T, ns_max
    # Thompson's size is what it was
    assert lib.adkf_thompson_pool_scratch_bytes(16, 128, 65, 1024) == 0


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, ard=True, best=True) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, S=256, m=4096, q=64, flags=MAXIMIZE, excl=(True, True)) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    for bit in (1, 4, 8, 16, 32, 64):
        assert _host_call(lib, flags=bit) == BADARG                            # any flag bit other than MAXIMIZE
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    for name in ("omega", "phase", "w", "eps", "sel_idx", "sel_val", "info", "ws"):
        assert _host_call(lib, missing=(name,)) == BADARG, name
    assert _host_call(lib, excl=(True, False)) == BADARG                       # excl_idx without excl_off
    assert _host_call(lib, S=0) == SIZE and _host_call(lib, S=257) == SIZE
    assert _host_call(lib, m=0) == SIZE and _host_call(lib, m=32) == SIZE and _host_call(lib, m=4160) == SIZE
    assert _host_call(lib, m=100) == SIZE                                      # not a multiple of 64
    assert _host_call(lib, q=0) == SIZE and _host_call(lib, q=65) == SIZE
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, ard=True, ws_short=1) == WORKSPACE
    assert _host_call(lib, scratch_short=1) == WORKSPACE
    assert _host_call(lib, scratch_offset=4) == BADARG                         # a scratch that is not 8-byte aligned


# ---- the CPU twin

def _twin():
    """The twin's entry.  Skips only where there is neither a built twin nor a compiler to build it, decided before any work; a twin that
    does not compile, or lacks the entry, fails."""
    import os
    import shutil

    from oracle import cpu_twin
    if not os.path.exists(cpu_twin.LIB) and shutil.which("g++") is None:   # no host compiler: the twin is checker-only
        pytest.skip("CPU twin not built and no g++ to build it")
    tw = cpu_twin.load()      # (a failed build raises)
    fn = tw.adkf_qei_pool     # a twin library without the entry point fails here
    assert tw.adkf_qei_pool_scratch_bytes(4, 8, 4, 64) == 0
    return cpu_twin, fn


N_S = (12, 9, 4)
PHI = np.array([[-2.0, 0.3, 0.8], [-1.0, 0.0, 1.2], [-3.0, 0.5, 0.5]], np.float32)


def _problem(kind, seed, rows=90, n_s=N_S, d=5):
    from oracle import cpu_twin

    T, ns = len(n_s), max(n_s)
    g = torch.Generator().manual_seed(seed)
    Zs = torch.randn(T, ns, d, generator=g) * torch.tensor([1.0, 0.5, 2.0, 1.5, 0.8])[:d] + 0.7
    ys = torch.randn(T, ns, generator=g)
    X = torch.randn(rows, d, generator=g) + 0.7
    b = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((T, 4), np.float32), kind, n_s=np.array(n_s, np.int32))
    return b, Zs.numpy(), ys.numpy(), np.array(n_s), np.ascontiguousarray(X.numpy(), np.float32), PHI[:T].copy()


def _call(fn, b, phi, flags, X, omega, phase, w, eps, q, best_f=None, excl=None, want=True):
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows, S, m = b.T, X.shape[0], w.shape[1], omega.shape[0]
    trace = np.full((T, q, rows), np.nan, np.float32) if want else None
    inc = np.full((T, q + 1, S), np.nan, np.float32) if want else None
    info = np.full(T, -9, np.int32)
    sel_idx, sel_val = np.full((T, q), -7, np.int64), np.full((T, q), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(omega), pp(phase), m, pp(w), pp(eps), S, pp(best_f), pp(e_idx), pp(e_off), q,
            pp(trace), pp(inc), pp(sel_idx), pp(sel_val), pp(info), None, 0, None, 0, None)
    assert rc == 0 and (info == 0).all()
    return dict(sel_idx=sel_idx, sel_val=sel_val, trace=trace, inc=inc)


def _best(ys, n_s, maximize):
    return np.array([(ys[t, :n].max() if maximize else ys[t, :n].min()) for t, n in enumerate(n_s)], np.float32)


@pytest.mark.parametrize("noisy", [True, False])
@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_twin_against_the_float64_restatement(kind, noisy):
    _, fn = _twin()
    b, Zs, ys, n_s, X, phi = _problem(kind, 150 + kind)
    q, S, m = 6, 80, 128
    omega, phase = _np_basis(kind, b.d, m, 3 + kind)
    w, eps = _draws(b.T, S, m, b.ns, 4)
    refs = [task_paths(Zs[t, :n_s[t]], ys[t, :n_s[t]], phi[t], kind, X, omega, phase, w[t], eps[t]) for t in range(b.T)]
    for flags in (0, MAXIMIZE):
        best = None if noisy else _best(ys, n_s, flags)
        o = _call(fn, b, phi, flags, X, omega, phase, w, eps, q, best_f=best)
        for t in range(b.T):
            worst = check_task(refs[t][0], refs[t][1], None if noisy else best[t], bool(flags), o["sel_idx"][t], o["sel_val"][t], o["trace"][t],
                               o["inc"][t], tag=(kind, noisy, flags, t))
            print(f"kind {kind} noisy {noisy} flags {flags} task {t}: worst error / bound {worst:.3e}; picks {o['sel_idx'][t].tolist()}")
            p = o["sel_idx"][t]
            assert bits(o["sel_val"][t]).tolist() == bits(o["trace"][t][np.arange(q), p]).tolist()      # sel_val == trace at the pick, bit for bit


def test_cpu_twin_ard_against_the_float64_restatement():
    import test_thompson_pool_ard_cpu as A

    _, fn = _twin()
    kind = 1
    b, Zs, ys, n_s, X, phi = A._problem(kind, 51, rows=23)
    q, S, m = 6, 80, 128
    omega, phase = _np_basis(kind, b.d, m, 4)
    w, eps = _draws(b.T, S, m, b.ns, 4)
    for flags, noisy in ((0, True), (MAXIMIZE, False)):
        best = None if noisy else _best(ys, n_s, flags)
        o = _call(fn, b, phi, flags, X, omega, phase, w, eps, q, best_f=best)
        for t in range(b.T):
            n = n_s[t]
            paths, sup = task_paths(Zs[t, :n], ys[t, :n], phi[t], kind, X, omega, phase, w[t], eps[t], ard=True)
            worst = check_task(paths, sup, None if noisy else best[t], bool(flags), o["sel_idx"][t], o["sel_val"][t], o["trace"][t], o["inc"][t],
                               tag=("ard", flags, t))
            print(f"ard flags {flags} task {t}: worst error / bound {worst:.3e}")


@pytest.mark.parametrize("flags", [0, MAXIMIZE])
def test_identities_on_the_twin(flags):
    from qei_ref import TOL

    _, fn = _twin()
    kind = 1
    b, Zs, ys, n_s, X, phi = _problem(kind, 160)
    q, S, m = 6, 80, 128
    omega, phase = _np_basis(kind, b.d, m, 7)
    w, eps = _draws(b.T, S, m, b.ns, 8)
    o = _call(fn, b, phi, flags, X, omega, phase, w, eps, q)
    tr, inc = o["trace"].astype(np.float64), o["inc"].astype(np.float64)
    for t in range(b.T):
        paths, _ = task_paths(Zs[t, :n_s[t]], ys[t, :n_s[t]], phi[t], kind, X, omega, phase, w[t], eps[t])
        delta = 2 * TOL * max(1.0, np.abs(paths).max()) + S * 2.0 ** -24 * tr[t].max()
        # scores never increase (every term is a clipped difference against an incumbent that only improves; rounding: one ulp of the sum)
        assert (tr[t, 1:] <= tr[t, :-1] + S * 2.0 ** -24 * tr[t, :-1]).all()
        # sum_j score_j(p_j) = (1 / S) sum_s |b^0 - b^q|: the MC q-EI of the batch
        lhs = o["sel_val"][t].astype(np.float64).sum()
        rhs = np.abs(inc[t, 0] - inc[t, q]).mean()
        print(f"task {t}: sum of sel_val {lhs:.6f}, mean incumbent movement {rhs:.6f}")
        assert abs(lhs - rhs) <= q * delta
        # the incumbents move one way only
        d = inc[t, 1:] - inc[t, :-1]
        assert (d >= 0).all() if flags else (d <= 0).all()
    # nothing clips: score_0(x) = |best_f - mean_s f_s(x)|
    far = np.full(b.T, -64.0 if flags else 64.0, np.float32)
    o = _call(fn, b, phi, flags, X, omega, phase, w, eps, 1, best_f=far)
    for t in range(b.T):
        paths, _ = task_paths(Zs[t, :n_s[t]], ys[t, :n_s[t]], phi[t], kind, X, omega, phase, w[t], eps[t])
        assert np.abs(paths).max() < 60.0
        ref = np.abs(float(far[t]) - paths.mean(0))
        err = np.abs(o["trace"][t, 0] - ref).max()
        assert err <= 2 * TOL * max(1.0, np.abs(paths).max()) + S * 2.0 ** -24 * ref.max(), (t, err)


def test_selection_semantics_on_the_twin():
    _, fn = _twin()
    kind = 1
    b, Zs, ys, n_s, X, phi = _problem(kind, 170, rows=70)
    X[10] = X[3]; X[41] = X[3]; X[69] = X[20]          # exact duplicate rows: bit-equal scores
    q, S, m = 5, 16, 64
    omega, phase = _np_basis(kind, b.d, m, 8)
    w, eps = _draws(b.T, S, m, b.ns, 9)
    o = _call(fn, b, phi, 0, X, omega, phase, w, eps, q)
    tr = o["trace"]
    assert np.array_equal(bits(tr[:, :, 10]), bits(tr[:, :, 3])) and np.array_equal(bits(tr[:, :, 69]), bits(tr[:, :, 20]))
    for t in range(b.T):
        picks = o["sel_idx"][t].tolist()
        assert len(set(picks)) == q and min(picks) >= 0
        for j, p in enumerate(picks):   # the pick is the lowest index among the rows of its score that are still free
            same = [r for r in range(70) if bits(tr[t, j, r:r + 1])[0] == bits(tr[t, j, p:p + 1])[0] and r not in picks[:j]]
            assert p == min(same), (t, j, p, same)
    # a pool of copies of one row: every score is shared, the picks are 0, 1, 2, ... whatever the scores are (a zero step included:
    # after the first copy is picked no copy improves on the incumbents)
    Xd = np.ascontiguousarray(np.repeat(X[3:4], 9, 0))
    o = _call(fn, b, phi, 0, Xd, omega, phase, w, eps, 4)
    assert (o["sel_idx"] == np.arange(4)[None]).all()
    assert (o["trace"][:, 1:] == 0).all() and (o["sel_val"][:, 1:] == 0).all()       # all-zero steps pick the lowest eligible row
    ex = (np.array([-3, 0, 1, 99, 0], np.int64), np.array([0, 4, 4, 5], np.int64))   # ascending, with entries outside the pool
    o = _call(fn, b, phi, 0, Xd, omega, phase, w, eps, 3, excl=ex)
    assert o["sel_idx"].tolist() == [[2, 3, 4], [0, 1, 2], [1, 2, 3]]
    # rows < q, and a task that may select nothing
    Xs = np.ascontiguousarray(X[:3])
    lists = [[1], [], [0, 1, 2]]
    ex = (np.array([i for l in lists for i in l], np.int64), np.array([0, 1, 1, 4], np.int64))
    o = _call(fn, b, phi, 0, Xs, omega, phase, w, eps, 5, excl=ex)
    assert sorted(o["sel_idx"][0, :2].tolist()) == [0, 2] and (o["sel_idx"][0, 2:] == -1).all() and np.isneginf(o["sel_val"][0, 2:]).all()
    assert sorted(o["sel_idx"][1, :3].tolist()) == [0, 1, 2] and (o["sel_idx"][1, 3:] == -1).all()
    assert (o["sel_idx"][2] == -1).all() and np.isneginf(o["sel_val"][2]).all()
    assert np.array_equal(bits(o["inc"][2, 0]), bits(o["inc"][2, 5]))                 # no pick: the state stays
    assert np.array_equal(bits(o["inc"][0, 2]), bits(o["inc"][0, 5]))
    # trace = inc = NULL: the same selection, bit for bit
    o2 = _call(fn, b, phi, 0, Xs, omega, phase, w, eps, 5, excl=ex, want=False)
    assert np.array_equal(o2["sel_idx"], o["sel_idx"]) and np.array_equal(bits(o2["sel_val"]), bits(o["sel_val"]))
