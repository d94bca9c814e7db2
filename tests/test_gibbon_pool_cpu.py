"""CPU: adkf_gibbon_pool without a GPU - the entry is exported, clean refusal with no device, every argument check before any launch,
gp_ops.gibbon_pool's argument handling, the CPU twin against the float64 reference of gibbon_ref.py (isotropic and ARD, both senses,
all branches of h), and the semantics of the batch on the twin: step 0 is a q = 1 call, scores only fall, and the picks of a smooth
1-d pool are not mutual neighbours although the top-q of step 0 are."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import believer_ref as B
import gibbon_ref as R
from adkf_ift_amd import _lib
from test_believer_pool_ard_cpu import ard_posterior
from test_predict_pool_cpu import _problem, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE, LOG_EI = 1, 2, 16


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, q=4, S=5, ard=False, flags=0, x=True, ystar=True, sel=(True, True), extra=True,
               trace=False, excl=(False, False), info=True, ws=True, ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    qq = min(max(q, 1), 64)
    ystar_t = torch.zeros(T, min(max(S, 1), 64))
    tr = torch.zeros(T * qq * max(rows, 1))
    inf = torch.zeros(T, dtype=torch.int32)
    sel_idx, out = torch.zeros(T * qq, dtype=torch.int64), [torch.zeros(T * qq) for _ in range(3)]
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_believer_pool_scratch_bytes(T, ns, d, qq)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_gibbon_pool(C.byref(b), p(phi), flags, p(X), rows, p(ystar_t) if ystar else None, S, p(e_idx) if excl[0] else None,
                                p(e_off) if excl[1] else None, q, p(tr) if trace else None, p(sel_idx) if sel[0] else None,
                                p(out[0]) if sel[1] else None, p(out[1]) if extra else None, p(out[2]) if extra else None,
                                p(inf) if info else None, p(wsb) if ws else None, nb - ws_short,
                                C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_the_entry_is_exported(lib):
    assert "adkf_gibbon_pool" in _lib.SIGNATURES
    fn = lib.adkf_gibbon_pool   # a library without the entry point fails here
    assert fn.restype is C.c_int and len(fn.argtypes) == 21
    assert len(_lib.SIGNATURES["adkf_gibbon_pool"][1]) == len(_lib.SIGNATURES["adkf_believer_pool"][1]) + 1   # ystar, S for best_f


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, rows=0, x=False, extra=False) == LAUNCH
    assert _host_call(lib, ard=True, d=12, rows=7, q=3, S=1) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, q=64, S=64, trace=True, excl=(True, True), flags=MAXIMIZE) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    assert _host_call(lib, ystar=False) == BADARG
    assert _host_call(lib, sel=(False, True)) == BADARG
    assert _host_call(lib, sel=(True, False)) == BADARG
    assert _host_call(lib, info=False) == BADARG
    assert _host_call(lib, ws=False) == BADARG
    assert _host_call(lib, excl=(True, False)) == BADARG                       # excl_idx without excl_off
    for q in (0, -3):
        assert _host_call(lib, q=q) == BADARG
    for S in (0, -1):
        assert _host_call(lib, S=S) == BADARG
    assert _host_call(lib, scratch_off=4) == BADARG                            # a misaligned scratch
    for bit in (LATENT, 4, 8, LOG_EI, 32):
        assert _host_call(lib, flags=bit) == BADARG                            # flag bits other than MAXIMIZE
        assert _host_call(lib, flags=bit | MAXIMIZE) == BADARG
    assert _host_call(lib, q=65) == SIZE
    assert _host_call(lib, S=65) == SIZE
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, ard=True, ws_short=1) == WORKSPACE
    assert _host_call(lib, scratch_short=1) == WORKSPACE


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False, T=3, d=5)
    for q in (0, -1, 65):
        with pytest.raises(ValueError, match="q must be"):
            gp_ops.gibbon_pool(iso, None, None, ystar=torch.zeros(3, 4), q=q)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.gibbon_pool(types.SimpleNamespace(nq=3, ard=False, T=3, d=5), None, None, ystar=torch.zeros(3, 4), q=4)
    for bad in (None, torch.zeros(4), torch.zeros(4, 4), torch.zeros(3, 4, 1)):
        with pytest.raises(ValueError, match="ystar must be"):
            gp_ops.gibbon_pool(iso, None, None, ystar=bad, q=4)
    for S in (0, 65):
        with pytest.raises(ValueError, match="samples S must be"):
            gp_ops.gibbon_pool(iso, None, None, ystar=torch.zeros(3, S), q=4)


def test_the_bo_loop_refuses_an_unknown_batch():
    from adkf_ift_amd import bayes_opt as BO

    X, y = torch.randn(20, 3), torch.randn(20)
    with pytest.raises(ValueError, match="batch must be"):
        BO.run_gp_mes_bo_batched(X, y, 4, 2, 1, "matern", "cpu", 10, 0.01, True, rngs=[np.random.default_rng(0)], batch="greedy")


# ---- the twin
def _gb_twin():
    cpu_twin, _ = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_gibbon_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_gibbon_pool"]
    return fn


def gb_call(fn, b, phi, flags, X, ystar, q, excl=None, want_trace=True):
    """The twin's adkf_gibbon_pool on host arrays: (sel_idx, sel_val, sel_mean, sel_var, trace, info)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    ystar = np.ascontiguousarray(ystar, np.float32)
    trace = np.full((T, q, rows), np.nan, np.float32) if want_trace else None
    info = np.empty(T, np.int32)
    sel_idx = np.full((T, q), -7, np.int64)
    sel_val, sel_mean, sel_var = (np.full((T, q), np.nan, np.float32) for _ in range(3))
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(ystar), ystar.shape[1], pp(e_idx), pp(e_off), q, pp(trace), pp(sel_idx), pp(sel_val),
            pp(sel_mean), pp(sel_var), pp(info), None, 0, None, 0, None)
    assert rc == 0 and (info == 0).all()
    return sel_idx, sel_val, sel_mean, sel_var, trace, info


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_the_reference_itself():
    """0 < h < 1, increasing to the left, h -> 1, the fast float64 h against mpmath, the hand-off to NaN, and the identity the greedy
    score rests on: alpha(B + x) - alpha(B) = score_j(x) with alpha(B) = 1/2 log |R_B| + sum a."""
    xs = np.linspace(-30.0, 10.0, 161)
    h = np.array([R.h_ref(x) for x in xs])
    assert (h > 0).all() and (h < 1).all() and (np.diff(h) < 0).all()
    assert abs(R.h_ref(-30.0) - (1.0 - 1.0 / 900.0)) < 1e-5 and abs(R.h_ref(0.0) - 2.0 / np.pi) < 1e-15
    assert np.abs(R._h64v(xs) - h).max() < 2e-12   # (gamma + tau loses two digits just above gamma = -8)
    assert all(np.isnan(R.h_ref(x)) and np.isnan(R._h64(x)) for x in (np.nan, np.inf, -np.inf))
    b, Zs, ys, n_s, X, phi, _ = _problem(1, False, 50, rows=30)
    post = B.posterior(Zs[0, :n_s[0]], ys[0, :n_s[0]], X, phi[0], 1)
    m, S, noise, _ = post
    ystar = R.ystar_above(post, 5, True)
    a = R.a_ref(m, S.diagonal(), noise, ystar, True)[0]

    def alpha(B_):
        C_ = S[np.ix_(B_, B_)] + noise * np.eye(len(B_))
        sd = np.sqrt(C_.diagonal())
        return 0.5 * np.linalg.slogdet(C_ / np.outer(sd, sd))[1] + a[B_].sum()

    picks = [4, 17, 9]
    steps = R.gibbon_steps(post, ystar, True, picks + [-1])
    for j in range(1, 4):
        for x in (0, 11, 23):
            assert abs(alpha(picks[:j] + [x]) - alpha(picks[:j]) - steps[j][0][x]) < 1e-12, (j, x)
    assert np.array_equal(steps[0][0], a)


CASES = [(0, False, 1), (1, False, 5), (0, True, 64), (1, True, 5), (1, False, 64)]   # (kind, ARD, S)


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("kind,ard,S", CASES)
def test_cpu_twin_against_the_reference(kind, ard, S, maximize):
    fn = _gb_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(kind, ard, 60 + kind + 2 * ard, rows=40)
    q = 6
    flags = MAXIMIZE if maximize else 0
    posts = [(ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], X, phi[t], kind) if ard else
              B.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], kind)) for t in range(b.T)]
    seen = np.zeros(3, int)   # gamma > -1, -12 < gamma <= -1, gamma <= -12
    for make in (R.ystar_above, R.ystar_below):
        ystar = np.stack([make(posts[t], S, maximize) for t in range(b.T)])
        sel_idx, sel_val, sel_mean, sel_var, trace, _ = gb_call(fn, b, phi, flags, X, ystar, q)
        for t in range(b.T):
            m, S_, _, _ = posts[t]
            gamma = R.gamma_of(m, S_.diagonal(), ystar[t], maximize)
            seen += [(gamma > -1).sum(), ((gamma > -12) & (gamma <= -1)).sum(), (gamma <= -12).sum()]
            worst = R.check_task(posts[t], ystar[t], maximize, sel_idx[t], sel_val[t], sel_mean[t], sel_var[t], trace[t], tag=(kind, ard, S, t))
            print(f"kind {kind} ard {ard} S {S} {make.__name__} task {t}: picks {sel_idx[t].tolist()}, worst trace error / bound {worst:.2e}")
            assert len(set(sel_idx[t].tolist())) == q and (sel_idx[t] >= 0).all() and np.isfinite(sel_val[t]).all()
            assert (trace[t, 0] >= 0).all()
    assert (seen[:2] > 0).all() and (seen[2] > 0 or S == 1), seen   # (one sample reaches one branch on the left)


def test_semantics_on_the_twin():
    fn = _gb_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(1, False, 40, rows=70)
    X[10] = X[3]; X[41] = X[3]          # exact duplicate rows
    lists = [[5, 6, 17], [], sorted(set(range(70)) - {3, 10, 41, 50})]
    excl = (np.array([i for l in lists for i in l], np.int64), np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64))
    posts = [B.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], 1) for t in range(b.T)]
    for flags in (0, MAXIMIZE):
        q = 8
        ystar = np.stack([R.ystar_above(posts[t], 5, bool(flags)) for t in range(b.T)])
        sel_idx, sel_val, sel_mean, sel_var, trace, _ = gb_call(fn, b, phi, flags, X, ystar, q, excl=excl)
        one = gb_call(fn, b, phi, flags, X, ystar, 1, excl=excl)
        for t in range(b.T):
            got = [p for p in sel_idx[t].tolist() if p >= 0]
            assert len(set(got)) == len(got) and not set(got) & set(lists[t]), t
            R.check_task(posts[t], ystar[t], bool(flags), sel_idx[t], sel_val[t], sel_mean[t], sel_var[t], trace[t], excluded=lists[t], tag=(flags, t))
            # step 0 is a q = 1 call, bit for bit
            assert one[0][t, 0] == sel_idx[t, 0] and _bits(one[1][t, 0]) == _bits(sel_val[t, 0])
            assert np.array_equal(_bits(one[4][t, 0]), _bits(trace[t, 0]))
            assert _bits(one[2][t, 0]) == _bits(sel_mean[t, 0]) and _bits(one[3][t, 0]) == _bits(sel_var[t, 0])
            # a pick only lowers scores: the variance ratio is at most 1
            for j in range(1, q):
                assert (trace[t, j] <= trace[t, 0]).all() and (trace[t, j] <= trace[t, j - 1]).all(), (flags, t, j)
            # exact duplicates score alike at every step
            for j in range(q):
                assert _bits(trace[t, j, 10]) == _bits(trace[t, j, 41]) == _bits(trace[t, j, 3]), (t, j)
        # task 2 may take 3, 10, 41 and 50 only: then the -1 / -inf / 0 / 0 tail
        assert (sel_idx[2, 4:] == -1).all() and np.isneginf(sel_val[2, 4:]).all() and (sel_idx[2, :4] >= 0).all()
        assert (sel_mean[2, 4:] == 0).all() and (sel_var[2, 4:] == 0).all()
        # trace == NULL: the same selection, bit for bit
        again = gb_call(fn, b, phi, flags, X, ystar, q, excl=excl, want_trace=False)
        assert again[4] is None and np.array_equal(again[0], sel_idx)
        for a, c in zip(again[1:4], (sel_val, sel_mean, sel_var)):
            assert np.array_equal(_bits(a), _bits(c))


def test_the_batch_is_not_a_set_of_neighbours():
    """What the entry is for.  A smooth 1-d pool of 200 rows: the top-6 of the single-point score are neighbours of the winner; the
    greedy batch starts at the same row and then leaves its neighbourhood - no two picks are adjacent rows."""
    from oracle import cpu_twin

    fn = _gb_twin()
    g = np.random.default_rng(3)
    rows, ns, q = 200, 8, 6
    X = np.linspace(0.0, 1.0, rows, dtype=np.float32)[:, None]
    Zs = g.uniform(0.0, 1.0, (1, ns, 1)).astype(np.float32)
    ys = np.sin(6.0 * Zs[..., 0]).astype(np.float32)
    phi = np.array([[-3.0, 0.5, -1.5]], np.float32)        # a lengthscale of ~0.2: neighbouring rows are almost one observation
    b = cpu_twin.CpuBatch(Zs, ys, np.zeros((1, 4), np.float32), 0)
    post = B.posterior(Zs[0], ys[0], X, phi[0], 0)
    ystar = R.ystar_above(post, 8, True)[None]
    sel_idx, sel_val, _, _, trace, _ = gb_call(fn, b, phi, MAXIMIZE, X, ystar, q)
    top = np.argsort(-trace[0, 0], kind="stable")[:q]
    picks = sel_idx[0]
    print(f"top-{q} of the single-point score {top.tolist()}, the greedy batch {picks.tolist()}")
    assert picks[0] == top[0]
    assert top.max() - top.min() == q - 1, "the top-q are a run of neighbouring rows"
    gaps = np.abs(picks[:, None] - picks[None, :])[np.triu_indices(q, 1)]
    assert gaps.min() > 1, "no two picks of the batch are adjacent rows"
    assert set(picks.tolist()) != set(top.tolist())


def test_a_nan_sample_a_small_pool_and_a_skipped_task():
    fn = _gb_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(0, False, 41, rows=70)
    ystar = np.full((b.T, 4), 3.0, np.float32) + np.arange(4, dtype=np.float32) * 0.25
    full = gb_call(fn, b, phi, MAXIMIZE, X, ystar, 5)
    for bad in (np.nan, np.inf, -np.inf):
        ys2 = ystar.copy()
        ys2[1, 2] = bad
        sel_idx, sel_val, sel_mean, sel_var, trace, _ = gb_call(fn, b, phi, MAXIMIZE, X, ys2, 5)
        assert np.isnan(trace[1]).all() and (sel_idx[1] == -1).all() and np.isneginf(sel_val[1]).all()
        assert (sel_mean[1] == 0).all() and (sel_var[1] == 0).all()
        for t in (0, 2):
            assert np.array_equal(sel_idx[t], full[0][t]) and np.array_equal(_bits(trace[t]), _bits(full[4][t]))
    # a pool of 9 rows with q = 16: nine picks, then the tail; an empty pool: the tail only
    sel_idx, sel_val, sel_mean, sel_var, _, _ = gb_call(fn, b, phi, MAXIMIZE, X[:9], ystar, 16)
    for t in range(b.T):
        assert sorted(sel_idx[t, :9].tolist()) == list(range(9)) and (sel_idx[t, 9:] == -1).all()
        assert np.isfinite(sel_val[t, :9]).all() and np.isneginf(sel_val[t, 9:]).all()
        assert (sel_mean[t, 9:] == 0).all() and (sel_var[t, 9:] == 0).all() and (sel_var[t, :9] > 0).all()
    sel_idx, sel_val, sel_mean, sel_var, _, _ = gb_call(fn, b, phi, MAXIMIZE, X[:0], ystar, 3)
    assert (sel_idx == -1).all() and np.isneginf(sel_val).all() and (sel_mean == 0).all() and (sel_var == 0).all()
    # a task with n_s == 0 is skipped: -1 / -inf, zeros in trace; the others are what they are without it
    b.n_s[1] = 0
    sel_idx, sel_val, sel_mean, sel_var, trace, _ = gb_call(fn, b, phi, MAXIMIZE, X, ystar, 5)
    assert (sel_idx[1] == -1).all() and np.isneginf(sel_val[1]).all() and (trace[1] == 0).all() and (sel_mean[1] == 0).all()
    for t in (0, 2):
        assert np.array_equal(sel_idx[t], full[0][t]) and np.array_equal(_bits(trace[t]), _bits(full[4][t]))
