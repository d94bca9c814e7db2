"""CPU: adkf_liar_pool without a GPU - the entry and its argument count, clean refusal with no device, every argument check before
any launch, gp_ops.liar_pool's argument handling, the BO loop's new refusals, the CPU twin against the float64 reference of
liar_ref.py (which rebuilds the posterior with the picks appended: no recursion), and the semantics of the lie on the twin."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import liar_ref as R
from adkf_ift_amd import _lib
from test_believer_pool_cpu import _bv_twin, bv_call
from test_predict_pool_cpu import _problem, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE, LOG_EI = 1, 2, 16


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, q=4, ard=False, flags=0, x=True, best=True, lie=True, labels=False, stride=0, sel=(True, True),
               extra=True, trace=False, excl=(False, False), info=True, ws=True, ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    qq = min(max(q, 1), 64)
    tr = torch.zeros(T * qq * max(rows, 1))
    inf, bf, lv, lab = torch.zeros(T, dtype=torch.int32), torch.zeros(T), torch.zeros(T), torch.zeros(T * max(rows, 1))
    sel_idx, out = torch.zeros(T * qq, dtype=torch.int64), [torch.zeros(T * (qq + 1)) for _ in range(5)]
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_liar_pool_scratch_bytes(T, ns, d, q)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_liar_pool(C.byref(b), p(phi), flags, p(X), rows, p(bf) if best else None, p(lv) if lie else None,
                              p(lab) if labels else None, stride, p(e_idx) if excl[0] else None, p(e_off) if excl[1] else None, q,
                              p(tr) if trace else None, p(sel_idx) if sel[0] else None, p(out[0]) if sel[1] else None,
                              p(out[1]) if extra else None, p(out[2]) if extra else None, p(out[3]) if extra else None,
                              p(out[4]) if extra else None, p(inf) if info else None, p(wsb) if ws else None, nb - ws_short,
                              C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_entry_is_exported_with_its_arguments(lib):
    assert hasattr(lib, "adkf_liar_pool") and hasattr(lib, "adkf_liar_pool_scratch_bytes")
    restype, argtypes = _lib.SIGNATURES["adkf_liar_pool"]
    assert restype is C.c_int and len(argtypes) == 25
    assert argtypes[4] is C.c_int64 and argtypes[8] is C.c_int64 and argtypes[11] is C.c_int32
    assert len(_lib.SIGNATURES["adkf_liar_pool_scratch_bytes"][1]) == 4


def test_scratch_is_the_believers_plus_z(lib):
    f, g = lib.adkf_liar_pool_scratch_bytes, lib.adkf_believer_pool_scratch_bytes
    for T, ns, d, q in ((16, 128, 256, 8), (3, 48, 16, 1), (2, 1024, 12, 64)):
        extra = f(T, ns, d, q) - g(T, ns, d, q)
        assert 4 * T * q <= extra <= 12 * T * q + 512, (T, ns, d, q, extra)   # z [T, q] and its float64 twin, each rounded up to 256 bytes
    assert f(16, 128, 256, 0) == 0 and f(16, 128, 256, 65) == 0 and f(0, 128, 256, 8) == 0
    assert f(16, 128, 256, 8) < 1 << 20


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, ard=True, lie=False, labels=True, stride=10) == LAUNCH
    assert _host_call(lib, rows=0, x=False, extra=False) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, q=64, trace=True, labels=True, excl=(True, True), flags=MAXIMIZE | LOG_EI) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
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
    assert _host_call(lib, lie=False, labels=False) == BADARG                  # no value source: that call is adkf_believer_pool
    for stride in (1, 9, 11, -10, 30):
        assert _host_call(lib, labels=True, stride=stride) == BADARG           # a stride other than 0 and rows
    assert _host_call(lib, labels=False, stride=10) == BADARG                  # a stride without labels
    for bit in [LATENT, 4, 8] + [1 << k for k in range(5, 31)]:
        assert _host_call(lib, flags=bit) == BADARG                            # flag bits other than MAXIMIZE | LOG_EI
        assert _host_call(lib, flags=bit | MAXIMIZE | LOG_EI) == BADARG
    assert _host_call(lib, flags=-(1 << 31)) == BADARG
    assert _host_call(lib, q=65) == SIZE
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, scratch_short=1) == WORKSPACE


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False)
    for q in (0, -1, 65):
        with pytest.raises(ValueError, match="q must be"):
            gp_ops.liar_pool(iso, None, None, best_f=None, q=q, lie="min")
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.liar_pool(types.SimpleNamespace(nq=3, ard=False), None, None, best_f=None, q=4, lie="min")


def test_bo_loop_refusals():
    from adkf_ift_amd import bayes_opt as BO

    kw = dict(num_init_points=3, num_bo_iters=2, kernel_type="matern", device="cpu", init_from=0, noise_init=0.01, noise_prior=True, rngs=[])
    X, y = torch.zeros(8, 2), torch.arange(8.0)
    with pytest.raises(ValueError, match="batch must be"):
        BO.run_gp_ei_bo_batched(X, y, query_batch_size=1, batch="greedy", **kw)
    with pytest.raises(ValueError, match="refit_every"):
        BO.run_gp_ei_bo_batched(X, y, query_batch_size=2, refit_every=3, **kw)
    with pytest.raises(ValueError, match="refit_every"):
        BO.run_gp_ei_bo_batched(X, y, query_batch_size=1, refit_every=3, marginalize=4, **kw)
    with pytest.raises(ValueError, match="refit_every"):
        BO.run_gp_ei_bo_batched(X, y, query_batch_size=1, refit_every=0, **kw)


# ---- the twin
def _liar_twin():
    cpu_twin, _ = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_liar_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_liar_pool"]
    assert tw.adkf_liar_pool_scratch_bytes(4, 8, 3, 8) == 0
    return fn


def liar_call(fn, b, phi, flags, X, best, q, lie=None, labels=None, excl=None, want_trace=True, rc_only=False):
    """The twin's adkf_liar_pool on host arrays: (sel_idx, sel_val, sel_mean, sel_var, sel_lie, inc, trace)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    trace = np.full((T, q, rows), np.nan, np.float32) if want_trace else None
    info = np.empty(T, np.int32)
    sel_idx = np.full((T, q), -7, np.int64)
    sel_val, sel_mean, sel_var, sel_lie = (np.full((T, q), np.nan, np.float32) for _ in range(4))
    inc = np.full((T, q + 1), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    stride = rows if labels is not None and labels.ndim == 2 else 0
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(best), pp(lie), pp(labels), stride, pp(e_idx), pp(e_off), q, pp(trace), pp(sel_idx),
            pp(sel_val), pp(sel_mean), pp(sel_var), pp(sel_lie), pp(inc), pp(info), None, 0, None, 0, None)
    if rc_only:
        return rc
    assert rc == 0 and (info == 0).all()
    return sel_idx, sel_val, sel_mean, sel_var, sel_lie, inc, trace


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _labels_of(X, seed):
    g = np.random.default_rng(seed)
    return np.ascontiguousarray(np.sin(X[:, :4].sum(1)) + 0.1 * g.standard_normal(X.shape[0]), np.float32)


def _check(out, b, Zs, ys, n_s, X, phi, kind, ard, best, flags, lie, labels, tag):
    worst = l1 = 0.0
    for t in range(b.T):
        n = n_s[t]
        task = R.isotropic(Zs[t, :n], ys[t, :n], X, phi[t], ard)
        lab = None if labels is None else (labels[t] if labels.ndim == 2 else labels)
        w, l = R.check_task(task, kind, best[t], flags, tuple(o[t] for o in out[:6]) + (out[6][t],), lie=None if lie is None else lie[t],
                            labels=lab, tag=(tag, t))
        worst, l1 = max(worst, w), max(l1, l)
    print(f"{tag}: worst error / bound {worst:.2e}, largest os * ||beta||_1 {l1:.2f}")
    return worst


@pytest.mark.parametrize("flags", [0, MAXIMIZE, LOG_EI, LOG_EI | MAXIMIZE])
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_twin_against_the_reference(kind, ard, flags):
    fn = _liar_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(kind, ard, 60 + kind, rows=70)
    q = 6
    lie = np.array([ys[t, :n_s[t]].max() if flags & MAXIMIZE else ys[t, :n_s[t]].min() for t in range(b.T)], np.float32)
    shared = _labels_of(X, 3)
    per_task = np.ascontiguousarray(np.stack([shared, -shared, 0.5 * shared]))
    holes = shared.copy()
    holes[::2] = np.nan
    nolie = np.array([lie[0], np.nan, lie[2]], np.float32)
    for name, lv, lab in (("lie", lie, None), ("shared", None, shared), ("per task", None, per_task), ("holes, lie", lie, holes),
                          ("holes, lie of NaN", nolie, holes)):
        out = liar_call(fn, b, phi, flags, X, best, q, lie=lv, labels=lab)
        assert (out[0] >= 0).all() and all(len(set(out[0][t].tolist())) == q for t in range(b.T))
        worst = _check(out, b, Zs, ys, n_s, X, phi, kind, ard, best, flags, lv, lab, (kind, ard, flags, name))
        assert worst <= 1e-3, "the twin works in float64: far inside a float32 bound"
        if name == "holes, lie of NaN":   # every rule was exercised: a label, the lie, and task 1's own mean
            picked = out[0]
            assert np.isfinite(holes[picked]).any() and np.isnan(holes[picked[0]]).any() and np.isnan(holes[picked[1]]).any()
            t1 = np.isnan(holes[picked[1]])
            assert np.array_equal(_bits(out[4][1][t1]), _bits(out[2][1][t1]))


def test_a_lie_of_nan_is_the_believer():
    fn, bv = _liar_twin(), _bv_twin()
    for kind, ard, flags in ((0, False, 0), (1, False, LOG_EI), (1, False, MAXIMIZE)):
        b, Zs, ys, n_s, X, phi, best = _problem(kind, ard, 60 + kind, rows=70)
        out = liar_call(fn, b, phi, flags, X, best, 8, lie=np.full(b.T, np.nan, np.float32))
        ref = bv_call(bv, b, phi, flags, X, best, 8)
        assert np.array_equal(out[0], ref[0])
        for a, c in zip(out[1:4] + (out[6],), ref[1:4] + (ref[4],)):
            assert np.array_equal(_bits(a), _bits(c))
        assert np.array_equal(_bits(out[4]), _bits(out[2]))


def test_twin_refuses_what_the_library_refuses():
    fn = _liar_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(0, False, 60, rows=20)
    lab = _labels_of(X, 1)
    assert liar_call(fn, b, phi, 0, X, best, 3, rc_only=True) == BADARG
    assert liar_call(fn, b, phi, 4, X, best, 3, lie=best, rc_only=True) == BADARG
    assert liar_call(fn, b, phi, 0, X, best, 65, lie=best, rc_only=True) == SIZE
    pp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = [np.zeros((b.T, 4), np.float32) for _ in range(2)]
    idx, info = np.zeros((b.T, 3), np.int64), np.zeros(b.T, np.int32)
    for labels, stride in ((lab, 7), (None, 20)):
        rc = fn(C.byref(b.c), pp(phi), 0, pp(X), 20, pp(best), pp(best), None if labels is None else pp(labels), stride, None, None, 3, None,
                pp(idx), pp(out[0]), None, None, None, None, pp(info), None, 0, None, 0, None)
        assert rc == BADARG


def _spread(picks, x):
    return float(np.ptp(x[picks]))


def test_cl_min_spreads_wider_than_the_believer_and_cl_max_does_not():
    """A smooth 1-D pool, maximising (the sense in which the names are usually read; minimising swaps the two roles).  CL-min: every
    pick is believed to have come out at the worst label seen, which pulls the mean down around it, so EI leaves the neighbourhood -
    it explores harder than the believer, whose mean stays.  CL-max: every pick is believed to have come out at the best label, the
    mean rises around it and the batch stays on the peak.
    Measured on this problem (201 rows on [-3, 3], lengthscale 1.04), the range of the six picks per task:
        believer 0.18 0.15 0.15      CL-min 6.00 6.00 6.00      CL-max 0.30 0.15 0.15
    CL-min is wider by the whole domain.  CL-max is NOT "no wider" at the resolution of the pool's cells: both clusters sit on the
    same peak, but where the lie lifts the mean to the incumbent the score is all variance, and that is largest a few cells from the
    pick, so CL-max's cluster is up to four cells (0.12) wider than the believer's.  The ranges are therefore compared in whole
    lengthscales, the resolution at which two picks are different places for the model."""
    from oracle import cpu_twin

    fn, bv = _liar_twin(), _bv_twin()
    g = np.random.default_rng(11)
    T, ns, rows, q = 3, 8, 201, 6
    Zs = np.sort(g.uniform(-3.0, 3.0, (T, ns, 1)), axis=1).astype(np.float32)
    ys = (np.sin(1.3 * Zs[..., 0]) + 0.3 * Zs[..., 0] + 0.02 * g.standard_normal((T, ns))).astype(np.float32)
    X = np.ascontiguousarray(np.linspace(-3.0, 3.0, rows, dtype=np.float32)[:, None])
    phi = np.tile(np.array([[-3.0, 0.5, 0.6]], np.float32), (T, 1))
    b = cpu_twin.CpuBatch(Zs, ys, np.zeros((T, 4), np.float32), 0, n_s=np.full(T, ns, np.int32))
    best = np.ascontiguousarray(ys.max(1))
    bel = bv_call(bv, b, phi, MAXIMIZE, X, best, q)[0]
    cl_min = liar_call(fn, b, phi, MAXIMIZE, X, best, q, lie=np.ascontiguousarray(ys.min(1)))[0]
    cl_max = liar_call(fn, b, phi, MAXIMIZE, X, best, q, lie=np.ascontiguousarray(ys.max(1)))[0]
    assert (bel >= 0).all() and (cl_min >= 0).all() and (cl_max >= 0).all()
    x = X[:, 0]
    s_bel, s_min, s_max = (np.array([_spread(p[t], x) for t in range(T)]) for p in (bel, cl_min, cl_max))
    print("spread of the picks, believer / CL-min / CL-max:", s_bel, s_min, s_max)
    ls = float(np.logaddexp(0.0, phi[0, 2]))
    assert (s_min > s_bel).all() and (np.floor(s_min / ls) > np.floor(s_bel / ls)).all()
    assert (np.floor(s_max / ls) <= np.floor(s_bel / ls)).all()


def test_a_pool_smaller_than_the_batch_and_an_empty_task():
    fn = _liar_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(0, False, 41, rows=70)
    lab = _labels_of(X, 2)
    si, sv, sm, sr, sl, inc, _ = liar_call(fn, b, phi, 0, X[:9], best, 16, labels=lab[:9])
    for t in range(b.T):
        assert sorted(si[t, :9].tolist()) == list(range(9)) and (si[t, 9:] == -1).all()
        assert np.isneginf(sv[t, 9:]).all() and (sm[t, 9:] == 0).all() and (sr[t, 9:] == 0).all() and (sl[t, 9:] == 0).all()
        assert np.array_equal(_bits(sl[t, :9]), _bits(lab[si[t, :9]]))
        assert (inc[t, 9:] == min(best[t], lab[:9].min())).all() and inc[t, 0] == best[t] and (np.diff(inc[t]) <= 0).all()
    si, sv, sm, sr, sl, inc, _ = liar_call(fn, b, phi, 0, X[:0], best, 3, lie=best)
    assert (si == -1).all() and np.isneginf(sv).all() and (sl == 0).all() and (inc == best[:, None]).all()
    full = liar_call(fn, b, phi, 0, X, best, 4, labels=lab)
    b.n_s[1] = 0
    si, sv, sm, sr, sl, inc, trace = liar_call(fn, b, phi, 0, X, best, 4, labels=lab)
    assert (si[1] == -1).all() and np.isneginf(sv[1]).all() and (trace[1] == 0).all() and (sl[1] == 0).all() and (inc[1] == best[1]).all()
    for t in (0, 2):
        assert np.array_equal(si[t], full[0][t]) and np.array_equal(_bits(trace[t]), _bits(full[6][t]))
