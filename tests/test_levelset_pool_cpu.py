"""CPU: adkf_levelset_pool without a GPU - the entry is exported, clean refusal with no device, every argument check before any launch,
gp_ops.levelset_pool's argument handling, the CPU twin against the float64 reference of levelset_ref.py (both kernels, isotropic and
ARD, both senses, all three scores, with an exclusion list), the exact properties of the entry on the twin, bit for bit, and what the
batch means on a smooth 1-d pool: the top-8 of the straddle are neighbours, the 8 picks are not, and they settle rows."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import believer_ref as B
import levelset_ref as R
from adkf_ift_amd import _lib
from test_believer_pool_ard_cpu import ard_posterior
from test_predict_pool_cpu import _call as pool_call, _problem, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE, SCORE_MEAN, LOG_EI = 1, 2, 4, 16
NAMES = ("straddle", "prob", "bound")


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, q=4, ard=False, flags=0, score=0, x=True, tau=True, beta=True, sel=(True, True), extra=True,
               trace=False, cls=False, counts=True, hits=True, excl=(False, False), info=True, ws=True, ws_short=0, scratch_short=0,
               scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    small = min(max(rows, 1), 64)   # (a refused call never looks at its buffers: a huge `rows` needs no huge pool)
    X = torch.zeros(small, d) if x else None
    qq = min(max(q, 1), 64)
    tau_t, beta_t = torch.zeros(T), torch.ones(T)
    tr, cl = torch.zeros(T * qq * small), torch.zeros(T * small, dtype=torch.int8)
    cn, hi = torch.zeros(T * qq * 3, dtype=torch.int64), torch.zeros(T * qq)
    inf = torch.zeros(T, dtype=torch.int32)
    sel_idx, out = torch.zeros(T * qq, dtype=torch.int64), [torch.zeros(T * qq) for _ in range(3)]
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_levelset_pool_scratch_bytes(T, ns, d, qq)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_levelset_pool(C.byref(b), p(phi), flags, p(X), rows, p(tau_t) if tau else None, p(beta_t) if beta else None, score,
                                  p(e_idx) if excl[0] else None, p(e_off) if excl[1] else None, q, p(tr) if trace else None,
                                  p(cl) if cls else None, p(cn) if counts else None, p(hi) if hits else None,
                                  p(sel_idx) if sel[0] else None, p(out[0]) if sel[1] else None, p(out[1]) if extra else None,
                                  p(out[2]) if extra else None, p(inf) if info else None, p(wsb) if ws else None, nb - ws_short,
                                  C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_the_entry_is_exported(lib):
    assert "adkf_levelset_pool" in _lib.SIGNATURES and "adkf_levelset_pool_scratch_bytes" in _lib.SIGNATURES
    fn = lib.adkf_levelset_pool   # a library without the entry point fails here
    assert fn.restype is C.c_int and len(fn.argtypes) == 25
    assert (_lib.LS_STRADDLE, _lib.LS_PROB, _lib.LS_BOUND) == (0, 1, 2)


def test_the_scratch_is_the_believers_plus_four_accumulators_per_task(lib):
    for T, ns, d, q in ((3, 16, 8, 4), (1, 200, 5, 64), (300, 8, 4, 8), (5000, 128, 256, 8)):
        bv = lib.adkf_believer_pool_scratch_bytes(T, ns, d, q)
        ls = lib.adkf_levelset_pool_scratch_bytes(T, ns, d, q)
        assert bv > 0 and 32 * T <= ls - bv < 32 * T + 256, (T, ns, d, q, bv, ls)   # (the arena aligns each part)
    for shape in ((0, 16, 8, 4), (3, 0, 8, 4), (3, 16, 0, 4), (3, 16, 8, 0), (3, 16, 8, 65)):
        assert lib.adkf_levelset_pool_scratch_bytes(*shape) == 0, shape


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, rows=0, x=False, extra=False, counts=False, hits=False) == LAUNCH
    assert _host_call(lib, ard=True, d=12, rows=7, q=3, score=1) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, q=64, score=2, trace=True, cls=True, excl=(True, True), flags=MAXIMIZE) == LAUNCH
    assert _host_call(lib, rows=(1 << 31) + 1, counts=False, hits=False) == LAUNCH   # more rows than the sums allow, but nobody asks for them


@pytest.mark.parametrize("ard", [False, True])
def test_bad_arguments_are_rejected_before_any_launch(lib, ard):
    call = lambda **kw: _host_call(lib, ard=ard, **kw)
    assert call(nq=4) == BADARG                                     # a batch with a query set
    for bit in (LATENT, SCORE_MEAN, 8, LOG_EI, 32, 64):
        assert call(flags=bit) == BADARG                            # flag bits other than MAXIMIZE (LATENT among them)
        assert call(flags=bit | MAXIMIZE) == BADARG
    for score in (-1, 3, 7):
        assert call(score=score) == BADARG
    assert call(rows=-1) == BADARG
    assert call(x=False) == BADARG                                  # rows > 0 without X
    assert call(tau=False) == BADARG
    assert call(beta=False) == BADARG
    assert call(sel=(False, True)) == BADARG
    assert call(sel=(True, False)) == BADARG
    assert call(info=False) == BADARG
    assert call(ws=False) == BADARG
    assert call(excl=(True, False)) == BADARG                       # excl_idx without excl_off
    for q in (0, -3):
        assert call(q=q) == BADARG
    assert call(q=65) == SIZE
    assert call(rows=(1 << 31) + 1) == SIZE                         # rows > 2^31 with counts or hits
    assert call(rows=(1 << 31) + 1, counts=False) == SIZE
    assert call(rows=(1 << 31) + 1, hits=False) == SIZE
    assert call(ws_short=1) == WORKSPACE
    assert call(scratch_short=1) == WORKSPACE
    assert call(scratch_off=4) == BADARG                            # a misaligned scratch


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False, T=3, d=5, device=torch.device("cpu"))
    for q in (0, -1, 65):
        with pytest.raises(ValueError, match="q must be"):
            gp_ops.levelset_pool(iso, None, None, tau=0.0, q=q)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.levelset_pool(types.SimpleNamespace(nq=3, ard=False, T=3, d=5), None, None, tau=0.0, q=4)
    with pytest.raises(ValueError, match="score must be"):
        gp_ops.levelset_pool(iso, None, None, tau=0.0, q=4, score="ucb")
    for bad in (torch.zeros(2), [0.0, 1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="tau must be"):
            gp_ops.levelset_pool(iso, None, None, tau=bad, q=4)
        with pytest.raises(ValueError, match="beta must be"):
            gp_ops.levelset_pool(iso, None, None, tau=0.0, beta=bad, q=4)
    assert gp_ops._per_task(iso, 1.5, "tau").tolist() == [1.5] * 3
    assert gp_ops._per_task(iso, torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), "tau").dtype == torch.float32


# ---- the twin
def _ls_twin():
    cpu_twin, _ = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_levelset_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_levelset_pool"]
    assert tw.adkf_levelset_pool_scratch_bytes(3, 16, 8, 4) == 0
    return fn


def ls_call(fn, b, phi, flags, X, tau, beta, score, q, excl=None, want_trace=True, want_cls=True, want_counts=True, ok_info=True):
    """The twin's adkf_levelset_pool on host arrays: a dict as gp_ops.levelset_pool returns it."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    tau = np.ascontiguousarray(np.broadcast_to(np.asarray(tau, np.float32), (T,)))
    beta = np.ascontiguousarray(np.broadcast_to(np.asarray(beta, np.float32), (T,)))
    trace = np.full((T, q, rows), np.nan, np.float32) if want_trace else None
    cls = np.full((T, rows), 77, np.int8) if want_cls else None
    counts = np.full((T, q, 3), -7, np.int64) if want_counts else None
    hits = np.full((T, q), np.nan, np.float32) if want_counts else None
    info = np.empty(T, np.int32)
    sel_idx = np.full((T, q), -7, np.int64)
    sel_val, sel_mean, sel_var = (np.full((T, q), np.nan, np.float32) for _ in range(3))
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(tau), pp(beta), score, pp(e_idx), pp(e_off), q, pp(trace), pp(cls), pp(counts),
            pp(hits), pp(sel_idx), pp(sel_val), pp(sel_mean), pp(sel_var), pp(info), None, 0, None, 0, None)
    assert rc == 0 and (not ok_info or (info == 0).all())
    return dict(sel_idx=sel_idx, sel_val=sel_val, sel_mean=sel_mean, sel_var=sel_var, counts=counts, hits=hits, cls=cls, trace=trace, info=info)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, c):
    return all(np.array_equal(_bits(a[k]) if a[k].dtype == np.float32 else a[k], _bits(c[k]) if c[k].dtype == np.float32 else c[k])
               for k in a if a[k] is not None and k != "info")


def seeded_problem(kind, ard, seed, rows=96):
    """test_predict_pool_cpu._problem with a pool that has decided rows: the first 29 rows are the three tasks' support rows, the next
    29 those rows plus 0.15 N(0, I).  (A random pool alone is far from every support set and leaves everything undecided.)"""
    b, Zs, ys, n_s, X, phi, best = _problem(kind, ard, seed, rows=rows)
    sup = np.concatenate([Zs[t, :n_s[t]].numpy() for t in range(b.T)]).astype(np.float32)
    assert sup.shape[0] == 29
    X[:29] = sup
    X[29:58] = sup + 0.15 * np.random.default_rng(3).standard_normal(sup.shape).astype(np.float32)
    return b, Zs, ys, n_s, X, phi


def posteriors(b, Zs, ys, n_s, X, phi, kind, ard):
    return [(ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], X, phi[t], kind) if ard else
             B.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], kind)) for t in range(b.T)]


EXCL = [[5, 6, 17, 30], [], [0, 1, 2, 40, 41, 90]]


def excl_lists(lists):
    return (np.array([i for l in lists for i in l], np.int64), np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64))


def test_the_reference_itself():
    """The three pieces in float32 against float64 on every range, the limits, and the straddle's meaning: positive exactly when the band
    holds tau."""
    z = np.concatenate([np.linspace(-60, 8, 2001), [-1.0, 0.0, -16.0]])
    y = R.prob_yardstick(z)
    print("numpy-float32 log Phi, worst error per range in units of eps32 (1 + z^2):", y.tolist())
    assert (y > 0).all() and (y < 8).all()
    with np.errstate(all="ignore"):
        lim = R.log_cdf_f32(np.array([np.inf, -np.inf, np.nan, -1e4], np.float32))
    assert lim[0] == 0 and np.isneginf(lim[1]) and np.isnan(lim[2]) and np.isfinite(lim[3])
    m, v = np.array([0.0, 1.0, 1.0, -2.0]), np.array([1.0, 0.25, 4.0, 1.0])
    score, straddle, cls, zz, sg = R.rows_ref(m, v, 0.5, 1.0, R.STRADDLE, True)
    assert np.array_equal(straddle > 0, (m - sg < 0.5) & (0.5 < m + sg))
    assert cls.tolist() == [2, 0, 2, 1]   # (row 1: the band's edge is on tau, not around it)
    assert R.rows_ref(m, v, 0.5, 0.5, R.STRADDLE, True)[2].tolist() == [1, 0, 2, 1]
    assert R.rows_ref(m, v, 0.5, 0.5, R.STRADDLE, False)[2].tolist() == [0, 1, 2, 0]
    assert np.array_equal(R.straddle_f32(m, v, 0.5, 1.0), straddle.astype(np.float32))


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_twin_against_the_reference(kind, ard, maximize):
    fn = _ls_twin()
    b, Zs, ys, n_s, X, phi = seeded_problem(kind, ard, 70 + kind + 2 * ard)
    posts = posteriors(b, Zs, ys, n_s, X, phi, kind, ard)
    q, beta = 8, 0.5
    tau = np.array([np.median(p[0]) for p in posts], np.float32)
    flags = MAXIMIZE if maximize else 0
    excl = excl_lists(EXCL)
    tally = R.new_tally()
    for score in (R.STRADDLE, R.PROB, R.BOUND):
        out = ls_call(fn, b, phi, flags, X, tau, beta, score, q, excl=excl)
        for t in range(b.T):
            worst = R.check_task(posts[t], tau[t], beta, score, maximize, out["sel_idx"][t], out["sel_val"][t], out["sel_mean"][t], out["sel_var"][t],
                                 out["trace"][t], counts=out["counts"][t], hits=out["hits"][t], excluded=EXCL[t], tally=tally, tag=(kind, ard, score, t))
            print(f"kind {kind} ard {ard} {NAMES[score]} task {t}: picks {out['sel_idx'][t].tolist()}, counts {out['counts'][t, 0].tolist()} -> "
                  f"{out['counts'][t, -1].tolist()}, hits {out['hits'][t, 0]:.3f}, worst trace error / bound {worst:.2e}")
            assert len(set(out["sel_idx"][t].tolist())) == q and (out["sel_idx"][t] >= 0).all()
            assert (out["counts"][t, 0] > 0).all(), "every class is populated at step 0"
            assert np.array_equal(np.bincount(out["cls"][t], minlength=3), out["counts"][t, 0])
    print("band rows / rows compared:", tally)
    R.assert_tally(tally)


@pytest.mark.parametrize("ard", [False, True])
def test_exact_properties_on_the_twin(ard):
    cpu_twin, pp_fn = _twin()
    fn = _ls_twin()
    kind = 1
    b, Zs, ys, n_s, X, phi = seeded_problem(kind, ard, 81 + ard)
    posts = posteriors(b, Zs, ys, n_s, X, phi, kind, ard)
    tau = np.array([np.median(p[0]) for p in posts], np.float32)
    q, beta = 8, 0.5
    excl = excl_lists(EXCL)
    rows = X.shape[0]
    for flags in (0, MAXIMIZE):
        outs = [ls_call(fn, b, phi, flags, X, tau, beta, s, q, excl=excl) for s in range(3)]
        for s, out in enumerate(outs):
            # step 0 of a q = 8 call is the q = 1 call
            one = ls_call(fn, b, phi, flags, X, tau, beta, s, 1, excl=excl)
            for k in ("sel_val", "sel_mean", "sel_var", "hits", "trace"):
                assert np.array_equal(_bits(one[k][:, 0]), _bits(out[k][:, 0])), (s, k)
            assert np.array_equal(one["sel_idx"][:, 0], out["sel_idx"][:, 0]) and np.array_equal(one["counts"][:, 0], out["counts"][:, 0])
            assert np.array_equal(one["cls"], out["cls"])
            # step-0 counts, hits and cls do not depend on the score
            assert np.array_equal(out["counts"][:, 0], outs[0]["counts"][:, 0]) and np.array_equal(out["cls"], outs[0]["cls"])
            assert np.array_equal(_bits(out["hits"][:, 0]), _bits(outs[0]["hits"][:, 0]))
            assert (out["counts"].sum(-1) == rows).all()
            # the undecided count never rises; STRADDLE and BOUND traces never rise
            assert (np.diff(out["counts"][..., 2], axis=1) <= 0).all(), s
            if s != R.PROB:
                assert (np.diff(out["trace"], axis=1) <= 0).all(), s
            # outputs that were not asked for change nothing
            bare = ls_call(fn, b, phi, flags, X, tau, beta, s, q, excl=excl, want_trace=False, want_cls=False, want_counts=False)
            assert bare["trace"] is None and bare["counts"] is None and np.array_equal(bare["sel_idx"], out["sel_idx"])
            assert np.array_equal(_bits(bare["sel_val"]), _bits(out["sel_val"]))
        # the class is decided from the value a STRADDLE call stores
        assert np.array_equal(outs[0]["counts"][..., 2], (outs[0]["trace"] > 0).sum(-1))
        assert np.array_equal(outs[0]["cls"] == 2, outs[0]["trace"][:, 0] > 0)
        # score = bound with beta = 0 is the ranking by the mean
        flat = ls_call(fn, b, phi, flags, X, tau, 0.0, R.BOUND, q, excl=excl)
        best = np.zeros(b.T, np.float32)
        _, _, _, top_idx, top_val = pool_call(pp_fn, b, phi, flags | SCORE_MEAN | LATENT, X, best, k=q, excl=excl, per_row=False)
        assert np.array_equal(flat["sel_idx"], top_idx) and np.array_equal(flat["sel_val"], top_val)
        # a permuted pool: the same counts and hits, the picks mapped through the permutation
        perm = np.random.default_rng(11).permutation(rows)
        inv = np.argsort(perm)
        lists_p = [sorted(int(inv[i]) for i in l) for l in EXCL]
        for s in range(3):
            out_p = ls_call(fn, b, phi, flags, np.ascontiguousarray(X[perm]), tau, beta, s, q, excl=excl_lists(lists_p))
            assert np.array_equal(out_p["counts"], outs[s]["counts"]) and np.array_equal(_bits(out_p["hits"]), _bits(outs[s]["hits"])), s
            assert np.array_equal(perm[out_p["sel_idx"]], outs[s]["sel_idx"]), s
            assert np.array_equal(_bits(out_p["trace"]), _bits(outs[s]["trace"][:, :, perm])), s
        # a task alone is the task in the batch
        for t in range(b.T):
            n = int(n_s[t])
            solo = cpu_twin.CpuBatch(Zs[t:t + 1, :n].numpy(), ys[t:t + 1, :n].numpy(), np.zeros((1, 4), np.float32), kind)
            if ard:
                solo.c.flags = ARD
            one = ls_call(fn, solo, np.ascontiguousarray(phi[t:t + 1]), flags, X, tau[t:t + 1], beta, 0, q, excl=excl_lists([EXCL[t]]))
            assert np.array_equal(one["counts"][0], outs[0]["counts"][t]) and np.array_equal(_bits(one["hits"][0]), _bits(outs[0]["hits"][t]))
            assert np.array_equal(one["sel_idx"][0], outs[0]["sel_idx"][t]) and np.array_equal(_bits(one["trace"][0]), _bits(outs[0]["trace"][t]))


def test_refusal_by_value_a_skipped_task_and_an_empty_pool():
    fn = _ls_twin()
    b, Zs, ys, n_s, X, phi = seeded_problem(0, False, 91)
    tau, q = np.array([0.1, -0.2, 0.3], np.float32), 5
    full = ls_call(fn, b, phi, MAXIMIZE, X, tau, 0.5, 0, q)

    def dead(out, t, nan_trace):
        assert (out["sel_idx"][t] == -1).all() and np.isneginf(out["sel_val"][t]).all()
        assert (out["sel_mean"][t] == 0).all() and (out["sel_var"][t] == 0).all()
        assert (out["counts"][t] == 0).all() and (out["hits"][t] == 0).all() and (out["cls"][t] == -1).all()
        assert np.isnan(out["trace"][t]).all() if nan_trace else (out["trace"][t] == 0).all()

    def others(out, ts):
        for t in ts:
            assert np.array_equal(out["sel_idx"][t], full["sel_idx"][t]) and np.array_equal(_bits(out["trace"][t]), _bits(full["trace"][t]))
            assert np.array_equal(out["counts"][t], full["counts"][t]) and np.array_equal(_bits(out["hits"][t]), _bits(full["hits"][t]))

    for bad in (np.nan, np.inf, -np.inf):
        t2 = tau.copy(); t2[1] = bad
        for s in range(3):
            dead(ls_call(fn, b, phi, MAXIMIZE, X, t2, 0.5, s, q), 1, True)
        others(ls_call(fn, b, phi, MAXIMIZE, X, t2, 0.5, 0, q), (0, 2))
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        out = ls_call(fn, b, phi, MAXIMIZE, X, tau, np.array([0.5, 0.5, bad], np.float32), 0, q)
        dead(out, 2, True)
        others(out, (0, 1))
    # an empty pool: the tail only, zero counts
    out = ls_call(fn, b, phi, 0, X[:0], tau, 0.5, 0, 3)
    assert (out["sel_idx"] == -1).all() and np.isneginf(out["sel_val"]).all() and (out["counts"] == 0).all() and (out["hits"] == 0).all()
    # a pool of 9 rows with q = 16: nine picks, then the tail; the counts go on covering all 9 rows
    out = ls_call(fn, b, phi, 0, X[:9], tau, 0.5, 2, 16)
    for t in range(b.T):
        assert sorted(out["sel_idx"][t, :9].tolist()) == list(range(9)) and (out["sel_idx"][t, 9:] == -1).all()
        assert (out["counts"][t].sum(-1) == 9).all() and np.array_equal(out["counts"][t, 9], out["counts"][t, 15])
    # a task with n_s == 0 is skipped; the others are what they are without it
    b.n_s[1] = 0
    out = ls_call(fn, b, phi, MAXIMIZE, X, tau, 0.5, 0, q)
    dead(out, 1, False)
    others(out, (0, 2))


def test_the_batch_settles_rows_and_is_not_a_set_of_neighbours():
    """What the entry is for.  A sine through 12 support points, 200 sorted rows, tau at a level it crosses: the top-8 of the straddle at
    step 0 are mutual neighbours; the 8 picks of a q = 8 call are not, and after them strictly fewer rows are undecided."""
    from oracle import cpu_twin

    fn = _ls_twin()
    g = np.random.default_rng(3)
    rows, ns, q = 200, 12, 8
    X = np.linspace(0.0, 1.0, rows, dtype=np.float32)[:, None]
    Zs = np.sort(g.uniform(0.0, 1.0, (1, ns, 1)).astype(np.float32), axis=1)
    ys = np.sin(6.0 * Zs[..., 0]).astype(np.float32)
    phi = np.array([[-3.0, 0.5, -1.5]], np.float32)        # a lengthscale of ~0.2: neighbouring rows are almost one observation
    b = cpu_twin.CpuBatch(Zs, ys, np.zeros((1, 4), np.float32), 0)
    out = ls_call(fn, b, phi, MAXIMIZE, X, -0.1, 1.96, R.STRADDLE, q + 1)   # sin(6 x) crosses -0.1 once on [0, 1], near row 108
    top = np.argsort(-out["trace"][0, 0], kind="stable")[:q]
    picks = out["sel_idx"][0, :q]
    print(f"top-{q} of the straddle {sorted(top.tolist())}, the batch {picks.tolist()}, undecided {out['counts'][0, :, 2].tolist()}")
    assert picks[0] == top[0]
    assert top.max() - top.min() == q - 1, "the top-q are a run of neighbouring rows"
    # the picks are not: one pick spends the variance of its whole neighbourhood - here an end of the pool, where the band is widest -
    # and the batch moves on to the other end and to the crossing, which keeps attracting picks (|m - tau| ~ 0 there, and the noise
    # keeps sigma off 0)
    assert picks.max() - picks.min() > q - 1 and len(set(picks.tolist()) & set(top.tolist())) == 1
    assert min(picks) < 20 and max(picks) > 180 and min(abs(int(p) - 108) for p in picks) <= 4
    assert out["counts"][0, q, 2] < out["counts"][0, 0, 2]
    assert (np.diff(out["counts"][0, :, 2]) <= 0).all()
