"""CPU: adkf_mix_pool without a GPU - the reference of mix_ref.py against Monte Carlo and its own identities; the entry is exported,
refuses cleanly with no device and checks every argument before any launch; gp_ops.mix_pool's, gp_ops.replicate_batch's and the BO
loop's argument handling; the CPU twin against the reference (isotropic and ARD, RBF and Matern, M = 1, 3, 5 and 64, padding, a zero
weight, unequal weights) and the semantics of the call on the twin; the Laplace sampler; and that the bounds of the GPU test are
informative on the GPU test's problems."""
import ctypes as C
import glob
import os
import types

import numpy as np
import pytest
import torch

import mix_ref as R
from adkf_ift_amd import _lib
from test_predict_pool_cpu import _problem, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE, SCORE_MEAN, LOG, BALD = R.LATENT, R.MAXIMIZE, R.SCORE_MEAN, R.LOG_EI, R.SCORE_BALD
EPS32 = R.EPS32
CHUNK = _lib.MIX_CHUNK_ROWS
KIND_FLAGS = {"ei": 0, "log_ei": LOG, "smean": SCORE_MEAN, "bald": BALD}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- the reference checks itself
def test_the_reference_against_monte_carlo_and_its_identities():
    g = np.random.default_rng(3)
    compared = 0
    for n in (1, 2, 5):
        for _ in range(3):
            m, v = g.normal(size=(n, 1)), g.uniform(0.05, 1.0, (n, 1))
            wt = g.uniform(0.2, 1.0, n)
            wt /= wt.sum()
            out = R.mix(m, v, None, wt)
            mu, se_mu, s2, se_s2 = R.by_monte_carlo(m[:, 0], v[:, 0], wt, seed=compared)
            assert abs(out["mean"][0] - mu) <= 4.5 * se_mu and abs(out["var"][0] - s2) <= 4.5 * se_s2, (n, out["mean"][0], mu, out["var"][0], s2)
            compared += 1
    assert compared == 9
    # BALD is a Jensen gap: never negative in float64, 0 for one member and for equal members
    rows = 300
    m, v = g.normal(size=(6, rows)), g.uniform(1e-3, 2.0, (6, rows))
    wt = g.uniform(0.1, 1.0, 6)
    wt /= wt.sum()
    assert (R.mix(m, v, None, wt)["bald"] >= 0).all() and R.mix(m, v, None, wt)["bald"].max() > 0.1
    assert (R.mix(m[:1], v[:1], None, [1.0])["bald"] == 0).all()
    assert np.abs(R.mix(np.repeat(m[:1], 3, 0), np.repeat(v[:1], 3, 0), None, [0.25, 0.5, 0.25])["bald"]).max() <= 1e-15
    # the log score is the log of the linear one where both exist, and finite where the linear one has underflowed
    le = g.uniform(-30.0, 1.0, (6, rows))
    lin, lg = R.mix(m, v, np.exp(le), wt)["ei"], R.mix(m, v, le, wt, log=True)["log_ei"]
    assert np.abs(lg - np.log(lin)).max() <= 1e-12
    far = R.mix(m, v, le - 800.0, wt, log=True)["log_ei"]
    assert (R.mix(m, v, np.exp(le - 800.0), wt)["ei"] == 0).all() and np.isfinite(far).all() and np.abs(far - (lg - 800.0)).max() <= 1e-9
    le[2] = -np.inf                       # a -inf member is skipped, all -inf gives -inf
    assert np.isfinite(R.mix(m, v, le, wt, log=True)["log_ei"]).all()
    assert np.isneginf(R.mix(m, v, np.full_like(le, -np.inf), wt, log=True)["log_ei"]).all()
    # the weights as the library normalises them
    ts, w = R.weights_of([4, -1, 2, 7], [1.0, np.nan, 0.0, 3.0])
    assert ts.tolist() == [4, 7] and w.tolist() == [0.25, 0.75]
    assert R.weights_of([4, 2], [1.0, -1.0]) is None and R.weights_of([-1, -1]) is None and R.weights_of([1, 2], [0.0, 0.0]) is None


# ---- the entry of the device library
def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, G=2, M=3, k=3, ard=False, flags=0, x=True, mem=True, w=True, best=True,
               outs=(True, True, True), top=(True, True), excl=(False, False), info=True, ws=True, ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    Gm, Mm, kk = max(G, 1), min(max(M, 1), 64), min(max(k, 0), 64)
    mem_t, w_t, bf = torch.zeros(Gm, Mm, dtype=torch.int32), torch.ones(Gm, Mm), torch.zeros(T)
    out = [torch.zeros(Gm * max(rows, 1)) for _ in range(3)]
    inf = torch.zeros(T, dtype=torch.int32)
    top_idx, top_val = torch.zeros(Gm * max(kk, 1), dtype=torch.int64), torch.zeros(Gm * max(kk, 1))
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(Gm + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_mix_pool_scratch_bytes(T, Gm, kk)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_mix_pool(C.byref(b), p(phi), flags, p(X), rows, G, p(mem_t) if mem else None, p(w_t) if w else None, M,
                             p(bf) if best else None, p(e_idx) if excl[0] else None, p(e_off) if excl[1] else None,
                             p(out[0]) if outs[0] else None, p(out[1]) if outs[1] else None, p(out[2]) if outs[2] else None, k,
                             p(top_idx) if top[0] else None, p(top_val) if top[1] else None, p(inf) if info else None,
                             p(wsb) if ws else None, nb - ws_short, C.c_void_p(scratch.data_ptr() + scratch_off), sb - scratch_short, None)


def test_the_entry_is_exported(lib):
    assert "adkf_mix_pool" in _lib.SIGNATURES and "adkf_mix_pool_scratch_bytes" in _lib.SIGNATURES
    fn = lib.adkf_mix_pool   # a library without the entry point fails here
    assert fn.restype is C.c_int and len(fn.argtypes) == 24
    assert _lib.PM_SCORE_BALD == 32 and _lib.MIX_MEMBERS_MAX == 64 and CHUNK % 64 == 0 and CHUNK > 0


def test_the_scratch_size(lib):
    f = lib.adkf_mix_pool_scratch_bytes
    assert len(f.argtypes) == 3   # T, G, k: rows, ns, d and M are no arguments
    base = f(3, 2, 0)
    assert base >= 3 * 3 * CHUNK * 4 and base % 8 == 0           # three planes of one chunk
    assert f(4, 2, 0) - base >= 3 * CHUNK * 4
    assert all(f(T + 1, 2, 5) > f(T, 2, 5) for T in range(1, 40))
    assert all(f(3, G + 1, 5) >= f(3, G, 5) for G in range(1, 300)) and f(3, 300, 5) > f(3, 1, 5) and f(3, 10000, 5) > f(3, 4096, 5)
    assert all(f(3, 7, k + 1) > f(3, 7, k) for k in range(0, 64))
    assert all(f(T, G, k) % 8 == 0 for T in (1, 5) for G in (1, 3, 5000) for k in (0, 1, 7, 64))
    for bad in ((0, 2, 0), (-1, 2, 0), (3, 0, 0), (3, -2, 4), (3, 2, -1), (3, 2, 65)):
        assert f(*bad) == 0, bad


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0, x=False) == LAUNCH
    assert _host_call(lib, ard=True, d=12, rows=7, k=0, flags=LOG, w=False) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, G=600, M=64, k=64, excl=(True, True), flags=BALD | LATENT, best=False) == LAUNCH
    assert _host_call(lib, k=0, outs=(True, False, False), best=False) == LAUNCH           # the mean alone reads no best_f
    assert _host_call(lib, k=2, outs=(False, False, False), flags=SCORE_MEAN | MAXIMIZE, best=False) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    for G in (0, -3):
        assert _host_call(lib, G=G) == BADARG
    for M in (0, -1):
        assert _host_call(lib, M=M) == BADARG
    assert _host_call(lib, M=65) == SIZE
    assert _host_call(lib, k=65) == SIZE
    assert _host_call(lib, mem=False) == BADARG
    assert _host_call(lib, k=-1) == BADARG
    for bit in (8, 64, 128, 1 << 20):
        assert _host_call(lib, flags=bit) == BADARG                            # a flag bit outside the five
        assert _host_call(lib, flags=bit | LATENT | MAXIMIZE) == BADARG
    assert _host_call(lib, flags=SCORE_MEAN | BALD) == BADARG
    assert _host_call(lib, flags=LOG | SCORE_MEAN) == BADARG
    assert _host_call(lib, flags=LOG | BALD) == BADARG
    for flags in (0, LOG, MAXIMIZE):
        assert _host_call(lib, flags=flags, best=False) == BADARG              # the EI score read (score and k) without best_f
        assert _host_call(lib, flags=flags, best=False, k=0) == BADARG         # ... by score alone
        assert _host_call(lib, flags=flags, best=False, outs=(True, True, False)) == BADARG   # ... by the selection alone
    assert _host_call(lib, top=(False, True)) == BADARG
    assert _host_call(lib, top=(True, False)) == BADARG
    assert _host_call(lib, k=0, outs=(False, False, False)) == BADARG          # no output at all
    assert _host_call(lib, info=False) == BADARG
    assert _host_call(lib, ws=False) == BADARG
    assert _host_call(lib, excl=(True, False)) == BADARG                       # excl_idx without excl_off
    assert _host_call(lib, scratch_off=4) == BADARG                            # a misaligned scratch
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, ard=True, ws_short=1) == WORKSPACE
    assert _host_call(lib, scratch_short=1) == WORKSPACE


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False, T=6, d=5)
    mem = [[0, 1, 2], [3, 4, -1]]
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.mix_pool(types.SimpleNamespace(nq=3, ard=False, T=6, d=5), None, None, members=mem)
    with pytest.raises(ValueError, match="score must be"):
        gp_ops.mix_pool(iso, None, None, members=mem, score="ucb")
    for k in (-1, 65):
        with pytest.raises(ValueError, match="topk must be"):
            gp_ops.mix_pool(iso, None, None, members=mem, topk=k)
    for bad in (torch.zeros(2, 3), [0, 1], torch.zeros(0, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="members must be"):
            gp_ops.mix_pool(iso, None, None, members=bad)
    for bad in (torch.zeros(2, 0, dtype=torch.int32), torch.zeros(2, 65, dtype=torch.int32)):
        with pytest.raises(ValueError, match="members M must be"):
            gp_ops.mix_pool(iso, None, None, members=bad)
    for bad in (torch.zeros(2, 2), torch.zeros(3, 3), torch.zeros(6)):
        with pytest.raises(ValueError, match="weights must be"):
            gp_ops.mix_pool(iso, None, None, members=mem, weights=bad)
    for score in ("ei", "log_ei"):
        with pytest.raises(ValueError, match="need best_f"):
            gp_ops.mix_pool(iso, None, None, members=mem, score=score)
    with pytest.raises(ValueError, match="best_f must have"):
        gp_ops.mix_pool(iso, None, None, members=mem, best_f=torch.zeros(5))
    with pytest.raises(ValueError, match="no output"):
        gp_ops.mix_pool(iso, None, None, members=mem, score="mean", want_mean=False, want_var=False, want_score=False)
    for M in (0, 65):
        with pytest.raises(ValueError, match="replicas M must be"):
            gp_ops.replicate_batch(iso, M)
    with pytest.raises(ValueError, match="isotropic batches only"):
        gp_ops.phi_laplace_samples(types.SimpleNamespace(ard=True), None, 4)
    with pytest.raises(ValueError, match="n_samples must be"):
        gp_ops.phi_laplace_samples(types.SimpleNamespace(ard=False), None, 0)


def test_the_bo_loop_checks_its_arguments():
    from adkf_ift_amd import bayes_opt as BO

    X, y = torch.randn(20, 3), torch.randn(20)
    run = lambda **kw: BO.run_gp_ei_bo_batched(X, y, 4, 2, 1, "matern", "cpu", 10, 0.01, True, rngs=[np.random.default_rng(0)], **kw)
    for M in (1, -2, 65):
        with pytest.raises(ValueError, match="marginalize must be"):
            run(marginalize=M)
    with pytest.raises(ValueError, match="batch='topk'"):
        run(marginalize=4, batch="believer")
    with pytest.raises(ValueError, match="ard=False"):
        run(marginalize=4, ard=True)


# ---- the twin
def _mix_twin():
    cpu_twin, pool = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_mix_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_mix_pool"]
    sb = tw.adkf_mix_pool_scratch_bytes
    sb.restype, sb.argtypes = _lib.SIGNATURES["adkf_mix_pool_scratch_bytes"]
    assert sb(3, 2, 5) == 0
    return cpu_twin, fn, pool


def mix_call(fn, b, phi, X, members, weights=None, best=None, flags=0, k=0, excl=None, want=(True, True, True), ok=True):
    """The twin's adkf_mix_pool on host arrays: dict(mean, var, score, top_idx, top_val, info)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    members = np.ascontiguousarray(members, np.int32)
    weights = None if weights is None else np.ascontiguousarray(weights, np.float32)
    rows, (G, M) = X.shape[0], members.shape
    mean, var, score = (np.full((G, rows), -7.0, np.float32) if w else None for w in want)
    info = np.empty(b.T, np.int32)
    top_idx = np.full((G, max(k, 1)), -7, np.int64)
    top_val = np.full((G, max(k, 1)), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, G, pp(members), pp(weights), M, pp(best), pp(e_idx), pp(e_off), pp(mean), pp(var),
            pp(score), k, pp(top_idx) if k else None, pp(top_val) if k else None, pp(info), None, 0, None, 0, None)
    assert rc == 0
    if ok:
        assert (info == 0).all()
    return dict(mean=mean, var=var, score=score, top_idx=top_idx, top_val=top_val, info=info)


def twin_members(pool, b, phi, X, best, flags):
    """adkf_predict_pool's float32 mean, var and ei [T, rows] on the twin, under the mixture call's LATENT | MAXIMIZE | LOG_EI."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    mean, var, ei = (np.full((T, rows), np.nan, np.float32) for _ in range(3))
    info = np.empty(T, np.int32)
    rc = pool(C.byref(b.c), pp(phi), flags & (LATENT | MAXIMIZE | LOG), pp(X), rows, pp(best), None, None, pp(mean), pp(var), pp(ei), 0, None, None,
              pp(info), None, 0, None, 0, None)
    assert rc == 0 and (info == 0).all()
    return mean, var, ei


def _replicated(cpu_twin, kind, ard, seed, M, rows, spread=0.3):
    """test_predict_pool_cpu's problem with every task replicated M times under phi + spread randn: (b, X, phi, best, T0)."""
    b0, Zs, ys, n_s, X, phi, best = _problem(kind, ard, seed, rows=rows)
    T0 = b0.T
    rep = lambda a: np.repeat(np.asarray(a), M, 0)
    g = np.random.default_rng(seed)
    phis = rep(phi) + (spread * g.standard_normal((T0 * M, phi.shape[1]))).astype(np.float32)
    b = cpu_twin.CpuBatch(rep(Zs.numpy()), rep(ys.numpy()), np.zeros((T0 * M, 4), np.float32), kind, n_s=rep(n_s))
    if ard:
        b.c.flags = ARD
    return b, X, np.ascontiguousarray(phis, np.float32), np.ascontiguousarray(rep(best), np.float32), T0


def ref_outputs(mvE, members, weights, g, key, maximize):
    """mix_ref.mix of group g from the members' arrays (mean, var, ei) [T, rows] each."""
    ts, wt = R.weights_of(members[g], None if weights is None else weights[g])
    return R.mix(mvE[0][ts], mvE[1][ts], mvE[2][ts] if key in ("ei", "log_ei") else None, wt, maximize=maximize, log=key == "log_ei")


@pytest.mark.parametrize("kind,ard,M", [(0, False, 1), (1, False, 3), (0, True, 5), (1, True, 3), (1, False, 64), (0, False, 5)])
def test_cpu_twin_against_the_reference(kind, ard, M):
    """The twin mixes adkf_predict_pool's float32 members in float64 and rounds once: |got - ref| <= 2 eps32 |ref| + 1e-8 on mean,
    var and all four scores, with -1 padding, a zero weight and unequal weights in the table (M >= 3)."""
    cpu_twin, fn, pool = _mix_twin()
    rows = 40
    b, X, phi, best, T0 = _replicated(cpu_twin, kind, ard, 60 + kind + 2 * ard + M, M, rows)
    members = np.arange(T0 * M, dtype=np.int32).reshape(T0, M)
    weights = None
    if M >= 3:
        weights = np.random.default_rng(M).uniform(0.2, 3.0, (T0, M)).astype(np.float32)
        members[0, 1] = -1
        weights[1, 2] = 0.0
        weights[0, 1] = np.nan            # not read: the entry is not there
    compared = 0
    for base in (0, LATENT, MAXIMIZE | LATENT):
        for key, bit in KIND_FLAGS.items():
            flags = base | bit
            mvE = twin_members(pool, b, phi, X, best, flags)
            out = mix_call(fn, b, phi, X, members, weights, best, flags)
            for g in range(T0):
                ref = ref_outputs(mvE, members, weights, g, key, bool(base & MAXIMIZE))
                for name, want in (("mean", ref["mean"]), ("var", ref["var"]), ("score", ref[key])):
                    err = np.abs(out[name][g].astype(np.float64) - want)
                    assert (err <= 2 * EPS32 * np.abs(want) + 1e-8).all(), (flags, g, name, float(err.max()))
                    compared += want.size
    assert compared == 3 * 4 * T0 * 3 * rows


def test_semantics_on_the_twin():
    cpu_twin, fn, pool = _mix_twin()
    rows, M = 70, 3
    b, X, phi, best, T0 = _replicated(cpu_twin, 1, False, 91, M, rows)
    X[10] = X[3]; X[41] = X[3]; X[69] = X[20]          # exact duplicate rows: bit-equal scores
    members = np.arange(T0 * M, dtype=np.int32).reshape(T0, M)
    members[2, 1] = 0                                   # a task shared by two groups
    weights = np.array([[1.0, 2.0, 0.5], [1.0, 1.0, 1.0], [0.3, 0.3, 2.0]], np.float32)
    base = {key: mix_call(fn, b, phi, X, members, weights, best, bit) for key, bit in KIND_FLAGS.items()}
    # exclusions per group, the order on duplicates, and score == NULL gives the same selection
    lists = [sorted({int(np.argmax(base["ei"]["score"][0])), 5, 6}), [], sorted(set(range(rows)) - {3, 10, 41, 50})]
    e_idx = np.array([i for l in lists for i in l], np.int64)
    e_off = np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64)
    for key, k in (("ei", 1), ("bald", 7), ("log_ei", 64), ("smean", 5)):
        out = mix_call(fn, b, phi, X, members, weights, best, KIND_FLAGS[key], k=k, excl=(e_idx, e_off))
        assert np.array_equal(_bits(out["score"]), _bits(base[key]["score"]))
        for g in range(3):
            idx, val = R.topk_of(out["score"][g], k, lists[g])
            assert np.array_equal(out["top_idx"][g], idx) and np.array_equal(_bits(out["top_val"][g]), _bits(val)), (key, k, g)
        if k == 64:
            got = out["top_idx"][2, :4].tolist()
            assert (out["top_idx"][2, 4:] == -1).all() and np.isneginf(out["top_val"][2, 4:]).all()
            assert got.index(3) < got.index(10) < got.index(41)
        quiet = mix_call(fn, b, phi, X, members, weights, best, KIND_FLAGS[key], k=k, excl=(e_idx, e_off), want=(False, False, False))
        assert np.array_equal(quiet["top_idx"], out["top_idx"]) and np.array_equal(_bits(quiet["top_val"]), _bits(out["top_val"]))
    # a group alone has the bits it has among three
    for g in range(3):
        alone = mix_call(fn, b, phi, X, members[g:g + 1], weights[g:g + 1], best, 0)
        for name in ("mean", "var", "score"):
            assert np.array_equal(_bits(alone[name][0]), _bits(base["ei"][name][g])), (g, name)
    # the anchors hold on the twin too: one used member, and two equal entries of one task, are prediction's bits; BALD is 0
    mvE = twin_members(pool, b, phi, X, best, 0)
    for mem, w in (([[4, -1, -1]], None), ([[4, 7, 2]], [[1.0, 0.0, 0.0]]), ([[4, 4, -1]], [[0.7, 0.7, 9.0]])):
        one = mix_call(fn, b, phi, X, mem, w, best, 0)
        t = mem[0][0]
        assert all(np.array_equal(_bits(one[n][0]), _bits(a[t])) for n, a in zip(("mean", "var", "score"), mvE)), mem
        assert (mix_call(fn, b, phi, X, mem, w, best, BALD)["score"] == 0).all()
    # each way a group can be bad: NaN everywhere and no selection, the other groups keep their bits
    def broken(mem=None, w=None):
        m2, w2 = members.copy(), weights.copy()
        if mem is not None:
            m2[mem[0]] = mem[1]
        if w is not None:
            w2[w[0]] = w[1]
        return m2, w2
    cases = [broken(mem=((1, 0), 9)), broken(mem=((1, 2), -2)), broken(w=((1, 1), -1.0)), broken(w=((1, 0), np.nan)), broken(w=((1, 2), np.inf)),
             broken(mem=((1, slice(None)), -1)), broken(w=((1, slice(None)), 0.0))]
    for i, (m2, w2) in enumerate(cases):
        out = mix_call(fn, b, phi, X, m2, w2, best, 0, k=4)
        assert all(np.isnan(out[n][1]).all() for n in ("mean", "var", "score")), i
        assert (out["top_idx"][1] == -1).all() and np.isneginf(out["top_val"][1]).all(), i
        for g in (0, 2):
            assert all(np.array_equal(_bits(out[n][g]), _bits(base["ei"][n][g])) for n in ("mean", "var", "score")), (i, g)
    # an unused entry's NaN weight is bad only if the entry is there
    m2, w2 = broken(mem=((1, 1), -1), w=((1, 1), np.nan))
    assert np.isfinite(mix_call(fn, b, phi, X, m2, w2, best, 0)["score"]).all()
    # an empty pool: nothing selected
    out = mix_call(fn, b, phi, X[:0], members, weights, best, 0, k=3)
    assert (out["top_idx"] == -1).all() and np.isneginf(out["top_val"]).all()
    # a NaN pool row is NaN in every group and never selected; its neighbours keep their bits
    Xn = X.copy()
    Xn[12, 2] = np.nan
    keep = np.arange(rows) != 12
    for key, bit in KIND_FLAGS.items():
        out = mix_call(fn, b, phi, Xn, members, weights, best, bit, k=5)
        for n in ("mean", "var", "score"):
            assert np.isnan(out[n][:, 12]).all() and np.array_equal(_bits(out[n][:, keep]), _bits(base[key][n][:, keep])), (key, n)
        assert not (out["top_idx"] == 12).any()


def test_an_empty_or_failed_member_makes_its_groups_nan_on_the_twin():
    cpu_twin, fn, pool = _mix_twin()
    rows, M = 20, 2
    b, X, phi, best, T0 = _replicated(cpu_twin, 0, False, 95, M, rows)
    members = np.arange(T0 * M, dtype=np.int32).reshape(T0, M)
    base = mix_call(fn, b, phi, X, members, None, best, 0)
    b.n_s[3] = 0                                        # task 3 is empty: group 1 uses it, groups 0 and 2 do not
    out = mix_call(fn, b, phi, X, members, None, best, 0, k=2)
    assert np.isnan(out["score"][1]).all() and np.isnan(out["mean"][1]).all() and (out["top_idx"][1] == -1).all()
    for g in (0, 2):
        assert np.array_equal(_bits(out["score"][g]), _bits(base["score"][g]))
    # with a zero weight the empty task is not used, and the group is its other member
    w = np.ones((T0, M), np.float32)
    w[1, 1] = 0.0
    out = mix_call(fn, b, phi, X, members, w, best, 0)
    assert np.isfinite(out["score"]).all()
    mvE = twin_members(pool, cpu_twin.CpuBatch(b.Z_s[2:3], b.y_s[2:3], np.zeros((1, 4), np.float32), 0, n_s=b.n_s[2:3]), phi[2:3], X, best[2:3], 0)
    assert np.array_equal(_bits(out["score"][1]), _bits(mvE[2][0]))


# ---- the Laplace sampler
def test_laplace_draws():
    from adkf_ift_amd import gp_ops

    g = torch.Generator().manual_seed(5)
    A = torch.randn(2, 3, 3, generator=g, dtype=torch.float64)
    H = A @ A.transpose(1, 2) + 0.5 * torch.eye(3, dtype=torch.float64)          # PD, eigenvalues >= 0.5
    n_s = torch.tensor([16, 64])
    S = 20000
    eps = torch.randn(2, S, 3, generator=g, dtype=torch.float64)
    off = gp_ops.laplace_draws(H, n_s, eps, max_sd=2.0)                          # n lambda >= 8 > 1 / 4: no floor
    assert off.shape == (2, S, 3) and off.dtype == torch.float64
    for t in range(2):
        want = torch.linalg.inv(n_s[t] * H[t])
        got = torch.cov(off[t].T)
        # a sample covariance entry has a standard error of about sqrt(2 / S) = 1 % of the scale
        assert (got - want).abs().max() <= 0.06 * want.abs().max(), (t, got, want)
    # an asymmetric H is symmetrised
    skew = torch.tensor([[0.0, 0.3, 0.0], [-0.3, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    assert (gp_ops.laplace_draws(H + skew, n_s, eps[:, :8]) - off[:, :8]).abs().max() <= 1e-13
    # floored directions have standard deviation max_sd: a flat direction and an indefinite one
    Q = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0]
    Hf = (Q @ torch.diag(torch.tensor([2.0, 1e-6, -3.0], dtype=torch.float64)) @ Q.T)[None]
    for max_sd in (2.0, 0.5):
        proj = gp_ops.laplace_draws(Hf, [10], eps[:1], max_sd=max_sd)[0] @ Q
        sd = proj.std(0)
        assert abs(sd[0] - (10 * 2.0) ** -0.5) <= 0.03 * sd[0] and abs(sd[1] - max_sd) <= 0.03 * max_sd and abs(sd[2] - max_sd) <= 0.03 * max_sd
    with pytest.raises(ValueError, match="H must be"):
        gp_ops.laplace_draws(torch.zeros(2, 3, 2), n_s, eps)
    with pytest.raises(ValueError, match="eps must be"):
        gp_ops.laplace_draws(H, n_s, eps[:1])
    with pytest.raises(ValueError, match="n_s must have"):
        gp_ops.laplace_draws(H, [3], eps)


def test_phi_laplace_samples_on_a_stand_in_batch(monkeypatch):
    """The sampler end to end with the CPU twin's gradient in the place of the device's: draw 0 is the MAP point, the draws repeat under
    a seeded generator and differ under another, and their spread is the Laplace covariance."""
    from adkf_ift_amd import gp_ops
    from oracle import cpu_twin as TW
    from test_cpu_twin import _batch

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "gp_N16_Nq32_d16_k0_r1_s0.npz"))
    tb, phi, n, m = _batch(g)
    monkeypatch.setattr(gp_ops, "mll_value_grad", lambda b, p: (None, torch.from_numpy(TW.mll_value_grad(tb, p.numpy(), want_dZ=False)[1])))
    stand_in = types.SimpleNamespace(ard=False, T=1, ns=n, n_s=None, device="cpu", check_phi=lambda p: p)
    p0 = torch.from_numpy(phi)
    draw = lambda seed, **kw: gp_ops.phi_laplace_samples(stand_in, p0, 16, generator=torch.Generator().manual_seed(seed), **kw)
    a, a2, c = draw(1), draw(1), draw(2)
    assert a.shape == (1, 16, 3) and a.dtype == torch.float32
    assert torch.equal(a[:, 0], p0) and torch.equal(a, a2) and not torch.equal(a[:, 1:], c[:, 1:])
    assert not torch.equal(draw(1, keep_map=False)[:, 0], p0)
    H = torch.from_numpy(TW.ift_hypergrad(tb, phi)["H"].astype(np.float64))
    eps = torch.randn(1, 16, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = p0.double().unsqueeze(1) + gp_ops.laplace_draws(H, [n], eps)
    want[:, 0] = p0.double()
    assert (a.double() - want).abs().max() <= 1e-3 * (want - p0.double().unsqueeze(1)).abs().max() + 1e-6


def test_the_differenced_hessian_against_the_twin_at_the_default_step():
    """hessian_by_differences on the twin's adkf_mll_value_grad against the H of its adkf_ift_hypergrad, every golden gp_* fixture:
    max |H_d - H| <= 1e-4 max |H| at gp_ops.LAPLACE_STEP (measured: 2.7e-5 on the worst fixture; the docstring of
    phi_laplace_samples has the other steps)."""
    from adkf_ift_amd import gp_ops
    from oracle import cpu_twin as TW
    from test_cpu_twin import _batch

    files = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "gp_*.npz")))
    assert len(files) >= 30
    worst = 0.0
    for f in files:
        b, phi, n, m = _batch(np.load(f))
        H = TW.ift_hypergrad(b, phi)["H"][0].astype(np.float64)
        grad = lambda p: torch.from_numpy(TW.mll_value_grad(b, p.numpy(), want_dZ=False)[1])
        Hd = gp_ops.hessian_by_differences(grad, torch.from_numpy(phi), gp_ops.LAPLACE_STEP)[0].numpy()
        assert np.array_equal(Hd, Hd.T)
        worst = max(worst, float(np.abs(Hd - H).max() / np.abs(H).max()))
    print(f"differenced Hessian at step {gp_ops.LAPLACE_STEP:g}: worst max |H_d - H| / max |H| = {worst:.2e} over {len(files)} fixtures")
    assert worst <= 1e-4


# ---- the GPU problems are informative
_cases = {}


def twin_case(case):
    """A GPU case through the twin, once: (problem, b, fn, pool)."""
    if case not in _cases:
        cpu_twin, fn, pool = _mix_twin()
        p = R.problem(case)
        b = cpu_twin.CpuBatch(p["Zs"].numpy(), p["ys"].numpy(), np.zeros((p["G"] * p["M"], 4), np.float32), 0 if p["kernel"] == "rbf" else 1, n_s=p["n_s"])
        if p["ard"]:
            b.c.flags = ARD
        _cases[case] = (p, b, fn, pool)
    return _cases[case]


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_the_gpu_problems_are_informative(case):
    """Where the bound of the GPU test is a small fraction of the value it bounds, the test can see an error: the linear score is
    above 1e-30 on at least half the rows with a median eps32 unit / ref of at most 1e-3; BALD is above 1e-3 on at least half the rows
    with a median eps32 unit_bald / ref of at most 1e-2 over those; with best_f moved by 4 (M <= 5) the float32 linear score is 0
    on at least a quarter of the rows and positive on at least a twentieth; moved by 25 it is 0 on every row while every member's
    log EI is finite."""
    p, b, fn, pool = twin_case(case)
    X, phi, best = np.ascontiguousarray(p["X"].numpy()), np.ascontiguousarray(p["phi"].numpy()), p["best_f"]
    G, M, rows = p["G"], p["M"], p["rows"]
    mvE = twin_members(pool, b, phi, X, best, LATENT)
    lin_ok = bald_ok = 0
    rel_lin, rel_bald = [], []
    for g in range(G):
        ref = ref_outputs(mvE, p["members"], p["weights"], g, "ei", False)
        big = ref["ei"] > 1e-30
        lin_ok += int(big.sum())
        rel_lin.append(EPS32 * ref["unit_ei"][big] / ref["ei"][big])
        big = ref["bald"] > 1e-3
        bald_ok += int(big.sum())
        rel_bald.append(EPS32 * ref["unit_bald"][big] / ref["bald"][big])
    print(f"case {case}: linear score above 1e-30 on {lin_ok} of {G * rows} rows, BALD above 1e-3 on {bald_ok}; median eps32 unit / ref: "
          f"linear {np.median(np.concatenate(rel_lin)):.2e}, BALD {np.median(np.concatenate(rel_bald)):.2e}")
    assert 2 * lin_ok >= G * rows and np.median(np.concatenate(rel_lin)) <= 1e-3
    assert 2 * bald_ok >= G * rows and np.median(np.concatenate(rel_bald)) <= 1e-2
    for shift in ((R.MID_SHIFT, R.FAR_SHIFT) if M <= 5 else (R.FAR_SHIFT,)):
        moved = (best - np.float32(shift)).astype(np.float32)
        lin = mix_call(fn, b, phi, X, p["members"], p["weights"], moved, LATENT, want=(False, False, True))["score"]
        zero, pos = int((lin == 0).sum()), int((lin > 0).sum())
        print(f"case {case} shift {shift:g}: {zero} of {lin.size} rows with a float32 linear score of 0, {pos} with a positive one")
        if shift == R.MID_SHIFT:
            assert 4 * zero >= lin.size and 20 * pos >= lin.size
        else:
            assert zero == lin.size
            assert np.isfinite(twin_members(pool, b, phi, X, moved, LATENT | LOG)[2]).all()
