"""GPU: Monte-Carlo (noisy) q-EI over a shared pool (adkf_qei_pool / gp_ops.qei_pool) - the five assertions of tests/qei_ref.py against
the float64 restatement on every kernel instance (one, two and four sample blocks, the float64 kernel, ARD), the bit-for-bit
properties (the incumbents move by Thompson's own path values, sel_val is the trace at the pick, NULL outputs, repeated calls, a task
alone, copies of a task), more tasks than workgroups, a pool of several chunks with planted duplicates, guard bands, exclusions and
small pools, and the batched q-EI BO loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_predict_marginal as M
import test_gpu_predict_pool as P
from qei_ref import check_task, task_paths
from test_gpu_believer_pool import _explicit
from test_gpu_thompson_pool import _basis_and_draws

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _refs(b, phi, Zs, ys, n_s, X, omega, phase, w, eps, ard=False):
    """(paths, sup_paths) of every task, float64: computed once per problem and shared by its modes."""
    Xh, ph = X.cpu().numpy(), phi.cpu().numpy()
    Zs, ys = np.asarray(Zs), np.asarray(ys)
    return [task_paths(Zs[t, :n_s[t]], ys[t, :n_s[t]], ph[t], b.kernel, Xh, omega.cpu().numpy(), phase.cpu().numpy(), w[t].cpu().numpy(),
                       eps[t].cpu().numpy(), ard=ard) for t in range(b.T)]


def _check(out, refs, best, maximize, tag, lists=None):
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    si, sv = out["sel_idx"].cpu().numpy(), out["sel_val"].cpu().numpy()
    tr = out["trace"].cpu().numpy() if out["trace"] is not None else None
    inc = out["inc"].cpu().numpy() if out["inc"] is not None else None
    for t, (paths, sup) in enumerate(refs):
        worst = check_task(paths, sup, None if best is None else float(best[t]), maximize, si[t], sv[t], None if tr is None else tr[t],
                           None if inc is None else inc[t], excluded=lists[t] if lists else (), tag=(tag, t))
        print(f"{tag} task {t}: picks {si[t].tolist()[:8]}, sel_val[0] {sv[t, 0]:.5f}, worst error / bound {worst:.3f}")
        if tr is not None:   # sel_val is the trace at the pick, bit for bit
            for j, p in enumerate(si[t].tolist()):
                if p >= 0:
                    assert sv[t, j:j + 1].view(np.int32)[0] == tr[t, j, p:p + 1].view(np.int32)[0], (tag, t, j)


def _modes(ys, n_s):
    """(maximize, best_f or None): noisy and plain q-EI, in both senses; best_f the median label, the believer tests' incumbent (the best
    observed label leaves plain q-EI within a few delta of zero on these pools, which the reference must not be)."""
    med = torch.tensor([float(ys[t, :n].median()) for t, n in enumerate(n_s)])
    return ((False, None), (True, None), (False, med), (True, med))


CASES = [  # (kernel, n_s, d, rows, q, S, m)
    ("rbf", [5, 4, 2], 12, 37, 3, 3, 64),                # one partial tile, one partial block
    ("matern", [48, 45, 31], 16, 300, 8, 80, 128),       # NB = 2, second block partial, several tiles
    ("rbf", [128, 125, 85], 64, 130, 5, 256, 256),       # NB = 4, full panels
    ("rbf", [200, 197, 133], 64, 333, 4, 16, 128),       # more than 128 points, refined tasks
    ("rbf", [32, 29, 21], 8, 200, 64, 16, 64),           # the full pick count
]


@pytest.mark.parametrize("kernel,n_s,d,rows,q,S,m", CASES)
def test_against_the_reference(dev, kernel, n_s, d, rows, q, S, m):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, _ = _explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    omega, phase, w, eps = _basis_and_draws(kernel, b.T, S, m, b.ns, d, 7, dev)
    refs = _refs(b, phi, Zs, ys, n_s, X, omega, phase, w, eps)
    try:
        for flags in (0, gp_ops.REUSE_DIST | gp_ops.REUSE_INNER):   # (the second: the state the call before it left)
            b.flags = flags
            for maximize, best in _modes(ys, n_s):
                out = gp_ops.qei_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, q=q, w=w, eps=eps, maximize=maximize,
                                      best_f=None if best is None else best.to(dev), want_trace=True, want_inc=True)
                _check(out, refs, best, maximize, (kernel, max(n_s), S, flags, maximize, best is None))
                assert bool((out["sel_idx"] >= 0).all())
    finally:
        b.flags = 0


def _ill(dev):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, _ = P._ill_batch(dev)   # (asserts that task 1 is flagged and another one is not)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    # a pool twice as wide as the support sets: inside their hull no row improves on task 0's noisy incumbents (the reference, alone on
    # the CPU, has a step-0 maximum of 0 there at a scale of 0.6), and the reference maximum has to be far from zero
    X = torch.cat([P._pool(300, 2, 3) * 2.0, b.Z_s[1, :5].cpu()]).to(dev)
    return b, phi, Zs, ys, n_s, X


def test_mixed_kinds_in_one_call(dev):
    """A float64 task and float32 tasks in one call, at one and at two sample blocks."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X = _ill(dev)
    for S in (16, 80):
        omega, phase, w, eps = _basis_and_draws("rbf", b.T, S, 128, b.ns, 2, 8, dev)
        refs = _refs(b, phi, Zs, ys, n_s, X, omega, phase, w, eps)
        for maximize, best in _modes(ys, n_s):
            out = gp_ops.qei_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, q=5, w=w, eps=eps, maximize=maximize,
                                  best_f=None if best is None else best.to(dev), want_trace=True, want_inc=True)
            _check(out, refs, best, maximize, ("mixed", S, maximize, best is None))


def test_ard_batch(dev):
    import test_gpu_believer_pool_ard as BVA

    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, S, m = "matern", [48, 45, 32], 64, 333, 80, 256
    b, phi, Zs, ys, n_s, X, _ = BVA._explicit(dev, kernel, n_s, d, rows, 748)
    omega, phase, w, eps = _basis_and_draws(kernel, b.T, S, m, b.ns, d, 7, dev)
    refs = _refs(b, phi, Zs, ys, n_s, X, omega, phase, w, eps, ard=True)
    for maximize, best in _modes(ys, n_s):
        out = gp_ops.qei_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, q=5, w=w, eps=eps, maximize=maximize,
                              best_f=None if best is None else best.to(dev), want_trace=True, want_inc=True)
        _check(out, refs, best, maximize, ("ard", maximize, best is None))


def _thompson_paths(b, phi, X, omega, phase, w, eps):
    """paths [T, S, rows] of gp_ops.thompson_pool on the same draws, in blocks of at most 64 samples."""
    from adkf_ift_amd import gp_ops

    draw = gp_ops.thompson_pool_ard if b.ard else gp_ops.thompson_pool
    S = w.shape[1]
    parts = [draw(b, phi, X, omega=omega, phase=phase, n_samples=min(64, S - s0), w=w[:, s0:s0 + 64].contiguous(),
                  eps=eps[:, s0:s0 + 64].contiguous(), want_paths=True)["paths"] for s0 in range(0, S, 64)]
    return torch.cat(parts, 1)


def test_the_incumbents_move_by_thompsons_path_values_bit_for_bit(dev):
    from adkf_ift_amd import gp_ops

    S, q = 80, 6
    kernel, n_s, d, rows = "matern", [48, 45, 31], 16, 300
    b, phi, Zs, ys, n_s, X, _ = _explicit(dev, kernel, n_s, d, rows, 548)
    problems = [(b, phi, X, _basis_and_draws(kernel, b.T, S, 128, b.ns, d, 7, dev))]
    bi, phii, _, _, _, Xi = _ill(dev)
    problems.append((bi, phii, Xi, _basis_and_draws("rbf", bi.T, S, 128, bi.ns, 2, 8, dev)))
    for k, (b, phi, X, (omega, phase, w, eps)) in enumerate(problems):
        paths = _thompson_paths(b, phi, X, omega, phase, w, eps)
        for maximize in (False, True):
            out = gp_ops.qei_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, q=q, w=w, eps=eps, maximize=maximize, want_inc=True)
            inc, si = out["inc"], out["sel_idx"]
            assert bool((si >= 0).all())
            for t in range(b.T):
                for j in range(q):
                    f = paths[t, :, int(si[t, j])]
                    want = torch.maximum(inc[t, j], f) if maximize else torch.minimum(inc[t, j], f)
                    assert torch.equal(inc[t, j + 1], want), (k, maximize, t, j)
            assert not torch.equal(inc[:, 0], inc[:, q])


def test_deterministic_and_independent_of_the_batch(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, q, S, m = CASES[1]
    b, phi, Zs, ys, n_s, X, _ = _explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    omega, phase, w, eps = _basis_and_draws(kernel, b.T, S, m, b.ns, d, 7, dev)
    lists = [[0, 7], [], [3]]
    kw = dict(omega=omega, phase=phase, n_samples=S, q=q)
    first = gp_ops.qei_pool(b, phi, X, w=w, eps=eps, exclude=lists, want_trace=True, want_inc=True, **kw)
    again = gp_ops.qei_pool(b, phi, X, w=w, eps=eps, exclude=lists, want_trace=True, want_inc=True, **kw)
    names = ("sel_idx", "sel_val", "trace", "inc")
    for name in names:
        assert torch.equal(first[name], again[name]), name
    none = gp_ops.qei_pool(b, phi, X, w=w, eps=eps, exclude=lists, **kw)      # trace == inc == NULL: the same bits
    assert none["trace"] is None and none["inc"] is None
    for name in names[:2]:
        assert torch.equal(first[name], none[name]), name
    for t in range(b.T):   # each task alone in a T = 1 batch
        b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), kernel,
                            n_s=torch.tensor([n_s[t]], dtype=torch.int32))
        o1 = gp_ops.qei_pool(b1, phi[t:t + 1].contiguous(), X, w=w[t:t + 1].contiguous(), eps=eps[t:t + 1].contiguous(), exclude=[lists[t]],
                             want_trace=True, want_inc=True, **kw)
        for name in names:
            assert torch.equal(o1[name][0], first[name][t]), (t, name)
    # a batch of copies of task 0: every copy gets the same bits
    rep = lambda a: a[:1].expand(3, *a.shape[1:]).contiguous()
    bc = gp_ops.GPBatch(rep(b.Z_s), rep(b.y_s), rep(b.priors), kernel, n_s=torch.tensor([n_s[0]] * 3, dtype=torch.int32))
    oc = gp_ops.qei_pool(bc, rep(phi), X, w=rep(w), eps=rep(eps), exclude=[lists[0]] * 3, want_trace=True, want_inc=True, **kw)
    for name in names:
        for t in range(3):
            assert torch.equal(oc[name][t], first[name][0]), (name, t)


def test_more_tasks_than_workgroups(dev):
    """T = 300 tiny tasks (the shape of the believer's test of this name), one workgroup serving several tasks: assertions 1-5 on every task."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, q, S, m = 300, 8, 4, 130, 3, 16, 64
    g = torch.Generator().manual_seed(77)
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 77, True)
    n_s = [int(x) for x in torch.randint(3, ns + 1, (T,), generator=g)]
    n_s[0] = ns
    b = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.empty(T, 4, device=dev), "matern", n_s=torch.tensor(n_s, dtype=torch.int32))
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    phi = phi0.clone()
    phi[:, 0] = torch.linspace(-1.0, -3.0, T, device=dev)
    phi[:, 1] = 0.3
    X = P._pool(rows, d, 78).to(dev)
    omega, phase, w, eps = _basis_and_draws("matern", T, S, m, ns, d, 9, dev)
    refs = _refs(b, phi, Zs, ys, n_s, X, omega, phase, w, eps)
    out = gp_ops.qei_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, q=q, w=w, eps=eps, want_trace=True, want_inc=True)
    gp_ops.check_info(out["info"])
    si, sv, tr, inc = (out[k].cpu().numpy() for k in ("sel_idx", "sel_val", "trace", "inc"))
    worst = max(check_task(refs[t][0], refs[t][1], None, False, si[t], sv[t], tr[t], inc[t], tag=("T300", t)) for t in range(T))
    print(f"T = 300: worst error / bound {worst:.3f}")


def test_a_pool_of_several_chunks_with_planted_duplicates(dev):
    from adkf_ift_amd import gp_ops

    b, phi, X, _ = P._selection_problem(dev, "float64+refined")   # 100 003 rows; a float64 task and float32 ones
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    _, _, Zs, ys, n_s, _ = P._ill_batch(dev)
    q, S, m = 3, 16, 64
    omega, phase, w, eps = _basis_and_draws("rbf", b.T, S, m, b.ns, 2, 10, dev)
    refs = _refs(b, phi, Zs, ys, n_s, X, omega, phase, w, eps)
    out = gp_ops.qei_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, q=q, w=w, eps=eps, want_trace=True, want_inc=True)
    _check(out, refs, None, False, "100003")
    tr = out["trace"]
    for src, dst in ((11, 70001), (11, 99999), (5000, 64), (5000, 65), (31234, 31235)):   # duplicates score alike, bit for bit
        assert torch.equal(tr[:, :, src], tr[:, :, dst]), (src, dst)
    # the best row of task 0 excluded, two copies of it planted far apart in other chunks: the pick is the lower copy
    p0 = int(out["sel_idx"][0, 0])
    Xd = X.clone()
    Xd[70001] = X[p0]; Xd[99999] = X[p0]
    o2 = gp_ops.qei_pool(b, phi, Xd, omega=omega, phase=phase, n_samples=S, q=1, w=w, eps=eps, exclude=[[p0], [], [], []], want_trace=True)
    assert torch.equal(o2["trace"][0, 0, 70001], o2["trace"][0, 0, p0]) and torch.equal(o2["trace"][0, 0, 99999], o2["trace"][0, 0, p0])
    assert int(o2["sel_idx"][0, 0]) == 70001 and torch.equal(o2["sel_val"][0, 0], out["sel_val"][0, 0])
    none = gp_ops.qei_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, q=q, w=w, eps=eps)   # nothing of size T x rows
    assert torch.equal(none["sel_idx"], out["sel_idx"]) and torch.equal(none["sel_val"], out["sel_val"])


def test_guard_bands(dev):
    from adkf_ift_amd import _lib, gp_ops

    kernel, n_s, d, rows, q, S, m = CASES[1]
    b, phi, Zs, ys, n_s, X, _ = _explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    omega, phase, w, eps = _basis_and_draws(kernel, b.T, S, m, b.ns, d, 7, dev)
    T, ns = b.T, b.ns
    lib = _lib.load()
    need = lib.adkf_workspace_bytes(T, ns, 0, d)
    sb = lib.adkf_qei_pool_scratch_bytes(T, ns, S, m)
    guard = 4096
    ws_g = torch.full((need + guard,), 0x5a, dtype=torch.uint8, device=dev)
    scratch = torch.full((sb + guard,), 0x5a, dtype=torch.uint8, device=dev)
    trace = torch.full((T * q * rows + guard,), 12345.0, device=dev)
    inc = torch.full((T * (q + 1) * S + guard,), 12345.0, device=dev)
    sel_idx = torch.full((T * q + guard,), 12345, dtype=torch.int64, device=dev)
    sel_val = torch.full((T * q + guard,), 12345.0, device=dev)
    info = torch.empty(T, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    cb = b.c_struct()
    skipped = torch.tensor([n_s[0], 0, n_s[2]], dtype=torch.int32, device=dev)   # task 1: skipped
    cb.n_s = skipped.data_ptr()
    cb.flags = 0
    rc = lib.adkf_qei_pool(C.byref(cb), p(phi), 0, p(X), rows, p(omega), p(phase), m, p(w), p(eps), S, None, None, None, q, p(trace), p(inc),
                           p(sel_idx), p(sel_val), p(info), p(ws_g), need, p(scratch), sb, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    gp_ops.check_info(info)
    assert bool((ws_g[need:] == 0x5a).all()) and bool((scratch[sb:] == 0x5a).all())
    assert bool((trace[T * q * rows:] == 12345.0).all()) and bool((inc[T * (q + 1) * S:] == 12345.0).all())
    assert bool((sel_idx[T * q:] == 12345).all()) and bool((sel_val[T * q:] == 12345.0).all())
    si, sv = sel_idx[:T * q].view(T, q), sel_val[:T * q].view(T, q)
    tr = trace[:T * q * rows].view(T, q, rows)
    assert bool((si[1] == -1).all()) and bool(torch.isneginf(sv[1]).all()) and bool((tr[1] == 0).all())
    # the other tasks do not see the skipped one
    full = gp_ops.qei_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, q=q, w=w, eps=eps, want_trace=True, want_inc=True)
    for t in (0, 2):
        assert torch.equal(si[t], full["sel_idx"][t]) and torch.equal(tr[t], full["trace"][t])
        assert torch.equal(inc[:T * (q + 1) * S].view(T, q + 1, S)[t], full["inc"][t])


def test_exclusions_and_small_pools(dev):
    from adkf_ift_amd import gp_ops

    T, d, rows, S, m = 3, 16, 6000, 16, 64
    b, phi, Zs, ys, n_s, _, _ = _explicit(dev, "matern", [48, 45, 31], d, 300, 548)
    X = P._pool(rows, d, 5).to(dev)
    omega, phase, w, eps = _basis_and_draws("matern", T, S, m, b.ns, d, 7, dev)
    kw = dict(omega=omega, phase=phase, n_samples=S, w=w, eps=eps)
    free = gp_ops.qei_pool(b, phi, X, q=4, **kw)
    keep = sorted(set(range(0, rows, 7)) | set(free["sel_idx"][0].tolist()))
    lists = [[i for i in range(rows) if i not in keep][:5000] + free["sel_idx"][0].tolist(), [], free["sel_idx"][2, :1].tolist()]
    assert len(lists[0]) > 5000
    out = gp_ops.qei_pool(b, phi, X, q=4, exclude=lists, **kw)
    for t in range(T):
        got = out["sel_idx"][t].tolist()
        assert len(set(got)) == 4 and min(got) >= 0 and not set(got) & set(lists[t]), t
    assert torch.equal(out["sel_idx"][1], free["sel_idx"][1]) and out["sel_idx"][2, 0] != free["sel_idx"][2, 0]
    # a pool of 9 rows with q = 16: nine picks, then the -1 / -inf tail with the state unchanged; an empty pool: the tail only
    out = gp_ops.qei_pool(b, phi, X[:9], q=16, want_trace=True, want_inc=True, **kw)
    si = out["sel_idx"].cpu()
    for t in range(T):
        assert sorted(si[t, :9].tolist()) == list(range(9)) and bool((si[t, 9:] == -1).all())
    assert bool(torch.isneginf(out["sel_val"][:, 9:]).all())
    assert torch.equal(out["inc"][:, 9:10].expand(-1, 8, -1), out["inc"][:, 9:])
    assert torch.equal(out["trace"][:, 9:10].expand(-1, 7, -1), out["trace"][:, 9:])
    empty = gp_ops.qei_pool(b, phi, X[:0], q=3, want_trace=True, want_inc=True, **kw)
    assert bool((empty["sel_idx"] == -1).all()) and bool(torch.isneginf(empty["sel_val"]).all()) and empty["trace"].shape == (T, 3, 0)
    assert torch.equal(empty["inc"][:, 0], out["inc"][:, 0]) and torch.equal(empty["inc"][:, 3], out["inc"][:, 0])   # the noisy incumbents need no pool
    with pytest.raises(ValueError):
        gp_ops.qei_pool(b, phi, X[:, :4].contiguous(), q=3, **kw)
    with pytest.raises(ValueError):
        gp_ops.qei_pool(b, phi, X, q=65, **kw)
    with pytest.raises(ValueError):
        gp_ops.qei_pool(b, phi, X, q=3, omega=omega, phase=phase, n_samples=257)
    with pytest.raises(ValueError):
        gp_ops.qei_pool(b, phi, X, q=3, best_f=torch.zeros(2, device=dev), **kw)
    with pytest.raises(RuntimeError):
        gp_ops.qei_pool(b, phi, X.cpu(), q=3, **kw)


def test_bo_loop(dev):
    """The problem of the believer's BO test: picks are distinct and were not queried before, the best value found never gets worse,
    and the same seeds give the same records."""
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(5)
    X = torch.randn(200, 8, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, num_bo_iters=3, kernel_type="matern", device=dev, init_from=100, noise_init=0.01, noise_prior=True,
              n_samples=32, n_features=128)
    rngs = lambda: [np.random.default_rng(s) for s in range(2)]
    for noisy in (True, False):
        recs = BO.run_gp_qei_bo_batched(X, y, rngs=rngs(), query_batch_size=4, noisy=noisy, **kw)
        assert len(recs) == 2
        for r, rec in enumerate(recs):
            assert len(rec) == 1 + 3 * 4 and len(set(rec[1:])) == 12
            init = np.random.default_rng(r).choice(np.arange(100, 200), size=6, replace=False).tolist()
            assert rec[0] == min(init) and not set(rec[1:]) & set(init)
            best = np.minimum.accumulate(np.array(rec))      # (the pool is sorted by y: the index is the rank)
            assert (np.diff(best) <= 0).all()
        assert recs == BO.run_gp_qei_bo_batched(X, y, rngs=rngs(), query_batch_size=4, noisy=noisy, **kw)
    with pytest.raises(ValueError):
        BO.run_gp_qei_bo_batched(X, y, rngs=rngs(), query_batch_size=65, **kw)
