"""GPU: Thompson sampling over a shared pool (adkf_thompson_pool / gp_ops.thompson_pool) - the paths against the float64
restatement of the specification on every kind of task, the device selection against the ordering rule and against the oracle,
guard bands, independence from the other tasks of the batch, and the batched Thompson BO loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_predict_marginal as M
from test_gpu_predict_pool import _ill_batch, _pool
from test_predict_pool_cpu import select_ref
from test_thompson_pool_cpu import paths_ref

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _basis_and_draws(kernel, T, S, m, ns, d, seed, dev):
    from adkf_ift_amd import gp_ops

    g = torch.Generator().manual_seed(seed)
    omega, phase = gp_ops.rff_basis(kernel, d, m, generator=g)
    w, eps = torch.randn(T, S, m, generator=g), torch.randn(T, S, ns, generator=g)
    return omega.to(dev), phase.to(dev), w.to(dev), eps.to(dev)


def _check_paths(out, b, phi, Zs, ys, n_s, X, omega, phase, w, eps, tag):
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    paths = out["paths"].cpu().numpy()
    worst = 0.0
    for t in range(b.T):
        n = n_s[t]
        ref = paths_ref(Zs[t, :n], ys[t, :n], phi[t].cpu(), b.kernel, X.cpu(), omega.cpu(), phase.cpu(), w[t].cpu(), eps[t].cpu())
        err = np.abs(paths[t] - ref).max() / max(1.0, np.abs(ref).max())
        worst = max(worst, err)
        print(f"{tag} task {t} (n = {n}): |paths - ref| max / max(1, |ref| max) = {err:.3e}")
        assert err <= TOL, (tag, t, err)
        for q in range(paths.shape[1]):
            idx, val = select_ref(-paths[t, q], 1)
            assert int(out["sel_idx"][t, q]) == idx[0] and out["sel_val"][t, q].cpu().numpy().view(np.int32) == val[0].view(np.int32)
    return worst


PARITY_CASES = [  # (kernel, ns_max, d, rows, S, m): plain tasks (rows < 64, rows not a multiple of 64), then more than 128 points
    ("rbf", 5, 12, 37, 3, 64), ("matern", 48, 64, 333, 16, 1024), ("rbf", 128, 256, 130, 16, 256), ("matern", 128, 2048, 70, 8, 128),
    ("rbf", 200, 64, 333, 16, 256), ("matern", 1024, 12, 300, 5, 128),
]


@pytest.mark.parametrize("kernel,ns,d,rows,S,m", PARITY_CASES)
def test_parity_with_the_float64_restatement(dev, kernel, ns, d, rows, S, m):
    from adkf_ift_amd import gp_ops

    T = 3
    n_s = [ns, max(2, ns - 3), max(2, (2 * ns) // 3)]   # ragged
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 500 + ns + d, True)
    b, phi = M._fit(dev, Zs, ys, n_s, kernel, True)
    torch.cuda.synchronize()
    if ns <= 128:
        assert all(M._path(sc) < 2 for sc in M._scalars(b)), "these cases are meant for the float32 kernels"
    X = _pool(rows, d, 19).to(dev)
    omega, phase, w, eps = _basis_and_draws(kernel, T, S, m, ns, d, 7, dev)
    for flags in (gp_ops.REUSE_DIST | gp_ops.REUSE_INNER, 0):
        b.flags = flags
        out = gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, want_paths=True)
        _check_paths(out, b, phi, Zs, ys, n_s, X, omega, phase, w, eps, (kernel, ns, d, flags))


def test_parity_float64_task(dev):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, _ = _ill_batch(dev)   # (asserts that task 1 is flagged and another one is not)
    X = torch.cat([_pool(450, 2, 3) * 0.6, b.Z_s[1, :5].cpu()]).to(dev)
    S, m = 16, 256
    omega, phase, w, eps = _basis_and_draws("rbf", b.T, S, m, b.ns, 2, 8, dev)
    for flags in (gp_ops.REUSE_DIST | gp_ops.REUSE_INNER, 0):
        b.flags = flags
        out = gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, want_paths=True)
        _check_paths(out, b, phi, Zs, ys, n_s, X, omega, phase, w, eps, ("float64", flags))


def _selection_problem(dev, which):
    if which == "float64":
        b, phi, Zs, ys, n_s, _ = _ill_batch(dev)
        d = 2
    else:
        T, ns, d = 4, 48, 16
        n_s = [48, 45, 32, 12]
        Zs, ys, _ = M._features(T, ns, [0] * T, d, 92, True)
        b, phi = M._fit(dev, Zs, ys, n_s, "matern", True)
    rows = 100003
    X = _pool(rows, d, 13) * (1.0 if d > 2 else 0.6)
    for src, dst in ((11, 70001), (11, 99999), (5000, 64), (5000, 65), (31234, 31235)):
        X[dst] = X[src]
    return b, phi, Zs, ys, n_s, X.to(dev)


@pytest.mark.parametrize("which", ["float64", "float32"])
def test_selection_on_the_device(dev, which):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X = _selection_problem(dev, which)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    T, rows, S, m = b.T, X.shape[0], 16, 256
    omega, phase, w, eps = _basis_and_draws("rbf" if which == "float64" else "matern", T, S, m, b.ns, b.d, 9, dev)
    kw = dict(omega=omega, phase=phase, n_samples=S, w=w, eps=eps)
    first = gp_ops.thompson_pool(b, phi, X, **kw)
    assert first["paths"] is None and bool((first["sel_idx"] >= 0).all())
    win = first["sel_idx"].cpu()
    g = np.random.default_rng(2)
    # different lengths, each with the task's unexcluded winners: all of them; nothing; many rows; the duplicates' first copies
    lists = [win[0].tolist() + [3, 2, 2, rows + 5, -1], [], sorted(g.choice(rows, 5000, replace=False).tolist() + win[2, :3].tolist()),
             [11, 5000, int(win[3, 0])]]
    clean = [sorted({i for i in l if 0 <= i < rows}) for l in lists]
    for maximize in (False, True):
        out = gp_ops.thompson_pool(b, phi, X, maximize=maximize, exclude=lists, want_paths=True, **kw)
        paths = out["paths"].cpu().numpy()
        assert np.array_equal(paths[:, :, 11], paths[:, :, 70001]) and np.array_equal(paths[:, :, 64], paths[:, :, 5000])
        si, sv = out["sel_idx"].cpu().numpy(), out["sel_val"].cpu().numpy()
        for t in range(T):
            for q in range(S):
                idx, val = select_ref(paths[t, q] if maximize else -paths[t, q], 1, clean[t])
                assert si[t, q] == idx[0], (maximize, t, q, si[t, q], idx)
                assert sv[t, q].view(np.int32) == val[0].view(np.int32), (maximize, t, q)
        if not maximize:
            assert not set(si[0].tolist()) & set(win[0].tolist())
        for _ in range(2):   # paths = NULL: the same bits; and again
            o2 = gp_ops.thompson_pool(b, phi, X, maximize=maximize, exclude=lists, **kw)
            assert o2["paths"] is None
            assert torch.equal(o2["sel_idx"], out["sel_idx"]) and torch.equal(o2["sel_val"], out["sel_val"])


def test_planted_ties_go_to_the_lowest_index(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d, S, m = 4, 32, 16, 8, 128
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 78, True)
    b, phi = M._fit(dev, Zs, ys, [32, 20, 27, 9], "rbf", True)
    rows = 20011
    X = _pool(5, d, 1)[torch.arange(rows) % 5].contiguous().to(dev)   # five distinct rows: every score is shared by thousands
    omega, phase, w, eps = _basis_and_draws("rbf", T, S, m, ns, d, 10, dev)
    ex = [[0, 5], [], [1], []]
    out = gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, exclude=ex, want_paths=True)
    paths = out["paths"].cpu().numpy()
    for t in range(T):
        for q in range(S):
            idx, val = select_ref(-paths[t, q], 1, ex[t])
            assert int(out["sel_idx"][t, q]) == idx[0] and idx[0] < 15, (t, q)


def test_more_tasks_than_workgroups(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, S, m = 2000, 8, 8, 130, 4, 64
    g = torch.Generator().manual_seed(6)
    n_s = torch.randint(3, ns + 1, (T,), generator=g).tolist()
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 66, True)
    b, phi = M._fit(dev, Zs, ys, n_s, "rbf", True)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = _pool(rows, d, 14).to(dev)
    omega, phase, w, eps = _basis_and_draws("rbf", T, S, m, ns, d, 11, dev)
    ex = [[t % rows] for t in range(T)]
    out = gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, exclude=ex, want_paths=True)
    gp_ops.check_info(out["info"])
    paths, si, sv = out["paths"].cpu().numpy(), out["sel_idx"].cpu().numpy(), out["sel_val"].cpu().numpy()
    for t in range(T):
        for q in range(S):
            idx, val = select_ref(-paths[t, q], 1, ex[t])
            assert si[t, q] == idx[0] and sv[t, q].view(np.int32) == val[0].view(np.int32), (t, q)
    for t in (0, 777, 1999):
        ref = paths_ref(Zs[t, :n_s[t]], ys[t, :n_s[t]], phi[t].cpu(), 0, X.cpu(), omega.cpu(), phase.cpu(), w[t].cpu(), eps[t].cpu())
        assert np.abs(paths[t] - ref).max() <= TOL * max(1.0, np.abs(ref).max()), t


def test_a_task_does_not_depend_on_the_rest_of_the_batch(dev):
    """A task fitted and scored alone (a batch of one, with its own w / eps slices) gives the same paths and selection as inside a
    batch of four, bit for bit."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, S, m = 4, 40, 24, 1000, 8, 128
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 41, True)
    b, phi = M._fit(dev, Zs, ys, None, "matern", True)
    X = _pool(rows, d, 15).to(dev)
    omega, phase, w, eps = _basis_and_draws("matern", T, S, m, ns, d, 12, dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    out = gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, want_paths=True)
    for t in range(T):
        b1, phi1 = M._fit(dev, Zs[t:t + 1], ys[t:t + 1], None, "matern", True)
        assert torch.equal(phi1[0], phi[t]), "the fit itself must not couple tasks"
        b1.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
        o1 = gp_ops.thompson_pool(b1, phi1, X, omega=omega, phase=phase, n_samples=S, w=w[t:t + 1].contiguous(),
                                  eps=eps[t:t + 1].contiguous(), want_paths=True)
        assert torch.equal(o1["paths"][0], out["paths"][t]), t
        assert torch.equal(o1["sel_idx"][0], out["sel_idx"][t]) and torch.equal(o1["sel_val"][0], out["sel_val"][t]), t


def test_the_selection_is_right(dev):
    """Not only self-consistent: the picked row's oracle score is within 2 delta of the oracle's best eligible score, delta =
    1e-4 max(1, max|ref|) being the bound the paths are held to (the pick's device score is at least the true best row's device
    score, and each of the two is within delta of its oracle value)."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, S, m = 4, 48, 16, 20000, 16, 512
    n_s = [48, 45, 32, 12]
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 124, True)
    b, phi = M._fit(dev, Zs, ys, n_s, "matern", True)
    X = _pool(rows, d, 29).to(dev)
    omega, phase, w, eps = _basis_and_draws("matern", T, S, m, ns, d, 13, dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    ex = [list(range(0, rows, 7)), [], [5], list(range(100))]
    for maximize in (False, True):
        out = gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, maximize=maximize, exclude=ex)
        sel = out["sel_idx"].cpu().numpy()
        for t in range(T):
            ref = paths_ref(Zs[t, :n_s[t]], ys[t, :n_s[t]], phi[t].cpu(), 1, X.cpu(), omega.cpu(), phase.cpu(), w[t].cpu(), eps[t].cpu())
            score = ref if maximize else -ref
            ok = np.ones(rows, bool)
            ok[ex[t]] = False
            delta = 1e-4 * max(1.0, np.abs(ref).max())
            for q in range(S):
                assert ok[sel[t, q]], (t, q)
                assert score[q, sel[t, q]] >= score[q, ok].max() - 2 * delta, (maximize, t, q, score[q, sel[t, q]], score[q, ok].max())


def test_guard_bands_exact_sizes_and_a_skipped_task(dev):
    from adkf_ift_amd import _lib, gp_ops

    T, ns, d, rows, S, m = 3, 128, 64, 5003, 16, 256
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 8, True)
    b, phi = M._fit(dev, Zs, ys, [128, 100, 77], "rbf", True)
    lib = _lib.load()
    need = lib.adkf_workspace_bytes(T, ns, 0, d)
    ws, nb = b.workspace()
    assert nb == need
    b.n_s = torch.tensor([128, 0, 77], dtype=torch.int32, device=dev)   # task 1: skipped
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = _pool(rows, d, 3).to(dev)
    omega, phase, w, eps = _basis_and_draws("rbf", T, S, m, ns, d, 14, dev)
    guard = 4096
    ws_g = torch.full((need + guard,), 0x5a, dtype=torch.uint8, device=dev)
    ws_g[:need] = ws[:need]
    paths = torch.full((T * S * rows + guard,), 12345.0, device=dev)
    sel_idx = torch.full((T * S + guard,), 12345, dtype=torch.int64, device=dev)
    sel_val = torch.full((T * S + guard,), 12345.0, device=dev)
    sb = lib.adkf_thompson_pool_scratch_bytes(T, ns, S, m)
    assert sb > 0 and sb == lib.adkf_thompson_pool_scratch_bytes(T, ns, S, 4096)
    scratch = torch.full((sb + guard,), 0x5a, dtype=torch.uint8, device=dev)
    info = torch.empty(T, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    cb = b.c_struct()
    rc = lib.adkf_thompson_pool(C.byref(cb), p(phi), 0, p(X), rows, p(omega), p(phase), m, p(w), p(eps), S, None, None, p(paths), p(sel_idx),
                                p(sel_val), p(info), p(ws_g), need, p(scratch), sb, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    gp_ops.check_info(info)
    assert bool((ws_g[need:] == 0x5a).all()) and bool((scratch[sb:] == 0x5a).all())
    assert bool((paths[T * S * rows:] == 12345.0).all())
    assert bool((sel_idx[T * S:] == 12345).all()) and bool((sel_val[T * S:] == 12345.0).all())
    P = paths[:T * S * rows].view(T, S, rows)
    si, sv = sel_idx[:T * S].view(T, S).cpu().numpy(), sel_val[:T * S].view(T, S).cpu().numpy()
    assert bool((P[1] == 0).all()) and (si[1] == -1).all() and np.isneginf(sv[1]).all()
    for t in (0, 2):
        n = int(b.n_s[t])
        ref = paths_ref(Zs[t, :n], ys[t, :n], phi[t].cpu(), 0, X.cpu(), omega.cpu(), phase.cpu(), w[t].cpu(), eps[t].cpu())
        assert np.abs(P[t].cpu().numpy() - ref).max() <= TOL * max(1.0, np.abs(ref).max()), t
        for q in range(S):
            idx, val = select_ref(-P[t, q].cpu().numpy(), 1)
            assert si[t, q] == idx[0] and sv[t, q].view(np.int32) == val[0].view(np.int32)


def test_small_pools_and_argument_checks(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d, S, m = 4, 16, 8, 4, 64
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 4, True)
    b, phi = M._fit(dev, Zs, ys, [16, 8, 12, 5], "rbf", True)
    omega, phase, w, eps = _basis_and_draws("rbf", T, S, m, ns, d, 15, dev)
    kw = dict(omega=omega, phase=phase, n_samples=S, w=w, eps=eps)
    X = _pool(5, d, 2).to(dev)
    out = gp_ops.thompson_pool(b, phi, X, exclude=[[0, 1, 2, 3, 4], [], [2], None], want_paths=True, **kw)
    assert bool((out["sel_idx"][0] == -1).all()) and bool(torch.isneginf(out["sel_val"][0]).all())
    assert bool((out["sel_idx"][1:] >= 0).all()) and not bool((out["sel_idx"][2] == 2).any())
    out = gp_ops.thompson_pool(b, phi, X[:0], want_paths=True, **kw)      # an empty pool
    assert out["paths"].shape == (T, S, 0) and bool((out["sel_idx"] == -1).all()) and bool(torch.isneginf(out["sel_val"]).all())
    # the draws the call makes itself come back, and reproduce it
    o1 = gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, generator=torch.Generator().manual_seed(1))
    assert o1["w"].shape == (T, S, m) and o1["eps"].shape == (T, S, ns)
    o2 = gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, w=o1["w"], eps=o1["eps"])
    assert torch.equal(o1["sel_idx"], o2["sel_idx"]) and torch.equal(o1["sel_val"], o2["sel_val"])
    with pytest.raises(ValueError):
        gp_ops.thompson_pool(b, phi, X[:, :4].contiguous(), **kw)
    with pytest.raises(ValueError):
        gp_ops.thompson_pool(b, phi, X, omega=omega[:32], phase=phase[:32], n_samples=S)
    with pytest.raises(ValueError):
        gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=65)
    with pytest.raises(ValueError):
        gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w[:, :2], eps=eps)
    with pytest.raises(RuntimeError):
        gp_ops.thompson_pool(b, phi, X.cpu(), **kw)
    b_ard = gp_ops.GPBatch(b.Z_s, b.y_s, b.priors, "rbf", ard=True)
    with pytest.raises(ValueError):
        gp_ops.thompson_pool(b_ard, torch.zeros(T, 2 + d, device=dev), X, **kw)


def test_thompson_bo_loop(dev):
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=2, num_bo_iters=3, kernel_type="matern", device=dev, init_from=5000, noise_init=0.01,
              noise_prior=True, n_features=256)
    R = 4
    recs = BO.run_gp_ts_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(R)], **kw)
    again = BO.run_gp_ts_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(R)], **kw)
    assert recs == again, "two runs give equal records"
    assert len(recs) == R
    for r in range(R):
        assert len(recs[r]) == 1 + 3 * 2 and len(set(recs[r][1:])) == 6
        alone = BO.run_gp_ts_bo_batched(X, y, rngs=[np.random.default_rng(r)], **kw)
        assert alone[0] == recs[r], (r, "the batch couples replicates")
