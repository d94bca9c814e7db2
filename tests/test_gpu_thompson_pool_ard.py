"""GPU: Thompson sampling over a shared pool for ARD batches (adkf_thompson_pool_ard / gp_ops.thompson_pool_ard) - the paths
against the float64 restatement on the scaled features at fixed per-dimension lengthscales and after an ARD fit, on the float64
path, against the isotropic entry at equal lengthscales, the device selection, bit-for-bit properties, guard bands, the gp_ops
surface and the batched Thompson BO loop with ard=True."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_predict_marginal import _features, _path, _scalars
from test_gpu_predict_marginal_ard import _batch, _fit_ard, _isp, _spread_phi
from test_gpu_predict_pool import _pool
from test_gpu_thompson_pool import _basis_and_draws
from test_predict_pool_cpu import select_ref
from test_thompson_pool_ard_cpu import ard_paths_ref

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _check_paths(out, b, phi, Zs, ys, n_s, X, omega, phase, w, eps, tag, maximize=False):
    """The normalisation of test_gpu_thompson_pool._check_paths, against the ARD restatement; the selection bit for bit."""
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    paths = out["paths"].cpu().numpy()
    worst = 0.0
    for t in range(b.T):
        n = n_s[t]
        ref = ard_paths_ref(Zs[t, :n].numpy(), ys[t, :n], phi[t].cpu().numpy(), b.kernel, X.cpu().numpy(), omega.cpu(), phase.cpu(),
                            w[t].cpu(), eps[t].cpu())
        err = np.abs(paths[t] - ref).max() / max(1.0, np.abs(ref).max())
        worst = max(worst, err)
        print(f"{tag} task {t} (n = {n}): |paths - ref| max / max(1, |ref| max) = {err:.3e}")
        assert err <= TOL, (tag, t, err)
        for q in range(paths.shape[1]):
            idx, val = select_ref(paths[t, q] if maximize else -paths[t, q], 1)
            assert int(out["sel_idx"][t, q]) == idx[0] and out["sel_val"][t, q].cpu().numpy().view(np.int32) == val[0].view(np.int32)
    return worst


def _ragged(ns):
    return [ns, max(2, ns - 3), max(2, (2 * ns) // 3)]


PARITY_CASES = [  # (kernel, ns_max, d, rows, S, m)
    ("rbf", 5, 6, 37, 3, 64),            # d not a multiple of 4, rows < 64
    ("matern", 48, 64, 333, 16, 256),    # one support panel, a partial last row tile
    ("rbf", 128, 12, 130, 5, 128),       # two support panels
    ("matern", 200, 12, 300, 16, 128),   # more than 128 points
]


@pytest.mark.parametrize("kernel,ns,d,rows,S,m", PARITY_CASES)
def test_parity_at_a_fixed_phi(dev, kernel, ns, d, rows, S, m):
    from adkf_ift_amd import gp_ops

    T = 3
    n_s = _ragged(ns)
    Zs, ys, _ = _features(T, ns, [0] * T, d, 700 + ns + d, True)
    b = _batch(dev, Zs, ys, n_s, kernel)
    phi = _spread_phi(dev, b, True, ns + d)
    X = _pool(rows, d, 19).to(dev)
    omega, phase, w, eps = _basis_and_draws(kernel, T, S, m, ns, d, 7, dev)
    for flags in (0, gp_ops.REUSE_INNER):   # REUSE_INNER: the state the evaluation before it left
        b.flags = flags
        out = gp_ops.thompson_pool_ard(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, want_paths=True)
        _check_paths(out, b, phi, Zs, ys, n_s, X, omega, phase, w, eps, (kernel, ns, d, flags))


@pytest.mark.parametrize("kernel,ns,d", [("matern", 16, 12), ("rbf", 64, 64)])
def test_parity_after_an_ard_fit(dev, kernel, ns, d):
    from adkf_ift_amd import gp_ops

    T, rows, S, m = 3, 333, 8, 128
    n_s = _ragged(ns)
    Zs, ys, _ = _features(T, ns, [0] * T, d, 300 + ns + d, True)
    b, phi = _fit_ard(dev, Zs, ys, n_s, kernel, True)
    assert phi.shape == (T, 2 + d)
    X = _pool(rows, d, 23).to(dev)
    omega, phase, w, eps = _basis_and_draws(kernel, T, S, m, ns, d, 17, dev)
    # the size of the cosine's argument at the fitted lengthscales (short lengthscales make it large)
    ell = torch.nn.functional.softplus(phi[:, 2:].double().cpu())
    for t in range(T):
        xt = (X.double().cpu() - Zs[t, :n_s[t]].double().mean(0)) / ell[t]
        print(f"{kernel} ns {ns} d {d} task {t}: largest |omega_j . x~| = {float((xt @ omega.double().cpu().T).abs().max()):.3e}, "
              f"lengthscales in [{float(ell[t].min()):.3e}, {float(ell[t].max()):.3e}]")
    b.flags = gp_ops.REUSE_INNER
    out = gp_ops.thompson_pool_ard(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, want_paths=True)
    _check_paths(out, b, phi, Zs, ys, n_s, X, omega, phase, w, eps, (kernel, ns, d, "fit"))


def test_float64_path(dev):
    """The recipe of test_gpu_predict_marginal_ard.test_float64_path: every task takes the float64 kernels."""
    from adkf_ift_amd import gp_ops
    from adkf_ift_amd.synthetic import make_tasks

    tasks = make_tasks(3, 16, 2, N_q=64, regression=True, first_task=1800)
    Zs, _ = tasks.features()
    n_s = [16, 15, 16]
    b = _batch(dev, Zs, tasks.y_s, n_s, "rbf")
    b.priors.copy_(torch.tensor([[0.0, -1.0, 0.0, -1.0]] * 3))
    phi = torch.tensor([[-9.0, 0.0, _isp(2.0), _isp(3.0)]] * 3, dtype=torch.float32, device=dev)
    X = torch.cat([_pool(450, 2, 3) * 0.6, Zs[1, :5]]).to(dev)   # with five copies of support rows
    S, m = 16, 256
    assert X.shape[0] == 455
    omega, phase, w, eps = _basis_and_draws("rbf", 3, S, m, 16, 2, 8, dev)
    for flags in (0, gp_ops.REUSE_INNER):
        b.flags = flags
        out = gp_ops.thompson_pool_ard(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, want_paths=True)
        torch.cuda.synchronize()
        sc = _scalars(b)
        assert all(_path(sc[t]) == 2 for t in range(3)), [float(sc[t][45]) for t in range(3)]
        _check_paths(out, b, phi, Zs, tasks.y_s, n_s, X, omega, phase, w, eps, ("float64", flags))


def test_equal_lengthscales_match_the_isotropic_entry(dev):
    """Each call is within TOL of the same float64 reference (same normalisation), so the two are within 2 TOL of each other."""
    from adkf_ift_amd import gp_ops
    from test_thompson_pool_cpu import paths_ref

    T, ns, d, rows, S, m = 3, 48, 20, 200, 8, 128
    n_s = [48, 40, 29]
    Zs, ys, _ = _features(T, ns, [0] * T, d, 17, True)
    raw = torch.tensor([[-2.5, 0.2, _isp(3.0)], [-1.5, -0.3, _isp(4.5)], [-3.0, 0.5, _isp(2.2)]], dtype=torch.float32, device=dev)
    phi_ard = torch.cat([raw[:, :2], raw[:, 2:].expand(T, d)], 1).contiguous()
    ba = _batch(dev, Zs, ys, n_s, "rbf")
    ba.priors.zero_()
    bi = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.zeros(T, 4, device=dev), "rbf", n_s=torch.tensor(n_s, dtype=torch.int32))
    X = _pool(rows, d, 31).to(dev)
    omega, phase, w, eps = _basis_and_draws("rbf", T, S, m, ns, d, 18, dev)
    kw = dict(omega=omega, phase=phase, n_samples=S, w=w, eps=eps, want_paths=True)
    pa = gp_ops.thompson_pool_ard(ba, phi_ard, X, **kw)
    pi = gp_ops.thompson_pool(bi, raw, X, **kw)
    gp_ops.check_info(pa["info"]); gp_ops.check_info(pi["info"])
    for t in range(T):
        ref = paths_ref(Zs[t, :n_s[t]], ys[t, :n_s[t]], raw[t].cpu(), 0, X.cpu(), omega.cpu(), phase.cpu(), w[t].cpu(), eps[t].cpu())
        err = float((pa["paths"][t] - pi["paths"][t]).abs().max()) / max(1.0, np.abs(ref).max())
        print(f"task {t}: |ard - iso| max / max(1, |ref| max) = {err:.3e}")
        assert err <= 2 * TOL, (t, err)


def test_selection_on_the_device(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d = 4, 48, 16
    n_s = [48, 45, 32, 12]
    Zs, ys, _ = _features(T, ns, [0] * T, d, 92, True)
    b = _batch(dev, Zs, ys, n_s, "matern")
    phi = _spread_phi(dev, b, True, 5)
    rows = 100003
    X = _pool(rows, d, 13)
    for src, dst in ((11, 70001), (11, 99999), (5000, 64), (5000, 65), (31234, 31235)):   # as _selection_problem plants them
        X[dst] = X[src]
    X = X.to(dev)
    S, m = 16, 256
    omega, phase, w, eps = _basis_and_draws("matern", T, S, m, ns, d, 9, dev)
    kw = dict(omega=omega, phase=phase, n_samples=S, w=w, eps=eps)
    first = gp_ops.thompson_pool_ard(b, phi, X, **kw)
    gp_ops.check_info(first["info"])
    assert first["paths"] is None and bool((first["sel_idx"] >= 0).all())
    b.flags = gp_ops.REUSE_INNER
    win = first["sel_idx"].cpu()
    g = np.random.default_rng(2)
    # different lengths, each with the task's unexcluded winners: all of them; nothing; many rows; the duplicates' first copies
    lists = [win[0].tolist() + [3, 2, 2, rows + 5, -1], [], sorted(g.choice(rows, 5000, replace=False).tolist() + win[2, :3].tolist()),
             [11, 5000, int(win[3, 0])]]
    clean = [sorted({i for i in l if 0 <= i < rows}) for l in lists]
    for maximize in (False, True):
        out = gp_ops.thompson_pool_ard(b, phi, X, maximize=maximize, exclude=lists, want_paths=True, **kw)
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
        o2 = gp_ops.thompson_pool_ard(b, phi, X, maximize=maximize, exclude=lists, **kw)   # paths = NULL: the same bits
        assert o2["paths"] is None
        assert torch.equal(o2["sel_idx"], out["sel_idx"]) and torch.equal(o2["sel_val"], out["sel_val"])


def test_bit_for_bit_properties(dev):
    """A repeated call is equal; a task run alone (a batch of one, with its own w / eps slices) equals its slice of the batch."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, S, m = 4, 40, 24, 1000, 8, 128
    n_s = [40, 31, 40, 9]
    Zs, ys, _ = _features(T, ns, [0] * T, d, 41, True)
    b = _batch(dev, Zs, ys, n_s, "matern")
    phi = _spread_phi(dev, b, True, 6)
    X = _pool(rows, d, 15).to(dev)
    omega, phase, w, eps = _basis_and_draws("matern", T, S, m, ns, d, 12, dev)
    kw = dict(omega=omega, phase=phase, n_samples=S, want_paths=True)
    out = gp_ops.thompson_pool_ard(b, phi, X, w=w, eps=eps, **kw)
    gp_ops.check_info(out["info"])
    again = gp_ops.thompson_pool_ard(b, phi, X, w=w, eps=eps, **kw)
    for k in ("paths", "sel_idx", "sel_val"):
        assert torch.equal(out[k], again[k]), k
    for t in range(T):
        b1 = gp_ops.GPBatch(Zs[t:t + 1].to(dev), ys[t:t + 1].to(dev), b.priors[t:t + 1].clone(), "matern", ard=True,
                            n_s=torch.tensor(n_s[t:t + 1], dtype=torch.int32))
        o1 = gp_ops.thompson_pool_ard(b1, phi[t:t + 1].contiguous(), X, w=w[t:t + 1].contiguous(), eps=eps[t:t + 1].contiguous(), **kw)
        assert torch.equal(o1["paths"][0], out["paths"][t]), t
        assert torch.equal(o1["sel_idx"][0], out["sel_idx"][t]) and torch.equal(o1["sel_val"][0], out["sel_val"][t]), t


def test_guard_bands_exact_sizes_and_a_skipped_task(dev):
    from adkf_ift_amd import _lib, gp_ops

    T, ns, d, rows, S, m = 3, 128, 64, 5003, 16, 256
    n_s = [128, 0, 77]   # task 1: skipped
    Zs, ys, _ = _features(T, ns, [0] * T, d, 8, True)
    b = _batch(dev, Zs, ys, [128, 100, 77], "rbf")
    phi = _spread_phi(dev, b, True, 8)
    lib = _lib.load()
    need = lib.adkf_workspace_bytes_ard(T, ns, 0, d)
    _, nb = b.workspace()
    assert nb == need
    b.n_s = torch.tensor(n_s, dtype=torch.int32, device=dev)
    b.flags = 0
    X = _pool(rows, d, 3).to(dev)
    omega, phase, w, eps = _basis_and_draws("rbf", T, S, m, ns, d, 14, dev)
    excl = torch.arange(rows, dtype=torch.int64, device=dev)      # task 2 may select nothing: its list is the whole pool
    excl_off = torch.tensor([0, 0, 0, rows], dtype=torch.int64, device=dev)
    guard = 4096
    ws_g = torch.full((need + guard,), 0x5a, dtype=torch.uint8, device=dev)
    paths = torch.full((T * S * rows + guard,), 12345.0, device=dev)
    sel_idx = torch.full((T * S + guard,), 12345, dtype=torch.int64, device=dev)
    sel_val = torch.full((T * S + guard,), 12345.0, device=dev)
    sb = lib.adkf_thompson_pool_scratch_bytes(T, ns, S, m)
    scratch = torch.full((sb + guard,), 0x5a, dtype=torch.uint8, device=dev)
    info = torch.empty(T, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    cb = b.c_struct()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.adkf_thompson_pool_ard(C.byref(cb), p(phi), 0, p(X), rows, p(omega), p(phase), m, p(w), p(eps), S, p(excl), p(excl_off),
                                    p(paths), p(sel_idx), p(sel_val), p(info), p(ws_g), need, p(scratch), sb, stream)
    assert rc == 0
    gp_ops.check_info(info)
    assert bool((ws_g[need:] == 0x5a).all()) and bool((scratch[sb:] == 0x5a).all())
    assert bool((paths[T * S * rows:] == 12345.0).all())
    assert bool((sel_idx[T * S:] == 12345).all()) and bool((sel_val[T * S:] == 12345.0).all())
    P = paths[:T * S * rows].view(T, S, rows)
    si, sv = sel_idx[:T * S].view(T, S).cpu().numpy(), sel_val[:T * S].view(T, S).cpu().numpy()
    assert bool((P[1] == 0).all()) and (si[1] == -1).all() and np.isneginf(sv[1]).all()       # n_s = 0
    assert (si[2] == -1).all() and np.isneginf(sv[2]).all() and bool((P[2] != 0).any())       # every row excluded
    for t in (0, 2):
        n = n_s[t]
        ref = ard_paths_ref(Zs[t, :n].numpy(), ys[t, :n], phi[t].cpu().numpy(), 0, X.cpu().numpy(), omega.cpu(), phase.cpu(), w[t].cpu(),
                            eps[t].cpu())
        assert np.abs(P[t].cpu().numpy() - ref).max() <= TOL * max(1.0, np.abs(ref).max()), t
    for q in range(S):
        idx, val = select_ref(-P[0, q].cpu().numpy(), 1)
        assert si[0, q] == idx[0] and sv[0, q].view(np.int32) == val[0].view(np.int32)
    # an empty pool with the same exact buffers: -1 / -inf everywhere, nothing beyond the ends
    sel_idx.fill_(12345); sel_val.fill_(12345.0)
    rc = lib.adkf_thompson_pool_ard(C.byref(cb), p(phi), 0, None, 0, p(omega), p(phase), m, p(w), p(eps), S, None, None,
                                    None, p(sel_idx), p(sel_val), p(info), p(ws_g), need, p(scratch), sb, stream)
    assert rc == 0
    assert bool((sel_idx[:T * S] == -1).all()) and bool(torch.isneginf(sel_val[:T * S]).all())
    assert bool((sel_idx[T * S:] == 12345).all()) and bool((sel_val[T * S:] == 12345.0).all())
    assert bool((ws_g[need:] == 0x5a).all()) and bool((scratch[sb:] == 0x5a).all())


def test_the_gp_ops_surface(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d, S, m = 4, 16, 8, 4, 64
    Zs, ys, _ = _features(T, ns, [0] * T, d, 4, True)
    b = _batch(dev, Zs, ys, [16, 8, 12, 5], "rbf")
    phi = _spread_phi(dev, b, True, 4)
    omega, phase, w, eps = _basis_and_draws("rbf", T, S, m, ns, d, 15, dev)
    kw = dict(omega=omega, phase=phase, n_samples=S, w=w, eps=eps)
    X = _pool(5, d, 2).to(dev)
    out = gp_ops.thompson_pool_ard(b, phi, X, exclude=[[0, 1, 2, 3, 4], [], [2], None], want_paths=True, **kw)
    assert bool((out["sel_idx"][0] == -1).all()) and bool(torch.isneginf(out["sel_val"][0]).all())
    assert bool((out["sel_idx"][1:] >= 0).all()) and not bool((out["sel_idx"][2] == 2).any())
    out = gp_ops.thompson_pool_ard(b, phi, X[:0], want_paths=True, **kw)      # an empty pool
    assert out["paths"].shape == (T, S, 0) and bool((out["sel_idx"] == -1).all()) and bool(torch.isneginf(out["sel_val"]).all())
    # the draws the call makes itself come back, and reproduce it
    o1 = gp_ops.thompson_pool_ard(b, phi, X, omega=omega, phase=phase, n_samples=S, generator=torch.Generator().manual_seed(1))
    assert o1["w"].shape == (T, S, m) and o1["eps"].shape == (T, S, ns)
    o2 = gp_ops.thompson_pool_ard(b, phi, X, omega=omega, phase=phase, n_samples=S, w=o1["w"], eps=o1["eps"])
    assert torch.equal(o1["sel_idx"], o2["sel_idx"]) and torch.equal(o1["sel_val"], o2["sel_val"])
    b_iso = gp_ops.GPBatch(b.Z_s, b.y_s, b.priors, "rbf")
    with pytest.raises(ValueError):
        gp_ops.thompson_pool_ard(b_iso, torch.zeros(T, 3, device=dev), X, **kw)
    with pytest.raises(ValueError):
        gp_ops.thompson_pool_ard(b, phi, X[:, :4].contiguous(), **kw)
    with pytest.raises(ValueError):
        gp_ops.thompson_pool_ard(b, phi, X, omega=omega[:, :4].contiguous(), phase=phase, n_samples=S)
    with pytest.raises(ValueError):
        gp_ops.thompson_pool_ard(b, phi, X, omega=omega, phase=phase, n_samples=65)
    with pytest.raises(ValueError):
        gp_ops.thompson_pool_ard(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w[:, :2], eps=eps)
    with pytest.raises(RuntimeError):
        gp_ops.thompson_pool_ard(b, phi, X.cpu(), **kw)


def test_thompson_bo_loop_with_ard(dev):
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=2, num_bo_iters=3, kernel_type="matern", device=dev, init_from=5000, noise_init=0.01,
              noise_prior=True, n_features=256, ard=True)
    R = 3
    recs = BO.run_gp_ts_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(R)], **kw)
    again = BO.run_gp_ts_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(R)], **kw)
    assert recs == again, "two runs give equal records"
    assert len(recs) == R
    for r in range(R):
        assert len(recs[r]) == 1 + 3 * 2 and len(set(recs[r][1:])) == 6
        alone = BO.run_gp_ts_bo_batched(X, y, rngs=[np.random.default_rng(r)], **kw)
        assert alone[0] == recs[r], (r, "the batch couples replicates")
