"""GPU: Kriging-believer batch selection over a shared pool for ARD batches (adkf_believer_pool_ard / gp_ops.believer_pool_ard) -
every step's scores and pick against the float64 reference conditioned on the device's own earlier picks (believer_ref.py,
assertions 1-4, on the features over l at unit lengthscale) on every task kind, after an ARD fit, step 0 bit for bit against ARD
predict_pool, determinism and independence of the batch, more tasks than workgroups, guard bands, exclusions, the refusals in both
directions, and the batched BO loop with ard=True."""
import ctypes as C

import numpy as np
import pytest
import torch

import believer_ref as R
from test_believer_pool_ard_cpu import _bv_twin, ard_posterior, bv_call
from test_gpu_predict_marginal import _features, _path, _scalars
from test_gpu_predict_marginal_ard import _batch, _fit_ard, _isp, _spread_phi
from test_gpu_predict_pool import _pool

pytestmark = pytest.mark.gpu

ARD = 4
MAXIMIZE, LOG_EI = 2, 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


_problems = {}


def _explicit(dev, kernel, n_s, d, rows, seed):
    """A support-only ARD batch with phi GIVEN, not fitted: raw noise from -1 to -3 (noise >= 0.04), raw outputscale from 0.3 to 0,
    the median-heuristic lengthscale with a +-30 % spread per dimension (_spread_phi).  One per shape, shared by the tests and left
    unchanged: (b, phi, Zs, ys, n_s, X, best), X on the device."""
    key = (kernel, tuple(n_s), d, rows, seed)
    if key not in _problems:
        T, ns = len(n_s), max(n_s)
        Zs, ys, _ = _features(T, ns, [0] * T, d, seed, True)
        b = _batch(dev, Zs, ys, n_s, kernel)
        phi = _spread_phi(dev, b, True, seed)
        phi[:, 0] = torch.linspace(-1.0, -3.0, T, device=dev)
        phi[:, 1] = torch.linspace(0.3, 0.0, T, device=dev)
        X = _pool(rows, d, seed + 1)
        best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(T)])
        _problems[key] = (b, phi, Zs, ys, list(n_s), X.to(dev), best)
    return _problems[key]


def _check_device(out, b, phi, Zs, ys, n_s, X, best, flags, tag, lists=None):
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    si, sv, sm, sr, tr = (out[k].cpu().numpy() for k in ("sel_idx", "sel_val", "sel_mean", "sel_var", "trace"))
    Xh, ph = X.cpu().numpy(), phi.cpu().numpy()
    worst_all = 0.0
    for t in range(b.T):
        n = n_s[t]
        post = ard_posterior(Zs[t, :n].numpy(), ys[t, :n], Xh, ph[t], b.kernel)
        s0 = R.believer_ref(post, float(best[t]), flags & MAXIMIZE, [-1])[0][0]
        assert s0.max() >= 0.01, (tag, t, s0.max(), "EI must stay far from underflow")
        worst = R.check_task(post, float(best[t]), flags, si[t], sv[t], sm[t], sr[t], tr[t], excluded=lists[t] if lists else (), tag=(tag, t))
        print(f"{tag} task {t}: picks {si[t].tolist()[:8]}, step-0 max {s0.max():.3f}, worst trace error / bound {worst:.3f}")
        worst_all = max(worst_all, worst)
        got = [p for p in si[t].tolist() if p >= 0]
        assert len(set(got)) == len(got)
    print(f"{tag}: worst error / bound {worst_all:.3f}")
    return worst_all


def _check_twin(kernel_id, Zs, ys, n_s, X, phi, best, flags, q, tag):
    """The twin meets assertions 1-4 on this shape too (so that a miss of the device is the device's)."""
    from oracle import cpu_twin

    fn = _bv_twin()
    T = len(n_s)
    hb = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((T, 4), np.float32), kernel_id, n_s=np.array(n_s, np.int32))
    hb.c.flags = ARD
    Xh, ph, bh = X.cpu().numpy(), np.ascontiguousarray(phi.cpu().numpy()), np.ascontiguousarray(best.numpy(), np.float32)
    si, sv, sm, sr, tr, _ = bv_call(fn, hb, ph, flags, np.ascontiguousarray(Xh), bh, q)
    for t in range(T):
        post = ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], Xh, ph[t], kernel_id)
        R.check_task(post, float(best[t]), flags, si[t], sv[t], sm[t], sr[t], tr[t], tag=(tag, "twin", t))


CASES = [  # (kernel, n_s, d, rows, q)
    ("rbf", [5, 4, 3], 6, 37, 5),                 # d no multiple of 4 (the unvectorised il loads), fewer rows than one tile
    ("matern", [48, 45, 31], 16, 300, 8),         # one panel, a partial last tile
    ("rbf", [128, 125, 85], 12, 130, 5),          # two support panels
    ("matern", [200, 197, 133], 12, 333, 8),      # refined, tiles in LDS
    ("matern", [300, 263, 200], 12, 130, 4),      # refined, global slots beside the ARD region
    ("rbf", [32, 29, 21], 8, 200, 64),            # the full pick panel
]


@pytest.mark.parametrize("kernel,n_s,d,rows,q", CASES)
def test_against_the_reference(dev, kernel, n_s, d, rows, q):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, best = _explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    if max(n_s) >= 200:
        _check_twin(b.kernel, Zs, ys, n_s, X, phi, best, 0, q, (kernel, max(n_s)))
    modes = ((0, False, False), (MAXIMIZE, True, False), (LOG_EI, False, True)) if max(n_s) <= 200 else ((0, False, False),)
    for flags, maximize, log_ei in modes:
        bf = best if not maximize else best - 0.5
        out = gp_ops.believer_pool_ard(b, phi, X, best_f=bf.to(dev), q=q, maximize=maximize, log_ei=log_ei, want_trace=True)
        _check_device(out, b, phi, Zs, ys, n_s, X, bf, flags, (kernel, max(n_s), flags))
        assert bool((out["sel_idx"] >= 0).all()) or rows < q


@pytest.mark.parametrize("kernel,ns,d", [("matern", 16, 12), ("rbf", 64, 64)])
def test_after_an_ard_fit(dev, kernel, ns, d):
    """The fit's state through REUSE_INNER; the fitted noise can fall below 0.04.  best starts at the median of y_s; a task whose
    float64 step-0 maximum at the device's fitted phi is below 0.01 gets its best raised by 0.5 until it is not (an input replaced,
    not a bound loosened); what was used is printed.  On the MI355X the fitted noise was 0.010 on every task of both cases, the
    step-0 maxima were 0.78 - 1.11 and no best had to be raised: the medians were used."""
    from adkf_ift_amd import gp_ops

    T, rows, q = 3, 333, 6
    n_s = [ns, max(2, ns - 3), max(2, (2 * ns) // 3)]
    Zs, ys, _ = _features(T, ns, [0] * T, d, 300 + ns + d, True)
    b, phi = _fit_ard(dev, Zs, ys, n_s, kernel, True)
    X = _pool(rows, d, 9).to(dev)
    Xh, ph = X.cpu().numpy(), phi.cpu().numpy()
    best = [float(ys[t, :n_s[t]].median()) for t in range(T)]
    for t in range(T):
        post = ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], Xh, ph[t], b.kernel)
        for _ in range(8):
            if R.believer_ref(post, best[t], 0, [-1])[0][0].max() >= 0.01:
                break
            best[t] += 0.5
        noise = float(np.logaddexp(0.0, float(ph[t, 0]))) + 1e-4
        print(f"fit {kernel} ns {ns} task {t}: noise {noise:.3e}, best used {best[t]:.4f} (median {float(ys[t, :n_s[t]].median()):.4f})")
    best = torch.tensor(best)
    b.flags = gp_ops.REUSE_INNER
    out = gp_ops.believer_pool_ard(b, phi, X, best_f=best.to(dev), q=q, want_trace=True)
    _check_device(out, b, phi, Zs, ys, n_s, X, best, 0, (kernel, ns, d, "fit"))


def _f64_batch(dev):
    """The recipe of test_gpu_predict_marginal_ard.test_float64_path, and the pool: 300 rows plus five support rows of task 1."""
    from adkf_ift_amd.synthetic import make_tasks

    tasks = make_tasks(3, 16, 2, N_q=64, regression=True, first_task=1800)
    Zs, _ = tasks.features()
    n_s = [16, 15, 16]
    b = _batch(dev, Zs, tasks.y_s, n_s, "rbf")
    b.priors.copy_(torch.tensor([[0.0, -1.0, 0.0, -1.0]] * 3))
    phi = torch.tensor([[-9.0, 0.0, _isp(2.0), _isp(3.0)]] * 3, dtype=torch.float32, device=dev)
    X = torch.cat([_pool(300, 2, 3), Zs[1, :5]]).to(dev)
    best = torch.tensor([float(tasks.y_s[t, :n_s[t]].median()) for t in range(3)])
    return b, phi, Zs, tasks.y_s, n_s, X, best


def test_float64_path(dev):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, best = _f64_batch(dev)
    for flags, log_ei in ((0, False), (LOG_EI, True)):
        out = gp_ops.believer_pool_ard(b, phi, X, best_f=best.to(dev), q=6, log_ei=log_ei, want_trace=True)
        torch.cuda.synchronize()
        sc = _scalars(b)
        assert all(_path(sc[t]) == 2 for t in range(3)), [float(sc[t][45]) for t in range(3)]
        _check_device(out, b, phi, Zs, ys, n_s, X, best, flags, ("float64", flags))


def test_mixed_kinds_in_one_call(dev):
    """Task 1 at the float64 recipe, phi = (-9, 0, isp(2), isp(3)); tasks 0, 2 and 3 at phi = (-1, the raw outputscale of
    init_params_batch, the median-heuristic lengthscale in both dimensions): both kernels of the walk in one call, asserted from
    the scalars as test_gpu_predict_pool._ill_batch does.  The phi used, as the MI355X gave it: task 0 (-1, 0, 1.0588, 1.0588),
    task 1 (-9, 0, 1.8546, 2.9489), task 2 (-1, 0, -0.3408, -0.3408), task 3 (-1, 0, -0.2231, -0.2231); kinds [0, 2, 0, 0]."""
    from adkf_ift_amd import gp_ops
    from adkf_ift_amd.synthetic import make_tasks

    tasks = make_tasks(4, 16, 2, N_q=64, regression=True, first_task=1800)
    Zs, _ = tasks.features()
    n_s = [16, 15, 5, 3]
    b = _batch(dev, Zs, tasks.y_s, n_s, "rbf")
    phi, _ = gp_ops.init_params_batch(b, True, True)
    b.priors.copy_(torch.tensor([[0.0, -1.0, 0.0, -1.0]] * 4))
    phi = phi.clone()
    phi[:, 0] = -1.0
    phi[1] = torch.tensor([-9.0, 0.0, _isp(2.0), _isp(3.0)], device=dev)
    X = torch.cat([_pool(300, 2, 3), Zs[1, :5]]).to(dev)
    best = torch.tensor([float(tasks.y_s[t, :n_s[t]].median()) for t in range(4)])
    out = gp_ops.believer_pool_ard(b, phi, X, best_f=best.to(dev), q=6, want_trace=True)
    torch.cuda.synchronize()
    kinds = [_path(sc) for sc in _scalars(b)]
    print("kinds of the mixed ARD batch:", kinds, "phi", phi.cpu().tolist())
    assert kinds[1] == 2 and min(kinds) < 2, kinds
    _check_device(out, b, phi, Zs, tasks.y_s, n_s, X, best, 0, "mixed")


def _step0_equals_predict_pool(b, phi, X, best, tag):
    from adkf_ift_amd import gp_ops

    for flags in (0, gp_ops.REUSE_INNER):   # REUSE_INNER: the state the evaluation before it left
        b.flags = flags
        for log_ei in (False, True):
            ref = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, topk=1, want_ei=True, log_ei=log_ei)
            out = gp_ops.believer_pool_ard(b, phi, X, best_f=best, q=3, log_ei=log_ei, want_trace=True)
            assert torch.equal(out["sel_idx"][:, 0], ref["top_idx"][:, 0]), (tag, flags, log_ei)
            assert torch.equal(out["sel_val"][:, 0], ref["top_val"][:, 0]), (tag, flags, log_ei)
            assert torch.equal(out["trace"][:, 0], ref["ei"]), (tag, flags, log_ei)
            assert bool((ref["ei"] != 0).any())
    b.flags = 0


def test_step_0_is_predict_pool_bit_for_bit(dev):
    for kernel, n_s, d, rows, q in (CASES[1], CASES[3]):          # plain; refined
        b, phi, Zs, ys, n_s, X, best = _explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
        _step0_equals_predict_pool(b, phi, X, best.to(dev), (kernel, max(n_s)))
    b, phi, Zs, ys, n_s, X, best = _f64_batch(dev)                 # float64
    _step0_equals_predict_pool(b, phi, X, torch.tensor([0.1, -0.2, 0.3], device=dev), "float64")


def test_deterministic_and_independent_of_the_batch(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, q = CASES[1]
    b, phi, Zs, ys, n_s, X, best = _explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    lists = [[0, 7], [], [3]]
    kw = dict(q=q, exclude=lists, want_trace=True)
    first = gp_ops.believer_pool_ard(b, phi, X, best_f=best.to(dev), **kw)
    again = gp_ops.believer_pool_ard(b, phi, X, best_f=best.to(dev), **kw)
    names = ("sel_idx", "sel_val", "sel_mean", "sel_var", "trace")
    for name in names:
        assert torch.equal(first[name], again[name]), name
    none = gp_ops.believer_pool_ard(b, phi, X, best_f=best.to(dev), q=q, exclude=lists)      # trace == NULL: the same bits
    assert none["trace"] is None
    for name in names[:4]:
        assert torch.equal(first[name], none[name]), name
    for t in range(b.T):   # each task alone in a T = 1 batch
        b1 = _batch(dev, Zs[t:t + 1].contiguous(), ys[t:t + 1].contiguous(), [n_s[t]], kernel)
        b1.priors.copy_(b.priors[t:t + 1])
        o1 = gp_ops.believer_pool_ard(b1, phi[t:t + 1].contiguous(), X, best_f=best[t:t + 1].to(dev), q=q, exclude=[lists[t]], want_trace=True)
        for name in names:
            assert torch.equal(o1[name][0], first[name][t]), (t, name)


def test_more_tasks_than_workgroups(dev):
    """T = 300 tiny tasks: assertions 2-4 hold on every task (no whole pick sequence is compared)."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, q = 300, 8, 4, 130, 3
    g = torch.Generator().manual_seed(77)
    Zs, ys, _ = _features(T, ns, [0] * T, d, 77, True)
    n_s = [int(x) for x in torch.randint(3, ns + 1, (T,), generator=g)]
    n_s[0] = ns
    b = _batch(dev, Zs, ys, n_s, "matern")
    phi = _spread_phi(dev, b, True, 77)
    phi[:, 0] = torch.linspace(-1.0, -3.0, T, device=dev)
    phi[:, 1] = 0.3
    X = _pool(rows, d, 78)
    best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(T)])
    out = gp_ops.believer_pool_ard(b, phi, X.to(dev), best_f=best.to(dev), q=q)
    gp_ops.check_info(out["info"])
    si, sv, sm, sr = (out[k].cpu().numpy() for k in ("sel_idx", "sel_val", "sel_mean", "sel_var"))
    ph = phi.cpu().numpy()
    for t in range(T):
        post = ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], X.numpy(), ph[t], b.kernel)
        R.check_task(post, float(best[t]), 0, si[t], sv[t], sm[t], sr[t], None, tag=("T300", t))
        assert len(set(si[t].tolist())) == q and (si[t] >= 0).all()


def test_guard_bands(dev):
    from adkf_ift_amd import _lib, gp_ops

    kernel, n_s, d, rows, q = CASES[1]
    b, phi, Zs, ys, n_s, X, best = _explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    T, ns = b.T, b.ns
    lib = _lib.load()
    need = lib.adkf_workspace_bytes_ard(T, ns, 0, d)
    assert b.workspace()[1] == need
    sb = lib.adkf_believer_pool_scratch_bytes(T, ns, d, q)
    guard = 4096
    ws_g = torch.full((need + guard,), 0x5a, dtype=torch.uint8, device=dev)
    scratch = torch.full((sb + guard,), 0x5a, dtype=torch.uint8, device=dev)
    trace = torch.full((T * q * rows + guard,), 12345.0, device=dev)
    sel_idx = torch.full((T * q + guard,), 12345, dtype=torch.int64, device=dev)
    sel = [torch.full((T * q + guard,), 12345.0, device=dev) for _ in range(3)]
    info = torch.empty(T, dtype=torch.int32, device=dev)
    bf = best.to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    cb = b.c_struct()
    skipped = torch.tensor([n_s[0], 0, n_s[2]], dtype=torch.int32, device=dev)   # task 1: skipped
    cb.n_s = skipped.data_ptr()
    cb.flags = ARD
    rc = lib.adkf_believer_pool_ard(C.byref(cb), p(phi), 0, p(X), rows, p(bf), None, None, q, p(trace), p(sel_idx), p(sel[0]), p(sel[1]),
                                    p(sel[2]), p(info), p(ws_g), need, p(scratch), sb, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    gp_ops.check_info(info)
    assert bool((ws_g[need:] == 0x5a).all()) and bool((scratch[sb:] == 0x5a).all())
    assert bool((trace[T * q * rows:] == 12345.0).all()) and bool((sel_idx[T * q:] == 12345).all())
    assert all(bool((s[T * q:] == 12345.0).all()) for s in sel)
    si = sel_idx[:T * q].view(T, q)
    tr = trace[:T * q * rows].view(T, q, rows)
    assert bool((si[1] == -1).all()) and bool(torch.isneginf(sel[0][:T * q].view(T, q)[1]).all()) and bool((tr[1] == 0).all())
    assert bool((sel[1][:T * q].view(T, q)[1] == 0).all()) and bool((sel[2][:T * q].view(T, q)[1] == 0).all())
    # the other tasks do not see the skipped one
    full = gp_ops.believer_pool_ard(b, phi, X, best_f=bf, q=q, want_trace=True)
    for t in (0, 2):
        assert torch.equal(si[t], full["sel_idx"][t]) and torch.equal(tr[t], full["trace"][t])
        for k, name in enumerate(("sel_val", "sel_mean", "sel_var")):
            assert torch.equal(sel[k][:T * q].view(T, q)[t], full[name][t]), (t, name)


def test_exclusions_and_small_pools(dev):
    from adkf_ift_amd import gp_ops

    T, d, rows = 3, 16, 6000
    b, phi, Zs, ys, n_s, _, best = _explicit(dev, "matern", [48, 45, 31], d, 300, 548)
    X = _pool(rows, d, 5).to(dev)
    bf = best.to(dev)
    free = gp_ops.believer_pool_ard(b, phi, X, best_f=bf, q=4)
    keep = sorted(set(range(0, rows, 7)) | set(free["sel_idx"][0].tolist()))
    lists = [[i for i in range(rows) if i not in keep][:5000] + free["sel_idx"][0].tolist(), [], free["sel_idx"][2, :1].tolist()]
    assert len(lists[0]) > 5000
    out = gp_ops.believer_pool_ard(b, phi, X, best_f=bf, q=4, exclude=lists)
    for t in range(T):
        got = out["sel_idx"][t].tolist()
        assert len(set(got)) == 4 and min(got) >= 0 and not set(got) & set(lists[t]), t
    assert torch.equal(out["sel_idx"][1], free["sel_idx"][1]) and out["sel_idx"][2, 0] != free["sel_idx"][2, 0]
    # a pool of 9 rows with q = 16: nine picks, then the -1 / -inf tail; an empty pool: the tail only
    out = gp_ops.believer_pool_ard(b, phi, X[:9], best_f=bf, q=16, want_trace=True)
    si = out["sel_idx"].cpu()
    for t in range(T):
        assert sorted(si[t, :9].tolist()) == list(range(9)) and bool((si[t, 9:] == -1).all())
    assert bool(torch.isneginf(out["sel_val"][:, 9:]).all()) and bool((out["sel_mean"][:, 9:] == 0).all()) and bool((out["sel_var"][:, 9:] == 0).all())
    out = gp_ops.believer_pool_ard(b, phi, X[:0], best_f=bf, q=3, want_trace=True)
    assert bool((out["sel_idx"] == -1).all()) and bool(torch.isneginf(out["sel_val"]).all()) and out["trace"].shape == (T, 3, 0)
    with pytest.raises(ValueError):
        gp_ops.believer_pool_ard(b, phi, X[:, :4].contiguous(), best_f=bf, q=3)
    with pytest.raises(ValueError):
        gp_ops.believer_pool_ard(b, phi, X, best_f=bf[:2], q=3)
    with pytest.raises(RuntimeError):
        gp_ops.believer_pool_ard(b, phi, X.cpu(), best_f=bf, q=3)


def test_each_entry_refuses_the_other_kind_of_batch(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, q = CASES[0]
    b, phi, Zs, ys, n_s, X, best = _explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    with pytest.raises(ValueError, match="ARD"):
        gp_ops.believer_pool(b, phi, X, best_f=best.to(dev), q=2)
    iso = gp_ops.GPBatch(b.Z_s, b.y_s, b.priors, kernel, n_s=torch.tensor(n_s, dtype=torch.int32))
    with pytest.raises(ValueError, match="ARD"):
        gp_ops.believer_pool_ard(iso, phi[:, :3].contiguous(), X, best_f=best.to(dev), q=2)


def test_bo_loop(dev):
    """The toy problem of test_gpu_believer_pool.test_bo_loop with ard=True.  query_batch_size = 1: batch="believer" is
    batch="topk" (step 0 is predict_pool).  query_batch_size = 4: records of the right length without repeats.  ard=False is the
    call without the argument."""
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(5)
    X = torch.randn(200, 8, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, num_bo_iters=3, kernel_type="matern", device=dev, init_from=100, noise_init=0.01, noise_prior=True)
    rngs = lambda: [np.random.default_rng(s) for s in range(2)]
    one = BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=1, batch="believer", ard=True, **kw)
    assert one == BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=1, batch="topk", ard=True, **kw)
    four = BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=4, batch="believer", ard=True, **kw)
    assert len(four) == 2
    for rec in four:
        assert len(rec) == 1 + 3 * 4 and len(set(rec[1:])) == 12
    for batch in ("topk", "believer"):
        assert (BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=2, batch=batch, ard=False, **kw)
                == BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=2, batch=batch, **kw))
