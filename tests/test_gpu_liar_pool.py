"""GPU: constant-liar and label-replay batches over a shared pool (adkf_liar_pool / gp_ops.liar_pool) - every step's scores, pick,
conditioned mean and variance against the float64 reference that REBUILDS the posterior with the device's own earlier picks appended
(liar_ref.py: no recursion), on every task kind, isotropic and ARD; sel_lie and inc exactly by the rule; step 0 bit for bit against
predict_pool; a lie of NaN bit for bit against adkf_believer_pool; a shared label table against its repeated copy; determinism and
independence of the batch; more tasks than workgroups; exclusions and small pools; guard bands; and the BO loop's refit_every.

Worst error / bound per case as measured on the MI355X: the table in DESIGN.md ("The constant liar and label replay")."""
import ctypes as C

import numpy as np
import pytest
import torch

import liar_ref as R
import test_gpu_believer_pool as B
import test_gpu_believer_pool_ard as BA
import test_gpu_predict_marginal as M
import test_gpu_predict_pool as P
from test_liar_pool_cpu import _liar_twin, liar_call

pytestmark = pytest.mark.gpu

MAXIMIZE, LOG_EI = 2, 16
NAMES = ("sel_idx", "sel_val", "sel_mean", "sel_var", "sel_lie", "inc", "trace")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _pool_labels(X, seed):
    """Pool labels by the rule of the support labels (test_gpu_predict_marginal._features): sin(sum of 4 features) + 0.1 noise."""
    g = torch.Generator().manual_seed(seed)
    Xc = X.cpu()
    return (torch.sin(Xc[:, : min(Xc.shape[1], 4)].sum(-1)) + 0.1 * torch.randn(Xc.shape[0], generator=g)).float()


def _lie_of(mode, ys, n_s):
    f = {"min": torch.min, "max": torch.max, "mean": torch.mean}[mode]
    return torch.tensor([float(f(ys[t, :n_s[t]])) for t in range(len(n_s))])


def _check_device(out, b, phi, Zs, ys, n_s, X, best, flags, tag, lie=None, labels=None, lists=None, ard=False):
    """liar_ref.check_task on every task; lie [T] / labels [rows] or [T, rows] on the host.  Prints the worst error / bound."""
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    o = [out[k].cpu().numpy() if out[k] is not None else None for k in NAMES]
    Xh, ph = X.cpu().numpy(), phi.cpu().numpy()
    worst = l1 = 0.0
    for t in range(b.T):
        n = n_s[t]
        task = R.isotropic(Zs[t, :n].numpy(), ys[t, :n].numpy(), Xh, ph[t], ard)
        lab = None if labels is None else (labels[t] if labels.dim() == 2 else labels).numpy()
        w, l = R.check_task(task, b.kernel, float(best[t]), flags, tuple(a[t] for a in o[:6]) + (None if o[6] is None else o[6][t],),
                            lie=None if lie is None else float(lie[t]), labels=lab, excluded=lists[t] if lists else (), tag=(tag, t))
        worst, l1 = max(worst, w), max(l1, l)
        got = [p for p in o[0][t].tolist() if p >= 0]
        assert len(set(got)) == len(got)
    print(f"{tag}: worst error / bound {worst:.3f}, largest os * ||beta||_1 {l1:.2f}")
    return worst


def _modes(q, ns):
    """(flags, what): replay and the lie max only up to q = 8 (liar_ref.L1_CAP); the large case one mode."""
    if ns > 200:
        return ((0, "replay"),)
    if q > 8:
        return ((0, "mean"), (LOG_EI, "min"))
    return ((0, "min"), (MAXIMIZE, "max"), (LOG_EI, "replay"), (0, "mean"))


def _run(dev, b, phi, X, bf, q, flags, what, ys, n_s, **kw):
    from adkf_ift_amd import gp_ops

    lie = labels = None
    if what == "replay":
        labels = _pool_labels(X, 9)
    else:
        lie = _lie_of(what, ys, n_s)
    out = gp_ops.liar_pool(b, phi, X, best_f=bf.to(dev), q=q, lie=None if lie is None else lie.to(dev),
                           labels=None if labels is None else labels.to(dev), maximize=bool(flags & MAXIMIZE), log_ei=bool(flags & LOG_EI),
                           want_trace=True, **kw)
    return out, lie, labels


@pytest.mark.parametrize("kernel,n_s,d,rows,q,twin", B.CASES)
def test_against_the_reference(dev, kernel, n_s, d, rows, q, twin):
    b, phi, Zs, ys, n_s, X, best = B._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    if twin:   # the twin meets the same assertions on this shape (so that a miss of the device is the device's)
        from oracle import cpu_twin

        lab = _pool_labels(X, 9).numpy()
        hb = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((b.T, 4), np.float32), b.kernel, n_s=np.array(n_s, np.int32))
        Xh, ph = np.ascontiguousarray(X.cpu().numpy()), np.ascontiguousarray(phi.cpu().numpy())
        o = liar_call(_liar_twin(), hb, ph, 0, Xh, np.ascontiguousarray(best.numpy(), np.float32), q, labels=lab)
        for t in range(b.T):
            task = R.isotropic(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]].numpy(), Xh, ph[t], False)
            R.check_task(task, b.kernel, float(best[t]), 0, tuple(a[t] for a in o), labels=lab, tag=(kernel, "twin", t))
    for flags, what in _modes(q, max(n_s)):
        bf = best if not flags & MAXIMIZE else best - 0.5
        out, lie, labels = _run(dev, b, phi, X, bf, q, flags, what, ys, n_s)
        _check_device(out, b, phi, Zs, ys, n_s, X, bf, flags, (kernel, max(n_s), q, flags, what), lie=lie, labels=labels)
        assert bool((out["sel_idx"] >= 0).all()) or rows < q


def test_ard_against_the_reference(dev):
    for case in (BA.CASES[1], BA.CASES[3]):   # plain, a partial last tile; refined
        kernel, n_s, d, rows, q = case
        b, phi, Zs, ys, n_s, X, best = BA._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
        for flags, what in ((0, "min"), (LOG_EI, "replay")):
            out, lie, labels = _run(dev, b, phi, X, best, q, flags, what, ys, n_s)
            _check_device(out, b, phi, Zs, ys, n_s, X, best, flags, ("ard", kernel, max(n_s), flags, what), lie=lie, labels=labels, ard=True)


_ill_problem = []


def _ill(dev):
    """test_gpu_predict_pool._ill_batch with a pool and incumbents, fitted once and shared; the batch reuses the fit's state."""
    from adkf_ift_amd import gp_ops

    if not _ill_problem:
        b, phi, Zs, ys, n_s, _ = P._ill_batch(dev)
        b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
        X = torch.cat([P._pool(300, 2, 3), b.Z_s[1, :5].cpu()]).to(dev)
        best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(4)])
        _ill_problem.append((b, phi, Zs, ys, n_s, X, best))
    return _ill_problem[0]


def test_mixed_kinds_with_labels(dev):
    """test_gpu_predict_pool._ill_batch: task 1 takes the float64 walk and keeps z in float64.  The label table [T, rows] holds, per
    task, a draw around the task's own float64 posterior - m_0 + 0.1 sd N(0, 1), sd the noisy predictive deviation - so that the
    observations are ones the fitted model finds plausible: the fitted noise is small (0.01 on task 1), beta grows with 1 / noise,
    and os * ||beta||_1, which is linear in the residuals, was 115 from the reference at 0.5 sd - above liar_ref.L1_CAP."""
    from adkf_ift_amd import gp_ops
    from believer_ref import posterior

    b, phi, Zs, ys, n_s, X, best = _ill(dev)
    g = torch.Generator().manual_seed(4)
    Xh, ph = X.cpu().numpy(), phi.cpu().numpy()
    labels = torch.empty(b.T, X.shape[0])
    for t in range(b.T):
        m0, S0, noise, _ = posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]].numpy(), Xh, ph[t], b.kernel)
        labels[t] = torch.from_numpy(m0 + 0.1 * np.sqrt(S0.diagonal() + noise) * torch.randn(X.shape[0], generator=g).numpy()).float()
    out = gp_ops.liar_pool(b, phi, X, best_f=best.to(dev), q=6, labels=labels.to(dev), want_trace=True)
    _check_device(out, b, phi, Zs, ys, n_s, X, best, 0, "mixed", labels=labels)


def test_step_0_is_predict_pool_bit_for_bit(dev):
    from adkf_ift_amd import gp_ops

    probs = [B._explicit(dev, k, n, d, r, 500 + max(n)) for k, n, d, r, _, _ in (B.CASES[0], B.CASES[2])]
    probs.append(_ill(dev))
    for b, phi, Zs, ys, n_s, X, best in probs:
        bf, lab = best.to(dev), _pool_labels(X, 9).to(dev)
        for log_ei in (False, True):
            ref = gp_ops.predict_pool(b, phi, X, latent=True, best_f=bf, topk=1, want_ei=True, log_ei=log_ei)
            out = gp_ops.liar_pool(b, phi, X, best_f=bf, q=3, labels=lab, log_ei=log_ei, want_trace=True)
            assert torch.equal(out["sel_idx"][:, 0], ref["top_idx"][:, 0]) and torch.equal(out["sel_val"][:, 0], ref["top_val"][:, 0])
            assert torch.equal(out["trace"][:, 0], ref["ei"]) and bool((ref["ei"] != 0).any())
            assert torch.equal(out["inc"][:, 0], bf)


def test_a_lie_of_nan_is_the_believer_bit_for_bit(dev):
    from adkf_ift_amd import gp_ops

    def same(b, phi, X, bf, q, believe):
        nan = torch.full((b.T,), float("nan"), device=dev)
        for log_ei in (False, True):
            ref = believe(b, phi, X, best_f=bf, q=q, log_ei=log_ei, want_trace=True)
            out = gp_ops.liar_pool(b, phi, X, best_f=bf, q=q, lie=nan, log_ei=log_ei, want_trace=True)
            for name in ("sel_idx", "sel_val", "sel_mean", "sel_var", "trace"):
                assert torch.equal(out[name], ref[name]), (name, log_ei)
            assert torch.equal(out["sel_lie"], out["sel_mean"])
            assert bool((out["sel_idx"] >= 0).all())

    kernel, n_s, d, rows, q, _ = B.CASES[2]
    b, phi, Zs, ys, n_s, X, best = B._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    same(b, phi, X, best.to(dev), q, gp_ops.believer_pool)
    kernel, n_s, d, rows, q = BA.CASES[1]
    b, phi, Zs, ys, n_s, X, best = BA._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    same(b, phi, X, best.to(dev), q, gp_ops.believer_pool_ard)
    b, phi, Zs, ys, n_s, X, best = _ill(dev)
    same(b, phi, X, best.to(dev), 6, gp_ops.believer_pool)


def test_deterministic_shared_table_and_independent_of_the_batch(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, q, _ = B.CASES[0]
    b, phi, Zs, ys, n_s, X, best = B._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    lists = [[0, 7], [], [3]]
    lab = _pool_labels(X, 9).to(dev)
    lie = _lie_of("min", ys, n_s).to(dev)
    kw = dict(q=q, exclude=lists, want_trace=True, log_ei=True)
    first = gp_ops.liar_pool(b, phi, X, best_f=best.to(dev), labels=lab, **kw)
    again = gp_ops.liar_pool(b, phi, X, best_f=best.to(dev), labels=lab, **kw)
    tiled = gp_ops.liar_pool(b, phi, X, best_f=best.to(dev), labels=lab[None].repeat(b.T, 1).contiguous(), **kw)
    for name in NAMES:
        assert torch.equal(first[name], again[name]), name
        assert torch.equal(first[name], tiled[name]), name
    none = gp_ops.liar_pool(b, phi, X, best_f=best.to(dev), labels=lab, q=q, exclude=lists, log_ei=True)   # trace == NULL: the same bits
    assert none["trace"] is None
    for name in NAMES[:6]:
        assert torch.equal(first[name], none[name]), name
    holes = lab.clone()
    holes[::2] = float("nan")
    mixed = gp_ops.liar_pool(b, phi, X, best_f=best.to(dev), labels=holes, lie=lie, **kw)
    for t in range(b.T):   # each task alone in a T = 1 batch
        b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), kernel,
                            n_s=torch.tensor([n_s[t]], dtype=torch.int32))
        o1 = gp_ops.liar_pool(b1, phi[t:t + 1].contiguous(), X, best_f=best[t:t + 1].to(dev), labels=holes, lie=lie[t:t + 1], q=q,
                              exclude=[lists[t]], want_trace=True, log_ei=True)
        for name in NAMES:
            assert torch.equal(o1[name][0], mixed[name][t]), (t, name)
    # lie="min" is the tensor of the tasks' own smallest support labels
    named = gp_ops.liar_pool(b, phi, X, best_f=best.to(dev), lie="min", q=q)
    given = gp_ops.liar_pool(b, phi, X, best_f=best.to(dev), lie=lie, q=q)
    assert torch.equal(named["sel_idx"], given["sel_idx"]) and torch.equal(named["sel_lie"], given["sel_lie"])
    assert torch.equal(given["sel_lie"], lie[:, None].expand(-1, q))


def test_more_tasks_than_workgroups(dev):
    """T = 300 tiny tasks replaying one label table: the reference's assertions hold on every task, sel_lie and inc by the rule."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, q = 300, 8, 4, 130, 3
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
    best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(T)])
    labels = _pool_labels(X, 9)
    out = gp_ops.liar_pool(b, phi, X, best_f=best.to(dev), q=q, labels=labels.to(dev))
    _check_device(out, b, phi, Zs, ys, n_s, X, best, 0, "T300", labels=labels)
    assert bool((out["sel_idx"] >= 0).all())


def test_exclusions_and_small_pools(dev):
    from adkf_ift_amd import gp_ops

    T, d, rows = 3, 16, 6000
    b, phi, Zs, ys, n_s, _, best = B._explicit(dev, "matern", [48, 45, 31], d, 300, 548)
    X = P._pool(rows, d, 5).to(dev)
    bf, lab = best.to(dev), _pool_labels(X, 9).to(dev)
    free = gp_ops.liar_pool(b, phi, X, best_f=bf, q=4, labels=lab)
    keep = sorted(set(range(0, rows, 7)) | set(free["sel_idx"][0].tolist()))
    lists = [[i for i in range(rows) if i not in keep][:5000] + free["sel_idx"][0].tolist(), [], free["sel_idx"][2, :1].tolist()]
    out = gp_ops.liar_pool(b, phi, X, best_f=bf, q=4, labels=lab, exclude=lists)
    for t in range(T):
        got = out["sel_idx"][t].tolist()
        assert len(set(got)) == 4 and min(got) >= 0 and not set(got) & set(lists[t]), t
        assert torch.equal(out["sel_lie"][t], lab[out["sel_idx"][t]])
    assert torch.equal(out["sel_idx"][1], free["sel_idx"][1]) and out["sel_idx"][2, 0] != free["sel_idx"][2, 0]
    # a pool of 9 rows with q = 16: nine picks, then the -1 / -inf tail with 0 in sel_lie and the incumbent repeated
    out = gp_ops.liar_pool(b, phi, X[:9], best_f=bf, q=16, labels=lab[:9], want_trace=True)
    si = out["sel_idx"].cpu()
    for t in range(T):
        assert sorted(si[t, :9].tolist()) == list(range(9)) and bool((si[t, 9:] == -1).all())
        assert bool((out["inc"][t, 9:] == torch.minimum(bf[t], lab[:9].min())).all())
    assert bool(torch.isneginf(out["sel_val"][:, 9:]).all()) and bool((out["sel_mean"][:, 9:] == 0).all()) and bool((out["sel_var"][:, 9:] == 0).all())
    assert bool((out["sel_lie"][:, 9:] == 0).all())
    out = gp_ops.liar_pool(b, phi, X[:0], best_f=bf, q=3, lie="mean", want_trace=True)
    assert bool((out["sel_idx"] == -1).all()) and bool(torch.isneginf(out["sel_val"]).all()) and out["trace"].shape == (T, 3, 0)
    assert torch.equal(out["inc"], bf[:, None].expand(-1, 4)) and bool((out["sel_lie"] == 0).all())
    with pytest.raises(ValueError):
        gp_ops.liar_pool(b, phi, X, best_f=bf, q=3)                                   # neither lie nor labels
    with pytest.raises(ValueError):
        gp_ops.liar_pool(b, phi, X, best_f=bf, q=3, lie="median")
    with pytest.raises(ValueError):
        gp_ops.liar_pool(b, phi, X, best_f=bf, q=3, labels=lab[:-1])
    with pytest.raises(ValueError):
        gp_ops.liar_pool(b, phi, X, best_f=bf, q=3, lie=bf[:2])
    with pytest.raises(RuntimeError):
        gp_ops.liar_pool(b, phi, X, best_f=bf, q=3, labels=lab.cpu())


def test_guard_bands(dev):
    from adkf_ift_amd import _lib, gp_ops

    kernel, n_s, d, rows, q, _ = B.CASES[0]
    b, phi, Zs, ys, n_s, X, best = B._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    T, ns = b.T, b.ns
    lib = _lib.load()
    need = lib.adkf_workspace_bytes(T, ns, 0, d)
    sb = lib.adkf_liar_pool_scratch_bytes(T, ns, d, q)
    guard = 4096
    ws_g = torch.full((need + guard,), 0x5a, dtype=torch.uint8, device=dev)
    scratch = torch.full((sb + guard,), 0x5a, dtype=torch.uint8, device=dev)
    trace = torch.full((T * q * rows + guard,), 12345.0, device=dev)
    sel_idx = torch.full((T * q + guard,), 12345, dtype=torch.int64, device=dev)
    sel = [torch.full((T * q + guard,), 12345.0, device=dev) for _ in range(4)]
    inc = torch.full((T * (q + 1) + guard,), 12345.0, device=dev)
    info = torch.empty(T, dtype=torch.int32, device=dev)
    bf, lab = best.to(dev), _pool_labels(X, 9).to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    cb = b.c_struct()
    skipped = torch.tensor([n_s[0], 0, n_s[2]], dtype=torch.int32, device=dev)   # task 1: skipped
    cb.n_s = skipped.data_ptr()
    cb.flags = 0
    rc = lib.adkf_liar_pool(C.byref(cb), p(phi), 0, p(X), rows, p(bf), None, p(lab), 0, None, None, q, p(trace), p(sel_idx), p(sel[0]), p(sel[1]),
                            p(sel[2]), p(sel[3]), p(inc), p(info), p(ws_g), need, p(scratch), sb,
                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    gp_ops.check_info(info)
    assert bool((ws_g[need:] == 0x5a).all()) and bool((scratch[sb:] == 0x5a).all())
    assert bool((trace[T * q * rows:] == 12345.0).all()) and bool((sel_idx[T * q:] == 12345).all())
    assert all(bool((s[T * q:] == 12345.0).all()) for s in sel) and bool((inc[T * (q + 1):] == 12345.0).all())
    si = sel_idx[:T * q].view(T, q)
    tr = trace[:T * q * rows].view(T, q, rows)
    assert bool((si[1] == -1).all()) and bool(torch.isneginf(sel[0][:T * q].view(T, q)[1]).all()) and bool((tr[1] == 0).all())
    assert all(bool((s[:T * q].view(T, q)[1] == 0).all()) for s in sel[1:]) and bool((inc[:T * (q + 1)].view(T, q + 1)[1] == bf[1]).all())
    full = gp_ops.liar_pool(b, phi, X, best_f=bf, q=q, labels=lab, want_trace=True)   # the other tasks do not see the skipped one
    for t in (0, 2):
        assert torch.equal(si[t], full["sel_idx"][t]) and torch.equal(tr[t], full["trace"][t])
        assert torch.equal(inc[:T * (q + 1)].view(T, q + 1)[t], full["inc"][t])


def test_bo_loop(dev):
    """refit_every=1 is today's loop; batch="liar" with one pick per iteration is batch="topk"; refit_every=4 gives records of the
    right length without repeats, equal on two runs, and a replicate alone gives what it gives beside another."""
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(5)
    X = torch.randn(200, 8, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, kernel_type="matern", device=dev, init_from=100, noise_init=0.01, noise_prior=True)
    rngs = lambda seeds=(0, 1): [np.random.default_rng(s) for s in seeds]
    today = BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=1, num_bo_iters=3, **kw)
    assert today == BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=1, num_bo_iters=3, refit_every=1, **kw)
    assert today == BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=1, num_bo_iters=3, batch="liar", **kw)
    four = BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=4, num_bo_iters=2, batch="liar", lie="mean", **kw)
    for rec in four:
        assert len(rec) == 1 + 2 * 4 and len(set(rec[1:])) == 8
    replay = BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=1, num_bo_iters=6, refit_every=4, acquisition="log_ei", **kw)
    assert len(replay) == 2
    for rec in replay:
        assert len(rec) == 1 + 6 and len(set(rec[1:])) == 6
    assert replay == BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=1, num_bo_iters=6, refit_every=4, acquisition="log_ei", **kw)
    for r in (0, 1):
        alone = BO.run_gp_ei_bo_batched(X, y, rngs=rngs((r,)), query_batch_size=1, num_bo_iters=6, refit_every=4, acquisition="log_ei", **kw)
        assert alone == [replay[r]]
    assert [rec[:2] for rec in replay] == [rec[:2] for rec in BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=1, num_bo_iters=1,
                                                                                     acquisition="log_ei", **kw)]
    with pytest.raises(ValueError):
        BO.run_gp_ei_bo_batched(X, y, rngs=rngs(), query_batch_size=2, num_bo_iters=2, refit_every=2, **kw)
