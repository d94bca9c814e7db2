"""GPU: feature gradients of streaming prediction (adkf_predict_grad / gp_ops.predict_grad) against float64 autograd through the
oracle (grad_ref.py) on every path - the matrix-pipe tile with one and two support panels and a tail chunk of d, the row kernel
beyond 128 points and on a task of the float64 path, an ARD batch - for each cotangent alone and all together, EI and log EI in
both senses; log EI where float32 EI is 0; the exact properties; and the two callers.

The bound is the project's own: max |got - ref| <= 1e-4 max |ref| over a task's [rows_t, d] block."""
import numpy as np
import pytest
import torch

import grad_ref as R
import test_gpu_believer_pool as B
import test_gpu_believer_pool_ard as BA
import test_gpu_predict_marginal as M

pytestmark = pytest.mark.gpu

NQ = [37, 0, 130]          # partial tiles and an empty task
ROWS = sum(NQ)
SEED = 900


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _q_off(dev, nq=NQ):
    return torch.tensor([0] + list(np.cumsum(nq)), dtype=torch.int64, device=dev)


_refs = {}


def _ref(key, Zs, ys, n_s, Xh, ph, kind, t, lo, hi, combo, cots, best):
    """The reference block of task t for one cotangent set, computed once per problem and left unchanged."""
    k = (key, t, combo[0], None if best is None else float(best))
    if k not in _refs:
        _, um, uv, ue, maximize, log_ei = combo
        sl = lambda use, a: a[lo:hi] if use else None
        _refs[k] = R.predict_grad_ref(Zs[t, :n_s[t]], ys[t, :n_s[t]], Xh[lo:hi], ph[t], kind, sl(um, cots[0]), sl(uv, cots[1]), sl(ue, cots[2]),
                                      best, maximize, log_ei)
    return _refs[k]


def _median_best(key, Zs, ys, n_s, Xh, ph, kind, q_off):
    """best_f per task: the median of the reference mean over the task's rows, so that u_e is centred (float32 array [T])."""
    k = (key, "best")
    if k not in _refs:
        out = np.zeros(len(n_s), np.float32)
        for t in range(len(n_s)):
            lo, hi = q_off[t], q_off[t + 1]
            if hi > lo:
                out[t] = np.median(R.predict_grad_ref(Zs[t, :n_s[t]], ys[t, :n_s[t]], Xh[lo:hi], ph[t], kind, g_mean=np.ones(hi - lo))[1])
        _refs[k] = out
    return _refs[k]


def _call(b, phi, X, q_off, combo, cots, best):
    from adkf_ift_amd import gp_ops

    _, um, uv, ue, maximize, log_ei = combo
    g = [torch.from_numpy(c).to(b.device) if use else None for c, use in zip(cots, (um, uv, ue))]
    dZ, info = gp_ops.predict_grad(b, phi, X, q_off, g_mean=g[0], g_var=g[1], g_ei=g[2], best_f=best if ue else None, maximize=maximize,
                                   log_ei=log_ei)
    gp_ops.check_info(info)
    return dZ


def _check_problem(key, b, phi, Zs, ys, n_s, X, q_off, tag, u_max=8.0, best=None):
    """Every cotangent set of grad_ref.COMBOS on one problem; the input conditions come from the reference alone.  Returns the worst
    error / bound."""
    Xh, ph, off = X.cpu().numpy(), phi.cpu().numpy(), q_off.cpu().tolist()
    Zs, ys = np.asarray(Zs), np.asarray(ys)
    cots = R.cotangents(Xh.shape[0], 7)
    if best is None:
        best = _median_best(key, Zs, ys, n_s, Xh, ph, b.kernel, off)
    best_d = torch.from_numpy(best).to(b.device)
    worst = 0.0
    for combo in R.COMBOS:
        dZ = _call(b, phi, X, q_off, combo, cots, best_d).cpu().numpy()
        for t in range(b.T):
            lo, hi = off[t], off[t + 1]
            if hi == lo:
                continue
            ref, _, v, u, os_ = _ref(key, Zs, ys, n_s, Xh, ph, b.kernel, t, lo, hi, combo, cots, best[t] if combo[3] else None)
            assert v.min() >= 0.01 * os_, (tag, t, v.min() / os_, "the rows must keep a variance of at least 0.01 os")
            if u is not None:
                assert np.abs(u).max() <= u_max, (tag, t, np.abs(u).max())
            err = R.rel(dZ[lo:hi], ref)
            worst = max(worst, err / R.TOL)
            print(f"{tag} {combo[0]} task {t}: min v / os {v.min() / os_:.3f}, error / bound {err / R.TOL:.4f}")
            assert err <= R.TOL, (tag, combo[0], t, err)
    print(f"{tag}: worst error / bound {worst:.4f}")
    return worst


SHAPES = [  # (kernel, n_s, d): the smallest shapes that reach each path
    ("rbf", [5, 4, 3], 12),                # a corner of one panel
    ("matern", [48, 45, 31], 33),          # one panel, d % 4 != 0
    ("rbf", [128, 125, 85], 130),          # two panels, three chunks of d with a tail
    ("matern", [200, 197, 133], 24),       # beyond 128 points: the row kernel, refined solves
]


@pytest.mark.parametrize("kernel,n_s,d", SHAPES)
def test_against_autograd(dev, kernel, n_s, d):
    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, ROWS, SEED + max(n_s))
    _check_problem((kernel, tuple(n_s), d), b, phi, Zs, ys, n_s, X, _q_off(dev), (kernel, max(n_s), d))


def test_a_task_of_the_float64_path(dev):
    """The ill-conditioned batch of test_gpu_predict_marginal.test_ill_conditioned_tasks: task 1 takes the float64 path (asserted from
    the fitted scalars), its neighbours a float32 one; after the fit (REUSE_INNER) and evaluated afresh.  The fitted noise is tiny and
    the 2-D query rows lie among the support points, so most of them have almost no variance left: the candidates are the task's
    query rows and the same rows 1.5 times as far from the support mean, and the rows kept are those that meet the input conditions
    (v >= 0.01 os, |u_e| <= 8 against the median mean; selected at 0.02 and 7, so that the assertions hold with a margin) - chosen from
    the reference alone."""
    from adkf_ift_amd import gp_ops
    from adkf_ift_amd.synthetic import make_tasks

    tasks = make_tasks(3, 16, 2, N_q=64, regression=True, first_task=1800)
    Zs, Zq = tasks.features()
    n_s, nq = [16, 15, 16], [64, 31, 50]
    b, phi = M._fit(dev, Zs, tasks.y_s, n_s, "rbf", True)
    torch.cuda.synchronize()
    assert M._path(M._scalars(b)[1]) == 2
    ph = phi.cpu().numpy()
    rows, best = [], np.zeros(3, np.float32)
    for t in range(3):
        zs, mu = Zs[t, :n_s[t]], Zs[t, :n_s[t]].mean(0)
        cand = torch.cat([Zq[t, :nq[t]], mu + 1.5 * (Zq[t, :nq[t]] - mu)]).numpy()
        _, m, v, _, os_ = R.predict_grad_ref(zs.numpy(), tasks.y_s[t, :n_s[t]].numpy(), cand, ph[t], 0, g_mean=np.ones(len(cand)))
        ok = v >= 0.02 * os_
        best[t] = np.float32(np.median(m[ok]))
        ok &= np.abs((float(best[t]) - m) / np.sqrt(v)) <= 7.0
        assert ok.sum() >= 8, (t, ok.sum())
        rows.append(cand[ok])
    X = torch.from_numpy(np.concatenate(rows)).to(dev)
    q_off = _q_off(dev, [len(r) for r in rows])
    for flags in (gp_ops.REUSE_DIST | gp_ops.REUSE_INNER, 0):
        b.flags = flags
        _check_problem("ill", b, phi, Zs, tasks.y_s, n_s, X, q_off, ("float64 path", flags), best=best)


def test_an_ard_batch(dev):
    kernel, n_s, d, _, _ = BA.CASES[0]
    b, phi, Zs, ys, n_s, X, _ = BA._explicit(dev, kernel, n_s, d, ROWS, SEED + max(n_s))
    _check_problem("ard", b, phi, Zs, ys, n_s, X, _q_off(dev), "ard")


def test_log_ei_where_float32_ei_is_zero(dev):
    """best_f shifted so that u_e lies in [-25, -15] on every row kept (the rows are chosen from the reference alone): float32 EI is 0
    there, the gradient of log EI is finite and within the bound."""
    from adkf_ift_amd import gp_ops

    kernel, n_s, d = SHAPES[1]
    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, ROWS, SEED + max(n_s))
    Xh, ph = X.cpu().numpy(), phi.cpu().numpy()
    Zs, ys = np.asarray(Zs), np.asarray(ys)
    off = [0] + list(np.cumsum(NQ))
    keep, best, nq = [], np.zeros(b.T, np.float32), []
    for t in range(b.T):
        lo, hi = off[t], off[t + 1]
        if hi == lo:
            nq.append(0)
            continue
        _, m, v, _, _ = R.predict_grad_ref(Zs[t, :n_s[t]], ys[t, :n_s[t]], Xh[lo:hi], ph[t], b.kernel, g_mean=np.ones(hi - lo))
        s = np.sqrt(v)
        best[t] = np.float32(np.median(m - 20.0 * s))      # minimisation: u_e = (best_f - m) / sigma, about -20
        u = (float(best[t]) - m) / s
        rows = np.nonzero((u >= -25.0) & (u <= -15.0))[0] + lo
        assert len(rows) >= 16, (t, len(rows))
        keep.append(rows)
        nq.append(len(rows))
    Xk = X[torch.from_numpy(np.concatenate(keep)).to(dev)].contiguous()
    q_off = _q_off(dev, nq)
    best_d = torch.from_numpy(best).to(dev)
    _, _, ei, _ = gp_ops.predict_marginal(b, phi, Xk, q_off, best_f=best_d)
    assert bool((ei.abs() < 1e-37).all()), ei.abs().max()       # 0, or a negative denormal
    ge = R.cotangents(Xk.shape[0], 5)[2]
    dZ, info = gp_ops.predict_grad(b, phi, Xk, q_off, g_ei=torch.from_numpy(ge).to(dev), best_f=best_d, log_ei=True)
    gp_ops.check_info(info)
    dZ = dZ.cpu().numpy()
    assert np.isfinite(dZ).all()
    offk, Xkh = q_off.cpu().tolist(), Xk.cpu().numpy()
    for t in range(b.T):
        lo, hi = offk[t], offk[t + 1]
        if hi == lo:
            continue
        ref, _, _, u, _ = R.predict_grad_ref(Zs[t, :n_s[t]], ys[t, :n_s[t]], Xkh[lo:hi], ph[t], b.kernel, g_ei=ge[lo:hi], best=best[t], log_ei=True)
        assert u.min() >= -25.0 and u.max() <= -15.0, (t, u.min(), u.max())
        err = R.rel(dZ[lo:hi], ref)
        print(f"far log EI task {t}: {hi - lo} rows, u_e in [{u.min():.2f}, {u.max():.2f}], error / bound {err / R.TOL:.4f}")
        assert err <= R.TOL, (t, err)


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("kernel,n_s,d", [SHAPES[1], SHAPES[3]])
def test_exact_properties(dev, kernel, n_s, d):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, ROWS, SEED + max(n_s))
    T = b.T
    q_off = _q_off(dev)
    cots = [torch.from_numpy(c).to(dev) for c in R.cotangents(ROWS, 7)]
    best = torch.zeros(T, device=dev)
    kw = dict(g_mean=cots[0], g_var=cots[1], g_ei=cots[2], best_f=best, log_ei=True)
    first, info = gp_ops.predict_grad(b, phi, X, q_off, **kw)
    gp_ops.check_info(info)
    assert bool(torch.isfinite(first).all()) and bool((first[:37] != 0).any()) and bool((first[37:] != 0).any())
    # two calls give equal bits
    again, _ = gp_ops.predict_grad(b, phi, X, q_off, **kw)
    assert torch.equal(_bits(first), _bits(again))
    # zero cotangents give bit-zero dZq
    z = torch.zeros(ROWS, device=dev)
    out, _ = gp_ops.predict_grad(b, phi, X, q_off, g_mean=z, g_var=z, g_ei=z, best_f=best)
    assert bool((_bits(out) == 0).all())
    # cotangents times 2 give dZq times 2, bit for bit
    out, _ = gp_ops.predict_grad(b, phi, X, q_off, **dict(kw, g_mean=2 * cots[0], g_var=2 * cots[1], g_ei=2 * cots[2]))
    assert torch.equal(_bits(out), _bits(2 * first))
    # a task alone equals the same task inside the batch, bit for bit
    off = q_off.cpu().tolist()
    for t in (0, 2):
        lo, hi = off[t], off[t + 1]
        b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].clone(), kernel, n_s=b.n_s[t:t + 1].cpu())
        o1, _ = gp_ops.predict_grad(b1, phi[t:t + 1].contiguous(), X[lo:hi].contiguous(), torch.tensor([0, hi - lo], dtype=torch.int64, device=dev),
                                    g_mean=cots[0][lo:hi].contiguous(), g_var=cots[1][lo:hi].contiguous(), g_ei=cots[2][lo:hi].contiguous(),
                                    best_f=best[t:t + 1].contiguous(), log_ei=True)
        assert torch.equal(_bits(o1), _bits(first[lo:hi])), t
    # unowned rows are 0; so are the rows of a task with info != 0 (a NaN noise), and the healthy tasks' bits do not move
    q_part = torch.tensor([2, 30, 30, 150], dtype=torch.int64, device=dev)   # rows 0, 1 and 150.. belong to nobody
    out, _ = gp_ops.predict_grad(b, phi, X, q_part, **kw)
    assert bool((_bits(out[:2]) == 0).all()) and bool((_bits(out[150:]) == 0).all()) and bool((out[2:30] != 0).any())
    phib = phi.clone()
    phib[2, 0] = float("nan")
    out, info = gp_ops.predict_grad(b, phib, X, q_off, **kw)
    info = info.cpu()
    assert int(info[2]) != 0 and int(info[0]) == 0 and int(info[1]) == 0, info.tolist()
    assert bool((_bits(out[37:]) == 0).all()) and torch.equal(_bits(out[:37]), _bits(first[:37]))
    # a NaN stays in its own row
    Xn = X.clone()
    Xn[40, 1] = float("nan")
    out, _ = gp_ops.predict_grad(b, phi, Xn, q_off, **kw)
    assert bool(torch.isnan(out[40]).any())
    keep = torch.ones(ROWS, dtype=torch.bool, device=dev)
    keep[40] = False
    assert torch.equal(_bits(out[keep]), _bits(first[keep]))
    with pytest.raises(ValueError):
        gp_ops.predict_grad(b, phi, X, q_off)
    with pytest.raises(ValueError):
        gp_ops.predict_grad(b, phi, X, q_off, g_ei=cots[2])


def test_reuse_inner_after_a_fit(dev):
    """REUSE_INNER after a fit equals a fresh evaluation at the fitted phi, within the bound."""
    from adkf_ift_amd import gp_ops

    T, ns, d = 3, 48, 33
    n_s = [48, 45, 31]
    Zs, ys, Zq = M._features(T, ns, NQ, d, 11, True)
    b, phi = M._fit(dev, Zs, ys, n_s, "matern", True)
    X, q_off = torch.cat(Zq).to(dev), _q_off(dev)
    cots = [torch.from_numpy(c).to(dev) for c in R.cotangents(ROWS, 7)]
    kw = dict(g_mean=cots[0], g_var=cots[1], g_ei=cots[2], best_f=torch.zeros(T, device=dev))
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    reused, info = gp_ops.predict_grad(b, phi, X, q_off, **kw)
    gp_ops.check_info(info)
    b.flags = 0
    fresh, info = gp_ops.predict_grad(b, phi, X, q_off, **kw)
    gp_ops.check_info(info)
    off = q_off.cpu().tolist()
    for t in (0, 2):
        err = R.rel(reused[off[t]:off[t + 1]].cpu().numpy(), fresh[off[t]:off[t + 1]].cpu().numpy())
        print(f"REUSE_INNER task {t}: error / bound {err / R.TOL:.4f}")
        assert err <= R.TOL, (t, err)


def test_predict_marginal_diff_under_a_feature_map(dev):
    """models.predict_marginal_diff behind a small nn.Linear: the weight gradient of sum(mean) + sum(var) against the float64 chain."""
    from adkf_ift_amd import models

    kernel, n_s, d = SHAPES[1]
    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, ROWS, SEED + max(n_s))
    q_off = _q_off(dev)
    torch.manual_seed(3)
    lin = torch.nn.Linear(d, d)
    with torch.no_grad():
        lin.weight.copy_(torch.eye(d) + 0.05 * torch.randn(d, d))
        lin.bias.copy_(0.02 * torch.randn(d))
    lin64 = torch.nn.Linear(d, d).double()
    with torch.no_grad():
        lin64.weight.copy_(lin.weight.double()); lin64.bias.copy_(lin.bias.double())
    lin = lin.to(dev)
    phi_g = phi.clone().requires_grad_(True)
    mean, var, ei = models.predict_marginal_diff(b, phi_g, lin(X), q_off)
    assert not ei.requires_grad
    (mean.sum() + var.sum()).backward()
    assert phi_g.grad is None                       # phi and the support set are constants of the fitted state
    Z64 = lin64(X.cpu().double())
    off, ph = q_off.cpu().tolist(), phi.cpu().double()
    total = torch.zeros((), dtype=torch.float64)
    for t in range(b.T):
        lo, hi = off[t], off[t + 1]
        if hi > lo:
            m, v, _ = R.posterior(Zs[t, :n_s[t]].double(), ys[t, :n_s[t]].double(), Z64[lo:hi], ph[t], b.kernel)
            total = total + m.sum() + v.sum()
    total.backward()
    for got, ref, name in ((lin.weight.grad, lin64.weight.grad, "weight"), (lin.bias.grad, lin64.bias.grad, "bias")):
        err = R.rel(got.cpu().numpy(), ref.numpy())
        print(f"predict_marginal_diff {name} gradient: error / bound {err / R.TOL:.4f}")
        assert err <= R.TOL, (name, err)


def test_explain_hits_on_a_model(dev):
    """evaluate.explain_hits on screen's top_idx with a -1 tail: the rows' feature gradients of the mean at the returned phi against
    autograd on the model's own features; -1 entries give zero rows."""
    from adkf_ift_amd import evaluate as E
    from adkf_ift_amd import gp_ops
    from adkf_ift_amd.meta_batch import collate_meta_batch
    from adkf_ift_amd.models import ADKTModel
    from test_meta_batch import random_task, small_model

    torch.manual_seed(1)
    model = ADKTModel(small_model(True)).to(dev)
    tasks = [random_task(16, 40, 21).to(dev), random_task(13, 9, 22).to(dev), random_task(16, 130, 23).to(dev)]
    mb = collate_meta_batch(tasks).to(dev)
    Z_s, Z_q = E.meta_features(model, mb)
    y_s, _ = mb.labels(True)
    lib_rows = Z_q[2, :130].detach().float().contiguous()
    top_idx, _, phi = E.screen(model, mb, lib_rows, 4)
    idx = torch.cat([top_idx, torch.full((3, 2), -1, dtype=torch.int64, device=dev)], 1)
    for of in ("mean", "log_ei"):
        G = E.explain_hits(model, mb, lib_rows, idx, of=of)
        assert G.shape == (3, 6, lib_rows.shape[1]) and bool((G[:, 4:] == 0).all()) and bool(torch.isfinite(G).all())
        if of != "mean":
            continue
        Xh, ph = lib_rows.cpu().numpy(), phi.cpu().numpy()
        for t, n in enumerate(mb.n_s.tolist()):
            rows = top_idx[t].cpu().numpy()
            ref = R.predict_grad_ref(Z_s[t, :n].detach().float().cpu().numpy(), y_s[t, :n].float().cpu().numpy(), Xh[rows], ph[t],
                                     gp_ops.kernel_id(model.config.gp_kernel), g_mean=np.ones(4))[0]
            err = R.rel(G[t, :4].cpu().numpy(), ref)
            print(f"explain_hits task {t}: error / bound {err / R.TOL:.4f}")
            assert err <= R.TOL, (t, err)
