"""GPU: streaming marginal prediction for ARD batches (adkf_predict_marginal_ard / gp_ops.predict_marginal with ard=True) against
the float64 oracle, against ARD adkf_predict on the same fitted batch, on the float64 path, against the isotropic entry at equal
lengthscales, beyond the old cap in a fixed workspace, bit for bit against itself, and through its callers."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

from test_gpu_predict_marginal import _features, _oracle_diag, _path, _rel, _scalars

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _isp(x):
    return math.log(math.expm1(x))


def _batch(dev, Zs, ys, n_s, kernel):
    from adkf_ift_amd import gp_ops

    T = Zs.shape[0]
    return gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.empty(T, 4, device=dev), kernel, ard=True,
                          n_s=None if n_s is None else torch.tensor(n_s, dtype=torch.int32))


def _fit_ard(dev, Zs, ys, n_s, kernel, numeric, max_evals=100):
    from adkf_ift_amd import gp_ops

    b = _batch(dev, Zs, ys, n_s, kernel)
    phi0, _ = gp_ops.init_params_batch(b, numeric, True)
    phi, _, _, _, info = gp_ops.fit(b, phi0, max_evals)
    gp_ops.check_info(info)
    return b, phi


def _spread_phi(dev, b, numeric, seed):
    """A per-dimension phi without a fit: the median-heuristic lengthscale of init_params_batch with a seeded +-30 % spread."""
    from adkf_ift_amd import gp_ops

    phi0, l0 = gp_ops.init_params_batch(b, numeric, True)
    g = torch.Generator().manual_seed(seed)
    f = 1.0 + 0.3 * (2.0 * torch.rand(b.T, b.d, generator=g, dtype=torch.float64) - 1.0)
    ell = l0.double().cpu()[:, None] * f
    phi = phi0.clone()
    phi[:, 2:] = torch.log(torch.expm1(ell)).float().to(dev)
    return phi


def _q(dev, nq):
    return torch.tensor([0] + list(np.cumsum(nq)), dtype=torch.int64, device=dev)


CASES = [  # (kernel, regression, ns_max, d)
    ("rbf", False, 5, 4), ("matern", True, 16, 12), ("rbf", True, 64, 64), ("matern", False, 128, 256), ("rbf", True, 128, 12),
]


@pytest.mark.parametrize("kernel,regression,ns,d", CASES)
def test_parity_after_an_ard_fit(dev, kernel, regression, ns, d):
    from adkf_ift_amd import gp_ops

    T = 3
    n_s = [ns, max(2, ns - 3), max(2, (2 * ns) // 3)]
    nq = [37, 0, 130]
    Zs, ys, Zq = _features(T, ns, nq, d, 300 + ns + d, regression)
    b, phi = _fit_ard(dev, Zs, ys, n_s, kernel, regression)
    assert phi.shape == (T, 2 + d)
    q_off = _q(dev, nq)
    b.flags = gp_ops.REUSE_INNER
    mean, var, _, info = gp_ops.predict_marginal(b, phi, torch.cat(Zq).to(dev), q_off)
    gp_ops.check_info(info)
    kind = gp_ops.kernel_id(kernel)
    for t in range(T):
        lo, hi = int(q_off[t]), int(q_off[t + 1])
        if hi == lo:
            continue
        m_ref, v_ref, _ = _oracle_diag(Zs[t, :n_s[t]], ys[t, :n_s[t]], Zq[t], phi[t], kind)
        assert _rel(mean[lo:hi].cpu(), m_ref) <= TOL, (t, "mean")
        assert _rel(var[lo:hi].cpu(), v_ref) <= TOL, (t, "var")
    # ARD adkf_predict on the same fitted batch (padded query set)
    nq_max = max(nq)
    Zq_pad = torch.zeros(T, nq_max, d)
    for t in range(T):
        Zq_pad[t, :nq[t]] = Zq[t]
    bj = gp_ops.GPBatch(b.Z_s, b.y_s, b.priors, kernel, Z_q=Zq_pad.to(dev), y_q=torch.zeros(T, nq_max, device=dev), n_s=b.n_s,
                        n_q=torch.tensor(nq, dtype=torch.int32), ard=True)
    mj, vj, _, info = gp_ops.predict(bj, phi)
    gp_ops.check_info(info)
    for t in range(T):
        lo, hi = int(q_off[t]), int(q_off[t + 1])
        if hi > lo:
            assert _rel(mean[lo:hi].cpu(), mj[t, :nq[t]].cpu()) <= 2e-5, (t, "mean vs adkf_predict")
            assert _rel(var[lo:hi].cpu(), vj[t, :nq[t]].cpu()) <= 2e-5, (t, "var vs adkf_predict")


@pytest.mark.parametrize("ns", [200, 1024])
def test_more_than_128_points_at_a_fixed_phi(dev, ns):
    """The refined instance (every task beyond 128 points), and at 1024 points the global-slot instances; no fit."""
    from adkf_ift_amd import gp_ops

    T, d = 3, 12
    n_s = [ns, ns - 37, (2 * ns) // 3]
    nq = [150, 0, 301]
    Zs, ys, Zq = _features(T, ns, nq, d, 500 + ns, True)
    b = _batch(dev, Zs, ys, n_s, "matern")
    phi = _spread_phi(dev, b, False, ns)
    q_off = _q(dev, nq)
    mean, var, _, info = gp_ops.predict_marginal(b, phi, torch.cat(Zq).to(dev), q_off)
    gp_ops.check_info(info)
    for t in range(T):
        lo, hi = int(q_off[t]), int(q_off[t + 1])
        if hi == lo:
            continue
        m_ref, v_ref, _ = _oracle_diag(Zs[t, :n_s[t]], ys[t, :n_s[t]], Zq[t], phi[t], 1)
        assert _rel(mean[lo:hi].cpu(), m_ref) <= TOL, (t, "mean")
        assert _rel(var[lo:hi].cpu(), v_ref) <= TOL, (t, "var")


def test_float64_path(dev):
    """The 2-D tasks of test_gpu_predict_marginal.test_ill_conditioned_tasks at long per-dimension lengthscales and a noise near
    its floor: every task takes the float64 path (asserted from the scalars, whose base-carve offsets hold in the ARD workspace)."""
    from adkf_ift_amd import gp_ops
    from adkf_ift_amd.synthetic import make_tasks

    tasks = make_tasks(3, 16, 2, N_q=64, regression=True, first_task=1800)
    Zs, Zq = tasks.features()
    n_s, nq = [16, 15, 16], [64, 31, 50]
    b = _batch(dev, Zs, tasks.y_s, n_s, "rbf")
    b.priors.copy_(torch.tensor([[0.0, -1.0, 0.0, -1.0]] * 3))
    phi = torch.tensor([[-9.0, 0.0, _isp(2.0), _isp(3.0)]] * 3, dtype=torch.float32, device=dev)
    q_off = _q(dev, nq)
    mean, var, _, info = gp_ops.predict_marginal(b, phi, torch.cat([Zq[t, :nq[t]] for t in range(3)]).to(dev), q_off)
    gp_ops.check_info(info)
    torch.cuda.synchronize()
    sc = _scalars(b)
    assert all(_path(sc[t]) == 2 for t in range(3)), [float(sc[t][45]) for t in range(3)]
    for t in range(3):
        lo, hi = int(q_off[t]), int(q_off[t + 1])
        m_ref, v_ref, _ = _oracle_diag(Zs[t, :n_s[t]], tasks.y_s[t, :n_s[t]], Zq[t, :nq[t]], phi[t], 0)
        assert _rel(mean[lo:hi].cpu(), m_ref) <= TOL, (t, "mean")
        assert _rel(var[lo:hi].cpu(), v_ref) <= TOL, (t, "var")


def test_equal_lengthscales_match_the_isotropic_entry(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d = 3, 48, 20
    nq = [70, 33, 0]
    n_s = [48, 40, 29]
    Zs, ys, Zq = _features(T, ns, nq, d, 17, True)
    raw = torch.tensor([[-2.5, 0.2, _isp(3.0)], [-1.5, -0.3, _isp(4.5)], [-3.0, 0.5, _isp(2.2)]], dtype=torch.float32, device=dev)
    phi_ard = torch.cat([raw[:, :2], raw[:, 2:].expand(T, d)], 1).contiguous()
    q_off = _q(dev, nq)
    Zq_p = torch.cat(Zq).to(dev)
    ba = _batch(dev, Zs, ys, n_s, "rbf")
    bi = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.zeros(T, 4, device=dev), "rbf", n_s=torch.tensor(n_s, dtype=torch.int32))
    ba.priors.zero_()
    ra = gp_ops.predict_marginal(ba, phi_ard, Zq_p, q_off)
    ri = gp_ops.predict_marginal(bi, raw, Zq_p, q_off)
    for x, y in zip(ra[:2], ri[:2]):
        assert _rel(x.cpu(), y.cpu()) <= 2e-5


def test_fixed_workspace_beyond_the_old_cap(dev):
    from adkf_ift_amd import _lib, gp_ops

    T, ns, d = 3, 128, 256
    nq = [0, 70000, 5000]
    Zs, ys, Zq = _features(T, ns, nq, d, 7, True)
    b = _batch(dev, Zs, ys, None, "rbf")
    phi = _spread_phi(dev, b, False, 7)
    lib = _lib.load()
    need = lib.adkf_workspace_bytes_ard(T, ns, 0, d)
    ws, nb = b.workspace()
    assert nb == need
    rows = sum(nq)
    q_off = _q(dev, nq)
    Zq_p = torch.cat(Zq).to(dev).contiguous()
    guard = 4096
    out = {k: torch.full((rows + guard,), 12345.0, device=dev) for k in ("mean", "var", "ei")}
    info = torch.empty(T, dtype=torch.int32, device=dev)
    best = torch.zeros(T, device=dev)
    cb = b.c_struct()
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.adkf_predict_marginal_ard(C.byref(cb), p(phi), 0, p(Zq_p), p(q_off), rows, p(best), p(out["mean"]), p(out["var"]),
                                       p(out["ei"]), p(info), p(ws), need, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    gp_ops.check_info(info)
    for k in out:
        assert bool((out[k][rows:] == 12345.0).all()), k
    for t in range(T):
        lo, hi = int(q_off[t]), int(q_off[t + 1])
        if hi == lo:
            continue
        m_ref, v_ref, _ = _oracle_diag(Zs[t], ys[t], Zq[t], phi[t], 0)
        assert _rel(out["mean"][lo:hi].cpu(), m_ref) <= TOL, t
        assert _rel(out["var"][lo:hi].cpu(), v_ref) <= TOL, t


def test_bit_for_bit_properties(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d = 4, 48, 64
    nq = [100, 0, 257, 64]
    n_s = [48, 30, 41, 12]
    Zs, ys, Zq = _features(T, ns, nq, d, 11, True)
    b, phi = _fit_ard(dev, Zs, ys, n_s, "matern", True)
    best = torch.tensor([0.1, -0.2, 0.3, 0.0], device=dev)
    q_off = _q(dev, nq)
    Zq_p = torch.cat(Zq).to(dev)
    b.flags = 0
    r1 = gp_ops.predict_marginal(b, phi, Zq_p, q_off, best_f=best)
    r2 = gp_ops.predict_marginal(b, phi, Zq_p, q_off, best_f=best)
    for x, y in zip(r1[:3], r2[:3]):
        assert torch.equal(x, y)
    # task order permuted: the per-row results permute with it
    perm = [2, 0, 3, 1]
    bp = gp_ops.GPBatch(Zs[perm].to(dev), ys[perm].to(dev), b.priors[perm].clone(), "matern",
                        n_s=torch.tensor([n_s[q] for q in perm], dtype=torch.int32), ard=True)
    nq_p = [nq[q] for q in perm]
    q_off_p = _q(dev, nq_p)
    rp = gp_ops.predict_marginal(bp, phi[perm].contiguous(), torch.cat([Zq[q] for q in perm]).to(dev), q_off_p,
                                 best_f=best[perm].contiguous())
    for k in range(3):
        for j, q in enumerate(perm):
            assert torch.equal(rp[k][int(q_off_p[j]):int(q_off_p[j + 1])], r1[k][int(q_off[q]):int(q_off[q + 1])]), (k, q)
    # REUSE_INNER after an ARD gp_ops.fit equals the call without reuse at the fitted phi
    b2 = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), b.priors.clone(), "matern", n_s=torch.tensor(n_s, dtype=torch.int32), ard=True)
    phi2, _, _, _, info = gp_ops.fit(b2, phi, 100)
    gp_ops.check_info(info)
    b2.flags = gp_ops.REUSE_INNER
    ra = gp_ops.predict_marginal(b2, phi2, Zq_p, q_off, best_f=best)
    b2.flags = 0
    rb = gp_ops.predict_marginal(b2, phi2, Zq_p, q_off, best_f=best)
    for x, y in zip(ra[:3], rb[:3]):
        assert torch.equal(x, y)


def test_unowned_rows_and_empty_tasks_are_zero(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d = 3, 16, 8
    Zs, ys, _ = _features(T, ns, [0, 0, 0], d, 4, True)
    b, phi = _fit_ard(dev, Zs, ys, [16, 8, 12], "rbf", True)
    b.n_s = torch.tensor([16, 0, 12], dtype=torch.int32, device=dev)   # task 1: no support points at prediction time
    b.flags = gp_ops.REUSE_INNER
    rows = 40
    Zq = torch.randn(rows, d, device=dev)
    q_off = torch.tensor([2, 10, 20, 25], dtype=torch.int64, device=dev)   # rows 0..1 and 25..39 belong to nobody
    for _ in range(2):   # (the second call lands in memory the first one filled)
        mean, var, ei, _ = gp_ops.predict_marginal(b, phi, Zq, q_off, best_f=torch.zeros(T, device=dev))
        for x in (mean, var, ei):
            x = x.cpu()
            assert bool((x[:2] == 0).all()) and bool((x[25:] == 0).all()) and bool((x[10:20] == 0).all())
            assert bool((x[2:10] != 0).any()) and bool((x[20:25] != 0).any())


def test_latent_and_ei(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d = 2, 32, 16
    nq = [90, 70]
    Zs, ys, Zq = _features(T, ns, nq, d, 5, True)
    b, phi = _fit_ard(dev, Zs, ys, None, "rbf", True)
    q_off = _q(dev, nq)
    Zq_p = torch.cat(Zq).to(dev)
    best = torch.tensor([-0.3, 0.2], device=dev)
    b.flags = gp_ops.REUSE_INNER
    for maximize in (False, True):
        mean, var, ei, _ = gp_ops.predict_marginal(b, phi, Zq_p, q_off, latent=True, best_f=best, maximize=maximize)
        for t in range(T):
            lo, hi = int(q_off[t]), int(q_off[t + 1])
            m_ref, v_ref, noise = _oracle_diag(Zs[t], ys[t], Zq[t], phi[t], 0)
            vl = np.maximum(v_ref - noise, 1e-12)
            assert _rel(mean[lo:hi].cpu(), m_ref) <= TOL
            assert _rel(var[lo:hi].cpu(), vl) <= TOL
            s = np.sqrt(vl)
            u = ((m_ref - best[t].item()) if maximize else (best[t].item() - m_ref)) / s
            cdf = 0.5 * torch.erfc(torch.from_numpy(-u / math.sqrt(2.0))).numpy()
            e_ref = s * (u * cdf + np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi))
            assert np.abs(ei[lo:hi].cpu().numpy() - e_ref).max() <= 1e-4 * max(1.0, np.abs(e_ref).max())


def test_callers(dev):
    from adkf_ift_amd import _lib
    from adkf_ift_amd import bayes_opt as BO
    from adkf_ift_amd import evaluate as E
    from adkf_ift_amd.meta_batch import collate_meta_batch
    from adkf_ift_amd.models import (ADKTModel, ExactGPLayer, ExactMarginalLogLikelihood, GaussianLikelihood,
                                     fit_gpytorch_scipy)
    from test_meta_batch import random_task, small_model

    torch.manual_seed(1)
    model = ADKTModel(dataclasses.replace(small_model(False), use_ard=True)).to(dev)
    tasks = [random_task(16, 40, 21).to(dev), random_task(13, 9, 22).to(dev), random_task(16, 130, 23).to(dev)]
    mb = collate_meta_batch(tasks).to(dev)
    p0, v0, phi0, _ = E.meta_test(model, mb, want_var=True)
    p1, v1, phi1, _ = E.meta_test(model, mb, want_var=True, streaming=True)
    assert phi1.shape == (3, 2 + model.config.fc_out_dim)
    assert torch.equal(phi0, phi1)
    assert _rel(p1.cpu(), p0.cpu()) <= 2e-5 and _rel(v1.cpu(), v0.cpu()) <= 2e-5

    d = 6
    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, d, generator=g) * torch.tensor([1.0, 0.5, 2.0, 1.0, 3.0, 0.7])
    y = ((X - 0.3) ** 2 * torch.tensor([1.0, 2.0, 0.2, 1.0, 0.05, 1.5])).sum(1)
    X, y = X.to(dev), y.to(dev)
    idx = list(range(0, 10000, 80))
    ys = (y[idx] - y[idx].mean()) / y[idx].std()
    likelihood = GaussianLikelihood(noise_prior=(math.log(0.01) + 0.0625, 0.25)).to(dev)
    gp = ExactGPLayer(X[idx], ys, likelihood, "matern", ard_num_dims=d).to(dev)
    likelihood.noise = 0.01
    gp.covar_module.base_kernel.lengthscale = torch.ones(d) * 2.0
    mll = ExactMarginalLogLikelihood(likelihood, gp).to(dev)
    fit_gpytorch_scipy(mll)
    phi = torch.cat([p.detach().reshape(-1) for p in mll.raw_params()])
    assert phi.numel() == 2 + d
    m_ref, v_ref, noise = _oracle_diag(X[idx], ys, X, phi, 1)
    vl_ref = np.maximum(v_ref - noise, 1e-12)
    assert X.shape[0] > _lib.load().adkf_max_points()
    for streaming in (True, None):   # None: beyond adkf_max_points() rows it streams
        mean, var = BO.latent_posterior(gp, mll, X, streaming=streaming)
        assert _rel(mean.cpu(), m_ref) <= TOL and _rel(var.cpu(), vl_ref) <= TOL, streaming
    # the joint path (adkf_predict) holds at most adkf_max_points() rows, and only up to R64_MAXN = 1024 points does its workspace
    # carry the float64 region this fitted (ill-conditioned) task needs.  Its variance is os - sum C K + noise in float32 even
    # for a float64 task (k_predict), and the noise is taken off afterwards: the latent variance keeps about 3e-4 of its
    # range here (the streaming float64 kernel sums in float64)
    sub = 1000
    mean, var = BO.latent_posterior(gp, mll, X[:sub], streaming=False)
    assert _rel(mean.cpu(), m_ref[:sub]) <= TOL and _rel(var.cpu(), vl_ref[:sub]) <= 1e-3
