"""GPU: streaming marginal prediction (adkf_predict_marginal / gp_ops.predict_marginal) against the float64 oracle, against
adkf_predict on the same fitted batch, beyond the old 4096-point cap, bit for bit against itself, and through its callers."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def _oracle_diag(zs, ys, zq, phi, kind, chunk=4096):
    """float64 mean and noisy variance diagonal of the rows zq, in chunks (no [rows, rows] block)."""
    from oracle import gp_oracle as O

    zs, ys, zq, phi = zs.double().cpu(), ys.double().cpu(), zq.double().cpu(), phi.double().cpu()
    noise, os_, ls = O.transform_phi(phi)
    A = O.kernel_matrix(zs, zs, os_, ls, kind) + noise * torch.eye(zs.shape[0], dtype=torch.float64)
    L = torch.linalg.cholesky(A)
    alpha = torch.cholesky_solve(ys[:, None], L)[:, 0]
    means, vars_ = [], []
    for lo in range(0, zq.shape[0], chunk):
        K = O.kernel_matrix(zq[lo:lo + chunk], zs, os_, ls, kind)
        W = torch.linalg.solve_triangular(L, K.T, upper=False)
        means.append(K @ alpha)
        vars_.append(os_ - (W * W).sum(0) + noise)
    if not means:
        return np.zeros(0), np.zeros(0), float(noise)
    return torch.cat(means).numpy(), torch.cat(vars_).numpy(), float(noise)


def _features(T, ns_max, nq_list, d, seed, regression):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(d, d, generator=g) / math.sqrt(d)
    Zs = torch.randn(T, ns_max, d, generator=g) @ W
    Zq = [torch.randn(m, d, generator=g) @ W for m in nq_list]
    f = lambda z: torch.sin(z[..., : min(d, 4)].sum(-1))
    ys = f(Zs) + 0.1 * torch.randn(T, ns_max, generator=g)
    if not regression:
        ys = (ys > 0).float()
    return Zs.float(), ys.float(), [z.float() for z in Zq]


def _fit(dev, Zs, ys, n_s, kernel, numeric):
    from adkf_ift_amd import gp_ops

    T = Zs.shape[0]
    b = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.empty(T, 4, device=dev), kernel,
                       n_s=None if n_s is None else torch.tensor(n_s, dtype=torch.int32))
    phi0, _ = gp_ops.init_params_batch(b, numeric, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    return b, phi


S_PIVR_A, S_CONDA = 45, 47          # per-task scalar slots (csrc/device_utils.h enum Scal)
R64_THRESHOLD, REFINE32_THRESHOLD = 30.0, 3.0


def _scalars(b):
    """The per-task scalars [T, 64] the fit left in the workspace of a support-only batch: the carve() order of csrc/host_gp.h
    (mean, D2ss, Ainv, P, W_ss, vecs, scal; every block 256-byte aligned; the query blocks are empty)."""
    ws, _ = b.workspace()
    al = lambda nfloat: (nfloat * 4 + 255) // 256 * 256
    T, ns, d = b.T, b.ns, b.d
    off = al(T * d) + 4 * al(T * ns * ns) + al(T * 16 * ns)
    return ws[off:off + T * 64 * 4].view(torch.float32).view(T, 64).cpu()


def _path(sc):
    """0 plain, 1 refined C, 2 float64 - the choice of predict_stream.h's pm_kind_of (ns <= 128)."""
    return 2 if sc[S_PIVR_A] > R64_THRESHOLD else (1 if sc[S_CONDA] > REFINE32_THRESHOLD else 0)


CASES = [  # (kernel, regression, ns_max, d)
    ("rbf", False, 5, 12), ("matern", True, 16, 64), ("rbf", True, 64, 256), ("matern", False, 128, 2048),
    ("rbf", False, 200, 64), ("matern", True, 1024, 12), ("rbf", True, 128, 12), ("matern", False, 64, 2048),
]


@pytest.mark.parametrize("kernel,regression,ns,d", CASES)
def test_oracle_and_adkf_predict_parity(dev, kernel, regression, ns, d):
    from adkf_ift_amd import gp_ops

    T = 3
    n_s = [ns, max(2, ns - 3), max(2, (2 * ns) // 3)]
    nq = [37, 0, 130]
    Zs, ys, Zq = _features(T, ns, nq, d, 100 + ns + d, regression)
    b, phi = _fit(dev, Zs, ys, n_s, kernel, regression)
    q_off = torch.tensor([0] + list(np.cumsum(nq)), dtype=torch.int64, device=dev)
    Zq_p = torch.cat(Zq).to(dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    mean, var, _, info = gp_ops.predict_marginal(b, phi, Zq_p, q_off)
    gp_ops.check_info(info)
    kind = gp_ops.kernel_id(kernel)
    for t in range(T):
        lo, hi = int(q_off[t]), int(q_off[t + 1])
        if hi == lo:
            continue
        m_ref, v_ref, _ = _oracle_diag(Zs[t, :n_s[t]], ys[t, :n_s[t]], Zq[t], phi[t], kind)
        assert _rel(mean[lo:hi].cpu(), m_ref) <= TOL, (t, "mean")
        assert _rel(var[lo:hi].cpu(), v_ref) <= TOL, (t, "var")
    # adkf_predict on the same fitted batch (padded query set)
    nq_max = max(nq)
    Zq_pad = torch.zeros(T, nq_max, d)
    for t in range(T):
        Zq_pad[t, :nq[t]] = Zq[t]
    bj = gp_ops.GPBatch(b.Z_s, b.y_s, b.priors, kernel, Z_q=Zq_pad.to(dev), y_q=torch.zeros(T, nq_max, device=dev), n_s=b.n_s,
                        n_q=torch.tensor(nq, dtype=torch.int32))
    mj, vj, _, info = gp_ops.predict(bj, phi)
    gp_ops.check_info(info)
    for t in range(T):
        lo, hi = int(q_off[t]), int(q_off[t + 1])
        if hi > lo:
            assert _rel(mean[lo:hi].cpu(), mj[t, :nq[t]].cpu()) <= 2e-5, (t, "mean vs adkf_predict")
            assert _rel(var[lo:hi].cpu(), vj[t, :nq[t]].cpu()) <= 2e-5, (t, "var vs adkf_predict")


def test_ill_conditioned_tasks(dev):
    """The 2-D regression tasks of test_ill_conditioned_regression_task_is_resolved_stably (task 1: 15 + 31 points takes the
    float64 path - asserted from the fitted scalars) and their neighbours, every task against the oracle."""
    from adkf_ift_amd import gp_ops
    from adkf_ift_amd.synthetic import make_tasks

    tasks = make_tasks(3, 16, 2, N_q=64, regression=True, first_task=1800)
    Zs, Zq = tasks.features()
    n_s, nq = [16, 15, 16], [64, 31, 50]
    b, phi = _fit(dev, Zs, tasks.y_s, n_s, "rbf", True)
    torch.cuda.synchronize()
    assert _path(_scalars(b)[1]) == 2
    q_off = torch.tensor([0] + list(np.cumsum(nq)), dtype=torch.int64, device=dev)
    Zq_p = torch.cat([Zq[t, :nq[t]] for t in range(3)]).to(dev)
    for flags in (gp_ops.REUSE_DIST | gp_ops.REUSE_INNER, 0):
        b.flags = flags
        mean, var, _, info = gp_ops.predict_marginal(b, phi, Zq_p, q_off)
        gp_ops.check_info(info)
        for t in range(3):
            lo, hi = int(q_off[t]), int(q_off[t + 1])
            m_ref, v_ref, _ = _oracle_diag(Zs[t, :n_s[t]], tasks.y_s[t, :n_s[t]], Zq[t, :nq[t]], phi[t], 0)
            assert _rel(mean[lo:hi].cpu(), m_ref) <= TOL, (flags, t, "mean")
            assert _rel(var[lo:hi].cpu(), v_ref) <= TOL, (flags, t, "var")


def test_beyond_the_old_cap_with_a_fixed_workspace(dev):
    from adkf_ift_amd import _lib, gp_ops

    T, ns, d = 3, 128, 256
    nq = [0, 70000, 5000]
    Zs, ys, Zq = _features(T, ns, nq, d, 7, True)
    b, phi = _fit(dev, Zs, ys, None, "rbf", True)
    lib = _lib.load()
    need = lib.adkf_workspace_bytes(T, ns, 0, d)
    ws, nb = b.workspace()
    assert nb == need
    rows = sum(nq)
    q_off = torch.tensor([0] + list(np.cumsum(nq)), dtype=torch.int64, device=dev)
    Zq_p = torch.cat(Zq).to(dev).contiguous()
    guard = 4096
    out = {k: torch.full((rows + guard,), 12345.0, device=dev) for k in ("mean", "var", "ei")}
    info = torch.empty(T, dtype=torch.int32, device=dev)
    best = torch.zeros(T, device=dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    cb = b.c_struct()
    import ctypes as C
    rc = lib.adkf_predict_marginal(C.byref(cb), C.c_void_p(phi.data_ptr()), 0, C.c_void_p(Zq_p.data_ptr()), C.c_void_p(q_off.data_ptr()),
                                   rows, C.c_void_p(best.data_ptr()), C.c_void_p(out["mean"].data_ptr()), C.c_void_p(out["var"].data_ptr()),
                                   C.c_void_p(out["ei"].data_ptr()), C.c_void_p(info.data_ptr()), C.c_void_p(ws.data_ptr()), need,
                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
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
    b, phi = _fit(dev, Zs, ys, n_s, "matern", True)
    best = torch.tensor([0.1, -0.2, 0.3, 0.0], device=dev)
    q_off = torch.tensor([0] + list(np.cumsum(nq)), dtype=torch.int64, device=dev)
    Zq_p = torch.cat(Zq).to(dev)
    b.flags = 0
    r1 = gp_ops.predict_marginal(b, phi, Zq_p, q_off, best_f=best)
    r2 = gp_ops.predict_marginal(b, phi, Zq_p, q_off, best_f=best)
    for x, y in zip(r1[:3], r2[:3]):
        assert torch.equal(x, y)
    # task order permuted: the per-row results permute with it
    perm = [2, 0, 3, 1]
    bp = gp_ops.GPBatch(Zs[perm].to(dev), ys[perm].to(dev), b.priors[perm].clone(), "matern",
                        n_s=torch.tensor([n_s[p] for p in perm], dtype=torch.int32))
    nq_p = [nq[p] for p in perm]
    q_off_p = torch.tensor([0] + list(np.cumsum(nq_p)), dtype=torch.int64, device=dev)
    rp = gp_ops.predict_marginal(bp, phi[perm].contiguous(), torch.cat([Zq[p] for p in perm]).to(dev), q_off_p, best_f=best[perm].contiguous())
    for k in range(3):
        for j, p in enumerate(perm):
            assert torch.equal(rp[k][int(q_off_p[j]):int(q_off_p[j + 1])], r1[k][int(q_off[p]):int(q_off[p + 1])]), (k, p)
    # REUSE_INNER after adkf_fit (with and without DEFER_REFINE) equals the call without reuse at the fitted phi
    for extra in (0, gp_ops.DEFER_REFINE):
        b2 = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), b.priors.clone(), "matern", n_s=torch.tensor(n_s, dtype=torch.int32))
        b2.flags = extra
        phi2, _, _, _, info = gp_ops.fit(b2, phi, 200)
        gp_ops.check_info(info)
        b2.flags = gp_ops.REUSE_INNER
        ra = gp_ops.predict_marginal(b2, phi2, Zq_p, q_off, best_f=best)
        b2.flags = 0
        rb = gp_ops.predict_marginal(b2, phi2, Zq_p, q_off, best_f=best)
        for x, y in zip(ra[:3], rb[:3]):
            assert torch.equal(x, y), extra


def test_latent_and_ei(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d = 2, 32, 16
    nq = [90, 70]
    Zs, ys, Zq = _features(T, ns, nq, d, 5, True)
    b, phi = _fit(dev, Zs, ys, None, "rbf", True)
    q_off = torch.tensor([0] + list(np.cumsum(nq)), dtype=torch.int64, device=dev)
    Zq_p = torch.cat(Zq).to(dev)
    best = torch.tensor([-0.3, 0.2], device=dev)
    for maximize in (False, True):
        mean, var, ei, _ = gp_ops.predict_marginal(b, phi, Zq_p, q_off, latent=True, best_f=best, maximize=maximize)
        for t in range(T):
            lo, hi = int(q_off[t]), int(q_off[t + 1])
            m_ref, v_ref, noise = _oracle_diag(Zs[t], ys[t], Zq[t], phi[t], 0)
            vl = np.maximum(v_ref - noise, 1e-12)
            assert _rel(var[lo:hi].cpu(), vl) <= TOL
            s = np.sqrt(vl)
            u = ((m_ref - best[t].item()) if maximize else (best[t].item() - m_ref)) / s
            cdf = 0.5 * torch.erfc(torch.from_numpy(-u / math.sqrt(2.0))).numpy()
            e_ref = s * (u * cdf + np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi))
            assert np.abs(ei[lo:hi].cpu().numpy() - e_ref).max() <= 1e-4 * max(1.0, np.abs(e_ref).max())


def test_callers(dev):
    from adkf_ift_amd import bayes_opt as BO
    from adkf_ift_amd import evaluate as E
    from adkf_ift_amd.meta_batch import collate_meta_batch
    from adkf_ift_amd.models import ADKTModel, fit_gpytorch_scipy
    from test_meta_batch import random_task, small_model

    torch.manual_seed(1)
    model = ADKTModel(small_model(False)).to(dev)
    tasks = [random_task(16, 40, 21).to(dev), random_task(13, 9, 22).to(dev), random_task(16, 130, 23).to(dev)]
    mb = collate_meta_batch(tasks).to(dev)
    p0, v0, phi0, _ = E.meta_test(model, mb, want_var=True)
    p1, v1, phi1, _ = E.meta_test(model, mb, want_var=True, streaming=True)
    assert torch.equal(phi0, phi1)
    assert _rel(p1.cpu(), p0.cpu()) <= 2e-5 and _rel(v1.cpu(), v0.cpu()) <= 2e-5

    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    idx = list(range(9000, 10000, 40))
    ys = (y - y.mean()) / y.std()
    _, gp, mll = BO.create_gp(X[idx], ys[idx], "matern", dev, noise_init=0.01, noise_prior=True)
    fit_gpytorch_scipy(mll)
    mean, var = BO.latent_posterior(gp, mll, X, streaming=True)
    phi = torch.cat([p.detach().reshape(-1) for p in mll.raw_params()])
    m_ref, v_ref, noise = _oracle_diag(X[idx], ys[idx], X, phi, 1)
    assert _rel(mean.cpu(), m_ref) <= TOL
    assert _rel(var.cpu(), np.maximum(v_ref - noise, 1e-12)) <= TOL
    rec = BO.run_gp_ei_bo(X, y, num_init_points=6, query_batch_size=2, num_bo_iters=3, kernel_type="matern", device=dev,
                          init_from=5000, noise_init=0.01, noise_prior=True, rng=np.random.default_rng(0), streaming=True)
    assert len(rec) == 1 + 3 * 2 and len(set(rec[1:])) == 6


_REFINED_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_predict_marginal as M
from adkf_ift_amd import gp_ops
dev = torch.device("cuda:0")
T, ns, d, nq = 3, 64, 16, [40, 0, 75]
n_s = [64, 50, 33]
Zs, ys, Zq = M._features(T, ns, nq, d, 21, True)
b, phi = M._fit(dev, Zs, ys, n_s, "matern", True)
torch.cuda.synchronize()
sc = M._scalars(b)
assert all(float(sc[t][M.S_CONDA]) > 0.0 for t in range(T))   # above the threshold 0: every task takes the refined C
q_off = torch.tensor([0] + list(np.cumsum(nq)), dtype=torch.int64, device=dev)
b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
mean, var, _, info = gp_ops.predict_marginal(b, phi, torch.cat(Zq).to(dev), q_off)
gp_ops.check_info(info)
for t in range(T):
    lo, hi = int(q_off[t]), int(q_off[t + 1])
    if hi > lo:
        m_ref, v_ref, _ = M._oracle_diag(Zs[t, :n_s[t]], ys[t, :n_s[t]], Zq[t], phi[t], 1)
        assert M._rel(mean[lo:hi].cpu(), m_ref) <= M.TOL and M._rel(var[lo:hi].cpu(), v_ref) <= M.TOL, t
print("refined ok")
"""


def test_refined_c_branch_at_most_128_points(dev):
    """The refined-C instance (REFINE = true, LDS row tiles) on tasks of at most 128 points: a fresh process with the refinement
    threshold at 0 (ADKF_REFINE32_THRESHOLD, read once per process) sends every task there; against the oracle.  (Beyond 128
    points every task takes it anyway: the 200- and 1024-point parity cases.)"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ADKF_REFINE32_THRESHOLD="0", ADKF_R64_THRESHOLD="1e30")
    r = subprocess.run([sys.executable, "-c", _REFINED_CHILD, root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "refined ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_unowned_rows_and_empty_tasks_are_zero(dev):
    """Rows outside every task's (clamped) range and rows of a task with n_s == 0 come back as 0, not as uninitialised memory."""
    from adkf_ift_amd import gp_ops

    T, ns, d = 3, 16, 8
    Zs, ys, _ = _features(T, ns, [0, 0, 0], d, 4, True)
    b, phi = _fit(dev, Zs, ys, [16, 8, 12], "rbf", True)
    b.n_s = torch.tensor([16, 0, 12], dtype=torch.int32, device=dev)   # task 1: no support points at prediction time
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    rows = 40
    Zq = torch.randn(rows, d, device=dev)
    q_off = torch.tensor([2, 10, 20, 25], dtype=torch.int64, device=dev)   # rows 0..1 and 25..39 belong to nobody
    for _ in range(2):   # (the second call lands in memory the first one filled)
        mean, var, ei, _ = gp_ops.predict_marginal(b, phi, Zq, q_off, best_f=torch.zeros(T, device=dev))
        for x in (mean, var, ei):
            x = x.cpu()
            assert bool((x[:2] == 0).all()) and bool((x[25:] == 0).all()) and bool((x[10:20] == 0).all())
            assert bool((x[2:10] != 0).any())
