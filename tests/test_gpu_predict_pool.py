"""GPU: shared-pool prediction (adkf_predict_pool / gp_ops.predict_pool) - bit for bit against the packed call on every task
kind, against the float64 oracle, the device selection against the ordering rule and against the oracle's EI, guard bands, and
the batched BO loop against the sequential one."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import test_gpu_predict_marginal as M
import test_gpu_predict_marginal_ard as MA
from test_predict_pool_cpu import select_ref

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _pool(rows, d, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(d, d, generator=g) / math.sqrt(d)
    return (torch.randn(rows, d, generator=g) @ W).float()


def _ill_batch(dev):
    """Four ragged 2-D regression tasks of mixed kinds: task 1 (15 points) takes the float64 path (asserted from the fitted
    scalars, as test_gpu_predict_marginal.test_ill_conditioned_tasks does), at least one other task a float32 one."""
    from adkf_ift_amd.synthetic import make_tasks

    tasks = make_tasks(4, 16, 2, N_q=64, regression=True, first_task=1800)
    Zs, Zq = tasks.features()
    n_s = [16, 15, 5, 3]
    b, phi = M._fit(dev, Zs, tasks.y_s, n_s, "rbf", True)
    torch.cuda.synchronize()
    kinds = [M._path(sc) for sc in M._scalars(b)]
    print("kinds of the ill-conditioned batch:", kinds)
    assert kinds[1] == 2 and min(kinds) < 2, kinds
    return b, phi, Zs, tasks.y_s, n_s, Zq


def _assert_equals_packed(b, phi, X, best, tag):
    """predict_pool(...)[t] == predict_marginal with q_off giving task t the whole pool and every other task nothing."""
    from adkf_ift_amd import gp_ops

    T, rows = b.T, X.shape[0]
    for latent, maximize in ((False, False), (True, True)):
        out = gp_ops.predict_pool(b, phi, X, latent=latent, best_f=best, maximize=maximize)
        gp_ops.check_info(out["info"])
        for t in range(T):
            q_off = torch.tensor([0] * (t + 1) + [rows] * (T - t), dtype=torch.int64, device=X.device)
            mean, var, ei, _ = gp_ops.predict_marginal(b, phi, X, q_off, latent=latent, best_f=best, maximize=maximize)
            assert torch.equal(out["mean"][t], mean), (tag, t, "mean")
            assert torch.equal(out["var"][t], var), (tag, t, "var")
            assert torch.equal(out["ei"][t], ei), (tag, t, "ei")
            assert bool((mean != 0).any())


BIT_CASES = [  # (kernel, ns_max, d, rows): plain; rows < 64; refined with LDS row tiles; refined with global slots
    ("matern", 48, 64, 1000), ("rbf", 128, 256, 37), ("rbf", 200, 64, 333), ("matern", 1024, 12, 300),
]


@pytest.mark.parametrize("kernel,ns,d,rows", BIT_CASES)
def test_bit_for_bit_against_the_packed_call(dev, kernel, ns, d, rows):
    from adkf_ift_amd import gp_ops

    T = 4
    n_s = [ns, max(2, ns - 3), max(2, (2 * ns) // 3), max(2, ns // 4)]
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 300 + ns + d, True)
    b, phi = M._fit(dev, Zs, ys, n_s, kernel, True)
    torch.cuda.synchronize()
    if ns <= 128:
        assert all(M._path(sc) == 0 for sc in M._scalars(b)), "these cases are meant to reach the plain instance"
    X = _pool(rows, d, 17).to(dev)
    best = torch.tensor([0.1, -0.2, 0.3, 0.0], device=dev)
    for flags in (gp_ops.REUSE_DIST | gp_ops.REUSE_INNER, 0):
        b.flags = flags
        _assert_equals_packed(b, phi, X, best, (kernel, ns, flags))


def test_bit_for_bit_float64_task(dev):
    from adkf_ift_amd import gp_ops

    b, phi, *_ = _ill_batch(dev)
    X = torch.cat([_pool(450, 2, 3), b.Z_s[1, :5].cpu()]).to(dev)
    best = torch.tensor([0.1, -0.2, 0.3, 0.0], device=dev)
    for flags in (gp_ops.REUSE_DIST | gp_ops.REUSE_INNER, 0):
        b.flags = flags
        _assert_equals_packed(b, phi, X, best, ("float64", flags))


def test_bit_for_bit_ard(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d = 4, 64, 12
    n_s = [64, 50, 33, 9]
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 31, True)
    b, phi = MA._fit_ard(dev, Zs, ys, n_s, "matern", True)
    X = _pool(523, d, 5).to(dev)
    best = torch.tensor([0.1, -0.2, 0.3, 0.0], device=dev)
    for flags in (gp_ops.REUSE_INNER, 0):
        b.flags = flags
        _assert_equals_packed(b, phi, X, best, ("ard", flags))


_REFINED_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_predict_marginal as M
import test_gpu_predict_pool as P
from adkf_ift_amd import gp_ops
dev = torch.device("cuda:0")
T, ns, d = 4, 64, 16
n_s = [64, 50, 33, 20]
Zs, ys, _ = M._features(T, ns, [0] * T, d, 21, True)
b, phi = M._fit(dev, Zs, ys, n_s, "matern", True)
torch.cuda.synchronize()
sc = M._scalars(b)
assert all(float(sc[t][M.S_CONDA]) > 0.0 for t in range(T))   # above the threshold 0: every task takes the refined C
X = P._pool(301, d, 9).to(dev)
best = torch.tensor([0.1, -0.2, 0.3, 0.0], device=dev)
for flags in (gp_ops.REUSE_DIST | gp_ops.REUSE_INNER, 0):
    b.flags = flags
    P._assert_equals_packed(b, phi, X, best, ("refined", flags))
out = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, topk=7)
for t in range(T):
    idx, val = P.select_ref(out["ei"][t].cpu().numpy(), 7)
    assert np.array_equal(out["top_idx"][t].cpu().numpy(), idx) and np.array_equal(out["top_val"][t].cpu().numpy().view(np.int32), val.view(np.int32))
print("refined ok")
"""


def test_bit_for_bit_refined_at_most_128_points(dev):
    """The refined-C instance with LDS row tiles on tasks of at most 128 points: a fresh process with the refinement threshold
    at 0, as test_gpu_predict_marginal.test_refined_c_branch_at_most_128_points."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ADKF_REFINE32_THRESHOLD="0", ADKF_R64_THRESHOLD="1e30")
    r = subprocess.run([sys.executable, "-c", _REFINED_CHILD, root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "refined ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _oracle_ei(zs, ys, X, phi, kind, best, maximize):
    m_ref, v_ref, noise = M._oracle_diag(zs, ys, X, phi, kind)
    vl = np.maximum(v_ref - noise, 1e-12)
    s = np.sqrt(vl)
    u = ((m_ref - best) if maximize else (best - m_ref)) / s
    cdf = 0.5 * torch.erfc(torch.from_numpy(-u / math.sqrt(2.0))).numpy()
    return m_ref, v_ref, vl, s * (u * cdf + np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi))


@pytest.mark.parametrize("kernel,ns,d", [("rbf", 32, 16), ("matern", 200, 64)])
def test_against_the_oracle(dev, kernel, ns, d):
    from adkf_ift_amd import gp_ops

    T, rows = 4, 777
    n_s = [ns, ns - 3, (2 * ns) // 3, ns // 4]
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 55 + ns, True)
    b, phi = M._fit(dev, Zs, ys, n_s, kernel, True)
    X = _pool(rows, d, 8)
    best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(T)])
    kind = gp_ops.kernel_id(kernel)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    for latent, maximize in ((False, False), (True, True)):
        out = gp_ops.predict_pool(b, phi, X.to(dev), latent=latent, best_f=best.to(dev), maximize=maximize)
        for t in range(T):
            m_ref, v_ref, vl, e_ref = _oracle_ei(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], kind, best[t].item(), maximize)
            assert M._rel(out["mean"][t].cpu(), m_ref) <= TOL, (t, "mean")
            assert M._rel(out["var"][t].cpu(), vl if latent else v_ref) <= TOL, (t, "var")
            assert np.abs(out["ei"][t].cpu().numpy() - e_ref).max() <= 1e-4 * max(1.0, np.abs(e_ref).max()), (t, "ei")


def _selection_problem(dev, which):
    """(b, phi, X, best): a batch of mixed kinds and a pool of more than 100 000 rows with planted duplicate rows."""
    if which == "float64+refined":
        b, phi, Zs, ys, n_s, _ = _ill_batch(dev)
        d = 2
    else:   # more than 128 points: every task takes the refined C, with row tiles in LDS
        T, ns, d = 4, 200, 64
        n_s = [200, 197, 133, 150]
        Zs, ys, _ = M._features(T, ns, [0] * T, d, 91, True)
        b, phi = M._fit(dev, Zs, ys, n_s, "matern", True)
    rows = 100003
    X = _pool(rows, d, 13) * (1.0 if d > 2 else 0.6)
    for src, dst in ((11, 70001), (11, 99999), (5000, 64), (5000, 65), (31234, 31235)):
        X[dst] = X[src]
    best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(b.T)])
    return b, phi, X.to(dev), best.to(dev)


@pytest.mark.parametrize("which", ["float64+refined", "refined"])
def test_selection_on_the_device(dev, which):
    from adkf_ift_amd import gp_ops

    b, phi, X, best = _selection_problem(dev, which)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    T, rows = b.T, X.shape[0]
    first = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, want_mean=False, want_var=False, topk=8)
    top0 = first["top_idx"].cpu()
    assert bool((first["top_val"][:, 0] > 0).all()), "EI must not have underflowed everywhere"
    g = np.random.default_rng(2)
    # different lengths: task 0's best row (and its runner-ups' neighbours), nothing, many rows, the duplicates' first copy
    lists = [[int(top0[0, 0]), 3, 2, 2, rows + 5, -1], [], sorted(g.choice(rows, 5000, replace=False).tolist() + top0[2, :3].tolist()),
             [11, 5000, int(top0[3, 1])]]
    clean = [sorted({i for i in l if 0 <= i < rows}) for l in lists]
    for k in (1, 7, 64):
        out = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, topk=k, exclude=lists)
        ei = out["ei"].cpu().numpy()
        ti, tv = out["top_idx"].cpu().numpy(), out["top_val"].cpu().numpy()
        for t in range(T):
            idx, val = select_ref(ei[t], k, clean[t])
            assert np.array_equal(ti[t], idx), (k, t, ti[t], idx)
            assert np.array_equal(tv[t].view(np.int32), val.view(np.int32)), (k, t)
        assert int(ti[0, 0]) != int(top0[0, 0])
        # nothing per row: the same selection; and again: bit-equal
        for _ in range(2):
            o2 = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=k,
                                     exclude=lists)
            assert o2["mean"] is None and o2["var"] is None and o2["ei"] is None
            assert torch.equal(o2["top_idx"], out["top_idx"]) and torch.equal(o2["top_val"], out["top_val"])
    # duplicates: whenever both copies are selected the lower index comes first (already implied by the rule; spelled out)
    out = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, topk=64)
    assert torch.equal(out["ei"][:, 11], out["ei"][:, 70001]) and torch.equal(out["ei"][:, 64], out["ei"][:, 5000])
    for maximize in (False, True):
        out = gp_ops.predict_pool(b, phi, X, maximize=maximize, score="mean", topk=7, exclude=lists)
        mean = out["mean"].cpu().numpy()
        for t in range(T):
            idx, val = select_ref(mean[t] if maximize else -mean[t], 7, clean[t])
            assert np.array_equal(out["top_idx"][t].cpu().numpy(), idx), (maximize, t)
            assert np.array_equal(out["top_val"][t].cpu().numpy().view(np.int32), val.view(np.int32)), (maximize, t)
        o2 = gp_ops.predict_pool(b, phi, X, maximize=maximize, score="mean", want_mean=False, want_var=False, topk=7, exclude=lists)
        assert torch.equal(o2["top_idx"], out["top_idx"]) and torch.equal(o2["top_val"], out["top_val"])


def test_planted_ties_come_back_in_index_order(dev):
    """A pool made of a few distinct rows repeated many times: every score is shared by many rows, so the order of the selection is
    decided by the index rule alone, across tiles, chunks and the final merge."""
    from adkf_ift_amd import gp_ops

    T, ns, d = 4, 32, 16
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 77, True)
    b, phi = M._fit(dev, Zs, ys, [32, 20, 27, 9], "rbf", True)
    base = _pool(5, d, 1)
    rows = 20011
    X = base[torch.arange(rows) % 5].contiguous().to(dev)
    best = torch.tensor([float(ys[t].median()) for t in range(T)], device=dev)
    out = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, topk=64, exclude=[[0, 5], [], [1], []])
    ei = out["ei"].cpu().numpy()
    for t, ex in enumerate(([0, 5], [], [1], [])):
        idx, val = select_ref(ei[t], 64, ex)
        assert np.array_equal(out["top_idx"][t].cpu().numpy(), idx), t
        assert np.array_equal(out["top_val"][t].cpu().numpy().view(np.int32), val.view(np.int32)), t
        assert len(np.unique(ei[t])) <= 5


def test_more_tasks_than_workgroups(dev):
    """2000 small tasks: more than a grid has workgroups, so a workgroup serves several tasks one after the other and writes one
    candidate list per task."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows = 2000, 8, 8, 130
    g = torch.Generator().manual_seed(6)
    n_s = torch.randint(3, ns + 1, (T,), generator=g).tolist()
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 66, True)
    b, phi = M._fit(dev, Zs, ys, n_s, "rbf", True)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = _pool(rows, d, 14)
    best = ys.median(1).values
    out = gp_ops.predict_pool(b, phi, X.to(dev), latent=True, best_f=best.to(dev), topk=5, exclude=[[t % rows] for t in range(T)])
    ei, ti, tv = out["ei"].cpu().numpy(), out["top_idx"].cpu().numpy(), out["top_val"].cpu().numpy()
    for t in range(T):
        idx, val = select_ref(ei[t], 5, [t % rows])
        assert np.array_equal(ti[t], idx) and np.array_equal(tv[t].view(np.int32), val.view(np.int32)), t
    for t in (0, 777, 1999):
        _, _, _, e_ref = _oracle_ei(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], 0, best[t].item(), False)
        assert np.abs(ei[t] - e_ref).max() <= 1e-4 * max(1.0, np.abs(e_ref).max()), t


def test_the_selection_is_right(dev):
    """Not only self-consistent: the pick is within 2 delta of the oracle's best EI, delta = 1e-4 max(1, max|e_ref|) being the
    bound the per-row EI is held to (the pick's device score is at least the true best row's device score, and each of the two
    is within delta of its oracle value)."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows = 4, 48, 16, 20000
    n_s = [48, 45, 32, 12]
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 123, True)
    b, phi = M._fit(dev, Zs, ys, n_s, "matern", True)
    X = _pool(rows, d, 29)
    best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(T)])
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    out = gp_ops.predict_pool(b, phi, X.to(dev), latent=True, best_f=best.to(dev), want_mean=False, want_var=False, want_ei=False, topk=4)
    top = out["top_idx"].cpu().numpy()
    for t in range(T):
        _, _, _, e_ref = _oracle_ei(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], 1, best[t].item(), False)
        assert e_ref.max() >= 0.01, "the test problem must keep EI far from float32 underflow"
        delta = 1e-4 * max(1.0, np.abs(e_ref).max())
        assert e_ref[top[t, 0]] >= e_ref.max() - 2 * delta, (t, e_ref[top[t, 0]], e_ref.max())


def test_guard_bands_exact_sizes_and_a_skipped_task(dev):
    from adkf_ift_amd import _lib, gp_ops

    T, ns, d, rows, k = 3, 128, 256, 70001, 64
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 7, True)
    b, phi = M._fit(dev, Zs, ys, [128, 100, 77], "rbf", True)
    lib = _lib.load()
    need = lib.adkf_workspace_bytes(T, ns, 0, d)
    ws, nb = b.workspace()
    assert nb == need
    b.n_s = torch.tensor([128, 0, 77], dtype=torch.int32, device=dev)   # task 1: skipped at prediction time
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = _pool(rows, d, 3).to(dev)
    guard = 4096
    out = {n: torch.full((T * rows + guard,), 12345.0, device=dev) for n in ("mean", "var", "ei")}
    top_idx = torch.full((T * k + guard,), 12345, dtype=torch.int64, device=dev)
    top_val = torch.full((T * k + guard,), 12345.0, device=dev)
    sb = lib.adkf_predict_pool_scratch_bytes(T, k)
    assert 0 < sb <= 4 << 20
    scratch = torch.full((sb + guard,), 0x5a, dtype=torch.uint8, device=dev)
    info = torch.empty(T, dtype=torch.int32, device=dev)
    best = torch.tensor([float(ys[t].median()) for t in range(T)], device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    cb = b.c_struct()
    rc = lib.adkf_predict_pool(C.byref(cb), p(phi), 0, p(X), rows, p(best), None, None, p(out["mean"]), p(out["var"]), p(out["ei"]), k,
                               p(top_idx), p(top_val), p(info), p(ws), need, p(scratch), sb,
                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    gp_ops.check_info(info)
    for n in out:
        assert bool((out[n][T * rows:] == 12345.0).all()), n
        assert bool((out[n][rows:2 * rows] == 0).all()), n            # the skipped task's slice
        assert bool((out[n][:rows] != 0).any()) and bool((out[n][2 * rows:3 * rows] != 0).any()), n
    assert bool((top_idx[T * k:] == 12345).all()) and bool((top_val[T * k:] == 12345.0).all())
    assert bool((scratch[sb:] == 0x5a).all())
    ti, tv = top_idx[:T * k].view(T, k).cpu().numpy(), top_val[:T * k].view(T, k).cpu().numpy()
    assert (ti[1] == -1).all() and np.isneginf(tv[1]).all()
    ei = out["ei"][:T * rows].view(T, rows).cpu().numpy()
    for t in (0, 2):
        idx, val = select_ref(ei[t], k)
        assert np.array_equal(ti[t], idx) and np.array_equal(tv[t].view(np.int32), val.view(np.int32))
    m_ref, v_ref, _ = M._oracle_diag(Zs[2, :77], ys[2, :77], X[:3000].cpu(), phi[2], 0)
    assert M._rel(out["mean"][2 * rows:2 * rows + 3000].cpu(), m_ref) <= TOL
    assert M._rel(out["var"][2 * rows:2 * rows + 3000].cpu(), v_ref) <= TOL


def test_small_pools_and_argument_checks(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d = 4, 16, 8
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 4, True)
    b, phi = M._fit(dev, Zs, ys, [16, 8, 12, 5], "rbf", True)
    best = torch.zeros(T, device=dev)
    X = _pool(5, d, 2).to(dev)
    out = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, topk=8, exclude=[[0, 1, 2, 3, 4], [], [2], None])
    ei = out["ei"].cpu().numpy()
    for t, ex in enumerate(([0, 1, 2, 3, 4], [], [2], [])):
        idx, val = select_ref(ei[t], 8, ex)
        assert np.array_equal(out["top_idx"][t].cpu().numpy(), idx) and np.array_equal(out["top_val"][t].cpu().numpy().view(np.int32), val.view(np.int32))
    assert bool((out["top_idx"][0] == -1).all()) and bool(torch.isneginf(out["top_val"][0]).all())
    out = gp_ops.predict_pool(b, phi, X[:0], latent=True, best_f=best, topk=3)      # an empty pool
    assert out["mean"].shape == (T, 0) and bool((out["top_idx"] == -1).all()) and bool(torch.isneginf(out["top_val"]).all())
    with pytest.raises(ValueError):
        gp_ops.predict_pool(b, phi, X[:, :4].contiguous())
    with pytest.raises(ValueError):
        gp_ops.predict_pool(b, phi, X, topk=3)                 # ranking by EI without best_f
    with pytest.raises(ValueError):
        gp_ops.predict_pool(b, phi, X, topk=65, best_f=best)
    with pytest.raises(ValueError):
        gp_ops.predict_pool(b, phi, X, best_f=best[:2])
    with pytest.raises(ValueError):
        gp_ops.predict_pool(b, phi, X, want_mean=False, want_var=False)
    with pytest.raises(ValueError):
        gp_ops.predict_pool(b, phi, X, score="ucb")
    with pytest.raises(RuntimeError):
        gp_ops.predict_pool(b, phi, X.cpu())


def test_batched_bo_loop(dev):
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=2, num_bo_iters=3, kernel_type="matern", device=dev, init_from=5000, noise_init=0.01,
              noise_prior=True)
    R = 4
    recs = BO.run_gp_ei_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(R)], **kw)
    assert len(recs) == R
    for r in range(R):
        assert len(recs[r]) == 1 + 3 * 2 and len(set(recs[r][1:])) == 6
        alone = BO.run_gp_ei_bo_batched(X, y, rngs=[np.random.default_rng(r)], **kw)
        assert alone[0] == recs[r], (r, "the batch couples replicates")
        seq = BO.run_gp_ei_bo(X, y, rng=np.random.default_rng(r), streaming=True, **kw)
        assert seq == recs[r], (r, "batched vs sequential")


def test_screen_ranks_a_library_by_the_posterior_mean(dev):
    from adkf_ift_amd import evaluate as E
    from adkf_ift_amd import gp_ops
    from adkf_ift_amd.meta_batch import collate_meta_batch
    from adkf_ift_amd.models import ADKTModel
    from test_meta_batch import random_task, small_model

    torch.manual_seed(1)
    model = ADKTModel(small_model(False)).to(dev)
    tasks = [random_task(16, 40, 21).to(dev), random_task(13, 9, 22).to(dev), random_task(16, 130, 23).to(dev)]
    mb = collate_meta_batch(tasks).to(dev)
    _, Z_q = E.meta_features(model, mb)
    lib_rows = Z_q[2, :130].float().contiguous()          # a library in the model's feature space
    preds, _, phi_ref, _ = E.meta_test(model, mb, streaming=True)
    for maximize in (True, False):
        top_idx, top_val, phi = E.screen(model, mb, lib_rows, 5, maximize=maximize)
        assert torch.equal(phi, phi_ref) and top_idx.shape == (3, 5) and top_idx.dtype == torch.int64
        # task 2's library rows are its own query rows: the ranking is that of its meta-test predictions (sigmoid is monotone)
        order = torch.argsort(preds[2, :130], descending=maximize, stable=True)[:5]
        assert torch.equal(preds[2, top_idx[2]].sort().values, preds[2, order].sort().values)   # (ties under the sigmoid allowed)
        assert bool((top_val[:, :-1] >= top_val[:, 1:]).all())
