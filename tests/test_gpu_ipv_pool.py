"""GPU: target-variance batch selection over a shared pool (adkf_ipv_pool / gp_ops.ipv_pool) - every step's scores, pick and target
variance against the float64 reference conditioned on the device's own earlier picks (ipv_ref.py) on every path of the walk and at
the ends of the entry panel, mixed kinds and an ARD batch, M = q = 1 against the same expression from kg_pool's covariances,
determinism and independence of the batch, permuted and skipped target entries, more tasks than workgroups, small pools and failed
tasks, and the batched active-learning loop."""
import numpy as np
import pytest
import torch

import ipv_ref as R
import test_gpu_believer_pool as B
import test_gpu_believer_pool_ard as BA
import test_gpu_predict_marginal as M
import test_gpu_predict_pool as P
from test_believer_pool_ard_cpu import ard_posterior
from test_ipv_pool_cpu import _ipv_twin, ipv_call, targets_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _check_device(out, b, phi, Zs, ys, n_s, X, tgt, w, tag, lists=None, post_fn=R.posterior):
    """ipv_ref.check_task on every task of a call with want_trace; returns the worst error / bound."""
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    si, sv, tv, tr = (None if out[k] is None else out[k].cpu().numpy() for k in ("sel_idx", "sel_val", "tvar", "trace"))
    Xh, ph = X.cpu().numpy(), phi.cpu().numpy()
    worst_all = 0.0
    for t in range(b.T):
        n = n_s[t]
        post = post_fn(np.asarray(Zs[t, :n]), ys[t, :n], Xh, ph[t], b.kernel)
        worst = R.check_task(post, tgt[t], None if w is None else w[t], si[t], sv[t], None if tv is None else tv[t],
                             None if tr is None else tr[t], excluded=lists[t] if lists else (), tag=(tag, t))
        worst_all = max(worst_all, worst)
        got = [p for p in si[t].tolist() if p >= 0]
        assert len(set(got)) == len(got)
    print(f"{tag}: worst error / bound {worst_all:.3f}")
    return worst_all


CASES = [  # (kernel, n_s, d, rows, M, q, weighted, targets excluded, twin too)
    ("matern", [48, 45, 31], 16, 300, 8, 8, True, False, False),       # plain, one panel
    ("rbf", [128, 125, 85], 64, 37, 5, 5, False, False, False),        # two support panels, one partial tile
    ("rbf", [200, 197, 133], 64, 333, 8, 8, False, True, False),       # refined, LDS row tiles
    ("matern", [1024, 700], 12, 130, 4, 4, False, False, True),        # global slots
    ("rbf", [32, 29, 21], 8, 200, 32, 32, False, False, False),        # the full entry panel, M + q = 64
    ("rbf", [32, 29, 21], 8, 200, 63, 1, False, False, False),         # targets nearly fill the panel
    ("rbf", [32, 29, 21], 8, 200, 1, 63, False, False, False),         # picks nearly fill the panel
]


@pytest.mark.parametrize("kernel,n_s,d,rows,Mt,q,weighted,excluded,twin", CASES)
def test_against_the_reference(dev, kernel, n_s, d, rows, Mt, q, weighted, excluded, twin):
    from adkf_ift_amd import gp_ops
    from oracle import cpu_twin

    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    tgt, w = targets_of(b.T, rows, Mt, 7)
    w = w if weighted else None
    lists = [sorted(tgt[t].tolist()) for t in range(b.T)] if excluded else None
    if twin:   # the twin meets the assertions on this shape too (so that a miss of the device is the device's)
        hb = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((b.T, 4), np.float32), b.kernel, n_s=np.array(n_s, np.int32))
        Xh, ph = np.ascontiguousarray(X.cpu().numpy()), np.ascontiguousarray(phi.cpu().numpy())
        si, sv, tv, tr, _ = ipv_call(_ipv_twin(), hb, ph, Xh, tgt, w, q)
        for t in range(b.T):
            post = R.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], Xh, ph[t], b.kernel)
            R.check_task(post, tgt[t], None, si[t], sv[t], tv[t], tr[t], tag=(kernel, "twin", t))
    out = gp_ops.ipv_pool(b, phi, X, targets=tgt, weights=None if w is None else torch.from_numpy(w), q=q, exclude=lists, want_trace=True)
    _check_device(out, b, phi, Zs, ys, n_s, X, tgt, w, (kernel, max(n_s), Mt, q), lists=lists)
    assert bool((out["sel_idx"] >= 0).all())
    assert bool((out["tvar"][:, 1:] < out["tvar"][:, :-1]).all())
    if excluded:
        for t in range(b.T):
            assert not set(out["sel_idx"][t].tolist()) & set(lists[t])


def _mixed(dev):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, _ = P._ill_batch(dev)
    # what the mixed tests rest on, from the fitted scalars: a task on k_ipv_walk64 and a task on a float32 walk
    kinds = [M._path(sc) for sc in M._scalars(b)]
    assert 2 in kinds and min(kinds) < 2, kinds
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.cat([P._pool(300, 2, 3), b.Z_s[1, :5].cpu()]).to(dev)
    return b, phi, Zs, ys, n_s, X


def test_mixed_kinds_in_one_call(dev):
    """test_gpu_predict_pool._ill_batch: task 1 takes the float64 walk (asserted there from the fitted scalars), the others a
    float32 one - both kernels of the walk in one call."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X = _mixed(dev)
    tgt, w = targets_of(b.T, X.shape[0], 4, 21)
    out = gp_ops.ipv_pool(b, phi, X, targets=tgt, weights=torch.from_numpy(w), q=6, want_trace=True)
    _check_device(out, b, phi, Zs, ys, n_s, X, tgt, w, "mixed")


def test_an_ard_batch(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, _ = BA.CASES[0]
    b, phi, Zs, ys, n_s, X, _ = BA._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    tgt, w = targets_of(b.T, rows, 4, 22)
    out = gp_ops.ipv_pool(b, phi, X, targets=tgt, weights=torch.from_numpy(w), q=5, want_trace=True)
    _check_device(out, b, phi, Zs.numpy(), ys, n_s, X, tgt, w, "ard", post_fn=ard_posterior)


def test_one_target_one_pick_is_kg_pools_covariance(dev):
    """M = 1, q = 1, weight 1: score_0(x) = cov(x, r)^2 / (max(v, 1e-12) + noise), against the same expression formed in float64 from
    kg_pool's cov and predict_pool's latent var on the same batch, to 8 eps32 |score| per row: two roundings of the square, one of
    the sum v + noise, one of the quotient, and a factor 2 for margin.  It fails if the panel's cov is not KG's bit for bit."""
    from adkf_ift_amd import gp_ops

    eps = float(np.finfo(np.float32).eps)
    plain = B._explicit(dev, *CASES[0][:4], 548)
    problems = [("plain", plain[0], plain[1], plain[5]), ("mixed",) + tuple(_mixed(dev)[i] for i in (0, 1, 5))]
    for name, b, phi, X in problems:
        rows = X.shape[0]
        tgt = torch.tensor([[(17 * (t + 1)) % rows] for t in range(b.T)], dtype=torch.int64, device=dev)
        out = gp_ops.ipv_pool(b, phi, X, targets=tgt, q=1, want_trace=True)
        kg = gp_ops.kg_pool(b, phi, X, ref_idx=tgt, want_cov=True, want_score=False)
        pp = gp_ops.predict_pool(b, phi, X, latent=True, want_mean=False)
        gp_ops.check_info(out["info"])
        noise = M._scalars(b)[:, 0].double().numpy()   # S_NOISE, as the kernels read it
        cov, var, got = kg["cov"][:, :, 0].double().cpu().numpy(), pp["var"].double().cpu().numpy(), out["trace"][:, 0].double().cpu().numpy()
        for t in range(b.T):
            want = cov[t] ** 2 / (np.maximum(var[t], 1e-12) + noise[t])
            ratio = np.abs(got[t] - want) / (8 * eps * np.abs(want) + 1e-300)
            print(f"M = q = 1, {name} task {t}: worst |score - cov^2 / (v + noise)| / (8 eps |score|) = {ratio.max():.3f}")
            assert ratio.max() <= 1.0, (name, t, float(ratio.max()), int(ratio.argmax()), "the panel's cov is not kg_pool's, or the score's roundings are not the four counted")
            assert want.max() > 0


def test_deterministic_and_independent_of_the_batch(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, Mt, q = CASES[0][:6]
    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    tgt, w = targets_of(b.T, rows, Mt, 7)
    wt = torch.from_numpy(w)
    lists = [[0, 7], [], [3]]
    kw = dict(q=q, exclude=lists, want_trace=True)
    first = gp_ops.ipv_pool(b, phi, X, targets=tgt, weights=wt, **kw)
    again = gp_ops.ipv_pool(b, phi, X, targets=tgt, weights=wt, **kw)
    names = ("sel_idx", "sel_val", "tvar", "trace")
    for name in names:
        assert torch.equal(first[name], again[name]), name
    none = gp_ops.ipv_pool(b, phi, X, targets=tgt, weights=wt, q=q, exclude=lists)      # trace == NULL: the same bits
    assert none["trace"] is None
    for name in names[:3]:
        assert torch.equal(first[name], none[name]), name
    for t in range(b.T):   # each task alone in a T = 1 batch
        b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), kernel,
                            n_s=torch.tensor([n_s[t]], dtype=torch.int32))
        o1 = gp_ops.ipv_pool(b1, phi[t:t + 1].contiguous(), X, targets=tgt[t:t + 1], weights=wt[t:t + 1], q=q, exclude=[lists[t]], want_trace=True)
        for name in names:
            assert torch.equal(o1[name][0], first[name][t]), (t, name)
    # a permutation of the entries with their weights: the same picks
    perm = np.random.default_rng(3).permutation(Mt)
    moved = gp_ops.ipv_pool(b, phi, X, targets=tgt[:, perm], weights=wt[:, perm], **kw)
    assert torch.equal(moved["sel_idx"], first["sel_idx"])
    # skipped entries appended: -1, >= rows, a repeat, and weights 0, NaN and below 0 - no output bit changes
    T = b.T
    col = lambda v: np.full((T, 1), v)
    tgt2 = np.concatenate([tgt, col(-1), col(rows), tgt[:, :1], col(17), col(18), col(19)], 1).astype(np.int64)
    w2 = np.concatenate([w, col(1.0), col(1.0), col(3.0), col(0.0), col(np.nan), col(-1.0)], 1).astype(np.float32)
    more = gp_ops.ipv_pool(b, phi, X, targets=tgt2, weights=torch.from_numpy(w2), **kw)
    for name in names:
        assert torch.equal(more[name], first[name]), name


def test_more_tasks_than_workgroups(dev):
    """T = 300 tiny tasks (test_gpu_believer_pool's construction): assertions 1-4 and tvar on every task, every row of every step
    of the trace included."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, Mt, q = 300, 8, 4, 130, 3, 3
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
    tgt, w = targets_of(T, rows, Mt, 79)
    out = gp_ops.ipv_pool(b, phi, X, targets=tgt, weights=torch.from_numpy(w), q=q, want_trace=True)
    assert out["trace"].shape == (T, q, rows)
    _check_device(out, b, phi, Zs, ys, n_s, X, tgt, w, "T300")


def test_small_pools_exclusions_and_a_failed_task(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows = CASES[0][:4]
    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    T = b.T
    t5 = torch.tensor([[0, 3, 4]] * T, dtype=torch.int64)
    # rows < q: five picks, then the -1 / -inf tail with tvar repeated
    out = gp_ops.ipv_pool(b, phi, X[:5], targets=t5, q=8, want_trace=True)
    si = out["sel_idx"].cpu()
    for t in range(T):
        assert sorted(si[t, :5].tolist()) == list(range(5)) and bool((si[t, 5:] == -1).all())
    assert bool(torch.isneginf(out["sel_val"][:, 5:]).all()) and bool((out["tvar"][:, 5:] == out["tvar"][:, 5:6]).all())
    _check_device(out, b, phi, Zs, ys, n_s, X[:5], t5.numpy(), None, "five rows")
    # every row excluded: nothing is picked, tvar stays
    out = gp_ops.ipv_pool(b, phi, X[:5], targets=t5, q=3, exclude=[list(range(5))] * T)
    assert bool((out["sel_idx"] == -1).all()) and bool(torch.isneginf(out["sel_val"]).all())
    assert bool((out["tvar"] > 0).all()) and bool((out["tvar"] == out["tvar"][:, :1]).all())
    # rows = 0
    out = gp_ops.ipv_pool(b, phi, X[:0], targets=t5, q=3, want_trace=True)
    assert bool((out["sel_idx"] == -1).all()) and bool(torch.isneginf(out["sel_val"]).all()) and bool((out["tvar"] == 0).all())
    assert out["trace"].shape == (T, 3, 0)
    # a task without a valid target among tasks that have some
    tgt, w = targets_of(T, rows, 3, 12)
    full = gp_ops.ipv_pool(b, phi, X, targets=tgt, q=4, want_trace=True)
    tgt1 = tgt.copy()
    tgt1[1] = [-1, rows, rows + 5]
    out = gp_ops.ipv_pool(b, phi, X, targets=tgt1, q=4, want_trace=True)
    assert bool((out["sel_idx"][1] == -1).all()) and bool(torch.isneginf(out["sel_val"][1]).all())
    assert bool((out["tvar"][1] == 0).all()) and bool((out["trace"][1] == 0).all())
    for t in (0, 2):
        assert torch.equal(out["sel_idx"][t], full["sel_idx"][t]) and torch.equal(out["trace"][t], full["trace"][t])
    # a task with info != 0: a NaN noise makes every pivot of its factorisation NaN, which is reported as not positive
    phib = phi.clone()
    phib[1, 0] = float("nan")
    out = gp_ops.ipv_pool(b, phib, X, targets=tgt, q=4, want_trace=True)
    info = out["info"].cpu()
    assert int(info[1]) != 0 and int(info[0]) == 0 and int(info[2]) == 0, info.tolist()
    assert bool((out["sel_idx"][1] == -1).all()) and bool(torch.isneginf(out["sel_val"][1]).all())
    assert bool((out["tvar"][1] == 0).all()) and bool((out["trace"][1] == 0).all())
    for t in (0, 2):
        assert torch.equal(out["sel_idx"][t], full["sel_idx"][t]) and torch.equal(out["trace"][t], full["trace"][t])
    with pytest.raises(ValueError):
        gp_ops.ipv_pool(b, phi, X[:, :4].contiguous(), targets=tgt, q=3)
    with pytest.raises(RuntimeError):
        gp_ops.ipv_pool(b, phi, X.cpu(), targets=tgt, q=3)


def test_select_support_on_a_model(dev):
    """evaluate.select_support: the fit is meta_test's, and the picks, their scores and tvar meet the reference at the fitted phi
    on the model's own features (assertions 2-4 and tvar; the call returns no trace)."""
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
    lib_rows = Z_q[2, :130].detach().float().contiguous()          # a library in the model's feature space
    _, _, phi_ref, _ = E.meta_test(model, mb, streaming=True)
    targets = [[1, 5, 9, 77], [0, 2, 129, 64], [3, 4, 5, 6]]
    sel_idx, sel_val, tvar, phi = E.select_support(model, mb, lib_rows, targets, 5, exclude=targets)
    assert torch.equal(phi, phi_ref) and sel_idx.shape == (3, 5) and sel_idx.dtype == torch.int64 and tvar.shape == (3, 6)
    si, sv, tv, Xh, ph = sel_idx.cpu().numpy(), sel_val.cpu().numpy(), tvar.cpu().numpy(), lib_rows.cpu().numpy(), phi.cpu().numpy()
    for t, n in enumerate(mb.n_s.tolist()):
        post = R.posterior(Z_s[t, :n].detach().float().cpu(), y_s[t, :n].float().cpu(), Xh, ph[t], gp_ops.kernel_id("matern"))
        worst = R.check_task(post, targets[t], None, si[t], sv[t], tv[t], None, excluded=targets[t], tag=("select_support", t))
        print(f"select_support task {t}: picks {si[t].tolist()}, worst error / bound {worst:.3f}")
        assert (si[t] >= 0).all() and not set(si[t].tolist()) & set(targets[t])


def test_the_active_learning_loop(dev, monkeypatch):
    """Records without repeats or targets, and within each round's call a target variance that only falls."""
    from adkf_ift_amd import bayes_opt as BO
    from adkf_ift_amd import gp_ops

    g = torch.Generator().manual_seed(5)
    X = torch.randn(400, 6, generator=g)
    y = torch.sin(X[:, :3].sum(1)) + 0.05 * torch.randn(400, generator=g)
    X, y = X.to(dev), y.to(dev)
    targets = [3, 50, 51, 120, 399]
    calls = []
    real = gp_ops.ipv_pool

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append(out)
        return out

    monkeypatch.setattr(gp_ops, "ipv_pool", spy)
    recs = BO.run_gp_ipv_al_batched(X, y, targets, num_init_points=6, query_batch_size=4, num_rounds=3, kernel_type="matern", device=dev,
                                    init_from=0, noise_init=0.01, noise_prior=True, rngs=[np.random.default_rng(s) for s in range(2)])
    assert len(recs) == 2 and len(calls) == 3
    for rec in recs:
        assert len(rec) == 12 and len(set(rec)) == 12 and not set(rec) & set(targets)
    for out in calls:
        tv = out["tvar"].cpu()
        assert bool((tv[:, 1:] <= tv[:, :-1]).all()) and bool((tv > 0).all()), tv.tolist()
        assert bool((out["sel_idx"] >= 0).all())
