"""GPU: leave-one-out checks and jackknife+ intervals over a shared pool (adkf_jackknife_pool / gp_ops.jackknife_pool) - every row,
level and form and the selection against the float64 reference (jackknife_ref.py) on every path of the walk, mixed kinds and an ARD
batch, the closed forms against deleting each point ON THE DEVICE, exact order properties, determinism and independence of the
batch, more tasks than workgroups, the edge cases, and the two callers in evaluate."""
import numpy as np
import pytest
import torch

import jackknife_ref as R
import test_gpu_believer_pool as B
import test_gpu_believer_pool_ard as BA
import test_gpu_predict_marginal as M
import test_gpu_predict_pool as P

pytestmark = pytest.mark.gpu

LEVELS = (0.1, 0.25)
NAMES = ("lo", "hi", "loo_mean", "loo_var", "loo_lpd", "top_idx", "top_val")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


_states = {}


def _states_of(key, b, phi, Zs, ys, n_s, X, state_fn=R.state):
    """The float64 reference state of every task, once per problem."""
    if key not in _states:
        Xh, ph = X.cpu().numpy(), phi.cpu().numpy()
        _states[key] = [state_fn(np.asarray(Zs[t, :n_s[t]]), np.asarray(ys[t, :n_s[t]]), Xh, ph[t], b.kernel) for t in range(b.T)]
    return _states[key]


def _check_device(out, states, alphas, scaled, maximize, tag, lists=None):
    """jackknife_ref.check_task on every task of a call; returns the worst error / bound."""
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    h = {k: None if out[k] is None else out[k].cpu().numpy() for k in NAMES}
    worst = 0.0
    for t, st in enumerate(states):
        loo = None if h["loo_mean"] is None else (h["loo_mean"][t], h["loo_var"][t], h["loo_lpd"][t])
        w = R.check_task(st, alphas, scaled, maximize, None if h["lo"] is None else h["lo"][t], None if h["hi"] is None else h["hi"][t], loo,
                         None if h["top_idx"] is None else h["top_idx"][t], None if h["top_val"] is None else h["top_val"][t],
                         excluded=lists[t] if lists else (), tag=(tag, t))
        worst = max(worst, w)
    print(f"{tag}: worst error / bound {worst:.4f}")
    return worst


CASES = [  # (kernel, n_s, d, rows): the smallest shapes that reach each path
    ("matern", [48, 45, 31], 16, 300),      # one panel, plain
    ("rbf", [128, 125, 85], 64, 37),        # two panels, a partial tile
    ("rbf", [200, 197, 133], 64, 133),      # refined, beyond 128
    ("matern", [256, 19, 3], 12, 70),       # the size limit; k = 1 and k = 0 tasks in one batch
]


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("kernel,n_s,d,rows", CASES)
def test_against_the_reference(dev, kernel, n_s, d, rows, scaled):
    from adkf_ift_amd import gp_ops

    seed = 500 + max(n_s)
    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, rows, seed)
    states = _states_of((kernel, tuple(n_s), d, rows, seed), b, phi, Zs, ys, n_s, X)
    lists = [[0, 7], [], [3, 11, 12]]
    for maximize in (False, True):
        out = gp_ops.jackknife_pool(b, phi, X, alpha=LEVELS, scaled=scaled, maximize=maximize, topk=8, exclude=lists)
        _check_device(out, states, LEVELS, scaled, maximize, (kernel, max(n_s), "scaled" if scaled else "plain", maximize), lists)
        for t, n in enumerate(n_s):
            if R.rank(LEVELS[0], n) == 0:   # no rank at level 0: the infinities, and nothing is selected
                assert bool(torch.isneginf(out["lo"][t, 0]).all()) and bool(torch.isposinf(out["hi"][t, 0]).all())
                assert bool((out["top_idx"][t] == -1).all()) and bool(torch.isneginf(out["top_val"][t]).all())
            else:
                assert bool((out["top_idx"][t] >= 0).all())


def _mixed(dev):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, _ = P._ill_batch(dev)
    # what the mixed test rests on, from the fitted scalars: a task on k_jk_walk64 and a task on a float32 walk
    kinds = [M._path(sc) for sc in M._scalars(b)]
    assert 2 in kinds and min(kinds) < 2, kinds
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.cat([P._pool(300, 2, 3), b.Z_s[1, :5].cpu()]).to(dev)
    return b, phi, Zs, ys, n_s, X


@pytest.mark.parametrize("scaled", [False, True])
def test_mixed_kinds_in_one_call(dev, scaled):
    """test_gpu_predict_pool._ill_batch: task 1 takes the float64 walk (asserted from the fitted scalars), the others a float32 one."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X = _mixed(dev)
    states = _states_of("mixed", b, phi, Zs, ys, n_s, X)
    alphas = (0.1, 0.25, 0.4)
    out = gp_ops.jackknife_pool(b, phi, X, alpha=alphas, scaled=scaled, maximize=True, topk=8)
    _check_device(out, states, alphas, scaled, True, ("mixed", scaled))


@pytest.mark.parametrize("scaled", [False, True])
def test_an_ard_batch(dev, scaled):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, _ = BA.CASES[0]
    b, phi, Zs, ys, n_s, X, _ = BA._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    states = _states_of("ard", b, phi, Zs.numpy(), ys, n_s, X, state_fn=R.ard_state)
    alphas, lists = (0.2, 0.4), [[1], [], [0, 5]]   # (n_s = 5, 4, 3: ranks 1, 1, 0 and 2, 2, 1)
    out = gp_ops.jackknife_pool(b, phi, X, alpha=alphas, scaled=scaled, topk=8, exclude=lists)
    _check_device(out, states, alphas, scaled, False, ("ard", scaled), lists)


@pytest.mark.parametrize("scaled", [False, True])
def test_deletion_on_the_device_itself(dev, scaled):
    """One task of 12 points; a second batch of 12 tasks, task i the set without point i, through predict_pool over X and the 12
    support rows: mu_-i(x), v_-i(x), g_i = y_i - mu_-i(z_i) and the observed variance at z_i from THOSE calls, put through the
    definitions in float64, reproduce lo / hi / loo_* of the one jackknife call within jackknife_ref's bounds (formed from the
    device's own numbers).  Independent of the reference's closed forms: a wrong sign, rank or identity fails here."""
    from adkf_ift_amd import gp_ops

    n, d, rows = 12, 6, 50
    Zs, ys, _ = M._features(1, n, [0], d, 901, True)
    X = P._pool(rows, d, 902).to(dev)
    b = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.empty(1, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    phi = phi0.clone()
    phi[0, 0], phi[0, 1] = -2.0, 0.2
    alphas = (0.1, 0.25, 0.45)
    out = gp_ops.jackknife_pool(b, phi, X, alpha=alphas, scaled=scaled)
    gp_ops.check_info(out["info"])
    keep = [[j for j in range(n) if j != i] for i in range(n)]
    Zd = torch.stack([Zs[0, k] for k in keep])
    yd = torch.stack([ys[0, k] for k in keep])
    bd = gp_ops.GPBatch(Zd.to(dev), yd.to(dev), b.priors.expand(n, 4).contiguous(), "matern")
    pd = gp_ops.predict_pool(bd, phi.expand(n, 3).contiguous(), torch.cat([X, Zs[0].to(dev)]), latent=True)
    gp_ops.check_info(pd["info"])
    sc = M._scalars(bd)
    noise, os_ = float(sc[0, 0]), float(sc[0, 1])
    mean, var = pd["mean"].double().cpu().numpy(), pd["var"].double().cpu().numpy()      # [n, rows + n]
    y = ys[0].double().numpy()
    mu = mean[:, :rows].T                                                                # [rows, n]: mu_-i(x)
    g = y - mean[np.arange(n), rows + np.arange(n)]
    lvar = var[np.arange(n), rows + np.arange(n)] + noise                                # 1 / B_ii
    Mx = max(1.0, np.abs(y).max(), np.abs(mu).max())
    if scaled:
        s, bii = np.abs(g) / np.sqrt(lvar), 1.0 / lvar
        sd = np.sqrt(np.maximum(var[:, :rows].T, 1e-12) + noise)
        w = s[None, :] * sd
        delta = (R.TOL * Mx + sd * (np.sqrt(bii) * R.TOL * Mx + s * R.TOL * os_ * bii / 2.0) + s * R.TOL * os_ / (2.0 * sd)).max(1)
    else:
        w = np.abs(g)[None, :]
        delta = np.full(rows, 2.0 * R.TOL * Mx)
    sa, sb = np.sort(mu - w, 1), -np.sort(-(mu + w), 1)
    lo, hi = out["lo"][0].double().cpu().numpy(), out["hi"][0].double().cpu().numpy()
    worst = 0.0
    for l, al in enumerate(alphas):
        k = R.rank(al, n)
        assert k == (1, 3, 5)[l]
        e = max((np.abs(lo[l] - sa[:, k - 1]) / delta).max(), (np.abs(hi[l] - sb[:, k - 1]) / delta).max())
        worst = max(worst, float(e))
        assert e <= 1.0, (scaled, l, k, float(e))
    e_mean = np.abs(out["loo_mean"][0].double().cpu().numpy() - (y - g)).max() / (R.TOL * Mx)
    e_var = np.abs(out["loo_var"][0].double().cpu().numpy() - lvar).max() / (R.TOL * os_)
    lpd = float(np.sum(-0.5 * np.log(2.0 * np.pi * lvar) - 0.5 * g * g / lvar))
    b_lpd = float(np.sum(np.abs(g) / lvar * R.TOL * Mx + 0.5 * np.abs(g * g / lvar ** 2 - 1.0 / lvar) * R.TOL * os_))
    e_lpd = abs(float(out["loo_lpd"][0]) - lpd) / b_lpd
    print(f"deletion on the device, scaled={scaled}: worst error / bound {worst:.4f} (intervals), {e_mean:.4f} {e_var:.4f} {e_lpd:.4f} (loo)")
    assert e_mean <= 1.0 and e_var <= 1.0 and e_lpd <= 1.0, (e_mean, e_var, e_lpd)


@pytest.mark.parametrize("scaled", [False, True])
def test_exact_properties(dev, scaled):
    """lo non-decreasing and hi non-increasing in alpha, lo <= hi below one half, a repeated level gives equal bits - no tolerance;
    y -> -y mirrors the interval within delta."""
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows = CASES[0]
    seed = 500 + max(n_s)
    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, rows, seed)
    alphas = (0.05, 0.1, 0.25, 0.1, 0.45, 0.5, 0.8)
    out = gp_ops.jackknife_pool(b, phi, X, alpha=alphas, scaled=scaled)
    lo, hi = out["lo"], out["hi"]
    order = [0, 1, 2, 4, 5, 6]   # ascending levels
    for p, q in zip(order[:-1], order[1:]):
        assert bool((lo[:, p] <= lo[:, q]).all()) and bool((hi[:, p] >= hi[:, q]).all()), (p, q)
    for l in (0, 1, 2, 4):
        assert bool((lo[:, l] <= hi[:, l]).all()), l
    assert torch.equal(lo[:, 1], lo[:, 3]) and torch.equal(hi[:, 1], hi[:, 3])
    # the mirror image
    bm = gp_ops.GPBatch(b.Z_s, (-b.y_s).contiguous(), b.priors, kernel, n_s=torch.tensor(n_s, dtype=torch.int32))
    om = gp_ops.jackknife_pool(bm, phi, X, alpha=alphas, scaled=scaled)
    states = _states_of((kernel, tuple(n_s), d, rows, seed), b, phi, Zs, ys, n_s, X)
    for t, st in enumerate(states):
        delta = R.jackknife_ref(st, alphas, scaled)[2]
        err = max(float(((om["lo"][t] + hi[t]).abs().double().cpu().numpy() / delta).max()),
                  float(((om["hi"][t] + lo[t]).abs().double().cpu().numpy() / delta).max()))
        assert err <= 1.0, (t, err)
    print(f"y -> -y, scaled={scaled}: lo' == -hi bit for bit: {torch.equal(om['lo'], -hi)}; hi' == -lo: {torch.equal(om['hi'], -lo)}")


def test_deterministic_and_independent_of_the_batch(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows = CASES[0]
    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    lists = [[0, 7], [], [3]]
    for scaled in (False, True):
        kw = dict(alpha=LEVELS, scaled=scaled, maximize=True, topk=8)
        first = gp_ops.jackknife_pool(b, phi, X, exclude=lists, **kw)
        again = gp_ops.jackknife_pool(b, phi, X, exclude=lists, **kw)
        for name in NAMES:
            assert torch.equal(first[name], again[name]), name
        sel = gp_ops.jackknife_pool(b, phi, X, exclude=lists, want_lo=False, want_hi=False, want_loo=False, **kw)   # null outputs: the same selection
        assert sel["lo"] is None and torch.equal(sel["top_idx"], first["top_idx"]) and torch.equal(sel["top_val"], first["top_val"])
        for t in range(b.T):   # each task alone in a T = 1 batch
            n = n_s[t]
            b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), kernel,
                                n_s=torch.tensor([n], dtype=torch.int32))
            o1 = gp_ops.jackknife_pool(b1, phi[t:t + 1].contiguous(), X, exclude=[lists[t]], **kw)
            for name in NAMES:
                assert torch.equal(o1[name][0], first[name][t]), (t, name)


def test_more_tasks_than_workgroups(dev):
    """T = 300 tiny tasks, n_s in 3 .. 8 (test_gpu_believer_pool's construction): every task against the reference."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows = 300, 8, 4, 130
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
    alphas = (0.25, 0.4)
    states = _states_of("T300", b, phi, Zs, ys, n_s, X)
    out = gp_ops.jackknife_pool(b, phi, X, alpha=alphas, scaled=True, maximize=True, topk=3)
    _check_device(out, states, alphas, True, True, "T300")


def test_edge_cases(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows = CASES[0]
    seed = 500 + max(n_s)
    b, phi, Zs, ys, n_s, X, _ = B._explicit(dev, kernel, n_s, d, rows, seed)
    T = b.T
    full = gp_ops.jackknife_pool(b, phi, X, alpha=LEVELS, topk=4)
    # rows = 0: the leave-one-out diagnostic alone, the same bits; gp_ops.loo is that call
    none = gp_ops.jackknife_pool(b, phi, X[:0], alpha=LEVELS, topk=4)
    assert none["lo"].shape == (T, 2, 0) and bool((none["top_idx"] == -1).all()) and bool(torch.isneginf(none["top_val"]).all())
    loo = gp_ops.loo(b, phi)
    for name in ("loo_mean", "loo_var", "loo_lpd"):
        assert torch.equal(none[name], full[name]) and torch.equal(loo[name], full[name]), name
    states = _states_of((kernel, tuple(n_s), d, 0, seed), b, phi, Zs, ys, n_s, X[:0])
    _check_device(dict(none, lo=None, hi=None, top_idx=None, top_val=None), states, LEVELS, False, False, "rows = 0")
    # every row excluded; rows < k
    out = gp_ops.jackknife_pool(b, phi, X[:5], alpha=LEVELS, topk=3, exclude=[list(range(5))] * T)
    assert bool((out["top_idx"] == -1).all()) and bool(torch.isneginf(out["top_val"]).all())
    out = gp_ops.jackknife_pool(b, phi, X[:5], alpha=LEVELS, topk=8)
    si = out["top_idx"].cpu()
    for t in range(T):
        assert sorted(si[t, :5].tolist()) == list(range(5)) and bool((si[t, 5:] == -1).all())
    assert bool(torch.isneginf(out["top_val"][:, 5:]).all())
    assert torch.equal(out["lo"], full["lo"][:, :, :5]) and torch.equal(out["hi"], full["hi"][:, :, :5])
    # a task with info != 0 (a NaN noise) among healthy ones, whose bits do not move
    phib = phi.clone()
    phib[1, 0] = float("nan")
    out = gp_ops.jackknife_pool(b, phib, X, alpha=LEVELS, topk=4)
    info = out["info"].cpu()
    assert int(info[1]) != 0 and int(info[0]) == 0 and int(info[2]) == 0, info.tolist()
    for name in NAMES[:5]:
        assert bool((out[name][1] == 0).all()), name
    assert bool((out["top_idx"][1] == -1).all()) and bool(torch.isneginf(out["top_val"][1]).all())
    for t in (0, 2):
        for name in NAMES:
            assert torch.equal(out[name][t], full[name][t]), (t, name)
    with pytest.raises(ValueError):
        gp_ops.jackknife_pool(b, phi, X[:, :4].contiguous(), alpha=LEVELS)
    with pytest.raises(RuntimeError):
        gp_ops.jackknife_pool(b, phi, X.cpu(), alpha=LEVELS)


def test_the_callers_on_a_model(dev):
    """evaluate.predict_intervals and loo_check: the fit is meta_test's, and the intervals, the selection and the leave-one-out
    outputs meet the reference at the returned phi on the model's own features."""
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
    lo, hi, top_idx, top_val, phi = E.predict_intervals(model, mb, lib_rows, alpha=0.1, k=5)
    loo_mean, loo_var, loo_lpd, phi2 = E.loo_check(model, mb)
    assert torch.equal(phi, phi_ref) and torch.equal(phi2, phi_ref) and lo.shape == (3, 1, 130) and top_idx.shape == (3, 5)
    Xh, ph = lib_rows.cpu().numpy(), phi.cpu().numpy()
    h = lambda x: x.cpu().numpy()
    for t, n in enumerate(mb.n_s.tolist()):
        st = R.state(Z_s[t, :n].detach().float().cpu().numpy(), y_s[t, :n].float().cpu().numpy(), Xh, ph[t], gp_ops.kernel_id("matern"))
        worst = R.check_task(st, (0.1,), True, True, h(lo[t]), h(hi[t]), (h(loo_mean[t]), h(loo_var[t]), h(loo_lpd[t])), h(top_idx[t]),
                             h(top_val[t]), tag=("callers", t))
        print(f"predict_intervals / loo_check task {t}: picks {h(top_idx[t]).tolist()}, worst error / bound {worst:.4f}")
