"""GPU: level-set estimation and batch UCB over a shared pool (adkf_levelset_pool / gp_ops.levelset_pool) - the epilogue alone at the
call's own float32 mean and variance, every step's scores, pick, class counts and hits against the float64 reference conditioned on
the device's own earlier picks (levelset_ref.py) on every task kind, an ARD batch and the float64 walk, the bitwise properties of the
call (deterministic, grid- and batch-independent, invariant under a permutation of the pool), hits against its own trace, small
pools and edge cases, and the Python layers (evaluate.find_actives, the LSE and GP-BUCB loops)."""
import numpy as np
import pytest
import torch

import levelset_ref as R
import test_gpu_believer_pool as BV
import test_gpu_believer_pool_ard as BVA
import test_gpu_gibbon_pool as GB
import test_gpu_log_ei as L
import test_gpu_predict_marginal as M
import test_gpu_predict_pool as P
from test_levelset_pool_cpu import _ls_twin, ls_call

pytestmark = pytest.mark.gpu

SCORES = ("straddle", "prob", "bound")
EPS32 = R.EPS32
RANGE_NAMES = ("z > 0", "-1 < z <= 0", "-16 < z <= -1", "z <= -16")
KEYS = ("sel_idx", "sel_val", "sel_mean", "sel_var", "counts", "hits", "cls", "trace")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _eq(x, y):
    """bit-equal tensors (NaN payloads included)"""
    if x is None or y is None:
        return x is None and y is None
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)


def _same_out(a, c, t=None, u=None, keys=KEYS):
    for k in keys:
        x, y = (a[k], c[k]) if t is None or a[k] is None else (a[k][t], c[k][u])
        assert _eq(x, y), (k, t)


def _call(b, phi, X, tau, beta, score, q, maximize=False, exclude=None, **kw):
    from adkf_ift_amd import gp_ops
    kw = dict(dict(want_trace=True, want_cls=True), **kw)
    return gp_ops.levelset_pool(b, phi, X, tau=tau, beta=beta, q=q, score=score, maximize=maximize, exclude=exclude, **kw)


@pytest.mark.parametrize("kernel,ns,d", L.SHAPES)
def test_the_epilogue_alone(dev, kernel, ns, d):
    """Step 0 of a q = 1 call against float64 at the call's OWN float32 mean and latent variance (predict_pool on the same batch: the
    same tile arithmetic), sigma and z formed in float64 from them with the kernel's float32 clamp, which leaves the GP's float32
    error out.  777 rows: a partial last tile; the pool holds task 0's support rows: small variances, large |z|, decided rows.
      STRADDLE   |got - ref| <= 4 eps32 (beta sigma + |m - tau|): one rounding each for the root, the difference and the fused
                 multiply-add, plus one ulp of sqrtf.
      BOUND      |got - ref| <= 4 eps32 (beta sigma + |m|): the same count with the mean in the place of the difference - the score has
                 no difference, its fused multiply-add rounds a value of size |+-m + beta sigma|, which |m - tau| says nothing about.
      PROB       per range of z, in units of eps32 (1 + z^2): the device's worst ratio is at most 4 x that of a plain numpy-float32
                 evaluation of the same formula from the same float32 mean and variance (levelset_ref.prob_f32), computed here;
                 the 4 allows for the device's erfcf / erfcxf / logf differing from the host's by a few ulps each.  Both are printed.
    tau is shifted per case so that every range is reached, below log Phi = -32 too, where the Gumbel function clamps."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    T, ROWS = L.T, L.ROWS
    pp = gp_ops.predict_pool(b, phi, Xc, latent=True)
    gp_ops.check_info(pp["info"])
    mean, var = pp["mean"].cpu().numpy(), pp["var"].cpu().numpy()
    beta = 1.0
    yard, devr, count = np.zeros(4), np.zeros(4), np.zeros(4, int)
    lowest = 0.0
    for maximize, shift in ((True, 0.0), (False, 0.0), (True, 30.0), (False, -30.0)):
        tau = (np.median(mean, axis=1) + shift).astype(np.float32)
        outs = {s: _call(b, phi, Xc, torch.from_numpy(tau).to(dev), beta, s, 1, maximize=maximize) for s in SCORES}
        for s in SCORES:
            gp_ops.check_info(outs[s]["info"])
        got = {s: outs[s]["trace"][:, 0].cpu().numpy().astype(np.float64) for s in SCORES}
        for t in range(T):
            m, v = mean[t].astype(np.float64), var[t].astype(np.float64)
            sg = np.sqrt(np.maximum(v, L.CLAMP32))
            score, straddle, cls, z, _ = R.rows_ref(m, sg * sg, float(tau[t]), beta, R.PROB, maximize)
            err = np.abs(got["straddle"][t] - straddle) / (4 * EPS32 * (beta * sg + np.abs(m - float(tau[t]))))
            assert err.max() <= 1.0, ("straddle", maximize, shift, t, float(err.max()))
            bound = (m if maximize else -m) + beta * sg
            err = np.abs(got["bound"][t] - bound) / (4 * EPS32 * (beta * sg + np.abs(m)))
            assert err.max() <= 1.0, ("bound", maximize, shift, t, float(err.max()))
            assert np.isfinite(got["prob"][t]).all()
            host32, z32 = R.prob_f32(mean[t], var[t], tau[t], maximize)
            unit = EPS32 * (1.0 + z * z)
            rg = R.range_of(z)
            for k in range(4):
                sel = rg == k
                if sel.any():
                    yard[k] = max(yard[k], float((np.abs(host32[sel].astype(np.float64) - score[sel]) / unit[sel]).max()))
                    devr[k] = max(devr[k], float((np.abs(got["prob"][t][sel] - score[sel]) / unit[sel]).max()))
                    count[k] += int(sel.sum())
            lowest = min(lowest, float(score.min()))
    print(f"{kernel}: log Phi, worst error in units of eps32 (1 + z^2) per range {RANGE_NAMES}: numpy float32 {yard.round(3).tolist()}, "
          f"device {devr.round(3).tolist()}, rows {count.tolist()}, lowest log Phi {lowest:.1f}")
    assert (count > 0).all(), count          # every range of the evaluation was reached
    assert lowest < -32.0                    # and the region where pm_neg_log_cdf clamps
    assert (devr <= 4.0 * yard).all(), (devr.tolist(), yard.tolist())


def _seeded(X, Zs, n_s, dev):
    """The pool with its first rows overwritten by support rows of every task (8 each) and as many jittered copies: decided rows."""
    Xd = X.clone()
    sup = torch.cat([Zs[t, :min(8, n_s[t])] for t in range(len(n_s))]).to(dev)
    k = min(sup.shape[0], X.shape[0] // 4)
    g = torch.Generator().manual_seed(3)
    Xd[:k] = sup[:k]
    Xd[k:2 * k] = sup[:k] + 0.15 * torch.randn(k, X.shape[1], generator=g).to(dev)
    return Xd.contiguous()


def _lists(rows, T):
    base = [[0, 7, rows - 1], [], [3, 5]]
    return [base[t % 3] for t in range(T)]


def _check_device(out, posts, tau, beta, score, maximize, tag, lists, tally):
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    h = {k: out[k].cpu().numpy() for k in KEYS}
    worst_all = 0.0
    for t, post in enumerate(posts):
        worst = R.check_task(post, tau[t], beta, SCORES.index(score), maximize, h["sel_idx"][t], h["sel_val"][t], h["sel_mean"][t], h["sel_var"][t],
                             h["trace"][t], counts=h["counts"][t], hits=h["hits"][t], excluded=lists[t], tally=tally, tag=(tag, t))
        worst_all = max(worst_all, worst)
        assert np.array_equal(np.bincount(h["cls"][t].astype(np.int64), minlength=3), h["counts"][t, 0]), (tag, t)
    print(f"{tag}: picks of task 0 {h['sel_idx'][0].tolist()}, counts {h['counts'][0, 0].tolist()} -> {h['counts'][0, -1].tolist()}, "
          f"worst trace error / bound {worst_all:.3f}")
    return h


def _check_twin(b, Zs, ys, n_s, X, phi, posts, tau, beta, score, maximize, q, lists, tag, ard=False):
    """The twin meets the same assertions on this shape (so that a miss of the device is the device's)."""
    from oracle import cpu_twin
    from test_levelset_pool_cpu import excl_lists

    fn = _ls_twin()
    T = len(n_s)
    hb = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((T, 4), np.float32), b.kernel, n_s=np.array(n_s, np.int32))
    if ard:
        hb.c.flags = 4
    Xh, ph = np.ascontiguousarray(X.cpu().numpy()), np.ascontiguousarray(phi.cpu().numpy())
    out = ls_call(fn, hb, ph, 2 if maximize else 0, Xh, tau, beta, SCORES.index(score), q, excl=excl_lists(lists))
    for t in range(T):
        R.check_task(posts[t], tau[t], beta, SCORES.index(score), maximize, out["sel_idx"][t], out["sel_val"][t], out["sel_mean"][t],
                     out["sel_var"][t], out["trace"][t], counts=out["counts"][t], hits=out["hits"][t], excluded=lists[t], tag=(tag, "twin", t))


def _every_step(dev, b, phi, Zs, ys, n_s, X, tag, ard=False, twin=True, q=8, beta=0.5):
    posts = GB._post_of(b, phi, Zs, ys, n_s, X, ard=ard)
    tau = np.array([np.median(p[0]) for p in posts], np.float32)
    lists = _lists(X.shape[0], len(n_s))
    tally = R.new_tally()
    classes = np.zeros(3, np.int64)
    for maximize in (False, True):
        for score in SCORES:
            if twin and maximize == (score == "prob"):   # (each score once, both senses between them)
                _check_twin(b, Zs, ys, n_s, X, phi, posts, tau, beta, score, maximize, q, lists, tag, ard=ard)
            out = _call(b, phi, X, torch.from_numpy(tau).to(dev), beta, score, q, maximize=maximize, exclude=lists)
            h = _check_device(out, posts, tau, beta, score, maximize, (tag, score, maximize), lists, tally)
            classes += h["counts"][:, 0].sum(0)
            for t in range(len(n_s)):
                got = [p for p in h["sel_idx"][t].tolist() if p >= 0]
                assert len(got) == q and len(set(got)) == q and not set(got) & set(lists[t])
    print(f"{tag}: band rows / rows compared {tally}, rows per class at step 0 {classes.tolist()}")
    R.assert_tally(tally)
    assert (classes > 0).all(), classes


CASES = [  # (kernel, n_s, d, rows, twin too): the believer's shapes
    ("matern", [48, 45, 31], 16, 300, True),        # plain, one panel
    ("rbf", [200, 197, 133], 64, 333, True),        # refined, LDS tiles
    ("matern", [1024, 700], 12, 130, False),        # global slots
]


@pytest.mark.parametrize("kernel,n_s,d,rows,twin", CASES)
def test_every_step_against_the_reference(dev, kernel, n_s, d, rows, twin):
    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    _every_step(dev, b, phi, Zs, ys, n_s, _seeded(X, Zs, n_s, dev), (kernel, max(n_s)), twin=twin)


def test_every_step_on_an_ard_batch(dev):
    b, phi, Zs, ys, n_s, X, _ = BVA._explicit(dev, "matern", [48, 45, 31], 12, 300, 548)
    _every_step(dev, b, phi, Zs, ys, n_s, _seeded(X, Zs, n_s, dev), "ard", ard=True)


def test_every_step_with_the_float64_walk(dev):
    """test_gpu_predict_pool._ill_batch: task 1 takes the float64 walk, the others a float32 one - both kernels of the walk in one call.
    The pool ends in task 1's support rows."""
    b, phi, Zs, ys, n_s, X = GB._ill(dev)
    try:
        _every_step(dev, b, phi, Zs, ys, n_s, X, "mixed", twin=False)
    finally:
        b.flags = 0


def test_bitwise_properties(dev):
    """Deterministic over two runs; outputs not asked for change nothing; step 0 of a q = 8 call is the q = 1 call; the undecided count
    is the number of positive entries of a STRADDLE trace; step-0 counts, hits and cls do not depend on the score; STRADDLE and BOUND
    traces and the undecided count never rise; a task alone is the task in the batch; a permuted pool gives the same counts and hits
    bits and the picks mapped through the permutation - on the plain and refined float32 walks and with the float64 walk."""
    from adkf_ift_amd import gp_ops

    problems = []
    for kernel, n_s, d, rows, _ in CASES[:2]:
        b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
        problems.append((b, phi, Zs, ys, n_s, _seeded(X, Zs, n_s, dev), True))
    b64 = GB._ill(dev)
    problems.append(b64 + (False,))
    try:
        for b, phi, Zs, ys, n_s, X, alone in problems:
            T, rows, q, beta = b.T, X.shape[0], 8, 0.5
            pp = gp_ops.predict_pool(b, phi, X, latent=True)
            tau = pp["mean"].median(dim=1).values.contiguous()
            tau_hi = (pp["mean"].max(dim=1).values + 0.25).contiguous()
            lists = _lists(rows, T)
            kw = dict(maximize=True, exclude=lists)
            outs = {s: _call(b, phi, X, tau, beta, s, q, **kw) for s in SCORES}
            perm = torch.randperm(rows, generator=torch.Generator().manual_seed(11))
            inv = torch.argsort(perm)
            lists_p = [sorted(int(inv[i]) for i in l) for l in lists]
            permd = perm.to(dev)
            for s in SCORES:
                first = outs[s]
                _same_out(first, _call(b, phi, X, tau, beta, s, q, **kw))
                bare = _call(b, phi, X, tau, beta, s, q, want_trace=False, want_cls=False, want_counts=False, **kw)
                assert bare["trace"] is None and bare["cls"] is None and bare["counts"] is None and bare["hits"] is None
                _same_out(first, bare, keys=KEYS[:4])
                one = _call(b, phi, X, tau, beta, s, 1, **kw)
                for k in KEYS[:6] + ("trace",):
                    assert _eq(one[k][:, 0], first[k][:, 0]), (s, k)
                assert _eq(one["cls"], first["cls"])
                assert _eq(first["counts"][:, 0], outs["straddle"]["counts"][:, 0]) and _eq(first["hits"][:, 0], outs["straddle"]["hits"][:, 0])
                assert _eq(first["cls"], outs["straddle"]["cls"])
                assert bool((first["counts"].sum(-1) == rows).all())
                assert bool((first["counts"][:, 1:, 2] <= first["counts"][:, :-1, 2]).all()), s
                if s != "prob":
                    assert bool((first["trace"][:, 1:] <= first["trace"][:, :-1]).all()), s
                    assert bool((first["trace"][:, 1:] < first["trace"][:, :-1]).any()), s
                outp = _call(b, phi, X[permd].contiguous(), tau, beta, s, q, maximize=True, exclude=lists_p)
                assert _eq(outp["counts"][:, 0], first["counts"][:, 0]) and _eq(outp["hits"][:, 0], first["hits"][:, 0]), (s, "permutation")
                assert _eq(outp["cls"], first["cls"][:, permd])
                if s == "prob":
                    # at the median the support rows in the pool have z > 14, where float32 log Phi is -0 for all of them: equal scores
                    # go to the lower row index, which a permutation changes.  With tau above every mean no two rows share a score.
                    first = _call(b, phi, X, tau_hi, beta, s, q, **kw)
                    outp = _call(b, phi, X[permd].contiguous(), tau_hi, beta, s, q, maximize=True, exclude=lists_p)
                    assert bool((first["counts"][:, 0, 0] == 0).all()) and bool((first["sel_val"] < 0).all())
                assert _eq(outp["counts"], first["counts"]) and _eq(outp["hits"], first["hits"]), (s, "permutation")
                assert torch.equal(permd[outp["sel_idx"]], first["sel_idx"]), (s, "permutation")
            st = outs["straddle"]
            assert torch.equal(st["counts"][..., 2], (st["trace"] > 0).sum(-1))
            assert torch.equal(st["cls"] == 2, st["trace"][:, 0] > 0)
            if alone:
                for t in range(T):   # each task alone in a T = 1 batch
                    b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), b.kernel,
                                        n_s=torch.tensor([n_s[t]], dtype=torch.int32))
                    o1 = _call(b1, phi[t:t + 1].contiguous(), X, tau[t:t + 1].contiguous(), beta, "straddle", q, maximize=True, exclude=[lists[t]])
                    _same_out(o1, st, 0, t)
        # the float64-walk task alone (both evaluate at phi: no state of a fit is reused)
        b, phi, Zs, ys, n_s, X, _ = problems[-1]
        b.flags = 0
        tau = gp_ops.predict_pool(b, phi, X, latent=True)["mean"].median(dim=1).values.contiguous()
        full = _call(b, phi, X, tau, 0.5, "prob", 8)
        b1 = gp_ops.GPBatch(b.Z_s[1:2].contiguous(), b.y_s[1:2].contiguous(), b.priors[1:2].contiguous(), b.kernel,
                            n_s=torch.tensor([n_s[1]], dtype=torch.int32))
        _same_out(_call(b1, phi[1:2].contiguous(), X, tau[1:2].contiguous(), 0.5, "prob", 8), full, 0, 1)
    finally:
        b64[0].flags = 0


@pytest.mark.parametrize("kernel,ns,d", L.SHAPES)
def test_step_0_is_prediction_where_they_overlap(dev, kernel, ns, d):
    """score = bound with beta = 0 is predict_pool's ranking by the mean, picks and values; step 0 of STRADDLE is the straddle formed in
    numpy float32 from predict_pool's own mean and latent variance (levelset_ref.straddle_f32), within 2 ulps of beta sigma + |m - tau|
    (numpy's root and the device's may differ in the last bit, and the difference is rounded once on either side)."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    lists = _lists(L.ROWS, L.T)
    pp = gp_ops.predict_pool(b, phi, Xc, latent=True)
    tau = pp["mean"].median(dim=1).values.contiguous()
    for maximize in (False, True):
        top = gp_ops.predict_pool(b, phi, Xc, maximize=maximize, score="mean", want_mean=False, want_var=False, topk=8, exclude=lists)
        flat = _call(b, phi, Xc, tau, 0.0, "bound", 8, maximize=maximize, exclude=lists)
        assert torch.equal(flat["sel_idx"], top["top_idx"]) and torch.equal(flat["sel_val"], top["top_val"])
        beta = 1.5
        out = _call(b, phi, Xc, tau, beta, "straddle", 1, maximize=maximize)
        mean, var, got = pp["mean"].cpu().numpy(), pp["var"].cpu().numpy(), out["trace"][:, 0].cpu().numpy()
        for t in range(L.T):
            ref = R.straddle_f32(mean[t], var[t], tau[t].item(), beta).astype(np.float64)
            size = beta * np.sqrt(np.maximum(var[t].astype(np.float64), 1e-12)) + np.abs(mean[t].astype(np.float64) - tau[t].item())
            assert (np.abs(got[t].astype(np.float64) - ref) <= 2 * 2.0 ** -23 * size).all(), (maximize, t)


def test_hits_against_the_calls_own_trace(dev):
    """hits_j of a PROB call against sum_r exp(trace_j[r]) in float64, within levelset_ref.hits_from_trace_bound - the fixed-point
    rounding rows 2^-32 plus the float32 evaluation of Phi and of exp(log Phi), roundings counted there."""
    kernel, n_s, d, rows, _ = CASES[1]
    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    Xd = _seeded(X, Zs, n_s, dev)
    posts = GB._post_of(b, phi, Zs, ys, n_s, Xd)
    for maximize, shift in ((False, 0.0), (True, 0.0), (True, 1.0), (False, 8.0)):
        tau = np.array([np.median(p[0]) + shift for p in posts], np.float32)
        out = _call(b, phi, Xd, torch.from_numpy(tau).to(dev), 1.0, "prob", 8, maximize=maximize)
        tr, hits = out["trace"].cpu().numpy().astype(np.float64), out["hits"].cpu().numpy().astype(np.float64)
        for t in range(len(n_s)):
            for j in range(8):
                want, bound = np.exp(tr[t, j]).sum(), R.hits_from_trace_bound(tr[t, j])
                assert abs(hits[t, j] - want) <= bound, (maximize, shift, t, j, hits[t, j], want, bound)
        print(f"maximize {maximize} shift {shift}: hits at step 0 {hits[:, 0].round(3).tolist()} of {rows} rows, bound {bound:.2e}")


def test_more_tasks_than_workgroups(dev):
    """T = 300 tiny tasks over three tiles, one partial: the assertions of the reference on every task (no trace), counts that cover the
    pool, and three tasks alone are the tasks in the batch."""
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
    X[:ns] = Zs[0].to(dev)
    posts = GB._post_of(b, phi, Zs, ys, n_s, X)
    tau = np.array([np.median(p[0]) for p in posts], np.float32)
    taud = torch.from_numpy(tau).to(dev)
    out = _call(b, phi, X, taud, 0.5, "straddle", q, want_trace=False)
    gp_ops.check_info(out["info"])
    h = {k: out[k].cpu().numpy() for k in KEYS if out[k] is not None}
    tally = R.new_tally()
    for t in range(T):
        R.check_task(posts[t], tau[t], 0.5, R.STRADDLE, False, h["sel_idx"][t], h["sel_val"][t], h["sel_mean"][t], h["sel_var"][t], None,
                     counts=h["counts"][t], hits=h["hits"][t], tally=tally, tag=("T300", t))
        assert (h["sel_idx"][t] >= 0).all() and len(set(h["sel_idx"][t].tolist())) == q
    R.assert_tally(tally)
    for t in (0, 151, 299):
        b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), "matern",
                            n_s=torch.tensor([n_s[t]], dtype=torch.int32))
        o1 = _call(b1, phi[t:t + 1].contiguous(), X, taud[t:t + 1].contiguous(), 0.5, "straddle", q, want_trace=False)
        _same_out(o1, out, 0, t)


def test_small_pools_and_edge_cases(dev):
    from adkf_ift_amd import gp_ops

    T, d = 3, 16
    b, phi, Zs, ys, n_s, X300, _ = BV._explicit(dev, "matern", [48, 45, 31], d, 300, 548)
    Xd = _seeded(X300, Zs, n_s, dev)
    posts = GB._post_of(b, phi, Zs, ys, n_s, Xd)
    tau = np.array([np.median(p[0]) for p in posts], np.float32)
    taud = torch.from_numpy(tau).to(dev)
    # 1 row and the sizes around a tile: the picks are the pool's rows, then the -1 / -inf / 0 / 0 tail; the counts go on covering the pool
    for rows in (1, 63, 64, 65):
        q = 4 if rows > 1 else 3
        for s in SCORES:
            out = _call(b, phi, Xd[:rows].contiguous(), taud, 0.5, s, q)
            gp_ops.check_info(out["info"])
            assert bool((out["counts"].sum(-1) == rows).all()), (rows, s)
            assert torch.equal(out["counts"][:, 0], torch.stack([torch.bincount(out["cls"][t].long(), minlength=3) for t in range(T)]))
            n = min(rows, q)
            assert bool((out["sel_idx"][:, :n] >= 0).all()) and bool((out["sel_idx"][:, n:] == -1).all()) and bool(torch.isneginf(out["sel_val"][:, n:]).all())
            assert bool((out["sel_mean"][:, n:] == 0).all()) and bool((out["sel_var"][:, n:] == 0).all())
            full = _call(b, phi, Xd, taud, 0.5, s, 1)
            assert _eq(out["trace"][:, 0], full["trace"][:, 0, :rows].contiguous()) and _eq(out["cls"], full["cls"][:, :rows].contiguous()), (rows, s)
    # every row excluded: no pick, and the counts are what they are without the exclusion
    free = _call(b, phi, Xd[:65].contiguous(), taud, 0.5, "straddle", 3)
    out = _call(b, phi, Xd[:65].contiguous(), taud, 0.5, "straddle", 3, exclude=[list(range(65)), [], list(range(64))])
    assert bool((out["sel_idx"][0] == -1).all()) and bool(torch.isneginf(out["sel_val"][0]).all()) and out["sel_idx"][2].tolist() == [64, -1, -1]
    assert _eq(out["counts"][:, 0], free["counts"][:, 0]) and _eq(out["hits"][:, 0], free["hits"][:, 0]) and _eq(out["cls"], free["cls"])
    assert _eq(out["counts"][0, 1:], free["counts"][0, :1].expand(2, 3).contiguous())   # no pick: the state stays
    _same_out(out, free, 1, 1)
    # an empty pool
    out = _call(b, phi, Xd[:0].contiguous(), taud, 0.5, "prob", 3)
    assert bool((out["sel_idx"] == -1).all()) and bool((out["counts"] == 0).all()) and bool((out["hits"] == 0).all()) and out["cls"].shape == (T, 0)
    # a NaN tau, a negative beta: that task has no pick, NaN scores, zero counts and cls = -1; the others are unchanged
    full = _call(b, phi, Xd, taud, 0.5, "bound", 4)
    for bad_tau, bad_beta in ((float("nan"), 0.5), (float("inf"), 0.5), (0.0, -1.0), (0.0, float("nan"))):
        t2, b2 = taud.clone(), torch.full((T,), 0.5, device=dev)
        t2[1] = bad_tau if bad_tau != 0.0 else t2[1]
        b2[1] = bad_beta
        out = _call(b, phi, Xd, t2, b2, "bound", 4)
        assert bool((out["sel_idx"][1] == -1).all()) and bool(torch.isneginf(out["sel_val"][1]).all()) and bool(torch.isnan(out["trace"][1]).all())
        assert bool((out["counts"][1] == 0).all()) and bool((out["hits"][1] == 0).all()) and bool((out["cls"][1] == -1).all())
        for t in (0, 2):
            _same_out(out, full, t, t)
    with pytest.raises(ValueError):
        _call(b, phi, Xd[:, :4].contiguous(), taud, 0.5, "straddle", 3)
    with pytest.raises(ValueError):
        _call(b, phi, Xd, taud[:2], 0.5, "straddle", 3)


def test_find_actives_on_a_model(dev):
    """evaluate.find_actives on the synthetic model of test_gpu_ipv_pool.test_select_support_on_a_model: the fit is meta_test's, cls
    agrees with counts, hits lies between the decided actives and the pool, and the batch leaves no more rows undecided."""
    from adkf_ift_amd import evaluate as E
    from adkf_ift_amd.meta_batch import collate_meta_batch
    from adkf_ift_amd.models import ADKTModel
    from test_meta_batch import random_task, small_model

    torch.manual_seed(1)
    model = ADKTModel(small_model(True)).to(dev)
    tasks = [random_task(16, 40, 21).to(dev), random_task(13, 9, 22).to(dev), random_task(16, 130, 23).to(dev)]
    mb = collate_meta_batch(tasks).to(dev)
    Z_s, Z_q = E.meta_features(model, mb)
    lib_rows = torch.cat([Z_q[2, :130], Z_s[0, :16], Z_s[2, :16]]).detach().float().contiguous()   # a library in the model's feature space
    rows = lib_rows.shape[0]
    _, _, phi_ref, _ = E.meta_test(model, mb, streaming=True)
    y_s, _ = mb.labels(True)
    tau = torch.stack([y_s[t, :n].float().median() for t, n in enumerate(mb.n_s.tolist())]).to(dev)
    lists = [[1, 5], [], [0]]
    cls, counts, hits, sel_idx, after, phi = E.find_actives(model, mb, lib_rows, tau, beta=1.0, q=5, exclude=lists)
    assert torch.equal(phi, phi_ref) and cls.shape == (3, rows) and cls.dtype == torch.int8 and sel_idx.shape == (3, 5)
    assert counts.shape == (3, 3) and after.shape == (3, 3) and hits.shape == (3,)
    for t in range(3):
        assert torch.equal(torch.bincount(cls[t].long(), minlength=3), counts[t]), t
        assert not set(sel_idx[t].tolist()) & set(lists[t]) and len(set(sel_idx[t].tolist())) == 5 and int(sel_idx[t].min()) >= 0
        assert 0.0 <= float(hits[t]) <= rows
    assert bool((counts.sum(1) == rows).all()) and bool((after.sum(1) == rows).all())
    assert bool((after[:, 2] <= counts[:, 2]).all())
    print("find_actives: counts", counts.tolist(), "after the batch", after.tolist(), "hits", hits.tolist())
    cls0, counts0, _, sel0, after0, _ = E.find_actives(model, mb, lib_rows, tau, beta=1.0)
    assert torch.equal(cls0, cls) and torch.equal(counts0, counts) and torch.equal(after0, counts) and sel0.shape == (3, 0)


def test_the_loops(dev):
    """run_gp_lse_al_batched and run_gp_ucb_bo_batched on a generated pool of 400 rows, 3 replicates, 4 iterations: record lengths, no
    repeats, reproducible, a replicate alone is the replicate in the batch."""
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(3)
    X = torch.randn(400, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    X, y = X.to(dev), y.to(dev)
    kw = dict(num_init_points=6, query_batch_size=3, kernel_type="matern", device=dev, init_from=200, noise_init=0.01, noise_prior=True)
    rngs = lambda n=3: [np.random.default_rng(s) for s in range(n)]
    tau = float(y.median())
    recs, counts = BO.run_gp_lse_al_batched(X, y, tau, num_iters=4, rngs=rngs(), return_counts=True, **kw)
    assert counts.shape == (4, 3, 3) and bool((counts.sum(-1) == 400).all())
    again = BO.run_gp_lse_al_batched(X, y, tau, num_iters=4, rngs=rngs(), **kw)
    ucb = BO.run_gp_ucb_bo_batched(X, y, num_bo_iters=4, rngs=rngs(), **kw)
    for rec in recs + ucb:
        assert len(rec) == 1 + 4 * 3 and len(set(rec[1:])) == 12 and all(0 <= i < 400 for i in rec), rec
    assert recs == again and ucb == BO.run_gp_ucb_bo_batched(X, y, num_bo_iters=4, rngs=rngs(), **kw)
    assert BO.run_gp_lse_al_batched(X, y, tau, num_iters=4, rngs=[np.random.default_rng(2)], **kw)[0] == recs[2]
    assert BO.run_gp_ucb_bo_batched(X, y, num_bo_iters=4, rngs=[np.random.default_rng(2)], ard=True, **kw)[0][0] == ucb[2][0]
    print("undecided rows before each LSE batch:", counts[..., 2].tolist())
    with pytest.raises(ValueError):
        BO.run_gp_ucb_bo_batched(X, y, num_bo_iters=1, rngs=rngs(1), **dict(kw, query_batch_size=65))
