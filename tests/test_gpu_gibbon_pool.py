"""GPU: GIBBON batch max-value entropy search over a shared pool (adkf_gibbon_pool / gp_ops.gibbon_pool) - the new epilogue alone
against the mpmath reference at the call's own mean and variance, every step's scores and pick against the float64 reference
conditioned on the device's own earlier picks (gibbon_ref.py, assertions 1-4) on every task kind and on an ARD batch, the bitwise
properties of the call (deterministic, independent of the batch, step 0 is a q = 1 call, scores only fall), more tasks than
workgroups, guard bands, exclusions, small pools, a NaN sample, and the batched BO loop with batch="gibbon"."""
import ctypes as C

import numpy as np
import pytest
import torch

import believer_ref as B
import gibbon_ref as R
import test_gpu_believer_pool as BV
import test_gpu_believer_pool_ard as BVA
import test_gpu_log_ei as L
import test_gpu_predict_marginal as M
import test_gpu_predict_pool as P
from test_believer_pool_ard_cpu import ard_posterior
from test_gibbon_pool_cpu import _gb_twin, gb_call

pytestmark = pytest.mark.gpu

MAXIMIZE = 2
EPS32 = R.EPS32
RANGES = (("gamma > -1", -1.0, np.inf), ("-12 < gamma <= -1", -12.0, -1.0), ("gamma <= -12", -np.inf, -12.0))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, c):
    """bit-equal float tensors (NaN payloads included)"""
    return torch.equal(_bits(a), _bits(c))


NAMES = ("sel_idx", "sel_val", "sel_mean", "sel_var", "trace")


def _same_out(a, c, t=None, u=None, names=NAMES):
    for name in names:
        x, y = (a[name], c[name]) if t is None else (a[name][t], c[name][u])
        assert torch.equal(x, y) if name == "sel_idx" else _same(x, y), (name, t)


@pytest.mark.parametrize("kernel,ns,d", L.SHAPES)
def test_the_epilogue_alone(dev, kernel, ns, d):
    """pm_gibbon_term and the sum over the samples (step 0 of a q = 1 call) against mpmath at the call's OWN float32 mean and latent
    variance (predict_pool on the same batch: the same tile arithmetic), sigma, rho2 and gamma formed in float64 from them with the
    kernel's clamp, which leaves the GP's float32 error out:
        |got - ref| <= EVAL_C eps32 mean_s (1 + gamma_s^2),
    EVAL_C = 4 x the largest ratio this test has measured, rounded up to a power of two (gibbon_ref.py).  The pool holds task 0's
    support rows: small variances, large |gamma|.  Both samples of a call lie in one band, so that most rows fall into one range of
    the evaluation; every range must be reached."""
    from adkf_ift_amd import gp_ops
    from oracle import gp_oracle as O

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    T, ROWS = L.T, L.ROWS
    pp = gp_ops.predict_pool(b, phi, Xc, latent=True)
    gp_ops.check_info(pp["info"])
    mean, var = pp["mean"].cpu().numpy(), pp["var"].cpu().numpy()
    noise = [float(np.float32(float(O.transform_phi(phi[t].double().cpu())[0]))) for t in range(T)]
    worst = {name: 0.0 for name, _, _ in RANGES}
    count = {name: 0 for name, _, _ in RANGES}
    compared = 0
    for maximize, shift in ((False, -0.5), (True, 1.5), (False, 30.0)):   # gamma around 0 and above; moderately negative; far left
        base = np.median(mean, axis=1)
        ystar = np.stack([base + shift, base + shift + 0.25], 1).astype(np.float32)   # minimisation: gamma = (m - ystar) / sigma
        if maximize:
            ystar = np.stack([base - shift, base - shift - 0.25], 1).astype(np.float32)
        out = gp_ops.gibbon_pool(b, phi, Xc, ystar=torch.from_numpy(ystar).to(dev), q=1, maximize=maximize, want_trace=True)
        gp_ops.check_info(out["info"])
        got = out["trace"][:, 0].cpu().numpy()
        assert got.shape == (T, ROWS) and np.isfinite(got).all() and (got >= 0).all()
        for t in range(T):
            ref, gamma = R.a_ref(mean[t], var[t], noise[t], ystar[t], maximize, clamp=L.CLAMP32)
            unit = EPS32 * R.gamma_weight(gamma)
            err = np.abs(got[t].astype(np.float64) - ref)
            for name, lo, hi in RANGES:
                sel = ((gamma > lo) & (gamma <= hi)).all(axis=1)
                if sel.any():
                    worst[name] = max(worst[name], float((err[sel] / unit[sel]).max()))
                    count[name] += int(sel.sum())
            print(f"{kernel} maximize {maximize} shift {shift} task {t}: gamma in [{gamma.min():.4g}, {gamma.max():.4g}], "
                  f"min var {var[t].min():.3g}, worst err / unit {float((err / unit).max()):.3f}")
            assert (err <= R.EVAL_C * unit).all(), (shift, t, float((err / unit).max()), gamma[(err / unit).argmax()])
            compared += ref.size
    print(f"{kernel}: worst |got - ref| / (eps32 mean_s (1 + gamma_s^2)) per range {worst}, rows per range {count}")
    assert compared == 3 * T * ROWS                      # no row was left out
    assert all(count[name] > 0 for name in count), count   # and every range of the evaluation was reached


_posts = {}


def _post_of(b, phi, Zs, ys, n_s, X, ard=False):
    """The float64 posterior of every task over the pool, once per problem (the problems are shared and left unchanged)."""
    key = (b.kernel, tuple(n_s), tuple(X.shape), ard, float(X.double().sum()), float(phi.double().sum()), float(ys.double().sum()))
    if key not in _posts:
        Xh, ph = X.cpu().numpy(), phi.cpu().numpy()
        _posts[key] = [(ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], Xh, ph[t], b.kernel) if ard else
                        B.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], Xh, ph[t], b.kernel)) for t in range(len(n_s))]
    return _posts[key]


def _check_device(out, posts, ystar, maximize, tag, lists=None):
    from adkf_ift_amd import gp_ops

    gp_ops.check_info(out["info"])
    si, sv, sm, sr, tr = (out[k].cpu().numpy() for k in NAMES)
    worst_all = 0.0
    for t, post in enumerate(posts):
        worst = R.check_task(post, ystar[t], maximize, si[t], sv[t], sm[t], sr[t], tr[t], excluded=lists[t] if lists else (), tag=(tag, t))
        print(f"{tag} task {t}: picks {si[t].tolist()[:8]}, worst trace error / bound {worst:.3f}")
        worst_all = max(worst_all, worst)
        got = [p for p in si[t].tolist() if p >= 0]
        assert len(set(got)) == len(got)
    assert (tr[:, 1:] <= tr[:, :1]).all(), (tag, "a pick raised a score")   # bit for bit: float comparison of the stored values
    return worst_all


def _check_twin(b, Zs, ys, n_s, X, phi, posts, ystar, maximize, q, tag, ard=False):
    """The twin meets assertions 1-4 on this shape too (so that a miss of the device is the device's)."""
    from oracle import cpu_twin

    fn = _gb_twin()
    T = len(n_s)
    hb = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((T, 4), np.float32), b.kernel, n_s=np.array(n_s, np.int32))
    if ard:
        hb.c.flags = 4
    Xh, ph = np.ascontiguousarray(X.cpu().numpy()), np.ascontiguousarray(phi.cpu().numpy())
    si, sv, sm, sr, tr, _ = gb_call(fn, hb, ph, MAXIMIZE if maximize else 0, Xh, ystar, q)
    for t in range(T):
        R.check_task(posts[t], ystar[t], maximize, si[t], sv[t], sm[t], sr[t], tr[t], tag=(tag, "twin", t))


CASES = [  # (kernel, n_s, d, rows, q, S, twin too): the believer's shapes, S spread over them
    ("matern", [48, 45, 31], 16, 300, 8, 5, False),       # plain, one panel
    ("rbf", [128, 125, 85], 64, 37, 5, 64, False),        # two panels, one partial tile
    ("rbf", [200, 197, 133], 64, 333, 8, 5, True),        # refined, LDS tiles
    ("matern", [1024, 700], 12, 130, 4, 1, False),        # global slots
    ("rbf", [32, 29, 21], 8, 200, 64, 1, False),          # the full pick panel
]


@pytest.mark.parametrize("kernel,n_s,d,rows,q,S,twin", CASES)
def test_against_the_reference(dev, kernel, n_s, d, rows, q, S, twin):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    for maximize in ((False, True) if max(n_s) <= 200 else (False,)):
        ystar = np.stack([R.ystar_above(post, S, maximize) for post in posts])
        if twin and not maximize:
            _check_twin(b, Zs, ys, n_s, X, phi, posts, ystar, maximize, q, (kernel, max(n_s)))
        out = gp_ops.gibbon_pool(b, phi, X, ystar=torch.from_numpy(ystar).to(dev), q=q, maximize=maximize, want_trace=True)
        _check_device(out, posts, ystar, maximize, (kernel, max(n_s), S, maximize))
        assert bool((out["sel_idx"] >= 0).all()) and bool(torch.isfinite(out["sel_val"]).all())
        assert bool((out["trace"][:, 0] >= 0).all())


def test_samples_below_the_means_reach_every_branch(dev):
    """The second set of reference inputs on the plain shape: every gamma <= -1, the far samples <= -12 - with the first set all three
    branches of pm_gibbon_term run on the device and are compared."""
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, q, S, _ = CASES[0]
    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    for maximize in (False, True):
        ystar = np.stack([R.ystar_below(post, S, maximize) for post in posts])
        gamma = np.concatenate([R.gamma_of(p[0], p[1].diagonal(), ystar[t], maximize).ravel() for t, p in enumerate(posts)])
        assert (gamma <= -1).all() and (gamma <= -12).any() and (gamma > -12).any()
        out = gp_ops.gibbon_pool(b, phi, X, ystar=torch.from_numpy(ystar).to(dev), q=q, maximize=maximize, want_trace=True)
        _check_device(out, posts, ystar, maximize, ("below", maximize))
        assert bool((out["sel_idx"] >= 0).all())


def test_ard(dev):
    from adkf_ift_amd import gp_ops

    kernel, n_s, d, rows, q, S = "matern", [48, 45, 31], 12, 300, 8, 5
    b, phi, Zs, ys, n_s, X, _ = BVA._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    posts = _post_of(b, phi, Zs, ys, n_s, X, ard=True)
    for maximize in (False, True):
        ystar = np.stack([R.ystar_above(post, S, maximize) for post in posts])
        if maximize:
            _check_twin(b, Zs, ys, n_s, X, phi, posts, ystar, maximize, q, "ard", ard=True)
        out = gp_ops.gibbon_pool(b, phi, X, ystar=torch.from_numpy(ystar).to(dev), q=q, maximize=maximize, want_trace=True)
        _check_device(out, posts, ystar, maximize, ("ard", maximize))
        assert bool((out["sel_idx"] >= 0).all())


def _ill(dev):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, _ = P._ill_batch(dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.cat([P._pool(300, 2, 3), b.Z_s[1, :5].cpu()]).to(dev)
    return b, phi, Zs, ys, n_s, X


def test_mixed_kinds_in_one_call(dev):
    """test_gpu_predict_pool._ill_batch: task 1 takes the float64 walk (asserted there from the fitted scalars), the others a
    float32 one - both kernels of the walk in one call."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X = _ill(dev)
    Xs = X[-69:].contiguous()   # two tiles of the float32 walks, 18 passes of a float64 workgroup; task 1's support rows included
    for S, maximize, make, pool in ((5, False, R.ystar_above, X), (64, True, R.ystar_above, Xs), (5, True, R.ystar_below, X)):
        posts = _post_of(b, phi, Zs, ys, n_s, pool)
        ystar = np.stack([make(post, S, maximize) for post in posts])
        out = gp_ops.gibbon_pool(b, phi, pool, ystar=torch.from_numpy(ystar).to(dev), q=6, maximize=maximize, want_trace=True)
        _check_device(out, posts, ystar, maximize, ("mixed", S, maximize, make.__name__))
    b.flags = 0


def test_bitwise_properties(dev):
    """Deterministic; trace == NULL changes nothing; a task alone is the task in a batch; step 0 of a q = 8 call is a q = 1 call;
    trace[j] <= trace[0] (the float32 downdate only subtracts squares, the logarithm of a ratio at most 1 is at most 0) - on the
    plain and refined float32 walks and on the float64 walk."""
    from adkf_ift_amd import gp_ops

    for case in (CASES[0], CASES[2]):
        kernel, n_s, d, rows, q, S, _ = case
        b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
        posts = _post_of(b, phi, Zs, ys, n_s, X)
        ystar = torch.from_numpy(np.stack([R.ystar_above(post, S, True) for post in posts])).to(dev)
        lists = [[0, 7], [], [3]]
        kw = dict(q=q, maximize=True, exclude=lists)
        first = gp_ops.gibbon_pool(b, phi, X, ystar=ystar, want_trace=True, **kw)
        _same_out(first, gp_ops.gibbon_pool(b, phi, X, ystar=ystar, want_trace=True, **kw))
        none = gp_ops.gibbon_pool(b, phi, X, ystar=ystar, **kw)
        assert none["trace"] is None
        _same_out(first, none, names=NAMES[:4])
        one = gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=1, maximize=True, exclude=lists, want_trace=True)
        for name in NAMES[:4]:
            assert _same(one[name][:, 0].float(), first[name][:, 0].float()), name
        assert _same(one["trace"][:, 0], first["trace"][:, 0])
        assert bool((first["trace"][:, 1:] <= first["trace"][:, :1]).all())
        assert bool((first["trace"][:, 1:] < first["trace"][:, :1]).any())
        for t in range(b.T):   # each task alone in a T = 1 batch
            b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), kernel,
                                n_s=torch.tensor([n_s[t]], dtype=torch.int32))
            o1 = gp_ops.gibbon_pool(b1, phi[t:t + 1].contiguous(), X, ystar=ystar[t:t + 1].contiguous(), q=q, maximize=True, exclude=[lists[t]],
                                    want_trace=True)
            _same_out(o1, first, 0, t)
    b, phi, Zs, ys, n_s, X = _ill(dev)                       # the float64 walk (task 1) beside float32 ones
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    ystar = torch.from_numpy(np.stack([R.ystar_above(post, 5, False) for post in posts])).to(dev)
    first = gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=8, want_trace=True)
    _same_out(first, gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=8, want_trace=True))
    one = gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=1, want_trace=True)
    assert torch.equal(one["sel_idx"][:, 0], first["sel_idx"][:, 0]) and _same(one["trace"][:, 0], first["trace"][:, 0])
    assert bool((first["trace"][:, 1:] <= first["trace"][:, :1]).all())
    b1 = gp_ops.GPBatch(b.Z_s[1:2].contiguous(), b.y_s[1:2].contiguous(), b.priors[1:2].contiguous(), b.kernel,
                        n_s=torch.tensor([n_s[1]], dtype=torch.int32))
    o1 = gp_ops.gibbon_pool(b1, phi[1:2].contiguous(), X, ystar=ystar[1:2].contiguous(), q=8, want_trace=True)
    b.flags = 0
    full = gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=8, want_trace=True)   # (both evaluate at phi: no state of a fit is reused)
    _same_out(o1, full, 0, 1)


def test_more_tasks_than_workgroups(dev):
    """T = 300 tiny tasks over two tiles, one partial: assertions 2-4 on every task, and three tasks alone are the tasks in the batch."""
    from adkf_ift_amd import gp_ops

    T, ns, d, rows, q, S = 300, 8, 4, 70, 3, 1
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
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    ystar = np.stack([R.ystar_above(post, S, False) for post in posts])
    yd = torch.from_numpy(ystar).to(dev)
    out = gp_ops.gibbon_pool(b, phi, X, ystar=yd, q=q)
    gp_ops.check_info(out["info"])
    si, sv, sm, sr = (out[k].cpu().numpy() for k in NAMES[:4])
    for t in range(T):
        R.check_task(posts[t], ystar[t], False, si[t], sv[t], sm[t], sr[t], None, tag=("T300", t))
        assert (si[t] >= 0).all() and len(set(si[t].tolist())) == q
    for t in (0, 151, 299):
        b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), "matern",
                            n_s=torch.tensor([n_s[t]], dtype=torch.int32))
        o1 = gp_ops.gibbon_pool(b1, phi[t:t + 1].contiguous(), X, ystar=yd[t:t + 1].contiguous(), q=q)
        _same_out(o1, out, 0, t, names=NAMES[:4])


def test_guard_bands(dev):
    from adkf_ift_amd import _lib, gp_ops

    kernel, n_s, d, rows, q, S, _ = CASES[0]
    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
    posts = _post_of(b, phi, Zs, ys, n_s, X)
    T, ns = b.T, b.ns
    lib = _lib.load()
    need = lib.adkf_workspace_bytes(T, ns, 0, d)
    sb = lib.adkf_believer_pool_scratch_bytes(T, ns, d, q)
    guard = 4096
    ws_g = torch.full((need + guard,), 0x5a, dtype=torch.uint8, device=dev)
    scratch = torch.full((sb + guard,), 0x5a, dtype=torch.uint8, device=dev)
    trace = torch.full((T * q * rows + guard,), 12345.0, device=dev)
    sel_idx = torch.full((T * q + guard,), 12345, dtype=torch.int64, device=dev)
    sel = [torch.full((T * q + guard,), 12345.0, device=dev) for _ in range(3)]
    info = torch.empty(T, dtype=torch.int32, device=dev)
    ystar = torch.from_numpy(np.stack([R.ystar_above(post, S, False) for post in posts])).to(dev)   # exactly [T, S]: nothing behind it
    p = lambda t: C.c_void_p(t.data_ptr())
    cb = b.c_struct()
    skipped = torch.tensor([n_s[0], 0, n_s[2]], dtype=torch.int32, device=dev)   # task 1: skipped
    cb.n_s = skipped.data_ptr()
    cb.flags = 0
    rc = lib.adkf_gibbon_pool(C.byref(cb), p(phi), 0, p(X), rows, p(ystar), S, None, None, q, p(trace), p(sel_idx), p(sel[0]), p(sel[1]), p(sel[2]),
                              p(info), p(ws_g), need, p(scratch), sb, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
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
    full = gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=q, want_trace=True)
    for t in (0, 2):
        assert torch.equal(si[t], full["sel_idx"][t]) and _same(tr[t], full["trace"][t])


def test_exclusions_small_pools_and_a_nan_sample(dev):
    from adkf_ift_amd import gp_ops

    T, d, rows = 3, 16, 6000
    b, phi, Zs, ys, n_s, X300, _ = BV._explicit(dev, "matern", [48, 45, 31], d, 300, 548)
    X = P._pool(rows, d, 5).to(dev)
    ystar = torch.from_numpy(np.stack([R.ystar_above(post, 5, False) for post in _post_of(b, phi, Zs, ys, n_s, X300)])).to(dev)
    free = gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=4)
    keep = sorted(set(range(0, rows, 7)) | set(free["sel_idx"][0].tolist()))
    lists = [[i for i in range(rows) if i not in keep][:5000] + free["sel_idx"][0].tolist(), [], free["sel_idx"][2, :1].tolist()]
    assert len(lists[0]) > 5000
    out = gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=4, exclude=lists)
    for t in range(T):
        got = out["sel_idx"][t].tolist()
        assert len(set(got)) == 4 and min(got) >= 0 and not set(got) & set(lists[t]), t
    assert torch.equal(out["sel_idx"][1], free["sel_idx"][1]) and out["sel_idx"][2, 0] != free["sel_idx"][2, 0]
    # a pool of 9 rows with q = 16: nine picks, then the -1 / -inf / 0 / 0 tail; an empty pool: the tail only
    out = gp_ops.gibbon_pool(b, phi, X[:9], ystar=ystar, q=16, want_trace=True)
    si = out["sel_idx"].cpu()
    for t in range(T):
        assert sorted(si[t, :9].tolist()) == list(range(9)) and bool((si[t, 9:] == -1).all())
    assert bool(torch.isfinite(out["sel_val"][:, :9]).all()) and bool(torch.isneginf(out["sel_val"][:, 9:]).all())
    assert bool((out["sel_mean"][:, 9:] == 0).all()) and bool((out["sel_var"][:, 9:] == 0).all())
    out = gp_ops.gibbon_pool(b, phi, X[:0], ystar=ystar, q=3, want_trace=True)
    assert bool((out["sel_idx"] == -1).all()) and bool(torch.isneginf(out["sel_val"]).all()) and out["trace"].shape == (T, 3, 0)
    # a NaN or infinite sample: that task has no pick and NaN scores, the others are unchanged
    full = gp_ops.gibbon_pool(b, phi, X300, ystar=ystar, q=4, want_trace=True)
    for bad in (float("nan"), float("inf"), float("-inf")):
        ys2 = ystar.clone()
        ys2[1, 2] = bad
        out = gp_ops.gibbon_pool(b, phi, X300, ystar=ys2, q=4, want_trace=True)
        assert bool((out["sel_idx"][1] == -1).all()) and bool(torch.isneginf(out["sel_val"][1]).all()) and bool(torch.isnan(out["trace"][1]).all())
        assert bool((out["sel_mean"][1] == 0).all()) and bool((out["sel_var"][1] == 0).all())
        for t in (0, 2):
            _same_out(out, full, t, t)
    with pytest.raises(ValueError):
        gp_ops.gibbon_pool(b, phi, X[:, :4].contiguous(), ystar=ystar, q=3)
    with pytest.raises(ValueError):
        gp_ops.gibbon_pool(b, phi, X, ystar=ystar[:2], q=3)
    with pytest.raises(RuntimeError):
        gp_ops.gibbon_pool(b, phi, X, ystar=ystar.cpu(), q=3)


def test_bo_loop(dev, monkeypatch):
    """The toy pool of test_gpu_mes_pool.test_bo_loop.  batch="gibbon": records of the right length with distinct picks, two runs are
    equal, a replicate alone is the replicate in a batch of four, and the loop calls gibbon_pool instead of mes_pool.  batch="topk"
    is the loop as it was: the default's records, from mes_pool calls only."""
    from adkf_ift_amd import bayes_opt as BO
    from adkf_ift_amd import gp_ops

    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=3, num_bo_iters=3, kernel_type="matern", device=dev, init_from=5000, noise_init=0.01,
              noise_prior=True, n_features=256)
    calls = {"mes": 0, "gibbon": 0}
    mes_pool, gibbon_pool = gp_ops.mes_pool, gp_ops.gibbon_pool

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(gp_ops, "mes_pool", counted("mes", mes_pool))
    monkeypatch.setattr(gp_ops, "gibbon_pool", counted("gibbon", gibbon_pool))
    Rn = 4
    rngs = lambda n=Rn: [np.random.default_rng(s) for s in range(n)]
    recs = BO.run_gp_mes_bo_batched(X, y, rngs=rngs(), batch="gibbon", **kw)
    assert calls == {"mes": 0, "gibbon": 3}
    assert len(recs) == Rn
    for r in range(Rn):
        assert len(recs[r]) == 1 + 3 * 3 and len(set(recs[r][1:])) == 9 and all(0 <= i < 10000 for i in recs[r]), recs[r]
    assert recs == BO.run_gp_mes_bo_batched(X, y, rngs=rngs(), batch="gibbon", **kw)
    for r in (0, 3):
        alone = BO.run_gp_mes_bo_batched(X, y, rngs=[np.random.default_rng(r)], batch="gibbon", **kw)
        assert alone[0] == recs[r], (r, "the batch couples replicates")
    calls.update(mes=0, gibbon=0)
    topk = BO.run_gp_mes_bo_batched(X, y, rngs=rngs(2), batch="topk", **kw)
    assert topk == BO.run_gp_mes_bo_batched(X, y, rngs=rngs(2), **kw)
    assert calls == {"mes": 6, "gibbon": 0}
    gum = BO.run_gp_mes_bo_batched(X, y, rngs=rngs(2), batch="gibbon", max_value="gumbel", ard=True, **kw)
    for rec in gum:
        assert len(rec) == 1 + 3 * 3 and len(set(rec[1:])) == 9, rec
    with pytest.raises(ValueError):
        BO.run_gp_mes_bo_batched(X, y, rngs=rngs(1), batch="believer", **kw)
