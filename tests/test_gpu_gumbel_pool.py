"""GPU: Gumbel max-value sampling over a shared pool (adkf_gumbel_pool / gp_ops.gumbel_pool) - the reduction alone against the exact
quartiles of gumbel_ref.py at the call's own mean and variance, end to end against the float64 oracle, every path (float64 walk,
refined walk, ARD, global row-tile slots, more tasks than workgroups), bit-for-bit independence of the batch, the grid and the order
of the pool's rows, graph capture, guard bands, known answers, the draws against the call's own fit, and the batched BO loop."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.special import ndtri

import gumbel_ref as G
import test_gpu_log_ei as L
import test_gpu_predict_marginal as M
import test_gpu_predict_marginal_ard as MA
import test_gpu_predict_pool as P

pytestmark = pytest.mark.gpu

SHAPES = L.SHAPES          # ("rbf", 32, 16): the plain walk; ("matern", 200, 64): the refined one
T = L.T
EPS32 = 2.0 ** -24
# The quartile error of the reduction alone, in units of the reference b: the largest value seen on the MI355X over the cases of
# test_the_reduction_alone is 1.80e-4 (rbf, 65 rows of which 32 are task 0's support rows; elsewhere about 1e-4: the interpolation
# error of the second pass; the float32 terms add about 1e-6).  Four times that, for other shapes and devices; it may never exceed
# 1e-2 (with S <= 64 samples the sampling noise of any statistic of ystar is at least b / 8).
QUANT_BOUND = 4 * 1.80e-4
assert QUANT_BOUND <= 1e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, c):
    return torch.equal(_bits(a), _bits(c))


def _same_out(x, y, t=None, s=None):
    """quant, gumbel and ystar of two calls (of task s of x and task t of y), bit for bit"""
    pick = (lambda o, i: o if i is None else o[i])
    return all(_same(pick(x[n], s), pick(y[n], t)) for n in ("quant", "gumbel", "ystar"))


def _u(Tn, S, seed, dev):
    return torch.rand(Tn, S, generator=torch.Generator().manual_seed(seed)).to(dev)


def _own(b, phi, X, maximize):
    """mu (the score's sense) and sigma from the call's own float32 latent mean and variance: the same tile arithmetic"""
    from adkf_ift_amd import gp_ops

    pp = gp_ops.predict_pool(b, phi, X, latent=True)
    gp_ops.check_info(pp["info"])
    mean, var = pp["mean"].cpu().numpy().astype(np.float64), pp["var"].cpu().numpy()
    return (mean if maximize else -mean), np.sqrt(np.maximum(var, np.float32(1e-12))).astype(np.float64)


def _quant_err(out, t, mu, sigma, tag, extra=0.0):
    """the quartile error of task t in units of the reference b, asserted against QUANT_BOUND b (+ 4 eps32 max|q|: the float32 probes
    and outputs) + extra; gumbel against the fit of the reference"""
    q_ref = G.quartiles_exact(mu, sigma)
    a_ref, b_ref = G.gumbel_fit(q_ref)
    quant, gumbel = out["quant"][t].cpu().numpy().astype(np.float64), out["gumbel"][t].cpu().numpy().astype(np.float64)
    tol = QUANT_BOUND * b_ref + 4 * EPS32 * np.abs(q_ref).max() + extra
    err = np.abs(quant - q_ref).max()
    print(f"{tag}: rows {mu.size}, b {b_ref:.4g}, quartile error {err / b_ref:.3e} b, bound {tol / b_ref:.3e} b")
    assert err <= tol, (tag, err / b_ref, tol / b_ref)
    assert quant[0] <= quant[1] <= quant[2] and gumbel[1] >= 0
    assert abs(gumbel[1] - b_ref) <= 2 * tol / G.DENOM + 2 * EPS32 * b_ref and abs(gumbel[0] - a_ref) <= 2 * tol
    return err / b_ref


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_the_reduction_alone(dev, kernel, ns, d):
    """quant against the exact quartiles at the call's OWN mean and variance (predict_pool on the same batch: the posterior
    cancels), rows on both sides of the tile size, both senses."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    worst = 0.0
    for rows in (1, 63, 64, 65, 130, 1000):
        Xr = torch.cat([Xc, X])[:rows].contiguous()      # (the first rows: task 0's support rows, small variances)
        for maximize in (False, True):
            mu, sigma = _own(b, phi, Xr, maximize)
            out = gp_ops.gumbel_pool(b, phi, Xr, u=_u(T, 4, rows, dev), maximize=maximize)
            gp_ops.check_info(out["info"])
            for t in range(T):
                worst = max(worst, _quant_err(out, t, mu[t], sigma[t], f"{kernel} rows {rows} maximize {maximize} task {t}"))
    print(f"{kernel}: worst quartile error of the reduction alone {worst:.3e} b")


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_against_the_oracle(dev, kernel, ns, d):
    """End to end against oracle.gp_oracle.predict: the bound of the reduction alone plus max_i (|m_i - m_i^o| + 8 |sigma_i - sigma_i^o|),
    evaluated here.  A common shift of the means shifts every quantile by as much; at any z >= lo every gamma_i >= -1, and rows with
    gamma_i > 8 contribute under 1e-15 each, so a change of sigma_i acts as a change of mu_i by at most 8 |delta sigma_i|."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    for maximize in (False, True):
        mu, sigma = _own(b, phi, X, maximize)
        out = gp_ops.gumbel_pool(b, phi, X, u=_u(T, 8, 3, dev), maximize=maximize)
        gp_ops.check_info(out["info"])
        for t, (m, v) in enumerate(post):
            mu_o, sg_o = (m if maximize else -m), np.sqrt(np.maximum(v, 1e-12))
            extra = float((np.abs(mu[t] - mu_o) + 8 * np.abs(sigma[t] - sg_o)).max())
            _quant_err(out, t, mu_o, sg_o, f"oracle {kernel} maximize {maximize} task {t} (posterior term {extra:.2e})", extra)


def _alone(b, phi, t, n_s_t, ard=False):
    from adkf_ift_amd import gp_ops

    b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), b.kernel,
                        n_s=torch.tensor([n_s_t], dtype=torch.int32), ard=ard)
    return b1, phi[t:t + 1].contiguous()


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_bit_for_bit(dev, kernel, ns, d):
    """The same call twice; a task alone and inside a batch with a skipped task; a permutation of the pool's rows; the pool split as
    [A; B] and [B; A]; rows that end inside a tile."""
    from adkf_ift_amd import gp_ops

    b0, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    n_s2 = list(n_s)
    n_s2[2] = 0                                                                                          # task 2: skipped
    b = gp_ops.GPBatch(b0.Z_s, b0.y_s, b0.priors, b0.kernel, n_s=torch.tensor(n_s, dtype=torch.int32))
    gp_ops.check_info(gp_ops.predict_pool(b, phi, Xc[:1].contiguous(), latent=True)["info"])            # the inner quantities at phi, then reused
    b.n_s = torch.tensor(n_s2, dtype=torch.int32, device=dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    u = _u(T, 5, 7, dev)
    for maximize in (False, True):
        out = gp_ops.gumbel_pool(b, phi, Xc, u=u, maximize=maximize)
        assert _same_out(gp_ops.gumbel_pool(b, phi, Xc, u=u, maximize=maximize), out)
        inf = float("-inf") if maximize else float("inf")
        assert bool(torch.isneginf(out["quant"][2]).all()) and bool(torch.isneginf(out["gumbel"][2]).all()) and bool((out["ystar"][2] == inf).all())
        for t in (0, 1, 3):
            assert bool(torch.isfinite(out["ystar"][t]).all())
            b1, phi1 = _alone(b, phi, t, n_s2[t])
            assert _same_out(gp_ops.gumbel_pool(b1, phi1, Xc, u=u[t:t + 1].contiguous(), maximize=maximize), out, t, 0), (maximize, t)
        perm = torch.randperm(Xc.shape[0], generator=torch.Generator().manual_seed(1)).to(dev)
        assert _same_out(gp_ops.gumbel_pool(b, phi, Xc[perm].contiguous(), u=u, maximize=maximize), out), (maximize, "permutation")
        assert _same_out(gp_ops.gumbel_pool(b, phi, torch.cat([Xc[300:], Xc[:300]]).contiguous(), u=u, maximize=maximize), out), (maximize, "[B; A]")
    empty = gp_ops.gumbel_pool(b, phi, Xc[:0], u=u, maximize=True)
    assert bool(torch.isneginf(empty["ystar"]).all()) and bool(torch.isneginf(empty["quant"]).all()) and bool(torch.isneginf(empty["gumbel"]).all())
    assert bool(torch.isposinf(gp_ops.gumbel_pool(b, phi, Xc[:0], u=u)["ystar"]).all())
    # the samples of a skipped task make adkf_mes_pool's scores NaN, which are never selected
    ms = gp_ops.mes_pool(b, phi, Xc, ystar=out["ystar"], maximize=True, topk=3)
    assert bool((ms["top_idx"][2] == -1).all()) and bool((ms["top_idx"][0] >= 0).all())
    with pytest.raises(ValueError):
        gp_ops.gumbel_pool(b, phi, Xc[:, :4].contiguous(), u=u)
    with pytest.raises(RuntimeError):
        gp_ops.gumbel_pool(b, phi, Xc, u=u.cpu())


def test_graph_replay_equals_eager(dev):
    """No host synchronisation between the walks: the call is captured into a graph (every buffer it touches allocated before the
    capture and kept), and each replay gives the eager call's bits."""
    from adkf_ift_amd import _lib, gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, *SHAPES[0])
    S = 6
    u = _u(T, S, 9, dev)
    eager = gp_ops.gumbel_pool(b, phi, X, u=u, maximize=True)
    want = {n: eager[n].cpu() for n in ("ystar", "quant", "gumbel")}
    lib = _lib.load()
    out = {"ystar": torch.zeros(T, S, device=dev), "quant": torch.zeros(T, 3, device=dev), "gumbel": torch.zeros(T, 2, device=dev)}
    info = torch.zeros(T, dtype=torch.int32, device=dev)
    sb = lib.adkf_gumbel_pool_scratch_bytes(T)
    scratch = torch.zeros(sb, dtype=torch.uint8, device=dev)
    ws, nb = b.workspace()
    cb = b.c_struct()
    p = lambda t: C.c_void_p(t.data_ptr())

    def call():
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        return lib.adkf_gumbel_pool(C.byref(cb), p(phi), 2, p(X), X.shape[0], p(u), S, p(out["ystar"]), p(out["quant"]), p(out["gumbel"]),
                                    p(info), p(ws), nb, p(scratch), sb, st)

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call() == 0
    for _ in range(3):
        for n in want:
            out[n].fill_(7.0)
        info.fill_(5)
        graph.replay()
        torch.cuda.synchronize()
        assert bool((info.cpu() == 0).all())
        for n in want:
            assert _same(out[n].cpu(), want[n]), n


def test_the_float64_walk_and_a_mixed_batch(dev):
    """test_gpu_predict_pool._ill_batch: task 1 takes the float64 walk (asserted there), the others a float32 one, and task 3 is made
    a skipped one - k_gumbel_walk64 and the tile walk in one call, and each task alone gives the bits it has in the batch."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, _ = P._ill_batch(dev)
    X = (P._pool(300, 2, 3) * 0.6).to(dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    u = _u(4, 5, 2, dev)
    for maximize in (True, False):
        mu, sigma = _own(b, phi, X, maximize)
        out = gp_ops.gumbel_pool(b, phi, X, u=u, maximize=maximize)
        gp_ops.check_info(out["info"])
        for t in range(4):
            _quant_err(out, t, mu[t], sigma[t], f"float64 batch maximize {maximize} task {t}")
    post = [(m, v - noise) for m, v, noise in (M._oracle_diag(Zs[t, :n_s[t]], ys[t, :n_s[t]], X.cpu(), phi[t], 0) for t in range(4))]
    extra = float((np.abs(mu[1] + post[1][0]) + 8 * np.abs(sigma[1] - np.sqrt(np.maximum(post[1][1], 1e-12)))).max())
    _quant_err(out, 1, -post[1][0], np.sqrt(np.maximum(post[1][1], 1e-12)), f"float64 task against the oracle (posterior term {extra:.2e})", extra)
    n_s2 = [n_s[0], n_s[1], n_s[2], 0]
    bm = b
    bm.n_s = torch.tensor(n_s2, dtype=torch.int32, device=dev)
    mixed = gp_ops.gumbel_pool(bm, phi, X, u=u)
    assert bool(torch.isneginf(mixed["quant"][3]).all()) and bool(torch.isposinf(mixed["ystar"][3]).all())
    for t in range(3):
        b1, phi1 = _alone(bm, phi, t, n_s2[t])
        assert _same_out(gp_ops.gumbel_pool(b1, phi1, X, u=u[t:t + 1].contiguous()), mixed, t, 0), t
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(4)).to(dev)
    assert _same_out(gp_ops.gumbel_pool(bm, phi, X[perm].contiguous(), u=u), mixed)


def test_ard(dev):
    """The ARD batch of test_gpu_predict_pool.test_bit_for_bit_ard through the same entry."""
    from adkf_ift_amd import gp_ops

    ns, d = 64, 12
    n_s = [64, 50, 33, 9]
    Zs, ys, _ = M._features(4, ns, [0] * 4, d, 31, True)
    b, phi = MA._fit_ard(dev, Zs, ys, n_s, "matern", True)
    b.flags = gp_ops.REUSE_INNER
    X = P._pool(523, d, 5).to(dev)
    u = _u(4, 5, 5, dev)
    for maximize in (True, False):
        mu, sigma = _own(b, phi, X, maximize)
        out = gp_ops.gumbel_pool(b, phi, X, u=u, maximize=maximize)
        gp_ops.check_info(out["info"])
        for t in range(4):
            _quant_err(out, t, mu[t], sigma[t], f"ard maximize {maximize} task {t}")
    perm = torch.randperm(523, generator=torch.Generator().manual_seed(6)).to(dev)
    assert _same_out(gp_ops.gumbel_pool(b, phi, X[perm].contiguous(), u=u, maximize=False), out)


def test_global_row_tile_slots(dev):
    """The last of test_gpu_predict_pool.BIT_CASES: 1024 points, the row tiles in the global slots."""
    from adkf_ift_amd import gp_ops

    kernel, ns, d, rows = P.BIT_CASES[-1]
    n_s = [ns, max(2, ns - 3), max(2, (2 * ns) // 3), max(2, ns // 4)]
    Zs, ys, _ = M._features(4, ns, [0] * 4, d, 300 + ns + d, True)
    b, phi = M._fit(dev, Zs, ys, n_s, kernel, True)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = P._pool(rows, d, 17).to(dev)
    u = _u(4, 3, 8, dev)
    mu, sigma = _own(b, phi, X, True)
    out = gp_ops.gumbel_pool(b, phi, X, u=u, maximize=True)
    gp_ops.check_info(out["info"])
    for t in range(4):
        _quant_err(out, t, mu[t], sigma[t], f"global slots task {t}")
    assert _same_out(gp_ops.gumbel_pool(b, phi, X.flip(0).contiguous(), u=u, maximize=True), out)


def test_more_tasks_than_workgroups(dev):
    """test_gpu_predict_pool.test_more_tasks_than_workgroups's batch: 2000 small tasks, beyond the resident grid, so a workgroup serves
    several tasks one after the other; a task's result is what it is alone."""
    from adkf_ift_amd import gp_ops

    Tn, ns, d, rows = 2000, 8, 8, 130
    g = torch.Generator().manual_seed(6)
    n_s = torch.randint(3, ns + 1, (Tn,), generator=g).tolist()
    Zs, ys, _ = M._features(Tn, ns, [0] * Tn, d, 66, True)
    b, phi = M._fit(dev, Zs, ys, n_s, "rbf", True)
    b.flags = 0
    X = P._pool(rows, d, 14).to(dev)
    u = _u(Tn, 3, 10, dev)
    out = gp_ops.gumbel_pool(b, phi, X, u=u)
    gp_ops.check_info(out["info"])
    assert bool(torch.isfinite(out["ystar"]).all()) and bool((out["gumbel"][:, 1] > 0).all())
    mu, sigma = _own(b, phi, X, False)
    for t in (0, 777, 1999):
        _quant_err(out, t, mu[t], sigma[t], f"T2000[{t}]")
        b1, phi1 = _alone(b, phi, t, n_s[t])
        assert _same_out(gp_ops.gumbel_pool(b1, phi1, X, u=u[t:t + 1].contiguous()), out, t, 0), t


def test_guard_bands_and_exact_sizes(dev):
    from adkf_ift_amd import _lib, gp_ops

    Tn, ns, d, rows, S = 3, 128, 256, 7001, 7
    Zs, ys, _ = M._features(Tn, ns, [0] * Tn, d, 7, True)
    b, phi = M._fit(dev, Zs, ys, [128, 100, 77], "rbf", True)
    lib = _lib.load()
    need = lib.adkf_workspace_bytes(Tn, ns, 0, d)
    ws, nb = b.workspace()
    assert nb == need
    b.n_s = torch.tensor([128, 0, 77], dtype=torch.int32, device=dev)   # task 1: skipped
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = P._pool(rows, d, 3).to(dev)
    guard = 4096
    ystar = torch.full((Tn * S + guard,), 12345.0, device=dev)
    quant = torch.full((Tn * 3 + guard,), 12345.0, device=dev)
    gumbel = torch.full((Tn * 2 + guard,), 12345.0, device=dev)
    sb = lib.adkf_gumbel_pool_scratch_bytes(Tn)
    scratch = torch.full((sb + guard,), 0x5a, dtype=torch.uint8, device=dev)
    info = torch.empty(Tn, dtype=torch.int32, device=dev)
    u = _u(Tn, S, 1, dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    cb = b.c_struct()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.adkf_gumbel_pool(C.byref(cb), p(phi), 0, p(X), rows, p(u), S, p(ystar), p(quant), p(gumbel), p(info), p(ws), need, p(scratch), sb, st)
    assert rc == 0
    gp_ops.check_info(info)
    assert bool((ystar[Tn * S:] == 12345.0).all()) and bool((quant[Tn * 3:] == 12345.0).all()) and bool((gumbel[Tn * 2:] == 12345.0).all())
    assert bool((scratch[sb:] == 0x5a).all())
    ys_, q_ = ystar[:Tn * S].view(Tn, S), quant[:Tn * 3].view(Tn, 3)
    assert bool(torch.isposinf(ys_[1]).all()) and bool(torch.isneginf(q_[1]).all()) and bool(torch.isneginf(gumbel[2:4]).all())
    assert bool(torch.isfinite(ys_[0]).all()) and bool(torch.isfinite(ys_[2]).all())
    # quant == NULL and gumbel == NULL: the same samples, and nothing else is written
    ystar2 = torch.full((Tn * S + guard,), 12345.0, device=dev)
    rc = lib.adkf_gumbel_pool(C.byref(cb), p(phi), 0, p(X), rows, p(u), S, p(ystar2), None, None, p(info), p(ws), need, p(scratch), sb, st)
    assert rc == 0 and _same(ystar2, ystar) and bool((scratch[sb:] == 0x5a).all())
    wrapper = gp_ops.gumbel_pool(b, phi, X, u=u)
    assert _same(wrapper["ystar"], ys_) and _same(wrapper["quant"], q_)
    assert lib.adkf_gumbel_pool(C.byref(cb), p(phi), 0, p(X), rows, p(u), S, p(ystar2), None, None, p(info), p(ws), need, p(scratch), sb - 1, st) == -3


@pytest.mark.parametrize("rows", [1, 65])
def test_known_answers(dev, rows):
    """rows identical pool rows: Pr = Phi((z - mu) / sigma)^rows, so q = mu + sigma Phi^-1(p^(1 / rows)); rows = 1: mu -+ 0.67449 sigma, mu"""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, *SHAPES[0])
    Xr = X[5:6].repeat(rows, 1).contiguous()
    for maximize in (False, True):
        mu, sigma = _own(b, phi, Xr, maximize)
        out = gp_ops.gumbel_pool(b, phi, Xr, u=torch.full((T, 2), 0.5, device=dev), maximize=maximize)
        quant, gumbel, ystar = (out[n].cpu().numpy().astype(np.float64) for n in ("quant", "gumbel", "ystar"))
        for t in range(T):
            assert (mu[t] == mu[t, 0]).all() and (sigma[t] == sigma[t, 0]).all()
            q_ref = mu[t, 0] + sigma[t, 0] * ndtri(np.array([0.25, 0.5, 0.75]) ** (1.0 / rows))
            b_ref = G.gumbel_fit(q_ref)[1]
            tol = QUANT_BOUND * b_ref + 4 * EPS32 * np.abs(q_ref).max()
            assert np.abs(quant[t] - q_ref).max() <= tol, (rows, maximize, t, np.abs(quant[t] - q_ref).max() / b_ref)
            med = quant[t, 1] if maximize else -quant[t, 1]      # u = 1 / 2 draws the median, in f's sense
            assert np.abs(ystar[t] - med).max() <= 8 * EPS32 * (abs(gumbel[t, 0]) + gumbel[t, 1])


def test_ystar_against_the_calls_own_fit(dev):
    """ystar = a - b log(-log u) in float32 from the call's own (a, b), against float64 on the same float32 a, b and u:
        |got - ref| <= 8 eps32 (|a| + b max(1, |x|)),  x = log(-log u),  eps32 = 2^-24 (half an ulp): 4 ulps.
    The inner logarithm's relative error (1 ulp) is an absolute error of 2 eps32 in x, the outer logarithm adds 2 eps32 |x|, the
    product one rounding of b |x| and the difference one of |a| + b |x|: 6 eps32 in all, and room for one more ulp of either logarithm.
    u at 0 and 1 and beyond is clamped to [2^-24, 1 - 2^-24]: finite."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, *SHAPES[1])
    u = _u(T, 64, 12, dev)
    u[0, 0], u[0, 1], u[1, 0], u[1, 1], u[2, 0], u[2, 1] = 0.0, 1.0, -2.0, 3.0, 2.0 ** -24, 1.0 - 2.0 ** -24
    for maximize in (False, True):
        out = gp_ops.gumbel_pool(b, phi, X, u=u, maximize=maximize)
        assert out["u"] is u or _same(out["u"], u)
        ystar, gumbel, un = out["ystar"].cpu().numpy().astype(np.float64), out["gumbel"].cpu().numpy().astype(np.float64), u.cpu().numpy()
        assert np.isfinite(ystar).all()
        for t in range(T):
            a_, b_ = gumbel[t]
            ref = G.samples(a_, b_, un[t])
            x = np.log(-np.log(np.clip(un[t].astype(np.float64), G.U_MIN, 1 - G.U_MIN)))
            err = np.abs((ystar[t] if maximize else -ystar[t]) - ref)
            bound = 8 * EPS32 * (abs(a_) + b_ * np.maximum(1.0, np.abs(x)))
            print(f"maximize {maximize} task {t}: worst err / bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (maximize, t, float((err / bound).max()))
    # drawn here from a generator: reproducible, and returned
    o1 = gp_ops.gumbel_pool(b, phi, X, n_samples=9, generator=torch.Generator().manual_seed(5))
    o2 = gp_ops.gumbel_pool(b, phi, X, n_samples=9, generator=torch.Generator().manual_seed(5))
    assert o1["u"].shape == (T, 9) and _same(o1["u"], o2["u"]) and _same(o1["ystar"], o2["ystar"])
    assert _same(gp_ops.gumbel_pool(b, phi, X, u=o1["u"])["ystar"], o1["ystar"])


def test_bo_loop(dev, monkeypatch):
    """run_gp_mes_bo_batched(max_value="gumbel") on the problem of test_gpu_mes_pool.test_bo_loop: reproducible records, a replicate
    alone is the replicate in a batch of four, no basis is drawn and no Thompson call is made, the picks go through mes_pool; the
    default is "thompson", unchanged; on the toy pool of test_gpu_surface the loop finds one of the best three points."""
    from adkf_ift_amd import bayes_opt as BO
    from adkf_ift_amd import gp_ops

    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=2, num_bo_iters=3, kernel_type="matern", device=dev, init_from=5000, noise_init=0.01,
              noise_prior=True, n_features=256)
    rngs = lambda n: [np.random.default_rng(s) for s in range(n)]
    default = BO.run_gp_mes_bo_batched(X, y, rngs=rngs(2), **kw)
    assert default == BO.run_gp_mes_bo_batched(X, y, rngs=rngs(2), max_value="thompson", **kw)
    calls = {"mes": 0, "gumbel": 0}
    mes_pool, gumbel_pool = gp_ops.mes_pool, gp_ops.gumbel_pool

    def counted(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    def forbidden(*a, **k):
        raise AssertionError("max_value='gumbel' draws no basis and makes no Thompson call")

    monkeypatch.setattr(gp_ops, "mes_pool", counted("mes", mes_pool))
    monkeypatch.setattr(gp_ops, "gumbel_pool", counted("gumbel", gumbel_pool))
    monkeypatch.setattr(gp_ops, "rff_basis", forbidden)
    monkeypatch.setattr(gp_ops, "max_value_samples", forbidden)
    Rn = 4
    recs = BO.run_gp_mes_bo_batched(X, y, rngs=rngs(Rn), max_value="gumbel", **kw)
    assert calls == {"mes": 3, "gumbel": 3}
    assert len(recs) == Rn
    for r in range(Rn):
        assert len(recs[r]) == 1 + 3 * 2 and len(set(recs[r][1:])) == 6, recs[r]
    assert recs == BO.run_gp_mes_bo_batched(X, y, rngs=rngs(Rn), max_value="gumbel", **kw)
    alone = BO.run_gp_mes_bo_batched(X, y, rngs=[np.random.default_rng(3)], max_value="gumbel", **kw)
    assert alone[0] == recs[3], "the batch couples replicates"
    with pytest.raises(ValueError, match="max_value"):
        BO.run_gp_mes_bo_batched(X, y, rngs=rngs(1), max_value="nope", **kw)
    # the toy objective of test_gpu_surface.test_bayes_opt_gp_ei_loop: ascending y, index 0 is the optimum
    g = torch.Generator().manual_seed(0)
    Xt = torch.randn(60, 5, generator=g)
    yt = ((Xt - 0.3) ** 2).sum(1)
    order = torch.argsort(yt)
    Xt, yt = Xt[order].to(dev), yt[order].to(dev)
    rec = BO.run_gp_mes_bo_batched(Xt, yt, num_init_points=6, query_batch_size=2, num_bo_iters=8, kernel_type="matern", device=dev, init_from=20,
                                   noise_init=0.01, noise_prior=True, rngs=[np.random.default_rng(0)], max_value="gumbel")[0]
    assert len(rec) == 1 + 8 * 2 and len(set(rec[1:])) == 16
    assert min(rec) <= 2          # reaches (one of) the best three points out of 60 within 16 queries
