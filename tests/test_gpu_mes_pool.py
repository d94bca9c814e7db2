"""GPU: max-value entropy search over a shared pool (adkf_mes_pool / gp_ops.mes_pool) - the new epilogue alone against the mpmath
reference of mes_ref.py at the call's own mean and variance, end to end against the float64 oracle, the structure of the call
(selection, determinism, independence of the batch and of the grid, small pools, non-finite samples), every path (float64 walk,
ARD, global row-tile slots), guard bands, and the batched BO loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import mes_ref as R
import test_gpu_log_ei as L
import test_gpu_predict_marginal as M
import test_gpu_predict_marginal_ard as MA
import test_gpu_predict_pool as P
from test_predict_pool_cpu import select_ref

pytestmark = pytest.mark.gpu

SHAPES = L.SHAPES          # ("rbf", 32, 16): the plain walk; ("matern", 200, 64): the refined one
T, ROWS = L.T, L.ROWS
EPS32 = R.EPS32
CLAMP32 = L.CLAMP32
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


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_the_epilogue_alone(dev, kernel, ns, d):
    """pm_mes_term and the sum over the samples against mpmath at the call's OWN float32 mean and latent variance (predict_pool on
    the same batch: the same tile arithmetic), sigma and gamma formed in float64 from them with the kernel's clamp, which leaves the
    GP's float32 error out:
        |got - ref| <= 32 eps32 mean_s (1 + gamma_s^2).
    gamma carries three float32 roundings, which |gamma g'| < 1 turns into about 3 eps32; a float32 evaluation with an exact erfcx
    stays within 1.5 eps32 (1 + gamma^2); the rest is room for the device's erfcxf, logf and expf in the cancelling bracket - the
    room test_gpu_log_ei.test_the_epilogue_alone gives the same bracket.  The pool holds task 0's support rows: small variances,
    large |gamma|.  Both samples of a call lie in one band, so that most rows fall into one range of the evaluation."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    pp = gp_ops.predict_pool(b, phi, Xc, latent=True)
    gp_ops.check_info(pp["info"])
    mean, var = pp["mean"].cpu().numpy(), pp["var"].cpu().numpy()
    worst = {name: 0.0 for name, _, _ in RANGES}
    count = {name: 0 for name, _, _ in RANGES}
    compared = 0
    for maximize, shift in ((False, -0.5), (True, 1.5), (False, 30.0)):   # gamma around 0 and above; moderately negative; far left
        base = np.median(mean, axis=1)
        ystar = np.stack([base + shift, base + shift + 0.25], 1).astype(np.float32)   # minimisation: gamma = (m - ystar) / sigma
        if maximize:
            ystar = np.stack([base - shift, base - shift - 0.25], 1).astype(np.float32)
        out = gp_ops.mes_pool(b, phi, Xc, ystar=torch.from_numpy(ystar).to(dev), maximize=maximize)
        gp_ops.check_info(out["info"])
        got = out["score"].cpu().numpy()
        assert got.shape == (T, ROWS) and np.isfinite(got).all() and (got >= 0).all()   # (g underflows to 0 from gamma ~ 13)
        for t in range(T):
            ref, gamma = R.mes_ref(mean[t], var[t], ystar[t], maximize, clamp=CLAMP32)
            unit = EPS32 * R.gamma_weight(gamma)
            err = np.abs(got[t].astype(np.float64) - ref)
            for name, lo, hi in RANGES:
                sel = ((gamma > lo) & (gamma <= hi)).all(axis=1)
                if sel.any():
                    worst[name] = max(worst[name], float((err[sel] / unit[sel]).max()))
                    count[name] += int(sel.sum())
            print(f"{kernel} maximize {maximize} shift {shift} task {t}: gamma in [{gamma.min():.4g}, {gamma.max():.4g}], "
                  f"min var {var[t].min():.3g}, worst err / bound {float((err / (32 * unit)).max()):.3f}")
            assert (err <= 32 * unit).all(), (shift, t, float((err / (32 * unit)).max()), gamma[(err / unit).argmax()])
            compared += ref.size
    print(f"{kernel}: worst |got - ref| / (eps32 mean_s (1 + gamma_s^2)) per range {worst}, rows per range {count}")
    assert compared == 3 * T * ROWS                      # no row was left out
    assert all(count[name] > 0 for name in count), count   # and every range of the evaluation was reached


def _draw_ystar(post, S, seed):
    """ystar[t, s] = max_x (m + sigma z_s), z_s standard normal per row: samples of max f under independent marginals"""
    g = np.random.default_rng(seed)
    return np.stack([(m[None, :] + np.sqrt(np.maximum(v, 1e-12))[None, :] * g.standard_normal((S, m.size))).max(1) for m, v in post]).astype(np.float32)


def _oracle_post(Zs, ys, n_s, X, phi, kind):
    post = []
    for t in range(len(n_s)):
        m_ref, v_ref, noise = M._oracle_diag(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], kind)
        post.append((m_ref, v_ref - noise))
    return post


def _check_against_the_oracle(score, post, ystar, maximize, tag, spread=False):
    """Per row: |got - ref| <= 0.4 dm / sigma + dv / (2 v) + 32 eps32 mean_s (1 + gamma_s^2), dm = TOL max|m_ref|, dv = TOL max|v_ref|:
    the error test_gpu_predict_pool allows the mean and the latent variance, pushed through |g'| <= 0.4 and |gamma g'| < 1 (a
    relative error dv / v in the variance moves gamma by gamma dv / (2 v)), plus the bound of the epilogue alone."""
    for t, (m, v) in enumerate(post):
        ref, gamma = R.mes_ref(m, v, ystar[t], maximize)
        vc = np.maximum(v, 1e-12)
        dm, dv = P.TOL * np.abs(m).max(), P.TOL * np.abs(v).max()
        bound = 0.4 * dm / np.sqrt(vc) + dv / (2 * vc) + 32 * EPS32 * R.gamma_weight(gamma)
        err = np.abs(score[t].astype(np.float64) - ref)
        print(f"{tag} task {t}: gamma in [{gamma.min():.4g}, {gamma.max():.4g}], latent variance in [{v.min():.3g}, {v.max():.3g}], "
              f"worst err / bound {float((err / bound).max()):.3f}, largest bound {bound.max():.3g}, spread of the scores {ref.max() - ref.min():.3g}")
        if spread:
            assert bound.max() < 0.1 * (ref.max() - ref.min()), (tag, t, "the bound is vacuous for this draw")
        assert (err <= bound).all(), (tag, t, float((err / bound).max()))


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_against_the_oracle(dev, kernel, ns, d):
    """End to end on the pool of test_gpu_predict_pool.test_against_the_oracle, S = 8 samples of max f; the bound stays under a tenth
    of the spread of each task's scores."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    ystar = _draw_ystar(post, 8, 0)
    out = gp_ops.mes_pool(b, phi, X, ystar=torch.from_numpy(ystar).to(dev), maximize=True)
    gp_ops.check_info(out["info"])
    _check_against_the_oracle(out["score"].cpu().numpy(), post, ystar, True, kernel, spread=True)


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_structure(dev, kernel, ns, d):
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    Xd = Xc.clone()
    Xd[10] = Xd[3]; Xd[41] = Xd[3]; Xd[700] = Xd[20]          # planted duplicate rows: bit-equal scores
    g = np.random.default_rng(4)
    ystar = torch.from_numpy((np.array([float(x) for x in best])[:, None] + g.uniform(-2.0, 3.0, (T, 6))).astype(np.float32)).to(dev)
    lists = [[0, 1, 5, 700], [], sorted(set(range(ROWS)) - {3, 10, 41, 50}), [776]]
    for maximize in (False, True):
        full = gp_ops.mes_pool(b, phi, Xd, ystar=ystar, maximize=maximize)
        assert full["top_idx"] is None and full["top_val"] is None
        sc = full["score"].cpu().numpy()
        assert np.isfinite(sc).all() and (sc >= 0).all() and (sc > 0).any()
        assert _same(full["score"][:, 3], full["score"][:, 10]) and _same(full["score"][:, 3], full["score"][:, 41])
        for k in (1, 8, 64):
            out = gp_ops.mes_pool(b, phi, Xd, ystar=ystar, maximize=maximize, topk=k, exclude=lists, want_score=True)
            assert _same(out["score"], full["score"]), (maximize, k, "score with and without topk")
            ti, tv = out["top_idx"].cpu().numpy(), out["top_val"].cpu().numpy()
            for t in range(T):
                idx, val = select_ref(sc[t], k, lists[t])
                assert np.array_equal(ti[t], idx), (maximize, k, t, ti[t], idx)
                assert np.array_equal(tv[t].view(np.int32), val.view(np.int32)), (maximize, k, t)
            only = gp_ops.mes_pool(b, phi, Xd, ystar=ystar, maximize=maximize, topk=k, exclude=lists)     # nothing per row
            assert only["score"] is None and torch.equal(only["top_idx"], out["top_idx"]) and _same(only["top_val"], out["top_val"])
            again = gp_ops.mes_pool(b, phi, Xd, ystar=ystar, maximize=maximize, topk=k, exclude=lists, want_score=True)
            assert _same(again["score"], out["score"]) and torch.equal(again["top_idx"], out["top_idx"])
        # task 2 may take 3, 10, 41 and 50 only: the duplicates in index order, then the -1 / -inf tail
        assert (ti[2, 4:] == -1).all() and np.isneginf(tv[2, 4:]).all() and (ti[2, :4] >= 0).all()
        got = ti[2, :4].tolist()
        assert got.index(3) < got.index(10) < got.index(41)
        # fewer rows than a tile, and a number of rows that is no multiple of the tile: the same rows, the same bits
        for rows in (37, 130):
            small = gp_ops.mes_pool(b, phi, Xd[:rows], ystar=ystar, maximize=maximize, topk=8, want_score=True)
            assert _same(small["score"], full["score"][:, :rows]), (maximize, rows)
            for t in range(T):
                idx, val = select_ref(sc[t, :rows], 8)
                assert np.array_equal(small["top_idx"][t].cpu().numpy(), idx), (maximize, rows, t)
    empty = gp_ops.mes_pool(b, phi, Xd[:0], ystar=ystar, topk=3, want_score=True)
    assert empty["score"].shape == (T, 0) and bool((empty["top_idx"] == -1).all()) and bool(torch.isneginf(empty["top_val"]).all())
    # a NaN or infinite sample: the task's scores are NaN and nothing of it is selected; the other tasks do not see it
    ref = gp_ops.mes_pool(b, phi, Xd, ystar=ystar, topk=8, want_score=True)
    for bad in (float("nan"), float("inf"), float("-inf")):
        ys2 = ystar.clone()
        ys2[1, 2] = bad
        out = gp_ops.mes_pool(b, phi, Xd, ystar=ys2, topk=8, want_score=True)
        assert bool(torch.isnan(out["score"][1]).all()), bad
        assert bool((out["top_idx"][1] == -1).all()) and bool(torch.isneginf(out["top_val"][1]).all())
        for t in (0, 2, 3):
            assert _same(out["score"][t], ref["score"][t]) and torch.equal(out["top_idx"][t], ref["top_idx"][t])
    with pytest.raises(ValueError):
        gp_ops.mes_pool(b, phi, Xd[:, :4].contiguous(), ystar=ystar)
    with pytest.raises(ValueError):
        gp_ops.mes_pool(b, phi, Xd, ystar=ystar[:2])
    with pytest.raises(RuntimeError):
        gp_ops.mes_pool(b, phi, Xd, ystar=ystar.cpu())


def _alone(b, phi, t, n_s_t):
    from adkf_ift_amd import gp_ops

    b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), b.kernel,
                        n_s=torch.tensor([n_s_t], dtype=torch.int32))
    return b1, phi[t:t + 1].contiguous()


@pytest.mark.parametrize("kernel,ns,d", SHAPES)
def test_a_task_alone_and_inside_a_batch(dev, kernel, ns, d):
    from adkf_ift_amd import gp_ops

    b0, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, kernel, ns, d)
    b = gp_ops.GPBatch(b0.Z_s, b0.y_s, b0.priors, b0.kernel, n_s=torch.tensor(n_s, dtype=torch.int32))    # (no REUSE flag: evaluated at phi)
    g = np.random.default_rng(9)
    ystar = torch.from_numpy((np.array([float(x) for x in best])[:, None] + g.uniform(-2.0, 1.0, (T, 5))).astype(np.float32)).to(dev)
    lists = [[0, 7], [], [3], list(range(1, ROWS, 2))]
    out = gp_ops.mes_pool(b, phi, Xc, ystar=ystar, topk=8, exclude=lists, want_score=True)
    for t in range(T):
        b1, phi1 = _alone(b, phi, t, n_s[t])
        o1 = gp_ops.mes_pool(b1, phi1, Xc, ystar=ystar[t:t + 1].contiguous(), topk=8, exclude=[lists[t]], want_score=True)
        assert _same(o1["score"][0], out["score"][t]), t
        assert torch.equal(o1["top_idx"][0], out["top_idx"][t]) and _same(o1["top_val"][0], out["top_val"][t]), t


def test_more_tasks_than_workgroups(dev):
    """test_gpu_predict_pool.test_more_tasks_than_workgroups's batch: 2000 small tasks, so a workgroup serves several tasks one after
    the other and writes one candidate list per task."""
    from adkf_ift_amd import gp_ops

    Tn, ns, d, rows = 2000, 8, 8, 130
    g = torch.Generator().manual_seed(6)
    n_s = torch.randint(3, ns + 1, (Tn,), generator=g).tolist()
    Zs, ys, _ = M._features(Tn, ns, [0] * Tn, d, 66, True)
    b, phi = M._fit(dev, Zs, ys, n_s, "rbf", True)
    b.flags = 0
    X = P._pool(rows, d, 14).to(dev)
    ystar = (ys.min(1).values[:, None] - torch.rand(Tn, 3, generator=g)).to(dev)
    out = gp_ops.mes_pool(b, phi, X, ystar=ystar, topk=5, exclude=[[t % rows] for t in range(Tn)], want_score=True)
    gp_ops.check_info(out["info"])
    sc, ti, tv = out["score"].cpu().numpy(), out["top_idx"].cpu().numpy(), out["top_val"].cpu().numpy()
    assert np.isfinite(sc).all() and (sc >= 0).all() and (sc > 0).any()
    for t in range(Tn):
        idx, val = select_ref(sc[t], 5, [t % rows])
        assert np.array_equal(ti[t], idx) and np.array_equal(tv[t].view(np.int32), val.view(np.int32)), t
    for t in (0, 777, 1999):
        b1, phi1 = _alone(b, phi, t, n_s[t])
        o1 = gp_ops.mes_pool(b1, phi1, X, ystar=ystar[t:t + 1].contiguous(), topk=5, exclude=[[t % rows]], want_score=True)
        assert _same(o1["score"][0], out["score"][t]) and torch.equal(o1["top_idx"][0], out["top_idx"][t]), t
        post = _oracle_post(Zs[t:t + 1], ys[t:t + 1], [n_s[t]], X.cpu(), phi[t:t + 1], 0)
        _check_against_the_oracle(sc[t:t + 1], post, ystar[t:t + 1].cpu().numpy(), False, f"T2000[{t}]")


def test_the_float64_walk(dev):
    """test_gpu_predict_pool._ill_batch: task 1 takes the float64 walk (asserted there from the fitted scalars), the others a float32
    one - k_mes_walk64 and the tile walk in one call."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, _ = P._ill_batch(dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = P._pool(300, 2, 3) * 0.6
    post = _oracle_post(Zs, ys, n_s, X, phi, 0)
    ystar = _draw_ystar(post, 5, 1)
    out = gp_ops.mes_pool(b, phi, X.to(dev), ystar=torch.from_numpy(ystar).to(dev), maximize=True, topk=7, want_score=True)
    gp_ops.check_info(out["info"])
    sc = out["score"].cpu().numpy()
    _check_against_the_oracle(sc, post, ystar, True, "float64")
    for t in range(4):
        idx, val = select_ref(sc[t], 7)
        assert np.array_equal(out["top_idx"][t].cpu().numpy(), idx) and np.array_equal(out["top_val"][t].cpu().numpy().view(np.int32), val.view(np.int32)), t
    only = gp_ops.mes_pool(b, phi, X.to(dev), ystar=torch.from_numpy(ystar).to(dev), maximize=True, topk=7)
    assert torch.equal(only["top_idx"], out["top_idx"]) and _same(only["top_val"], out["top_val"])


def test_ard(dev):
    """The ARD batch of test_gpu_predict_pool.test_bit_for_bit_ard through the same entry."""
    from adkf_ift_amd import gp_ops

    ns, d = 64, 12
    n_s = [64, 50, 33, 9]
    Zs, ys, _ = M._features(4, ns, [0] * 4, d, 31, True)
    b, phi = MA._fit_ard(dev, Zs, ys, n_s, "matern", True)
    b.flags = gp_ops.REUSE_INNER
    X = P._pool(523, d, 5)
    post = _oracle_post(Zs, ys, n_s, X, phi, 1)
    for maximize in (True, False):
        ystar = _draw_ystar(post if maximize else [(-m, v) for m, v in post], 5, 2)
        ystar = ystar if maximize else -ystar                 # samples of min f
        out = gp_ops.mes_pool(b, phi, X.to(dev), ystar=torch.from_numpy(ystar).to(dev), maximize=maximize, topk=6, want_score=True)
        gp_ops.check_info(out["info"])
        sc = out["score"].cpu().numpy()
        _check_against_the_oracle(sc, post, ystar, maximize, f"ard maximize {maximize}")
        for t in range(4):
            idx, _ = select_ref(sc[t], 6)
            assert np.array_equal(out["top_idx"][t].cpu().numpy(), idx), t


def test_global_row_tile_slots(dev):
    """The last of test_gpu_predict_pool.BIT_CASES: 1024 points, the row tiles in the global slots."""
    from adkf_ift_amd import gp_ops

    kernel, ns, d, rows = P.BIT_CASES[-1]
    n_s = [ns, max(2, ns - 3), max(2, (2 * ns) // 3), max(2, ns // 4)]
    Zs, ys, _ = M._features(4, ns, [0] * 4, d, 300 + ns + d, True)
    b, phi = M._fit(dev, Zs, ys, n_s, kernel, True)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = P._pool(rows, d, 17)
    post = _oracle_post(Zs, ys, n_s, X, phi, gp_ops.kernel_id(kernel))
    ystar = _draw_ystar(post, 5, 3)
    out = gp_ops.mes_pool(b, phi, X.to(dev), ystar=torch.from_numpy(ystar).to(dev), maximize=True, topk=6, want_score=True)
    gp_ops.check_info(out["info"])
    sc = out["score"].cpu().numpy()
    _check_against_the_oracle(sc, post, ystar, True, "global slots")
    for t in range(4):
        idx, _ = select_ref(sc[t], 6)
        assert np.array_equal(out["top_idx"][t].cpu().numpy(), idx), t


def test_guard_bands_exact_sizes_and_a_skipped_task(dev):
    from adkf_ift_amd import _lib, gp_ops

    Tn, ns, d, rows, k, S = 3, 128, 256, 7001, 64, 7
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
    score = torch.full((Tn * rows + guard,), 12345.0, device=dev)
    top_idx = torch.full((Tn * k + guard,), 12345, dtype=torch.int64, device=dev)
    top_val = torch.full((Tn * k + guard,), 12345.0, device=dev)
    sb = lib.adkf_predict_pool_scratch_bytes(Tn, k)
    scratch = torch.full((sb + guard,), 0x5a, dtype=torch.uint8, device=dev)
    info = torch.empty(Tn, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(1)
    ystar = (ys.min(1).values[:, None] - torch.rand(Tn, S, generator=g)).contiguous().to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    cb = b.c_struct()
    rc = lib.adkf_mes_pool(C.byref(cb), p(phi), 0, p(X), rows, p(ystar), S, None, None, p(score), k, p(top_idx), p(top_val), p(info), p(ws),
                           need, p(scratch), sb, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    gp_ops.check_info(info)
    assert bool((score[Tn * rows:] == 12345.0).all())
    assert bool((score[rows:2 * rows] == 0).all())                      # the skipped task's slice
    assert bool((score[:Tn * rows] >= 0).all()) and bool((score[:rows] > 0).any()) and bool((score[2 * rows:3 * rows] > 0).any())
    assert bool((top_idx[Tn * k:] == 12345).all()) and bool((top_val[Tn * k:] == 12345.0).all())
    assert bool((scratch[sb:] == 0x5a).all())
    ti, tv = top_idx[:Tn * k].view(Tn, k).cpu().numpy(), top_val[:Tn * k].view(Tn, k).cpu().numpy()
    assert (ti[1] == -1).all() and np.isneginf(tv[1]).all()
    sc = score[:Tn * rows].view(Tn, rows).cpu().numpy()
    for t in (0, 2):
        idx, val = select_ref(sc[t], k)
        assert np.array_equal(ti[t], idx) and np.array_equal(tv[t].view(np.int32), val.view(np.int32))
    # score == NULL: the same selection, and nothing else is written
    top2 = torch.full((Tn * k + guard,), 12345, dtype=torch.int64, device=dev)
    val2 = torch.full((Tn * k + guard,), 12345.0, device=dev)
    rc = lib.adkf_mes_pool(C.byref(cb), p(phi), 0, p(X), rows, p(ystar), S, None, None, None, k, p(top2), p(val2), p(info), p(ws),
                           need, p(scratch), sb, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0 and torch.equal(top2, top_idx) and _same(val2, top_val) and bool((scratch[sb:] == 0x5a).all())


def test_max_value_samples(dev):
    """One Thompson call without exclusions: ystar is +sel_val with maximize and -sel_val without, the optimum of each drawn path."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, Xc, best, post = L._case(dev, *SHAPES[0])
    omega, phase = gp_ops.rff_basis("rbf", X.shape[1], 256, generator=torch.Generator().manual_seed(0), device=dev)
    for maximize in (False, True):
        mv = gp_ops.max_value_samples(b, phi, X, omega=omega, phase=phase, n_samples=6, generator=torch.Generator().manual_seed(1),
                                      maximize=maximize)
        ts = gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=6, w=mv["w"], eps=mv["eps"], maximize=maximize, want_paths=True)
        opt = ts["paths"].max(2).values if maximize else ts["paths"].min(2).values
        assert mv["ystar"].shape == (T, 6) and _same(mv["ystar"], opt)
        out = gp_ops.mes_pool(b, phi, X, ystar=mv["ystar"], maximize=maximize, topk=4)
        assert bool((out["top_idx"] >= 0).all()) and bool(torch.isfinite(out["top_val"]).all()) and bool((out["top_val"] > 0).all())


def test_bo_loop(dev):
    """The problem of test_gpu_predict_pool.test_batched_bo_loop: records of the right length with distinct picks, a replicate alone
    is the replicate in a batch of four, two runs are equal, and ARD runs.  No claim about regret."""
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=2, num_bo_iters=3, kernel_type="matern", device=dev, init_from=5000, noise_init=0.01,
              noise_prior=True, n_features=256)
    Rn = 4
    recs = BO.run_gp_mes_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(Rn)], **kw)
    assert len(recs) == Rn
    for r in range(Rn):
        assert len(recs[r]) == 1 + 3 * 2 and len(set(recs[r][1:])) == 6, recs[r]
    assert recs == BO.run_gp_mes_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(Rn)], **kw)
    for r in (0, 3):
        alone = BO.run_gp_mes_bo_batched(X, y, rngs=[np.random.default_rng(r)], **kw)
        assert alone[0] == recs[r], (r, "the batch couples replicates")
    ard = BO.run_gp_mes_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(2)], ard=True, **kw)
    for rec in ard:
        assert len(rec) == 1 + 3 * 2 and len(set(rec[1:])) == 6, rec
    with pytest.raises(ValueError):
        BO.run_gp_mes_bo_batched(X, y, rngs=[np.random.default_rng(0)], n_max_samples=65, **kw)
