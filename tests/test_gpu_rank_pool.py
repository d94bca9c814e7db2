"""GPU: adkf_rank_pool on the MI355X.  Every comparison is exact - indices equal, floats bit-equal - against select_ref applied to the
per-row score adkf_predict_pool itself returns for the whole pool: the selection at k from 1 to 65536 over several chunks, the ranks
and scores of named rows (the pool-equals-packed statement of this entry), n_ranked, ties across chunks and across the k-th place,
the prefix that is predict_pool's selection on every kind of task, evaluate.screen and evaluate.enrichment, the bitwise properties and
the edge cases."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_log_ei as L
import test_gpu_predict_marginal as M
import test_gpu_predict_marginal_ard as MA
import test_gpu_predict_pool as P
from test_gpu_levelset_pool import _lists
from test_predict_pool_cpu import select_ref
from test_rank_pool_cpu import rank_ref

pytestmark = pytest.mark.gpu

CHUNK = 16384
ROWS = 2 * CHUNK + 777          # two full chunks and a partial tile
KS = (1, 64, 65, 1000, 4097, 16384)
SCORES = (("ei", False, False), ("ei", True, True), ("mean", True, False), ("mean", False, False))   # (score, maximize, log_ei)
KEYS = ("top_idx", "top_val", "ref_rank", "ref_val", "n_ranked")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, c, t=None, u=None, keys=KEYS):
    for n in keys:
        x, y = a[n], c[n]
        if x is None or y is None:
            assert x is None and y is None, n
            continue
        if t is not None:
            x, y = x[t], y[u]
        assert torch.equal(_bits(x), _bits(y)), n


_built = {}


def _batch(dev, name):
    """(b, phi, X [ROWS, d], best [T]) of one kind of batch, built once and left unchanged: the two batches of test_gpu_log_ei._case
    (plain and refined tasks), P._ill_batch (task 1 takes the float64 walk) and an ARD batch as test_pool_equals_packed builds it."""
    from adkf_ift_amd import gp_ops

    if name not in _built:
        best = torch.tensor([0.1, -0.2, 0.3, 0.0], device=dev)
        if name in ("plain", "refined"):
            b, phi, *_ = L._case(dev, *L.SHAPES[0 if name == "plain" else 1])
            X = P._pool(ROWS, b.d, 21)
        elif name == "float64":
            b, phi, *_ = P._ill_batch(dev)
            b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
            X = torch.cat([P._pool(ROWS - 5, 2, 3), b.Z_s[1, :5].cpu()])
        else:
            Zs, ys, _ = M._features(4, 32, [0] * 4, 12, 31, True)
            b, phi = MA._fit_ard(dev, Zs, ys, [32, 25, 17, 9], "matern", True)
            b.flags = gp_ops.REUSE_INNER
            X = P._pool(ROWS, 12, 5)
        _built[name] = (b, phi, X.to(dev).contiguous(), best)
    return _built[name]


def _pool_score(b, phi, X, best, score, maximize, log_ei):
    """The per-row score adkf_predict_pool itself returns for the whole pool: numpy [T, rows]."""
    from adkf_ift_amd import gp_ops

    if score == "mean":
        m = gp_ops.predict_pool(b, phi, X, want_var=False, want_ei=False)["mean"]
        return (m if maximize else -m).cpu().numpy()
    return gp_ops.predict_pool(b, phi, X, best_f=best, maximize=maximize, log_ei=log_ei, want_mean=False, want_var=False)["ei"].cpu().numpy()


def _check(out, sc, lists, k, refs, tag):
    """A whole result against the reference on the score sc [T, rows]."""
    T, rows = sc.shape
    ti, tv = (out[n].cpu().numpy() if out[n] is not None else None for n in ("top_idx", "top_val"))
    nr = out["n_ranked"].cpu().numpy()
    row = np.arange(rows)
    for t in range(T):
        idx, val = select_ref(sc[t], k, lists[t])
        if k > 0:
            assert np.array_equal(ti[t], idx), (tag, t, "top_idx")
            assert np.array_equal(tv[t].view(np.int32), val.view(np.int32)), (tag, t, "top_val")
        ok = ~np.isnan(sc[t])
        ok[np.asarray(lists[t], np.int64)] = False
        assert nr[t] == ok.sum(), (tag, t, "n_ranked")
        if refs is None:
            continue
        rr, rv = out["ref_rank"][t].cpu().numpy(), out["ref_val"][t].cpu().numpy()
        for j, r in enumerate(refs[t].tolist()):
            if r < 0 or r >= rows or np.isnan(sc[t, r]):
                assert rr[j] == -1 and np.isnan(rv[j]), (tag, t, j)
                continue
            # the rank restated (test_rank_pool_cpu.rank_ref): the eligible rows that come strictly before row r
            want = int((ok & ((sc[t] > sc[t, r]) | ((sc[t] == sc[t, r]) & (row < r)))).sum())
            assert rr[j] == want, (tag, t, j, r, rr[j], want)
            assert rv[j].view(np.int32) == sc[t, r].view(np.int32), (tag, t, j, r)   # pool equals packed, for this entry
            if want < k and ok[r]:
                assert ti[t, want] == r, (tag, t, j)


def _refs(rows, T, lists, seed):
    """64 rows per task: some in each chunk, some excluded, one beyond the pool, one -1, one repeated."""
    g = torch.Generator().manual_seed(seed)
    refs = torch.randint(0, rows, (T, 64), generator=g)
    refs[:, 0], refs[:, 1], refs[:, 2] = 0, 7, rows - 1          # _lists excludes them for every third task
    refs[:, 3], refs[:, 4] = rows, -1
    refs[:, 5] = refs[:, 6]
    refs[:, 7], refs[:, 8], refs[:, 9] = 5, CHUNK + 5, 2 * CHUNK + 9
    for c in range((rows + CHUNK - 1) // CHUNK):
        refs[:, 10 + c] = min(c * CHUNK + 100, rows - 1)
    for t, l in enumerate(lists):
        if len(l) > 64:   # the task that excludes nearly everything: name rows it may list, and some it may not
            free = sorted(set(range(rows)) - set(l))
            refs[t, 20:20 + len(free)] = torch.tensor(free)
    return refs.to(torch.int64)


FREE = (1, CHUNK, 20000, 33000, ROWS - 1)   # what task 3 may list


@pytest.mark.parametrize("name", ["plain", "refined", "float64", "ard"])
def test_against_predictions_own_rows(dev, name):
    from adkf_ift_amd import gp_ops

    b, phi, X, best = _batch(dev, name)
    lists = _lists(ROWS, b.T)
    lists[3] = [r for r in range(ROWS) if r not in FREE]
    refs = _refs(ROWS, b.T, lists, 17)
    excl = gp_ops.pack_exclude(lists, b.T, ROWS, dev)
    for score, maximize, log_ei in SCORES:
        sc = _pool_score(b, phi, X, best, score, maximize, log_ei)
        for k in KS:
            out = gp_ops.rank_pool(b, phi, X, best_f=best, maximize=maximize, score=score, log_ei=log_ei, topk=k, rank_rows=refs.to(dev),
                                   exclude=excl)
            gp_ops.check_info(out["info"])
            _check(out, sc, lists, k, refs.numpy(), (name, score, maximize, log_ei, k))
            if k >= 64:
                assert out["top_idx"][3, :5].tolist() == sorted(FREE, key=lambda r: (-float(sc[3, r]), r)) and bool((out["top_idx"][3, 5:] == -1).all())


def test_ties_across_chunks_and_across_the_kth_place(dev):
    from adkf_ift_amd import gp_ops

    b, phi, X, best = _batch(dev, "plain")
    X = X.clone()
    X[CHUNK + 5] = X[5]
    X[2 * CHUNK + 9] = X[5]
    none = [[] for _ in range(b.T)]
    for score, maximize, log_ei in SCORES[1:3]:
        sc = _pool_score(b, phi, X, best, score, maximize, log_ei)
        rho = rank_ref(sc[0], [], 5)
        k = rho + 2
        refs = torch.tensor([[5, CHUNK + 5, 2 * CHUNK + 9]] * b.T)
        out = gp_ops.rank_pool(b, phi, X, best_f=best, maximize=maximize, score=score, log_ei=log_ei, topk=k, rank_rows=refs.to(dev))
        top = out["top_idx"][0].tolist()
        print(f"{score}: row 5 has rank {rho} for task 0, k = {k}")
        assert top[rho] == 5 and top[rho + 1] == CHUNK + 5 and 2 * CHUNK + 9 not in top, "the tie did not straddle the k-th place"
        assert out["ref_rank"][0].tolist() == [rho, rho + 1, rho + 2]
        _check(out, sc, none, k, refs.numpy(), ("ties", score))


def test_the_largest_k(dev):
    from adkf_ift_amd import gp_ops

    rows, k = 4 * CHUNK + 777, 65536
    Zs, ys, _ = M._features(2, 32, [0] * 2, 16, 87, True)
    b, phi = M._fit(dev, Zs, ys, [32, 29], "rbf", True)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = P._pool(rows, 16, 23).to(dev)
    best = torch.tensor([0.1, -0.2], device=dev)
    lists = [[0, 7, rows - 1], []]
    refs = _refs(rows, 2, lists, 19)
    sc = _pool_score(b, phi, X, best, "ei", False, True)
    out = gp_ops.rank_pool(b, phi, X, best_f=best, log_ei=True, topk=k, rank_rows=refs.to(dev), exclude=lists)
    _check(out, sc, lists, k, refs.numpy(), "largest k")
    assert bool((out["top_idx"] >= 0).all())
    # a pool far smaller than k: the tail
    out = gp_ops.rank_pool(b, phi, X[:100].contiguous(), score="mean", maximize=True, topk=k)
    sc = _pool_score(b, phi, X[:100].contiguous(), best, "mean", True, False)
    _check(out, sc, [[], []], k, None, "rows < k")
    assert bool((out["top_idx"][:, 100:] == -1).all()) and bool(torch.isneginf(out["top_val"][:, 100:]).all())
    assert bool((out["top_idx"][:, :100] >= 0).all()) and out["n_ranked"].tolist() == [100, 100]


@pytest.mark.parametrize("name", ["plain", "refined", "float64", "ard"])
def test_the_prefix_is_predict_pools_selection(dev, name):
    from adkf_ift_amd import gp_ops

    b, phi, X, best = _batch(dev, name)
    X = X[:CHUNK + 300].contiguous()
    lists = _lists(X.shape[0], b.T)
    for score, maximize, log_ei in SCORES:
        pp = gp_ops.predict_pool(b, phi, X, best_f=best, maximize=maximize, score=score, log_ei=log_ei, want_mean=False, want_var=False,
                                 want_ei=False, topk=64, exclude=lists)
        out = gp_ops.rank_pool(b, phi, X, best_f=best, maximize=maximize, score=score, log_ei=log_ei, topk=200, exclude=lists)
        assert torch.equal(out["top_idx"][:, :64], pp["top_idx"]), (name, score)
        assert torch.equal(_bits(out["top_val"][:, :64]), _bits(pp["top_val"])), (name, score)


def test_screen_and_enrichment(dev):
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
    base = Z_q[2, :130].float()
    g = torch.Generator().manual_seed(5)
    lib_rows = torch.cat([base + 0.05 * j * torch.randn(base.shape, generator=g).to(dev) for j in range(6)]).contiguous()   # 780 rows
    rows = lib_rows.shape[0]
    model.eval()
    with torch.no_grad():
        b, phi_ref = E._fitted_support(model, mb, 200, "reference")
    for maximize in (True, False):
        m = gp_ops.predict_pool(b, phi_ref, lib_rows, want_var=False, want_ei=False)["mean"]
        sc = (m if maximize else -m).cpu().numpy()
        # k = 5: the path and the answer of before
        top_idx, top_val, phi = E.screen(model, mb, lib_rows, 5, maximize=maximize)
        pp = gp_ops.predict_pool(b, phi_ref, lib_rows, maximize=maximize, score="mean", want_mean=False, want_var=False, topk=5)
        assert torch.equal(phi, phi_ref) and torch.equal(top_idx, pp["top_idx"]) and torch.equal(_bits(top_val), _bits(pp["top_val"]))
        # k = 500: beyond the cap of the other entries
        top_idx, top_val, phi = E.screen(model, mb, lib_rows, 500, maximize=maximize)
        assert torch.equal(phi, phi_ref) and top_idx.shape == (3, 500) and top_idx.dtype == torch.int64
        for t in range(3):
            idx, val = select_ref(sc[t], 500)
            assert np.array_equal(top_idx[t].cpu().numpy(), idx) and np.array_equal(top_val[t].cpu().numpy().view(np.int32), val.view(np.int32))
        # enrichment: the actives' ranks are their places in that order
        actives = [[3, 100, 700], [5], [0, 1, 2, 779]]
        ranks, n_ranked, ef, phi = E.enrichment(model, mb, lib_rows, actives, fractions=(0.01, 0.1), maximize=maximize, exclude=[[3], [], [779]])
        assert torch.equal(phi, phi_ref) and ranks.shape == (3, 4) and n_ranked.tolist() == [rows - 1, rows, rows - 1]
        lists = [[3], [], [779]]
        for t in range(3):
            want = [rank_ref(sc[t], lists[t], r) for r in actives[t]] + [-1] * (4 - len(actives[t]))
            assert ranks[t].tolist() == want
        assert torch.equal(ef, E.enrichment_from_ranks(ranks.cpu(), n_ranked.cpu(), (0.01, 0.1))) and ef.shape == (3, 2)


def test_bitwise_properties(dev):
    """Two calls agree; outputs not asked for change nothing (M = 0 against M > 0, k = 0 against k > 0); a task alone is the task in the
    batch; a replayed graph gives the eager call's bits."""
    from adkf_ift_amd import _lib, gp_ops

    b, phi, X, best = _batch(dev, "plain")
    T, k = b.T, 1000
    lists = _lists(ROWS, T)
    refs = _refs(ROWS, T, lists, 23).to(dev)
    kw = dict(best_f=best, log_ei=True, exclude=lists)
    first = gp_ops.rank_pool(b, phi, X, topk=k, rank_rows=refs, **kw)
    _same(first, gp_ops.rank_pool(b, phi, X, topk=k, rank_rows=refs, **kw))
    _same(first, gp_ops.rank_pool(b, phi, X, topk=k, **kw), keys=("top_idx", "top_val", "n_ranked"))
    _same(first, gp_ops.rank_pool(b, phi, X, topk=0, rank_rows=refs, **kw), keys=("ref_rank", "ref_val", "n_ranked"))
    _same(first, gp_ops.rank_pool(b, phi, X, topk=k, rank_rows=refs, latent=True, **kw))
    flags = b.flags
    try:
        b.flags = 0   # (both evaluate at phi: no state of a fit is reused)
        full = gp_ops.rank_pool(b, phi, X, topk=k, rank_rows=refs, **kw)
        n_s = b.n_s.tolist()
        for t in range(T):
            b1 = gp_ops.GPBatch(b.Z_s[t:t + 1].contiguous(), b.y_s[t:t + 1].contiguous(), b.priors[t:t + 1].contiguous(), b.kernel,
                                n_s=torch.tensor([n_s[t]], dtype=torch.int32))
            o1 = gp_ops.rank_pool(b1, phi[t:t + 1].contiguous(), X, best_f=best[t:t + 1], log_ei=True, exclude=[lists[t]], topk=k,
                                  rank_rows=refs[t:t + 1].contiguous())
            _same(o1, full, 0, t)
    finally:
        b.flags = flags
    # graph replay, as test_gpu_gumbel_pool captures its entry
    lib = _lib.load()
    M_ = refs.shape[1]
    out = dict(top_idx=torch.zeros(T, k, dtype=torch.int64, device=dev), top_val=torch.zeros(T, k, device=dev),
               ref_rank=torch.zeros(T, M_, dtype=torch.int64, device=dev), ref_val=torch.zeros(T, M_, device=dev),
               n_ranked=torch.zeros(T, dtype=torch.int64, device=dev))
    info = torch.zeros(T, dtype=torch.int32, device=dev)
    e_idx, e_off = gp_ops.pack_exclude(lists, T, ROWS, dev)
    sb = lib.adkf_rank_pool_scratch_bytes(T, k, M_, b.d)
    scratch = torch.zeros(sb, dtype=torch.uint8, device=dev)
    ws, nb = b.workspace()
    cb = b.c_struct()
    p = lambda t: C.c_void_p(t.data_ptr())

    def call():
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        return lib.adkf_rank_pool(C.byref(cb), p(phi), 16, p(X), ROWS, p(best), p(e_idx), p(e_off), k, p(out["top_idx"]), p(out["top_val"]),
                                  p(refs), M_, p(out["ref_rank"]), p(out["ref_val"]), p(out["n_ranked"]), p(info), p(ws), nb, p(scratch), sb, st)

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call() == 0
    for _ in range(2):
        for n in out:
            out[n].fill_(7)
        info.fill_(5)
        scratch.fill_(0x5a)
        graph.replay()
        torch.cuda.synchronize()
        assert bool((info == 0).all())
        _same(first, out)


def test_edge_cases(dev):
    from adkf_ift_amd import gp_ops

    T, ns, d = 4, 16, 8
    Zs, ys, _ = M._features(T, ns, [0] * T, d, 4, True)
    b, phi = M._fit(dev, Zs, ys, [16, 8, 12, 5], "rbf", True)
    best = torch.zeros(T, device=dev)
    X = P._pool(3000, d, 2).to(dev)
    refs = torch.tensor([[0, 1, -1, 2999]] * T, device=dev)
    # no rows at all
    out = gp_ops.rank_pool(b, phi, X[:0], best_f=best, topk=3, rank_rows=refs)
    assert bool((out["top_idx"] == -1).all()) and bool(torch.isneginf(out["top_val"]).all())
    assert bool((out["ref_rank"] == -1).all()) and bool(torch.isnan(out["ref_val"]).all()) and out["n_ranked"].tolist() == [0] * T
    # one row, k = 1, and k = 0 with the count alone
    for k in (1, 3):
        out = gp_ops.rank_pool(b, phi, X[:1].contiguous(), best_f=best, topk=k, rank_rows=refs)
        _check(out, _pool_score(b, phi, X[:1].contiguous(), best, "ei", False, False), [[]] * T, k, refs.cpu().numpy(), ("one row", k))
    out = gp_ops.rank_pool(b, phi, X, best_f=best, topk=1, exclude=[[int(i)] for i in gp_ops.rank_pool(b, phi, X, best_f=best, topk=1)["top_idx"][:, 0]])
    sc = _pool_score(b, phi, X, best, "ei", False, False)
    assert out["top_idx"][:, 0].tolist() == [int(select_ref(sc[t], 2)[0][1]) for t in range(T)]
    out = gp_ops.rank_pool(b, phi, X, best_f=best)
    assert out["top_idx"] is None and out["ref_rank"] is None and out["n_ranked"].tolist() == [3000] * T
    # a pool row with a NaN feature: whatever prediction makes of it (the clamps of the squared distance and of the variance swallow a
    # NaN on the device, so the row can come out with a number), the ranking is the reference's on prediction's own score
    Xn = X.clone()
    Xn[1234, 3] = float("nan")
    refs_n = torch.tensor([[1234, 1233, 1235, 0]] * T, device=dev)
    for score, maximize, log_ei in SCORES:
        sc = _pool_score(b, phi, Xn, best, score, maximize, log_ei)
        out = gp_ops.rank_pool(b, phi, Xn, best_f=best, maximize=maximize, score=score, log_ei=log_ei, topk=3000, rank_rows=refs_n)
        print(f"NaN feature, {score} maximize={maximize} log_ei={log_ei}: the row's scores {sc[:, 1234].tolist()}")
        _check(out, sc, [[]] * T, 3000, refs_n.cpu().numpy(), ("nan row", score))
    # NaN scores: a NaN best_f makes every EI of task 1 NaN - nothing listed, nothing ranked, every rank -1; the others as before
    bad = best.clone()
    bad[1] = float("nan")
    for log_ei in (False, True):
        sc = _pool_score(b, phi, X, bad, "ei", False, log_ei)
        assert np.isnan(sc[1]).all() and not np.isnan(sc[[0, 2, 3]]).any(), "the premise: task 1 has NaN scores only"
        out = gp_ops.rank_pool(b, phi, X, best_f=bad, log_ei=log_ei, topk=100, rank_rows=refs)
        _check(out, sc, [[]] * T, 100, refs.cpu().numpy(), ("nan scores", log_ei))
        assert bool((out["top_idx"][1] == -1).all()) and bool((out["ref_rank"][1] == -1).all()) and out["n_ranked"].tolist() == [3000, 0, 3000, 3000]
    # all-zero EI: 3 000 rows tied, listed in index order but for the excluded ones
    low = torch.full((T,), -1000.0, device=dev)
    sc = _pool_score(b, phi, X, low, "ei", False, False)
    assert (sc == 0).all(), "the premise: EI is 0 on the whole pool"
    lists = [[0, 2, 5], [], [1], [2999]]
    out = gp_ops.rank_pool(b, phi, X, best_f=low, topk=2998, rank_rows=refs, exclude=lists)
    _check(out, sc, lists, 2998, refs.cpu().numpy(), "zeros")
    for t in range(T):
        free = [r for r in range(3000) if r not in lists[t]][:2998]
        assert out["top_idx"][t].tolist() == free + [-1] * (2998 - len(free))
    # a skipped task: the fills
    n_s = b.n_s.clone()
    try:
        b.n_s = torch.tensor([16, 0, 12, 5], dtype=torch.int32, device=dev)
        out = gp_ops.rank_pool(b, phi, X, best_f=best, topk=100, rank_rows=refs)
        assert bool((out["top_idx"][1] == -1).all()) and bool(torch.isneginf(out["top_val"][1]).all())
        assert bool((out["ref_rank"][1] == -1).all()) and bool(torch.isnan(out["ref_val"][1]).all()) and out["n_ranked"].tolist() == [3000, 0, 3000, 3000]
        sc = _pool_score(b, phi, X, best, "ei", False, False)
        for t in (0, 2, 3):
            idx, val = select_ref(sc[t], 100)
            assert np.array_equal(out["top_idx"][t].cpu().numpy(), idx) and np.array_equal(out["top_val"][t].cpu().numpy().view(np.int32), val.view(np.int32))
    finally:
        b.n_s = n_s
    with pytest.raises(ValueError):
        gp_ops.rank_pool(b, phi, X, topk=3)                      # ranking by EI without best_f
    with pytest.raises(ValueError):
        gp_ops.rank_pool(b, phi, X, best_f=best, topk=65537)
    with pytest.raises(RuntimeError):
        gp_ops.rank_pool(b, phi, X.cpu(), best_f=best, topk=3)
