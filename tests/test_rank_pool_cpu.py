"""CPU: adkf_rank_pool without a GPU - the entry is exported, clean refusal with no device, every argument check before any launch, the
scratch formula, gp_ops.rank_pool's argument handling, and on the CPU twin, bit for bit: the selection against select_ref applied to
the per-row score adkf_predict_pool itself returns (both kernels, isotropic and ARD, EI / log EI / +-mean, with and without exclusion
lists, k up to and beyond the pool), the prefix that is predict_pool's selection, the ranks of every row, zeros, signed zeros; and
evaluate.enrichment_from_ranks on cases worked out by hand."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from adkf_ift_amd import _lib
from test_predict_pool_cpu import _call as pool_call, _problem, _twin, lib, select_ref  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE, SCORE_MEAN, LOG_EI = 1, 2, 4, 16
CHUNK = 16384


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, k=4, M=0, ard=False, flags=0, x=True, best=True, top=(True, True), refs=(True, True, True),
               ranked=True, excl=(False, False), info=True, ws=True, ws_short=0, scratch=True, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    small = min(max(rows, 1), 64)   # (a refused call never looks at its buffers)
    X = torch.zeros(small, d) if x else None
    kk, mm = min(max(k, 1), 64), min(max(M, 1), 64)
    bf, inf = torch.zeros(T), torch.zeros(T, dtype=torch.int32)
    top_idx, top_val = torch.zeros(T * kk, dtype=torch.int64), torch.zeros(T * kk)
    r_idx, r_rank, r_val = torch.zeros(T * mm, dtype=torch.int64), torch.zeros(T * mm, dtype=torch.int64), torch.zeros(T * mm)
    nr = torch.zeros(T, dtype=torch.int64)
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_rank_pool_scratch_bytes(T, min(max(k, 0), 64), min(max(M, 0), 64), d)
    sc = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_rank_pool(C.byref(b), p(phi), flags, p(X), rows, p(bf) if best else None, p(e_idx) if excl[0] else None,
                              p(e_off) if excl[1] else None, k, p(top_idx) if top[0] else None, p(top_val) if top[1] else None,
                              p(r_idx) if refs[0] else None, M, p(r_rank) if refs[1] else None, p(r_val) if refs[2] else None,
                              p(nr) if ranked else None, p(inf) if info else None, p(wsb) if ws else None, nb - ws_short,
                              C.c_void_p(sc.data_ptr() + scratch_off) if scratch else None, sb - scratch_short, None)


def test_the_entry_is_exported(lib):
    assert "adkf_rank_pool" in _lib.SIGNATURES and "adkf_rank_pool_scratch_bytes" in _lib.SIGNATURES
    fn = lib.adkf_rank_pool   # a library without the entry point fails here
    assert fn.restype is C.c_int and len(fn.argtypes) == 22
    assert len(lib.adkf_rank_pool_scratch_bytes.argtypes) == 4
    assert (_lib.RANK_K_MAX, _lib.RANK_REFS_MAX, _lib.RANK_CHUNK_ROWS) == (65536, 1024, CHUNK)
    assert _lib.POOL_TOPK_MAX == 64   # the other entries keep their cap


def test_the_scratch_formula(lib):
    """include/adkf_gp.h: every part rounded up to 256 bytes; no argument for rows or ns, so it depends on neither."""
    r = lambda x: (x + 255) // 256 * 256
    f = lib.adkf_rank_pool_scratch_bytes
    for T, k, M, d in ((3, 4, 0, 8), (1, 65536, 1024, 5), (4, 1000, 64, 16), (256, 16384, 64, 256), (300, 0, 7, 3), (2, 1, 1, 1)):
        want = r(4 * T * CHUNK) + r(16 * T * k) + r(8 * T * k) + r(8 * T) + r(4 * T * M * d) + 2 * r(4 * T * M) + r(8 * (T + 1))
        assert f(T, k, M, d) == want, (T, k, M, d)
    assert f(256, 65536, 0, 256) < 1 << 29   # 256 tasks at the largest k: under half a gigabyte, whatever the pool
    for shape in ((0, 4, 0, 8), (3, -1, 0, 8), (3, 65537, 0, 8), (3, 4, -1, 8), (3, 4, 1025, 8), (3, 4, 0, 0)):
        assert f(*shape) == 0, shape


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, rows=0, x=False, k=0, ranked=True) == LAUNCH
    assert _host_call(lib, ard=True, d=12, rows=7, k=3, M=5, flags=SCORE_MEAN | MAXIMIZE, best=False) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, k=64, M=64, excl=(True, True), flags=LOG_EI | LATENT) == LAUNCH
    assert _host_call(lib, k=0, M=3, ranked=False) == LAUNCH


@pytest.mark.parametrize("ard", [False, True])
def test_bad_arguments_are_rejected_before_any_launch(lib, ard):
    call = lambda **kw: _host_call(lib, ard=ard, **kw)
    assert call(nq=4) == BADARG                                     # a batch with a query set
    for bit in (8, 32, 64, 128):
        assert call(flags=bit) == BADARG                            # flag bits other than the four
        assert call(flags=bit | MAXIMIZE) == BADARG
    assert call(flags=LOG_EI | SCORE_MEAN) == BADARG                # nothing would read log EI
    assert call(rows=-1) == BADARG
    assert call(x=False) == BADARG                                  # rows > 0 without X
    assert call(best=False) == BADARG                               # EI without best_f
    assert call(best=False, flags=LOG_EI) == BADARG
    assert call(k=-1) == BADARG
    assert call(M=-1) == BADARG
    assert call(top=(False, True)) == BADARG                        # k > 0 without top_*
    assert call(top=(True, False)) == BADARG
    for refs in ((False, True, True), (True, False, True), (True, True, False)):
        assert call(M=3, refs=refs) == BADARG                       # M > 0 without ref_idx / ref_rank / ref_val
    assert call(k=0, M=0, ranked=False) == BADARG                   # nothing asked for
    assert call(info=False) == BADARG
    assert call(ws=False) == BADARG
    assert call(scratch=False) == BADARG
    assert call(excl=(True, False)) == BADARG                       # excl_idx without excl_off
    assert call(k=65537) == SIZE
    assert call(M=1025) == SIZE
    assert call(k=65537, top=(False, False)) == SIZE                # the size comes before the outputs, as in adkf_mix_pool
    assert call(ws_short=1) == WORKSPACE
    assert call(scratch_short=1) == WORKSPACE
    assert call(M=4, scratch_short=8) == WORKSPACE
    assert call(scratch_off=4) == WORKSPACE                         # a scratch off by 4 bytes
    assert call(k=0, M=2, scratch_off=4) == WORKSPACE


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False, T=3, d=5, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.rank_pool(types.SimpleNamespace(nq=3, ard=False, T=3, d=5), None, None, topk=4)
    with pytest.raises(ValueError, match="score must be"):
        gp_ops.rank_pool(iso, None, None, score="ucb", topk=4)
    with pytest.raises(ValueError, match="log_ei"):
        gp_ops.rank_pool(iso, None, None, score="mean", log_ei=True, topk=4)
    for k in (-1, 65537):
        with pytest.raises(ValueError, match="topk must be"):
            gp_ops.rank_pool(iso, None, None, score="mean", topk=k)
    with pytest.raises(ValueError, match="rank_rows must be"):
        gp_ops.rank_pool(iso, None, None, score="mean", rank_rows=torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="rank_rows must be"):
        gp_ops.rank_pool(iso, None, None, score="mean", rank_rows=torch.zeros(3, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="rank_rows must be"):
        gp_ops.rank_pool(iso, None, None, score="mean", rank_rows=[[1], [2]])
    with pytest.raises(ValueError, match="ranked rows M"):
        gp_ops.rank_pool(iso, None, None, score="mean", rank_rows=torch.zeros(3, 1025, dtype=torch.int64))
    with pytest.raises(ValueError, match="best_f"):
        gp_ops.rank_pool(iso, None, None, topk=4)
    with pytest.raises(ValueError, match="best_f must have"):
        gp_ops.rank_pool(iso, None, None, topk=4, best_f=torch.zeros(2))


# ---- the twin
def _rank_twin():
    cpu_twin, pool_fn = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_rank_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_rank_pool"]
    assert tw.adkf_rank_pool_scratch_bytes(3, 100, 8, 4) == 0
    return fn, pool_fn


def rank_call(fn, b, phi, flags, X, best, k=0, refs=None, excl=None, want_ranked=True, ok_info=True):
    """The twin's adkf_rank_pool on host arrays: a dict as gp_ops.rank_pool returns it."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, rows = b.T, X.shape[0]
    top_idx = np.full((T, max(k, 1)), -7, np.int64)
    top_val = np.full((T, max(k, 1)), np.nan, np.float32)
    refs = None if refs is None else np.ascontiguousarray(refs, np.int64)
    M = 0 if refs is None else refs.shape[1]
    ref_rank = np.full((T, max(M, 1)), -7, np.int64)
    ref_val = np.full((T, max(M, 1)), 7.0, np.float32)
    n_ranked = np.full(T, -7, np.int64)
    info = np.empty(T, np.int32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(X), rows, pp(best), pp(e_idx), pp(e_off), k, pp(top_idx) if k else None,
            pp(top_val) if k else None, pp(refs), M, pp(ref_rank) if M else None, pp(ref_val) if M else None,
            pp(n_ranked) if want_ranked else None, pp(info), None, 0, None, 0, None)
    assert rc == 0
    if ok_info:
        assert (info == 0).all()
    return dict(top_idx=top_idx[:, :k], top_val=top_val[:, :k], ref_rank=ref_rank[:, :M], ref_val=ref_val[:, :M], n_ranked=n_ranked, info=info)


def pool_score(pool_fn, b, phi, flags, X, best):
    """The per-row score adkf_predict_pool itself returns for the whole pool, [T, rows]."""
    mean, _, ei, _, _ = pool_call(pool_fn, b, phi, flags & ~SCORE_MEAN, X, best)
    if flags & SCORE_MEAN:
        return mean if flags & MAXIMIZE else -mean
    return ei


def rank_ref(score, excluded, r):
    """The rank of row r restated: the eligible rows that come strictly before it in select_ref's order; -1 for a NaN score."""
    score = np.asarray(score, np.float32)
    if r < 0 or r >= score.shape[0] or np.isnan(score[r]):
        return -1
    ok = ~np.isnan(score)
    ok[np.asarray(list(excluded), np.int64)] = False
    idx = np.arange(score.shape[0])
    return int((ok & ((score > score[r]) | ((score == score[r]) & (idx < r)))).sum())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _lists70(score0):
    lists = [sorted({int(np.argmax(score0)), 5, 6}), [], sorted(set(range(70)) - {3, 10, 41, 50})]
    e_idx = np.array([i for l in lists for i in l], np.int64)
    e_off = np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64)
    return lists, (e_idx, e_off)


FLAG_SETS = (LATENT, LATENT | MAXIMIZE, LOG_EI, LOG_EI | MAXIMIZE, SCORE_MEAN, SCORE_MEAN | MAXIMIZE)


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_the_twin_against_select_ref(kind, ard):
    fn, pool_fn = _rank_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(kind, ard, 40 + ard + 2 * kind, rows=70)
    X[10] = X[3]; X[41] = X[3]; X[69] = X[20]          # exact duplicate rows: bit-equal scores
    for flags in FLAG_SETS:
        score = pool_score(pool_fn, b, phi, flags, X, best)
        lists, packed = _lists70(score[0])
        for excl, ls in ((packed, lists), (None, [[], [], []])):
            for k in (1, 7, 64, 65, 70, 200):
                out = rank_call(fn, b, phi, flags, X, best, k=k, excl=excl)
                for t in range(b.T):
                    idx, val = select_ref(score[t], k, ls[t])
                    assert np.array_equal(out["top_idx"][t], idx), (flags, k, t)
                    assert np.array_equal(_bits(out["top_val"][t]), _bits(val)), (flags, k, t)
                    assert out["n_ranked"][t] == 70 - len(ls[t])
                if k == 200:   # k > rows: the -1 / -inf tail
                    assert (out["top_idx"][:, 70:] == -1).all() and np.isneginf(out["top_val"][:, 70:]).all()
                if excl is not None and k >= 7:   # task 2 has four eligible rows: the duplicates in index order
                    got = out["top_idx"][2, :4].tolist()
                    assert got.index(3) < got.index(10) < got.index(41) and (out["top_idx"][2, 4:] == -1).all()


@pytest.mark.parametrize("ard", [False, True])
def test_the_prefix_is_predict_pools_selection(ard):
    fn, pool_fn = _rank_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(1, ard, 47 + ard, rows=70)
    X[10] = X[3]; X[41] = X[3]
    for flags in FLAG_SETS:
        _, packed = _lists70(pool_score(pool_fn, b, phi, flags, X, best)[0])
        for excl in (packed, None):
            _, _, _, ti, tv = pool_call(pool_fn, b, phi, flags, X, best, k=64, excl=excl, per_row=False)
            for k in (64, 70, 200):
                out = rank_call(fn, b, phi, flags, X, best, k=k, excl=excl)
                assert np.array_equal(out["top_idx"][:, :64], ti) and np.array_equal(_bits(out["top_val"][:, :64]), _bits(tv)), (flags, k)


@pytest.mark.parametrize("ard", [False, True])
def test_the_ranks_of_every_row(ard):
    fn, pool_fn = _rank_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(0, ard, 52 + ard, rows=70)
    X[10] = X[3]; X[41] = X[3]; X[69] = X[20]
    X[33, 2] = np.nan                                    # one pool row with a NaN feature: its score is NaN for every task
    refs = np.tile(np.concatenate([np.arange(70), [-1, 70, 3, 3]]).astype(np.int64), (b.T, 1))   # every row, two outside, one repeated
    for flags in FLAG_SETS:
        score = pool_score(pool_fn, b, phi, flags, X, best)
        assert np.isnan(score[:, 33]).all() and np.isnan(score).sum() == b.T
        lists, packed = _lists70(np.nan_to_num(score[0], nan=-np.inf))
        for excl, ls in ((packed, lists), (None, [[], [], []])):
            out = rank_call(fn, b, phi, flags, X, best, k=70, refs=refs, excl=excl)
            for t in range(b.T):
                order, _ = select_ref(score[t], 70, ls[t])
                n = int((order >= 0).sum())
                assert out["n_ranked"][t] == n == 70 - len(set(ls[t]) | {33})
                want = [rank_ref(score[t], ls[t], int(r)) for r in refs[t]]
                assert out["ref_rank"][t].tolist() == want, (flags, t)
                for j, r in enumerate(refs[t].tolist()):
                    if want[j] < 0:
                        assert np.isnan(out["ref_val"][t, j]) and (r in (-1, 70, 33))
                        continue
                    assert _bits(out["ref_val"][t, j]) == _bits(score[t, r])
                    if r not in ls[t]:   # an eligible row: its rank is its position in select_ref's order
                        assert order[want[j]] == r and out["top_idx"][t, want[j]] == r
                    else:                # an excluded row: its insertion position
                        assert r not in order.tolist() and 0 <= want[j] <= n
                        if want[j] < n:
                            s_next = score[t, order[want[j]]]
                            assert s_next < score[t, r] or (s_next == score[t, r] and order[want[j]] > r)
                        if want[j] > 0:
                            s_prev = score[t, order[want[j] - 1]]
                            assert s_prev > score[t, r] or (s_prev == score[t, r] and order[want[j] - 1] < r)
            # the selection does not depend on the refs, and the counts not on k
            alone = rank_call(fn, b, phi, flags, X, best, k=70, excl=excl)
            assert np.array_equal(alone["top_idx"], out["top_idx"]) and np.array_equal(_bits(alone["top_val"]), _bits(out["top_val"]))
            only = rank_call(fn, b, phi, flags, X, best, k=0, refs=refs, excl=excl, want_ranked=False)
            assert np.array_equal(only["ref_rank"], out["ref_rank"])


def test_zeros_are_listed_in_index_order():
    """best_f far below every mean (as test_gpu_log_ei.test_the_underflow_case_is_fixed constructs it): EI is exactly 0 on every row,
    so the selection is the lowest rows that are not excluded, in index order, and a row's rank is the eligible rows below it."""
    fn, pool_fn = _rank_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(1, False, 61, rows=70)
    low = (best - 1000.0).astype(np.float32)
    score = pool_score(pool_fn, b, phi, LATENT, X, low)
    assert (score == 0).all(), "the premise: EI is 0 on the whole pool"
    lists = [[0, 2, 5], [], [1]]
    e_idx = np.array([i for l in lists for i in l], np.int64)
    e_off = np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64)
    refs = np.tile(np.array([0, 2, 7, 69], np.int64), (b.T, 1))
    out = rank_call(fn, b, phi, LATENT, X, low, k=66, refs=refs, excl=(e_idx, e_off))
    for t in range(b.T):
        free = [r for r in range(70) if r not in lists[t]]
        assert out["top_idx"][t].tolist() == free[:66] and (out["top_val"][t] == 0).all()
        assert out["ref_rank"][t].tolist() == [sum(1 for f in free if f < r) for r in refs[t]]


def test_signed_zeros_tie_by_row_and_keep_their_sign():
    """Task 0 has zero labels but for two entries of +-2^-149, the smallest float32: a posterior mean below 2^-150 in size rounds to
    a zero with the mean's own sign, and the pool is the rows where that happens, so the mean score is zero on every row and holds both
    -0.f and +0.f.  They tie: the listing is by row index, and top_val carries each row's own sign bit."""
    fn, pool_fn = _rank_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(0, False, 63, rows=70)
    tiny = np.float32(2.0 ** -149)
    b.y_s[0] = 0.0
    b.y_s[0, 0], b.y_s[0, 1] = tiny, -tiny
    X = np.ascontiguousarray(X[pool_score(pool_fn, b, phi, SCORE_MEAN, X, best)[0] == 0])   # (a row's score depends on the row alone)
    rows = X.shape[0]
    assert rows >= 20
    for flags in (SCORE_MEAN, SCORE_MEAN | MAXIMIZE):
        score = pool_score(pool_fn, b, phi, flags, X, best)
        sign = np.signbit(score[0])
        assert (score[0] == 0).all() and sign.sum() >= 3 and (~sign).sum() >= 3, "the premise: both zeros are present"
        refs = np.tile(np.arange(rows, dtype=np.int64), (b.T, 1))
        out = rank_call(fn, b, phi, flags, X, best, k=70, refs=refs)
        assert out["top_idx"][0].tolist() == list(range(rows)) + [-1] * (70 - rows)
        assert np.array_equal(_bits(out["top_val"][0, :rows]), _bits(score[0]))
        assert out["ref_rank"][0].tolist() == list(range(rows)) and np.array_equal(_bits(out["ref_val"][0]), _bits(score[0]))
        for t in (1, 2):
            idx, val = select_ref(score[t], 70)
            assert np.array_equal(out["top_idx"][t], idx) and np.array_equal(_bits(out["top_val"][t]), _bits(val))


def test_a_skipped_task_gets_the_fills():
    fn, pool_fn = _rank_twin()
    b, Zs, ys, n_s, X, phi, best = _problem(1, False, 65, rows=30)
    b.n_s[1] = 0
    refs = np.tile(np.array([0, 5, 29], np.int64), (b.T, 1))
    out = rank_call(fn, b, phi, SCORE_MEAN, X, best, k=8, refs=refs)
    assert (out["top_idx"][1] == -1).all() and np.isneginf(out["top_val"][1]).all()
    assert (out["ref_rank"][1] == -1).all() and np.isnan(out["ref_val"][1]).all() and out["n_ranked"][1] == 0
    assert (out["top_idx"][[0, 2]] >= 0).all() and (out["n_ranked"][[0, 2]] == 30).all()


def test_enrichment_from_ranks():
    from adkf_ift_amd.evaluate import enrichment_from_ranks

    # 1000 ranked rows; f = 1 %: the cut is rank < 10; f = 5 %: rank < 50
    ranks = torch.tensor([[0, 9, 10, 49, 50, 999, -1, -1],      # 6 ranked actives: 2 of 6 under 10, 4 of 6 under 50
                          [500, 600, 700, 800, 900, 999, 10, 50],   # 8 ranked: none under 10 (10 is not), one under 50 (50 is not)
                          [-1] * 8])                                # nothing ranked: NaN
    ef = enrichment_from_ranks(ranks, torch.tensor([1000, 1000, 1000]), (0.01, 0.05))
    assert ef.dtype == torch.float64 and ef.shape == (3, 2)
    assert ef[0].tolist() == [(2 / 6) / 0.01, (4 / 6) / 0.05]
    assert ef[1].tolist() == [0.0, (1 / 8) / 0.05]
    assert bool(torch.isnan(ef[2]).all())
    # the cut is ceil(f * n): 15 rows at f = 10 % give rank < 2; one active on rank 1, one on rank 2
    ef = enrichment_from_ranks(torch.tensor([[1, 2]]), torch.tensor([15]), (0.1,))
    assert math.ceil(0.1 * 15) == 2 and ef.tolist() == [[0.5 / 0.1]]
    # a perfect ranking reaches the ceiling 1 / f; f = 1 counts every ranked active
    ef = enrichment_from_ranks(torch.tensor([[0, 1, 2, 3]]), torch.tensor([400]), (0.01, 1.0))
    assert ef.tolist() == [[100.0, 1.0]]
    with pytest.raises(ValueError):
        enrichment_from_ranks(torch.zeros(2, 3, dtype=torch.int64), torch.tensor([5]), (0.1,))
    with pytest.raises(ValueError):
        enrichment_from_ranks(torch.zeros(1, 3, dtype=torch.int64), torch.tensor([5]), (0.0,))
