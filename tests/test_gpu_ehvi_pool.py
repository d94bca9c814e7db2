"""GPU: constrained EHVI across tasks over a shared pool (adkf_ehvi_pool / gp_ops.ehvi_pool) - the score alone against the float64 score
at the call's own float32 mean and variance, every row compared; the exactness anchors, bit for bit against predict_pool, on every kind
of task; the staircase against gp_ops.pareto_front; chunk boundaries, the selection across chunks and the independence of groups; the
NaN rule; the batched BO loop."""
import numpy as np
import pytest
import torch

import ehvi_ref as R
import jes_ref as J
import test_gpu_believer_pool as BV
import test_gpu_believer_pool_ard as BVA
import test_gpu_kg_pool as KG
from test_ehvi_pool_cpu import GPU_CASES, GPU_CHAIN, MID_SHIFT, far_groups, gpu_problem

pytestmark = pytest.mark.gpu

EPS32 = R.EPS32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, c):
    return torch.equal(_bits(a), _bits(c))


def _call(b, phi, X, grp, **kw):
    from adkf_ift_amd import gp_ops

    t = lambda a: None if a is None else torch.from_numpy(a)
    return gp_ops.ehvi_pool(b, phi, X, obj=t(grp["obj"]), ref=t(grp["ref"]), front=t(grp["front"]), front_n=t(grp["front_n"]),
                            obj_maximize=t(grp["obj_max"]), con=t(grp["con"]), con_thr=t(grp["con_thr"]), con_geq=t(grp["con_geq"]), **kw)


_built = {}


def _built_case(dev, case):
    """A score case on the device, once, shared and left unchanged: (b, phi, X, groups, mean32, var32)."""
    from adkf_ift_amd import gp_ops

    if case not in _built:
        kernel, n_s, d, rows, P, Cn = GPU_CASES[case]
        Zs, ys, X, phi, grp = gpu_problem(case)
        T = len(n_s)
        b = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.zeros(T, 4, device=dev), kernel, n_s=torch.tensor(n_s, dtype=torch.int32))
        phi, X = phi.to(dev), X.to(dev)
        pp = gp_ops.predict_pool(b, phi, X, latent=True)
        gp_ops.check_info(pp["info"])
        _built[case] = (b, phi, X, grp, pp["mean"].cpu().numpy(), pp["var"].cpu().numpy())
    return _built[case]


# ---- the score alone
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("case", range(len(GPU_CASES)))
def test_the_score_alone(dev, case, log):
    """score against the float64 score evaluated at the call's OWN float32 mean and latent variance (predict_pool(latent=True) on the
    same batch: by the anchors the same bits), every row of every group compared:
        linear  |got - ref| <= EVAL_C     eps32 PoF (unit_obj + EHVI sum_c (1 + z_c^2)) + 1e-37
        log     |got - ref| <= EVAL_C_LOG eps32 (unit_obj / EHVI + sum_c (1 + z_c^2) + 1 + |ref|)
    Three cases have fronts of support labels, which clean down to 1 to 7 points; two have anti-chain fronts whose staircases keep
    all 64 and all 33 points (asserted from stair_n): 65 strips a row, the most there can be, and 34, not a multiple of the four waves.
    The log form runs on the groups as they are, with the reference point moved by MID_SHIFT - the float32 linear score is 0 on at
    least a quarter of the pool and positive on at least a twentieth (asserted) - and moved by 25, where it is 0 on every row and
    pm_log_ei runs in its deep tail.  A NaN score, or a NaN ratio, fails the test.  The constants are 4 x the largest ratio this test
    has printed on the MI355X, rounded up to a power of two (ehvi_ref.py)."""
    from adkf_ift_amd import gp_ops

    b, phi, X, grp, mean, var = _built_case(dev, case)
    kernel, n_s, d, rows, P, Cn = GPU_CASES[case]
    worst, compared = 0.0, 0
    variants = (("near", grp), ("mid", far_groups(grp, MID_SHIFT)), ("far", far_groups(grp))) if log else (("near", grp),)
    for name, gs in variants:
        out = _call(b, phi, X, gs, log=log, want_stair=True)
        gp_ops.check_info(out["info"])
        if GPU_CHAIN[case]:
            assert (out["stair_n"] == P).all(), out["stair_n"]   # every point of the anti-chain is a step: P + 1 strips a row
        got = out["score"].cpu().numpy().astype(np.float64)
        assert not np.isnan(got).any(), (name, int(np.isnan(got).sum()))
        if name != "near":
            lin = _call(b, phi, X, gs)["score"]
            zero, pos = int((lin == 0).sum()), int((lin > 0).sum())
            print(f"case {case} {name}: {zero} of {lin.numel()} rows with a float32 linear score of 0, {pos} with a positive one")
            assert 4 * zero >= lin.numel()
            if name == "mid":   # zeros and non-zeros side by side: where the order the log form keeps matters
                assert 20 * pos >= lin.numel()
        for g in range(gs["G"]):
            gr = R.score_ref(mean, var, gs, g)
            ref = gr["log"] if log else gr["lin"]
            unit = R.bound_log(gr) if log else R.bound_linear(gr)
            assert np.isfinite(ref).all() and not np.isnan(unit).any(), (name, g)
            excess = np.maximum(np.abs(got[g] - ref) - (0.0 if log else 1e-37), 0.0)
            # a row with nothing beyond the floor is at ratio 0 whatever its unit; one beyond it on a unit of 0 is at infinity
            ratio = np.where(excess == 0.0, 0.0, excess / np.where(unit > 0.0, unit, 1.0))
            ratio = np.where((excess > 0.0) & ~(unit > 0.0), np.inf, ratio)
            assert not np.isnan(ratio).any(), (name, g)
            print(f"{kernel} ns {max(n_s)} P {P} C {Cn} {'log' if log else 'lin'} {name} group {g}: worst |got - ref| / (eps32 unit) = "
                  f"{float(ratio.max()):.3f} (row {int(ratio.argmax())}) over {ratio.size} rows")
            worst = max(worst, float(ratio.max()))
            compared += ratio.size
    const = R.EVAL_C_LOG if log else R.EVAL_C
    print(f"case {case} {'log' if log else 'lin'}: worst ratio {worst:.3f} (constant {const})")
    assert compared == len(variants) * grp["G"] * rows   # no row was left out
    assert worst <= const, worst


# ---- the anchors
def _anchor(b, phi, X, best, tag):
    """A single-objective group per task, no constraint: score and selection (k = 4) are predict_pool's ei, bit for bit, linear and
    log, minimised and maximised."""
    from adkf_ift_amd import gp_ops

    T = b.T
    obj = torch.tensor([[t, -1] for t in range(T)], dtype=torch.int32)
    ref = torch.stack([best.cpu().float(), torch.full((T,), float("nan"))], 1)   # the second coordinate is not read
    for log in (False, True):
        for mx in (False, True):
            pp = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best.to(X.device), maximize=mx, want_mean=False, want_var=False,
                                     want_ei=True, topk=4, log_ei=log)
            out = gp_ops.ehvi_pool(b, phi, X, obj=obj, ref=ref, obj_maximize=torch.tensor([[int(mx), 0]] * T), log=log, topk=4, want_score=True)
            assert torch.equal(out["info"], pp["info"]), tag
            assert _same(out["score"], pp["ei"]), (tag, log, mx, int((_bits(out["score"]) != _bits(pp["ei"])).sum()))
            assert torch.equal(out["top_idx"], pp["top_idx"]) and _same(out["top_val"], pp["top_val"]), (tag, log, mx)


def test_anchor_mixed_kinds(dev):
    b, phi, Zs, ys, n_s, X = KG._ill(dev)
    kinds = KG._kinds(b)
    print("kinds:", kinds)
    assert 2 in kinds and min(kinds) < 2
    best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(b.T)])
    _anchor(b, phi, X, best, "mixed kinds")


def test_anchor_global_row_tile_slots(dev):
    b, phi, Zs, ys, n_s, X, best = BV._explicit(dev, "matern", [1024, 700], 12, 130, 500 + 1024)
    _anchor(b, phi, X, best, "slots")


def test_anchor_ard(dev):
    b, phi, Zs, ys, n_s, X, best = BVA._explicit(dev, "matern", [48, 45, 31], 12, 130, 500 + 48)
    _anchor(b, phi, X, best, "ard")


def _small(dev, n_s, d, rows, seed, kernel="rbf"):
    from adkf_ift_amd import gp_ops

    Zs, ys, X, phi = J.problem(n_s, d, rows, seed)
    T = len(n_s)
    b = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.zeros(T, 4, device=dev), kernel, n_s=torch.tensor(n_s, dtype=torch.int32))
    return b, phi.to(dev), X.to(dev), ys


def test_anchor_one_support_row(dev):
    b, phi, X, ys = _small(dev, [1, 16], 5, 70, 21)
    _anchor(b, phi, X, torch.tensor([0.1, -0.2]), "n_s = 1")


def test_more_groups_than_resident_workgroups(dev):
    """G = 1500 two-objective groups with constraints over T = 3 tasks, 30 rows (one tile each): the score kernel keeps 4 workgroups a
    CU, 1024 on the 256 CUs of the MI355X, so its grid is smaller than G and a workgroup serves a second group - the group's state
    and its list are loaded again.  Group g repeats group g % 3, so its score and selection are those of a call with 3 groups, bit
    for bit; the exclusion lists differ per group."""
    from adkf_ift_amd import gp_ops

    b, phi, X, ys = _small(dev, [16, 12, 9], 5, 30, 27)
    three = R.make_groups(ys.numpy(), [16, 12, 9], 9, 1, 11, chain=True)
    G = 1500
    many = {key: (np.concatenate([val] * (G // 3)) if isinstance(val, np.ndarray) else val) for key, val in three.items()}
    many["G"] = G
    lists = [[g % 30, (7 * g) % 30] for g in range(G)]
    for log in (False, True):
        small = _call(b, phi, X, three, log=log, want_score=True, want_stair=True)
        assert (small["stair_n"] == 9).all()
        out = _call(b, phi, X, many, log=log, topk=4, exclude=lists, want_score=True)
        assert _same(out["score"], small["score"].repeat(G // 3, 1)), log
        score = small["score"].cpu().numpy()
        for g in list(range(0, 40)) + list(range(1000, 1500, 7)):
            wi, wv = R.topk_of(score[g % 3], 4, lists[g])
            assert np.array_equal(out["top_idx"][g].cpu().numpy(), wi), (log, g)
            assert np.array_equal(out["top_val"][g].cpu().numpy().view(np.int32), wv.view(np.int32)), (log, g)


def test_anchor_six_hundred_groups(dev):
    """G = 600 single-objective groups over T = 3 tasks, 70 rows: group g is task g % 3 with its own reference value.  (Fewer groups
    than the score kernel has resident workgroups on the MI355X: every group has a workgroup of its own.)"""
    from adkf_ift_amd import gp_ops

    b, phi, X, ys = _small(dev, [16, 12, 9], 5, 70, 22)
    G = 600
    obj = torch.tensor([[g % 3, -1] for g in range(G)], dtype=torch.int32)
    refs = torch.linspace(-1.0, 1.0, G)
    out = gp_ops.ehvi_pool(b, phi, X, obj=obj, ref=torch.stack([refs, refs], 1), log=True, topk=4, want_score=True)
    for j in range(0, G, 3):   # three groups at a time: one predict_pool call with their three reference values
        pp = gp_ops.predict_pool(b, phi, X, latent=True, best_f=refs[j:j + 3].to(dev), want_mean=False, want_var=False, want_ei=True, topk=4,
                                 log_ei=True)
        assert _same(out["score"][j:j + 3], pp["ei"]) and torch.equal(out["top_idx"][j:j + 3], pp["top_idx"]), j
        assert _same(out["top_val"][j:j + 3], pp["top_val"]), j


def test_anchor_the_empty_front_product(dev):
    """Two objectives and an empty staircase: ei_1(r1) ei_2(r2), in log form log ei_1 + log ei_2, each predict_pool's, combined in
    float32 - bit for bit."""
    from adkf_ift_amd import gp_ops

    b, phi, X, ys = _small(dev, [16, 12, 9], 5, 70, 23, "matern")
    obj = torch.tensor([[0, 1], [1, 2], [2, 0]], dtype=torch.int32)
    mx = torch.tensor([[0, 1], [1, 0], [0, 0]], dtype=torch.int32)
    ref = torch.tensor([[0.3, -0.2], [0.1, 0.4], [-0.1, 0.2]])
    front = torch.tensor([[[0.5, 0.0], [float("nan"), 0.0]], [[0.0, 0.1], [0.2, 0.6]], [[0.0, 0.3], [-0.2, 0.2]]])   # nothing survives
    for log in (False, True):
        ei = {}
        for sense in (0, 1):
            for col in (0, 1):
                best = torch.zeros(3)
                for g in range(3):
                    best[int(obj[g, col])] = ref[g, col]
                # each task is the first objective of one group and the second of another: one call per (column, sense)
                ei[(col, sense)] = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best.to(dev), maximize=bool(sense), want_mean=False,
                                                       want_var=False, want_ei=True, log_ei=log)["ei"]
        for fr in (None, front):
            out = gp_ops.ehvi_pool(b, phi, X, obj=obj, ref=ref, obj_maximize=mx, front=fr, log=log, want_stair=fr is not None)
            if fr is not None:
                assert (out["stair_n"] == 0).all() and (out["stair"] == 0).all()
            for g in range(3):
                e1 = ei[(0, int(mx[g, 0]))][int(obj[g, 0])]
                e2 = ei[(1, int(mx[g, 1]))][int(obj[g, 1])]
                want = e1 + e2 if log else e1 * e2
                assert _same(out["score"][g], want), (log, g, fr is None)


# ---- the staircase
def test_the_staircase(dev):
    from adkf_ift_amd import gp_ops

    b, phi, X, ys = _small(dev, [16, 12, 9], 5, 70, 24)
    g = np.random.default_rng(3)
    obj = torch.tensor([[0, 1], [1, 2], [2, 0]], dtype=torch.int32)
    mx = [[0, 1], [1, 1], [0, 0]]
    ref = np.array([[0.9, -0.9], [-0.8, -1.0], [1.0, 0.8]], np.float32)
    front = np.zeros((3, 64, 2), np.float32)
    clean, perm = [], np.zeros_like(front)
    for q in range(3):
        sg = np.array([-1.0 if m else 1.0 for m in mx[q]], np.float32)
        pts = g.uniform(-1.0, 1.0, (64, 2)).astype(np.float32)
        pts[5] = pts[2]; pts[40] = pts[2]                         # duplicates
        pts[7] = np.nan; pts[8, 1] = np.nan                       # NaNs
        pts[9] = (ref[q] * sg + 0.3) * sg                         # beyond ref in both
        pts[10, 0] = ref[q, 0]                                    # on the boundary: not strictly better
        front[q] = pts
        perm[q] = pts[g.permutation(64)]
        clean.append(gp_ops.pareto_front(torch.from_numpy(pts), [bool(m) for m in mx[q]], torch.from_numpy(ref[q])))
    kw = dict(obj=obj, ref=torch.from_numpy(ref), obj_maximize=torch.tensor(mx, dtype=torch.int32))
    for log in (False, True):
        out = gp_ops.ehvi_pool(b, phi, X, front=torch.from_numpy(front), log=log, want_score=True, want_stair=True, **kw)
        P2 = max(len(c) for c in clean)
        tidy = torch.zeros(3, P2, 2)
        for q in range(3):
            n = int(out["stair_n"][q])
            assert n == len(clean[q]) and 2 <= n < 60, (q, n)
            assert _same(out["stair"][q, :n].cpu(), clean[q]) and (out["stair"][q, n:] == 0).all(), q
            tidy[q, :n] = clean[q]
        fn = torch.tensor([len(c) for c in clean], dtype=torch.int32)
        again = gp_ops.ehvi_pool(b, phi, X, front=tidy, front_n=fn, log=log, want_score=True, want_stair=True, **kw)
        shuffled = gp_ops.ehvi_pool(b, phi, X, front=torch.from_numpy(perm), log=log, want_score=True, want_stair=True, **kw)
        assert _same(again["score"], out["score"]) and _same(shuffled["score"], out["score"]), log
        assert torch.equal(again["stair_n"], out["stair_n"]) and _same(shuffled["stair"], out["stair"])
        assert torch.isfinite(out["score"]).all() and (log or (out["score"] >= 0).all())


# ---- chunks and grids
def test_chunks_and_groups(dev):
    from adkf_ift_amd import _lib, gp_ops

    CH = _lib.EHVI_CHUNK_ROWS
    rows = CH + 70
    b, phi, X, ys = _small(dev, [16, 16], 4, rows, 25)
    grp = R.make_groups(ys.numpy(), [16, 16], 7, 1, 9)
    three = {key: (np.concatenate([val, val[:1]]) if isinstance(val, np.ndarray) else val) for key, val in grp.items()}
    three["G"] = 3
    three["obj"][2] = (0, -1)                                     # groups (0, 1), (1, 0) and task 0 alone
    first = _call(b, phi, X, three, want_score=True)["score"]
    # exclusions that remove the best rows of the first chunk from every group
    lists = [torch.topk(first[g, :CH], 40).indices.cpu().tolist() for g in range(3)]
    # ... and a copy of group 0's best row beyond the boundary: equal bits there, so the selection has to reach into the second chunk
    X = X.clone()
    X[CH + 5] = X[lists[0][0]]
    for log in (False, True):
        full = _call(b, phi, X, three, log=log, topk=64, exclude=lists, want_score=True)
        lo = CH - 10
        part = _call(b, phi, X[lo:].contiguous(), three, log=log, want_score=True)
        assert _same(full["score"][:, lo:], part["score"]), log        # the same bits on either side of the chunk boundary
        score = full["score"].cpu().numpy()
        assert score[0, CH + 5].view(np.int32) == score[0, lists[0][0]].view(np.int32)
        assert CH + 5 in full["top_idx"][0].tolist() and (full["top_idx"][0] < CH).any()
        for g in range(3):
            wi, wv = R.topk_of(score[g], 64, lists[g])
            assert np.array_equal(full["top_idx"][g].cpu().numpy(), wi), (log, g)
            assert np.array_equal(full["top_val"][g].cpu().numpy().view(np.int32), wv.view(np.int32)), (log, g)
            one ={key: (val[g:g + 1] if isinstance(val, np.ndarray) else val) for key, val in three.items()}
            one["G"] = 1
            alone = _call(b, phi, X, one, log=log, want_score=True)
            assert _same(alone["score"][0], full["score"][g]), (log, g)   # a group's bits do not depend on the other groups


# ---- semantics
def test_the_nan_rule_and_empty_inputs(dev):
    from adkf_ift_amd import gp_ops

    rows = 130
    n_s = [16, 0, 9, 12]
    b, phi, X, ys = _small(dev, [16, 12, 9, 12], 5, rows, 26, "matern")
    grp = R.make_groups(ys.numpy(), [16, 12, 9, 12], 7, 1, 4)
    base = _call(b, phi, X, grp, topk=4, want_score=True)
    gp_ops.check_info(base["info"])
    assert torch.isfinite(base["score"]).all() and (base["top_idx"] >= 0).all()

    def broken(key, idx, val):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in grp.items()}
        bad[key][idx] = val
        return bad
    for i, bad in enumerate([broken("obj", (1, 0), 4), broken("obj", (1, 0), -1), broken("obj", (1, 1), 1), broken("obj", (1, 1), -2),
                             broken("ref", (1, 1), np.nan), broken("con", (1, 0), 9), broken("con_thr", (1, 0), np.nan)]):
        out = _call(b, phi, X, bad, topk=4, want_score=True)
        assert torch.isnan(out["score"][1]).all() and (out["top_idx"][1] == -1).all() and torch.isneginf(out["top_val"][1]).all(), i
        for g in (0, 2, 3):
            assert _same(out["score"][g], base["score"][g]) and torch.equal(out["top_idx"][g], base["top_idx"][g]), (i, g)
    # an empty member task (task 1): groups 0 = (0, 1; constraint 1) and 1 = (1, 2) are NaN, group 3 = (3, 0; constraint 0) keeps its bits
    b0 = gp_ops.GPBatch(b.Z_s, b.y_s, torch.zeros(4, 4, device=dev), "matern", n_s=torch.tensor(n_s, dtype=torch.int32, device=dev))
    out = _call(b0, phi, X, grp, topk=4, want_score=True)
    assert torch.isnan(out["score"][:2]).all() and (out["top_idx"][:2] == -1).all()
    assert _same(out["score"][3], base["score"][3]) and torch.equal(out["top_idx"][3], base["top_idx"][3])
    # a pool row with a non-finite feature (an infinite one: the tile walk clamps a NaN distance to 0, as in prediction): NaN in the
    # groups whose tasks see it - prediction's own mean says which - and every other score keeps its bits
    Xn = X.clone()
    Xn[70, 1] = float("inf")
    seen = torch.isnan(gp_ops.predict_pool(b, phi, Xn, latent=True)["mean"][:, 70]).cpu().tolist()
    assert any(seen)
    out = _call(b, phi, Xn, grp, topk=4, want_score=True)
    keep = torch.arange(rows, device=dev) != 70
    assert _same(out["score"][:, keep], base["score"][:, keep])
    for g in range(4):
        members = [int(grp["obj"][g, 0]), int(grp["obj"][g, 1]), int(grp["con"][g, 0])]
        if any(seen[t] for t in members):
            assert torch.isnan(out["score"][g, 70]) and not (out["top_idx"][g] == 70).any(), g
        else:
            assert torch.isfinite(out["score"][g, 70]), g
    # an empty pool
    out = _call(b, phi, X[:0], grp, topk=4, want_stair=True)
    assert (out["top_idx"] == -1).all() and torch.isneginf(out["top_val"]).all()
    assert torch.equal(out["stair_n"], _call(b, phi, X, grp, want_stair=True)["stair_n"])


def test_the_batched_bo_loop(dev):
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(5)
    n, d, R_ = 160, 6, 3
    X = torch.randn(n, d, generator=g)
    y = torch.stack([torch.sin(X[:, 0]) + 0.3 * X[:, 1], torch.cos(X[:, 2]) - 0.2 * X[:, 3] ** 2], 1) + 0.05 * torch.randn(n, 2, generator=g)
    X, y = X.to(dev), y.to(dev)
    for acq in ("log_ehvi", "ehvi"):
        rngs = [np.random.default_rng(40 + r) for r in range(R_)]
        records, hv = BO.run_gp_ehvi_bo_batched(X, y, 8, 3, 4, "matern", dev, 10, 0.01, True, rngs=rngs, maximize=(False, True), acquisition=acq)
        assert len(records) == R_ and len(hv) == R_
        for r in range(R_):
            q = records[r]
            assert len(q) == 8 + 4 * 3 and len(set(q)) == len(q) and all(0 <= i < n for i in q), (acq, r)
            assert len(hv[r]) == 5 and all(hv[r][i + 1] >= hv[r][i] for i in range(4)) and hv[r][-1] > 0, (acq, r, hv[r])
