"""GPU: hyperparameter-marginalised prediction and acquisition over a shared pool (adkf_mix_pool / gp_ops.mix_pool) - the outputs alone
against the float64 mixture of the call's own float32 members, every row compared; the exactness anchors, bit for bit against
predict_pool, on every kind of task; chunk boundaries, the selection across chunks and the independence of groups; the NaN rule;
determinism; the marginalised BO loop."""
import numpy as np
import pytest
import torch

import jes_ref as J
import mix_ref as R
import test_gpu_believer_pool_ard as BVA
import test_gpu_kg_pool as KG

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


_built = {}


def _built_case(dev, case):
    """A case of mix_ref.problem on the device, once, shared and left unchanged: (problem, batch, phi, X, best_f)."""
    from adkf_ift_amd import gp_ops

    if case not in _built:
        p = R.problem(case)
        T = p["G"] * p["M"]
        b = gp_ops.GPBatch(p["Zs"].to(dev), p["ys"].to(dev), torch.zeros(T, 4, device=dev), p["kernel"], n_s=torch.from_numpy(p["n_s"]), ard=p["ard"])
        _built[case] = (p, b, p["phi"].to(dev), p["X"].to(dev), torch.from_numpy(p["best_f"]).to(dev))
    return _built[case]


def _members(b, phi, X, best, latent, log):
    """predict_pool's float32 mean, var and ei (log: log EI) [T, rows] on the same batch: by the anchors the call's own members."""
    from adkf_ift_amd import gp_ops

    pp = gp_ops.predict_pool(b, phi, X, latent=latent, best_f=best, want_ei=True, log_ei=log)
    gp_ops.check_info(pp["info"])
    return [pp[n].cpu().numpy() for n in ("mean", "var", "ei")]


def _ratios(got, ref, unit, floor=0.0):
    """|got - ref| / (eps32 unit) per row; nothing beyond the floor is ratio 0 whatever the unit, something beyond it on a unit of 0 is
    at infinity.  A NaN anywhere fails."""
    assert not np.isnan(got).any() and np.isfinite(ref).all() and not np.isnan(unit).any()
    excess = np.maximum(np.abs(got.astype(np.float64) - ref) - floor, 0.0)
    ratio = np.where(excess == 0.0, 0.0, excess / (EPS32 * np.where(unit > 0.0, unit, 1.0)))
    ratio = np.where((excess > 0.0) & ~(unit > 0.0), np.inf, ratio)
    assert not np.isnan(ratio).any()
    return ratio


# ---- the outputs alone
@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_the_outputs_alone(dev, case):
    """mean, var (latent and with the noise) and the four scores against mix_ref evaluated in float64 at the call's OWN float32
    members (predict_pool on the same batch: by the anchors the same bits), every row of every group compared:
        |got - ref| <= EVAL_C_x eps32 unit_x   (+ 1e-37 for the linear score)
    with unit_mean = sum wt |m_i|, unit_var = var + 2 (sum wt |m_i - mean|) unit_mean, unit_ei = ref, unit_log = 1 + |ref| and
    unit_bald = 1 + |log var| + sum wt |log v_i| + unit_var / var.  The log score runs on best_f as it is, moved by 4 (M <= 5: the
    float32 linear score is 0 on at least a quarter of the rows and positive on at least a twentieth, asserted) and moved by 25 (0 on
    every row).  A NaN fails the test.  The constants are 4 x the largest ratio this test has printed on the MI355X, rounded up to
    a power of two (mix_ref.py)."""
    from adkf_ift_amd import gp_ops

    p, b, phi, X, best = _built_case(dev, case)
    G, M, rows = p["G"], p["M"], p["rows"]
    kw = dict(members=torch.from_numpy(p["members"]), weights=None if p["weights"] is None else torch.from_numpy(p["weights"]))
    worst = dict(mean=0.0, var=0.0, ei=0.0, log_ei=0.0, smean=0.0, bald=0.0)
    compared = 0

    def check(out, mvE, pairs, maximize=False, log=False, tag=""):
        nonlocal compared
        for g in range(G):
            ts, wt = R.weights_of(p["members"][g], None if p["weights"] is None else p["weights"][g])
            ref = R.mix(mvE[0][ts], mvE[1][ts], mvE[2][ts], wt, maximize=maximize, log=log)
            for name, key, unit in pairs:
                ratio = _ratios(out[name][g].cpu().numpy(), ref[key], ref[unit], 1e-37 if key == "ei" else 0.0)
                worst[key] = max(worst[key], float(ratio.max()))
                compared += ratio.size
        print(f"case {case} {tag}: " + ", ".join(f"{key} {worst[key]:.3f}" for _, key, _ in pairs) + "  (worst |got - ref| / (eps32 unit) so far)")

    for latent in (True, False):
        mvE = _members(b, phi, X, best, latent, False)
        out = gp_ops.mix_pool(b, phi, X, best_f=best, score="ei", latent=latent, want_score=True, **kw)
        gp_ops.check_info(out["info"])
        check(out, mvE, (("mean", "mean", "unit_mean"), ("var", "var", "unit_var"), ("score", "ei", "unit_ei")), tag=f"latent={latent} ei")
        out = gp_ops.mix_pool(b, phi, X, score="bald", latent=latent, want_mean=False, want_var=False, want_score=True, **kw)
        check(out, mvE, (("score", "bald", "unit_bald"),), tag=f"latent={latent} bald")
    for mx in (False, True):
        out = gp_ops.mix_pool(b, phi, X, score="mean", maximize=mx, want_mean=False, want_var=False, want_score=True, **kw)
        check(out, mvE, (("score", "smean", "unit_mean"),), maximize=mx, tag=f"maximize={mx} mean")
    shifts = (("near", 0.0), ("mid", R.MID_SHIFT), ("far", R.FAR_SHIFT)) if M <= 5 else (("near", 0.0), ("far", R.FAR_SHIFT))
    for name, shift in shifts:
        moved = best - shift
        if name != "near":
            lin = gp_ops.mix_pool(b, phi, X, best_f=moved, score="ei", latent=True, want_mean=False, want_var=False, want_score=True, **kw)["score"]
            zero, pos = int((lin == 0).sum()), int((lin > 0).sum())
            print(f"case {case} {name}: {zero} of {lin.numel()} rows with a float32 linear score of 0, {pos} with a positive one")
            if name == "mid":
                assert 4 * zero >= lin.numel() and 20 * pos >= lin.numel()
            else:
                assert zero == lin.numel()
        mvE = _members(b, phi, X, moved, True, True)
        assert np.isfinite(mvE[2]).all()
        out = gp_ops.mix_pool(b, phi, X, best_f=moved, score="log_ei", latent=True, want_mean=False, want_var=False, want_score=True, **kw)
        check(out, mvE, (("score", "log_ei", "unit_log"),), log=True, tag=f"log_ei {name}")
    print(f"case {case}: worst ratios {worst}")
    assert compared == (2 * 4 + 2 + len(shifts)) * G * rows   # no row was left out
    assert worst["mean"] <= R.EVAL_C_MEAN and worst["smean"] <= R.EVAL_C_MEAN and worst["var"] <= R.EVAL_C_VAR, worst
    assert worst["ei"] <= R.EVAL_C_EI and worst["log_ei"] <= R.EVAL_C_LOG and worst["bald"] <= R.EVAL_C_BALD, worst


# ---- the anchors
def _anchor(b, phi, X, best, tag):
    """One group per task with that task alone, and one with two equal entries of it: mean, var (latent and noisy), ei and log EI,
    minimised and maximised, and the selection with k = 4 are predict_pool's, bit for bit; BALD is exactly 0."""
    from adkf_ift_amd import gp_ops

    T = b.T
    best = best.to(X.device).float()
    t = torch.arange(T, dtype=torch.int32)
    tables = ((torch.stack([t, torch.full_like(t, -1)], 1), None), (torch.stack([t, t, t], 1), torch.tensor([[0.7, 0.7, 0.0]]).repeat(T, 1)))
    for members, weights in tables:
        for latent in (True, False):
            for log in (False, True):
                for mx in (False, True):
                    pp = gp_ops.predict_pool(b, phi, X, latent=latent, best_f=best, maximize=mx, want_ei=True, topk=4, log_ei=log)
                    out = gp_ops.mix_pool(b, phi, X, members=members, weights=weights, best_f=best, score="log_ei" if log else "ei", latent=latent,
                                          maximize=mx, want_score=True, topk=4)
                    key = (tag, members.shape[1], latent, log, mx)
                    assert torch.equal(out["info"], pp["info"]), key
                    assert _same(out["mean"], pp["mean"]) and _same(out["var"], pp["var"]), key
                    diff = _bits(out["score"]) != _bits(pp["ei"])
                    assert not diff.any(), (key, int(diff.sum()), out["score"][diff][:4].tolist(), pp["ei"][diff][:4].tolist())
                    assert torch.equal(out["top_idx"], pp["top_idx"]) and _same(out["top_val"], pp["top_val"]), key
            bald = gp_ops.mix_pool(b, phi, X, members=members, weights=weights, score="bald", latent=latent, want_mean=False, want_var=False)
            assert (bald["score"] == 0).all(), (tag, members.shape[1], latent)
        by_mean = gp_ops.mix_pool(b, phi, X, members=members, weights=weights, score="mean", want_mean=False, want_var=False, topk=4, want_score=True)
        pp = gp_ops.predict_pool(b, phi, X, score="mean", want_var=False, topk=4)
        assert _same(by_mean["score"], -pp["mean"]) and torch.equal(by_mean["top_idx"], pp["top_idx"]), tag


def test_anchor_mixed_kinds(dev):
    b, phi, Zs, ys, n_s, X = KG._ill(dev)
    kinds = KG._kinds(b)
    print("kinds:", kinds)
    assert 2 in kinds and min(kinds) < 2
    _anchor(b, phi, X, torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(b.T)]), "mixed kinds")


def test_anchor_ard(dev):
    b, phi, Zs, ys, n_s, X, best = BVA._explicit(dev, "matern", [48, 45, 31], 12, 130, 500 + 48)
    _anchor(b, phi, X, best, "ard")


def _small(dev, n_s, d, rows, seed, kernel="rbf"):
    from adkf_ift_amd import gp_ops

    Zs, ys, X, phi = J.problem(n_s, d, rows, seed)
    T = len(n_s)
    b = gp_ops.GPBatch(Zs.to(dev), ys.to(dev), torch.zeros(T, 4, device=dev), kernel, n_s=torch.tensor(n_s, dtype=torch.int32))
    return b, phi.to(dev), X.to(dev), ys


def test_anchor_one_support_row_and_a_blocked_task(dev):
    b, phi, X, ys = _small(dev, [1, 16, 200], 5, 70, 21)
    _anchor(b, phi, X, torch.tensor([0.1, -0.2, 0.0]), "n_s = 1, 16, 200")


# ---- chunks and groups
def _six_tasks(dev, rows, seed):
    """Six tiny tasks (n_s = 16, d = 8): two data sets under three phi each."""
    from adkf_ift_amd import gp_ops

    Zs, ys, X, phi = J.problem([16, 16], 8, rows, seed)
    rep = lambda t: t.repeat_interleave(3, 0)
    phi = rep(phi) + 0.3 * torch.randn(6, 3, generator=torch.Generator().manual_seed(seed))
    b = gp_ops.GPBatch(rep(Zs).to(dev), rep(ys).to(dev), torch.zeros(6, 4, device=dev), "matern")
    best = torch.tensor([float(ys[0].min())] * 3 + [float(ys[1].min())] * 3, device=dev)
    return b, phi.to(dev), X.to(dev), best


def test_chunks_and_the_selection_across_them(dev):
    from adkf_ift_amd import _lib, gp_ops

    CH = _lib.MIX_CHUNK_ROWS
    rows = CH + 70
    b, phi, X, best = _six_tasks(dev, rows, 31)
    members = torch.tensor([[0, 1, 2], [3, 4, 5], [0, 4, -1]], dtype=torch.int32)
    weights = torch.tensor([[1.0, 2.0, 0.5], [1.0, 1.0, 1.0], [0.3, 1.0, 7.0]])
    kw = dict(members=members, weights=weights, best_f=best, latent=True)
    first = gp_ops.mix_pool(b, phi, X, score="ei", want_score=True, **kw)["score"]
    # exclusions that remove the best rows of the first chunk from every group, and a copy of group 0's best row beyond the boundary:
    # equal bits there, so the selection has to reach into the second chunk, and takes the copy after its original
    lists = [torch.topk(first[g, :CH], 40).indices.cpu().tolist() for g in range(3)]
    lists[0] = lists[0][1:]
    src = int(torch.argmax(first[0, :CH]))
    X = X.clone()
    X[CH + 5] = X[src]
    lo = CH - 10
    for score in ("ei", "log_ei", "bald"):
        full = gp_ops.mix_pool(b, phi, X, score=score, topk=64, exclude=lists, want_score=True, **kw)
        part = gp_ops.mix_pool(b, phi, X[lo:].contiguous(), score=score, want_score=True, **kw)
        for n in ("mean", "var", "score"):
            assert _same(full[n][:, lo:], part[n]), (score, n)       # the same bits on either side of the chunk boundary
        sc = full["score"].cpu().numpy()
        assert sc[0, CH + 5].view(np.int32) == sc[0, src].view(np.int32)
        got = full["top_idx"][0].tolist()
        if score == "ei":
            assert got[0] == src, got[:4]
        if score != "bald":
            assert src in got
        if src in got:                                               # the copy comes right after its original
            assert got[got.index(src) + 1] == CH + 5, (score, got[:4])
        for g in range(3):
            wi, wv = R.topk_of(sc[g], 64, lists[g])
            assert np.array_equal(full["top_idx"][g].cpu().numpy(), wi), (score, g)
            assert np.array_equal(full["top_val"][g].cpu().numpy().view(np.int32), wv.view(np.int32)), (score, g)


@pytest.mark.parametrize("G", [600, 2400])
def test_many_groups(dev, G):
    """G groups over 6 tasks, 70 rows (two tiles each).  The score kernel keeps 7 workgroups a CU, 1792 on the 256 CUs of the MI355X:
    with 600 groups every (group, walker) has a workgroup of its own, with 2400 the grid is smaller than G and a workgroup serves a
    second group - the group's state and its list are loaded again.  Group g repeats one of twelve tables, and equals that table
    evaluated in a call of its own, bit for bit; the exclusion lists differ per group."""
    from adkf_ift_amd import gp_ops

    b, phi, X, best = _six_tasks(dev, 70, 32)
    g = np.random.default_rng(6)
    base_m = torch.from_numpy(g.integers(-1, 6, (12, 4)).astype(np.int32))
    base_m[:, 0] = torch.arange(12, dtype=torch.int32) % 6                 # at least one member each
    base_w = torch.from_numpy(g.uniform(0.1, 2.0, (12, 4)).astype(np.float32))
    lists = [[q % 70, (7 * q) % 70] for q in range(G)]
    for score in ("ei", "log_ei", "bald"):
        kw = dict(best_f=best, score=score, latent=True, want_score=True)
        many = gp_ops.mix_pool(b, phi, X, members=base_m.repeat(G // 12, 1), weights=base_w.repeat(G // 12, 1), topk=4, exclude=lists, **kw)
        for q in range(12):
            alone = gp_ops.mix_pool(b, phi, X, members=base_m[q:q + 1], weights=base_w[q:q + 1], **kw)
            for n in ("mean", "var", "score"):
                assert _same(many[n][q::12], alone[n].repeat(G // 12, 1)), (score, q, n)
        sc = many["score"].cpu().numpy()
        for q in list(range(0, 40)) + list(range(G - 200, G, 7)):
            wi, wv = R.topk_of(sc[q], 4, lists[q])
            assert np.array_equal(many["top_idx"][q].cpu().numpy(), wi), (score, q)
            assert np.array_equal(many["top_val"][q].cpu().numpy().view(np.int32), wv.view(np.int32)), (score, q)


# ---- semantics
def test_the_nan_rule_and_empty_inputs(dev):
    from adkf_ift_amd import gp_ops

    rows = 130
    b, phi, X, best = _six_tasks(dev, rows, 33)
    members = torch.tensor([[0, 1, 2], [3, 4, 5], [0, 4, -1]], dtype=torch.int32)
    weights = torch.tensor([[1.0, 2.0, 0.5], [1.0, 1.0, 1.0], [0.3, 1.0, float("nan")]])   # (the NaN belongs to an entry that is not there)
    kw = dict(best_f=best, latent=True, topk=4, want_score=True)
    base = gp_ops.mix_pool(b, phi, X, members=members, weights=weights, **kw)
    gp_ops.check_info(base["info"])
    assert all(torch.isfinite(base[n]).all() for n in ("mean", "var", "score")) and (base["top_idx"] >= 0).all()

    def broken(mem=None, w=None):
        m2, w2 = members.clone(), weights.clone()
        if mem is not None:
            m2[mem[0]] = mem[1]
        if w is not None:
            w2[w[0]] = w[1]
        return m2, w2
    cases = [broken(mem=((1, 0), 6)), broken(mem=((1, 2), -2)), broken(w=((1, 1), -1.0)), broken(w=((1, 0), float("nan"))),
             broken(w=((1, 2), float("inf"))), broken(mem=((1, slice(None)), -1)), broken(w=((1, slice(None)), 0.0))]
    for i, (m2, w2) in enumerate(cases):
        out = gp_ops.mix_pool(b, phi, X, members=m2, weights=w2, **kw)
        assert all(torch.isnan(out[n][1]).all() for n in ("mean", "var", "score")), i
        assert (out["top_idx"][1] == -1).all() and torch.isneginf(out["top_val"][1]).all(), i
        for g in (0, 2):
            assert all(_same(out[n][g], base[n][g]) for n in ("mean", "var", "score")) and torch.equal(out["top_idx"][g], base["top_idx"][g]), (i, g)
    # an empty member task (task 4): groups 1 and 2 use it and are NaN, group 0 keeps its bits; with a zero weight it is not used
    n_s = torch.tensor([16, 16, 16, 16, 0, 16], dtype=torch.int32, device=dev)
    b0 = gp_ops.GPBatch(b.Z_s, b.y_s, torch.zeros(6, 4, device=dev), "matern", n_s=n_s)
    out = gp_ops.mix_pool(b0, phi, X, members=members, weights=weights, **kw)
    assert torch.isnan(out["score"][1:]).all() and (out["top_idx"][1:] == -1).all()
    assert _same(out["score"][0], base["score"][0]) and torch.equal(out["top_idx"][0], base["top_idx"][0])
    m2, w2 = broken(w=((slice(None), 1), 0.0))
    out = gp_ops.mix_pool(b0, phi, X, members=m2, weights=w2, **kw)
    assert torch.isfinite(out["score"]).all()
    assert _same(out["score"][2], gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, want_ei=True)["ei"][0])   # task 0 alone is left
    # a pool row with a non-finite feature (an infinite one: the tile walk clamps a NaN distance to 0, as in prediction): NaN in the
    # groups whose members see it - prediction's own mean says which - never selected there, and every other row keeps its bits
    Xn = X.clone()
    Xn[70, 1] = float("inf")
    seen = torch.isnan(gp_ops.predict_pool(b, phi, Xn, latent=True)["mean"][:, 70]).cpu().tolist()
    assert any(seen)
    keep = torch.arange(rows, device=dev) != 70
    for score in ("ei", "log_ei", "mean", "bald"):
        ref = gp_ops.mix_pool(b, phi, X, members=members, weights=weights, score=score, **kw)
        out = gp_ops.mix_pool(b, phi, Xn, members=members, weights=weights, score=score, **kw)
        for n in ("mean", "var", "score"):
            assert _same(out[n][:, keep], ref[n][:, keep]), (score, n)
        for q in range(3):
            if any(seen[t] for t in members[q].tolist() if t >= 0):
                assert torch.isnan(out["mean"][q, 70]) and torch.isnan(out["score"][q, 70]) and not (out["top_idx"][q] == 70).any(), (score, q)
            else:
                assert torch.isfinite(out["score"][q, 70]), (score, q)
    # an empty pool
    out = gp_ops.mix_pool(b, phi, X[:0], members=members, weights=weights, **kw)
    assert (out["top_idx"] == -1).all() and torch.isneginf(out["top_val"]).all() and out["score"].shape == (3, 0)


def test_determinism(dev):
    from adkf_ift_amd import gp_ops

    p, b, phi, X, best = _built_case(dev, 0)
    kw = dict(members=torch.from_numpy(p["members"]), best_f=best, latent=True, topk=16)
    for score in ("ei", "log_ei", "bald"):
        a = gp_ops.mix_pool(b, phi, X, score=score, want_score=True, **kw)
        c = gp_ops.mix_pool(b, phi, X, score=score, want_score=True, **kw)
        quiet = gp_ops.mix_pool(b, phi, X, score=score, want_mean=False, want_var=False, want_score=False, **kw)
        assert all(_same(a[n], c[n]) for n in ("mean", "var", "score", "top_val")) and torch.equal(a["top_idx"], c["top_idx"]), score
        assert quiet["score"] is None and torch.equal(quiet["top_idx"], a["top_idx"]) and _same(quiet["top_val"], a["top_val"]), score


# ---- the loop
def test_the_marginalised_bo_loop(dev):
    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(7)
    n, d, reps = 300, 8, 2
    X = torch.randn(n, d, generator=g)
    y = ((X - 0.3) ** 2).sum(1) + 0.05 * torch.randn(n, generator=g)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=2, num_bo_iters=3, kernel_type="matern", device=dev, init_from=150, noise_init=0.01,
              noise_prior=True)
    for acq in ("ei", "log_ei"):
        runs = [BO.run_gp_ei_bo_batched(X, y, rngs=[np.random.default_rng(50 + r) for r in range(reps)], acquisition=acq, marginalize=4, **kw)
                for _ in range(2)]
        assert runs[0] == runs[1], acq                             # the same seeds, the same records
        for rec in runs[0]:
            assert len(rec) == 1 + 3 * 2 and len(set(rec[1:])) == 6 and all(0 <= i < n for i in rec), (acq, rec)
        # marginalize = 0 is the loop as it was: the sequential loop's records, as before
        plain = BO.run_gp_ei_bo_batched(X, y, rngs=[np.random.default_rng(50 + r) for r in range(reps)], acquisition=acq, marginalize=0, **kw)
        for r in range(reps):
            assert plain[r] == BO.run_gp_ei_bo(X, y, rng=np.random.default_rng(50 + r), streaming=True, acquisition=acq, **kw), (acq, r)
