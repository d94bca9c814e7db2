"""CPU: the inputs of tests/test_gpu_dist_median.py (tests/gp_stage_inputs.py) have the properties its exact comparisons rely on, and a
distance stage or a median select that is subtly wrong could not pass them - the test of the tests.  Run with -s to read, for every exact
recipe and every hand-made matrix, which wrong kernel it would catch.  No GPU, no library call."""
import json
import os

import numpy as np
import pytest
import torch

import gp_stage_inputs as I
from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return int(np.float32(x).view(np.int32))


def _tasks(b):
    for t in range(len(b["n_s"])):
        yield t, b["n_s"][t], (b["n_q"][t] if b["n_q"] else 0)


def test_stage_view_follows_the_carve():
    T, ns, nq, d = 3, 65, 130, 33
    ws = torch.zeros(4 * 1024 * 1024, dtype=torch.uint8)
    mean, ss, qs, qq, end = I.stage_view(ws, T, ns, nq, d)
    assert mean.shape == (T, d) and ss.shape == (T, ns, ns) and qs.shape == (T, nq, ns) and qq.shape == (T, nq, nq)
    al = I.align256
    starts = [0, al(4 * T * d), al(4 * T * d) + al(4 * T * ns * ns), al(4 * T * d) + al(4 * T * ns * ns) + al(4 * T * nq * ns)]
    assert [v.data_ptr() - ws.data_ptr() for v in (mean, ss, qs, qq)] == starts and all(s % 256 == 0 for s in starts)
    assert end == starts[3] + 4 * T * nq * nq
    *_, end0 = I.stage_view(ws, T, ns, 0, d)           # no query set: the stage ends with D2ss
    assert end0 == starts[1] + 4 * T * ns * ns
    qq.fill_(1.0)
    assert ws[:starts[3]].sum() == 0 and ws[end:].sum() == 0


@pytest.mark.parametrize("ns,nq,d", I.dist_cases())
def test_exact_recipes_hold_their_conditions(ns, nq, d):
    """The stated conditions, the padding, and: the GEMM form in numpy float32 and with the six-term emulation of the split IS the
    integer answer."""
    for recipe in "abcd":
        b = I.exact_batch(recipe, I.ragged_sizes(ns), I.ragged_sizes(nq), ns, nq, d)
        m, c0 = I.RECIPES[recipe]
        assert 4 * m * m * (1 if recipe == "c" else d) < I.TWO24 and ns * (m + abs(c0)) < I.TWO24
        for t, n, n_q in _tasks(b):
            Zs, c = b["Z_s"][t], b["c"][t]
            assert (Zs[n:] == I.JUNK).all() and (Zs[:n].double().sum(0) == n * c.double()).all()
            assert (Zs[:n].double() - c.double()).abs().max() <= (2 * m if recipe == "d" else m)
            blocks = [("ss", Zs, n, Zs, n, b["D2ss"][t])]
            if nq:
                Zq = b["Z_q"][t]
                assert (Zq[n_q:] == I.JUNK).all()
                blocks += [("qs", Zq, n_q, Zs, n, b["D2qs"][t]), ("qq", Zq, n_q, Zq, n_q, b["D2qq"][t])]
            for name, X, nx, Y, ny, ref in blocks:
                if nx == 0 or ny == 0:
                    continue
                want = ref[:nx, :ny].numpy()
                assert want.max() < I.TWO24 and want.min() >= 0
                got = I.gemm_form_f32(X, c.float(), nx, Y, ny)
                assert np.array_equal(got.astype(np.int64), want) and got.dtype == np.float32, (recipe, t, name)
                Xc, Yc = (X[:nx] - c.float()), (Y[:ny] - c.float())
                assert np.array_equal(I.gemm_form_split(Xc, Yc).astype(np.int64), want), (recipe, t, name)
                if name != "qs":
                    assert (np.diag(want) == 0).all() and np.array_equal(want, want.T)
        if recipe == "d" and ns >= 64:
            assert int((b["D2ss"][0][:b["n_s"][0], :b["n_s"][0]] == 0).sum()) >= b["n_s"][0] + 4      # two coincident pairs
            assert not b["D2ss"][1].any()                                                            # all rows equal


@pytest.mark.parametrize("d", [32, 64, 100])
def test_recipe_b_is_inexact_without_the_centring(d):
    """A stage that skipped the centring (or centred with a wrong mean) cannot return the integers of recipe (b)."""
    b = I.exact_batch("b", I.ragged_sizes(65), I.ragged_sizes(130), 65, 130, d)
    Zs, n = b["Z_s"][0], b["n_s"][0]
    assert float((Zs[:n].double() ** 2).sum(1).max()) > I.TWO24
    got = I.gemm_form_f32(Zs, b["c"][0].float(), n, center=False).astype(np.float64)
    wrong = float(np.mean(got != b["D2ss"][0][:n, :n].numpy()))
    print(f"recipe (b), d = {d}: uncentred float32 GEMM form wrong on {wrong:.2f} of D2ss")
    assert wrong >= 0.5


@pytest.mark.parametrize("ns,nq,d", [(65, 130, 1), (65, 130, 33), (128, 132, 100), (5, 3, 32)])
def test_recipe_c_catches_a_split_that_lost_a_term(ns, nq, d):
    """On recipe (c) every operand has a non-zero piece 1: an emulation without x0 y1 + x1 y0, or without x1 y1, is wrong on at least
    half of the entries of every block."""
    b = I.exact_batch("c", I.ragged_sizes(ns), I.ragged_sizes(nq), ns, nq, d)
    for t, n, n_q in _tasks(b):
        Xs, Xq = b["Z_s"][t][:n] - b["c"][t].float(), b["Z_q"][t][:n_q] - b["c"][t].float()
        assert all(np.mean(I.pieces(X)[1] != 0) * d >= 0.9 * (X.shape[0] - 1) / X.shape[0] for X in (Xs, Xq))     # one entry per row, but the zero row
        for name, X, Y, ref in (("ss", Xs, Xs, b["D2ss"][t]), ("qs", Xq, Xs, b["D2qs"][t]), ("qq", Xq, Xq, b["D2qq"][t])):
            want = ref[:X.shape[0], :Y.shape[0]].numpy()
            for drop in (((0, 1), (1, 0)), ((1, 1),)):
                share = float(np.mean(I.gemm_form_split(X, Y, drop).astype(np.int64) != want))
                print(f"recipe (c) {ns} x {nq}, d = {d}, task {t}, D2{name}: without {drop} wrong on {share:.2f} of the entries")
                assert share >= 0.5


def test_exact_l0_agrees_with_the_oracle_on_random_features():
    g = torch.Generator().manual_seed(5)
    for n, d in ((2, 3), (17, 8), (128, 64), (300, 32)):
        Z = torch.randn(n, d, generator=g, dtype=torch.float64)
        D2 = (Z[:, None] - Z[None]).pow(2).sum(-1).float()
        want = float(O.median_lengthscale_init(Z))
        assert abs(float(I.exact_l0(D2, n)) - want) <= 1e-6 * want


def _all_matrices():
    for name, (ld, tasks) in I.MEDIAN_BATCHES.items():
        for i, (n, kind) in enumerate(tasks):
            yield name, ld, i, n, kind


def test_exact_l0_is_the_plain_sorted_list_evaluation_on_every_matrix():
    for name, ld, i, n, kind in _all_matrices():
        M = I.median_matrix(kind, n, ld, i)
        assert I.check_spacing(M, n), (name, kind, n)
        rows = M.double().tolist()
        vals = sorted(rows[r][c] for r in range(n) for c in range(r + 1, n) if rows[r][c] > 0)
        want = np.float32(np.sqrt(0.5 * vals[(len(vals) - 1) // 2])) if vals else np.float32(0)      # float64 sqrt, rounded to float32
        assert _bits(I.exact_l0(M, n)) == _bits(want), (name, kind, n)
        if kind == "all_zero":
            assert _bits(I.exact_l0(M, n)) == 0
        # the surroundings differ from the candidates: junk in the lower triangle, on the diagonal and outside n x n
        assert not torch.equal(M[:n, :n], M[:n, :n].t()) or n < 2
        outside = torch.cat((M[n:].flatten(), M[:n, n:].flatten())).view(torch.int32).numpy()
        assert (torch.diagonal(M[:n, :n]) >= 128).all() and not np.isin(outside, I.candidates(M, n)).any() and (outside != 0).all()


def test_digit_kinds_differ_only_in_their_digit():
    for kind, varying in (("low7", 0x7F), ("mid8", 0xFF << 7), ("hi8", 0xFF << 15), ("exponent", 0xFF << 23)):
        c = I.candidates(I.median_matrix(kind, 257, 257, 0), 257)
        assert len(np.unique(c)) >= 20 and len(np.unique(c & ~np.int32(varying))) == 1, kind


def test_every_matrix_says_which_wrong_select_it_catches():
    """Printed for every hand-made matrix: the exact answer and what the upper median, a rank off by one, zeros counted as candidates and
    the middle row counted twice would give.  Every answer a matrix is built to expose differs in bits from the exact one; and every batch
    of the GPU test exposes every one of the five that its sizes allow."""
    for name, (ld, tasks) in I.MEDIAN_BATCHES.items():
        caught = set()
        for i, (n, kind) in enumerate(tasks):
            M = I.median_matrix(kind, n, ld, i)
            e, w = I.exact_l0(M, n), I.wrong_l0(M, n)
            differ = sorted(k for k, v in w.items() if _bits(v) != _bits(e))
            print(f"{name} task {i}: n = {n} {kind}: l0 = {e!r}; " + ", ".join(f"{k} {v!r}" for k, v in w.items()) + f"; catches {differ}")
            for k in I.catches(kind, M, n):
                assert _bits(w[k]) != _bits(e), (name, i, kind, n, k)
            caught |= set(differ)
        want = {"upper", "rank+1", "rank-1", "zeros_counted"} | ({"middle_twice"} if any(n % 2 and n >= 5 for n, _ in tasks) else set())
        assert caught >= want, (name, want - caught)


def test_the_split_emulation_meets_the_random_data_bound_and_the_five_term_variants_are_reported():
    """The GPU test holds the stage on random features to twice the error of a float32 sequential evaluation.  The six-term emulation
    meets that at d = 32 and d = 96; whether a stage without x0 y2 + x2 y0 would exceed it is measured and printed here."""
    for d in I.RANDOM_D:
        yard, emu = I.dist_yardstick(d), I.split_emulation_errors(d)
        for blk in ("ss", "qs", "qq"):
            print(f"d = {d} D2{blk}: yardstick {yard[blk]:.3e} bound {2 * yard[blk]:.3e} six terms {emu[()][blk]:.3e} " +
                  " ".join(f"without {k}: {v[blk]:.3e} ({'exceeds' if v[blk] > 2 * yard[blk] else 'WITHIN'} the bound)" for k, v in emu.items() if k))
            assert emu[()][blk] <= 2 * yard[blk]


def test_the_recorded_yardsticks_are_the_ones_the_recipe_gives():
    prof = json.load(open(os.path.join(ROOT, "profiles", "dist_kernel_yardsticks.json")))
    for row in prof["random"]:
        yard = I.dist_yardstick(row["d"])
        for blk in ("ss", "qs", "qq"):
            assert row["f32_sequential"][blk] == pytest.approx(yard[blk], rel=0.05), (row["d"], blk)      # (the CPU's float32 ops may differ in the last place between torch builds)
