"""No GPU: the feature sets of tests/dist_fused_inputs.py are what they claim - the float32 pipeline reproduces their distances exactly, the
candidate counts, and where the rank falls among the ties - so that tests/test_gpu_dist_fused.py may compare bit for bit."""
import numpy as np
import pytest
import torch

import dist_fused_inputs as F
import gp_stage_inputs as I

N = F.N
SHAPES = [(T, d) for T in (1, 3, 9) for d in (32, 64, 96)]


def _cases(d):
    return [c for c in F.CASES if d >= F.min_d(c)]


def _sorted_candidates(D2):
    return I.candidates(D2, N)


@pytest.mark.parametrize("T,d", SHAPES)
def test_float32_reproduces_every_distance(T, d):
    """Inputs, mean and centred rows are float32 values; norms and inner products (and every partial sum of them: all terms are multiples
    of one power of two and their absolute sum stays below 2^24 units) are exact; |x|^2 + |y|^2 - 2 x.y evaluated in float32 in the
    kernel's order equals float32(exact), because at most one of its two operations rounds."""
    for case in _cases(d):
        c = F.fused_batch(case, T, d)
        assert torch.equal(c["mean"].double(), c["mean64"]), "the column mean is a float32"
        xs, xq = c["Z_s"].double() - c["mean64"][:, None, :], c["Z_q"].double() - c["mean64"][:, None, :]
        for X in (xs, xq):
            assert torch.equal(X.float().double(), X), "centred entries are float32 values"
            # three bfloat16 pieces hold 24 bits: the split is exact; each entry has at most 16 significant bits here, so piece products
            # (8 x 8 bits) and their sums are far inside float32
            m = X.abs()
            frac = torch.frexp(m[m > 0])[0]
            assert torch.equal(frac * 2 ** 16, (frac * 2 ** 16).round())
        for (X, Y), name in (((xs, xs), "D2ss"), ((xq, xs), "D2qs"), ((xq, xq), "D2qq")):
            nx, ny = (X * X).sum(2), (Y * Y).sum(2)
            xy, axy = X @ Y.transpose(1, 2), X.abs() @ Y.abs().transpose(1, 2)
            unit = float(min(X[X != 0].abs().min(), Y[Y != 0].abs().min())) ** 2 if (X != 0).any() and (Y != 0).any() else 1.0
            for v in (nx, ny):
                assert torch.equal(v.float().double(), v), "row norms are exact"
            # an inner product of ONE term is that product, a float32 (checked beside); with more terms any partial sum is a multiple of
            # `unit` of at most 2^24 units in absolute value
            terms = (X != 0).double() @ (Y != 0).double().transpose(1, 2)
            assert float((axy * (terms > 1)).max()) / unit <= 2 ** 24 and torch.equal(xy.float().double(), xy)
            f32 = (nx.float()[:, :, None] + ny.float()[:, None, :]) - 2 * xy.float()
            assert torch.equal(f32, c[name]), f"{case} {name}: float32 in the kernel's order is float32(exact)"
            inexact = c[name].double() != c["exact"][("D2ss", "D2qs", "D2qq").index(name)]
            assert not (inexact & (xy != 0)).any(), "a distance that is no float32 has a zero inner product: one rounding in all"
            if case != "b":
                assert not inexact.any()
        assert (c["D2ss"] >= 0).all() and torch.equal(c["D2ss"], c["D2ss"].transpose(1, 2))
        assert not torch.diagonal(c["exact"][0], dim1=1, dim2=2).any()


@pytest.mark.parametrize("T,d", SHAPES)
def test_candidate_counts_and_ties_at_the_rank(T, d):
    for case in _cases(d):
        c = F.fused_batch(case, T, d)
        for t in range(T):
            cand = _sorted_candidates(c["D2ss"][t])
            n, r = len(cand), (len(cand) - 1) // 2
            assert n == c["n_pos"][t]
            s = (1, 3)[t % 2]
            two, four = np.float32(2 * s * s).view(np.int32), np.float32(4 * s * s).view(np.int32)
            if case == "a":
                assert n == 8128 and (cand == two).sum() == 8064 and (cand == four).sum() == 64
                assert cand[r] == two and cand[r - 1] == two and cand[r + 1] == two, "the rank is inside the run of ties"
            elif case == "d":
                assert n == 8127, "one pair coincides: an odd count"
                assert cand[r] == two and cand[r - 1] == two and cand[r + 1] == two
                assert (cand == four).sum() == 64 and (cand == two).sum() == 8127 - 64
            elif case == "b":
                assert n == 8128
                assert int(cand[-1]) >> 23 >= (int(cand[0]) >> 23) + 12, "at least twelve octaves"
                assert cand[0] ^ cand[-1] >= 1 << 26, "min and max share no exponent prefix worth a pass"
                assert len(np.unique(cand)) >= 60
            elif case == "c":
                if t % 2 == 0:
                    assert n == 127 and len(np.unique(cand)) == 1, "one positive value, in the 127 pairs of the odd row"
                    assert cand[0] == np.float32((128 * (1 + t)) ** 2).view(np.int32)
                else:
                    assert n == 0 and I.exact_l0(c["D2ss"][t], N) == 0
            assert I.check_spacing(c["D2ss"][t], N)


def test_the_two_scales_of_a_differ_in_exponent_and_mantissa():
    c = F.fused_batch("a", 3, 64)
    m0 = int(_sorted_candidates(c["D2ss"][0])[4063])
    m1 = int(_sorted_candidates(c["D2ss"][1])[4063])
    assert (m0, m1) == (0x40000000, 0x41900000)
    assert (m0 ^ m1) & 0x7F800000 and (m0 ^ m1) & 0x007FFFFF
    # within one task the two values differ in exponent bits only
    for m, t in ((m0, 0), (m1, 1)):
        hi = int(_sorted_candidates(c["D2ss"][t])[-1])
        assert (m ^ hi) & 0x007FFFFF == 0 and (m ^ hi) & 0x7F800000


def test_tasks_of_a_batch_differ():
    for case in F.CASES:
        c = F.fused_batch(case, 9, 96)
        for t in range(1, 9):
            assert not torch.equal(c["Z_s"][t], c["Z_s"][t - 1])
