"""CPU: the inputs of tests/test_gpu_dense_kernels.py (tests/dense_kernel_inputs.py) have the properties its exact comparisons rely
on, and a kernel that lost one of its six product terms could not pass them - the test of the tests, by the numpy emulation of the
split (tests/test_x3_split.py).  No GPU, no library call."""
import numpy as np
import pytest
import torch

import dense_kernel_inputs as I

SK_CUS = 8     # the k_dense3_sk cases at a small stand-in CU count: what is checked depends on K and the recipe, not on M


def _exact_f32(t64):
    return torch.equal(t64.float().double(), t64)


def _share_nonzero(a):
    return float(np.mean(a != 0))


def _piece_sums_fit(a, b, bias=0.0):
    """Every partial sum of piece products, in any order, is an integer-valued float32: sum_k sum_terms |a_i||b_j| + |bias| <= 2^24."""
    pa, pb = I.pieces(a), I.pieces(b)
    tot = sum(np.abs(pa[i]).astype(np.float64) @ np.abs(pb[j]).astype(np.float64).T for i, j in I.KEPT)
    return float(tot.max()) + bias <= I.TWO24


def _check_ints(a, b, n, bits, ref64, wide_first):
    ba, bb = bits if wide_first else bits[::-1]
    assert n * (2 ** ba - 1) * (2 ** bb - 1) + 128 <= 2 ** 24
    assert a.abs().max() <= 2 ** ba - 1 and b.abs().max() <= 2 ** bb - 1
    assert torch.equal(a, a.round()) and torch.equal(b, b.round())
    assert _piece_sums_fit(a, b, 128.0)
    assert _exact_f32(ref64)
    for t, nb in ((a, ba), (b, bb)):
        if nb > 8 and t.numel() >= 512:     # more than 8 significant bits: piece 1 is exercised
            assert _share_nonzero(I.pieces(t)[1]) >= 0.25, nb


def _check_sparse(wide, sparse_along, ref64):
    """wide: the 22-bit operand; sparse_along: the other operand with the contraction along its LAST axis"""
    assert (wide.abs() > 2 ** 21).all() and (wide.abs() < 2 ** 22).all() and (wide % 2 == 1).all()
    assert set(sparse_along.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert ((sparse_along != 0).sum(-1) <= 2).all() and (sparse_along.abs().sum(-1) <= 3).all()
    assert ref64.abs().max() + 64 < 2 ** 24 and _exact_f32(ref64)
    p = I.pieces(wide)
    assert _share_nonzero(p[1]) >= 0.25 and _share_nonzero(p[2]) >= 0.25


FWD_ALL = list(I.FWD_SHAPES) + [(M, N, K) for M, N, K, *_ in I.sk_cases(SK_CUS)]


@pytest.mark.parametrize("M,N,K", FWD_ALL)
def test_forward_recipes_hold_their_conditions(M, N, K):
    for wide in "xw":
        c = I.forward_ints(M, N, K, wide)
        _check_ints(c["x"], c["w"], K, I.FWD_BITS[K], c["y64"], wide == "x")
        assert c["b"].abs().max() <= 64 and _exact_f32(c["y64"] + c["b"].double())
        assert torch.equal(c["ref_bias"].double(), c["y64"] + c["b"].double())
        c = I.forward_sparse(M, N, K, wide)
        _check_sparse(c[wide], c["w" if wide == "x" else "x"], c["y64"])
        assert _exact_f32(c["y64"] + c["b"].double())
        if min(M, N) >= K:                  # the cyclic positions reach every k, so every chunk
            assert ((c["w" if wide == "x" else "x"] != 0).sum(0) > 0).all()
    c = I.forward_onehot(M, N, K)
    x, w = c["x"], c["w"]
    assert ((x != 0).sum(1) == 1).all() and (x[torch.arange(M), torch.arange(M) % K] != 0).all()
    mant, ex = torch.frexp(x[x != 0])
    sig = (mant.abs() * 4096)
    assert torch.equal(sig, sig.round()) and (sig % 2 == 1).all() and (ex - 12 >= -60).all() and (ex - 12 <= 40).all()
    mant, ex = torch.frexp(w)
    assert torch.equal(mant * 4096, (mant * 4096).round()) and (mant != 0).all() and (ex - 12 >= -40).all() and (ex - 12 <= 40).all()
    assert _exact_f32(c["y64"])
    assert _share_nonzero(I.pieces(x[x != 0])[1]) >= 0.25 and _share_nonzero(I.pieces(w)[1]) >= 0.25      # x1 y1 has something to multiply
    assert not np.any(I.pieces(x)[2]) and not np.any(I.pieces(w)[2])


@pytest.mark.parametrize("M,N,K", list(I.WGRAD_SHAPES))
def test_weight_gradient_recipes_hold_their_conditions(M, N, K):
    for wide in "gx":
        c = I.wgrad_ints(M, N, K, wide)
        _check_ints(c["g"].t(), c["x"].t(), M, I.wgrad_bits(M), c["dw64"], wide == "g")
        c = I.wgrad_sparse(M, N, K, wide)
        _check_sparse(c[wide], c["x" if wide == "g" else "g"].t(), c["dw64"])
    # a long contraction is cut into row ranges: the sparse operand's non-zeros are spread over all of it
    if M >= 4096:
        for wide in "gx":
            c = I.wgrad_sparse(M, N, K, wide)
            rows = (c["x" if wide == "g" else "g"] != 0).any(1).nonzero().flatten()
            assert rows.min() < M // 8 and rows.max() > M - M // 4


def _wrong_share(terms, exact, drop):
    five = sum(v for k, v in terms.items() if k != drop)
    return float(np.mean(five != exact))


def test_six_terms_are_exact_and_five_are_not():
    """The emulated kernel (six products, float64 sums) reproduces the exact answer on every output of every exact recipe; with one
    term dropped it is wrong on at least 0.8 of the outputs of the recipe that is there for that term.  Emulation, for reference:
    dense integers K = 32 (10, 9): (0,0) (0,1) (1,0) 1.00, (1,1) 0.83; one-hot: all four 1.00; sparse wide: (0,0) (1,0) 1.00, (2,0) 0.99,
    and (0,1) (0,2) with the operands swapped."""
    shares = {}
    c = I.forward_ints(256, 256, 32, "x")
    t = I.term_products(c["x"], c["w"])
    assert np.array_equal(sum(t.values()), c["y64"].numpy())
    shares["ints"] = {d: _wrong_share(t, c["y64"].numpy(), d) for d in ((0, 0), (0, 1), (1, 0), (1, 1))}
    c = I.forward_onehot(256, 256, 32)
    t = I.term_products(c["x"], c["w"])
    assert np.array_equal(sum(t.values()), c["y64"].numpy())
    shares["onehot"] = {d: _wrong_share(t, c["y64"].numpy(), d) for d in ((0, 0), (0, 1), (1, 0), (1, 1))}
    for wide, drops in (("x", ((0, 0), (1, 0), (2, 0))), ("w", ((0, 0), (0, 1), (0, 2)))):
        c = I.forward_sparse(256, 256, 32, wide)
        t = I.term_products(c["x"], c["w"])
        assert np.array_equal(sum(t.values()), c["y64"].numpy())
        shares["sparse/" + wide] = {d: _wrong_share(t, c["y64"].numpy(), d) for d in drops}
    print(shares)
    for name, row in shares.items():
        for d, s in row.items():
            assert s >= 0.8, (name, d, s)


@pytest.mark.parametrize("M,N,K", [(129, 17, 96), (130, 260, 512)])
def test_six_term_emulation_is_exact_at_other_shapes(M, N, K):
    for name, c in I.forward_cases(M, N, K):
        assert np.array_equal(sum(I.term_products(c["x"], c["w"]).values()), c["y64"].numpy()), name
    for name, c in I.wgrad_cases(K, M, 40):
        assert np.array_equal(sum(I.term_products(c["g"].t().contiguous(), c["x"].t().contiguous()).values()), c["dw64"].numpy()), name


@pytest.mark.parametrize("K", I.ROUNDING_K)
def test_rounding_bound_separates_six_terms_from_five(K):
    """Check 6 of the GPU file: its bound, 2 x the error of a float32 sequential sum, lies below half the smallest five-term error on
    the same inputs, and the six-term emulation lies below half the bound.  (On these inputs: sequential sum 2.3e-7 at K = 32 and at
    K = 256, six terms 1.4e-8 / 3.0e-9, five terms from 3.0e-6 / 1.0e-6.)"""
    c = I.normal_case(256, 256, K)
    five = I.five_term_errors(c["x"], c["w"])
    five_min = min(v for k, v in five.items() if k is not None)
    yard = I.unit_error(I.f32_sequential(c["x"], c["w"]), c["x"], c["w"])
    print(K, "yardstick", yard, "bound", 2 * yard, "six", five[None], "five-term min", five_min)
    assert 2 * yard < 0.5 * five_min
    assert five[None] < yard            # the six-term form itself sits under half the bound
    assert I.rounding_bound(c["x"], c["w"], five_min) == (2 * yard, yard)
    big = I.normal_case(300, 256, K)
    assert torch.equal(big["x"][:256], c["x"]) and torch.equal(big["w"], c["w"])


def test_same_sign_data_is_what_it_says():
    M, N, K = I.SAME_SIGN
    c = I.same_sign_case(M, N, K)
    for t in (c["a"], c["b"]):
        assert t.min() >= 1.0 and t.max() < 2.0
    assert c["a"].shape == (M, K) and c["b"].shape == (N, K)


def test_the_persistent_form_is_selected_for_every_sk_case():
    for cus in (8, 256, 304):
        ms = set()
        for M, N, K, *_ in I.sk_cases(cus):
            assert I.takes_persistent_form(M, K, cus)
            ms.add(-(-(-(-M // 128)) // cus))
        assert ms == {1, 2, 3}            # row tiles of the busiest workgroup
        assert not I.takes_persistent_form(128 * (cus - 1), 64, cus) and not I.takes_persistent_form(128 * cus, 96, cus)


def test_the_cpu_cut_is_the_numpy_cut_and_its_planes_sum_to_x():
    """What the GPU file holds adkf_split_planes to: torch's CPU conversion, bit for bit the round-to-nearest-even cut of
    tests/test_x3_split.py, on every value of the split test - ties, binade crossings, the largest float that stays finite, 2^-108."""
    n = max(r * k for r, k in I.SPLIT_SHAPES + I.SPLIT_T_SHAPES)
    x = I.split_values(n)
    assert torch.isfinite(x).all() and (x == 0).any() and (x.abs() == 2.0 ** -108).any()
    assert (x.view(torch.int32) == 0x7F7F7FFF).any() and ((x.view(torch.int32) & 0xFFFF) == 0x8000).any()
    planes = I.cpu_cut(x)
    want = np.stack(I.pieces(x)).view(np.uint32) >> 16
    assert np.array_equal(planes.numpy().view(np.uint16), want.astype(np.uint16))
    assert torch.isfinite(planes.view(torch.bfloat16).float()).all()
    assert torch.equal(I.planes_sum(planes), x.double())
    small = x[(x != 0) & (x.abs() < 2.0 ** -108)]             # below 2^-108: bfloat16 values only (2^-126: the pieces are x, 0, 0)
    assert ((small.view(torch.int32) & 0xFFFF) == 0).all()
    d = I.denormal_values(256)
    assert (d.abs() < 2.0 ** -108).all() and (d != 0).all()


def test_weight_gradient_row_ranges_of_the_two_named_shapes():
    """(4099, 33, 70): 33 ranges - the reduce's groups of eight plus a tail; (8193, 8, 8): the cap of 64 asked for, 52 ranges of 160 rows."""
    assert I.wgrad_ranges(4099, 33, 70, 256) == 33 and I.wgrad_ranges(8193, 8, 8, 256) == 52 and I.wgrad_ranges(1, 1, 1, 256) == 1
