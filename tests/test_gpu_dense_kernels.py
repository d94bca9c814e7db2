"""GPU: the dense-layer kernels of csrc/dense_x3.h ALONE - k_split3, k_split3_t, k_dense3, k_dense3_sk<2|4|8>, k_dense3_tn and
k_dense3_reduce - through their C entries, on the inputs of tests/dense_kernel_inputs.py.  tests/test_gpu_dense.py holds them to
5e-7 of sum |x||w| on random data with K >= 512, where a kernel that lost one of its six product terms still passes; here the
answer is exactly representable and the comparison is ``torch.equal``.

  1. the split, bit for bit against the CPU cut (round to nearest even), and the float64 sum of the planes against x;
  2. k_dense3 at one, two, three and more chunks, M < 128, N < 64, N not a multiple of 16: exact;
  3. k_dense3_sk at one, two and three row tiles for the busiest workgroup and one, two and three column tiles: exact;
  4. k_dense3_tn + k_dense3_reduce from one row to the cap of the row ranges: exact, and the same bits twice;
  5. a non-finite value (or a finite one beyond bfloat16's range) stays in its row of x / column of w;
  6. on random data the error is below 2 x that of a float32 sequential sum, which lies below half of what five terms would give;
  7. same-sign data: no bias of the mean error (the leading term has an accumulator of its own).
Every output is pre-filled with NaN; every output, plane buffer and scratch has 4 KB of a fixed pattern before and behind it, the
padding columns of a strided y carry the same pattern, and all of it must be unchanged afterwards; the padding columns of a strided
INPUT hold NaN (they must not be read); the weight gradient's scratch is exactly what adkf_dense_weight_grad_scratch_bytes says.
tests/test_dense_kernel_inputs.py checks the inputs and that five-term kernels could not pass; no bound comes from a kernel's output."""
import pytest
import torch

import dense_kernel_inputs as I

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0x5A
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from adkf_ift_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _ok(rc, what):
    from adkf_ift_amd import _lib
    _lib.check(rc, what)


def _st(dev):
    from adkf_ift_amd import _lib
    return _lib.stream(dev)


def _p(t):
    from adkf_ift_amd import _lib
    return _lib.ptr(t)


class Guarded:
    """``nbytes`` of device memory, ``offset`` bytes past a 16-byte boundary, with GUARD bytes of FILL before and behind it."""

    def __init__(self, dev, nbytes, offset=0):
        assert nbytes % 4 == 0 and offset % 4 == 0
        self.raw = torch.full((GUARD + offset + nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.lo, self.hi = GUARD + offset, GUARD + offset + nbytes
        self.body = self.raw[self.lo:self.hi]
        assert self.body.data_ptr() % 16 == offset % 16

    def view(self, dtype, *shape):
        return self.body.view(dtype).view(*shape)

    def check(self, what):
        assert bool((self.raw[:self.lo] == FILL).all()), what + ": written BEFORE the buffer"
        assert bool((self.raw[self.hi:] == FILL).all()), what + ": written BEHIND the buffer"


def _strided(dev, t, pad):
    """[R, C] -> a device tensor of row stride C + pad whose padding columns hold NaN: an input's padding must not be read"""
    if pad == 0:
        return t.to(dev).contiguous()
    full = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=torch.float32, device=dev)
    full[:, :t.shape[1]] = t.to(dev)
    return full


def _split(lib, dev, w, transposed=False):
    """adkf_split_planes (w [rows, K]) or adkf_split_planes_t (w [K, N]) into a guarded buffer pre-filled with bfloat16 NaNs"""
    w = w.to(dev).contiguous()
    rows, K = (w.shape[1], w.shape[0]) if transposed else w.shape
    buf = Guarded(dev, 2 * 3 * rows * K)
    planes = buf.view(torch.int16, 3, rows, K)
    planes.fill_(0x7FC1)
    if transposed:
        _ok(lib.adkf_split_planes_t(_p(w), _p(planes), K, rows, _st(dev)), "adkf_split_planes_t")
    else:
        _ok(lib.adkf_split_planes(_p(w), _p(planes), rows, K, _st(dev)), "adkf_split_planes")
    torch.cuda.synchronize(dev)
    buf.check("planes")
    return planes


def _forward(lib, dev, x, planes, b, ldx_pad=0, ldy_pad=0, y_off=0):
    """adkf_dense_forward into a NaN-filled, guarded y of row stride N + ldy_pad; returns y[M, N], a view of it"""
    (M, K), N = x.shape, planes.shape[1]
    xs = _strided(dev, x, ldx_pad)
    bd = None if b is None else b.to(dev)
    ldy = N + ldy_pad
    buf = Guarded(dev, 4 * M * ldy, y_off)
    full = buf.view(torch.float32, M, ldy)
    full[:, :N] = NAN
    _ok(lib.adkf_dense_forward(_p(xs), xs.stride(0), _p(planes), _p(bd), _p(full), ldy, M, N, K, _st(dev)), "adkf_dense_forward")
    torch.cuda.synchronize(dev)
    buf.check("y")
    if ldy_pad:
        assert bool((full[:, N:].contiguous().view(torch.uint8) == FILL).all()), "y: a padding column was written"
    return full[:, :N]


def _weight_grad(lib, dev, g, x, ldg_pad=0, ldx_pad=0, cus=None):
    (M, N), K = g.shape, x.shape[1]
    gs, xs = _strided(dev, g, ldg_pad), _strided(dev, x, ldx_pad)
    need = lib.adkf_dense_weight_grad_scratch_bytes(M, N, K)
    if cus is not None:
        assert need == 4 * N * K * I.wgrad_ranges(M, N, K, cus), (need, I.wgrad_ranges(M, N, K, cus))
    sbuf, dbuf = Guarded(dev, need), Guarded(dev, 4 * N * K)
    sbuf.view(torch.float32, -1).fill_(NAN)
    dw = dbuf.view(torch.float32, N, K)
    dw.fill_(NAN)
    _ok(lib.adkf_dense_weight_grad(_p(gs), gs.stride(0), _p(xs), xs.stride(0), _p(dw), M, N, K, _p(sbuf.body), need, _st(dev)),
        "adkf_dense_weight_grad")
    torch.cuda.synchronize(dev)
    sbuf.check("scratch")
    dbuf.check("dw")
    return dw


def _assert_exact(got, ref, what):
    """``got`` (device) against the exact float32 answer: no NaN left, every element equal"""
    ref = ref.to(got.device)
    assert not torch.isnan(got).any(), what + ": an element was never written (or is NaN)"
    if not torch.equal(got, ref):
        bad = (got != ref)
        worst = (got.double() - ref.double()).abs().max().item()
        first = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ, worst by %g, first at %s" % (what, int(bad.sum()), bad.numel(), worst, first))


# ======================================================================================================================
# 1. the split
# ======================================================================================================================
def _assert_planes(planes, x, what):
    want = I.cpu_cut(x)
    got = planes.cpu()
    assert torch.equal(got, want), "%s: %d bit patterns differ from the CPU cut" % (what, int((got != want).sum()))
    assert torch.equal(I.planes_sum(got), x.double()), what + ": the planes do not sum to x"


@pytest.mark.parametrize("rows,K", I.SPLIT_SHAPES)
def test_split_planes_is_the_round_to_nearest_cut_bit_for_bit(dev, lib, rows, K):
    x = I.split_values(rows * K).view(rows, K)
    _assert_planes(_split(lib, dev, x), x, "adkf_split_planes %s" % ((rows, K),))


@pytest.mark.parametrize("K,N", I.SPLIT_T_SHAPES)
def test_split_planes_t_is_the_cut_of_the_transpose(dev, lib, K, N):
    w = I.split_values(K * N).view(K, N)
    _assert_planes(_split(lib, dev, w, transposed=True), w.t().contiguous(), "adkf_split_planes_t %s" % ((K, N),))


def test_split_below_two_to_the_minus_108_is_reported(dev, lib):
    """Below 2^-108 a piece is a bfloat16 denormal; what the converter does there is printed, not asserted.  (MI355X: all 256 values
    equal the CPU cut in all three planes - the converter keeps bfloat16 denormals - and the planes sum to x for 14 of them.)"""
    x = I.denormal_values(256).view(8, 32)
    got, want = _split(lib, dev, x).cpu(), I.cpu_cut(x)
    same = (got == want).all(0)
    sums = I.planes_sum(got) == x.double()
    print("split of |x| < 2^-108: %d of %d values equal the CPU cut in all three planes; the planes sum to x for %d; planes that differ: %s"
          % (int(same.sum()), same.numel(), int(sums.sum()), [int((got[q] != want[q]).sum()) for q in range(3)]))


# ======================================================================================================================
# 2. k_dense3
# ======================================================================================================================
@pytest.mark.parametrize("M,N,K", list(I.FWD_SHAPES))
def test_dense3_is_exact_on_representable_answers(dev, lib, cus, M, N, K):
    assert not I.takes_persistent_form(M, K, cus)
    ldx_pad, ldy_pad, y_off = I.FWD_SHAPES[(M, N, K)]
    for name, c in I.forward_cases(M, N, K):
        planes = _split(lib, dev, c["w"])
        for bias in (False, True):
            y = _forward(lib, dev, c["x"], planes, c["b"] if bias else None, ldx_pad, ldy_pad, y_off)
            _assert_exact(y, c["ref_bias" if bias else "ref"], "%s %s bias=%s" % ((M, N, K), name, bias))


# ======================================================================================================================
# 3. k_dense3_sk
# ======================================================================================================================
@pytest.mark.parametrize("case", range(6))
def test_dense3_sk_is_exact_on_representable_answers(dev, lib, cus, case):
    M, N, K, ldx_pad, ldy_pad, y_off, recipe, wide, bias = I.sk_cases(cus)[case]
    assert I.takes_persistent_form(M, K, cus)
    c = (I.forward_ints if recipe == "ints" else I.forward_sparse)(M, N, K, wide)
    x, w, b = c["x"].to(dev), c["w"].to(dev), c["b"].to(dev)
    ref = x.double() @ w.double().t() + (b.double() if bias else 0.0)       # integers: exact in float64 on the device as well
    assert torch.equal(ref[:300].cpu(), (c["y64"][:300] + (c["b"].double() if bias else 0.0)))
    y = _forward(lib, dev, x, _split(lib, dev, w), b if bias else None, ldx_pad, ldy_pad, y_off)
    _assert_exact(y, ref.float(), "sk %s %s/%s" % ((M, N, K), recipe, wide))
    # the one-hot recipe as well: of the integer tables only (9, 9) at K = 64 gives BOTH operands a piece 1, i.e. reaches x1 y1
    o = I.forward_onehot(M, N, K)
    y = _forward(lib, dev, o["x"], _split(lib, dev, o["w"]), None, ldx_pad, ldy_pad, y_off)
    _assert_exact(y, o["ref"], "sk %s onehot" % ((M, N, K),))


# ======================================================================================================================
# 4. k_dense3_tn + k_dense3_reduce
# ======================================================================================================================
@pytest.mark.parametrize("M,N,K", list(I.WGRAD_SHAPES))
def test_weight_gradient_is_exact_and_reproducible(dev, lib, cus, M, N, K):
    ldg_pad, ldx_pad = I.WGRAD_SHAPES[(M, N, K)]
    for name, c in I.wgrad_cases(M, N, K):
        dw = _weight_grad(lib, dev, c["g"], c["x"], ldg_pad, ldx_pad, cus)
        _assert_exact(dw, c["ref"], "dw %s %s" % ((M, N, K), name))
        again = _weight_grad(lib, dev, c["g"], c["x"], ldg_pad, ldx_pad)
        assert torch.equal(dw.view(torch.int32), again.view(torch.int32)), "two runs differ"


# ======================================================================================================================
# 5. non-finite values
# ======================================================================================================================
def test_a_non_finite_value_stays_in_its_row_of_x_and_its_column_of_w(dev, lib):
    """NaN, +inf and 3.40e38 (finite, but above bfloat16's largest finite value: its first piece is inf) in three rows of x: those rows
    of y are non-finite throughout, every other row has the bits of the same call with the three rows zeroed.  Row 0 is the row the
    padding lanes of the ragged second tile read.  The same for NaN in rows 0 and 77 of w (columns of y)."""
    M, N, K = I.NONFINITE_SHAPE
    c = I.forward_ints(M, N, K, "x")
    planes = _split(lib, dev, c["w"])
    rows = [0, 5, 130]
    x_bad, x_zero = c["x"].clone(), c["x"].clone()
    x_bad[0, 3], x_bad[5, K - 1], x_bad[130, 0] = NAN, float("inf"), 3.40e38
    x_zero[rows] = 0.0
    y_bad, y_zero = _forward(lib, dev, x_bad, planes, c["b"], 4, 3), _forward(lib, dev, x_zero, planes, c["b"], 4, 3)
    assert not torch.isfinite(y_bad[rows]).any()
    keep = torch.ones(M, dtype=torch.bool, device=dev)
    keep[rows] = False
    assert torch.equal(y_bad[keep].view(torch.int32), y_zero[keep].view(torch.int32))
    _assert_exact(y_zero[keep], c["ref_bias"][keep.cpu()], "rows without a non-finite value")

    w_bad = c["w"].clone()
    w_bad[0, 40], w_bad[77, 95] = NAN, NAN
    y_bad, y_clean = _forward(lib, dev, c["x"], _split(lib, dev, w_bad), c["b"], 0, 3), _forward(lib, dev, c["x"], planes, c["b"], 0, 3)
    assert torch.isnan(y_bad[:, [0, 77]]).all()
    keep = torch.ones(N, dtype=torch.bool, device=dev)
    keep[[0, 77]] = False
    assert torch.equal(y_bad[:, keep].view(torch.int32), y_clean[:, keep].view(torch.int32))
    _assert_exact(y_clean, c["ref_bias"], "clean call")


def test_a_nan_in_row_0_stays_there_in_the_persistent_form(dev, lib, cus):
    M, N, K = 128 * cus + 77, 130, 64
    assert I.takes_persistent_form(M, K, cus)
    c = I.forward_ints(M, N, K, "x")
    x_bad, w_bad = c["x"].clone(), c["w"].clone()
    x_bad[0, 9], w_bad[0, 33] = NAN, NAN
    y_bad = _forward(lib, dev, x_bad, _split(lib, dev, w_bad), c["b"], 0, 2)
    y_clean = _forward(lib, dev, c["x"], _split(lib, dev, c["w"]), c["b"], 0, 2)
    assert torch.isnan(y_bad[0]).all() and torch.isnan(y_bad[:, 0]).all()
    assert torch.equal(y_bad[1:, 1:].view(torch.int32), y_clean[1:, 1:].view(torch.int32))
    assert not torch.isnan(y_clean).any()


# ======================================================================================================================
# 6. rounding quality on random data
# ======================================================================================================================
def rounding_figures(lib, dev, K, M=256):
    """Check 6 at one shape: the kernel's error, the float32 sequential sum's, the bound and the five-term errors of the 256-row case
    (all in units of sum |x||w|, against float64)."""
    small, c = I.normal_case(256, 256, K), I.normal_case(M, 256, K)
    five = I.five_term_errors(small["x"], small["w"])
    five_min = min(v for k, v in five.items() if k is not None)
    bound, yard = I.rounding_bound(c["x"], c["w"], five_min)
    x, w = c["x"].to(dev), c["w"].to(dev)
    y = _forward(lib, dev, x, _split(lib, dev, w), None)
    return dict(M=M, N=256, K=K, kernel=I.unit_error(y, x, w), f32_sequential=yard, bound=bound, six_term_emulation=five[None],
                five_term_emulation={"%d%d" % k: v for k, v in five.items() if k is not None})


@pytest.mark.parametrize("K,persistent", [(32, False), (256, False), (256, True)])
def test_rounding_error_stays_below_twice_a_float32_sequential_sum(dev, lib, cus, K, persistent):
    """Measured on the MI355X (256 CUs): 1.0e-7 under 4.6e-7 at K = 32, 1.1e-7 under 4.5e-7 at K = 256, 1.2e-7 under 5.1e-7 in the
    persistent form (there the bound is the cap, half the smallest five-term error: twice the sequential sum's 3.9e-7 lies above it)."""
    M = 128 * cus + 77 if persistent else 256
    assert I.takes_persistent_form(M, K, cus) == persistent
    f = rounding_figures(lib, dev, K, M)
    print("check 6:", f)
    assert f["bound"] <= 0.5 * min(f["five_term_emulation"].values())
    assert f["kernel"] <= f["bound"], f


# ======================================================================================================================
# 7. separate accumulators
# ======================================================================================================================
def same_sign_figures(lib, dev):
    """Mean signed relative error of a b^T on operands uniform in [1, 2), contraction 256, 512 x 512 outputs: through the forward
    kernel, through the weight gradient (a^T and b^T as its operands) and through torch.matmul in float32 on the device."""
    M, N, K = I.SAME_SIGN
    c = I.same_sign_case(M, N, K)
    a, b = c["a"].to(dev), c["b"].to(dev)
    ref = a.double() @ b.double().t()
    mean = lambda got: ((got.double() - ref) / ref).mean().item()
    fwd = _forward(lib, dev, a, _split(lib, dev, b), None)
    wg = _weight_grad(lib, dev, a.t().contiguous(), b.t().contiguous())
    return dict(forward=mean(fwd), weight_grad=mean(wg), torch_matmul_f32=mean(a @ b.t()))


def test_same_sign_inner_products_are_not_biased(dev, lib):
    """csrc/gemm_x3.h records a mean error of 1e-8 with all six terms in one accumulator and at most 2e-9 for the form in the tree
    (the leading term alone in one): below 5e-9, between the two.  (MI355X, this test body: forward 1.8e-11, weight gradient -7.1e-11,
    torch.matmul in float32 5.8e-11.)"""
    f = same_sign_figures(lib, dev)
    print("check 7:", f)
    assert abs(f["forward"]) < 5e-9 and abs(f["weight_grad"]) < 5e-9, f
