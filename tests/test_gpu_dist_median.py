"""GPU: the first stage of every GP call ALONE - k_colmean, the distance launch (ProbDistMulti through k_bgemm on the FP32 pipe and
k_bgemm3 on the split-bfloat16 pipe), k_median<512, 16>, k_median<1024, 32>, the k_lg_med_hist / k_lg_med_pick radix select and
k_init_params - on the inputs of tests/gp_stage_inputs.py.  The rest of the suite sees this stage only through f_in, H and dL/dZ at 1e-4 of
float64, and l0 at 1e-5 on features whose distances concentrate; here the answers are exactly representable.

Distance stage (adkf_median_lengthscale and adkf_init_params, with and without a query set; workspace pre-filled with 0xFF bytes, NaN):
  * mean == c; D2ss, D2qs, D2qq equal the integer distances on n_x x n_y; the diagonal of the symmetric blocks is 0; every other byte of
    the four regions and of the gaps between them still holds the fill (one byte-for-byte comparison with the expected image);
  * an empty task (n_s = 0) has its mean row set to 0 and nothing else written: k_colmean writes 0 for it, the distance blocks with an
    empty operand are skipped, its query-query block is computed on the uncentred rows;
  * nothing behind D2qq changes up to 256 points; above, only the radix select's scratch (one range of at most align256(258 * 4 * T) bytes);
  * l0 is bit-equal to the lower median of the integer distances (stage and select together);
  * on random features D2ss is bit-symmetric with a zero diagonal and every block lies within twice the error of a float32 sequential
    evaluation on the CPU (tests/gp_stage_inputs.py::dist_yardstick; profiles/dist_kernel_yardsticks.json).  (The symmetry check found
    the one defect: a diagonal tile of the split-bfloat16 pipe stored both halves, each summed in its own order)
Median kernels alone (ADKF_BATCH_REUSE_DIST; hand-made matrices written into D2ss): l0 bit-equal to exact_l0, 0 without a positive
candidate or with n <= 1, the stage's regions byte-identical afterwards, the same bits from a second call, and through adkf_init_params
phi0[:, 2] and priors[:, 2] within 1e-6 of their float64 values at the device's own l0.
sqrtf on the device is correctly rounded (hipcc's default for float32 sqrt): the comparisons of l0 are bit for bit, and the fallback
through the candidates was not needed.
tests/test_gp_stage_inputs.py checks the inputs and which wrong kernel each would catch; no bound comes from a kernel's output."""
import math

import numpy as np
import pytest
import torch

import gp_stage_inputs as I

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _batch(dev, Zs, Zq, n_s, n_q, flags=0):
    from adkf_ift_amd import gp_ops
    T, ld = Zs.shape[:2]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)           # (device-side sizes: an empty task passes GPBatch's host check)
    b = gp_ops.GPBatch(Zs, torch.zeros(T, ld, device=dev), torch.zeros(T, 4, device=dev), "rbf", Z_q=Zq,
                       y_q=None if Zq is None else torch.zeros(T, Zq.shape[1], device=dev), n_s=i32(n_s), n_q=None if Zq is None else i32(n_q))
    b.flags = flags
    ws, nb = b.workspace()
    assert ws.numel() == nb
    ws.fill_(0xFF)
    return b, ws


def _call(b, entry, ls_prior=True):
    """-> (l0, phi0 or None)"""
    from adkf_ift_amd import gp_ops
    if entry == "median":
        return gp_ops.median_lengthscale(b), None
    phi, l0 = gp_ops.init_params_batch(b, use_lengthscale_prior=ls_prior)
    return l0, phi


def _bits(t):
    return torch.as_tensor(t).contiguous().cpu().view(torch.int32)


def _tail_ok(ws, end, T, ns):
    changed = (ws[end:] != 0xFF).nonzero()
    if ns <= 256:
        assert changed.numel() == 0, f"{changed.numel()} bytes behind D2qq were written"
    else:
        assert changed.numel() > 0 and int(changed.max() - changed.min()) + 1 <= I.lg_med_bytes(T)


def _expected_image(case, T, ns, nq, d):
    """The first bytes of the workspace after the stage: the fill everywhere but mean and the n_x x n_y corners of the three blocks."""
    img = torch.full((sum(I.align256(4 * k) for k in (T * d, T * ns * ns, T * nq * ns, T * nq * nq)),), 0xFF, dtype=torch.uint8)
    mean, ss, qs, qq, end = I.stage_view(img, T, ns, nq, d)
    mean.copy_(case["c"].float())
    for t in range(T):
        n, n_q = case["n_s"][t], (case["n_q"][t] if nq else 0)
        ss[t, :n, :n] = case["D2ss"][t, :n, :n].float()
        if nq:
            qs[t, :n_q, :n] = case["D2qs"][t, :n_q, :n].float()
            qq[t, :n_q, :n_q] = case["D2qq"][t, :n_q, :n_q].float()
    return img[:end], end


def _check_exact(dev, case, ns, nq, d, entry, Zs_dev=None):
    T = len(case["n_s"])
    Zs = case["Z_s"].to(dev) if Zs_dev is None else Zs_dev
    b, ws = _batch(dev, Zs, case["Z_q"].to(dev) if nq else None, case["n_s"], case["n_q"])
    l0, _ = _call(b, entry)
    torch.cuda.synchronize()
    img, end = _expected_image(case, T, ns, nq, d)
    got = ws[:end].cpu()
    if not torch.equal(got, img):        # say where, region by region, before the byte comparison fails
        for name, g, w in zip(("mean", "D2ss", "D2qs", "D2qq"), I.stage_view(got, T, ns, nq, d)[:4], I.stage_view(img, T, ns, nq, d)[:4]):
            bad = (_bits(g) != _bits(w)).nonzero()
            assert bad.numel() == 0, f"{name}: {bad.shape[0]} entries differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])].item()!r} want {w[tuple(bad[0])].item()!r}"
    assert torch.equal(got, img)
    _tail_ok(ws, end, T, ns)
    want = np.array([I.exact_l0(case["D2ss"][t].float(), case["n_s"][t]) for t in range(T)], np.float32)
    assert torch.equal(_bits(l0), _bits(want)), (l0.tolist(), want.tolist())


def _cases_of(ns, nq, d, recipes="abcd", n_s=None, n_q=None):
    return [I.exact_batch(r, n_s or I.ragged_sizes(ns), n_q or I.ragged_sizes(nq), ns, nq, d) for r in recipes]


@pytest.mark.parametrize("ns,nq,d", I.dist_cases())
def test_distance_stage_is_exact_on_integer_recipes(dev, ns, nq, d):
    for case in _cases_of(ns, nq, d):
        for entry in ("median", "init"):
            if nq:
                _check_exact(dev, case, ns, nq, d, entry)
            nocase = dict(case, Z_q=None, n_q=None)                      # the same support set without a query set
            _check_exact(dev, nocase, ns, 0, d, entry)


@pytest.mark.parametrize("d", [32, 31])
def test_single_point_and_empty_tasks(dev, d):
    ns, nq = 65, 130
    for n_s in ((65, 1, 64), (65, 0, 64)):
        for case in _cases_of(ns, nq, d, "ab", n_s=n_s, n_q=(130, 129, 66)):
            assert not case["c"][1].any() or n_s[1]                      # an empty task: mean 0
            for entry in ("median", "init"):
                _check_exact(dev, case, ns, nq, d, entry)
                _check_exact(dev, dict(case, Z_q=None, n_q=None), ns, 0, d, entry)


def test_unaligned_support_features_take_the_scalar_path(dev):
    """Z_s as a contiguous view 4 bytes into a larger buffer, at a d and sizes that would otherwise use 16-byte loads."""
    ns, nq, d = 128, 132, 32
    for case in _cases_of(ns, nq, d, "abc"):
        buf = torch.empty(case["Z_s"].numel() + 1, device=dev)
        Zs = buf[1:].view(case["Z_s"].shape)
        Zs.copy_(case["Z_s"])
        assert Zs.data_ptr() % 16 == 4 and Zs.is_contiguous()
        _check_exact(dev, case, ns, nq, d, "median", Zs_dev=Zs)
        _check_exact(dev, dict(case, Z_q=None, n_q=None), ns, 0, d, "init", Zs_dev=Zs)


@pytest.mark.parametrize("ns", [128, 200, 260])
def test_stage_and_select_together(dev, ns):
    """l0 of recipe (a) is bit-equal to the lower median of the exact integer distances: what ties test_gpu_parity's 1e-5 to an exact answer."""
    case = I.exact_batch("a", I.ragged_sizes(ns), I.ragged_sizes(0), ns, 0, 32)
    for entry in ("median", "init"):
        _check_exact(dev, case, ns, 0, 32, entry)


# ---- random features -----------------------------------------------------------------------------------------------------------------
def random_figures(dev, d):
    """The device's unit errors on random_case(d) (also what tools/dist_kernel_yardsticks.py records), after the exact properties."""
    c = I.random_case(d)
    b, ws = _batch(dev, c["Z_s"][None].to(dev), c["Z_q"][None].to(dev), [I.RANDOM_NS], [I.RANDOM_NQ])
    _call(b, "median")
    torch.cuda.synchronize()
    mean, ss, qs, qq, end = I.stage_view(ws.cpu(), 1, I.RANDOM_NS, I.RANDOM_NQ, d)
    for sym in (ss[0], qq[0]):
        assert torch.equal(_bits(sym), _bits(sym.t())), "the mirror image is the bit-exact image of the original"
        assert not torch.diagonal(sym).any()
    assert torch.isfinite(qs).all() and (qs >= 0).all() and (ss >= 0).all()
    return I.dist_unit_errors([ss[0], qs[0], qq[0]], c["Z_s"], c["Z_q"], mean[0])


@pytest.mark.parametrize("d", I.RANDOM_D)
def test_random_features_within_twice_the_float32_sequential_error(dev, d):
    got, yard = random_figures(dev, d), I.dist_yardstick(d)
    for blk in ("ss", "qs", "qq"):
        print(f"d = {d} D2{blk}: device {got[blk]:.3e} yardstick {yard[blk]:.3e} bound {2 * yard[blk]:.3e}")
    for blk in ("ss", "qs", "qq"):
        assert got[blk] <= 2 * yard[blk], (blk, got[blk], yard[blk])


# ---- the median kernels alone -----------------------------------------------------------------------------------------------------------
def _inv_softplus64(l):
    return l + math.log(-math.expm1(-l))


@pytest.mark.parametrize("name", list(I.MEDIAN_BATCHES))
def test_median_kernels_on_hand_made_matrices(dev, name):
    from adkf_ift_amd import gp_ops
    ld, tasks = I.MEDIAN_BATCHES[name]
    T, nq, d = len(tasks), 3, 4
    mats = torch.stack([I.median_matrix(kind, n, ld, i) for i, (n, kind) in enumerate(tasks)])
    want = np.array([I.exact_l0(mats[i], n) for i, (n, _) in enumerate(tasks)], np.float32)
    g = torch.Generator().manual_seed(1)
    Zs, Zq = (torch.rand(T, ld, d, generator=g) * 50 - 7).to(dev), torch.full((T, nq, d), -2.5, device=dev)      # nothing to do with the matrices
    b, ws = _batch(dev, Zs, Zq, [n for n, _ in tasks], [nq] * T, flags=gp_ops.REUSE_DIST)
    mean, ss, qs, qq, end = I.stage_view(ws, T, ld, nq, d)
    ss.copy_(mats.to(dev))
    before = ws[:end].clone()

    l0, _ = _call(b, "median")
    assert torch.equal(_bits(l0), _bits(want)), [(i, tasks[i], a, w) for i, (a, w) in enumerate(zip(l0.tolist(), want.tolist())) if np.float32(a) != w]
    for i, (n, kind) in enumerate(tasks):
        if n <= 1 or kind == "all_zero":
            assert _bits(l0)[i] == 0
    assert torch.equal(ws[:end], before), "REUSE_DIST: mean and the three distance regions are the caller's"
    _tail_ok(ws, end, T, ld)
    again, _ = _call(b, "median")
    assert torch.equal(_bits(again), _bits(want)), "a second call on the same workspace: the histogram is cleared by the call itself"

    # the same through adkf_init_params: fused into k_median up to 256 points, k_init_params above
    for ls_prior in (True, False):
        l0i, phi = _call(b, "init", ls_prior)
        assert torch.equal(_bits(l0i), _bits(want))
        assert torch.equal(ws[:end], before)
        _tail_ok(ws, end, T, ld)
        phi, pri, checked = phi.cpu().double(), b.priors.cpu().double(), 0
        for i, (n, kind) in enumerate(tasks):
            l = float(want[i])
            # (the 1e-6 is asked where inv_softplus and log are well conditioned - the kinds in [16, 32), l0 in [2.8, 4); the exponent
            # kind spans 2^-63 .. 2^63 and is held through l0 alone; a task with l0 = 0 has a non-finite phi0, which is not pinned)
            if l == 0.0 or kind == "exponent":
                continue
            assert 2.8 < l < 4.0
            assert abs(phi[i, 2] - _inv_softplus64(l)) <= 1e-6 * abs(_inv_softplus64(l)), (i, kind)
            assert pri[i, 3] == (0.25 if ls_prior else -1.0)
            if ls_prior:
                assert abs(pri[i, 2] - (math.log(l) + 1 / 16)) <= 1e-6 * abs(math.log(l) + 1 / 16), (i, kind)
            else:
                assert pri[i, 2] == 0.0
            assert phi[i, 1] == 0.0 and pri[i, 1] == 0.25
            checked += 1
        assert checked >= T // 2
