"""GPU: k_dist_task (csrc/dist_task.h) - the distance stage of a full batch of 128 support and 128 query points by one workgroup per
task - followed by k_median, on the inputs of tests/gp_stage_inputs.py.

The kernel exists at 128 + 128 points only; the small dimensions are T and d.  T = 1 and T = 3 pad the grid to 8, T = 9 has a second
group of eight; d = 32 is one K chunk (no steady state), d = 64 one buffer swap, d = 96 an odd chunk count, d = 256 the workload's K.
The fast path is taken when the batch carries NO n_s / n_q (host_gp.h::stage_dist); the same batch with n_s = n_q = 128 given as
tensors runs the generic launch (k_bgemm3<ProbDistMulti> + k_median), which tests/test_gpu_dist_median.py holds to exact answers.

  1. exact: on the integer recipes mean == c, the three blocks equal the integer distances bit for bit, every other byte of the four
     regions and everything behind D2qq keeps the 0xFF fill, l0 is bit-equal to exact_l0 (recipe d: coincident rows, and a task
     without a positive candidate, l0 == 0) - through adkf_median_lengthscale and adkf_init_params;
  2. on standard-normal features D2ss, D2qs, D2qq, l0, phi0 and priors are bit-identical to the generic path's, and the symmetric
     blocks are bit-symmetric with a zero diagonal;
  3. the fall-backs stay exact: Z_s 4 bytes off a 16-byte boundary, no query set, d = 100;
  4. REUSE_DIST at the full shape: the select runs on the caller's D2ss, nothing is recomputed or written;
  5. a second call on the same workspace gives the same bits.
No bound comes from a kernel's output: every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import gp_stage_inputs as I

pytestmark = pytest.mark.gpu

N = 128
TS, DS = (1, 3, 9), (32, 64, 96, 256)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return torch.as_tensor(t).contiguous().cpu().view(torch.int32)


def _batch(dev, Zs, Zq, sizes=False, flags=0):
    """A batch on a workspace filled with 0xFF; sizes: give n_s / n_q = the padded size as tensors (the generic launch)."""
    from adkf_ift_amd import gp_ops
    T, ld = Zs.shape[:2]
    full = lambda n: torch.full((T,), n, dtype=torch.int32, device=dev)
    b = gp_ops.GPBatch(Zs, torch.zeros(T, ld, device=dev), torch.zeros(T, 4, device=dev), "rbf", Z_q=Zq,
                       y_q=None if Zq is None else torch.zeros(T, Zq.shape[1], device=dev),
                       n_s=full(ld) if sizes else None, n_q=full(Zq.shape[1]) if sizes and Zq is not None else None)
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


def _expected_image(case, T, ns, nq, d):
    img = torch.full((sum(I.align256(4 * k) for k in (T * d, T * ns * ns, T * nq * ns, T * nq * nq)),), 0xFF, dtype=torch.uint8)
    mean, ss, qs, qq, end = I.stage_view(img, T, ns, nq, d)
    mean.copy_(case["c"].float())
    ss.copy_(case["D2ss"].float())
    if nq:
        qs.copy_(case["D2qs"].float())
        qq.copy_(case["D2qq"].float())
    return img[:end], end


def _check_exact(dev, case, nq, d, entry, Zs_dev=None):
    T = len(case["n_s"])
    assert all(n == N for n in case["n_s"]) and (not nq or all(n == nq for n in case["n_q"]))
    b, ws = _batch(dev, case["Z_s"].to(dev) if Zs_dev is None else Zs_dev, case["Z_q"].to(dev) if nq else None)
    l0, _ = _call(b, entry)
    torch.cuda.synchronize()
    img, end = _expected_image(case, T, N, nq, d)
    got = ws[:end].cpu()
    if not torch.equal(got, img):        # say where, region by region, before the byte comparison fails
        for name, g, w in zip(("mean", "D2ss", "D2qs", "D2qq"), I.stage_view(got, T, N, nq, d)[:4], I.stage_view(img, T, N, nq, d)[:4]):
            bad = (_bits(g) != _bits(w)).nonzero()
            assert bad.numel() == 0, f"{name}: {bad.shape[0]} entries differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])].item()!r} want {w[tuple(bad[0])].item()!r}"
    assert torch.equal(got, img)
    changed = (ws[end:] != 0xFF).nonzero()
    assert changed.numel() == 0, f"{changed.numel()} bytes behind D2qq were written"
    want = np.array([I.exact_l0(case["D2ss"][t].float(), N) for t in range(T)], np.float32)
    assert torch.equal(_bits(l0), _bits(want)), (l0.tolist(), want.tolist())
    return l0


def _full_case(recipe, T, d, nq=N):
    return I.exact_batch(recipe, (N,) * T, (nq,) * T, N, nq, d)


# ---- 1. exact ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("T", TS)
def test_exact_on_integer_recipes(dev, T, d):
    for recipe in "abcd":
        case = _full_case(recipe, T, d)
        for entry in ("median", "init"):
            l0 = _check_exact(dev, case, N, d, entry)
            if recipe == "d" and T > 1:
                assert _bits(l0)[1] == 0, "all rows equal: no positive candidate"
                assert _bits(l0)[0] != 0


# ---- 2. bit-identical to the generic launch on random features ------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("T", TS)
def test_random_features_bit_identical_to_the_generic_launch(dev, T, d):
    g = torch.Generator().manual_seed(9900 + 16 * T + d)
    Zs, Zq = torch.randn(T, N, d, generator=g).to(dev), torch.randn(T, N, d, generator=g).to(dev)
    out = {}
    for sizes in (False, True):
        for entry in ("median", "init"):
            b, ws = _batch(dev, Zs, Zq, sizes=sizes)
            l0, phi = _call(b, entry)
            torch.cuda.synchronize()
            mean, ss, qs, qq, end = I.stage_view(ws.cpu(), T, N, N, d)
            out[sizes, entry] = dict(mean=mean, ss=ss, qs=qs, qq=qq, l0=l0.cpu(), phi=None if phi is None else phi.cpu(),
                                     priors=b.priors.cpu() if entry == "init" else None)
    for entry in ("median", "init"):
        fast, ref = out[False, entry], out[True, entry]
        for name in ("mean", "ss", "qs", "qq", "l0") + (("phi", "priors") if entry == "init" else ()):
            assert torch.equal(_bits(fast[name]), _bits(ref[name])), (entry, name, int((_bits(fast[name]) != _bits(ref[name])).sum()))
        for sym in (fast["ss"], fast["qq"]):
            assert torch.equal(_bits(sym), _bits(sym.transpose(1, 2))), "the mirror image is the bit-exact image of the original"
            assert not torch.diagonal(sym, dim1=1, dim2=2).any()
        assert torch.isfinite(fast["qs"]).all() and (fast["l0"] > 0).all()
    assert torch.equal(_bits(out[False, "median"]["l0"]), _bits(out[False, "init"]["l0"]))


# ---- 3. the fall-backs ---------------------------------------------------------------------------------------------------------------
def test_fallback_unaligned_support_features(dev):
    """Z_s as a contiguous view 4 bytes into a larger buffer, at the full shape: the generic launch with scalar loads."""
    T, d = 3, 64
    case = _full_case("a", T, d)
    buf = torch.empty(case["Z_s"].numel() + 1, device=dev)
    Zs = buf[1:].view(case["Z_s"].shape)
    Zs.copy_(case["Z_s"])
    assert Zs.data_ptr() % 16 == 4 and Zs.is_contiguous()
    for entry in ("median", "init"):
        _check_exact(dev, case, N, d, entry, Zs_dev=Zs)


def test_fallback_without_a_query_set(dev):
    T, d = 3, 64
    case = dict(_full_case("a", T, d), Z_q=None, n_q=None)
    for entry in ("median", "init"):
        _check_exact(dev, case, 0, d, entry)


def test_fallback_d_not_a_multiple_of_the_chunk(dev):
    T, d = 3, 100
    case = _full_case("a", T, d)
    for entry in ("median", "init"):
        _check_exact(dev, case, N, d, entry)


# ---- 4. REUSE_DIST at the full shape ---------------------------------------------------------------------------------------------------
def test_reuse_dist_runs_the_select_on_the_callers_matrix(dev):
    from adkf_ift_amd import gp_ops
    kinds = [k for k in I.MEDIAN_KINDS]
    T, d = len(kinds), 32
    mats = torch.stack([I.median_matrix(kind, N, N, i) for i, kind in enumerate(kinds)])
    want = np.array([I.exact_l0(mats[i], N) for i in range(T)], np.float32)
    g = torch.Generator().manual_seed(2)
    Zs, Zq = (torch.rand(T, N, d, generator=g) * 50 - 7).to(dev), torch.full((T, N, d), -2.5, device=dev)    # nothing to do with the matrices
    b, ws = _batch(dev, Zs, Zq, flags=gp_ops.REUSE_DIST)
    mean, ss, qs, qq, end = I.stage_view(ws, T, N, N, d)
    ss.copy_(mats.to(dev))
    before = ws.clone()
    for entry in ("median", "init"):
        l0, _ = _call(b, entry)
        assert torch.equal(_bits(l0), _bits(want)), [(kinds[i], a, w) for i, (a, w) in enumerate(zip(l0.tolist(), want.tolist())) if np.float32(a) != w]
        assert torch.equal(ws, before), "REUSE_DIST: nothing is recomputed, nothing in the workspace is written"


# ---- 5. a second call ------------------------------------------------------------------------------------------------------------------
def test_second_call_on_the_same_workspace(dev):
    T, d = 9, 96
    g = torch.Generator().manual_seed(9990)
    Zs, Zq = torch.randn(T, N, d, generator=g).to(dev), torch.randn(T, N, d, generator=g).to(dev)
    b, ws = _batch(dev, Zs, Zq)
    l0, phi = _call(b, "init")
    torch.cuda.synchronize()
    end = I.stage_view(ws, T, N, N, d)[4]
    first, pri = ws[:end].clone(), b.priors.clone()
    l0b, phib = _call(b, "init")
    assert torch.equal(ws[:end], first) and torch.equal(_bits(l0), _bits(l0b)) and torch.equal(_bits(phi), _bits(phib))
    assert torch.equal(_bits(pri), _bits(b.priors))
    l0c, _ = _call(b, "median")
    assert torch.equal(ws[:end], first) and torch.equal(_bits(l0), _bits(l0c))
