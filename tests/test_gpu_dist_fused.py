"""GPU: the median select and the initialisation inside the distance launch (csrc/dist_task.h, SELECT instance; csrc/median_select.h), on
the feature sets of tests/dist_fused_inputs.py - ties in their thousands at the rank, twenty-four octaves of candidates, one positive
value, no positive candidate, an even and an odd count - at T in {1, 3, 9} and d in {32, 64, 96} (the axis-row cases need d >= 64).

Through adkf_median_lengthscale and adkf_init_params, with and without the lengthscale prior, bit for bit:
  1. l0 equals gp_stage_inputs.exact_l0 of the exact distances;
  2. the mean and the three distance blocks equal the host's values, and every other byte of a 0xFF-filled workspace keeps its fill;
  3. phi0 and the priors: the columns that do not depend on l0 equal their constants; the two that do (phi0[:, 2] = inv_softplus(l0),
     priors[:, 2] = log l0 + 1/16) come from the device's logf / expm1f, which no host library reproduces bit for bit: they are compared
     with what the SAME batch gives when n_s = n_q = 128 are passed as tensors - the generic launches, k_median calling the same
     init_params_task on the same l0 bits (that l0 is held to the host's in 1.);
  4. a task without a positive candidate: l0 == 0, phi0 / priors what init_params_task(..., 0) gives on the generic path;
  5. standard-normal features, T = 9, d = 96: the fused launch and the generic launches agree in mean, D2ss, D2qs, D2qq, l0, phi0 and priors;
  6. a second call on the same workspace gives the same bits.
No bound comes from a kernel's output."""
import numpy as np
import pytest
import torch

import dist_fused_inputs as F
import gp_stage_inputs as I

pytestmark = pytest.mark.gpu

N = F.N
TS, DS = (1, 3, 9), (32, 64, 96)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return torch.as_tensor(t).contiguous().cpu().view(torch.int32)


def _batch(dev, Zs, Zq, sizes=False):
    """A batch on a workspace filled with 0xFF; sizes: n_s = n_q = 128 as tensors (the generic launches and k_median)."""
    from adkf_ift_amd import gp_ops
    T = Zs.shape[0]
    full = lambda: torch.full((T,), N, dtype=torch.int32, device=dev)
    b = gp_ops.GPBatch(Zs, torch.zeros(T, N, device=dev), torch.zeros(T, 4, device=dev), "rbf", Z_q=Zq, y_q=torch.zeros(T, N, device=dev),
                       n_s=full() if sizes else None, n_q=full() if sizes else None)
    ws, nb = b.workspace()
    assert ws.numel() == nb
    ws.fill_(0xFF)
    return b, ws


def _call(b, entry):
    """entry: "median", "init" (with the lengthscale prior), "init_noprior" -> (l0, phi0 or None, priors or None)"""
    from adkf_ift_amd import gp_ops
    if entry == "median":
        return gp_ops.median_lengthscale(b), None, None
    phi, l0 = gp_ops.init_params_batch(b, use_lengthscale_prior=entry == "init")
    return l0, phi, b.priors.clone()


ENTRIES = ("median", "init", "init_noprior")


def _expected_image(c, T, d):
    img = torch.full((sum(I.align256(4 * k) for k in (T * d, T * N * N, T * N * N, T * N * N)),), 0xFF, dtype=torch.uint8)
    mean, ss, qs, qq, end = I.stage_view(img, T, N, N, d)
    mean.copy_(c["mean"]); ss.copy_(c["D2ss"]); qs.copy_(c["D2qs"]); qq.copy_(c["D2qq"])
    return img[:end], end


def _check_case(dev, case, T, d):
    c = F.fused_batch(case, T, d)
    want_l0 = np.array([I.exact_l0(c["D2ss"][t], N) for t in range(T)], np.float32)
    img, end = _expected_image(c, T, d)
    Zs, Zq = c["Z_s"].to(dev), c["Z_q"].to(dev)
    for entry in ENTRIES:
        b, ws = _batch(dev, Zs, Zq)
        l0, phi, pri = _call(b, entry)
        torch.cuda.synchronize()
        got = ws[:end].cpu()
        for name, g, w in zip(("mean", "D2ss", "D2qs", "D2qq"), I.stage_view(got, T, N, N, d)[:4], I.stage_view(img, T, N, N, d)[:4]):
            bad = (_bits(g) != _bits(w)).nonzero()
            assert bad.numel() == 0, f"{case} {entry} {name}: {bad.shape[0]} entries differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])].item()!r} want {w[tuple(bad[0])].item()!r}"
        assert torch.equal(got, img), "padding between the regions"
        changed = (ws[end:] != 0xFF).nonzero()
        assert changed.numel() == 0, f"{case} {entry}: {changed.numel()} bytes behind D2qq were written"
        assert torch.equal(_bits(l0), _bits(want_l0)), (case, entry, l0.tolist(), want_l0.tolist())
        if entry == "median":
            continue
        # the generic launches on the same batch: k_median's init_params_task on the same l0 bits
        bg, _ = _batch(dev, Zs, Zq, sizes=True)
        l0g, phig, prig = _call(bg, entry)
        assert torch.equal(_bits(l0g), _bits(want_l0))
        assert torch.equal(_bits(phi), _bits(phig)) and torch.equal(_bits(pri), _bits(prig)), (case, entry)
        phi, pri = phi.cpu(), pri.cpu()
        assert torch.equal(_bits(phi[:, 1]), torch.zeros(T, dtype=torch.int32)) and (pri[:, 1] == 0.25).all()
        assert (phi[:, 0] == phi[0, 0]).all() and (pri[:, 0] == pri[0, 0]).all() and torch.isfinite(phi[:, 0]).all()
        if entry == "init":
            assert (pri[:, 3] == 0.25).all()
        else:
            assert (pri[:, 3] == -1.0).all() and torch.equal(_bits(pri[:, 2]), torch.zeros(T, dtype=torch.int32))
        pos = torch.from_numpy(want_l0 > 0)
        assert torch.isfinite(phi[pos][:, 2]).all() and torch.isfinite(pri[pos][:, 2]).all()
    return want_l0


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("T", TS)
def test_exact_on_the_histograms_hard_cases(dev, T, d):
    for case in F.CASES:
        if d < F.min_d(case):
            continue
        want = _check_case(dev, case, T, d)
        if case == "c":
            assert all(want[t] == 0 for t in range(1, T, 2)), "all rows equal: no positive candidate, l0 == 0"
            assert all(want[t] == np.sqrt(np.float32(0.5) * np.float32((128 * (1 + t)) ** 2)) for t in range(0, T, 2))
        elif case in "ad":
            assert all(want[t] == (1, 3)[t % 2] for t in range(T)), "sqrt(2 s^2 / 2) = s"


def _run_all(dev, Zs, Zq, sizes):
    out = {}
    for entry in ENTRIES:
        b, ws = _batch(dev, Zs, Zq, sizes=sizes)
        l0, phi, pri = _call(b, entry)
        torch.cuda.synchronize()
        mean, ss, qs, qq, end = I.stage_view(ws.cpu(), *Zs.shape[:2], N, Zs.shape[2])
        out[entry] = dict(mean=mean, ss=ss, qs=qs, qq=qq, l0=l0.cpu(), phi=None if phi is None else phi.cpu(), priors=None if pri is None else pri.cpu())
    return out


def test_random_features_fused_against_generic(dev):
    T, d = 9, 96
    g = torch.Generator().manual_seed(9871)
    Zs, Zq = torch.randn(T, N, d, generator=g).to(dev), torch.randn(T, N, d, generator=g).to(dev)
    fused, generic = _run_all(dev, Zs, Zq, False), _run_all(dev, Zs, Zq, True)
    for entry in ENTRIES:
        for name in ("mean", "ss", "qs", "qq", "l0") + (() if entry == "median" else ("phi", "priors")):
            a, b = _bits(fused[entry][name]), _bits(generic[entry][name])
            assert torch.equal(a, b), (entry, name, int((a != b).sum()))
        assert (fused[entry]["l0"] > 0).all()
        want = np.array([I.exact_l0(fused[entry]["ss"][t], N) for t in range(T)], np.float32)
        assert torch.equal(_bits(fused[entry]["l0"]), _bits(want)), "the select is exact on the launch's own D2ss"


def test_second_call_gives_the_same_bits(dev):
    T, d = 9, 96
    c = F.fused_batch("d", T, d)
    b, ws = _batch(dev, c["Z_s"].to(dev), c["Z_q"].to(dev))
    l0, phi, pri = _call(b, "init")
    torch.cuda.synchronize()
    first = ws.clone()
    l0b, phib, prib = _call(b, "init")
    assert torch.equal(ws, first) and torch.equal(_bits(l0), _bits(l0b)) and torch.equal(_bits(phi), _bits(phib)) and torch.equal(_bits(pri), _bits(prib))
    l0c, _, _ = _call(b, "median")
    assert torch.equal(ws, first) and torch.equal(_bits(l0), _bits(l0c))
