"""GPU: k_dz_task (csrc/dz_task.h) - dL/dZ of a full batch of 128 support and 128 query points, both cotangents by one workgroup per
task - against the two tiled launches k_bgemm3<ProbDZ<false>> / k_bgemm3<ProbDZ<true>> (csrc/gemm_x3.h), which the same batch takes
with ``gp_ops.DZ_TILED`` (ADKF_BATCH_DZ_TILED, host_gp.h::dz_task_ok).

The kernel exists at 128 + 128 points only; the small dimensions are T and d.  T = 1 and T = 3 pad the grid to 8, T = 9 starts a second
group of eight; d = 32 is a quarter of a 128-column panel, d = 96 a partial panel, d = 160 a full panel and a partial one, d = 256 the
workload.  Inputs: the seeded recipe of tests/test_gpu_hyper_onchip.py::make_inputs with its D set to d (task 2 clustered, so batches
of T >= 3 have a task on k_hyper's refine branch); RBF at every shape, Matern-5/2 at d = 32 and 256.

  1. same bits: ift_hypergrad (default, ignore_grad_correction, ignore_direct_grad) and outer_nll_value_grad without and with DZ_TILED -
     k_hyper is the same instance in both, so the weights are the same bits - give torch.equal dZ_s, dZ_q and every other output;
  2. nothing else is written: dZ_s and dZ_q lie in one buffer between guard rows of 0xFF, checked byte for byte after every call;
  3. the fall-backs take the tiled form: Z_s 4 bytes off a 16-byte boundary and d = 100 are torch.equal to the same call with
     DZ_TILED; those two, dZ_q not requested and n_s = n_q = 128 given as tensors agree with the float64 oracle within the golden
     tolerance of tests/test_gpu_parity.py (1e-4 of the largest entry);
  4. a second call on the same workspace gives the same bits, and the tasks at positions 4, 0, 8 of a T = 9 batch equal the T = 3 batch.
No bound comes from a kernel's output: 1 - 2 and 4 are bit for bit, 3 uses the existing golden tolerance."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 128
TS, DS = (1, 3, 9), (32, 96, 160, 256)
CALLS = ("hypergrad", "hypergrad_no_correction", "hypergrad_no_direct", "outer_nll")
GUARD = 256          # floats of 0xFF before, between and behind dZ_s and dZ_q (a multiple of 4: the outputs stay 16-byte aligned)
TOL = 1e-4           # tests/test_gpu_parity.py


def kernels_for(d):
    return ("rbf", "matern") if d in (32, 256) else ("rbf",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def make_inputs(n_tasks, d, seed=17):
    """tests/test_gpu_hyper_onchip.py::make_inputs with D = d: (Z_s, y_s, Z_q, y_q, phi, priors) on the CPU, float32; task 2 is the
    clustered one; one generator per task, so task t is the same in a batch of any size."""
    from oracle import gp_oracle as O

    f = lambda z: torch.sin(z[..., :4].sum(-1))
    Zs, Zq, ys, yq, phi, pri = [], [], [], [], [], []
    for t in range(n_tasks):
        g = torch.Generator().manual_seed(seed + t)
        W = torch.randn(d, d, generator=g) / math.sqrt(d)
        if t == 2:
            centres = (torch.randn(N // 4, d, generator=g) @ W).repeat_interleave(4, dim=0)
            zs, zq = centres + 0.02 * torch.randn(N, d, generator=g), centres + 0.5 * torch.randn(N, d, generator=g)
        else:
            zs, zq = torch.randn(N, d, generator=g) @ W, torch.randn(N, d, generator=g) @ W
        Zs.append(zs.float()); Zq.append(zq.float())
        ys.append((f(zs) + 0.1 * torch.randn(N, generator=g)).float())
        yq.append((f(zq) + 0.1 * torch.randn(N, generator=g)).float())
        p, pr = O.init_phi(Zs[t], use_numeric_labels=False, use_lengthscale_prior=True)
        p[2] = O.inv_softplus(0.5 * O.softplus(p[2]))
        phi.append(p.float())
        pri.append(torch.tensor(pr.as_array(), dtype=torch.float32))
    return torch.stack(Zs), torch.stack(ys), torch.stack(Zq), torch.stack(yq), torch.stack(phi), torch.stack(pri)


_INPUTS = {}


def inputs(d):
    """the nine tasks at feature dimension d, made once and left unchanged"""
    if d not in _INPUTS:
        _INPUTS[d] = make_inputs(9, d)
    return _INPUTS[d]


def take(inp, sel):
    return tuple(x[sel] for x in inp)


def _batch(dev, inp, kernel, flags=0, sizes=False, misalign=False):
    from adkf_ift_amd import gp_ops

    Zs, ys, Zq, yq, phi, pri = inp
    T, _, d = Zs.shape
    if misalign:
        flat = torch.empty(T * N * d + 1, device=dev)
        Zs_dev = flat[1:].view(T, N, d)
        Zs_dev.copy_(Zs)
        assert Zs_dev.data_ptr() % 16 == 4 and Zs_dev.is_contiguous()
    else:
        Zs_dev = Zs.to(dev)
    n = torch.full((T,), N, dtype=torch.int32) if sizes else None
    b = gp_ops.GPBatch(Zs_dev, ys.to(dev), pri.to(dev), kernel, Z_q=Zq.to(dev), y_q=yq.to(dev), n_s=n, n_q=n)
    assert b.Z_s.data_ptr() == Zs_dev.data_ptr()
    b.flags = flags
    return b, phi.to(dev)


def _guarded(dev, T, d, want_q=True):
    """-> (buffer of 0xFF bytes, dZ_s view, dZ_q view or None): guard | dZ_s | guard | dZ_q | guard"""
    n = T * N * d
    buf = torch.empty(3 * GUARD + 2 * n, device=dev)
    buf.view(torch.uint8).fill_(0xFF)
    dZs = buf[GUARD:GUARD + n].view(T, N, d)
    dZq = buf[2 * GUARD + n:2 * GUARD + 2 * n].view(T, N, d)
    assert dZs.data_ptr() % 16 == 0 and dZq.data_ptr() % 16 == 0
    return buf, dZs, (dZq if want_q else None)


def _guards_intact(buf, T, d, want_q=True):
    n = T * N * d
    by = buf.view(torch.uint8)
    spans = [(0, GUARD), (GUARD + n, 2 * GUARD + n), (2 * GUARD + 2 * n, 3 * GUARD + 2 * n)]
    if not want_q:
        spans = [(0, GUARD), (GUARD + n, 3 * GUARD + 2 * n)]
    return all(bool((by[4 * lo:4 * hi] == 0xFF).all()) for lo, hi in spans)


def _call(b, phi, call, want_q=True):
    """One call whose dZ_s / dZ_q lie between guard rows -> {output name: tensor on the CPU}"""
    from adkf_ift_amd import _lib, gp_ops
    from adkf_ift_amd._lib import ptr, stream

    T, d = b.T, b.d
    buf, dZs, dZq = _guarded(b.device, T, d, want_q)
    if call == "outer_nll":
        lib = _lib.load()
        phi = b.check_phi(phi)
        f = torch.empty(T, device=b.device)
        g = torch.empty(T, b.h, device=b.device)
        info = torch.empty(T, dtype=torch.int32, device=b.device)
        ws, nb = b.workspace()
        cb = b.c_struct()
        _lib.check(lib.adkf_outer_nll_value_grad(C.byref(cb), ptr(phi), ptr(f), ptr(g), ptr(dZs), ptr(dZq), ptr(info), ptr(ws), nb,
                                                 stream(b.device)), "adkf_outer_nll_value_grad")
        out = dict(f_out=f, g_phi=g, dZ_s=dZs)
    else:
        assert want_q
        o = gp_ops.ift_hypergrad(b, phi, ignore_grad_correction=call == "hypergrad_no_correction",
                                 ignore_direct_grad=call == "hypergrad_no_direct", out_dZ=(dZs, dZq))
        info = o["info"]
        out = {k: o[k] for k in ("f_out", "g_phi", "v", "H", "dZ_s")}
    if want_q:
        out["dZ_q"] = dZq
    torch.cuda.synchronize()
    assert int(info.abs().max()) == 0, info.tolist()
    assert _guards_intact(buf, T, d, want_q), "bytes outside dZ_s / dZ_q were written"
    out = {k: v.detach().cpu().clone() for k, v in out.items()}
    for k, v in out.items():
        assert torch.isfinite(v).all(), k
    return out


def _run(dev, inp, kernel, call, flags=0, **kw):
    b, phi = _batch(dev, inp, kernel, flags, **kw)
    return _call(b, phi, call)


def _same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert torch.equal(a[name], b[name]), (what, name, float((a[name] - b[name]).abs().max()))


def _rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("T", TS)
def test_same_bits_as_the_tiled_launches(dev, T, d):
    from adkf_ift_amd import gp_ops

    inp = take(inputs(d), slice(0, T))
    for kernel in kernels_for(d):
        for call in CALLS:
            one = _run(dev, inp, kernel, call)
            tiled = _run(dev, inp, kernel, call, flags=gp_ops.DZ_TILED)
            _same(one, tiled, (T, d, kernel, call))


@pytest.fixture(scope="module")
def oracle_direct():
    """{d: float64 dL/dZ_s, dL/dZ_q of the outer objective for the plain tasks 0 and 1}, computed once per d"""
    from oracle import gp_oracle as O

    cache = {}

    def get(d):
        if d not in cache:
            Zs, ys, Zq, yq, phi, pri = take(inputs(d), slice(0, 2))
            qs = [O.full_reference_quantities(Zs[t], ys[t], Zq[t], yq[t], phi[t].double(), O.Priors(*pri[t].double().tolist()), O.KERNEL_RBF)
                  for t in range(2)]
            cache[d] = (np.stack([q["dZs_direct"] for q in qs]), np.stack([q["dZq_direct"] for q in qs]))
        return cache[d]
    return get


@pytest.mark.parametrize("case", ("misaligned_Zs", "d100", "no_dZq", "sizes_as_tensors"))
def test_fallbacks_take_the_tiled_form(dev, oracle_direct, case):
    from adkf_ift_amd import gp_ops

    d = 100 if case == "d100" else 32
    inp = take(inputs(d), slice(0, 2))
    kw = dict(misalign=case == "misaligned_Zs", sizes=case == "sizes_as_tensors")
    b, phi = _batch(dev, inp, "rbf", **kw)
    got = _call(b, phi, "outer_nll", want_q=case != "no_dZq")
    if case in ("misaligned_Zs", "d100"):
        bt, phit = _batch(dev, inp, "rbf", flags=gp_ops.DZ_TILED, **kw)
        _same(got, _call(bt, phit, "outer_nll"), case)
    ref_s, ref_q = oracle_direct(d)
    es = _rel(got["dZ_s"].numpy(), ref_s)
    print(f"{case}: dZ_s {es:.3e} of the largest entry")
    assert es <= TOL
    if case != "no_dZq":
        eq = _rel(got["dZ_q"].numpy(), ref_q)
        print(f"{case}: dZ_q {eq:.3e} of the largest entry")
        assert eq <= TOL


def test_second_call_on_the_same_workspace_gives_the_same_bits(dev):
    for d in (32, 256):
        b, phi = _batch(dev, take(inputs(d), slice(0, 3)), "rbf")
        first = _call(b, phi, "hypergrad")
        _same(_call(b, phi, "hypergrad"), first, d)


def test_no_cross_task_state_in_a_larger_batch(dev):
    """the three tasks at positions 4, 0 and 8 of a T = 9 batch: every per-task output identical to the bit"""
    where = [4, 0, 8]
    order = torch.tensor([1, 3, 5, 6, 0, 7, 4, 8, 2])      # order[where[t]] == t
    assert [int(order[w]) for w in where] == [0, 1, 2]
    for d in (32, 160):
        small = _run(dev, take(inputs(d), slice(0, 3)), "rbf", "hypergrad")
        big = _run(dev, take(inputs(d), order), "rbf", "hypergrad")
        for name, x in big.items():
            assert torch.equal(x[where], small[name]), (d, name)
