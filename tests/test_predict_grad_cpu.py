"""CPU: adkf_predict_grad without a GPU - the CPU twin against float64 autograd through the oracle (grad_ref.py) on ragged packed
tasks, argument checks before any launch, a clean refusal with no device, and the wiring of models._PredictMarginalFunction with
gp_ops stubbed by the twin."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_ref as R
from adkf_ift_amd import _lib

BADARG, WORKSPACE, LAUNCH = -1, -3, -4
ARD, LATENT, MAXIMIZE, LOG_EI = 4, 1, 2, 16


@pytest.fixture(scope="module")
def lib():
    try:
        return _lib.load()
    except (RuntimeError, OSError) as e:
        pytest.fail(f"libadkf_gp.so must be built (build() compiles it without a GPU): {e}")


def _twin():
    import os
    import shutil
    import subprocess

    from oracle import cpu_twin
    if not os.path.exists(cpu_twin.LIB) and shutil.which("g++") is None:   # no host compiler: the twin is checker-only
        pytest.skip("CPU twin not built and no g++ to build it")
    try:
        tw = cpu_twin.load()
    except subprocess.CalledProcessError as e:   # the compiler is there but cannot build it (e.g. no OpenMP)
        pytest.skip(f"CPU twin could not be built: {e}")
    return cpu_twin, tw.adkf_predict_grad   # a twin library without the entry point fails here


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, ard=False, flags=0, zq=True, dz=True, cot=(True, False, False), best=False,
               short_ws=False):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    Zq = torch.zeros(max(rows, 1), d) if zq else None
    dZq = torch.zeros(max(rows, 1), d) if dz else None
    g = [torch.zeros(max(rows, 1)) if c else None for c in cot]
    q_off = torch.zeros(T + 1, dtype=torch.int64)
    info, bf = torch.zeros(T, dtype=torch.int32), torch.zeros(T)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    ws = torch.zeros(nb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_predict_grad(C.byref(b), p(phi), flags, p(Zq), p(q_off), rows, p(bf) if best else None, p(g[0]), p(g[1]), p(g[2]),
                                 p(dZq), p(info), p(ws), nb // 2 if short_ws else nb, None)


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, cot=(True, True, True), best=True, flags=LOG_EI | MAXIMIZE) == LAUNCH
    assert _host_call(lib, ard=True, cot=(False, True, False)) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                           # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, zq=False) == BADARG                                       # rows > 0 without Zq
    assert _host_call(lib, dz=False) == BADARG                                       # rows > 0 without dZq
    assert _host_call(lib, cot=(False, False, False)) == BADARG                      # no cotangent at all
    assert _host_call(lib, cot=(False, False, True), best=False) == BADARG           # g_ei without best_f
    assert _host_call(lib, flags=LOG_EI, cot=(True, True, False), best=True) == BADARG   # LOG_EI without g_ei
    assert _host_call(lib, flags=8) == BADARG and _host_call(lib, flags=4) == BADARG     # any other flag bit
    assert _host_call(lib, short_ws=True) == WORKSPACE
    assert _host_call(lib, ard=True, short_ws=True) == WORKSPACE


def _ragged(kind, ard):
    """The ragged tasks of test_predict_marginal_cpu.py: T = 3, n_s = 12, 7, 10, d = 5, nq = 6, 0, 9."""
    T, ns, d = 3, 12, 5
    n_s = np.array([12, 7, 10], np.int32)
    nq = [6, 0, 9]
    g = torch.Generator().manual_seed(10 + kind)
    Zs = torch.randn(T, ns, d, generator=g)
    ys = torch.randn(T, ns, generator=g)
    Zq = [torch.randn(m, d, generator=g) for m in nq]
    phi = np.array([[-2.0, 0.3, 0.8], [-1.0, 0.0, 1.2], [-3.0, 0.5, 0.5]], np.float32)
    if ard:   # one lengthscale per dimension around each task's isotropic one
        spread = 1.0 + 0.3 * (2.0 * torch.rand(T, d, generator=g).numpy() - 1.0)
        ell = np.log1p(np.exp(phi[:, 2:3].astype(np.float64))) * spread
        phi = np.concatenate([phi[:, :2], np.log(np.expm1(ell)).astype(np.float32)], axis=1)
    best = np.array([0.2, -0.1, -0.4], np.float32)
    return Zs, ys, n_s, nq, Zq, np.ascontiguousarray(phi), best


def twin_grad(cpu_twin, fn, Zs, ys, n_s, kind, ard, phi, Zq_p, q_off, best, flags, gm, gv, ge):
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T = Zs.shape[0]
    b = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((T, 4), np.float32), kind, n_s=n_s)
    if ard:
        b.c.flags = ARD
    rows = Zq_p.shape[0]
    dZ, info = np.full((rows, Zq_p.shape[1]), 7.0, np.float32), np.empty(T, np.int32)
    rc = fn(C.byref(b.c), pp(phi), flags, pp(Zq_p), pp(q_off), rows, pp(best) if ge is not None else None, pp(gm), pp(gv), pp(ge),
            pp(dZ), pp(info), None, 0, None)
    assert rc == 0 and (info == 0).all()
    return dZ


@pytest.mark.parametrize("kind,ard", [(0, False), (1, False), (1, True)])
def test_cpu_twin_against_autograd(kind, ard):
    cpu_twin, fn = _twin()
    Zs, ys, n_s, nq, Zq, phi, best = _ragged(kind, ard)
    Zq_p = np.ascontiguousarray(torch.cat(Zq).numpy(), np.float32)
    q_off = np.array([0] + list(np.cumsum(nq)), np.int64)
    rows = Zq_p.shape[0]
    cots = R.cotangents(rows, 3)
    worst = 0.0
    for name, um, uv, ue, maximize, log_ei in R.COMBOS:
        gm, gv, ge = (cots[0] if um else None), (cots[1] if uv else None), (cots[2] if ue else None)
        flags = (MAXIMIZE if maximize else 0) | (LOG_EI if log_ei else 0)
        dZ = twin_grad(cpu_twin, fn, Zs, ys, n_s, kind, ard, phi, Zq_p, q_off, best, flags, gm, gv, ge)
        for t in range(3):
            lo, hi = q_off[t], q_off[t + 1]
            if hi == lo:
                continue
            n = n_s[t]
            sl = lambda a: None if a is None else a[lo:hi]
            ref = R.predict_grad_ref(Zs[t, :n], ys[t, :n], Zq[t], phi[t], kind, sl(gm), sl(gv), sl(ge), best[t], maximize, log_ei)[0]
            err = R.rel(dZ[lo:hi], ref)
            worst = max(worst, err / R.TOL)
            assert err <= R.TOL, (name, t, err)
        # LATENT changes no gradient
        assert np.array_equal(dZ, twin_grad(cpu_twin, fn, Zs, ys, n_s, kind, ard, phi, Zq_p, q_off, best, flags | LATENT, gm, gv, ge)), name
    print(f"kind {kind} ard {ard}: worst error / bound {worst:.2e}")


def test_cpu_twin_zero_rows_and_zero_cotangents():
    cpu_twin, fn = _twin()
    Zs, ys, n_s, nq, Zq, phi, best = _ragged(0, False)
    Zq_p = np.ascontiguousarray(torch.cat(Zq).numpy(), np.float32)
    rows = Zq_p.shape[0]
    q_off = np.array([2, 6, 6, 12], np.int64)   # rows 0, 1 and 12.. belong to nobody
    z = np.zeros(rows, np.float32)
    dZ = twin_grad(cpu_twin, fn, Zs, ys, n_s, 0, False, phi, Zq_p, q_off, best, 0, z, z, z)
    assert (dZ == 0).all()
    dZ = twin_grad(cpu_twin, fn, Zs, ys, n_s, 0, False, phi, Zq_p, q_off, best, 0, z + 1, None, None)
    assert (dZ[:2] == 0).all() and (dZ[12:] == 0).all() and (dZ[2:12] != 0).any()


class _StubBatch:
    """What models._PredictMarginalFunction hands to gp_ops: opaque there, the twin's batch here."""
    def __init__(self, cpu_twin, Zs, ys, n_s, kind):
        self.tw = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((Zs.shape[0], 4), np.float32), kind, n_s=n_s)
        self.T = Zs.shape[0]


def test_predict_marginal_function_wiring(monkeypatch):
    """models.predict_marginal_diff with gp_ops.predict_marginal / predict_grad / check_info stubbed by the twin on CPU tensors:
    the three cotangents reach one predict_grad call, only Zq gets a gradient, and the chain through a linear map is the oracle's."""
    from adkf_ift_amd import models

    cpu_twin, fn = _twin()
    tw = cpu_twin.load()
    Zs, ys, n_s, nq, Zq, phi, best = _ragged(1, False)
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    calls = []

    def predict_marginal(b, phi_t, Zq_t, q_off_t, latent=False, best_f=None, maximize=False, want_var=True, log_ei=False):
        z, off = np.ascontiguousarray(Zq_t.numpy(), np.float32), np.ascontiguousarray(q_off_t.numpy(), np.int64)
        rows = z.shape[0]
        m, v, e = (np.empty(rows, np.float32) for _ in range(3))
        info = np.empty(b.T, np.int32)
        bf = None if best_f is None else np.ascontiguousarray(best_f.numpy(), np.float32)
        flags = (LATENT if latent else 0) | (MAXIMIZE if maximize else 0) | (LOG_EI if log_ei else 0)
        assert tw.adkf_predict_marginal(C.byref(b.tw.c), pp(np.ascontiguousarray(phi_t.numpy())), flags, pp(z), pp(off), rows, pp(bf), pp(m), pp(v),
                                        pp(e) if bf is not None else None, pp(info), None, 0, None) == 0
        return torch.from_numpy(m), torch.from_numpy(v), (torch.from_numpy(e) if bf is not None else None), torch.from_numpy(info)

    def predict_grad(b, phi_t, Zq_t, q_off_t, *, g_mean=None, g_var=None, g_ei=None, best_f=None, maximize=False, log_ei=False):
        calls.append((g_mean is not None, g_var is not None, g_ei is not None, maximize, log_ei))
        z, off = np.ascontiguousarray(Zq_t.numpy(), np.float32), np.ascontiguousarray(q_off_t.numpy(), np.int64)
        f = lambda t: None if t is None else np.ascontiguousarray(t.numpy(), np.float32)
        dZ, info = np.empty(z.shape, np.float32), np.empty(b.T, np.int32)
        flags = (MAXIMIZE if maximize else 0) | (LOG_EI if log_ei else 0)
        assert fn(C.byref(b.tw.c), pp(np.ascontiguousarray(phi_t.numpy())), flags, pp(z), pp(off), z.shape[0], pp(f(best_f)), pp(f(g_mean)),
                  pp(f(g_var)), pp(f(g_ei)), pp(dZ), pp(info), None, 0, None) == 0
        return torch.from_numpy(dZ), torch.from_numpy(info)

    monkeypatch.setattr(models.gp_ops, "predict_marginal", predict_marginal)
    monkeypatch.setattr(models.gp_ops, "predict_grad", predict_grad)
    monkeypatch.setattr(models.gp_ops, "check_info", lambda info, what="": None)

    b = _StubBatch(cpu_twin, Zs, ys, n_s, 1)
    q_off = torch.tensor([0] + list(np.cumsum(nq)), dtype=torch.int64)
    X = torch.cat(Zq)                                   # [rows, 5]
    lin = torch.nn.Linear(5, 5)
    torch.manual_seed(0)
    with torch.no_grad():
        lin.weight.copy_(torch.eye(5) + 0.1 * torch.randn(5, 5))
        lin.bias.copy_(0.05 * torch.randn(5))
    phi_t = torch.from_numpy(phi).requires_grad_(True)
    best_t = torch.from_numpy(best)
    mean, var, ei = models.predict_marginal_diff(b, phi_t, lin(X), q_off, best_f=best_t, maximize=True, log_ei=True)
    (mean.sum() + 0.5 * var.sum() + 0.25 * ei.sum()).backward()
    assert calls == [(True, True, True, True, True)]
    assert phi_t.grad is None                           # phi is a constant of the fitted state
    # the same chain in float64 autograd
    lin64 = torch.nn.Linear(5, 5).double()
    with torch.no_grad():
        lin64.weight.copy_(lin.weight.double()); lin64.bias.copy_(lin.bias.double())
    Z64 = lin64(X.double())
    total = torch.zeros((), dtype=torch.float64)
    for t in range(3):
        lo, hi = int(q_off[t]), int(q_off[t + 1])
        if hi == lo:
            continue
        n = n_s[t]
        m, v, _ = R.posterior(Zs[t, :n].double(), ys[t, :n].double(), Z64[lo:hi], torch.from_numpy(phi[t]).double(), 1)
        E, _ = R.acquisition(m, v, float(best[t]), True, True)
        total = total + m.sum() + 0.5 * v.sum() + 0.25 * E.sum()
    total.backward()
    assert R.rel(lin.weight.grad.numpy(), lin64.weight.grad.numpy()) <= R.TOL
    assert R.rel(lin.bias.grad.numpy(), lin64.bias.grad.numpy()) <= R.TOL
    # without best_f the third output is a constant and the backward passes no g_ei
    calls.clear()
    mean, var, ei = models.predict_marginal_diff(b, phi_t, lin(X), q_off)
    assert not ei.requires_grad and bool((ei == 0).all())
    (mean.sum() + var.sum()).backward()
    assert calls == [(True, True, False, False, False)]
