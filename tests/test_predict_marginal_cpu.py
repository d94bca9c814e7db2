"""CPU: the ABI of adkf_predict_marginal without a GPU - clean refusal with no device, argument checks before any launch, the CPU
twin against the float64 oracle on ragged packed tasks - and gp_ops.pack_rows."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from adkf_ift_amd import _lib

BADARG, LAUNCH = -1, -4


def _rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.fixture(scope="module")
def lib():
    try:
        return _lib.load()
    except (RuntimeError, OSError) as e:
        pytest.fail(f"libadkf_gp.so must be built (build() compiles it without a GPU): {e}")


def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, ard=False, zq=True, ei=False, best=False):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    Zq = torch.zeros(rows, d) if zq else None
    q_off = torch.zeros(T + 1, dtype=torch.int64)
    out = torch.zeros(max(rows, 1)), torch.zeros(max(rows, 1)), torch.zeros(max(rows, 1))
    info, bf = torch.zeros(T, dtype=torch.int32), torch.zeros(T)
    nb = lib.adkf_workspace_bytes(T, ns, 0, d)
    ws = torch.zeros(nb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, 4 if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_predict_marginal(C.byref(b), p(phi), 0, p(Zq), p(q_off), rows, p(bf) if best else None, p(out[0]), p(out[1]),
                                     p(out[2]) if ei else None, p(info), p(ws), nb, None)


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, ei=True, best=True) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                 # a batch with a query set
    assert _host_call(lib, ard=True) == BADARG             # ARD
    assert _host_call(lib, zq=False) == BADARG             # rows > 0 without Zq
    assert _host_call(lib, ei=True, best=False) == BADARG  # ei without best_f


def test_pack_rows_round_trips():
    from adkf_ift_amd import gp_ops

    g = torch.Generator().manual_seed(0)
    Z = torch.randn(4, 9, 3, generator=g)
    n_q = torch.tensor([9, 0, 4, 1], dtype=torch.int32)
    P, q_off = gp_ops.pack_rows(Z, n_q)
    assert q_off.dtype == torch.int64 and q_off.tolist() == [0, 9, 9, 13, 14]
    assert P.shape == (14, 3)
    for t in range(4):
        assert torch.equal(P[q_off[t]:q_off[t + 1]], Z[t, :int(n_q[t])])
    back = torch.zeros_like(Z)
    for c in range(3):
        back[..., c] = gp_ops.unpack_rows(P[:, c].contiguous(), q_off, 9)
    mask = torch.arange(9)[None, :] < n_q[:, None]
    assert torch.equal(back[mask], Z[mask]) and bool((back[~mask] == 0).all())
    P2, off2 = gp_ops.pack_rows(Z)
    assert torch.equal(P2, Z.reshape(-1, 3)) and off2.tolist() == [0, 9, 18, 27, 36]


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
    fn = tw.adkf_predict_marginal   # a twin library without the entry point fails here
    return cpu_twin, fn


@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_twin_against_the_oracle(kind):
    from oracle import gp_oracle as O

    cpu_twin, fn = _twin()
    T, ns, d = 3, 12, 5
    n_s = np.array([12, 7, 10], np.int32)
    nq = [6, 0, 9]
    g = torch.Generator().manual_seed(10 + kind)
    Zs = torch.randn(T, ns, d, generator=g)
    ys = torch.randn(T, ns, generator=g)
    Zq = [torch.randn(m, d, generator=g) for m in nq]
    phi = np.array([[-2.0, 0.3, 0.8], [-1.0, 0.0, 1.2], [-3.0, 0.5, 0.5]], np.float32)
    pri = np.zeros((T, 4), np.float32)
    b = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), pri, kind, n_s=n_s)
    Zq_p = np.ascontiguousarray(torch.cat(Zq).numpy(), np.float32)
    q_off = np.array([0] + list(np.cumsum(nq)), np.int64)
    rows = Zq_p.shape[0]
    best = np.array([0.2, -0.1, -0.4], np.float32)
    pp = lambda a: a.ctypes.data_as(C.c_void_p)
    for flags in (0, 1, 2, 3):
        mean, var, ei, info = np.empty(rows, np.float32), np.empty(rows, np.float32), np.empty(rows, np.float32), np.empty(T, np.int32)
        assert fn(C.byref(b.c), pp(phi), flags, pp(Zq_p), pp(q_off), rows, pp(best), pp(mean), pp(var), pp(ei), pp(info), None, 0, None) == 0
        assert (info == 0).all()
        for t in range(T):
            lo, hi = q_off[t], q_off[t + 1]
            if hi == lo:
                continue
            n = n_s[t]
            m_ref, cov = O.predict(Zs[t, :n].double(), ys[t, :n].double(), Zq[t].double(), torch.from_numpy(phi[t]).double(), kind)
            noise = float(O.transform_phi(torch.from_numpy(phi[t]).double())[0])
            v_ref = cov.diagonal().numpy() - (noise if flags & 1 else 0.0)
            assert _rel(mean[lo:hi], m_ref.numpy()) <= 1e-4
            assert _rel(var[lo:hi], v_ref) <= 1e-4
            vl = np.maximum(cov.diagonal().numpy() - noise, 1e-12)
            s = np.sqrt(vl)
            u = ((m_ref.numpy() - best[t]) if flags & 2 else (best[t] - m_ref.numpy())) / s
            cdf = np.array([0.5 * math.erfc(-x / math.sqrt(2.0)) for x in u])
            e_ref = s * (u * cdf + np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi))
            assert _rel(ei[lo:hi], e_ref) <= 1e-4
