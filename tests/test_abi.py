"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/adkf_gp.h declares.
No compute call is made here (there is no GPU); host-only entry points are exercised."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from adkf_ift_amd import _lib

    ge.build()
    return _lib.load()


def test_every_declared_symbol_is_exported(lib):
    from adkf_ift_amd import _lib

    header = open(os.path.join(ROOT, "include", "adkf_gp.h")).read()
    declared = set(re.findall(r"\b(adkf_[a-z_]+)\s*\(", header))
    assert len(declared) >= 11
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name


def test_host_only_entry_points(lib):
    assert b"gfx950" in lib.adkf_version()
    assert lib.adkf_max_points() >= 256
    assert lib.adkf_workspace_bytes(0, 8, 8, 4) == 0
    small = lib.adkf_workspace_bytes(4, 16, 16, 8)
    big = lib.adkf_workspace_bytes(256, 128, 128, 256)
    assert 0 < small < big
    assert big > 11 * 256 * 128 * 128 * 4  # the eleven N x N work matrices


# What the size functions returned before the host layer was split by subsystem (a build of a970107): callers size their buffers by
# them, tests and tools read the workspace by the carve order behind them.  Shapes: at most 128 points (no blocked-sweep region), more
# than 128 (with it), more than 1024 (no float64 region), support-only batches, and more tasks than the 4096 candidate lists of a pool call.
PINNED_SIZES = {
    "adkf_workspace_bytes": {(4, 16, 16, 8): 794624, (256, 128, 128, 256): 625443840, (8, 1024, 0, 64): 431082240,
                             (3, 200, 256, 24): 22236928, (2, 17, 41, 33): 649728, (1, 2048, 0, 16): 69520896},
    "adkf_workspace_bytes_ard": {(4, 16, 0, 8): 745216, (4, 16, 16, 8): 826624, (3, 200, 0, 24): 9691136, (64, 128, 128, 256): 217598720},
    "adkf_predict_pool_scratch_bytes": {(3, 64): 3144960, (1, 1): 49152, (5000, 8): 480000, (256, 64): 3145728},
    "adkf_thompson_pool_scratch_bytes": {(3, 200, 16, 1024): 901632, (1, 16, 1, 64): 49664, (256, 128, 64, 4096): 28311552,
                                         (2, 2048, 8, 128): 524288},
    "adkf_block_combine_scratch_bytes": {(1000, 128): 12320},
}


@pytest.mark.skipif("ADKF_R64_MAXN" in os.environ, reason="ADKF_R64_MAXN changes the workspace sizes")
def test_size_functions_return_the_pinned_sizes(lib):
    for name, cases in PINNED_SIZES.items():
        for args, nbytes in cases.items():
            assert getattr(lib, name)(*args) == nbytes, (name, args)


def test_bad_arguments_are_rejected_without_touching_the_gpu(lib):
    import ctypes as C

    from adkf_ift_amd._lib import Batch

    b = Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel = 0, 8, 8, 4, 0
    assert lib.adkf_median_lengthscale(C.byref(b), None, None, 0, None) == -1
    b.T, b.Z_s = 2, 1  # non-null dummy pointer; rejected before any launch
    b.ns_max = 100000
    assert lib.adkf_median_lengthscale(C.byref(b), None, None, 0, None) == -2
    b.ns_max, b.kernel = 8, 7
    assert lib.adkf_median_lengthscale(C.byref(b), None, None, 0, None) == -1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from adkf_ift_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        _lib.load()


def test_cpu_tensors_are_refused():
    import torch

    from adkf_ift_amd import gp_ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gp_ops.GPBatch(torch.zeros(1, 4, 2), torch.zeros(1, 4), torch.zeros(1, 4))


def test_ctypes_signatures_agree_with_the_header(lib):
    """Every ctypes prototype in adkf_ift_amd/_lib.py has the argument count AND the scalar classes (pointer / integer /
    float / double) of the C declaration - a float passed where the header says double would be silently misread."""
    import ctypes as C

    from adkf_ift_amd import _lib

    header = open(os.path.join(ROOT, "include", "adkf_gp.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    protos = dict(re.findall(r"\b(adkf_[a-z_]+)\s*\(([^)]*)\)\s*;", header))
    assert set(protos) == set(_lib.SIGNATURES)

    def c_class(decl):
        decl = decl.strip()
        if decl in ("void", ""):
            return None
        if "*" in decl:
            return "ptr"
        ty = decl.rsplit(" ", 1)[0].replace("const", "").strip()
        return {"int32_t": "i32", "int": "i32", "int64_t": "i64", "size_t": "size", "float": "f32", "double": "f64"}[ty]

    def py_class(t):
        if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer)):
            return "ptr"
        return {C.c_int32: "i32", C.c_int: "i32", C.c_int64: "i64", C.c_size_t: "size", C.c_float: "f32", C.c_double: "f64"}[t]

    for name, args in protos.items():
        want = [c for c in (c_class(a) for a in args.split(",")) if c is not None]
        got = [py_class(t) for t in _lib.SIGNATURES[name][1]]
        assert want == got, (name, want, got)


def test_ctypes_structs_mirror_the_header():
    """adkf_batch_t / adkf_fit_options_t: same field names, order and scalar classes as the ctypes.Structure mirrors."""
    import ctypes as C

    from adkf_ift_amd import _lib

    header = open(os.path.join(ROOT, "include", "adkf_gp.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for cname, mirror in (("adkf_batch", _lib.Batch), ("adkf_fit_options", _lib.FitOptions)):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}" % cname, header, flags=re.S).group(1)
        fields = []
        for decl in (d.strip() for d in body.split(";")):
            if not decl:
                continue
            name = re.findall(r"[A-Za-z_0-9]+", decl)[-1]
            kind = "ptr" if "*" in decl else {"int32_t": "i32", "float": "f32"}[decl.split()[0]]
            fields.append((name, kind))
        got = [(n, "ptr" if t is C.c_void_p else {C.c_int32: "i32", C.c_float: "f32"}[t]) for n, t in mirror._fields_]
        assert fields == got, (cname, fields, got)


@pytest.mark.parametrize("ns,nq", [(32, 32), (128, 128), (200, 256)])
def test_entry_points_fail_cleanly_without_a_device(lib, ns, nq):
    """Host side of the entry points on a box WITHOUT a GPU: argument checks, workspace carving and the launch sequence run, every
    launch is refused by the runtime and the call returns ADKF_E_LAUNCH - it must not crash (round 5: a host-side recursion in the
    workspace helper took the whole process down on the first call, and no CPU test went through an entry point).  Host memory stands
    in for device memory: nothing is ever dereferenced on the host."""
    import ctypes as C

    import torch
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    from adkf_ift_amd import _lib

    T, d = 3, 8
    nb = lib.adkf_workspace_bytes(T, ns, nq, d)
    ws = torch.zeros(nb // 4 + 64)
    Zs, Zq, ys, yq = torch.zeros(T, ns, d), torch.zeros(T, nq, d), torch.zeros(T, ns), torch.zeros(T, nq)
    pri, phi, l0, f, g, info = torch.zeros(T, 4), torch.zeros(T, 3), torch.zeros(T), torch.zeros(T), torch.zeros(T, 3), torch.zeros(T, dtype=torch.int32)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.Z_q, b.y_q, b.priors = Zs.data_ptr(), ys.data_ptr(), Zq.data_ptr(), yq.data_ptr(), pri.data_ptr()
    p = lambda t: C.c_void_p(t.data_ptr())
    for flags in (0, 16, 32):   # ADKF_BATCH_LG_UNFUSED, ADKF_BATCH_LG_FUSED
        b.flags = flags
        assert lib.adkf_init_params(C.byref(b), 0, 1, p(phi), p(pri), p(l0), p(ws), nb, None) == -4
        assert lib.adkf_mll_value_grad(C.byref(b), p(phi), p(f), p(g), None, p(info), p(ws), nb, None) == -4
        opt = _lib.FitOptions(5, 1, 1e-5, 2.22e-9, None, None)
        assert lib.adkf_fit(C.byref(b), p(phi), C.byref(opt), p(f), p(l0), None, p(info), p(ws), nb, None) == -4
    assert b"device" in lib.adkf_last_hip_error() or lib.adkf_last_hip_error()


# ---- the GNN entries (csrc/pna.h, csrc/block.h, csrc/readout.h): rejected arguments return before any launch -----------------------
_E_BADARG, _E_SIZE, _E_WORKSPACE = -1, -2, -3


def _dummy(n):
    """n distinct non-null addresses that are never dereferenced: every call below must return from its argument checks."""
    import ctypes as C
    return [C.c_void_p(4096 + 64 * i) for i in range(n)]


def _msg_table(Es, backward):
    import ctypes as C

    from adkf_ift_amd import _lib
    tab = (_lib.MsgEt * len(Es))()
    for et, E in enumerate(Es):
        tab[et].src, tab[et].tgt, tab[et].W = 4096, 8192, 12288
        tab[et].bias = None if backward else 16384
        tab[et].dW, tab[et].db = (20480, 24576) if backward else (None, None)
        tab[et].E = E
    return C.cast(tab, C.c_void_p), tab


def test_block_combine_rejects_unsupported_widths_and_a_short_scratch(lib):
    d = _dummy(20)
    for hid in (100, 320):
        assert lib.adkf_block_combine(*d[:8], 1e-5, 8, hid, *d[8:12], None) == _E_SIZE
        assert lib.adkf_block_combine_backward(*d[:11], 8, hid, *d[11:18], 1 << 30, None) == _E_SIZE
    for V, hid in ((8, 64), (129, 256)):
        need = lib.adkf_block_combine_scratch_bytes(V, hid)
        assert need == 4 * ((V + 127) // 128) * (3 * hid + 1)
        assert lib.adkf_block_combine_backward(*d[:11], V, hid, *d[11:18], need - 1, None) == _E_WORKSPACE


def test_readout_pooling_rejects_shapes_beyond_its_budgets(lib):
    d = _dummy(24)
    V, G = 10, 2
    assert lib.adkf_readout_pool(*d[:7], V, G, 65, 4, 16, *d[7:13], None) == _E_BADARG
    for nh, K, ldh, D in ((65, 64, 64, 16), (4, 1025, 1025, 16), (4, 64, 63, 16), (4, 64, 64, 2049)):
        assert lib.adkf_readout_pool_hidden(*d[:4], ldh, *d[4:7], V, G, nh, K, D, *d[7:15], None) == _E_BADARG, (nh, K, ldh, D)
        assert lib.adkf_readout_pool_hidden_backward(*d[:2], ldh, *d[2:11], V, G, nh, K, D, *d[11:16], None) == _E_BADARG, (nh, K, ldh, D)


def test_message_entries_reject_bad_tables_and_a_short_scratch(lib):
    d = _dummy(12)
    H, inn, out = 3, 5, 7
    for backward in (False, True):
        for Es, n_et in (((10, 10, 10, 10, 10), 5), ((10, -1), 2)):
            ptr, keep = _msg_table(Es, backward)
            if backward:
                rc = lib.adkf_msg_backward(d[0], ptr, n_et, H, inn, out, d[1], d[2], d[3], d[4], d[5], d[6], 50, d[7], d[8], d[9], 1 << 30, None)
            else:
                rc = lib.adkf_msg_forward(d[0], ptr, n_et, H, inn, out, d[1], None)
            assert rc == _E_BADARG, (backward, Es)
    ptr, keep = _msg_table((513, 0, 10), True)
    need = lib.adkf_msg_backward_scratch_bytes(ptr, 3, H, inn, out)
    assert need > 0
    assert lib.adkf_msg_backward(d[0], ptr, 3, H, inn, out, d[1], d[2], d[3], d[4], d[5], d[6], 50, d[7], d[8], d[9], need - 1, None) == _E_WORKSPACE
    assert lib.adkf_msg_backward(d[0], ptr, 3, H, inn, out, d[1], d[2], d[3], d[4], d[5], d[6], 50, d[7], d[8], None, 0, None) == _E_WORKSPACE


def test_message_forward_without_any_edge_launches_nothing(lib):
    """A batch of single-atom graphs: every edge type is empty, nothing is launched and the call succeeds - with or without a device.
    (adkf_ift_amd/gnn.py passes one unused row where the empty message tensor has no address.)"""
    d = _dummy(2)
    ptr, keep = _msg_table((0, 0, 0), False)
    assert lib.adkf_msg_forward(d[0], ptr, 3, 4, 4, 18, d[1], None) == 0
    assert lib.adkf_msg_forward(d[0], ptr, 3, 4, 4, 18, None, None) == _E_BADARG     # a missing output is still a bad argument


def test_message_backward_chunking_is_a_function_of_E_alone(lib):
    """scratch = 4 sum_et nsplit(E_et) (2 H in out + H out) bytes with nsplit(E) = ceil(E / chunk), chunk = max(512, ceil(E / 64) rounded up
    to a multiple of 32): one partial of d W | d b per chunk (csrc/pna.h)."""
    nsplit = {0: 0, 1: 1, 512: 1, 513: 2, 4100: 9, 32768: 64, 32769: 61}
    for E, n in nsplit.items():
        chunk = max(512, -(-(-(-E // 64)) // 32) * 32)
        assert n == (-(-E // chunk) if E > 0 else 0)
    for H, inn, out in ((3, 5, 7), (4, 32, 192)):
        per = 2 * H * inn * out + H * out
        for E, n in nsplit.items():
            ptr, keep = _msg_table((E,), True)
            assert lib.adkf_msg_backward_scratch_bytes(ptr, 1, H, inn, out) == 4 * n * per, E
        for Es in ((0, 1, 512, 513), (4100, 32768, 32769), (32769, 0, 4100, 513)):
            ptr, keep = _msg_table(Es, True)
            assert lib.adkf_msg_backward_scratch_bytes(ptr, len(Es), H, inn, out) == 4 * sum(nsplit[E] for E in Es) * per, Es


# ---- the dense entries (csrc/dense_x3.h): rejected arguments return before any launch -----------------------------------------------
def test_split_entries_reject_bad_arguments(lib):
    import ctypes as C
    x, planes = C.c_void_p(4096), C.c_void_p(8192)
    for fn in (lib.adkf_split_planes, lib.adkf_split_planes_t):
        assert fn(None, planes, 8, 8, None) == _E_BADARG and fn(x, None, 8, 8, None) == _E_BADARG
        for a, b in ((0, 8), (8, 0), (-8, 8), (8, -8)):
            assert fn(x, planes, a, b, None) == _E_BADARG, (a, b)
        assert fn(x, C.c_void_p(8192 + 8), 8, 8, None) == _E_BADARG                 # planes: 16-byte aligned
    assert lib.adkf_split_planes(x, planes, 8, 7, None) == _E_BADARG                # K odd
    assert lib.adkf_split_planes_t(x, planes, 7, 8, None) == _E_BADARG
    assert lib.adkf_split_planes(x, planes, 1, 4, None) == _E_BADARG                # rows K not a multiple of 8
    assert lib.adkf_split_planes(x, planes, 3, 6, None) == _E_BADARG
    assert lib.adkf_split_planes_t(x, planes, 2, 3, None) == _E_BADARG              # N K not a multiple of 8
    assert lib.adkf_split_planes(C.c_void_p(4096 + 4), planes, 8, 8, None) == _E_BADARG      # x: 8-byte aligned (pairs)
    assert lib.adkf_split_planes_t(C.c_void_p(4096 + 2), planes, 8, 8, None) == _E_BADARG    # w: a float


def test_dense_forward_rejects_bad_arguments(lib):
    import ctypes as C
    x, planes, bias, y = _dummy(4)
    M, N, K = 5, 3, 32
    call = lambda x=x, ldx=K, planes=planes, y=y, ldy=N, M=M, N=N, K=K: lib.adkf_dense_forward(x, ldx, planes, bias, y, ldy, M, N, K, None)
    for kw in (dict(x=None), dict(planes=None), dict(y=None), dict(M=0), dict(N=0), dict(K=0, ldx=0), dict(M=-1), dict(N=-3), dict(K=-32),
               dict(ldx=K - 4), dict(ldy=N - 1)):
        assert call(**kw) == _E_BADARG, kw
    for kw in (dict(K=48, ldx=48), dict(K=31, ldx=32), dict(ldx=K + 1), dict(ldx=K + 2)):      # K a multiple of 32, ldx of 4
        assert call(**kw) == _E_SIZE, kw
    for kw in (dict(x=C.c_void_p(4096 + 8)), dict(x=C.c_void_p(4096 + 4)), dict(planes=C.c_void_p(8192 + 8)), dict(planes=C.c_void_p(8192 + 2))):
        assert call(**kw) == _E_BADARG, kw


def test_dense_weight_grad_rejects_bad_arguments_and_a_short_scratch(lib):
    g, x, dw, scratch = _dummy(4)
    M, N, K = 300, 5, 7
    need = lib.adkf_dense_weight_grad_scratch_bytes(M, N, K)
    assert need >= 4 * N * K and need % (4 * N * K) == 0
    call = lambda g=g, ldg=N, x=x, ldx=K, dw=dw, M=M, N=N, K=K, scratch=scratch, nb=need: lib.adkf_dense_weight_grad(
        g, ldg, x, ldx, dw, M, N, K, scratch, nb, None)
    for kw in (dict(g=None), dict(x=None), dict(dw=None), dict(scratch=None), dict(M=0), dict(N=0), dict(K=0), dict(M=-1), dict(N=-1),
               dict(K=-1), dict(ldg=N - 1), dict(ldx=K - 1)):
        assert call(**kw) == _E_BADARG, kw
    assert call(nb=need - 1) == _E_WORKSPACE and call(nb=0) == _E_WORKSPACE
    for M, N, K in ((1, 1, 1), (4099, 33, 70), (8193, 8, 8)):
        need = lib.adkf_dense_weight_grad_scratch_bytes(M, N, K)
        assert need > 0 and call(M=M, N=N, K=K, ldg=N, ldx=K, nb=need - 1) == _E_WORKSPACE
    for shape in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8), (8, -1, 8), (8, 8, -1)):
        assert lib.adkf_dense_weight_grad_scratch_bytes(*shape) == 0, shape
