"""GPU: every fused GNN kernel ALONE against the float64 reference of the same operation (oracle/gnn_kernel_refs.py), on float32
inputs built on the CPU (tests/gnn_kernel_inputs.py) and promoted to float64 for the reference.  tests/test_gpu_gnn.py reaches
these kernels through whole modules only, under bounds scaled by the largest gradient entry of the extractor; here each output is
held by itself, and the shapes are those at which a kernel takes another path (csrc/pna.h, csrc/block.h, csrc/readout.h).

What is compared how:
  * EXACTLY (``torch.equal``): arg-max ids and the values gathered there, routed gradients, empty segments, masks, x1 of the block
    against the float32 CPU evaluation of the unfused expression, every backward against its second run, the autograd Functions
    against the C entries called directly, ``_MessagePass`` against ``_MessageFunction`` + ``_PNAAggregate``.
  * Rule A - sums of products of the inputs: |got - ref| <= 2 (n + 2) 2^-24 R_abs per element, R_abs the reference on the absolute
    values (cotangent included; before the ReLU), n the number of terms of the longest sum behind the element.  Any float32 summation
    order stays within (n + 2) 2^-24 R_abs; the 2 allows for matrix-pipe accumulators that may not round to nearest.
  * Rule B - outputs behind expf, a division or rsqrtf: a fixed literal per (operation, output), relative to the reference's largest
    entry: 4 x the error of the reference code run in float32 on the CPU on these inputs (profiles/gnn_kernel_yardsticks.json,
    tools/gnn_kernel_yardsticks.py), rounded up to one digit, at least 2^-20.  tests/test_gnn_kernel_refs.py checks the derivation.
  * mean, std and d b of the aggregation come from float64 arithmetic on exact inputs, rounded once: 2^-22.
Every direct call of a C entry pre-fills its outputs with NaN (int32: -7) and none may be left: the wrappers allocate with
``torch.empty``.  No bound is taken from a kernel's output; the measured errors are printed next to the bounds."""
import ctypes as C

import pytest
import torch

import gnn_kernel_inputs as I

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LITERALS = {   # rule B (profiles/gnn_kernel_yardsticks.json: "literals")
    "block": dict(h=1e-6, mu=1e-6, rstd=1e-6, d_p=1e-6, d_x=1e-6, d_bias=1e-6, d_gamma=1e-6, d_beta=1e-6, d_alpha=2e-6),
    "pool": dict(w_mean=1e-6, w_sum=1e-6, g_mean=1e-6, g_sum=1e-6, d_s_mean=5e-6, d_v_mean=1e-6, d_s_sum=2e-6, d_v_sum=1e-6),
    "hidden": dict(w_mean=1e-6, w_sum=1e-6, p_mean=1e-6, p_sum=2e-6, wtot_sum=1e-6, d_s_mean=6e-6, d_h_mean=1e-6, d_s_sum=2e-6, d_h_sum=2e-6),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from adkf_ift_amd import _lib
    return _lib.load()


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _m7(dev, *shape):
    return torch.full(shape, -7, dtype=torch.int32, device=dev)


def _all_written(**outs):
    for name, t in outs.items():
        if t.dtype == torch.int32:
            assert not (t == -7).any(), "%s: an element was never written" % name
        else:
            assert not torch.isnan(t).any(), "%s: an element was never written (or is NaN)" % name


def _ok(rc, what):
    from adkf_ift_amd import _lib
    _lib.check(rc, what)


def _rule_a(got, ref, r_abs, n, what, worst):
    """|got - ref| <= 2 (n + 2) 2^-24 R_abs, element-wise (n a number or a tensor that broadcasts)."""
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 * (torch.as_tensor(n, dtype=torch.float64) + 2.0) * U * r_abs
    ratio = (err / bound.clamp(min=1e-300)).max().item() if err.numel() else 0.0
    worst[what] = max(worst.get(what, 0.0), ratio)
    assert (err <= bound).all(), (what, ratio)


def _rule_b(op, name, got, ref, worst, err=None):
    e = I.rel_err(got.cpu(), ref) if err is None else err
    worst[name] = (e, LITERALS[op][name])
    assert e <= LITERALS[op][name], (op, name, e, LITERALS[op][name])


# ======================================================================================================================
# PNA aggregation
# ======================================================================================================================
@pytest.mark.parametrize("H,m", I.PNA_SHAPES)
def test_pna_aggregate_forward_and_backward(dev, lib, H, m):
    """adkf_pna_aggregate / _backward / _backward_relu on in-degrees 0, 1, 2, 4, 3, 17, 0, 64, 5 with shuffled message ids: segments of
    identical rows (std at its floor), a segment of nearly equal mean-parts (the float64 cancellation), a maximum tied at two list
    positions in three columns (the FIRST in segment order wins), H m = 24, 256, 300 (strided column loop) and 1."""
    from adkf_ift_amd import gnn as G
    from oracle import gnn_kernel_refs as R

    c = I.pna_case(H, m)
    V, E = c["V"], c["msgs"].shape[0]
    perm, rowptr, tg = c["perm"], c["rowptr"], c["tg"]
    m64 = c["msgs"].double().requires_grad_(True)
    ref, am_ref = R.pna_aggregate(m64, perm, rowptr, V)
    d_ref, = torch.autograd.grad(ref, m64, c["d_agg"].double())
    deg = (rowptr[1:] - rowptr[:-1])

    msgs = c["msgs"].to(dev).requires_grad_(True)
    perm_d, rowptr_d, d_agg = perm.to(dev), rowptr.to(dev), c["d_agg"].to(dev)
    agg, argmax = G._PNAAggregate.apply(msgs, perm_d, rowptr_d, V)
    agg2, argmax2 = _nan(dev, V, H, 4 * m), _m7(dev, V, H, m)
    _ok(lib.adkf_pna_aggregate(_p(msgs), _p(perm_d), _p(rowptr_d), V, H, m, _p(agg2), _p(argmax2), _st(dev)), "adkf_pna_aggregate")
    _all_written(agg=agg2, argmax=argmax2)
    assert torch.equal(agg, agg2) and torch.equal(argmax, argmax2)

    got, am = agg.detach().cpu(), argmax.cpu().long()
    assert torch.equal(am, am_ref), "argmax: first maximum in segment order"
    hh, ff = torch.meshgrid(torch.arange(H), torch.arange(m), indexing="ij")
    full = deg > 0
    assert torch.equal(got[full][..., 3 * m:], c["msgs"][am[full], hh, 2 * m + ff]), "max is the gathered message, to the bit"
    assert (got[~full] == 0).all() and (am[~full] == -1).all(), "empty segments: 0 and -1"
    worst = {}
    ref_abs, _ = R.pna_aggregate(c["msgs"].double().abs(), perm, rowptr, V)
    _rule_a(got[..., :m], ref[..., :m].detach(), ref_abs[..., :m], deg.view(V, 1, 1).double(), "sum", worst)
    for name, lo in (("mean", m), ("std", 2 * m)):
        r = ref[..., lo:lo + m].detach()
        e = ((got[..., lo:lo + m].double() - r).abs() / r.abs().clamp(min=1e-300)).max().item()
        worst[name] = e
        assert ((got[..., lo:lo + m].double() - r).abs() <= 2.0 ** -22 * r.abs()).all(), (name, e)
    ids = perm[int(rowptr[2]):int(rowptr[3])]      # identical rows: the floor sqrt(deg 1e-7)
    assert (got[2][..., 2 * m:3 * m].double() - (2 * 1e-7) ** 0.5).abs().max().item() <= 2.0 ** -22 * (2 * 1e-7) ** 0.5 and ids.numel() == 2

    # ---- backward: twice, identical; C entry direct with NaN pre-fill; the ReLU variant is the masked plain one, to the bit
    d1, = torch.autograd.grad(agg, msgs, d_agg, retain_graph=True)
    d2, = torch.autograd.grad(agg, msgs, d_agg, retain_graph=True)
    assert torch.equal(d1, d2)
    d3, d4 = _nan(dev, E, H, 3 * m), _nan(dev, E, H, 3 * m)
    args = (_p(msgs), _p(perm_d), _p(rowptr_d), _p(agg), _p(argmax), _p(d_agg), V, H, m)
    _ok(lib.adkf_pna_aggregate_backward(*args, _p(d3), _st(dev)), "adkf_pna_aggregate_backward")
    _ok(lib.adkf_pna_aggregate_backward_relu(*args, _p(d4), _st(dev)), "adkf_pna_aggregate_backward_relu")
    _all_written(d_msgs=d3, d_pre=d4)
    assert torch.equal(d1, d3)
    assert torch.equal(d4, torch.where(msgs.detach() > 0, d3, torch.zeros_like(d3))), "backward_relu = where(msgs > 0, backward, 0)"
    d = d1.cpu()
    assert torch.equal(d[..., :m], c["d_agg"][tg][..., :m]), "d a_e = d_sum of the target, to the bit"
    want_c = torch.zeros(E, H, m)
    want_c[am[full], hh, ff] = c["d_agg"][full][..., 3 * m:]
    assert torch.equal(d[..., 2 * m:], want_c), "d c_e = d_max at the arg-max message, 0.0 elsewhere"
    rb = d_ref[..., m:2 * m]
    e = (d[..., m:2 * m].double() - rb).abs().max().item() / rb.abs().max().item()
    worst["d_b"] = e
    assert e <= 2.0 ** -22, ("d_b", e)
    print("pna (H=%d, m=%d): sum %.1e of its rule-A bound; mean %.1e, std %.1e (element-wise), d_b %.1e of the largest entry, bound 2^-22 = %.1e"
          % (H, m, worst["sum"], worst["mean"], worst["std"], worst["d_b"], 2.0 ** -22))


# ======================================================================================================================
# message functions
# ======================================================================================================================
def _msg_table(plan, Ws, bs=None, dWs=None, dbs=None):
    from adkf_ift_amd import _lib
    tab = (_lib.MsgEt * len(Ws))()
    for et in range(len(Ws)):
        tab[et].src, tab[et].tgt = plan.srcs[et].data_ptr(), plan.tgts[et].data_ptr()
        tab[et].W = Ws[et].data_ptr()
        tab[et].bias = bs[et].data_ptr() if bs is not None else None
        tab[et].dW = dWs[et].data_ptr() if dWs is not None else None
        tab[et].db = dbs[et].data_ptr() if dbs is not None else None
        tab[et].E = int(plan.srcs[et].shape[0])
    return tab


def _c_msg_backward(lib, dev, x, plan, dims, Ws, msgs, d):
    """adkf_msg_backward with the marshalling of adkf_ift_amd/gnn.py, every output (and the scratch) pre-filled with NaN."""
    H, inn, out = dims
    n_et, E_all, V = len(Ws), d.shape[0], x.shape[0]
    dcat, dx = _nan(dev, E_all, H, 2 * inn), _nan(dev, V, H * inn)
    dWs, dbs = [_nan(dev, *w.shape) for w in Ws], [_nan(dev, H, out) for _ in Ws]
    tab = _msg_table(plan, Ws, None, dWs, dbs)
    need = int(lib.adkf_msg_backward_scratch_bytes(C.cast(tab, C.c_void_p), n_et, H, inn, out))
    scratch = _nan(dev, max(need, 4) // 4)
    _ok(lib.adkf_msg_backward(_p(x), C.cast(tab, C.c_void_p), n_et, H, inn, out, _p(msgs) if msgs is not None else None, _p(d),
                              _p(plan.perm_src), _p(plan.rowptr_src), _p(plan.perm), _p(plan.rowptr), V, _p(dcat), _p(dx), _p(scratch),
                              scratch.numel() * 4, _st(dev)), "adkf_msg_backward")
    _all_written(dcat=dcat, dx=dx, **{"dW%d" % i: w for i, w in enumerate(dWs)}, **{"db%d" % i: b for i, b in enumerate(dbs)})
    return dcat, dx, dWs, dbs


@pytest.mark.parametrize("dims,counts,bidirectional,seed", I.MSG_CASES)
def test_message_functions_forward_and_backward(dev, lib, dims, counts, bidirectional, seed):
    """adkf_msg_forward / adkf_msg_backward: four edge types with an empty one in the middle, one tile plus one edge, two chunks;
    4100 edges (9 chunks: the unrolled-by-8 reduce and its tail); 33000 edges (chunk 544, 61 chunks); scalar and vector operand
    paths; nodes without edges.  msgs, d cat, d x, d W, d b under rule A (n = 2 in + 1 | out | out + degree | E of the type | E of the
    type).  The mask taken inside the entry (``_MessageFunction``) and the gradient masked beforehand (msgs = NULL, as
    ``_MessagePass`` calls it) are each held to the reference and to each other bit for bit; where out is 3 m, ``_MessagePass`` itself
    equals ``_MessageFunction`` + ``_PNAAggregate`` bit for bit, forward and backward."""
    from adkf_ift_amd import gnn as G
    from oracle import gnn_kernel_refs as R

    c = I.msg_case(dims, counts, bidirectional, seed)
    H, inn, out = dims
    plan, E_all, V, n_et = c["plan"], c["E_all"], I.MSG_V, len(counts)
    f64 = lambda ts: [t.double() for t in ts]
    x64, W64, b64, d64 = c["x"].double(), f64(c["Ws"]), f64(c["bs"]), c["d_msgs"].double()
    pre, _ = R.msg_linear(x64, plan.srcs, plan.tgts, W64, b64)
    pre_abs, _ = R.msg_linear(x64.abs(), plan.srcs, plan.tgts, [w.abs() for w in W64], [b.abs() for b in b64])
    ref = R.msg_backward(x64, plan.srcs, plan.tgts, W64, b64, d64, masked=False)
    d_pre_abs = (d64 * (pre > 0)).abs()
    ref_abs = R.msg_backward(x64.abs(), plan.srcs, plan.tgts, [w.abs() for w in W64], [b.abs() for b in b64], d_pre_abs, masked=True)

    pd = plan.to(dev)
    x = c["x"].to(dev).requires_grad_(True)
    Ws = [w.to(dev).requires_grad_(True) for w in c["Ws"]]
    bs = [b.to(dev).requires_grad_(True) for b in c["bs"]]
    d = c["d_msgs"].to(dev)
    msgs = G._MessageFunction.apply(x, pd, H, inn, out, *Ws, *bs)
    msgs2 = _nan(dev, E_all, H, out)
    _ok(lib.adkf_msg_forward(_p(x), C.cast(_msg_table(pd, Ws, bs), C.c_void_p), n_et, H, inn, out, _p(msgs2), _st(dev)), "adkf_msg_forward")
    _all_written(msgs=msgs2)
    assert torch.equal(msgs.detach(), msgs2)
    worst = {}
    got = msgs.detach().cpu()
    _rule_a(got, torch.relu(pre), pre_abs, 2 * inn + 1, "msgs", worst)
    assert torch.equal((got > 0) & c["safe"], (pre > 0) & c["safe"]), "the ReLU mask, away from the kink"

    # ---- backward: the autograd Function twice; the C entry with the mask inside; the C entry with msgs = NULL and the gradient masked here
    g1 = torch.autograd.grad(msgs, [x, *Ws, *bs], d, retain_graph=True)
    g2 = torch.autograd.grad(msgs, [x, *Ws, *bs], d, retain_graph=True)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    md = msgs.detach()
    dcat, dx, dWs, dbs = _c_msg_backward(lib, dev, x.detach(), pd, dims, [w.detach() for w in Ws], md, d)
    d_pre = torch.where(md > 0, d, torch.zeros_like(d))
    dcat0, dx0, dWs0, dbs0 = _c_msg_backward(lib, dev, x.detach(), pd, dims, [w.detach() for w in Ws], None, d_pre)
    for a, b, e in zip((dx, *dWs, *dbs), (dx0, *dWs0, *dbs0), g1):
        assert torch.equal(a, b), "mask inside the entry == gradient masked beforehand (msgs = NULL)"
        assert torch.equal(a, e), "C entry == autograd Function"
    assert torch.equal(dcat, dcat0)
    node_deg = (plan.rowptr_src[1:] - plan.rowptr_src[:-1]) + (plan.rowptr[1:] - plan.rowptr[:-1])
    _rule_a(dcat, ref[0], ref_abs[0], out, "dcat", worst)
    _rule_a(dx, ref[1], ref_abs[1], (out + node_deg).double().view(V, 1), "dx", worst)
    for et in range(n_et):
        E_et = int(plan.srcs[et].shape[0])
        _rule_a(dWs[et], ref[2][et], ref_abs[2][et], E_et, "dW", worst)
        _rule_a(dbs[et], ref[3][et], ref_abs[3][et], E_et, "db", worst)
        if E_et == 0:
            assert (dWs[et] == 0).all() and (dbs[et] == 0).all(), "an edge type without edges: exact zeros"
    assert (dx[node_deg.to(dev) == 0] == 0).all() and (node_deg == 0).sum() >= I.MSG_V - I.MSG_V_USED, "nodes without edges: d x = 0.0"
    print("msg %s E=%s%s: fraction of the rule-A bound used: %s" % (dims, list(counts), " bidirectional" if bidirectional else "",
                                                                    ", ".join("%s %.1e" % kv for kv in worst.items())))

    if out % 3 == 0:   # ``_MessagePass`` (legal where out = 3 m): one node of the graph == the two-node chain, to the bit
        m = out // 3
        d_agg = torch.randn(V, H, 4 * m, generator=torch.Generator().manual_seed(7)).to(dev)
        agg, am, msgs_p = G._MessagePass.apply(x, pd, H, inn, out, *Ws, *bs)
        agg_c, am_c = G._PNAAggregate.apply(msgs, pd.perm, pd.rowptr, V)
        assert torch.equal(msgs_p, md) and torch.equal(agg, agg_c) and torch.equal(am, am_c)
        gp = torch.autograd.grad(agg, [x, *Ws, *bs], d_agg)
        gc = torch.autograd.grad(agg_c, [x, *Ws, *bs], d_agg)
        for a, b in zip(gp, gc):
            assert torch.equal(a, b), "_MessagePass backward == _PNAAggregate backward + _MessageFunction backward"


@pytest.mark.parametrize("fused", [True, False])
def test_a_batch_without_any_edge(dev, fused):
    """Three single-atom graphs: no edge of any type, so every message tensor has zero rows (and a zero address).  The device path
    must give the float64 module's features to 2e-5 and every gradient to 5e-5 of the largest entry (the bounds of
    tests/test_gpu_gnn.py::test_fused_kernels_on_odd_shapes_vs_cpu_float64), through ``_MessagePass`` and through
    ``_MessageFunction`` + ``_PNAAggregate``."""
    from adkf_ift_amd import gnn as G
    from test_gnn import small_cfg

    cfg = small_cfg("PNA")
    gen = torch.Generator().manual_seed(21)
    batch = G.GraphBatch(torch.randn(3, 32, generator=gen, dtype=torch.float64), [torch.zeros(0, 2, dtype=torch.long) for _ in range(3)],
                         torch.arange(3), 3)
    torch.manual_seed(9)
    ref = G.GraphFeatureExtractor(cfg).double()
    with torch.no_grad():
        for blk in ref.gnn.gnn_blocks:
            blk.alpha.fill_(0.6)
    got = G.GraphFeatureExtractor(cfg)
    got.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    got = got.to(dev)
    b32 = batch.to(dev)
    b32.node_features = b32.node_features.float()
    want = ref(batch)
    w = torch.randn(want.shape, dtype=torch.float64, generator=gen)
    (want * w).sum().backward()
    old = G._FUSED_MP
    G._FUSED_MP = fused
    try:
        z = got(b32)
        (z * w.float().to(dev)).sum().backward()
    finally:
        G._FUSED_MP = old
    assert (z.double().cpu() - want).abs().max().item() <= 2e-5 * want.abs().max().item()
    named = dict(got.named_parameters())
    scale = max(p.grad.abs().max().item() for p in ref.parameters() if p.grad is not None)
    for n, p in ref.named_parameters():
        if p.grad is None:
            assert named[n].grad is None, n
            continue
        e = (named[n].grad.double().cpu() - p.grad).abs().max().item() / scale
        assert e <= 5e-5, (n, e)
        if ".mp.weights" in n or ".mp.biases" in n:
            assert (named[n].grad == 0).all(), n


# ======================================================================================================================
# block combine
# ======================================================================================================================
@pytest.mark.parametrize("hid,V,alpha", I.BLOCK_CASES)
def test_block_combine_forward_and_backward(dev, lib, hid, V, alpha):
    """adkf_block_combine / _backward at hid 64 ... 256 (C = 1 ... 4), V = 1, 5, 129 (a second workgroup of the backward with one row),
    1030 (9 workgroups: the unrolled-by-8 reduce and its tail; V % 4 = 2), amplify / attenuate from real degrees with an isolated
    node, a row whose x1 is constant (variance exactly 0; its g_h is scaled by 2^-8 so that its gradients are of the others' size),
    alpha 0.6 and 1e-7.  Per-row outputs are measured in three groups of rows (isolated | constant | rest), each against its own largest entry.  x1 equals the float32 CPU evaluation of the unfused
    expression of adkf_ift_amd/gnn.py::GNNBlock bit for bit (IEEE, no contraction); everything else under rule B, the four reduced
    gradients under the larger of rule B and the summation bound V 2^-24 sum_v |term_v| / max |output| (from the reference)."""
    from adkf_ift_amd import gnn as G

    c = I.block_case(hid, V, alpha)
    ref = I.block_ref(c)
    t = {k: c[k].to(dev) for k in ("p", "x", "amp", "att", "bias", "alpha", "gamma", "beta", "g_x1", "g_h")}
    diff = [t[k].requires_grad_(True) for k in ("p", "x", "bias", "alpha", "gamma", "beta")]
    x1, h = G._BlockCombine.apply(t["p"], t["x"], t["amp"], t["att"], t["bias"], t["alpha"], t["gamma"], t["beta"], c["eps"])
    o = dict(x1=_nan(dev, V, hid), h=_nan(dev, V, hid), mu=_nan(dev, V), rstd=_nan(dev, V))
    _ok(lib.adkf_block_combine(_p(t["p"]), _p(t["x"]), _p(t["amp"]), _p(t["att"]), _p(t["bias"]), _p(t["alpha"]), _p(t["gamma"]), _p(t["beta"]),
                               float(c["eps"]), V, hid, _p(o["x1"]), _p(o["h"]), _p(o["mu"]), _p(o["rstd"]), _st(dev)), "adkf_block_combine")
    _all_written(**o)
    assert torch.equal(x1.detach(), o["x1"]) and torch.equal(h.detach(), o["h"])
    # the unfused float32 expression as GNNBlock.forward writes it, on the CPU
    p32, amp32, att32 = c["p"], c["amp"].unsqueeze(-1), c["att"].unsqueeze(-1)
    new = p32[:, :hid] + amp32 * p32[:, hid:2 * hid] + att32 * p32[:, 2 * hid:] + c["bias"]
    new = c["alpha"] * new
    assert torch.equal(o["x1"].cpu(), c["x"] + new), "x1: the same numbers as the unfused float32 expression"
    if c["const_row"] is not None:
        assert (o["x1"][c["const_row"]] == 1.0).all()
    worst = {}
    for name in ("h", "mu", "rstd"):     # (isolated rows | the constant row | the rest, each against its own largest entry)
        _rule_b("block", name, o[name], ref[name], worst, err=I.block_row_err(c, o[name].cpu(), ref[name]))

    g1 = torch.autograd.grad([x1, h], diff, [t["g_x1"], t["g_h"]], retain_graph=True)
    g2 = torch.autograd.grad([x1, h], diff, [t["g_x1"], t["g_h"]], retain_graph=True)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    b = dict(d_p=_nan(dev, V, 3 * hid), d_x=_nan(dev, V, hid), d_bias=_nan(dev, hid), d_alpha=_nan(dev, 1), d_gamma=_nan(dev, hid), d_beta=_nan(dev, hid))
    need = int(lib.adkf_block_combine_scratch_bytes(V, hid))
    scratch = _nan(dev, need // 4)
    _ok(lib.adkf_block_combine_backward(_p(t["p"]), _p(o["x1"]), _p(t["amp"]), _p(t["att"]), _p(t["bias"]), _p(t["alpha"]), _p(t["gamma"]), _p(o["mu"]),
                                        _p(o["rstd"]), _p(t["g_x1"]), _p(t["g_h"]), V, hid, _p(b["d_p"]), _p(b["d_x"]), _p(b["d_bias"]), _p(b["d_alpha"]),
                                        _p(b["d_gamma"]), _p(b["d_beta"]), _p(scratch), need, _st(dev)), "adkf_block_combine_backward")
    _all_written(**b)
    for a, k in zip(g1, ("d_p", "d_x", "d_bias", "d_alpha", "d_gamma", "d_beta")):
        assert torch.equal(a, b[k]), k
    for name in ("d_p", "d_x"):
        _rule_b("block", name, b[name], ref[name], worst, err=I.block_row_err(c, b[name].cpu(), ref[name]))
    # the reduced gradients: terms of the sums over v, from the reference
    p64, al = c["p"].double(), float(c["alpha"].double())
    new64 = p64[:, :hid] + c["amp"].double().unsqueeze(1) * p64[:, hid:2 * hid] + c["att"].double().unsqueeze(1) * p64[:, 2 * hid:] + c["bias"].double()
    Gt = ref["d_x"]
    xhat = (ref["x1"] - ref["mu"].unsqueeze(1)) * ref["rstd"].unsqueeze(1)
    terms = dict(d_bias=(al * Gt).abs().sum(0), d_gamma=(c["g_h"].double() * xhat).abs().sum(0), d_beta=c["g_h"].double().abs().sum(0),
                 d_alpha=(Gt * new64).abs().sum().view(1))
    for name, tsum in terms.items():
        scale = ref[name].abs().max().item()
        bound = torch.clamp(V * U * tsum / scale, min=LITERALS["block"][name])
        err = (b[name].double().cpu() - ref[name]).abs() / scale
        worst[name] = (err.max().item(), bound[err.argmax()].item())
        assert (err <= bound).all(), (name, err.max().item(), bound.min().item())
    print("block (hid=%d, V=%d, alpha=%g): %s" % (hid, V, alpha, ", ".join("%s %.1e (bound %.0e)" % (k, e, bd) for k, (e, bd) in worst.items())))


# ======================================================================================================================
# read-out pooling
# ======================================================================================================================
def _readout_exact(c, got, ref, dev):
    """What must hold to the bit for both pooling kernels: arg-max (first maximum in node-list order), the gathered maximum, the routed
    gradient, empty graphs."""
    D, perm, rowptr = c["D"], c["perm"], c["rowptr"]
    full = (rowptr[1:] - rowptr[:-1]) > 0
    am = got["argmax"].cpu().long()
    assert torch.equal(am, ref["argmax"]), "argmax: first maximum in node-list order"
    assert torch.equal(got["g_max"].cpu()[full], c["emb"][am[full], torch.arange(D)]), "g_max is the gathered embedding, to the bit"
    assert (got["g_max"].cpu()[~full] == 0).all() and (am[~full] == -1).all() and (~full).sum() == 2, "empty graphs: 0 and -1"
    want = torch.zeros(c["V"], D)
    want[am[full], torch.arange(D)] = c["dg_max"][full]
    assert torch.equal(got["d_emb"].cpu(), want), "d emb = dg_max at the arg-max node, 0.0 elsewhere"
    return full


def _sigmoid_saturates(c, w_sum):
    """Shifted scores (s_sum = 100 u): 1 / (1 + expf(-s)) is EXACTLY 1 from s = 20 on (expf(-20) = 2e-9 < 2^-25 vanishes next to 1) and
    EXACTLY 0 below s = -90 (expf(90) overflows float32 to inf, 1 / inf = 0) - no NaN from inf on the way."""
    s, w = c["s_sum"], w_sum.cpu()
    assert (s >= 20).any() and (s <= -90).any()
    assert (w[s >= 20] == 1).all() and (w[s <= -90] == 0).all(), "the sigmoid saturates to exactly 1 and exactly 0"


@pytest.mark.parametrize("scores", I.SCORES)
@pytest.mark.parametrize("nh,hd,D", I.POOL_SHAPES)
def test_readout_pool_forward_and_backward(dev, lib, nh, hd, D, scores):
    """adkf_readout_pool / _backward on graphs of 0, 1, 3, 64, 65, 130, 4, 0 nodes with interleaved node ids; nh hd = 768, 35, 192, 210,
    hd = 70 (> 64: the strided dot product of the backward), D = 1 ... 300; scores N(0, 1) and (1000 + 30 u | 100 u): the softmax must
    come from shifted exponentials, the sigmoid saturates without a NaN; three embedding columns tie their maximum."""
    from adkf_ift_amd import gnn as G

    c = I.pool_case(nh, hd, D, scores)
    ref = I.pool_ref(c)
    V, Gn, HD = c["V"], c["G"], nh * hd
    names = ("s_mean", "v_mean", "s_sum", "v_sum", "emb")
    t = {k: c[k].to(dev).requires_grad_(True) for k in names}
    n2g, perm, rowptr = c["n2g"].to(dev), c["perm"].to(dev), c["rowptr"].to(dev)
    cot = [c[k].to(dev) for k in ("dg_mean", "dg_sum", "dg_max")]
    outs = G._ReadoutPool.apply(*(t[k] for k in names), n2g, Gn, nh, hd, perm, rowptr)
    g1 = torch.autograd.grad(outs, [t[k] for k in names], cot, retain_graph=True)
    g2 = torch.autograd.grad(outs, [t[k] for k in names], cot, retain_graph=True)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    o = dict(w_mean=_nan(dev, V, nh), w_sum=_nan(dev, V, nh), g_mean=_nan(dev, Gn, HD), g_sum=_nan(dev, Gn, HD), g_max=_nan(dev, Gn, D),
             argmax=_m7(dev, Gn, D))
    _ok(lib.adkf_readout_pool(*(_p(t[k]) for k in names), _p(perm), _p(rowptr), V, Gn, nh, hd, D, _p(o["w_mean"]), _p(o["w_sum"]), _p(o["g_mean"]),
                              _p(o["g_sum"]), _p(o["g_max"]), _p(o["argmax"]), _st(dev)), "adkf_readout_pool")
    _all_written(**o)
    for a, k in zip(outs, ("g_mean", "g_sum", "g_max")):
        assert torch.equal(a.detach(), o[k]), k
    b = dict(d_s_mean=_nan(dev, V, nh), d_v_mean=_nan(dev, V, HD), d_s_sum=_nan(dev, V, nh), d_v_sum=_nan(dev, V, HD), d_emb=_nan(dev, V, D))
    _ok(lib.adkf_readout_pool_backward(_p(t["v_mean"]), _p(t["v_sum"]), _p(o["w_mean"]), _p(o["w_sum"]), _p(o["g_mean"]), _p(o["argmax"]), _p(n2g),
                                       *(_p(x) for x in cot), V, Gn, nh, hd, D, _p(b["d_s_mean"]), _p(b["d_v_mean"]), _p(b["d_s_sum"]),
                                       _p(b["d_v_sum"]), _p(b["d_emb"]), _st(dev)), "adkf_readout_pool_backward")
    _all_written(**b)
    for a, k in zip(g1, ("d_s_mean", "d_v_mean", "d_s_sum", "d_v_sum", "d_emb")):
        assert torch.equal(a, b[k]), k
    got = {**o, **b}
    full = _readout_exact(c, got, ref, dev)
    assert (o["g_mean"].cpu()[~full] == 0).all() and (o["g_sum"].cpu()[~full] == 0).all(), "empty graphs: exact zeros"
    if scores == "shifted":
        _sigmoid_saturates(c, o["w_sum"])
    worst = {}
    for name in I.RULE_B["pool"]:
        _rule_b("pool", name, got[name], ref[name], worst)
    print("readout_pool (nh=%d, hd=%d, D=%d, %s scores): %s" % (nh, hd, D, scores, ", ".join("%s %.1e (bound %.0e)" % (k, e, bd) for k, (e, bd) in worst.items())))


@pytest.mark.parametrize("scores", I.SCORES)
@pytest.mark.parametrize("nh,K,D", I.HIDDEN_SHAPES)
def test_readout_pool_hidden_forward_and_backward(dev, lib, nh, K, D, scores):
    """adkf_readout_pool_hidden / _backward: (HB, KJ) = (12, 3) with the hidden states as column blocks of one [V, 4 K] tensor,
    (12, 2) with nh = 24 - two passes, the ``+=`` of d h -, (4, 4) with D = 2048, (1, 2) with D = 1, (4, 1) with 64 heads; stage
    boundaries at exactly 64 and 65 nodes; both score settings."""
    from adkf_ift_amd import gnn as G

    c = I.hidden_case(nh, K, D, scores)
    ref = I.hidden_ref(c)
    V, Gn = c["V"], c["G"]
    act = c["act"].to(dev)
    if c["strided"]:
        h_mean, h_sum, ldh = act[:, K:2 * K], act[:, 3 * K:], 4 * K
    else:
        h_mean, h_sum, ldh = act[:, K:2 * K].contiguous(), act[:, 3 * K:].contiguous(), K
    t = dict(s_mean=c["s_mean"].to(dev), h_mean=h_mean, s_sum=c["s_sum"].to(dev), h_sum=h_sum, emb=c["emb"].to(dev))
    names = ("s_mean", "h_mean", "s_sum", "h_sum", "emb")
    for k in names:
        t[k].requires_grad_(True)
    perm, rowptr = c["perm"].to(dev), c["rowptr"].to(dev)
    cot = {k: c[k].to(dev) for k in ("dp_mean", "dp_sum", "dwtot_sum", "dg_max")}
    p_mean, p_sum, wt_mean, wt_sum, g_max = G._ReadoutPoolHidden.apply(*(t[k] for k in names), Gn, nh, perm, rowptr)
    diff_out, diff_cot = [p_mean, p_sum, wt_sum, g_max], [cot[k] for k in ("dp_mean", "dp_sum", "dwtot_sum", "dg_max")]
    g1 = torch.autograd.grad(diff_out, [t[k] for k in names], diff_cot, retain_graph=True)
    g2 = torch.autograd.grad(diff_out, [t[k] for k in names], diff_cot, retain_graph=True)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    o = dict(w_mean=_nan(dev, V, nh), w_sum=_nan(dev, V, nh), p_mean=_nan(dev, nh, Gn, K), p_sum=_nan(dev, nh, Gn, K), wtot_mean=_nan(dev, Gn, nh),
             wtot_sum=_nan(dev, Gn, nh), g_max=_nan(dev, Gn, D), argmax=_m7(dev, Gn, D))
    _ok(lib.adkf_readout_pool_hidden(_p(t["s_mean"]), _p(h_mean), _p(t["s_sum"]), _p(h_sum), ldh, _p(t["emb"]), _p(perm), _p(rowptr), V, Gn, nh, K, D,
                                     _p(o["w_mean"]), _p(o["w_sum"]), _p(o["p_mean"]), _p(o["p_sum"]), _p(o["wtot_mean"]), _p(o["wtot_sum"]),
                                     _p(o["g_max"]), _p(o["argmax"]), _st(dev)), "adkf_readout_pool_hidden")
    _all_written(**o)
    for a, k in zip((p_mean, p_sum, wt_mean, wt_sum, g_max), ("p_mean", "p_sum", "wtot_mean", "wtot_sum", "g_max")):
        assert torch.equal(a.detach(), o[k]), k
    b = dict(d_s_mean=_nan(dev, V, nh), d_h_mean=_nan(dev, V, K), d_s_sum=_nan(dev, V, nh), d_h_sum=_nan(dev, V, K), d_emb=_nan(dev, V, D))
    _ok(lib.adkf_readout_pool_hidden_backward(_p(h_mean), _p(h_sum), ldh, _p(o["w_mean"]), _p(o["w_sum"]), _p(o["argmax"]), _p(perm), _p(rowptr),
                                              _p(cot["dp_mean"]), _p(cot["dp_sum"]), _p(cot["dwtot_sum"]), _p(cot["dg_max"]), V, Gn, nh, K, D,
                                              _p(b["d_s_mean"]), _p(b["d_h_mean"]), _p(b["d_s_sum"]), _p(b["d_h_sum"]), _p(b["d_emb"]), _st(dev)),
        "adkf_readout_pool_hidden_backward")
    _all_written(**b)
    for a, k in zip(g1, ("d_s_mean", "d_h_mean", "d_s_sum", "d_h_sum", "d_emb")):
        assert torch.equal(a, b[k]), k
    got = {**o, **b}
    full = _readout_exact(c, got, ref, dev)
    assert torch.equal(o["wtot_mean"].cpu(), full.float().view(Gn, 1).expand(Gn, nh)), "wtot_mean is 1 (0: empty graph)"
    for k in ("p_mean", "p_sum"):
        assert (o[k].cpu()[:, ~full] == 0).all(), "empty graphs: exact zeros"
    assert (o["wtot_sum"].cpu()[~full] == 0).all()
    if scores == "shifted":
        _sigmoid_saturates(c, o["w_sum"])
    worst = {}
    for name in I.RULE_B["hidden"]:
        _rule_b("hidden", name, got[name], ref[name], worst)
    print("readout_pool_hidden (nh=%d, K=%d, D=%d, %s scores): %s" % (nh, K, D, scores, ", ".join("%s %.1e (bound %.0e)" % (k, e, bd) for k, (e, bd) in worst.items())))
