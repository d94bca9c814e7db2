"""Seeded float32 inputs of the per-kernel GNN tests, built on the CPU.  tests/test_gpu_gnn_kernels.py runs the kernels on them,
tests/test_gnn_kernel_refs.py checks (without a GPU) that they have the properties the exact comparisons of the GPU test rely on,
and tools/gnn_kernel_yardsticks.py measures the float32 yardsticks of profiles/gnn_kernel_yardsticks.json on them."""
import functools
import math

import torch

from adkf_ift_amd.gnn import _GraphPlan

# ---- PNA aggregation -------------------------------------------------------------------------------------------------
PNA_SHAPES = [(4, 6), (4, 64), (3, 100), (1, 1)]            # (H, m): 24, exactly 256, 300 (> 256: the strided loop) and 1 columns
PNA_DEGREES = [0, 1, 2, 4, 3, 17, 0, 64, 5]                  # E = 96
PNA_IDENTICAL, PNA_NEAR_EQUAL, PNA_TIED = (2, 3), 5, 7       # segments of identical rows | b (1 + 1e-4 u) | a tied maximum
PNA_TIE_POS = (9, 40)                                        # positions in segment order that share the maximum


def pna_tie_columns(H, m):
    return sorted({(0, 0), (H // 2, m // 2), (H - 1, m - 1)})


@functools.lru_cache(maxsize=None)
def pna_case(H, m, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    V, E = len(PNA_DEGREES), sum(PNA_DEGREES)
    tg = torch.repeat_interleave(torch.arange(V), torch.tensor(PNA_DEGREES))[torch.randperm(E, generator=g)]   # message id -> target
    perm = torch.argsort(tg.double() + 0.5 * torch.rand(E, generator=g, dtype=torch.float64))   # by target; inside a segment NOT by id
    rowptr = torch.cat((torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(tg, minlength=V), 0)))
    seg = lambda v: perm[int(rowptr[v]):int(rowptr[v + 1])]
    x = torch.randn(E, H, 3 * m, generator=g)
    msgs = torch.relu(x)                                     # ReLU outputs: about half the entries are exactly 0
    hh, ff = torch.meshgrid(torch.arange(H), torch.arange(m), indexing="ij")
    for v in range(V):                                       # one strictly largest, positive entry per segment and max-column (gap >= 0.1)
        ids = seg(v)
        if ids.numel():
            c = x[ids][..., 2 * m:]
            msgs[ids[c.argmax(0)], hh, 2 * m + ff] = c.max(0).values.abs() + 0.1
    for v in PNA_IDENTICAL:                                  # identical rows: std at its floor sqrt(deg 1e-7), the maximum tied throughout
        msgs[seg(v)] = msgs[seg(v)[0]].clone()
    ids = seg(PNA_NEAR_EQUAL)                                # nearly equal mean-parts: b^2 - mean^2 cancels to ~1e-4 b^2
    b0 = 0.5 + torch.rand(H, m, generator=g, dtype=torch.float64)
    u = 2.0 * torch.rand(ids.numel(), H, m, generator=g, dtype=torch.float64) - 1.0
    msgs[ids, :, m:2 * m] = (b0 * (1.0 + 1e-4 * u)).float()
    ids = seg(PNA_TIED)                                      # the same positive maximum at two positions of the list, the EARLIER one with
    a, b = int(rowptr[PNA_TIED]) + PNA_TIE_POS[0], int(rowptr[PNA_TIED]) + PNA_TIE_POS[1]   # the larger id: "first in segment order"
    if perm[a] < perm[b]:                                    # is then not "smallest message id"
        perm[[a, b]] = perm[[b, a]]
    ids = seg(PNA_TIED)
    for h, f in pna_tie_columns(H, m):
        top = msgs[ids, h, 2 * m + f].max() + 1.0
        msgs[ids[PNA_TIE_POS[0]], h, 2 * m + f] = top
        msgs[ids[PNA_TIE_POS[1]], h, 2 * m + f] = top
    d_agg = torch.randn(V, H, 4 * m, generator=g)
    return dict(msgs=msgs, perm=perm, rowptr=rowptr, tg=tg, V=V, H=H, m=m, d_agg=d_agg)


# ---- message functions -----------------------------------------------------------------------------------------------
MSG_V, MSG_V_USED = 50, 40                                   # nodes 40 ... 49 carry no edge
MSG_CASES = [   # (H, in, out), edges per type, bidirectional, seed
    ((4, 4, 18), (1, 0, 65, 513), False, 0),                 # out % 4 != 0: scalar operand loads
    ((3, 5, 7), (1, 0, 65, 513), False, 0),                  # in % 4 != 0 too
    ((4, 32, 192), (1, 0, 65, 513), False, 0),               # the default width
    ((2, 36, 68), (1, 0, 65, 513), False, 0),                # vector loads, partial tiles in both N extents, contraction 72
    ((3, 5, 7), (1, 0, 65, 513), True, 1),                   # flipped copies appended (twice the edges)
    ((3, 5, 7), (4100,), False, 0),                          # 9 chunks: the unrolled reduce and its tail
    ((4, 4, 18), (4100,), False, 0),
    ((3, 5, 7), (33000, 0, 63), False, 0),                   # chunk 544, 61 chunks
]


@functools.lru_cache(maxsize=None)
def msg_case(dims, counts, bidirectional, seed=0):
    H, inn, out = dims
    g = torch.Generator().manual_seed(200 + seed)
    adj = [torch.randint(0, MSG_V_USED, (E, 2), generator=g) for E in counts]
    plan = _GraphPlan(adj, MSG_V, bidirectional, True)
    E_all = int(plan.all_tgts.shape[0])
    x = torch.randn(MSG_V, H * inn, generator=g)
    Ws = [torch.randn(H, 2 * inn, out, generator=g) / math.sqrt(2 * inn) for _ in counts]
    bs = [0.1 * torch.randn(H, out, generator=g) for _ in counts]
    d_msgs = torch.randn(E_all, H, out, generator=g)
    # Where a pre-activation is closer to zero than rule A allows the kernel's own value to be off (2 (n + 2) 2^-24 R_abs, n = 2 in + 1),
    # float32 rounding may legitimately put the entry on the other side of the ReLU: the cotangent is zero there, so that no
    # gradient depends on the mask at such an entry (a few entries in 1e5).
    from oracle import gnn_kernel_refs as R
    f64 = lambda ts: [t.double() for t in ts]
    pre, _ = R.msg_linear(x.double(), plan.srcs, plan.tgts, f64(Ws), f64(bs))
    pre_abs, _ = R.msg_linear(x.double().abs(), plan.srcs, plan.tgts, [w.abs() for w in f64(Ws)], [b.abs() for b in f64(bs)])
    safe = pre.abs() > 2.0 * (2 * inn + 3) * 2.0 ** -24 * pre_abs
    d_msgs = d_msgs * safe
    return dict(plan=plan, x=x, Ws=Ws, bs=bs, d_msgs=d_msgs, dims=dims, E_all=E_all, safe=safe)


# ---- block combine ---------------------------------------------------------------------------------------------------
BLOCK_CASES = [(64, 1, 0.6), (192, 5, 0.6), (256, 129, 0.6), (128, 1030, 0.6), (256, 1030, 0.6), (192, 5, 1e-7)]   # (hid, V, alpha)
BLOCK_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def block_case(hid, V, alpha, seed=0):
    g = torch.Generator().manual_seed(300 + seed)
    # degrees from a random graph over the nodes 0 ... V - 2: node V - 1 is isolated (amplify 0, attenuate 1.15e7)
    adj = [torch.randint(0, V - 1, (2 * V, 2), generator=g)] if V > 1 else [torch.zeros(0, 2, dtype=torch.long)]
    plan = _GraphPlan(adj, V, True, True)
    amp, att = plan.amplify.reshape(-1).clone(), plan.attenuate.reshape(-1).clone()
    p = torch.randn(V, 3 * hid, generator=g)
    p[amp == 0] = 0.0                                        # a node without incoming messages has zero aggregates, hence a zero p row
    bias = torch.round(torch.randn(hid, generator=g) * 256.0) / 256.0     # multiples of 2^-8: -bias + bias is exactly 0
    x = torch.randn(V, hid, generator=g)
    const_row = 1 if V >= 3 else None
    if const_row is not None:                                # new = 0 and x1 = 1 in every column, for every alpha: sums of ones are exact
        x[const_row] = 1.0                                   # in any order, so the variance is exactly 0 on both sides and h = beta
        p[const_row] = 0.0
        p[const_row, :hid] = -bias
    gamma = 1.0 + 0.1 * torch.randn(hid, generator=g)
    beta = 0.1 * torch.randn(hid, generator=g)
    g_x1, g_h = torch.randn(V, hid, generator=g), torch.randn(V, hid, generator=g)
    if const_row is not None:                                # rstd of that row is 1 / sqrt(eps) = 316: with g_h of the usual size its d x, d p and
        g_h[const_row] *= 2.0 ** -8                          # its share of d bias would be 300 x every other row's and set the scale of those outputs
    return dict(p=p, x=x, amp=amp, att=att, bias=bias, alpha=torch.tensor([alpha]), gamma=gamma, beta=beta, eps=BLOCK_EPS,
                g_x1=g_x1, g_h=g_h, const_row=const_row, isolated=(amp == 0))


# ---- read-out pooling ------------------------------------------------------------------------------------------------
READOUT_SIZES = [0, 1, 3, 64, 65, 130, 4, 0]                 # empty graphs first and last; a staging boundary at exactly 64 and 65 nodes
READOUT_TIED_GRAPH, READOUT_TIE_POS = 5, (20, 100)
POOL_SHAPES = [(12, 64, 300), (5, 7, 40), (64, 3, 1), (3, 70, 17)]                                  # (nh, hd, D)
HIDDEN_SHAPES = [(12, 768, 1408), (24, 257, 300), (8, 1000, 2048), (5, 300, 1), (64, 64, 40)]       # (nh, K, D)
SCORES = ["normal", "shifted"]


def readout_tie_columns(D):
    return sorted({0, D // 2, D - 1})


def _readout_nodes(g):
    G = len(READOUT_SIZES)
    n2g = torch.repeat_interleave(torch.arange(G), torch.tensor(READOUT_SIZES))
    n2g = n2g[torch.randperm(n2g.numel(), generator=g)]      # node ids interleaved across graphs
    perm = torch.argsort(n2g.double() + 0.5 * torch.rand(n2g.numel(), generator=g, dtype=torch.float64))   # inside a graph NOT by id
    rowptr = torch.cat((torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(n2g, minlength=G), 0)))
    return n2g, perm, rowptr


def _readout_common(g, nh, D, scores):
    n2g, perm, rowptr = _readout_nodes(g)
    V, G = n2g.numel(), len(READOUT_SIZES)
    u1, u2 = torch.randn(V, nh, generator=g), torch.randn(V, nh, generator=g)
    s_mean, s_sum = (u1, u2) if scores == "normal" else (1000.0 + 30.0 * u1, 100.0 * u2)
    emb = torch.randn(V, D, generator=g)
    a, b = int(rowptr[READOUT_TIED_GRAPH]) + READOUT_TIE_POS[0], int(rowptr[READOUT_TIED_GRAPH]) + READOUT_TIE_POS[1]
    if perm[a] < perm[b]:                                    # the earlier tied node has the larger id: "first in list order" != "smallest id"
        perm[[a, b]] = perm[[b, a]]
    ids = perm[int(rowptr[READOUT_TIED_GRAPH]):int(rowptr[READOUT_TIED_GRAPH + 1])]
    for c in readout_tie_columns(D):
        top = emb[ids, c].max() + 1.0
        emb[ids[READOUT_TIE_POS[0]], c] = top
        emb[ids[READOUT_TIE_POS[1]], c] = top
    return dict(n2g=n2g, perm=perm, rowptr=rowptr, V=V, G=G, s_mean=s_mean, s_sum=s_sum, emb=emb, dg_max=torch.randn(G, D, generator=g))


@functools.lru_cache(maxsize=None)
def pool_case(nh, hd, D, scores, seed=0):
    g = torch.Generator().manual_seed(400 + seed)
    c = _readout_common(g, nh, D, scores)
    V, G = c["V"], c["G"]
    c.update(nh=nh, hd=hd, D=D, v_mean=torch.randn(V, nh * hd, generator=g), v_sum=torch.randn(V, nh * hd, generator=g),
             dg_mean=torch.randn(G, nh * hd, generator=g), dg_sum=torch.randn(G, nh * hd, generator=g))
    return c


@functools.lru_cache(maxsize=None)
def hidden_case(nh, K, D, scores, seed=0):
    g = torch.Generator().manual_seed(500 + seed)
    c = _readout_common(g, nh, D, scores)
    V, G = c["V"], c["G"]
    act = torch.relu(torch.randn(V, 4 * K, generator=g))     # the read-out's first layer: [mean.score | mean.value | sum.score | sum.value]
    # K = 768 goes to the kernel as column blocks of the one activation tensor (row stride 4 K, no copies): the GPU test slices ``act``
    c.update(nh=nh, K=K, D=D, act=act, strided=(K == 768), h_mean=act[:, K:2 * K], h_sum=act[:, 3 * K:], dp_mean=torch.randn(nh, G, K, generator=g),
             dp_sum=torch.randn(nh, G, K, generator=g), dwtot_sum=torch.randn(G, nh, generator=g))
    return c


# ---- the references of oracle/gnn_kernel_refs.py on these cases, forward and backward, as {output name: tensor} -----------------
# dtype = float64: what the GPU test compares with.  dtype = float32: the same code on the same inputs - the yardstick E32 of rule B.
def block_ref(c, dtype=torch.float64):
    from oracle import gnn_kernel_refs as R
    names = ("p", "x", "amp", "att", "bias", "alpha", "gamma", "beta")
    t = {k: c[k].to(dtype).requires_grad_(k not in ("amp", "att")) for k in names}
    x1, h, mu, rstd = R.block_combine(*(t[k] for k in names), c["eps"])
    torch.autograd.backward([x1, h], [c["g_x1"].to(dtype), c["g_h"].to(dtype)])
    out = dict(x1=x1, h=h, mu=mu, rstd=rstd, d_p=t["p"].grad, d_x=t["x"].grad, d_bias=t["bias"].grad, d_gamma=t["gamma"].grad,
               d_beta=t["beta"].grad, d_alpha=t["alpha"].grad)
    return {k: v.detach() for k, v in out.items()}


def pool_ref(c, dtype=torch.float64):
    from oracle import gnn_kernel_refs as R
    names = ("s_mean", "v_mean", "s_sum", "v_sum", "emb")
    t = {k: c[k].to(dtype).requires_grad_(True) for k in names}
    g_mean, g_sum, g_max, argmax, w_mean, w_sum = R.readout_pool(*(t[k] for k in names), c["perm"], c["rowptr"], c["nh"], c["hd"])
    torch.autograd.backward([g_mean, g_sum, g_max], [c["dg_mean"].to(dtype), c["dg_sum"].to(dtype), c["dg_max"].to(dtype)])
    out = dict(g_mean=g_mean, g_sum=g_sum, g_max=g_max, argmax=argmax, w_mean=w_mean, w_sum=w_sum,
               **{"d_" + k: t[k].grad for k in names})
    return {k: v.detach() for k, v in out.items()}


def hidden_ref(c, dtype=torch.float64):
    from oracle import gnn_kernel_refs as R
    names = ("s_mean", "h_mean", "s_sum", "h_sum", "emb")
    t = {k: c[k].to(dtype).contiguous().requires_grad_(True) for k in names}
    p_mean, p_sum, wtot_mean, wtot_sum, g_max, argmax, w_mean, w_sum = R.readout_pool_hidden(*(t[k] for k in names), c["perm"], c["rowptr"], c["nh"])
    torch.autograd.backward([p_mean, p_sum, wtot_sum, g_max],
                            [c["dp_mean"].to(dtype), c["dp_sum"].to(dtype), c["dwtot_sum"].to(dtype), c["dg_max"].to(dtype)])
    out = dict(p_mean=p_mean, p_sum=p_sum, wtot_mean=wtot_mean, wtot_sum=wtot_sum, g_max=g_max, argmax=argmax, w_mean=w_mean, w_sum=w_sum,
               **{"d_" + k: t[k].grad for k in names})
    return {k: v.detach() for k, v in out.items()}


# outputs held to a rule-B literal, per operation (the others are compared exactly)
RULE_B = {"block": ("h", "mu", "rstd", "d_p", "d_x", "d_bias", "d_gamma", "d_beta", "d_alpha"),
          "pool": ("w_mean", "w_sum", "g_mean", "g_sum", "d_s_mean", "d_v_mean", "d_s_sum", "d_v_sum"),
          "hidden": ("w_mean", "w_sum", "p_mean", "p_sum", "wtot_sum", "d_s_mean", "d_h_mean", "d_s_sum", "d_h_sum")}


def rel_err(got, ref):
    """Largest |got - ref| relative to the largest |ref| entry (0 where the reference is all zeros and so is ``got``)."""
    scale = ref.abs().max().item() if ref.numel() else 0.0
    err = (got.double() - ref.double()).abs().max().item() if ref.numel() else 0.0
    return err / scale if scale > 0 else err


BLOCK_PER_ROW = ("h", "mu", "rstd", "d_p", "d_x")          # outputs with one row per node


def block_row_err(c, got, ref):
    """Per-row outputs of the block are measured in three groups of rows, each against its own largest entry: the isolated nodes
    (attenuate 1.15e7: their d p is 1e7 x the others'), the row of constant x1 (rstd = 316 against ~1) and all the rest - one
    such row must not set the scale for the others."""
    iso = c["isolated"].clone()
    const = torch.zeros_like(iso)
    if c["const_row"] is not None:
        const[c["const_row"]] = True
        iso[c["const_row"]] = False
    return max(rel_err(got[g], ref[g]) for g in (iso, const, ~(iso | const)) if g.any())


def literal_for(e32):
    """Rule B: 4 x E32 rounded UP to one significant digit, never below 2^-20."""
    v = max(4.0 * e32, 2.0 ** -20)
    e = math.floor(math.log10(v))
    return max(math.ceil(v / 10.0 ** e - 1e-9) * 10.0 ** e, 2.0 ** -20)
