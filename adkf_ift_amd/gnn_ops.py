"""GNN operators on the HIP library: thin torch-tensor front end of the GNN entries of include/adkf_gp.h (csrc/pna.h, csrc/block.h,
csrc/readout.h), the counterpart of ``gp_ops.py``.

One plain function per C entry: float32 / integer tensors on one ROCm device in, freshly allocated tensors out.  They know nothing of
autograd (``gnn.py`` holds the ``torch.autograd.Function``s that call them), check nothing the entries do not check themselves and
expect contiguous tensors unless a row stride is passed.  There is no fallback: a missing library raises.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import ptr, stream


def _addr(t: torch.Tensor):
    """Device address of ``t`` for a C entry.  A tensor without elements (the message list of a batch without a single edge, or
    of single-atom graphs only) has the address 0, which the entries reject as a missing argument: such a list is passed as one
    unused row instead - the kernels read nothing of it (every segment is empty) and still write what belongs to the nodes."""
    if t.numel() == 0:
        t = t.new_empty((1,) + tuple(t.shape[1:]))
    return C.c_void_p(t.data_ptr())


def msg_table(plan, weights, biases=None, dWs=None, dbs=None):
    """The ``adkf_msg_et_t`` array of the message entries: one row per edge type.  The caller keeps it alive across the call."""
    n_et = len(weights)
    tab = (_lib.MsgEt * n_et)()
    for et in range(n_et):
        tab[et].src, tab[et].tgt = plan.srcs[et].data_ptr(), plan.tgts[et].data_ptr()
        tab[et].W = weights[et].data_ptr()
        tab[et].bias = biases[et].data_ptr() if biases is not None else None
        tab[et].dW = dWs[et].data_ptr() if dWs is not None else None
        tab[et].db = dbs[et].data_ptr() if dbs is not None else None
        tab[et].E = int(plan.srcs[et].shape[0])
    return tab


def msg_forward(x, plan, H, in_dim, out_dim, weights, biases):
    """relu(cat(x[src], x[tgt]) W_et + b_et) for every edge type and tower -> msgs [E_all, H, out] (``adkf_msg_forward``: ONE
    launch for all edge types).  x [V, H*in]; weights[et] [H, 2 in, out], biases[et] [H, out]."""
    lib = _lib.load()
    n_et = len(weights)
    E_all = int(plan.all_tgts.shape[0])
    msgs = torch.empty(E_all, H, out_dim, dtype=torch.float32, device=x.device)
    tab = msg_table(plan, weights, biases)
    _lib.check(lib.adkf_msg_forward(ptr(x), C.cast(tab, C.c_void_p), n_et, H, in_dim, out_dim, _addr(msgs), stream(x.device)),
               "adkf_msg_forward")
    return msgs


def msg_backward(x, plan, H, in_dim, out_dim, weights, msgs, d):
    """Backward of ``msg_forward`` (``adkf_msg_backward``) -> (dx, dW list, db list).  With ``msgs`` given, ``d`` is the gradient
    behind the messages' ReLU and ``msgs`` supplies the mask; with ``msgs=None``, ``d`` is already the gradient in front of it."""
    lib = _lib.load()
    n_et, dev = len(weights), x.device
    E_all = int(plan.all_tgts.shape[0])
    # no floating-point atomics anywhere (csrc/pna.h): d cat is written once per edge and d x gathered over each node's
    # edge lists; d W / d b are per-chunk partials summed in a fixed order - every output element is written, none pre-filled
    dcat = torch.empty(E_all, H, 2 * in_dim, dtype=torch.float32, device=dev)
    dW_all = [torch.empty_like(w) for w in weights]
    db_all = torch.empty(n_et, H, out_dim, dtype=torch.float32, device=dev)
    dbs = [db_all[et] for et in range(n_et)]
    tab = msg_table(plan, weights, None, dW_all, dbs)
    need = int(lib.adkf_msg_backward_scratch_bytes(C.cast(tab, C.c_void_p), n_et, H, in_dim, out_dim))
    scratch = torch.empty(max(need, 4) // 4, dtype=torch.float32, device=dev)
    dx = torch.empty_like(x)
    _lib.check(lib.adkf_msg_backward(ptr(x), C.cast(tab, C.c_void_p), n_et, H, in_dim, out_dim, None if msgs is None else _addr(msgs),
                                     _addr(d), _addr(plan.perm_src), ptr(plan.rowptr_src), _addr(plan.perm), ptr(plan.rowptr), x.shape[0],
                                     _addr(dcat), ptr(dx), ptr(scratch), scratch.numel() * 4, stream(dev)), "adkf_msg_backward")
    return dx, dW_all, dbs


def pna_aggregate(msgs, perm, rowptr, V):
    """[E, H, 3m] messages -> agg [V, H, 4m] (sum | mean | std | max) and the arg-max message ids [V, H, m] int32
    (``adkf_pna_aggregate``); ``perm`` / ``rowptr``: the messages by target node."""
    lib = _lib.load()
    E, H, m3 = msgs.shape
    m = m3 // 3
    agg = torch.empty(V, H, 4 * m, dtype=torch.float32, device=msgs.device)
    argmax = torch.empty(V, H, m, dtype=torch.int32, device=msgs.device)
    _lib.check(lib.adkf_pna_aggregate(_addr(msgs), _addr(perm), ptr(rowptr), V, H, m, ptr(agg), ptr(argmax), stream(msgs.device)),
               "adkf_pna_aggregate")
    return agg, argmax


def pna_aggregate_backward(msgs, perm, rowptr, agg, argmax, d_agg, relu=False):
    """Backward of ``pna_aggregate`` -> d_msgs [E, H, 3m]; ``relu=True``: the gradient in front of the messages' ReLU instead
    (``adkf_pna_aggregate_backward_relu``), which ``msg_backward`` takes with ``msgs=None``."""
    lib = _lib.load()
    V, H, m4 = agg.shape
    d_msgs = torch.empty_like(msgs)
    name = "adkf_pna_aggregate_backward_relu" if relu else "adkf_pna_aggregate_backward"
    _lib.check(getattr(lib, name)(_addr(msgs), _addr(perm), ptr(rowptr), ptr(agg), ptr(argmax), ptr(d_agg), V, H, m4 // 4,
                                  _addr(d_msgs), stream(msgs.device)), name)
    return d_msgs


def block_combine(p, x, amp, att, bias, alpha, gamma, beta, eps):
    """new = p0 + amp p1 + att p2 + bias;  x1 = x + alpha new;  h = LayerNorm(x1)  ->  (x1, h, mu, rstd) with the row statistics of
    the layer norm (``adkf_block_combine``, csrc/block.h).  p [V, 3 hid], x [V, hid]."""
    lib = _lib.load()
    V, hid = x.shape
    x1, h = torch.empty_like(x), torch.empty_like(x)
    mu = torch.empty(V, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mu)
    _lib.check(lib.adkf_block_combine(ptr(p), ptr(x), ptr(amp), ptr(att), ptr(bias), ptr(alpha), ptr(gamma), ptr(beta), float(eps), V, hid,
                                      ptr(x1), ptr(h), ptr(mu), ptr(rstd), stream(x.device)), "adkf_block_combine")
    return x1, h, mu, rstd


def block_combine_backward(p, x1, amp, att, bias, alpha, gamma, mu, rstd, g_x1, g_h):
    """Backward of ``block_combine`` -> (d_p, d_x, d_bias, d_alpha, d_gamma, d_beta) (``adkf_block_combine_backward``)."""
    lib = _lib.load()
    V, hid = x1.shape
    dev = x1.device
    d_p, d_x = torch.empty_like(p), torch.empty_like(x1)
    d_bias, d_gamma, d_beta, d_alpha = torch.empty_like(bias), torch.empty_like(gamma), torch.empty_like(gamma), torch.empty_like(alpha)
    need = int(lib.adkf_block_combine_scratch_bytes(V, hid))
    scratch = torch.empty(need // 4, dtype=torch.float32, device=dev)
    _lib.check(lib.adkf_block_combine_backward(ptr(p), ptr(x1), ptr(amp), ptr(att), ptr(bias), ptr(alpha), ptr(gamma), ptr(mu), ptr(rstd),
                                               ptr(g_x1), ptr(g_h), V, hid, ptr(d_p), ptr(d_x), ptr(d_bias), ptr(d_alpha), ptr(d_gamma),
                                               ptr(d_beta), ptr(scratch), need, stream(dev)), "adkf_block_combine_backward")
    return d_p, d_x, d_bias, d_alpha, d_gamma, d_beta


def readout_pool(s_mean, v_mean, s_sum, v_sum, emb, perm, rowptr, G, nh, hd):
    """Per-graph segment softmax + weighted mean, sigmoid-weighted sum and max in ONE kernel (``adkf_readout_pool``,
    csrc/readout.h) -> (w_mean, w_sum [V, nh], g_mean, g_sum [G, nh hd], g_max [G, D], argmax [G, D] int32); ``perm`` / ``rowptr``:
    the nodes by graph."""
    lib = _lib.load()
    dev = emb.device
    V, D = emb.shape
    f32 = dict(dtype=torch.float32, device=dev)
    w_mean, w_sum = torch.empty(V, nh, **f32), torch.empty(V, nh, **f32)
    g_mean, g_sum, g_max = torch.empty(G, nh * hd, **f32), torch.empty(G, nh * hd, **f32), torch.empty(G, D, **f32)
    argmax = torch.empty(G, D, dtype=torch.int32, device=dev)
    _lib.check(lib.adkf_readout_pool(ptr(s_mean), ptr(v_mean), ptr(s_sum), ptr(v_sum), ptr(emb), ptr(perm), ptr(rowptr), V, G, nh, hd, D,
                                     ptr(w_mean), ptr(w_sum), ptr(g_mean), ptr(g_sum), ptr(g_max), ptr(argmax), stream(dev)), "adkf_readout_pool")
    return w_mean, w_sum, g_mean, g_sum, g_max, argmax


def readout_pool_backward(v_mean, v_sum, w_mean, w_sum, g_mean, argmax, n2g, dg_mean, dg_sum, dg_max, dims):
    """Backward of ``readout_pool`` -> (d_s_mean, d_v_mean, d_s_sum, d_v_sum, d_emb); ``dims = (V, G, nh, hd, D)``."""
    lib = _lib.load()
    V, G, nh, hd, D = dims
    dev = v_mean.device
    f32 = dict(dtype=torch.float32, device=dev)
    d_s_mean, d_s_sum = torch.empty(V, nh, **f32), torch.empty(V, nh, **f32)
    d_v_mean, d_v_sum, d_emb = torch.empty(V, nh * hd, **f32), torch.empty(V, nh * hd, **f32), torch.empty(V, D, **f32)
    _lib.check(lib.adkf_readout_pool_backward(ptr(v_mean), ptr(v_sum), ptr(w_mean), ptr(w_sum), ptr(g_mean), ptr(argmax), ptr(n2g),
                                              ptr(dg_mean), ptr(dg_sum), ptr(dg_max), V, G, nh, hd, D, ptr(d_s_mean), ptr(d_v_mean),
                                              ptr(d_s_sum), ptr(d_v_sum), ptr(d_emb), stream(dev)), "adkf_readout_pool_backward")
    return d_s_mean, d_v_mean, d_s_sum, d_v_sum, d_emb


def shared_row_stride(h_mean, h_sum):
    """``h_mean`` / ``h_sum`` [V, K] as ``readout_pool_hidden`` takes them, and their common row stride ``ldh``: column blocks of one
    activation tensor pass as they are (no copies); blocks that do not share a row stride are made contiguous.  A single row has no
    stride to speak of: ``K``."""
    if h_mean.stride(1) != 1 or h_sum.stride(1) != 1 or h_mean.stride(0) != h_sum.stride(0):
        h_mean, h_sum = h_mean.contiguous(), h_sum.contiguous()
    return h_mean, h_sum, (h_mean.stride(0) if h_mean.shape[0] > 1 else h_mean.shape[1])


def readout_pool_hidden(s_mean, h_mean, s_sum, h_sum, ldh, emb, perm, rowptr, G, nh):
    """The pooling of ``readout_pool`` taken BEFORE the last layer of the two value MLPs (``adkf_readout_pool_hidden``,
    csrc/readout.h) -> (w_mean, w_sum [V, nh], p_mean, p_sum [nh, G, K], wtot_mean, wtot_sum [G, nh], g_max [G, D], argmax);
    ``h_mean`` / ``h_sum`` [V, K] with row stride ``ldh`` (``shared_row_stride``)."""
    lib = _lib.load()
    dev = emb.device
    (V, D), K = emb.shape, h_mean.shape[1]
    f32 = dict(dtype=torch.float32, device=dev)
    w_mean, w_sum = torch.empty(V, nh, **f32), torch.empty(V, nh, **f32)
    p_mean, p_sum = torch.empty(nh, G, K, **f32), torch.empty(nh, G, K, **f32)
    wtot_mean, wtot_sum = torch.empty(G, nh, **f32), torch.empty(G, nh, **f32)
    g_max, argmax = torch.empty(G, D, **f32), torch.empty(G, D, dtype=torch.int32, device=dev)
    _lib.check(lib.adkf_readout_pool_hidden(ptr(s_mean), ptr(h_mean), ptr(s_sum), ptr(h_sum), ldh, ptr(emb), ptr(perm), ptr(rowptr), V, G, nh,
                                            K, D, ptr(w_mean), ptr(w_sum), ptr(p_mean), ptr(p_sum), ptr(wtot_mean), ptr(wtot_sum), ptr(g_max),
                                            ptr(argmax), stream(dev)), "adkf_readout_pool_hidden")
    return w_mean, w_sum, p_mean, p_sum, wtot_mean, wtot_sum, g_max, argmax


def readout_pool_hidden_backward(h_mean, h_sum, w_mean, w_sum, argmax, perm, rowptr, dp_mean, dp_sum, dwtot_sum, dg_max, dims):
    """Backward of ``readout_pool_hidden`` -> (d_s_mean, d_h_mean, d_s_sum, d_h_sum, d_emb); ``dims = (V, G, nh, K, D, ldh)``."""
    lib = _lib.load()
    V, G, nh, K, D, ldh = dims
    dev = w_mean.device
    f32 = dict(dtype=torch.float32, device=dev)
    d_s_mean, d_s_sum = torch.empty(V, nh, **f32), torch.empty(V, nh, **f32)
    d_h_mean, d_h_sum, d_emb = torch.empty(V, K, **f32), torch.empty(V, K, **f32), torch.empty(V, D, **f32)
    _lib.check(lib.adkf_readout_pool_hidden_backward(ptr(h_mean), ptr(h_sum), ldh, ptr(w_mean), ptr(w_sum), ptr(argmax), ptr(perm), ptr(rowptr),
                                                     ptr(dp_mean), ptr(dp_sum), ptr(dwtot_sum), ptr(dg_max), V, G, nh, K, D, ptr(d_s_mean),
                                                     ptr(d_h_mean), ptr(d_s_sum), ptr(d_h_sum), ptr(d_emb), stream(dev)),
               "adkf_readout_pool_hidden_backward")
    return d_s_mean, d_h_mean, d_s_sum, d_h_sum, d_emb
