"""Plain references of the fused GNN kernels, ONE PER OPERATION (csrc/pna.h, csrc/block.h, csrc/readout.h): each function
restates the header comment of its C entry in torch, in the dtype of its inputs (float64 in the tests; float32 on the CPU is the
yardstick of profiles/gnn_kernel_yardsticks.json), with autograd for the backward.  No scatter ops: segments are Python loops, a
maximum is an explicit scan with strict ``>`` in list order and the value a GATHER of that one element - which is the rule the
kernels state ("first maximum in segment order") and which PyTorch's ``amax`` backward (it splits the gradient among ties) does not.

tests/test_gnn_kernel_refs.py ties these to the modules' own float64 CPU branches (which oracle/gnn_oracle.py validates);
tests/test_gpu_gnn_kernels.py holds every kernel output to them."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

PNA_SMALL = 1e-7   # fs_mol/modules/gnn.py:213-216


def _first_max(rows: torch.Tensor, ids: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Scan ``rows[ids[0]], rows[ids[1]], ...`` ([.., *shape] each): running maximum with strict ``>`` -> (values, ids of the winners)."""
    best = torch.full(rows.shape[1:], float("-inf"), dtype=rows.dtype)
    who = torch.full(rows.shape[1:], -1, dtype=torch.long)
    for e in ids:
        better = rows[e] > best
        best = torch.where(better, rows[e], best)
        who = torch.where(better, torch.full_like(who, e), who)
    return best, who


def pna_aggregate(msgs: torch.Tensor, perm: torch.Tensor, rowptr: torch.Tensor, V: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """msgs [E, H, 3m] (sum-part | mean/std-part | max-part), perm [E] message ids by target node, rowptr [V + 1]
    -> agg [V, H, 4m] = (sum | mean | std | max), argmax [V, H, m] (message id; -1 and zeros for an empty segment).
    std = sqrt(sum_e (relu(b_e^2 - mean^2) + 1e-7))."""
    E, H, m3 = msgs.shape
    m = m3 // 3
    a, b, c = msgs[..., :m], msgs[..., m:2 * m], msgs[..., 2 * m:]
    hh, ff = torch.meshgrid(torch.arange(H), torch.arange(m), indexing="ij")
    rows, argmax = [], torch.full((V, H, m), -1, dtype=torch.long)
    for v in range(V):
        ids = perm[int(rowptr[v]):int(rowptr[v + 1])]
        if ids.numel() == 0:
            rows.append(msgs.new_zeros(H, 4 * m))
            continue
        _, who = _first_max(c.detach(), ids.tolist())
        argmax[v] = who
        mean = b[ids].sum(0) / ids.numel()
        std = torch.sqrt((torch.relu(b[ids] ** 2 - mean ** 2) + PNA_SMALL).sum(0))
        rows.append(torch.cat((a[ids].sum(0), mean, std, c[who, hh, ff]), dim=1))     # (max: a gather - d_max goes to that one message)
    return torch.stack(rows), argmax


def msg_linear(x: torch.Tensor, srcs: List[torch.Tensor], tgts: List[torch.Tensor], Ws: Sequence[torch.Tensor],
               biases: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """cat(x[src], x[tgt]) W_et + b_et for every edge type and tower: x [V, H * in], W_et [H, 2 in, out], b_et [H, out]
    -> (pre [E_all, H, out], the per-type ``cat`` tensors [E_et, H, 2 in] - graph intermediates: ``torch.autograd.grad`` with
    respect to them is d cat)."""
    H = Ws[0].shape[0]
    xt = x.view(x.shape[0], H, -1)
    cats, pre = [], []
    for src, tgt, W, b in zip(srcs, tgts, Ws, biases):
        cat = torch.cat((xt[src], xt[tgt]), dim=2)
        cats.append(cat)
        pre.append(torch.einsum("ehi,hio->eho", cat, W) + b)
    return torch.cat(pre, dim=0), cats


def msg_forward(x, srcs, tgts, Ws, biases) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """msgs = relu(cat(x[src], x[tgt]) W + b) -> (msgs [E_all, H, out], cats).  Its autograd backward is what ``adkf_msg_backward``
    computes when it is given ``msgs`` (the mask taken inside)."""
    pre, cats = msg_linear(x, srcs, tgts, Ws, biases)
    return torch.relu(pre), cats


def msg_backward(x, srcs, tgts, Ws, biases, d, masked: bool):
    """(d cat [E_all, H, 2 in], d x, [d W_et], [d b_et]) for the cotangent ``d`` [E_all, H, out] of the messages.  masked=False: ``d``
    arrives behind the ReLU (autograd of ``msg_forward``).  masked=True: ``d`` is ALREADY the gradient in front of the ReLU
    (``msgs = NULL`` in the C entry): the backward of the linear part alone."""
    x = x.detach().requires_grad_(True)
    Ws = [w.detach().requires_grad_(True) for w in Ws]
    biases = [b.detach().requires_grad_(True) for b in biases]
    out, cats = (msg_linear if masked else msg_forward)(x, srcs, tgts, Ws, biases)
    n = len(Ws)
    g = torch.autograd.grad(out, [x, *Ws, *biases, *cats], d)
    return torch.cat(g[1 + 2 * n:], dim=0), g[0], list(g[1:1 + n]), list(g[1 + n:1 + 2 * n])


def block_combine(p, x, amp, att, bias, alpha, gamma, beta, eps):
    """new = p0 + amp p1 + att p2 + bias;  x1 = x + alpha new;  h = LayerNorm(x1) with the BIASED variance
    -> (x1 [V, hid], h [V, hid], mu [V], rstd [V]).  p [V, 3 hid] = [p0 | p1 | p2], amp / att [V]."""
    hid = x.shape[1]
    new = p[:, :hid] + amp.unsqueeze(1) * p[:, hid:2 * hid] + att.unsqueeze(1) * p[:, 2 * hid:] + bias
    x1 = x + alpha * new
    mu = x1.mean(dim=1)
    var = ((x1 - mu.unsqueeze(1)) ** 2).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + eps)
    h = (x1 - mu.unsqueeze(1)) * rstd.unsqueeze(1) * gamma + beta
    return x1, h, mu, rstd


def _segment_weights(s_mean, s_sum, perm, rowptr):
    """w_mean = softmax of s_mean over the nodes of each graph (from exponentials shifted by the graph's maximum), w_sum = sigmoid."""
    G = rowptr.numel() - 1
    w_mean = torch.zeros_like(s_mean)
    for g in range(G):
        ids = perm[int(rowptr[g]):int(rowptr[g + 1])]
        if ids.numel():
            e = torch.exp(s_mean[ids] - s_mean[ids].max(dim=0).values.detach())
            w_mean = w_mean.index_put((ids,), e / e.sum(dim=0))
    return w_mean, torch.sigmoid(s_sum)


def _segment_max(emb, perm, rowptr):
    """g_max [G, D] = emb at the first maximum in node-list order (0 and -1 for a graph without nodes)."""
    G, D = rowptr.numel() - 1, emb.shape[1]
    argmax = torch.full((G, D), -1, dtype=torch.long)
    rows = []
    for g in range(G):
        ids = perm[int(rowptr[g]):int(rowptr[g + 1])]
        if ids.numel() == 0:
            rows.append(emb.new_zeros(D))
            continue
        _, who = _first_max(emb.detach(), ids.tolist())
        argmax[g] = who
        rows.append(emb[who, torch.arange(D)])
    return torch.stack(rows), argmax


def readout_pool(s_mean, v_mean, s_sum, v_sum, emb, perm, rowptr, nh, hd):
    """g_mean[g, h, :] = sum_v w_mean[v, h] v_mean[v, h, :], g_sum likewise with the sigmoid weights, g_max = max over the graph's nodes
    -> (g_mean [G, nh hd], g_sum [G, nh hd], g_max [G, D], argmax [G, D], w_mean [V, nh], w_sum [V, nh])."""
    V, G = emb.shape[0], rowptr.numel() - 1
    w_mean, w_sum = _segment_weights(s_mean, s_sum, perm, rowptr)
    gm, gs = [], []
    for g in range(G):
        ids = perm[int(rowptr[g]):int(rowptr[g + 1])]
        gm.append((w_mean[ids].unsqueeze(-1) * v_mean[ids].view(-1, nh, hd)).sum(0).reshape(nh * hd))
        gs.append((w_sum[ids].unsqueeze(-1) * v_sum[ids].view(-1, nh, hd)).sum(0).reshape(nh * hd))
    g_max, argmax = _segment_max(emb, perm, rowptr)
    return torch.stack(gm), torch.stack(gs), g_max, argmax, w_mean, w_sum


def readout_pool_hidden(s_mean, h_mean, s_sum, h_sum, emb, perm, rowptr, nh):
    """p[h, g, :] = sum_v w[v, h] r_v for the softmax- and the sigmoid-weighted head, wtot_mean[g, h] = 1 (0: empty graph; a constant),
    wtot_sum[g, h] = sum_v w_sum[v, h]
    -> (p_mean [nh, G, K], p_sum [nh, G, K], wtot_mean [G, nh], wtot_sum [G, nh], g_max, argmax, w_mean, w_sum)."""
    G = rowptr.numel() - 1
    w_mean, w_sum = _segment_weights(s_mean, s_sum, perm, rowptr)
    pm, ps, wm, ws = [], [], [], []
    for g in range(G):
        ids = perm[int(rowptr[g]):int(rowptr[g + 1])]
        pm.append(w_mean[ids].t() @ h_mean[ids])      # [nh, K]
        ps.append(w_sum[ids].t() @ h_sum[ids])
        wm.append(s_mean.new_full((nh,), 1.0 if ids.numel() else 0.0))
        ws.append(w_sum[ids].sum(0))
    g_max, argmax = _segment_max(emb, perm, rowptr)
    return torch.stack(pm, dim=1), torch.stack(ps, dim=1), torch.stack(wm), torch.stack(ws), g_max, argmax, w_mean, w_sum
