// Host side and entry points of the GNN kernels: message functions (forward and backward), PNA aggregation, the attention read-out
// and the fused middle of a block.
#pragma once
#include "host_common.h"

namespace {
// fills the per-edge-type table of MsgArgs; returns the total number of edges, or -1 for a bad argument
long msg_table(MsgArgs& m, const adkf_msg_et_t* ets, int n_et, bool backward) {
    long e_all = 0;
    int splits = 0;
    for (int q = 0; q < n_et; ++q) {
        const adkf_msg_et_t& s = ets[q];
        if (s.E < 0 || !s.W || (s.E > 0 && (!s.src || !s.tgt)) || (!backward && !s.bias) || (backward && (!s.dW || !s.db))) return -1;
        MsgEt& et = msg_row(m, q);
        et.src = s.src; et.tgt = s.tgt; et.W = s.W; et.bias = s.bias; et.dW = s.dW; et.db = s.db; et.E = s.E;
        et.e_off = (int)e_all; et.tile0 = 0; et.split0 = splits; et.chunk = s.E > 0 ? msg_chunk(s.E) : 1;
        splits += msg_nsplit(s.E);
        e_all += s.E;
        if (e_all > 0x7fffffffL) return -1;
    }
    m.n_et = n_et; m.nsplit_all = splits;
    return e_all;
}
int msg_tiles(MsgArgs& m, int n_cols) {   // lays the edge types' tiles side by side for a launch whose result has n_cols columns
    int total = 0;
    for (int q = 0; q < m.n_et; ++q) { msg_row(m, q).tile0 = total; total += ceil_div(msg_row(m, q).E, GT) * ceil_div(n_cols, GT); }
    return total;
}
}  // namespace

extern "C" {

int adkf_msg_forward(const float* x, const adkf_msg_et_t* ets, int32_t n_et, int32_t H, int32_t in, int32_t out, float* msgs, void* stream) {
    (void)hipGetLastError();
    if (!x || !ets || !msgs || n_et <= 0 || n_et > MSG_MAX_ET || H <= 0 || in <= 0 || out <= 0) return ADKF_E_BADARG;
    MsgArgs m{};
    m.x = x; m.msgs = msgs; m.H = H; m.in = in; m.out = out;
    if (msg_table(m, ets, n_et, false) < 0) return ADKF_E_BADARG;
    m.vec = (in % 4 == 0) && (out % 4 == 0) && aligned16(x) && aligned16(msgs);
    for (int q = 0; q < n_et; ++q) m.vec = m.vec && aligned16(ets[q].W);
    const int total = msg_tiles(m, out);
    if (total == 0) return 0;
    ProbMsgFwd p; p.m = m;
    k_bgemm<ProbMsgFwd, GT><<<grid_for(H, total), 256, 0, static_cast<hipStream_t>(stream)>>>(p, H, 1, total);
    LAUNCH_OK();
    return 0;
}

size_t adkf_msg_backward_scratch_bytes(const adkf_msg_et_t* ets, int32_t n_et, int32_t H, int32_t in, int32_t out) {
    if (!ets || n_et <= 0 || n_et > MSG_MAX_ET || H <= 0 || in <= 0 || out <= 0) return 0;
    size_t splits = 0;
    for (int q = 0; q < n_et; ++q) splits += (size_t)msg_nsplit(ets[q].E);
    return sizeof(float) * splits * msg_part_stride(H, in, out);
}

int adkf_msg_backward(const float* x, const adkf_msg_et_t* ets, int32_t n_et, int32_t H, int32_t in, int32_t out, const float* msgs,
                      const float* d_msgs, const int64_t* perm_src, const int64_t* rowptr_src, const int64_t* perm_tgt,
                      const int64_t* rowptr_tgt, int32_t V, float* dcat, float* dx, void* scratch, size_t scratch_bytes, void* stream) {
    (void)hipGetLastError();
    if (!x || !ets || !d_msgs || !dcat || !dx || !perm_src || !rowptr_src || !perm_tgt || !rowptr_tgt) return ADKF_E_BADARG;   // (msgs may be null: d_msgs already masked)
    if (n_et <= 0 || n_et > MSG_MAX_ET || H <= 0 || in <= 0 || out <= 0 || V <= 0) return ADKF_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MsgArgs m{};
    m.x = x; m.msgs = const_cast<float*>(msgs); m.d_msgs = d_msgs; m.dcat = dcat; m.part = static_cast<float*>(scratch);
    m.H = H; m.in = in; m.out = out;
    const long e_all = msg_table(m, ets, n_et, true);
    if (e_all < 0) return ADKF_E_BADARG;
    if (m.nsplit_all > 0 && (!scratch || scratch_bytes < adkf_msg_backward_scratch_bytes(ets, n_et, H, in, out))) return ADKF_E_WORKSPACE;
    m.vec = (in % 4 == 0) && (out % 4 == 0) && aligned16(x) && (!msgs || aligned16(msgs)) && aligned16(d_msgs);
    for (int q = 0; q < n_et; ++q) m.vec = m.vec && aligned16(ets[q].W);
    const int total = msg_tiles(m, 2 * in);
    if (total > 0) {
        ProbMsgBwdX px; px.m = m;
        k_bgemm<ProbMsgBwdX, GT><<<grid_for(H, total), 256, 0, st>>>(px, H, 1, total);
        ProbMsgBwdW pw; pw.m = m;
        launch_gemm(pw, H * m.nsplit_all, 2 * in, out, st);
        k_msg_dbias<<<dim3(ceil_div(H * out, 64), m.nsplit_all), 256, 0, st>>>(m);
    }
    // d W / d b of every edge type (exact zeros where it has no edges), then d x gathered over each node's edge lists
    k_msg_reduce<<<dim3(ceil_div(H * 2 * in * out + H * out, 256), n_et), 256, 0, st>>>(m);
    MsgDxArgs da{dcat, perm_src, rowptr_src, perm_tgt, rowptr_tgt, dx, V, H, in};
    const long n = (long)V * H * in;
    k_msg_dx<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(da);
    LAUNCH_OK();
    return 0;
}

int adkf_readout_pool(const float* s_mean, const float* v_mean, const float* s_sum, const float* v_sum, const float* emb,
                      const int64_t* perm, const int64_t* rowptr, int32_t V, int32_t G, int32_t nh, int32_t hd, int32_t D,
                      float* w_mean, float* w_sum, float* g_mean, float* g_sum, float* g_max, int32_t* argmax, void* stream) {
    (void)hipGetLastError();
    if (!s_mean || !v_mean || !s_sum || !v_sum || !emb || !perm || !rowptr || !w_mean || !w_sum || !g_mean || !g_sum || !g_max || !argmax)
        return ADKF_E_BADARG;
    if (V < 0 || G <= 0 || nh <= 0 || nh > READOUT_MAX_HEADS || hd <= 0 || D <= 0) return ADKF_E_BADARG;
    ReadoutArgs a{};
    a.s_mean = s_mean; a.v_mean = v_mean; a.s_sum = s_sum; a.v_sum = v_sum; a.emb = emb; a.perm = perm; a.rowptr = rowptr;
    a.w_mean = w_mean; a.w_sum = w_sum; a.g_mean = g_mean; a.g_sum = g_sum; a.g_max = g_max; a.argmax = argmax;
    a.V = V; a.G = G; a.nh = nh; a.hd = hd; a.D = D;
    k_readout_fwd<<<G, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    LAUNCH_OK();
    return 0;
}

int adkf_readout_pool_backward(const float* v_mean, const float* v_sum, const float* w_mean, const float* w_sum, const float* g_mean,
                               const int32_t* argmax, const int64_t* node_to_graph, const float* dg_mean, const float* dg_sum,
                               const float* dg_max, int32_t V, int32_t G, int32_t nh, int32_t hd, int32_t D, float* d_s_mean,
                               float* d_v_mean, float* d_s_sum, float* d_v_sum, float* d_emb, void* stream) {
    (void)hipGetLastError();
    if (!v_mean || !v_sum || !w_mean || !w_sum || !g_mean || !argmax || !node_to_graph || !dg_mean || !dg_sum || !dg_max || !d_s_mean ||
        !d_v_mean || !d_s_sum || !d_v_sum || !d_emb)
        return ADKF_E_BADARG;
    if (V < 0 || G <= 0 || nh <= 0 || hd <= 0 || D <= 0) return ADKF_E_BADARG;
    if (V == 0) return 0;
    ReadoutArgs a{};
    a.v_mean = v_mean; a.v_sum = v_sum; a.w_mean = const_cast<float*>(w_mean); a.w_sum = const_cast<float*>(w_sum);
    a.g_mean = const_cast<float*>(g_mean); a.argmax = const_cast<int32_t*>(argmax); a.n2g = node_to_graph;
    a.dg_mean = dg_mean; a.dg_sum = dg_sum; a.dg_max = dg_max;
    a.d_s_mean = d_s_mean; a.d_v_mean = d_v_mean; a.d_s_sum = d_s_sum; a.d_v_sum = d_v_sum; a.d_emb = d_emb;
    a.V = V; a.G = G; a.nh = nh; a.hd = hd; a.D = D;
    k_readout_bwd<<<V, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    LAUNCH_OK();
    return 0;
}

int adkf_readout_pool_hidden(const float* s_mean, const float* h_mean, const float* s_sum, const float* h_sum, int32_t ldh, const float* emb,
                             const int64_t* perm, const int64_t* rowptr, int32_t V, int32_t G, int32_t nh, int32_t K, int32_t D,
                             float* w_mean, float* w_sum, float* p_mean, float* p_sum, float* wtot_mean, float* wtot_sum, float* g_max,
                             int32_t* argmax, void* stream) {
    (void)hipGetLastError();
    if (!s_mean || !h_mean || !s_sum || !h_sum || !emb || !perm || !rowptr || !w_mean || !w_sum || !p_mean || !p_sum || !wtot_mean || !wtot_sum ||
        !g_max || !argmax)
        return ADKF_E_BADARG;
    if (V < 0 || G <= 0 || nh <= 0 || nh > READOUT_MAX_HEADS || K <= 0 || K > 256 * READOUT_KJ_MAX || ldh < K || D <= 0 || D > READOUT_MAX_D) return ADKF_E_BADARG;
    ReadoutHArgs a{};
    a.s_mean = s_mean; a.h_mean = h_mean; a.s_sum = s_sum; a.h_sum = h_sum; a.ldh = ldh; a.emb = emb; a.perm = perm; a.rowptr = rowptr;
    a.w_mean = w_mean; a.w_sum = w_sum; a.p_mean = p_mean; a.p_sum = p_sum; a.wtot_mean = wtot_mean; a.wtot_sum = wtot_sum;
    a.g_max = g_max; a.argmax = argmax; a.V = V; a.G = G; a.nh = nh; a.K = K; a.D = D;
    launch_readout_h(a, false, static_cast<hipStream_t>(stream));
    LAUNCH_OK();
    return 0;
}

int adkf_readout_pool_hidden_backward(const float* h_mean, const float* h_sum, int32_t ldh, const float* w_mean, const float* w_sum,
                                      const int32_t* argmax, const int64_t* perm, const int64_t* rowptr, const float* dp_mean,
                                      const float* dp_sum, const float* dwtot_sum, const float* dg_max, int32_t V, int32_t G, int32_t nh,
                                      int32_t K, int32_t D, float* d_s_mean, float* d_h_mean, float* d_s_sum, float* d_h_sum, float* d_emb,
                                      void* stream) {
    (void)hipGetLastError();
    if (!h_mean || !h_sum || !w_mean || !w_sum || !argmax || !perm || !rowptr || !dp_mean || !dp_sum || !dwtot_sum || !dg_max || !d_s_mean ||
        !d_h_mean || !d_s_sum || !d_h_sum || !d_emb)
        return ADKF_E_BADARG;
    if (V < 0 || G <= 0 || nh <= 0 || nh > READOUT_MAX_HEADS || K <= 0 || K > 256 * READOUT_KJ_MAX || ldh < K || D <= 0 || D > READOUT_MAX_D) return ADKF_E_BADARG;
    if (V == 0) return 0;
    ReadoutHArgs a{};
    a.h_mean = h_mean; a.h_sum = h_sum; a.ldh = ldh; a.w_mean = const_cast<float*>(w_mean); a.w_sum = const_cast<float*>(w_sum);
    a.argmax = const_cast<int32_t*>(argmax); a.perm = perm; a.rowptr = rowptr;
    a.dp_mean = dp_mean; a.dp_sum = dp_sum; a.dwtot_sum = dwtot_sum; a.dg_max = dg_max;
    a.d_s_mean = d_s_mean; a.d_h_mean = d_h_mean; a.d_s_sum = d_s_sum; a.d_h_sum = d_h_sum; a.d_emb = d_emb;
    a.V = V; a.G = G; a.nh = nh; a.K = K; a.D = D;
    launch_readout_h(a, true, static_cast<hipStream_t>(stream));
    LAUNCH_OK();
    return 0;
}

int adkf_pna_aggregate(const float* msgs, const int64_t* perm, const int64_t* rowptr, int32_t V, int32_t H, int32_t m, float* agg,
                       int32_t* argmax, void* stream) {
    (void)hipGetLastError();
    if (!msgs || !perm || !rowptr || !agg || !argmax || V <= 0 || H <= 0 || m <= 0) return ADKF_E_BADARG;
    PnaArgs a{msgs, perm, rowptr, agg, argmax, nullptr, nullptr, V, H, m};
    k_pna_fwd<<<V, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    LAUNCH_OK();
    return 0;
}

int adkf_pna_aggregate_backward(const float* msgs, const int64_t* perm, const int64_t* rowptr, const float* agg, const int32_t* argmax,
                                const float* d_agg, int32_t V, int32_t H, int32_t m, float* d_msgs, void* stream) {
    (void)hipGetLastError();
    if (!msgs || !perm || !rowptr || !agg || !argmax || !d_agg || !d_msgs || V <= 0 || H <= 0 || m <= 0) return ADKF_E_BADARG;
    PnaArgs a{msgs, perm, rowptr, const_cast<float*>(agg), const_cast<int32_t*>(argmax), d_agg, d_msgs, V, H, m, 0};
    k_pna_bwd<<<V, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    LAUNCH_OK();
    return 0;
}

int adkf_pna_aggregate_backward_relu(const float* msgs, const int64_t* perm, const int64_t* rowptr, const float* agg, const int32_t* argmax,
                                     const float* d_agg, int32_t V, int32_t H, int32_t m, float* d_pre, void* stream) {
    (void)hipGetLastError();
    if (!msgs || !perm || !rowptr || !agg || !argmax || !d_agg || !d_pre || V <= 0 || H <= 0 || m <= 0) return ADKF_E_BADARG;
    PnaArgs a{msgs, perm, rowptr, const_cast<float*>(agg), const_cast<int32_t*>(argmax), d_agg, d_pre, V, H, m, 1};
    k_pna_bwd<<<V, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    LAUNCH_OK();
    return 0;
}

int adkf_block_combine(const float* p, const float* x, const float* amp, const float* att, const float* bias, const float* alpha,
                       const float* gamma, const float* beta, float eps, int32_t V, int32_t hid, float* x1, float* h, float* mu,
                       float* rstd, void* stream) {
    (void)hipGetLastError();
    if (!p || !x || !amp || !att || !bias || !alpha || !gamma || !beta || !x1 || !h || !mu || !rstd) return ADKF_E_BADARG;
    if (V <= 0 || hid <= 0 || (hid % 64) || hid > 64 * BLK_MAXC) return ADKF_E_SIZE;
    BlockArgs a{};
    a.p = p; a.x = x; a.amp = amp; a.att = att; a.bias = bias; a.alpha = alpha; a.gamma = gamma; a.beta = beta;
    a.x1 = x1; a.h = h; a.mu = mu; a.rstd = rstd; a.eps = eps; a.V = V; a.hid = hid;
    int grid = ceil_div(V, 4);
    grid = grid > 16384 ? 16384 : grid;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (hid / 64) {
        case 1: k_block_fwd<1><<<grid, 256, 0, st>>>(a); break;
        case 2: k_block_fwd<2><<<grid, 256, 0, st>>>(a); break;
        case 3: k_block_fwd<3><<<grid, 256, 0, st>>>(a); break;
        default: k_block_fwd<4><<<grid, 256, 0, st>>>(a); break;
    }
    LAUNCH_OK();
    return 0;
}

size_t adkf_block_combine_scratch_bytes(int32_t V, int32_t hid) {
    if (V <= 0 || hid <= 0) return 0;
    return sizeof(float) * (size_t)ceil_div(V, BLK_ROWS) * (3 * (size_t)hid + 1);
}

int adkf_block_combine_backward(const float* p, const float* x1, const float* amp, const float* att, const float* bias,
                                const float* alpha, const float* gamma, const float* mu, const float* rstd, const float* g_x1,
                                const float* g_h, int32_t V, int32_t hid, float* d_p, float* d_x, float* d_bias, float* d_alpha,
                                float* d_gamma, float* d_beta, void* scratch, size_t scratch_bytes, void* stream) {
    (void)hipGetLastError();
    if (!p || !x1 || !amp || !att || !bias || !alpha || !gamma || !mu || !rstd || !g_x1 || !g_h || !d_p || !d_x || !d_bias || !d_alpha ||
        !d_gamma || !d_beta || !scratch)
        return ADKF_E_BADARG;
    if (V <= 0 || hid <= 0 || (hid % 64) || hid > 64 * BLK_MAXC) return ADKF_E_SIZE;
    if (scratch_bytes < adkf_block_combine_scratch_bytes(V, hid)) return ADKF_E_WORKSPACE;
    BlockArgs a{};
    a.p = p; a.x1 = const_cast<float*>(x1); a.amp = amp; a.att = att; a.bias = bias; a.alpha = alpha; a.gamma = gamma;
    a.mu = const_cast<float*>(mu); a.rstd = const_cast<float*>(rstd); a.g_x1 = g_x1; a.g_h = g_h; a.d_p = d_p; a.d_x = d_x;
    a.part = static_cast<float*>(scratch); a.V = V; a.hid = hid;
    const int nwg = ceil_div(V, BLK_ROWS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (hid / 64) {
        case 1: k_block_bwd<1><<<nwg, 256, 0, st>>>(a); break;
        case 2: k_block_bwd<2><<<nwg, 256, 0, st>>>(a); break;
        case 3: k_block_bwd<3><<<nwg, 256, 0, st>>>(a); break;
        default: k_block_bwd<4><<<nwg, 256, 0, st>>>(a); break;
    }
    const int n = 3 * hid + 1;
    k_block_reduce<<<ceil_div(n, 64), 64, 0, st>>>(a.part, nwg, n, d_bias, d_gamma, d_beta, d_alpha, hid);
    LAUNCH_OK();
    return 0;
}

}  // extern "C"
