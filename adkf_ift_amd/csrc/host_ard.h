// Host side of ARD batches (ADKF_BATCH_ARD): the ARD region of the workspace, one evaluation of the inner objective and its
// Hessian-vector product on the scaled batch, the L-BFGS fit and the conjugate-gradient hypergradient.  See ard.h for the formulation.
#pragma once
#include "host_gp.h"

namespace {

struct ArdWs {
    float *mu, *ell, *Zt_s, *Zt_q, *G, *Gd_s, *Gd_q, *Gdot, *phi3, *pri3, *f3, *g3, *g3o, *S1, *gt, *coldot;
    float *c, *ut2, *wn, *Ddot, *Wdot, *adot, *S2;
    ArdFitState* fst; float *x, *g, *p, *xe, *ge, *S, *Y, *fe; int32_t* info3;
    ArdCgState* cst; float *cx, *cr, *cp, *cHp, *gout; int32_t* n_eff;
    size_t bytes;
};

ArdWs carve_ard(void* base, size_t off0, int T, int ns, int nq, int d) {
    static_assert(sizeof(ArdFitState) % sizeof(float) == 0 && sizeof(ArdCgState) % sizeof(float) == 0, "carved as whole floats");
    ArdWs a;
    Arena ar{static_cast<char*>(base), off0};
    auto take = [&](size_t nfloat) { return ar.floats(nfloat ? nfloat : 1); };   // (a region of a batch without query points keeps one float)
    const size_t Tz = (size_t)T, h = 2 + (size_t)d;
    a.mu = take(Tz * d); a.ell = take(Tz * d);
    a.Zt_s = take(Tz * ns * d); a.Zt_q = take(Tz * nq * d);
    a.G = take(Tz * ns * d); a.Gd_s = take(Tz * ns * d); a.Gd_q = take(Tz * nq * d); a.Gdot = take(Tz * ns * d);
    a.phi3 = take(Tz * 3); a.pri3 = take(Tz * 4); a.f3 = take(Tz); a.g3 = take(Tz * 3); a.g3o = take(Tz * 3);
    a.S1 = take(Tz * d); a.gt = take(Tz * h); a.coldot = take(Tz * d);
    a.c = take(Tz * d); a.ut2 = take(Tz * 2); a.wn = take(Tz * ns);
    a.Ddot = take(Tz * ns * ns); a.Wdot = take(Tz * ns * ns); a.adot = take(Tz * ns); a.S2 = take(Tz * d);
    a.fst = ar.as<ArdFitState>(Tz);
    a.x = take(Tz * h); a.g = take(Tz * h); a.p = take(Tz * h); a.xe = take(Tz * h); a.ge = take(Tz * h);
    a.S = take(Tz * ARD_M * h); a.Y = take(Tz * ARD_M * h); a.fe = take(Tz);
    a.info3 = ar.as<int32_t>(Tz);
    a.cst = ar.as<ArdCgState>(Tz);
    a.cx = take(Tz * h); a.cr = take(Tz * h); a.cp = take(Tz * h); a.cHp = take(Tz * h); a.gout = take(Tz * h);
    a.n_eff = ar.as<int32_t>(Tz);
    a.bytes = ar.off;
    return a;
}

struct ArdCtx {
    const adkf_batch_t* b;
    adkf_batch_t bt;   // the scaled batch the non-ARD pipeline runs on
    Workspace w; ArdWs a; ArdView v;
    int T, ns, nq, d, h;
    hipStream_t st;
};

int ard_setup(const adkf_batch_t* b, void* ws, size_t ws_bytes, hipStream_t st, ArdCtx& c) {
    c.b = b; c.T = b->T; c.ns = b->ns_max; c.nq = b->nq_max; c.d = b->d; c.h = 2 + b->d; c.st = st;
    c.w = carve(ws, c.T, c.ns, c.nq, c.d);
    c.a = carve_ard(ws, c.w.bytes, c.T, c.ns, c.nq, c.d);
    if (ws_bytes < c.a.bytes) return ADKF_E_WORKSPACE;
    ArdView& v = c.v;
    v.T = c.T; v.d = c.d; v.h = c.h; v.ns_ld = c.ns; v.nq_ld = c.nq; v.n_s = b->n_s; v.n_q = b->n_q;
    v.Z_s = b->Z_s; v.Z_q = b->Z_q; v.Zt_s = c.a.Zt_s; v.Zt_q = c.a.Zt_q; v.mu = c.a.mu; v.ell = c.a.ell;
    v.phi3 = c.a.phi3; v.pri3 = c.a.pri3; v.priors = b->priors; v.f3 = c.a.f3; v.g3 = c.a.g3; v.S1 = c.a.S1; v.gt = c.a.gt;
    c.bt = *b;
    c.bt.Z_s = c.a.Zt_s; c.bt.Z_q = has_query(b) ? c.a.Zt_q : nullptr; c.bt.priors = c.a.pri3; c.bt.flags = 0;
    if (!(b->flags & ADKF_BATCH_REUSE_INNER))
        k_colmean<<<dim3(ceil_div(c.d, 64), c.T), 256, 0, st>>>(b->Z_s, b->n_s, c.ns, c.d, c.a.mu, c.T);
    hipMemsetAsync(c.w.mean, 0, sizeof(float) * (size_t)c.T * c.d, st);   // the scaled features are centred already (stage_dist parts bit 4)
    return 0;
}

// d f / d Z~_s for the weights in w.Wss (symmetric) -> out
void ard_dz_support(ArdCtx& c, const float* W, float* out, const int32_t* n_override = nullptr) {
    TaskView tv = make_tv(&c.bt, c.w, false);
    if (n_override) tv.n_s = n_override;
    ProbDZ<false> pz; pz.tv = tv; pz.Wss = W; pz.Wqs = nullptr; pz.Wqq = nullptr; pz.Zs = c.a.Zt_s; pz.Zq = nullptr; pz.dZ = out; pz.d = c.d;
    launch_gemm(pz, c.T, c.ns, c.d, c.st);   // (support only: the FP32 form, host_common.h)
}

// The inner quantities at x [T, h]: l, Zt_s, D2ss, Ainv, alpha and the scalars in the workspace (the first half of
// ard_eval; adkf_predict_marginal_ard runs it alone, so the fit and the prediction produce A^-1 by the same launches).
int ard_inner(ArdCtx& c, const float* x, int32_t* info3) {
    hipStream_t st = c.st;
    k_ard_params<<<dim3(ceil_div(c.d, 256), c.T), 256, 0, st>>>(c.v, x);
    k_ard_scale<<<dim3(ceil_div(c.ns, 4), c.T), 256, 0, st>>>(c.v, c.b->Z_s, c.a.Zt_s, c.b->n_s, c.ns);
    int rc = stage_dist(&c.bt, c.w, false, st, 1 | 4);
    if (rc) return rc;
    InnerArgs ia = inner_args(&c.bt, c.w, c.a.phi3, info3);
    ia.f_out = c.a.f3; ia.g_out = c.a.g3;
    return launch_inner(ia, c.w, st);
}

// One evaluation of f_in and its gradient in the h raw parameters at x [T, h]; leaves Zt_s, D2ss, Ainv, alpha, the
// scalars, G = d f_in / d Z~, S1 and gt for x in the workspace.
int ard_eval(ArdCtx& c, const float* x, float* f, float* g, int32_t* info3) {
    hipStream_t st = c.st;
    int rc = ard_inner(c, x, info3);
    if (rc) return rc;
    TaskView tv = make_tv(&c.bt, c.w, false);
    const int win_tiles = std::max(1, std::min(64, c.ns * c.ns / 2048));
    WinArgs wa{tv, c.w.Ainv, c.w.D2ss, c.w.Wss, c.w.scal, c.T, win_tiles};
    k_win<<<grid_for(c.T, win_tiles), 256, 0, st>>>(wa);
    ard_dz_support(c, c.w.Wss, c.a.G);
    ArdColdot cd{c.a.Zt_s, c.a.G, c.b->n_s, c.ns, nullptr, nullptr, nullptr, 0, c.a.S1, c.d};
    k_ard_coldot<<<dim3(ceil_div(c.d, 64), c.T), 256, 0, st>>>(cd);
    ArdEvalFin ef{c.v, x, f, g, info3};
    k_ard_eval_fin<<<c.T, 256, 0, st>>>(ef);
    LAUNCH_OK();
    return 0;
}

// masked = true: sizes come from n_eff (0 for tasks whose CG has converged), so every kernel of the product skips them
ArdHvp ard_hvp_args(ArdCtx& c, const float* x, const float* u, float* Hu, const ArdCgState* cg, bool masked = false) {
    ArdHvp hv;
    hv.v = c.v; hv.tv = make_tv(&c.bt, c.w, false); hv.x = x; hv.u = u; hv.Hu = Hu;
    if (masked) { hv.v.n_s = c.a.n_eff; hv.tv.n_s = c.a.n_eff; }
    hv.c = c.a.c; hv.ut2 = c.a.ut2; hv.wn = c.a.wn; hv.D2 = c.w.D2ss; hv.Ainv = c.w.Ainv;
    hv.Ddot = c.a.Ddot; hv.X = c.w.P; hv.Wdot = c.a.Wdot; hv.adot = c.a.adot;
    hv.part = c.w.part_ma; hv.ntiles = c.w.nt_ma; hv.G = c.a.G; hv.Gdot = c.a.Gdot; hv.S2 = c.a.S2; hv.cg = cg;
    return hv;
}

// Everything of one Hessian-vector product up to Gdot' = 4 (rowsum(Wdot) . Z~ - Wdot Z~) (needed alone by the mixed term)
void ard_hvp_core(ArdCtx& c, const ArdHvp& hv) {
    hipStream_t st = c.st;
    k_ard_dir<<<dim3(ceil_div(c.d, 256), c.T), 256, 0, st>>>(hv);
    k_ard_wnorm<<<dim3(ceil_div(c.ns, 4), c.T), 256, 0, st>>>(hv);
    ProbArdDdot pd; pd.h = hv; launch_gemm(pd, c.T, c.ns, c.ns, st);
    ProbArdX px; px.h = hv; launch_gemm(px, c.T, c.ns, c.ns, st);
    k_ard_adot<<<dim3(ceil_div(c.ns, 4), c.T), 256, 0, st>>>(hv);
    ProbArdY py; py.h = hv; launch_gemm(py, c.T, c.ns, c.ns, st);
    ard_dz_support(c, c.a.Wdot, c.a.Gdot, hv.tv.n_s);
}

void ard_hvp(ArdCtx& c, const float* x, const float* u, float* Hu, const ArdCgState* cg) {
    ArdHvp hv = ard_hvp_args(c, x, u, Hu, cg, cg != nullptr);
    ard_hvp_core(c, hv);
    ArdColdot cd{c.a.Zt_s, c.a.Gdot, hv.tv.n_s, c.ns, nullptr, nullptr, nullptr, 0, c.a.S2, c.d};
    k_ard_coldot<<<dim3(ceil_div(c.d, 64), c.T), 256, 0, c.st>>>(cd);
    k_ard_hvp_fin<<<c.T, 256, 0, c.st>>>(hv);
}

__global__ void k_ard_expand_phi(const float* phi3, float* phi, int T, int h) {
    const int t = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k < h) phi[(size_t)t * h + k] = phi3[t * 3 + (k < 2 ? k : 2)];
}

__global__ void k_ard_cg_info(const ArdCgState* cg, int32_t* info, int32_t* iters, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    if (iters) iters[t] = cg[t].iters;
    if (cg[t].breakdown && info[t] == 0) info[t] = 200000 + cg[t].iters + 1;   // H not positive definite along a CG direction
}

int ard_fit(const adkf_batch_t* b, float* phi, const adkf_fit_options_t* opt, float* f_final, float* gnorm, int32_t* n_evals,
            int32_t* info, void* ws, size_t ws_bytes, hipStream_t st) {
    ArdCtx c;
    adkf_batch_t b0 = *b; b0.flags &= ~ADKF_BATCH_REUSE_INNER;
    int rc = ard_setup(&b0, ws, ws_bytes, st, c);
    if (rc) return rc;
    ArdFitArgs fa;
    fa.T = c.T; fa.h = c.h; fa.max_evals = opt->max_evals; fa.exact_evals = opt->exact_evals; fa.gtol = opt->gtol; fa.ftol = opt->ftol;
    fa.st = c.a.fst; fa.x = c.a.x; fa.g = c.a.g; fa.p = c.a.p; fa.xe = c.a.xe; fa.ge = c.a.ge; fa.S = c.a.S; fa.Y = c.a.Y;
    fa.fe = c.a.fe; fa.info_eval = c.a.info3; fa.phi = phi; fa.f_final = f_final; fa.gnorm = gnorm; fa.nevals = n_evals; fa.info = info;
    k_ard_fit_begin<<<dim3(ceil_div(c.h, 256), c.T), 256, 0, st>>>(fa);
    if (opt->ev_start && hipEventRecord(static_cast<hipEvent_t>(opt->ev_start), st) != hipSuccess) return ADKF_E_LAUNCH;
    FitPoll poll(!opt->exact_evals, opt->max_evals, c.a.n_eff, st);   // n_eff[0] is only used by the CG of the hypergradient
    for (int e = 0; e < opt->max_evals; ++e) {
        rc = ard_eval(c, c.a.xe, c.a.fe, c.a.ge, c.a.info3);
        if (rc) return rc;
        k_ard_advance<<<c.T, 256, 0, st>>>(fa);
        if (poll.finished(e, c.a.fst, sizeof(ArdFitState), offsetof(ArdFitState, phase), c.T, st)) break;
    }
    if (opt->ev_stop && hipEventRecord(static_cast<hipEvent_t>(opt->ev_stop), st) != hipSuccess) return ADKF_E_LAUNCH;
    LAUNCH_OK();
    return 0;
}

// The outer stages on the scaled batch: query scaling + distances, f_out, direct feature gradients, g_out (h entries).
int ard_outer(ArdCtx& c, const float* phi, int flags, float* f_out, int32_t* info, bool want_grads) {
    hipStream_t st = c.st;
    int rc;
    if (!(c.b->flags & ADKF_BATCH_REUSE_INNER)) {
        rc = ard_eval(c, phi, c.a.fe, c.a.ge, c.a.info3);
        if (rc) return rc;
        hipMemcpyAsync(info, c.a.info3, sizeof(int32_t) * (size_t)c.T, hipMemcpyDeviceToDevice, st);
    } else {
        hipMemsetAsync(info, 0, sizeof(int32_t) * (size_t)c.T, st);
    }
    k_ard_scale<<<dim3(ceil_div(c.nq, 4), c.T), 256, 0, st>>>(c.v, c.b->Z_q, c.a.Zt_q, c.b->n_q, c.nq);
    rc = stage_dist(&c.bt, c.w, true, st, 2 | 4);
    if (rc) return rc;
    if (!want_grads) return 0;
    adkf_batch_t bq = c.bt;
    bq.flags = ADKF_BATCH_REUSE_DIST | ADKF_BATCH_REUSE_INNER;
    int32_t* info_o = c.a.info3;   // outer factorisation status, merged below
    rc = outer_pipeline(&bq, c.w, c.a.phi3, flags & ADKF_IGNORE_DIRECT_GRAD, false, f_out, c.a.Gd_s, c.a.Gd_q, c.a.g3o, nullptr, nullptr, info_o, st);
    if (rc) return rc;
    ArdColdot cd{c.a.Zt_s, c.a.Gd_s, c.b->n_s, c.ns, c.a.Zt_q, c.a.Gd_q, c.b->n_q, c.nq, c.a.coldot, c.d};
    k_ard_coldot<<<dim3(ceil_div(c.d, 64), c.T), 256, 0, st>>>(cd);
    ArdGout go{c.v, phi, c.a.coldot, c.a.g3o, c.a.gout};
    k_ard_gout<<<dim3(ceil_div(c.d, 256), c.T), 256, 0, st>>>(go);
    LAUNCH_OK();
    return 0;
}

__global__ void k_merge_info(const int32_t* extra, int32_t* info, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < T && info[t] == 0 && extra[t] != 0) info[t] = extra[t];
}

int ard_ift(const adkf_batch_t* b, const float* phi, int flags, bool with_hessian, int cg_maxiter, float cg_tol, float* f_out,
            float* dZ_s, float* dZ_q, float* g_phi_out, float* v_out, int32_t* cg_iters, int32_t* info, void* ws, size_t ws_bytes,
            hipStream_t st) {
    ArdCtx c;
    int rc = ard_setup(b, ws, ws_bytes, st, c);
    if (rc) return rc;
    if (b->flags & ADKF_BATCH_REUSE_INNER) k_ard_params<<<dim3(ceil_div(c.d, 256), c.T), 256, 0, st>>>(c.v, phi);
    rc = ard_outer(c, phi, flags, f_out, info, true);
    if (rc) return rc;
    k_merge_info<<<ceil_div(c.T, 64), 64, 0, st>>>(c.a.info3, info, c.T);
    const size_t hb = sizeof(float) * (size_t)c.T * c.h;
    if (g_phi_out) hipMemcpyAsync(g_phi_out, c.a.gout, hb, hipMemcpyDeviceToDevice, st);
    const bool correct = with_hessian && !(flags & ADKF_IGNORE_GRAD_CORRECTION);
    if (correct) {
        // (round 5, measured and dropped: CG preconditioned with the L-BFGS history the fit has just built at this point - two-loop
        // recursion per round - needed MORE rounds than plain CG at the C2 shapes, h = 258: 10.1 on average, 17 at most, against 9.0 / 11
        // (profiles/r05_bench_ard_pcg.json), and its step kernel took 19 us instead of 4.  Twenty evaluations of a 258-parameter fit do
        // not leave a useful picture of the curvature; the lengthscale prior already keeps cond(H) near 1e3.)
        ArdCg cg{c.T, c.h, cg_tol, c.a.cst, c.a.gout, c.a.cx, c.a.cr, c.a.cp, c.a.cHp, b->n_s, c.ns, c.a.n_eff};
        k_ard_cg_begin<<<c.T, 256, 0, st>>>(cg);
        FitPoll poll(true, cg_maxiter, c.a.info3, st);   // info3 was merged into info above; free as a counter now
        for (int it = 0; it < cg_maxiter; ++it) {
            ard_hvp(c, phi, c.a.cp, c.a.cHp, c.a.cst);
            k_ard_cg_step<<<c.T, 256, 0, st>>>(cg);
            if (poll.finished(it, c.a.cst, sizeof(ArdCgState), offsetof(ArdCgState, done), c.T, st, 1, 2)) break;   // plain CG needs 9 rounds on average, 11 at most at the C2 shapes
        }
        k_ard_cg_info<<<ceil_div(c.T, 64), 64, 0, st>>>(c.a.cst, info, cg_iters, c.T);
        if (v_out) hipMemcpyAsync(v_out, c.a.cx, hb, hipMemcpyDeviceToDevice, st);
        ArdHvp hv = ard_hvp_args(c, phi, c.a.cx, c.a.cHp, nullptr);
        ard_hvp_core(c, hv);   // Gdot'(v), c(v)
    } else {
        if (v_out) hipMemsetAsync(v_out, 0, hb, st);
        if (cg_iters) hipMemsetAsync(cg_iters, 0, sizeof(int32_t) * (size_t)c.T, st);
    }
    if (dZ_s) {
        ArdDzFin fs{c.v, c.a.Gd_s, correct ? c.a.Gdot : nullptr, c.a.G, c.a.c, correct ? 1.f : 0.f, dZ_s, b->n_s, c.ns};
        k_ard_dz_fin<<<dim3(ceil_div(c.d, 256), c.ns, c.T), 256, 0, st>>>(fs);
    }
    if (dZ_q) {
        ArdDzFin fq{c.v, c.a.Gd_q, nullptr, nullptr, nullptr, 0.f, dZ_q, b->n_q, c.nq};
        k_ard_dz_fin<<<dim3(ceil_div(c.d, 256), c.nq, c.T), 256, 0, st>>>(fq);
    }
    LAUNCH_OK();
    return 0;
}

}  // namespace
