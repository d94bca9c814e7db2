// libadkf_gp.so - host side of the C ABI declared in include/adkf_gp.h: argument checks, workspace
// carving and the kernel pipeline of each entry point.  gfx950 only; no allocation, no synchronisation
// (except adkf_check_info), everything enqueued on the caller's stream.
//
// One translation unit.  The host code of each subsystem is a header of its own: host_common.h (helpers, the three values read from
// the environment), host_gp.h (GP pipeline), host_ard.h, host_stream.h (streaming prediction, pool selection and sampling),
// and - entry points included, at the end of this file - host_gnn.h and host_dense.h (dense layers, optimiser).  This file has the
// entry points of the GP, ARD and streaming calls.  The kernel headers come first, in the order the device code is emitted in.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "../../include/adkf_gp.h"
#include "ard.h"
#include "pna.h"
#include "readout.h"
#include "block.h"
#include "outer_step.h"
#include "refine64.h"
#include "hyper.h"
#include "large_fused.h"
#include "gemm_x3.h"
#include "dense_x3.h"
#include "dist_task.h"
#include "dz_task.h"
#include "predict_stream.h"
#include "thompson_stream.h"
#include "believer_stream.h"
#include "mes_stream.h"
#include "gumbel_stream.h"
#include "gibbon_stream.h"
#include "liar_stream.h"
#include "levelset_stream.h"
#include "kg_stream.h"
#include "jes_stream.h"
#include "ipv_stream.h"
#include "jackknife_stream.h"
#include "ehvi_stream.h"
#include "mix_stream.h"
#include "rank_stream.h"
#include "qei_stream.h"
#include "grad_stream.h"

#include "host_common.h"
#include "host_gp.h"
#include "host_ard.h"
#include "host_stream.h"

extern "C" {

const char* adkf_last_hip_error(void) { return hipGetErrorString(g_last_hip_error); }

const char* adkf_version(void) { return "adkf_gp 0.1 (gfx950)"; }

int adkf_path_info(int32_t ns_max, int32_t nq_max) {
    if (ns_max <= 0 || nq_max < 0 || ns_max > MAX_POINTS || nq_max > MAX_POINTS) return ADKF_E_SIZE;
    int bits = 0;
    const int hi = ns_max > nq_max ? ns_max : nq_max;
    if (nq_max > 0 && use_fused_outer(ns_max, nq_max)) bits |= ADKF_PATH_FUSED_OUTER;
    if (hi > REG_POINTS) { bits |= ADKF_PATH_BLOCKED; if (lg_fused_by_size(hi)) bits |= ADKF_PATH_BLOCKED_FUSED; }
    if (carve(nullptr, 1, ns_max, nq_max > 0 ? nq_max : 1, 4).w64_stride != 0) bits |= ADKF_PATH_R64_REGION;
    if (refine64_lds_optin()) bits |= ADKF_PATH_R64_LDS;
    return bits;
}

int adkf_max_points(void) { return MAX_POINTS; }

size_t adkf_workspace_bytes(int32_t T, int32_t ns_max, int32_t nq_max, int32_t d) {
    if (T <= 0 || ns_max <= 0 || nq_max < 0 || d <= 0) return 0;
    return carve(nullptr, T, ns_max, nq_max, d).bytes;
}

size_t adkf_workspace_bytes_ard(int32_t T, int32_t ns_max, int32_t nq_max, int32_t d) {
    if (T <= 0 || ns_max <= 0 || nq_max < 0 || d <= 0) return 0;
    return carve_ard(nullptr, carve(nullptr, T, ns_max, nq_max, d).bytes, T, ns_max, nq_max, d).bytes;
}

// median heuristic (+ optionally a4 in the same launch); returns true through *fused when init was applied
static int median_core(const adkf_batch_t* b, const Workspace& w, float* l0, const InitArgs& init, bool* fused, hipStream_t st) {
    bool selected = false;
    int rc = stage_dist(b, w, has_query(b), st, 3, l0, &init, &selected);
    if (rc) return rc;
    *fused = b->ns_max <= 256;
    if (selected) return 0;   // k_dist_task has written l0 (and phi / priors): no k_median
    if (b->ns_max <= 128) k_median<512, 16><<<grid_for(b->T, 1), 512, 0, st>>>(w.D2ss, b->n_s, b->ns_max, l0, b->T, init);
    else if (b->ns_max <= 256) k_median<1024, 32><<<grid_for(b->T, 1), 1024, 0, st>>>(w.D2ss, b->n_s, b->ns_max, l0, b->T, init);
    else {
        LgMedian lm{w.D2ss, b->n_s, b->ns_max, l0, b->T, reinterpret_cast<uint32_t*>(w.lg_med), w.lg_med + b->T, w.lg_med + 2 * (size_t)b->T};
        hipMemsetAsync(lm.hist, 0, sizeof(int) * 256 * (size_t)b->T, st);
        const int rows_blocks = ceil_div(b->ns_max, 16) < 64 ? ceil_div(b->ns_max, 16) : 64;
        for (int pass = 0; pass < 4; ++pass) {
            k_lg_med_hist<<<dim3(rows_blocks, b->T), 256, 0, st>>>(lm, pass);
            k_lg_med_pick<<<ceil_div(b->T, 64), 64, 0, st>>>(lm, pass);
        }
    }
    LAUNCH_OK();
    return 0;
}

int adkf_median_lengthscale(const adkf_batch_t* b, float* l0, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_batch(b, false);
    if (rc) return rc;
    if (!l0 || !ws) return ADKF_E_BADARG;
    Workspace w = carve_for(b, ws);
    if (ws_bytes < w.bytes) return ADKF_E_WORKSPACE;
    bool fused;
    return median_core(b, w, l0, InitArgs{0, 0, nullptr, nullptr}, &fused, static_cast<hipStream_t>(stream));
}

int adkf_init_params(const adkf_batch_t* b, int32_t use_numeric_labels, int32_t use_lengthscale_prior, float* phi,
                     float* priors, float* l0, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_batch(b, false);
    if (rc) return rc;
    if (!phi || !priors || !ws) return ADKF_E_BADARG;
    Workspace w = carve_for(b, ws);
    if (ws_bytes < w.bytes) return ADKF_E_WORKSPACE;
    float* l0p = l0 ? l0 : w.l0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    InitArgs init{use_numeric_labels, use_lengthscale_prior, phi, priors};
    ArdWs a{};
    if (is_ard(b)) {  // every lengthscale starts at the median heuristic (adaptive_dkt.py:101)
        a = carve_ard(ws, w.bytes, b->T, b->ns_max, b->nq_max, b->d);
        if (ws_bytes < a.bytes) return ADKF_E_WORKSPACE;
        init.phi = a.phi3;
    }
    bool fused = false;
    rc = median_core(b, w, l0p, init, &fused, st);
    if (rc) return rc;
    if (!fused) k_init_params<<<ceil_div(b->T, 64), 64, 0, st>>>(l0p, b->T, init);
    if (is_ard(b)) k_ard_expand_phi<<<dim3(ceil_div(2 + b->d, 256), b->T), 256, 0, st>>>(a.phi3, phi, b->T, 2 + b->d);
    LAUNCH_OK();
    return 0;
}

int adkf_mll_value_grad(const adkf_batch_t* b, const float* phi, float* f_in, float* g_phi, float* dZ_s, int32_t* info,
                        void* ws, size_t ws_bytes, void* stream) {
    int rc = check_batch(b, false);
    if (rc) return rc;
    if (!phi || !f_in || !info || !ws || !b->y_s || !b->priors) return ADKF_E_BADARG;
    if (is_ard(b)) {
        ArdCtx c;
        adkf_batch_t b0 = *b; b0.flags &= ~ADKF_BATCH_REUSE_INNER;
        rc = ard_setup(&b0, ws, ws_bytes, static_cast<hipStream_t>(stream), c);
        if (rc) return rc;
        rc = ard_eval(c, phi, f_in, g_phi ? g_phi : c.a.ge, info);
        if (rc) return rc;
        if (dZ_s) {
            ArdDzFin fs{c.v, c.a.G, nullptr, nullptr, nullptr, 0.f, dZ_s, b->n_s, c.ns};
            k_ard_dz_fin<<<dim3(ceil_div(c.d, 256), c.ns, c.T), 256, 0, c.st>>>(fs);
            LAUNCH_OK();
        }
        return 0;
    }
    Workspace w = carve_for(b, ws);
    if (ws_bytes < w.bytes) return ADKF_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = stage_dist(b, w, has_query(b), st);
    if (rc) return rc;
    InnerArgs ia = inner_args(b, w, const_cast<float*>(phi), info);
    ia.f_out = f_in; ia.g_out = g_phi;
    rc = launch_inner(ia, w, st);
    if (rc) return rc;
    launch_refine(make_tv(b, w, false), b, w, false, 0, nullptr, info, st, f_in, g_phi, nullptr);
    if (dZ_s) {
        TaskView tv = make_tv(b, w, false);
        const int win_tiles = std::max(1, std::min(64, b->ns_max * b->ns_max / 2048));
        WinArgs wa{tv, w.Ainv, w.D2ss, w.Wss, w.scal, b->T, win_tiles};
        k_win<<<grid_for(b->T, win_tiles), 256, 0, st>>>(wa);
        hipMemsetAsync(dZ_s, 0, (size_t)b->T * b->ns_max * b->d * sizeof(float), st);
        ProbDZ<false> pz; pz.tv = tv; pz.Wss = w.Wss; pz.Wqs = nullptr; pz.Wqq = nullptr; pz.Zs = b->Z_s; pz.Zq = nullptr; pz.dZ = dZ_s; pz.d = b->d;
        launch_gemm(pz, b->T, b->ns_max, b->d, st);   // (support only: the FP32 form, host_common.h)
        LAUNCH_OK();
    }
    return 0;
}

int adkf_fit(const adkf_batch_t* b, float* phi, const adkf_fit_options_t* opt, float* f_final, float* gnorm,
             int32_t* n_evals, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_batch(b, false);
    if (rc) return rc;
    if (!phi || !opt || !info || !ws || !b->y_s || !b->priors || opt->max_evals < 2) return ADKF_E_BADARG;
    if (is_ard(b)) return ard_fit(b, phi, opt, f_final, gnorm, n_evals, info, ws, ws_bytes, static_cast<hipStream_t>(stream));
    Workspace w = carve_for(b, ws);
    if (ws_bytes < w.bytes) return ADKF_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = stage_dist(b, w, has_query(b), st);
    if (rc) return rc;
    InnerArgs ia = inner_args(b, w, phi, info);
    ia.f_out = f_final; ia.gnorm_out = gnorm; ia.nevals_out = n_evals;
    ia.max_evals = opt->max_evals; ia.exact_evals = opt->exact_evals; ia.gtol = opt->gtol; ia.ftol = opt->ftol;
    if (opt->ev_start && hipEventRecord(static_cast<hipEvent_t>(opt->ev_start), st) != hipSuccess) return ADKF_E_LAUNCH;
    rc = launch_inner(ia, w, st);
    if (opt->ev_stop && hipEventRecord(static_cast<hipEvent_t>(opt->ev_stop), st) != hipSuccess) return ADKF_E_LAUNCH;
    if (rc) return rc;
    // ill-conditioned tasks: float64 value at phi* - unless the caller says that the next call on this workspace redoes it anyway
    if (!(b->flags & ADKF_BATCH_DEFER_REFINE)) launch_refine(make_tv(b, w, false), b, w, false, 0, nullptr, info, st, f_final, nullptr, gnorm);
    LAUNCH_OK();
    return 0;
}

int adkf_predict(const adkf_batch_t* b, const float* phi, float* mean, float* var, float* cov, int32_t* info, void* ws,
                 size_t ws_bytes, void* stream) {
    int rc = check_batch(b, true);
    if (rc) return rc;
    if (!phi || !mean || !info || !ws || !b->y_s || !b->priors) return ADKF_E_BADARG;
    if (is_ard(b)) {
        ArdCtx c;
        rc = ard_setup(b, ws, ws_bytes, static_cast<hipStream_t>(stream), c);
        if (rc) return rc;
        if (b->flags & ADKF_BATCH_REUSE_INNER) k_ard_params<<<dim3(ceil_div(c.d, 256), c.T), 256, 0, c.st>>>(c.v, phi);
        rc = ard_outer(c, phi, 0, nullptr, info, false);
        if (rc) return rc;
        adkf_batch_t bq = c.bt;
        return predict_core(&bq, c.w, mean, var, cov, info, c.st);
    }
    Workspace w = carve_for(b, ws);
    if (ws_bytes < w.bytes) return ADKF_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = stage_dist(b, w, true, st);
    if (rc) return rc;
    rc = inner_stage(b, w, phi, info, true, st);
    if (rc) return rc;
    return predict_core(b, w, mean, var, cov, info, st);
}

int adkf_predict_marginal(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows,
                          const float* best_f, float* mean, float* var, float* ei, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    return predict_marginal(false, b, phi, flags, Zq, q_off, rows, best_f, mean, var, ei, info, ws, ws_bytes, stream);
}

int adkf_predict_marginal_ard(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows,
                              const float* best_f, float* mean, float* var, float* ei, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    return predict_marginal(true, b, phi, flags, Zq, q_off, rows, best_f, mean, var, ei, info, ws, ws_bytes, stream);
}

int adkf_predict_grad(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows,
                      const float* best_f, const float* g_mean, const float* g_var, const float* g_ei, float* dZq, int32_t* info,
                      void* ws, size_t ws_bytes, void* stream) {
    return predict_grad(b, phi, flags, Zq, q_off, rows, best_f, g_mean, g_var, g_ei, dZq, info, ws, ws_bytes, stream);
}

size_t adkf_predict_pool_scratch_bytes(int32_t T, int32_t k) {
    if (T <= 0 || k <= 0 || k > ADKF_POOL_TOPK_MAX) return 0;
    return pool_scratch(nullptr, T, k).bytes;
}

int adkf_predict_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                      const int64_t* excl_idx, const int64_t* excl_off, float* mean, float* var, float* ei, int32_t k, int64_t* top_idx,
                      float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    return predict_pool(b, phi, flags, X, rows, best_f, excl_idx, excl_off, mean, var, ei, k, top_idx, top_val, info, ws, ws_bytes, scratch,
                        scratch_bytes, stream);
}

size_t adkf_thompson_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t S, int32_t m) {
    if (T <= 0 || ns_max <= 0 || ns_max > MAX_POINTS || S < 1 || S > ADKF_TS_SAMPLES_MAX) return 0;
    if (m < 64 || m > ADKF_TS_FEATURES_MAX || (m & 63)) return 0;
    return ts_scratch(nullptr, T, ns_max, S).bytes;
}

int adkf_thompson_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega,
                       const float* phase, int32_t m, const float* w, const float* eps, int32_t S, const int64_t* excl_idx,
                       const int64_t* excl_off, float* paths, int64_t* sel_idx, float* sel_val, int32_t* info, void* ws, size_t ws_bytes,
                       void* scratch, size_t scratch_bytes, void* stream) {
    return thompson_pool(false, b, phi, flags, X, rows, omega, phase, m, w, eps, S, excl_idx, excl_off, paths, sel_idx, sel_val, info, ws,
                         ws_bytes, scratch, scratch_bytes, stream);
}

int adkf_thompson_pool_ard(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega,
                           const float* phase, int32_t m, const float* w, const float* eps, int32_t S, const int64_t* excl_idx,
                           const int64_t* excl_off, float* paths, int64_t* sel_idx, float* sel_val, int32_t* info, void* ws, size_t ws_bytes,
                           void* scratch, size_t scratch_bytes, void* stream) {
    return thompson_pool(true, b, phi, flags, X, rows, omega, phase, m, w, eps, S, excl_idx, excl_off, paths, sel_idx, sel_val, info, ws,
                         ws_bytes, scratch, scratch_bytes, stream);
}

size_t adkf_qei_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t S, int32_t m) {
    if (T <= 0 || ns_max <= 0 || ns_max > MAX_POINTS || S < 1 || S > ADKF_QEI_SAMPLES_MAX) return 0;
    if (m < 64 || m > ADKF_TS_FEATURES_MAX || (m & 63)) return 0;
    return qe_scratch(nullptr, T, ns_max, S).bytes;
}

int adkf_qei_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega, const float* phase,
                  int32_t m, const float* w, const float* eps, int32_t S, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off,
                  int32_t q, float* trace, float* inc, int64_t* sel_idx, float* sel_val, int32_t* info, void* ws, size_t ws_bytes,
                  void* scratch, size_t scratch_bytes, void* stream) {
    return qei_pool(b, phi, flags, X, rows, omega, phase, m, w, eps, S, best_f, excl_idx, excl_off, q, trace, inc, sel_idx, sel_val, info, ws,
                    ws_bytes, scratch, scratch_bytes, stream);
}

size_t adkf_believer_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t q) {
    if (T <= 0 || ns_max <= 0 || ns_max > MAX_POINTS || d <= 0 || q < 1 || q > ADKF_POOL_TOPK_MAX) return 0;
    return bv_scratch(nullptr, T, ns_max, d, q).bytes;
}

int adkf_believer_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                       const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val,
                       float* sel_mean, float* sel_var, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes,
                       void* stream) {
    return believer_pool(false, b, phi, flags, X, rows, best_f, excl_idx, excl_off, q, trace, sel_idx, sel_val, sel_mean, sel_var, info, ws,
                         ws_bytes, scratch, scratch_bytes, stream);
}

int adkf_believer_pool_ard(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                           const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val,
                           float* sel_mean, float* sel_var, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes,
                           void* stream) {
    return believer_pool(true, b, phi, flags, X, rows, best_f, excl_idx, excl_off, q, trace, sel_idx, sel_val, sel_mean, sel_var, info, ws,
                         ws_bytes, scratch, scratch_bytes, stream);
}

int adkf_mes_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* ystar, int32_t S,
                  const int64_t* excl_idx, const int64_t* excl_off, float* score, int32_t k, int64_t* top_idx, float* top_val, int32_t* info,
                  void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    return mes_pool(b, phi, flags, X, rows, ystar, S, excl_idx, excl_off, score, k, top_idx, top_val, info, ws, ws_bytes, scratch, scratch_bytes,
                    stream);
}

size_t adkf_gumbel_pool_scratch_bytes(int32_t T) {
    if (T <= 0) return 0;
    return gb_scratch(nullptr, T).bytes;
}

int adkf_gumbel_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* u, int32_t S,
                     float* ystar, float* quant, float* gumbel, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes,
                     void* stream) {
    return gumbel_pool(b, phi, flags, X, rows, u, S, ystar, quant, gumbel, info, ws, ws_bytes, scratch, scratch_bytes, stream);
}

int adkf_gibbon_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* ystar, int32_t S,
                     const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val,
                     float* sel_mean, float* sel_var, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes,
                     void* stream) {
    return gibbon_pool(b, phi, flags, X, rows, ystar, S, excl_idx, excl_off, q, trace, sel_idx, sel_val, sel_mean, sel_var, info, ws, ws_bytes,
                       scratch, scratch_bytes, stream);
}

size_t adkf_levelset_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t q) {
    if (T <= 0 || ns_max <= 0 || ns_max > MAX_POINTS || d <= 0 || q < 1 || q > ADKF_POOL_TOPK_MAX) return 0;
    return ls_scratch(nullptr, T, ns_max, d, q).bytes;
}

int adkf_levelset_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* tau, const float* beta,
                       int32_t score, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int8_t* cls, int64_t* counts,
                       float* hits, int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, int32_t* info, void* ws,
                       size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    return levelset_pool(b, phi, flags, X, rows, tau, beta, score, excl_idx, excl_off, q, trace, cls, counts, hits, sel_idx, sel_val, sel_mean,
                         sel_var, info, ws, ws_bytes, scratch, scratch_bytes, stream);
}

size_t adkf_liar_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t q) {
    if (T <= 0 || ns_max <= 0 || ns_max > MAX_POINTS || d <= 0 || q < 1 || q > ADKF_POOL_TOPK_MAX) return 0;
    return liar_scratch(nullptr, T, ns_max, d, q).bytes;
}

int adkf_liar_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f, const float* lie,
                   const float* labels, int64_t label_stride, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace,
                   int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, float* sel_lie, float* inc, int32_t* info, void* ws,
                   size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    return liar_pool(b, phi, flags, X, rows, best_f, lie, labels, label_stride, excl_idx, excl_off, q, trace, sel_idx, sel_val, sel_mean,
                     sel_var, sel_lie, inc, info, ws, ws_bytes, scratch, scratch_bytes, stream);
}

size_t adkf_kg_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t M, int32_t k) {
    if (T <= 0 || ns_max <= 0 || ns_max > MAX_POINTS || d <= 0 || M < 1 || M > ADKF_KG_REFS_MAX || k < 0 || k > ADKF_POOL_TOPK_MAX) return 0;
    return kg_scratch(nullptr, T, ns_max, d, M, k).bytes;
}

int adkf_kg_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* ref_idx, int32_t M,
                 const int64_t* excl_idx, const int64_t* excl_off, float* score, float* cov, float* ref_mean, int32_t k, int64_t* top_idx,
                 float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    return kg_pool(b, phi, flags, X, rows, ref_idx, M, excl_idx, excl_off, score, cov, ref_mean, k, top_idx, top_val, info, ws, ws_bytes, scratch,
                   scratch_bytes, stream);
}

size_t adkf_jes_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t S, int32_t k) {
    if (T <= 0 || ns_max <= 0 || ns_max > MAX_POINTS || d <= 0 || S < 1 || S > ADKF_TS_SAMPLES_MAX || k < 0 || k > ADKF_POOL_TOPK_MAX) return 0;
    return jes_scratch(nullptr, T, ns_max, d, S, k).bytes;
}

int adkf_jes_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* opt_idx,
                  const float* opt_val, int32_t S, float cond_noise, const int64_t* excl_idx, const int64_t* excl_off, float* score,
                  float* opt_mean, float* opt_var, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes,
                  void* scratch, size_t scratch_bytes, void* stream) {
    return jes_pool(b, phi, flags, X, rows, opt_idx, opt_val, S, cond_noise, excl_idx, excl_off, score, opt_mean, opt_var, k, top_idx, top_val,
                    info, ws, ws_bytes, scratch, scratch_bytes, stream);
}

size_t adkf_ipv_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t M, int32_t q) {
    if (T <= 0 || ns_max <= 0 || ns_max > MAX_POINTS || d <= 0 || M < 1 || q < 1 || (int64_t)M + q > ADKF_IPV_ENTRIES_MAX) return 0;
    return ipv_scratch(nullptr, T, ns_max, d, M, q).bytes;
}

int adkf_ipv_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* tgt_idx,
                  const float* tgt_w, int32_t M, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx,
                  float* sel_val, float* tvar, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    return ipv_pool(b, phi, flags, X, rows, tgt_idx, tgt_w, M, excl_idx, excl_off, q, trace, sel_idx, sel_val, tvar, info, ws, ws_bytes, scratch,
                    scratch_bytes, stream);
}

size_t adkf_jackknife_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t L, int32_t k) {
    if (T <= 0 || ns_max <= 0 || ns_max > ADKF_JK_POINTS_MAX || L < 1 || L > ADKF_JK_LEVELS_MAX || k < 0 || k > ADKF_POOL_TOPK_MAX) return 0;
    return jk_scratch(nullptr, T, ns_max, k).bytes;
}

int adkf_jackknife_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* alpha, int32_t L,
                        const int64_t* excl_idx, const int64_t* excl_off, float* lo, float* hi, float* loo_mean, float* loo_var, float* loo_lpd,
                        int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch,
                        size_t scratch_bytes, void* stream) {
    return jackknife_pool(b, phi, flags, X, rows, alpha, L, excl_idx, excl_off, lo, hi, loo_mean, loo_var, loo_lpd, k, top_idx, top_val, info, ws,
                          ws_bytes, scratch, scratch_bytes, stream);
}

size_t adkf_ehvi_pool_scratch_bytes(int32_t T, int32_t G, int32_t k) {
    if (T <= 0 || G < 1 || k < 0 || k > ADKF_POOL_TOPK_MAX) return 0;
    return ehvi_scratch(nullptr, T, G, k).bytes;
}

int adkf_ehvi_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, int32_t G, const int32_t* obj,
                   const int32_t* obj_max, const float* ref, const float* front, const int32_t* front_n, int32_t P, const int32_t* con,
                   const float* con_thr, const int32_t* con_geq, int32_t C, const int64_t* excl_idx, const int64_t* excl_off, float* score,
                   float* stair, int32_t* stair_n, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes,
                   void* scratch, size_t scratch_bytes, void* stream) {
    return ehvi_pool(b, phi, flags, X, rows, G, obj, obj_max, ref, front, front_n, P, con, con_thr, con_geq, C, excl_idx, excl_off, score,
                     stair, stair_n, k, top_idx, top_val, info, ws, ws_bytes, scratch, scratch_bytes, stream);
}

size_t adkf_rank_pool_scratch_bytes(int32_t T, int32_t k, int32_t M, int32_t d) {
    if (T <= 0 || k < 0 || k > ADKF_RANK_K_MAX || M < 0 || M > ADKF_RANK_REFS_MAX || d <= 0) return 0;
    return rank_scratch(nullptr, T, k, M, d).bytes;
}

int adkf_rank_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                   const int64_t* excl_idx, const int64_t* excl_off, int32_t k, int64_t* top_idx, float* top_val, const int64_t* ref_idx,
                   int32_t M, int64_t* ref_rank, float* ref_val, int64_t* n_ranked, int32_t* info, void* ws, size_t ws_bytes, void* scratch,
                   size_t scratch_bytes, void* stream) {
    return rank_pool(b, phi, flags, X, rows, best_f, excl_idx, excl_off, k, top_idx, top_val, ref_idx, M, ref_rank, ref_val, n_ranked, info,
                     ws, ws_bytes, scratch, scratch_bytes, stream);
}

size_t adkf_mix_pool_scratch_bytes(int32_t T, int32_t G, int32_t k) {
    if (T <= 0 || G < 1 || k < 0 || k > ADKF_POOL_TOPK_MAX) return 0;
    return mix_scratch(nullptr, T, G, k).bytes;
}

int adkf_mix_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, int32_t G, const int32_t* mem,
                  const float* w, int32_t M, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off, float* mean,
                  float* var, float* score, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes,
                  void* scratch, size_t scratch_bytes, void* stream) {
    return mix_pool(b, phi, flags, X, rows, G, mem, w, M, best_f, excl_idx, excl_off, mean, var, score, k, top_idx, top_val, info, ws,
                    ws_bytes, scratch, scratch_bytes, stream);
}

int adkf_outer_nll_value_grad(const adkf_batch_t* b, const float* phi, float* f_out, float* g_phi, float* dZ_s,
                              float* dZ_q, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_batch(b, true);
    if (rc) return rc;
    if (!phi || !f_out || !info || !ws || !b->y_s || !b->y_q || !b->priors) return ADKF_E_BADARG;
    if (is_ard(b))
        return ard_ift(b, phi, 0, false, 0, 0.f, f_out, dZ_s, dZ_q, g_phi, nullptr, nullptr, info, ws, ws_bytes, static_cast<hipStream_t>(stream));
    Workspace w = carve_for(b, ws);
    if (ws_bytes < w.bytes) return ADKF_E_WORKSPACE;
    return outer_pipeline(b, w, phi, 0, false, f_out, dZ_s, dZ_q, g_phi, nullptr, nullptr, info, static_cast<hipStream_t>(stream));
}

int adkf_ift_hypergrad(const adkf_batch_t* b, const float* phi, int32_t flags, float* f_out, float* dZ_s, float* dZ_q,
                       float* g_phi_out, float* v, float* H, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_batch(b, true);
    if (rc) return rc;
    if (!phi || !f_out || !dZ_s || !dZ_q || !info || !ws || !b->y_s || !b->y_q || !b->priors) return ADKF_E_BADARG;
    if (is_ard(b)) {
        if (H) return ADKF_E_BADARG;   // the h x h Hessian is never formed: the system is solved by conjugate gradients
        return ard_ift(b, phi, flags, true, ADKF_CG_DEFAULT_MAXITER, ADKF_CG_DEFAULT_TOL, f_out, dZ_s, dZ_q, g_phi_out, v, nullptr, info,
                       ws, ws_bytes, static_cast<hipStream_t>(stream));
    }
    Workspace w = carve_for(b, ws);
    if (ws_bytes < w.bytes) return ADKF_E_WORKSPACE;
    return outer_pipeline(b, w, phi, flags, true, f_out, dZ_s, dZ_q, g_phi_out, v, H, info, static_cast<hipStream_t>(stream));
}

int adkf_double_path_tasks(const adkf_batch_t* b, int32_t* flagged, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_batch(b, true);
    if (rc) return rc;
    if (!flagged || !ws || is_ard(b)) return ADKF_E_BADARG;
    Workspace w = carve_for(b, ws);
    if (ws_bytes < w.bytes) return ADKF_E_WORKSPACE;
    (void)hipGetLastError();
    k_double_path_tasks<<<ceil_div(b->T, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(w.scal, b->ns_max, b->nq_max, w.w64 ? r64_threshold() : INFINITY, b->T, flagged);
    LAUNCH_OK();
    return 0;
}

int adkf_ift_hypergrad_cg(const adkf_batch_t* b, const float* phi, int32_t flags, int32_t cg_maxiter, float cg_tol, float* f_out,
                          float* dZ_s, float* dZ_q, float* g_phi_out, float* v, int32_t* cg_iters, int32_t* info, void* ws,
                          size_t ws_bytes, void* stream) {
    int rc = check_batch(b, true);
    if (rc) return rc;
    if (!is_ard(b) || cg_maxiter < 1 || !(cg_tol > 0.f)) return ADKF_E_BADARG;
    if (!phi || !f_out || !dZ_s || !dZ_q || !info || !ws || !b->y_s || !b->y_q || !b->priors) return ADKF_E_BADARG;
    return ard_ift(b, phi, flags, true, cg_maxiter, cg_tol, f_out, dZ_s, dZ_q, g_phi_out, v, cg_iters, info, ws, ws_bytes,
                   static_cast<hipStream_t>(stream));
}

int adkf_check_info(const int32_t* info, int32_t T, void* stream) {
    if (!info || T <= 0) return ADKF_E_BADARG;
    int32_t* host = static_cast<int32_t*>(malloc(sizeof(int32_t) * (size_t)T));
    if (!host) return ADKF_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemcpyAsync(host, info, sizeof(int32_t) * (size_t)T, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        free(host);
        return ADKF_E_LAUNCH;
    }
    int rc = 0;
    for (int t = 0; t < T; ++t) if (host[t] != 0) { rc = t + 1; break; }
    free(host);
    return rc;
}

}  // extern "C"

// the entry points of the other subsystems (here, after the GP entries: the device code keeps the order it has always had)
#include "host_gnn.h"
#include "host_dense.h"
