// Host side of streaming prediction on a support-only batch (adkf_predict_marginal, adkf_predict_pool, adkf_thompson_pool, their
// ARD forms, adkf_believer_pool, adkf_believer_pool_ard, adkf_liar_pool, adkf_levelset_pool, adkf_mes_pool, adkf_gibbon_pool, adkf_gumbel_pool, adkf_kg_pool, adkf_jes_pool, adkf_ipv_pool, adkf_jackknife_pool, adkf_ehvi_pool, adkf_mix_pool, adkf_rank_pool, adkf_qei_pool and adkf_predict_grad): the inner quantities into the workspace, the row-tile slots borrowed from it, the scratch layouts, the launch drivers the
// pool calls share (pool_walks, pool_select, pool_greedy) and the body of every entry.
#pragma once
#include "host_ard.h"

namespace {

constexpr int PM_POOL_LISTS = 4096;   // cap of the candidate lists of a call (the scratch size must not depend on the device)
inline int pm_pool_chunks_max(int T) { return std::max(1, PM_POOL_LISTS / T); }
// the workgroups per task of the float64 kernels: four rows per workgroup and pass
inline int pm64_grid(int64_t rows) { return (int)std::min<int64_t>(64, (rows + PM64_WAVES - 1) / PM64_WAVES); }

// adkf_predict_marginal borrows regions of a support-only workspace that prediction does not read - [P, W_ss] and, beyond 128
// points, the blocked sweep's scratch [lg_Dinv, lg_F] - for its row-tile slots.  Both spans are checked here against every
// buffer prediction reads (a reorder of carve() that broke that makes the span unusable instead of silently overwritten).
// also_read: further buffers the kernels read (adkf_predict_marginal_ard: the ARD region's mu, il, l and Zt_s, carved after
// the base carve).
struct SlotRegion { float* base; size_t floats; };
void pm_slot_regions(const Workspace& w, int T, int ns, SlotRegion (&r)[2], const SlotRegion* also_read = nullptr, int n_also = 0) {
    const size_t Tz = (size_t)T;
    r[0] = {w.P, (size_t)(w.Wss - w.P) + Tz * ns * ns};
    r[1] = {w.lg_Dinv, w.lg_Dinv ? (size_t)(w.lg_F - w.lg_Dinv) + Tz * LB * w.vld : 0};
    const char* rd[][2] = {   // [begin, end) of what the prediction kernels and k_refine64 (level 0) read or keep
        {reinterpret_cast<const char*>(w.mean), reinterpret_cast<const char*>(w.D2ss)},   // (mean [T, d] is carved first, D2ss right after)
        {reinterpret_cast<const char*>(w.D2ss), reinterpret_cast<const char*>(w.D2ss + Tz * ns * ns)},
        {reinterpret_cast<const char*>(w.Ainv), reinterpret_cast<const char*>(w.Ainv + Tz * ns * ns)},
        {reinterpret_cast<const char*>(w.vecs), reinterpret_cast<const char*>(w.vecs + Tz * NVEC * w.vld)},
        {reinterpret_cast<const char*>(w.scal), reinterpret_cast<const char*>(w.scal + Tz * NSCAL)},
        {reinterpret_cast<const char*>(w.lg_fit), reinterpret_cast<const char*>(w.lg_fit ? w.lg_fit + Tz : nullptr)},
        {reinterpret_cast<const char*>(w.w64), reinterpret_cast<const char*>(w.w64 ? w.w64 + 2 * Tz * w.w64_stride : nullptr)}};
    for (SlotRegion& q : r) {
        if (!q.base || q.floats == 0) { q = {nullptr, 0}; continue; }
        const char *b0 = reinterpret_cast<const char*>(q.base), *b1 = reinterpret_cast<const char*>(q.base + q.floats);
        for (const auto& x : rd)
            if (x[0] && x[0] < b1 && b0 < x[1]) { q = {nullptr, 0}; break; }
        for (int k = 0; k < n_also && q.base; ++k) {
            const char *x0 = reinterpret_cast<const char*>(also_read[k].base), *x1 = reinterpret_cast<const char*>(also_read[k].base + also_read[k].floats);
            if (x0 && x0 < b1 && b0 < x1) q = {nullptr, 0};
        }
    }
}

// What the streaming kernels of adkf_predict_marginal(_ard), adkf_predict_pool and adkf_thompson_pool run on, once pm_prepare has
// put the inner quantities of the support-only batch into the workspace.
struct PmCtx {
    adkf_batch_t b;             // the batch the kernels see; ARD: the scaled batch (Z_s = Zt_s)
    Workspace w;
    const float* mean_s;        // the support column means
    bool ard;
    PmArd r;                    // ARD: the query scaling
    SlotRegion also_read[4];    // ARD: the buffers of the ARD region the kernels read (kept out of the row-tile slots)
    int n_also;
    hipStream_t st;
};

// The inner quantities of b into its workspace (or the fit's, with REUSE_INNER) and the float64 A^-1 and alpha of flagged tasks.  ARD:
// PmCtx::r names the query scaling, whose 1 / l pm_launch writes into ArdWs::c (not read by prediction otherwise).
int pm_prepare(const adkf_batch_t* b, const float* phi, int32_t* info, void* ws, size_t ws_bytes, void* stream, PmCtx& c) {
    c.st = static_cast<hipStream_t>(stream);
    c.ard = is_ard(b);
    c.r = PmArd{};
    c.n_also = 0;
    int rc;
    if (c.ard) {
        ArdCtx ac;
        rc = ard_setup(b, ws, ws_bytes, c.st, ac);   // (checks the workspace size before it launches anything)
        if (rc) return rc;
        if (b->flags & ADKF_BATCH_REUSE_INNER) {   // the fit's state: mu, Zt_s, D2ss, A^-1, alpha, the scalars (ard_fit ends with an evaluation at phi*)
            k_ard_params<<<dim3(ceil_div(ac.d, 256), ac.T), 256, 0, c.st>>>(ac.v, phi);
            hipMemsetAsync(info, 0, sizeof(int32_t) * (size_t)ac.T, c.st);
        } else {
            rc = ard_inner(ac, phi, info);
            if (rc) return rc;
        }
        const size_t td = (size_t)ac.T * ac.d;
        c.b = ac.bt; c.w = ac.w; c.mean_s = ac.a.mu;
        c.r = PmArd{ac.a.c, ac.a.ell};
        c.also_read[0] = {ac.a.mu, td}; c.also_read[1] = {ac.a.ell, td}; c.also_read[2] = {ac.a.c, td}; c.also_read[3] = {ac.a.Zt_s, td * ac.ns};
        c.n_also = 4;
    } else {
        c.w = carve_for(b, ws);
        if (ws_bytes < c.w.bytes) return ADKF_E_WORKSPACE;
        rc = stage_dist(b, c.w, false, c.st);
        if (rc) return rc;
        rc = inner_stage(b, c.w, phi, info, true, c.st);
        if (rc) return rc;
        c.b = *b; c.mean_s = c.w.mean;
    }
    // flagged tasks: float64 A^-1 and alpha (a no-op re-evaluation after a fit that already ran it; needed after DEFER_REFINE, and
    // ard_fit does not run it)
    launch_refine(make_tv(&c.b, c.w, false), &c.b, c.w, false, 0, nullptr, info, c.st);
    LAUNCH_OK();
    return 0;
}

// The kernel arguments that do not depend on the call's outputs; Zq [rows, d]: the packed query rows or the shared pool.
PmArgs pm_args(const PmCtx& c, int32_t flags, const float* Zq, int64_t rows, const int32_t* info) {
    const adkf_batch_t& b = c.b;
    PmArgs pa{};
    pa.Zq = Zq; pa.Zs = b.Z_s; pa.mean_s = c.mean_s; pa.rows = rows;
    pa.n_s = b.n_s; pa.ns_ld = b.ns_max; pa.d = b.d; pa.kind = b.kernel; pa.T = b.T;
    pa.Ainv = c.w.Ainv; pa.D2ss = c.w.D2ss; pa.y_s = b.y_s; pa.scal = c.w.scal;
    pa.info = info;
    pa.refine_thresh = refine32_threshold(); pa.r64_thresh = c.w.w64 ? r64_threshold() : INFINITY;
    pa.latent = (flags & ADKF_PM_LATENT) ? 1 : 0; pa.maximize = (flags & ADKF_PM_MAXIMIZE) ? 1 : 0;
    pa.log_ei = (flags & ADKF_PM_LOG_EI) ? 1 : 0;
    pa.vec = ((b.d & 3) == 0 && aligned16(Zq) && aligned16(b.Z_s)) ? 1 : 0;
    pa.buf_ld = ceil_div(b.ns_max, PM_TM) * PM_TM + 4;
    pa.w64 = c.w.w64; pa.w64_stride = c.w.w64_stride;
    return pa;
}

// ARD: the query scaling il = 1 / l, into ArdWs::c
void launch_ard_il(const PmCtx& c) {
    const size_t td = (size_t)c.b.T * c.b.d;
    k_pm_ard_il<<<(unsigned)((td + 255) / 256), 256, 0, c.st>>>(c.r.ell, const_cast<float*>(c.r.il), (int64_t)td);
}

// What a kernel of the PmArgsOf family receives: pa, and the groups its instance has (ARD: the query scaling; POOL: *pool; v: the
// epilogue's arguments)
template <bool ARD, bool POOL, class EPI = PmRowEpilogue>
PmArgsOf<ARD, POOL, EPI> pm_kargs(const PmCtx& c, const PmArgs& pa, const PmPool* pool, const typename EPI::Args& v = {}) {
    PmArgsOf<ARD, POOL, EPI> k{};
    k.p = pa;
    if constexpr (ARD) k.r = c.r;
    if constexpr (POOL) k.s = *pool;
    k.v = v;
    return k;
}

// The grid of a persistent kernel (block, dyn bytes of dynamic LDS) over `items` work items: as many workgroups as are resident at once
template <class K>
int pm_persistent_grid(K kernel, int block, size_t dyn, int64_t items) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, dyn) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 1; }
    return (int)std::min<int64_t>(items, (int64_t)num_cus() * per_cu);
}

// The selection state of a pool call: lists of k entries per (task, chunk) in the scratch, every list empty at the start (one that no
// workgroup writes holds nothing), the exclusion lists only with their offsets.  The caller adds score_mean and top_*; the launches
// fill grid[].
PmPool pm_pool(const int64_t* excl_idx, const int64_t* excl_off, int k, int T, int64_t* cand_idx, float* cand_val, int64_t rows, hipStream_t st) {
    PmPool s{};
    s.excl_idx = excl_off ? excl_idx : nullptr; s.excl_off = excl_off;
    s.k = k; s.chunks_max = pm_pool_chunks_max(T);
    s.cand_idx = cand_idx; s.cand_val = cand_val;
    s.walked = rows > 0 ? 1 : 0;
    if (k > 0) hipMemsetAsync(cand_idx, 0xff, sizeof(int64_t) * (size_t)T * s.chunks_max * k, st);
    return s;
}

// a caller's scratch of `need` bytes: large enough, and (where anything is needed) there and 8-byte aligned
int check_scratch(const void* scratch, size_t have, size_t need) {
    if (have < need) return ADKF_E_WORKSPACE;
    if (need > 0 && (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 7u))) return ADKF_E_BADARG;
    return 0;
}

// The rows and outputs of a prediction call.  POOL (adkf_predict_pool): Zq is the shared pool, q_off unused, mean / var / ei are
// [T, rows] and nullable, *pool (pm_pool) carries the selection; pm_launch fills its grid[].
struct PmCall {
    int32_t flags;
    const float* Zq; const int64_t* q_off; int64_t rows;
    const float* best_f;
    float *mean, *var, *ei;
    int32_t* info;
    PmPool* pool;
};

// One walk of k_predict_marginal over the tasks of one kind (REFINE: the refined ones) with the epilogue EPI (arguments v): row tiles
// in LDS while they fit, otherwise in the global slots.  Both sizes come from the kernel's own LDS use: its static arrays, plus
// EPI_LDS bytes of the epilogue's (0 for prediction's and for the believer's, which works in the staging buffers).  POOL: the grid
// goes into pool->grid[REFINE].  tiles: an upper bound of the number of items.
template <bool REFINE, bool ARD, bool POOL, class EPI = PmRowEpilogue, int EPI_LDS = 0>
int pm_launch_walk(const PmCtx& c, PmArgs& pa, PmPool* pool, const typename EPI::Args& v, int64_t tiles) {
    const Workspace& w = c.w;
    hipStream_t st = c.st;
    const int T = c.b.T, ns = c.b.ns_max;
    const int ns_pad = pa.buf_ld - 4;
    constexpr int static_lds = (2 * PM_TM * LD_MN + 2 * PM_TM + 4 * PM_TM) * (int)sizeof(float) + EPI_LDS;
    constexpr int dyn_max = PM_LDS_BYTES - static_lds;
    static const bool optin = lds_optin(dyn_max, {kernel_ptr(&k_predict_marginal<REFINE, false, ARD, POOL, EPI>)});
    // a workgroup's row tiles: K (plain); K, C and the vector A^-1 y (refined)
    const size_t tile_floats = REFINE ? (size_t)2 * PM_TM * pa.buf_ld + ns_pad : (size_t)PM_TM * pa.buf_ld;
    const size_t dyn = tile_floats * sizeof(float);
    if (optin && dyn <= (size_t)dyn_max) {
        const int grid = pm_persistent_grid(k_predict_marginal<REFINE, false, ARD, POOL, EPI>, PM_NT, dyn, tiles);
        if constexpr (POOL) pool->grid[REFINE ? 1 : 0] = grid;
        k_predict_marginal<REFINE, false, ARD, POOL, EPI><<<grid, PM_NT, dyn, st>>>(pm_kargs<ARD, POOL, EPI>(c, pa, pool, v));
    } else {
        // global row-tile slots: [P, W_ss] and, beyond 128 points, the blocked path's scratch [lg_Dinv, lg_F] - neither is read by prediction
        pa.slot_floats = tile_floats;
        SlotRegion r[2];
        pm_slot_regions(w, T, ns, r, c.also_read, c.n_also);
        for (int q = 0; q < 2; ++q) { pa.slots[q] = r[q].base; pa.slot_count[q] = (int)std::min<size_t>(r[q].floats / pa.slot_floats, 1 << 20); }
        const int64_t slots = (int64_t)pa.slot_count[0] + pa.slot_count[1];
        if (slots < 1) return ADKF_E_WORKSPACE;
        const int grid = (int)std::min<int64_t>(tiles, std::min<int64_t>(slots, (int64_t)num_cus() * 8));
        if constexpr (POOL) pool->grid[REFINE ? 1 : 0] = grid;
        k_predict_marginal<REFINE, true, ARD, POOL, EPI><<<grid, PM_NT, 0, st>>>(pm_kargs<ARD, POOL, EPI>(c, pa, pool, v));
    }
    return 0;
}

// A float64 walk or a reference kernel of a pool call with the epilogue EPI: k_predict_marginal64, k_mes_walk64, k_kg_walk64, k_kg_refs ...
template <bool ARD, class EPI>
using PoolKernel = void (*)(PmArgsOf<ARD, true, EPI>);

// The walks of a pool call over the whole pool with the epilogue EPI (arguments v): the plain tasks, the refined ones and, where
// the caller has given the float64 walk a grid (pool.grid[2] > 0), the flagged ones with walk64.  No rows: nothing.  EPI_LDS: the
// static LDS of the epilogue itself (pm_launch_walk; JkEpilogue's row tile C - every other epilogue works in the staging buffers).
template <bool ARD, class EPI, int EPI_LDS = 0>
int pool_walks(const PmCtx& c, PmArgs& pa, PmPool& pool, const typename EPI::Args& v, PoolKernel<ARD, EPI> walk64 = nullptr) {
    if (pa.rows <= 0) return 0;
    const int T = c.b.T;
    const int64_t tiles = ((pa.rows + PM_TM - 1) / PM_TM) * T;
    int rc;
    if ((rc = pm_launch_walk<false, ARD, true, EPI, EPI_LDS>(c, pa, &pool, v, tiles))) return rc;
    if ((rc = pm_launch_walk<true, ARD, true, EPI, EPI_LDS>(c, pa, &pool, v, tiles))) return rc;
    if (pool.grid[2] > 0) walk64<<<dim3(pool.grid[2], T), PM64_NT, 0, c.st>>>(pm_kargs<ARD, true, EPI>(c, pa, &pool, v));
    return 0;
}

// the grid of the float64 walk of a pool call: 0 where none runs (run64: the call has a float64 region)
inline int pool_grid64(const PmPool& pool, int64_t rows, bool run64) {
    return (run64 && rows > 0) ? std::min(pm64_grid(rows), pool.chunks_max) : 0;
}

// "Score, then select" - adkf_predict_pool, adkf_mes_pool, adkf_kg_pool, adkf_jes_pool: (ARD) the 1 / l pass, the reference state
// where the call has one (refs: n_refs workgroups per task, with or without rows), the walks and the merge of the lists.  The caller
// has zeroed its outputs.  EPI_LDS: the static LDS of the epilogue itself (pm_launch_walk).
template <bool ARD, class EPI, int EPI_LDS = 0>
int pool_select(const PmCtx& c, PmArgs& pa, PmPool& pool, const typename EPI::Args& v, PoolKernel<ARD, EPI> walk64, bool run64,
                PoolKernel<ARD, EPI> refs = nullptr, int n_refs = 0) {
    const int T = c.b.T;
    if constexpr (ARD) launch_ard_il(c);
    if (refs) refs<<<dim3(n_refs, T), 256, 0, c.st>>>(pm_kargs<ARD, true, EPI>(c, pa, &pool, v));
    pool.grid[2] = pool_grid64(pool, pa.rows, run64);
    const int rc = pool_walks<ARD, EPI, EPI_LDS>(c, pa, pool, v, walk64);
    if (rc) return rc;
    if (pool.k > 0) k_pool_topk<<<T, 64, 0, c.st>>>(pm_kargs<false, true>(c, pa, &pool));
    LAUNCH_OK();
    return 0;
}

// "q greedy steps" - adkf_believer_pool(_ard) (v and bv are one) and adkf_gibbon_pool (bv = v.b): q chained steps, each the walks with
// the epilogue EPI and the believer's one workgroup per task on the believer's arguments.  adkf_liar_pool and adkf_levelset_pool
// (bv = v.b) name their own step kernel and that kernel's arguments sv, which hold bv (so they follow the step).
template <bool ARD, class EPI, class SEPI>
int pool_greedy(const PmCtx& c, PmArgs& pa, PmPool& pool, typename EPI::Args& v, BvArgs& bv, PoolKernel<ARD, EPI> walk64, bool have64,
                PoolKernel<ARD, SEPI> step, const typename SEPI::Args& sv) {
    if constexpr (ARD) launch_ard_il(c);
    pool.grid[2] = pool_grid64(pool, pa.rows, have64);
    for (int j = 0; j < bv.q; ++j) {
        bv.j = j;
        const int rc = pool_walks<ARD, EPI>(c, pa, pool, v, walk64);
        if (rc) return rc;
        step<<<c.b.T, 256, 0, c.st>>>(pm_kargs<ARD, true, SEPI>(c, pa, &pool, sv));
    }
    LAUNCH_OK();
    return 0;
}
template <bool ARD, class EPI>
int pool_greedy(const PmCtx& c, PmArgs& pa, PmPool& pool, typename EPI::Args& v, BvArgs& bv, PoolKernel<ARD, EPI> walk64, bool have64) {
    return pool_greedy<ARD, EPI, BvEpilogue>(c, pa, pool, v, bv, walk64, have64, k_bv_step<ARD>, bv);
}

// The streaming launches of a prepared prediction call.  POOL: pool_select with prediction's own epilogue.
template <bool ARD, bool POOL = false>
int pm_launch(const PmCtx& c, const PmCall& io) {
    hipStream_t st = c.st;
    const int T = c.b.T;
    const int64_t rows = io.rows;
    PmArgs pa = pm_args(c, io.flags, io.Zq, rows, io.info);
    pa.q_off = io.q_off; pa.best_f = io.best_f; pa.mean = io.mean; pa.var = io.var; pa.ei = io.ei;
    // every output row starts at 0: rows outside every task's range and those of skipped tasks (n_s == 0, info != 0) stay so
    const size_t out_n = POOL ? (size_t)rows * T : (size_t)rows;
    if (io.mean && out_n) hipMemsetAsync(io.mean, 0, sizeof(float) * out_n, st);
    if (io.var && out_n) hipMemsetAsync(io.var, 0, sizeof(float) * out_n, st);
    if (io.ei && out_n) hipMemsetAsync(io.ei, 0, sizeof(float) * out_n, st);
    if constexpr (POOL) {
        return pool_select<ARD, PmRowEpilogue>(c, pa, *io.pool, {}, k_predict_marginal64<ARD, true>, c.w.w64 != nullptr);
    } else {
        if constexpr (ARD) launch_ard_il(c);
        // upper bound of the tile count (the true one depends on q_off, which lives on the device)
        const int64_t tiles = rows / PM_TM + T;
        int rc;
        if (rows > 0) {
            if ((rc = pm_launch_walk<false, ARD, false>(c, pa, nullptr, {}, tiles))) return rc;
            if ((rc = pm_launch_walk<true, ARD, false>(c, pa, nullptr, {}, tiles))) return rc;
        }
        if (c.w.w64 && rows > 0) k_predict_marginal64<ARD, false><<<dim3(pm64_grid(rows), T), PM64_NT, 0, st>>>(pm_kargs<ARD, false>(c, pa, nullptr));
        LAUNCH_OK();
        return 0;
    }
}

// What every pool entry asks after check_support_only: a pool where there are rows, and exclusion lists only with their offsets
inline bool pool_args_ok(const float* X, int64_t rows, const int64_t* excl_idx, const int64_t* excl_off) {
    return !(rows > 0 && !X) && !(excl_idx && !excl_off);
}

// the selection of k rows per task: k itself and the two outputs it needs
inline int check_topk(int k, const int64_t* top_idx, const float* top_val) {
    if (k < 0 || (k > 0 && (!top_idx || !top_val))) return ADKF_E_BADARG;
    return k > ADKF_POOL_TOPK_MAX ? ADKF_E_SIZE : 0;
}

// Whether the call keeps float64 twins of its own state for flagged tasks: the workspace has a float64 region and the scratch, at this
// shape, the twins.  Without them no task takes the float64 walk.
inline bool pm_have64(const PmCtx& c, PmArgs& pa) {
    const bool have64 = c.w.w64 && c.b.ns_max <= R64_MAXN;
    if (!have64) pa.r64_thresh = INFINITY;
    return have64;
}

// What adkf_predict_marginal, adkf_thompson_pool (with their ARD forms) and adkf_predict_pool ask of their batch and first arguments:
// the support set only, with its labels, priors and phi.
int check_support_only(const adkf_batch_t* b, const float* phi, const int32_t* info, const void* ws, int64_t rows) {
    const int rc = check_batch(b, false);
    if (rc) return rc;
    if (b->nq_max != 0 || b->Z_q || b->y_q || !phi || !info || !ws || !b->y_s || !b->priors || rows < 0) return ADKF_E_BADARG;
    return 0;
}

// adkf_predict_marginal and adkf_predict_marginal_ard: the same call on a batch that is (ard) or is not an ARD batch
int predict_marginal(bool ard, const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows,
                     const float* best_f, float* mean, float* var, float* ei, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (is_ard(b) != ard || !q_off) return ADKF_E_BADARG;
    if (rows > 0 && (!Zq || !mean)) return ADKF_E_BADARG;
    if (ei && !best_f) return ADKF_E_BADARG;
    if (flags & ~(ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    if ((flags & ADKF_PM_LOG_EI) && !ei) return ADKF_E_BADARG;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    if (rows == 0) return 0;
    const PmCall io{flags, Zq, q_off, rows, best_f, mean, var, ei, info, nullptr};
    return ard ? pm_launch<true>(c, io) : pm_launch<false>(c, io);
}

// The launches of a prepared adkf_predict_grad call (grad_stream.h): the tile kernel for the plain tasks where its three row tiles fit
// in LDS (up to 128 points; otherwise the row kernel takes them too), the row kernel for the rest.
template <bool ARD>
int pg_launch(const PmCtx& c, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows, const float* best_f, PgArgs g, const int32_t* info) {
    hipStream_t st = c.st;
    const int T = c.b.T, ns = c.b.ns_max;
    PmArgs pa = pm_args(c, flags, Zq, rows, info);
    pa.q_off = q_off; pa.best_f = best_f;
    hipMemsetAsync(g.dZq, 0, sizeof(float) * (size_t)rows * c.b.d, st);   // rows of no task's range and of skipped tasks stay 0
    if constexpr (ARD) launch_ard_il(c);
    PgArgsOf<ARD> k{};
    k.p = pa;
    if constexpr (ARD) k.r = c.r;
    k.g = g;
    constexpr int static_lds = (2 * PM_TM * LD_MN + 2 * PM_TM + 4 * PM_TM + 3 * PM_TM) * (int)sizeof(float);
    constexpr int dyn_max = PM_LDS_BYTES - static_lds;
    static const bool optin = lds_optin(dyn_max, {kernel_ptr(&k_predict_grad_tile<ARD>)});
    const size_t dyn = ((size_t)3 * PM_TM * pa.buf_ld + (pa.buf_ld - 4)) * sizeof(float);
    const bool tile = optin && ns <= 128 && dyn <= (size_t)dyn_max;
    k.g.row_kinds = tile ? 6 : 7;
    if (tile) {
        const int64_t tiles = rows / PM_TM + T;   // upper bound (the true count depends on q_off, which lives on the device)
        const int grid = pm_persistent_grid(k_predict_grad_tile<ARD>, PM_NT, dyn, tiles);
        k_predict_grad_tile<ARD><<<grid, PM_NT, dyn, st>>>(k);
    }
    const size_t dyn_row = pg_row_lds(ns, c.w.w64 != nullptr);
    static const bool optin_row = lds_optin(pg_row_lds(MAX_POINTS, false), {kernel_ptr(&k_predict_grad_row<ARD>)});
    if (dyn_row > 64 * 1024 && !optin_row) return ADKF_E_LAUNCH;
    k_predict_grad_row<ARD><<<dim3((unsigned)std::min<int64_t>(rows, 64), T), PG_NT, dyn_row, st>>>(k);
    LAUNCH_OK();
    return 0;
}

// adkf_predict_grad: one entry for isotropic and ARD batches
int predict_grad(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows, const float* best_f,
                 const float* g_mean, const float* g_var, const float* g_ei, float* dZq, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (!q_off || (rows > 0 && (!Zq || !dZq))) return ADKF_E_BADARG;
    if (!g_mean && !g_var && !g_ei) return ADKF_E_BADARG;
    if (g_ei && !best_f) return ADKF_E_BADARG;
    if (flags & ~(ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    if ((flags & ADKF_PM_LOG_EI) && !g_ei) return ADKF_E_BADARG;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    if (rows == 0) return 0;
    const PgArgs g{g_mean, g_var, g_ei, dZq, 0};
    return c.ard ? pg_launch<true>(c, flags, Zq, q_off, rows, best_f, g, info) : pg_launch<false>(c, flags, Zq, q_off, rows, best_f, g, info);
}

// The candidate lists at the end of a scratch: n row indices (int64), then n scores
struct CandLists { int64_t* idx; float* val; };
inline CandLists carve_cand(Arena& ar, size_t n) {
    int64_t* idx = ar.as<int64_t>(n);
    return {idx, ar.floats(n)};
}

// The head of the believer's, the knowledge gradient's and joint entropy search's scratch, for n entries per task: w [T, n, ns], its
// float64 twin where a workspace of this shape can have a float64 region, and the entries' feature rows [T, n, d]
struct RefHead { float* W; double* W64; float* Xp; };
inline RefHead carve_ref_head(Arena& ar, int T, int n, int ns, int d) {
    const size_t e = (size_t)T * n * ns;
    float* W = ar.floats(e);
    double* W64 = ar.as<double>(ns <= R64_MAXN ? e : 0);
    return {W, W64, ar.floats((size_t)T * n * d)};
}

// adkf_thompson_pool: the scratch is V [T, S, ns] (float32), the same in float64 for flagged tasks where the workspace of this
// shape can have a float64 region, and one (row, score) pair per (task, chunk, sample)
struct TsScratch { float* v; double* v64; int64_t* cand_idx; float* cand_val; size_t bytes; };
static_assert(TS_M_MAX == ADKF_TS_FEATURES_MAX && TS_S_MAX == ADKF_TS_SAMPLES_MAX && TS_NS_MAX >= MAX_POINTS, "thompson_stream.h limits");
inline TsScratch ts_scratch(void* base, int T, int ns, int S) {
    Arena ar{static_cast<char*>(base), 0};
    const size_t e = (size_t)T * S * ns, c = (size_t)T * pm_pool_chunks_max(T) * S;
    float* v = ar.floats(e);
    double* v64 = ar.as<double>(ns <= R64_MAXN ? e : 0);
    const CandLists cand = carve_cand(ar, c);
    return {v, v64, cand.idx, cand.val, ar.off};
}

// adkf_predict_pool: the scratch is the candidate lists, cand_idx [T, chunks_max, k] (int64) directly followed by cand_val (float32)
struct PoolScratch { int64_t* cand_idx; float* cand_val; size_t bytes; };
inline PoolScratch pool_scratch(void* base, int T, int k) {
    const size_t n = (size_t)T * pm_pool_chunks_max(T) * k;
    int64_t* idx = static_cast<int64_t*>(base);
    return {idx, base ? reinterpret_cast<float*>(idx + n) : nullptr, n * (sizeof(int64_t) + sizeof(float))};
}

// The launches of a prepared Thompson call.  ARD: c.r names the query scaling, whose 1 / l goes into ArdWs::c first (as pm_launch).
template <bool ARD>
int ts_launch(const PmCtx& c, TsArgs& ta, int64_t rows) {
    hipStream_t st = c.st;
    const int T = c.b.T, ns = c.b.ns_max, S = ta.S;
    auto args = [&] {
        TsArgsOf<ARD> k{};
        static_cast<TsArgs&>(k) = ta;
        if constexpr (ARD) k.r = c.r;
        return k;
    };
    if (rows > 0) {
        if constexpr (ARD) launch_ard_il(c);
        k_ts_resid<false, ARD><<<dim3(ns, T), 256, 0, st>>>(ta);
        if (ta.V64) k_ts_resid<true, ARD><<<dim3(ns, T), 256, 0, st>>>(ta);
        k_ts_solve<false><<<dim3(S, T), 256, 0, st>>>(ta);
        if (ta.V64) k_ts_solve<true><<<dim3(S, T), 256, 0, st>>>(ta);
        ta.s.grid[0] = pm_persistent_grid(k_ts_stream<ARD>, PM_NT, 0, ((rows + PM_TM - 1) / PM_TM) * T);
        ta.s.grid[2] = ta.V64 ? std::min(pm64_grid(rows), ta.s.chunks_max) : 0;
        k_ts_stream<ARD><<<ta.s.grid[0], PM_NT, 0, st>>>(args());
        if (ta.V64) k_ts_stream64<ARD><<<dim3(ta.s.grid[2], T), PM64_NT, 0, st>>>(args());
    }
    k_ts_merge<<<T, 64, 0, st>>>(ta);
    LAUNCH_OK();
    return 0;
}

// adkf_thompson_pool and adkf_thompson_pool_ard: the same call on a batch that is (ard) or is not an ARD batch
int thompson_pool(bool ard, const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega,
                  const float* phase, int32_t m, const float* w, const float* eps, int32_t S, const int64_t* excl_idx,
                  const int64_t* excl_off, float* paths, int64_t* sel_idx, float* sel_val, int32_t* info, void* ws, size_t ws_bytes,
                  void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (is_ard(b) != ard) return ADKF_E_BADARG;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!omega || !phase || !w || !eps || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (S < 1 || S > ADKF_TS_SAMPLES_MAX) return ADKF_E_SIZE;
    if (m < 64 || m > ADKF_TS_FEATURES_MAX || (m & 63)) return ADKF_E_SIZE;
    const TsScratch l = ts_scratch(scratch, b->T, b->ns_max, S);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    hipStream_t st = c.st;
    const int T = b->T;
    TsArgs ta{};
    ta.p = pm_args(c, flags, X, rows, info);
    ta.s = pm_pool(excl_idx, excl_off, S, T, l.cand_idx, l.cand_val, rows, st);
    ta.s.top_idx = sel_idx; ta.s.top_val = sel_val;
    ta.omega = omega; ta.phase = phase; ta.w = w; ta.eps = eps; ta.m = m; ta.S = S;
    ta.vec_om = ((b->d & 3) == 0 && aligned16(omega)) ? 1 : 0;
    ta.V = l.v;
    ta.V64 = pm_have64(c, ta.p) ? l.v64 : nullptr;
    ta.paths = paths;
    // skipped tasks keep zeros in paths
    if (paths && rows > 0) hipMemsetAsync(paths, 0, sizeof(float) * (size_t)T * S * (size_t)rows, st);
    return ard ? ts_launch<true>(c, ta, rows) : ts_launch<false>(c, ta, rows);
}

// adkf_qei_pool: the scratch is Thompson's V [T, S, ns] (and its float64 twin where the workspace of this shape can have a float64
// region), the incumbents b [T, S], a pick count per task, one (row, score) pair per (task, chunk) and that candidate's S path values
struct QeScratch { float* v; double* v64; float* b; int32_t* cnt; CandLists cand; float* slots; size_t bytes; };
static_assert(QE_S_MAX == ADKF_QEI_SAMPLES_MAX && QE_Q_MAX == ADKF_QEI_PICKS_MAX && QE_NB_MAX == 4, "qei_stream.h limits");
inline QeScratch qe_scratch(void* base, int T, int ns, int S) {
    Arena ar{static_cast<char*>(base), 0};
    const size_t e = (size_t)T * S * ns, c = (size_t)T * pm_pool_chunks_max(T);
    QeScratch l{};
    l.v = ar.floats(e);
    l.v64 = ar.as<double>(ns <= R64_MAXN ? e : 0);
    l.b = ar.floats((size_t)T * S);
    l.cnt = ar.as<int32_t>((size_t)T);
    l.cand = carve_cand(ar, c);
    l.slots = ar.floats(c * S);
    l.bytes = ar.off;
    return l;
}

// The launches of a prepared q-EI call: Thompson's residual and solve once, the state, then q x (the walks, the step).  The walks are
// Thompson's (one persistent walk over the plain and the refined tasks, the float64 kernel for the flagged ones), which is why the
// loop is written here and is not pool_greedy's, whose walks are prediction's.
template <bool ARD, int NB>
int qe_launch(const PmCtx& c, QeArgs& v, int64_t rows) {
    hipStream_t st = c.st;
    const int T = c.b.T, ns = c.b.ns_max, S = v.S;
    auto args = [&] {
        QeArgsOf<ARD> k{};
        static_cast<QeArgs&>(k) = v;
        if constexpr (ARD) k.r = c.r;
        return k;
    };
    // (with or without rows: the noisy incumbents, inc row 0, come out of v)
    k_ts_resid<false, ARD><<<dim3(ns, T), 256, 0, st>>>(v);
    if (v.V64) k_ts_resid<true, ARD><<<dim3(ns, T), 256, 0, st>>>(v);
    k_ts_solve<false><<<dim3(S, T), 256, 0, st>>>(v);
    if (v.V64) k_ts_solve<true><<<dim3(S, T), 256, 0, st>>>(v);
    if (rows > 0) {
        if constexpr (ARD) launch_ard_il(c);
        v.s.grid[0] = pm_persistent_grid(k_qei_stream<ARD, NB>, PM_NT, 0, ((rows + PM_TM - 1) / PM_TM) * T);
        v.s.grid[2] = v.V64 ? std::min(pm64_grid(rows), v.s.chunks_max) : 0;
    }
    k_qei_init<<<T, 256, 0, st>>>(v);
    for (int j = 0; j < v.q; ++j) {
        v.j = j;
        if (rows > 0) {
            k_qei_stream<ARD, NB><<<v.s.grid[0], PM_NT, 0, st>>>(args());
            if (v.V64) k_qei_stream64<ARD><<<dim3(v.s.grid[2], T), PM64_NT, 0, st>>>(args());
        }
        k_qei_step<<<T, 256, 0, st>>>(v);
    }
    LAUNCH_OK();
    return 0;
}

// adkf_qei_pool: isotropic and ARD batches alike (as adkf_mes_pool)
int qei_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega, const float* phase,
             int32_t m, const float* w, const float* eps, int32_t S, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off,
             int32_t q, float* trace, float* inc, int64_t* sel_idx, float* sel_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch,
             size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!omega || !phase || !w || !eps || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (S < 1 || S > ADKF_QEI_SAMPLES_MAX) return ADKF_E_SIZE;
    if (m < 64 || m > ADKF_TS_FEATURES_MAX || (m & 63)) return ADKF_E_SIZE;
    if (q < 1 || q > ADKF_QEI_PICKS_MAX) return ADKF_E_SIZE;
    const QeScratch l = qe_scratch(scratch, b->T, b->ns_max, S);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    hipStream_t st = c.st;
    const int T = b->T;
    QeArgs v{};
    v.p = pm_args(c, flags, X, rows, info);
    v.s = pm_pool(excl_idx, excl_off, 1, T, l.cand.idx, l.cand.val, rows, st);
    v.omega = omega; v.phase = phase; v.w = w; v.eps = eps; v.m = m; v.S = S;
    v.vec_om = ((b->d & 3) == 0 && aligned16(omega)) ? 1 : 0;
    v.V = l.v;
    v.V64 = pm_have64(c, v.p) ? l.v64 : nullptr;
    v.q = q; v.b = l.b; v.cnt = l.cnt; v.slots = l.slots; v.best_f = best_f;
    v.trace = trace; v.inc = inc; v.sel_idx = sel_idx; v.sel_val = sel_val;
    // skipped tasks keep zeros in trace
    if (trace && rows > 0) hipMemsetAsync(trace, 0, sizeof(float) * (size_t)T * q * (size_t)rows, st);
    const int nb = S <= TS_S_MAX ? 1 : (S <= 2 * TS_S_MAX ? 2 : 4);
    if (c.ard) return nb == 1 ? qe_launch<true, 1>(c, v, rows) : (nb == 2 ? qe_launch<true, 2>(c, v, rows) : qe_launch<true, 4>(c, v, rows));
    return nb == 1 ? qe_launch<false, 1>(c, v, rows) : (nb == 2 ? qe_launch<false, 2>(c, v, rows) : qe_launch<false, 4>(c, v, rows));
}

// adkf_believer_pool: the scratch is w [T, q, ns] (and its float64 twin where a workspace of this shape can have a float64 region),
// the picks' feature rows [T, q, d], G [T, q, q] (and its twin), the incumbent and the pick count per task, and one (row, score)
// pair per (task, chunk)
struct BvScratch { RefHead h; float* G; double* G64; float* best; int32_t* cnt; CandLists cand; size_t bytes; };
inline BvScratch bv_scratch(void* base, int T, int ns, int d, int q) {
    Arena ar{static_cast<char*>(base), 0};
    const size_t g = (size_t)T * q * q;
    BvScratch l{};
    l.h = carve_ref_head(ar, T, q, ns, d);
    l.G = ar.floats(g);
    l.G64 = ar.as<double>(ns <= R64_MAXN ? g : 0);
    l.best = ar.floats((size_t)T);
    l.cnt = ar.as<int32_t>((size_t)T);
    l.cand = carve_cand(ar, (size_t)T * pm_pool_chunks_max(T));
    l.bytes = ar.off;
    return l;
}

// The believer's arguments on its scratch
BvArgs bv_args(const BvScratch& l, bool have64, int q, float* trace, int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var) {
    BvArgs v{};
    v.q = q;
    v.W = l.h.W; v.W64 = have64 ? l.h.W64 : nullptr; v.Xp = l.h.Xp; v.G = l.G; v.G64 = have64 ? l.G64 : nullptr;
    v.best = l.best; v.cnt = l.cnt; v.trace = trace;
    v.sel_idx = sel_idx; v.sel_val = sel_val; v.sel_mean = sel_mean; v.sel_var = sel_var;
    return v;
}

// adkf_believer_pool and adkf_believer_pool_ard: the same call on a batch that is (ard) or is not an ARD batch
int believer_pool(bool ard, const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                  const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val, float* sel_mean,
                  float* sel_var, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (is_ard(b) != ard) return ADKF_E_BADARG;
    if (flags & ~(ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!best_f || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (q < 1) return ADKF_E_BADARG;
    if (q > ADKF_POOL_TOPK_MAX) return ADKF_E_SIZE;
    const BvScratch l = bv_scratch(scratch, b->T, b->ns_max, b->d, q);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    hipStream_t st = c.st;
    const int T = b->T;
    PmArgs pa = pm_args(c, flags, X, rows, info);
    pa.best_f = best_f;
    const bool have64 = pm_have64(c, pa);
    PmPool pool = pm_pool(excl_idx, excl_off, 1, T, l.cand.idx, l.cand.val, rows, st);
    BvArgs v = bv_args(l, have64, q, trace, sel_idx, sel_val, sel_mean, sel_var);
    // skipped tasks keep zeros in trace
    if (trace && rows > 0) hipMemsetAsync(trace, 0, sizeof(float) * (size_t)T * q * (size_t)rows, st);
    k_bv_init<<<ceil_div(T, 256), 256, 0, st>>>(v, best_f, T);
    return ard ? pool_greedy<true, BvEpilogue>(c, pa, pool, v, v, k_bv_walk64<true>, have64)
               : pool_greedy<false, BvEpilogue>(c, pa, pool, v, v, k_bv_walk64<false>, have64);
}

// adkf_liar_pool: the scratch is the believer's (bv_scratch), then z [T, q] and its float64 twin
struct LiarScratch { BvScratch b; float* z; double* z64; size_t bytes; };
inline LiarScratch liar_scratch(void* base, int T, int ns, int d, int q) {
    LiarScratch l{};
    l.b = bv_scratch(base, T, ns, d, q);
    Arena ar{static_cast<char*>(base), l.b.bytes};
    l.z = ar.floats((size_t)T * q);
    l.z64 = ar.as<double>(ns <= R64_MAXN ? (size_t)T * q : 0);
    l.bytes = ar.off;
    return l;
}

// adkf_liar_pool: isotropic and ARD batches alike (as adkf_gibbon_pool)
int liar_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f, const float* lie,
              const float* labels, int64_t label_stride, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace,
              int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, float* sel_lie, float* inc, int32_t* info, void* ws,
              size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~(ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!best_f || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (!lie && !labels) return ADKF_E_BADARG;   // (that call is adkf_believer_pool)
    if (label_stride != 0 && (label_stride != rows || !labels)) return ADKF_E_BADARG;
    if (q < 1) return ADKF_E_BADARG;
    if (q > ADKF_POOL_TOPK_MAX) return ADKF_E_SIZE;
    const LiarScratch l = liar_scratch(scratch, b->T, b->ns_max, b->d, q);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    hipStream_t st = c.st;
    const int T = b->T;
    PmArgs pa = pm_args(c, flags, X, rows, info);
    pa.best_f = best_f;
    const bool have64 = pm_have64(c, pa);
    PmPool pool = pm_pool(excl_idx, excl_off, 1, T, l.b.cand.idx, l.b.cand.val, rows, st);
    LiarArgs v{};
    v.b = bv_args(l.b, have64, q, trace, sel_idx, sel_val, sel_mean, sel_var);
    v.lie = lie; v.labels = labels; v.stride = label_stride;
    v.z = l.z; v.z64 = have64 ? l.z64 : nullptr; v.sel_lie = sel_lie; v.inc = inc;
    // skipped tasks keep zeros in trace
    if (trace && rows > 0) hipMemsetAsync(trace, 0, sizeof(float) * (size_t)T * q * (size_t)rows, st);
    k_bv_init<<<ceil_div(T, 256), 256, 0, st>>>(v.b, best_f, T);
    k_liar_init<<<ceil_div(T, 256), 256, 0, st>>>(v, best_f, T);
    return c.ard ? pool_greedy<true, LiarEpilogue, LiarEpilogue>(c, pa, pool, v, v.b, k_liar_walk64<true>, have64, k_liar_step<true>, v)
                 : pool_greedy<false, LiarEpilogue, LiarEpilogue>(c, pa, pool, v, v.b, k_liar_walk64<false>, have64, k_liar_step<false>, v);
}

// adkf_predict_pool: isotropic and ARD batches alike
int predict_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                 const int64_t* excl_idx, const int64_t* excl_off, float* mean, float* var, float* ei, int32_t k, int64_t* top_idx,
                 float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~(ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_SCORE_MEAN | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    const bool by_mean = (flags & ADKF_PM_SCORE_MEAN) != 0;
    if ((flags & ADKF_PM_LOG_EI) && !ei && (k == 0 || by_mean)) return ADKF_E_BADARG;   // nothing would read it
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if ((ei || (k > 0 && !by_mean)) && !best_f) return ADKF_E_BADARG;
    if (!mean && !var && !ei && k == 0) return ADKF_E_BADARG;
    if ((rc = check_topk(k, top_idx, top_val))) return rc;
    const PoolScratch l = pool_scratch(scratch, b->T, k);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    PmPool pool = pm_pool(excl_idx, excl_off, k, b->T, l.cand_idx, l.cand_val, rows, c.st);
    pool.score_mean = by_mean ? 1 : 0; pool.top_idx = top_idx; pool.top_val = top_val;
    const PmCall io{flags & (ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI), X, nullptr, rows, best_f, mean, var, ei, info, &pool};
    return c.ard ? pm_launch<true, true>(c, io) : pm_launch<false, true>(c, io);
}

// adkf_mes_pool: isotropic and ARD batches alike (as adkf_predict_pool); the scratch is adkf_predict_pool's candidate lists
int mes_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* ystar, int32_t S,
             const int64_t* excl_idx, const int64_t* excl_off, float* score, int32_t k, int64_t* top_idx, float* top_val, int32_t* info,
             void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!ystar) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k == 0 && !score) return ADKF_E_BADARG;
    if ((rc = check_topk(k, top_idx, top_val))) return rc;
    if (S < 1 || S > ADKF_TS_SAMPLES_MAX) return ADKF_E_SIZE;
    const PoolScratch l = pool_scratch(scratch, b->T, k);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    PmPool pool = pm_pool(excl_idx, excl_off, k, b->T, l.cand_idx, l.cand_val, rows, c.st);
    pool.top_idx = top_idx; pool.top_val = top_val;
    PmArgs pa = pm_args(c, flags, X, rows, info);
    const MesArgs v{ystar, S, score};
    // every score starts at 0: the rows of skipped tasks (n_s == 0, info != 0) stay so
    if (score && rows > 0) hipMemsetAsync(score, 0, sizeof(float) * (size_t)rows * b->T, c.st);
    // (no scratch twin: the float64 walk runs wherever the workspace has a float64 region)
    return c.ard ? pool_select<true, MesEpilogue>(c, pa, pool, v, k_mes_walk64<true>, c.w.w64 != nullptr)
                 : pool_select<false, MesEpilogue>(c, pa, pool, v, k_mes_walk64<false>, c.w.w64 != nullptr);
}

// adkf_gibbon_pool: isotropic and ARD batches alike (as adkf_mes_pool); the scratch is the believer's, with the believer's layout
int gibbon_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* ystar, int32_t S,
                const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val, float* sel_mean,
                float* sel_var, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!ystar || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (q < 1 || S < 1) return ADKF_E_BADARG;
    if (q > ADKF_POOL_TOPK_MAX || S > ADKF_TS_SAMPLES_MAX) return ADKF_E_SIZE;
    const BvScratch l = bv_scratch(scratch, b->T, b->ns_max, b->d, q);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    hipStream_t st = c.st;
    const int T = b->T;
    PmArgs pa = pm_args(c, flags, X, rows, info);
    const bool have64 = pm_have64(c, pa);
    PmPool pool = pm_pool(excl_idx, excl_off, 1, T, l.cand.idx, l.cand.val, rows, st);
    GibbonArgs v{};
    v.b = bv_args(l, have64, q, trace, sel_idx, sel_val, sel_mean, sel_var);
    v.ystar = ystar; v.S = S;
    // skipped tasks keep zeros in trace
    if (trace && rows > 0) hipMemsetAsync(trace, 0, sizeof(float) * (size_t)T * q * (size_t)rows, st);
    // there is no incumbent: the believer's slot [T] is filled from the first T floats of ystar (S >= 1) and never read by a score
    k_bv_init<<<ceil_div(T, 256), 256, 0, st>>>(v.b, ystar, T);
    return c.ard ? pool_greedy<true, GibbonEpilogue>(c, pa, pool, v, v.b, k_gb_walk64<true>, have64)
                 : pool_greedy<false, GibbonEpilogue>(c, pa, pool, v, v.b, k_gb_walk64<false>, have64);
}

// adkf_levelset_pool: the scratch is the believer's (bv_scratch), then four 64-bit accumulators per task
struct LsScratch { BvScratch b; unsigned long long* acc; size_t bytes; };
inline LsScratch ls_scratch(void* base, int T, int ns, int d, int q) {
    LsScratch l{};
    l.b = bv_scratch(base, T, ns, d, q);
    Arena ar{static_cast<char*>(base), l.b.bytes};
    l.acc = ar.as<unsigned long long>((size_t)T * 4);
    l.bytes = ar.off;
    return l;
}

// adkf_levelset_pool: isotropic and ARD batches alike (as adkf_gibbon_pool)
int levelset_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* tau, const float* beta,
                  int32_t score, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int8_t* cls, int64_t* counts,
                  float* hits, int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, int32_t* info, void* ws, size_t ws_bytes,
                  void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (score < ADKF_LS_STRADDLE || score > ADKF_LS_BOUND) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!tau || !beta || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (q < 1) return ADKF_E_BADARG;
    if (q > ADKF_POOL_TOPK_MAX) return ADKF_E_SIZE;
    if ((counts || hits) && rows > ((int64_t)1 << 31)) return ADKF_E_SIZE;   // (below that the fixed-point sum cannot wrap)
    const LsScratch l = ls_scratch(scratch, b->T, b->ns_max, b->d, q);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    hipStream_t st = c.st;
    const int T = b->T;
    PmArgs pa = pm_args(c, flags, X, rows, info);
    const bool have64 = pm_have64(c, pa);
    PmPool pool = pm_pool(excl_idx, excl_off, 1, T, l.b.cand.idx, l.b.cand.val, rows, st);
    LsArgs v{};
    v.b = bv_args(l.b, have64, q, trace, sel_idx, sel_val, sel_mean, sel_var);
    v.tau = tau; v.beta = beta; v.kind = score; v.cls = cls;
    v.acc = (counts || hits) ? l.acc : nullptr; v.counts = counts; v.hits = hits;
    // skipped tasks keep zeros in trace, counts and hits, and "not evaluated" in cls
    if (trace && rows > 0) hipMemsetAsync(trace, 0, sizeof(float) * (size_t)T * q * (size_t)rows, st);
    if (cls && rows > 0) hipMemsetAsync(cls, 0xff, (size_t)T * (size_t)rows, st);
    if (counts) hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)T * q * 3, st);
    if (hits) hipMemsetAsync(hits, 0, sizeof(float) * (size_t)T * q, st);
    k_ls_init<<<ceil_div(T, 256), 256, 0, st>>>(v, T);
    return c.ard ? pool_greedy<true, LsEpilogue, LsEpilogue>(c, pa, pool, v, v.b, k_ls_walk64<true>, have64, k_ls_step<true>, v)
                 : pool_greedy<false, LsEpilogue, LsEpilogue>(c, pa, pool, v, v.b, k_ls_walk64<false>, have64, k_ls_step<false>, v);
}

// adkf_kg_pool: the scratch is the reference state - w [T, M, ns] (and its float64 twin where a workspace of this shape can have a
// float64 region), the entries' feature rows [T, M, d], their means [T, M] and their pool rows [T, M] (-1: a skipped entry) - and
// prediction's candidate lists [T, chunks_max, k].  It does not depend on rows.
struct KgScratch { RefHead h; float* am; int64_t* ridx; CandLists cand; size_t bytes; };
inline KgScratch kg_scratch(void* base, int T, int ns, int d, int M, int k) {
    Arena ar{static_cast<char*>(base), 0};
    KgScratch l{};
    l.h = carve_ref_head(ar, T, M, ns, d);
    l.am = ar.floats((size_t)T * M);
    l.ridx = ar.as<int64_t>((size_t)T * M);
    l.cand = carve_cand(ar, (size_t)T * pm_pool_chunks_max(T) * k);
    l.bytes = ar.off;
    return l;
}

// adkf_kg_pool: isotropic and ARD batches alike (as adkf_mes_pool)
int kg_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* ref_idx, int32_t M,
            const int64_t* excl_idx, const int64_t* excl_off, float* score, float* cov, float* ref_mean, int32_t k, int64_t* top_idx,
            float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~(ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    if (!ref_idx) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k == 0 && !score && !cov && !ref_mean) return ADKF_E_BADARG;
    if ((rc = check_topk(k, top_idx, top_val))) return rc;
    if (M < 1 || M > ADKF_KG_REFS_MAX) return ADKF_E_SIZE;
    const KgScratch l = kg_scratch(scratch, b->T, b->ns_max, b->d, M, k);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    PmPool pool = pm_pool(excl_idx, excl_off, k, b->T, l.cand.idx, l.cand.val, rows, c.st);
    pool.top_idx = top_idx; pool.top_val = top_val;
    PmArgs pa = pm_args(c, flags, X, rows, info);
    const bool have64 = pm_have64(c, pa);
    KgArgs v{};
    v.M = M; v.ref_idx = ref_idx;
    v.W = l.h.W; v.W64 = have64 ? l.h.W64 : nullptr; v.Xp = l.h.Xp; v.am = l.am; v.ridx = l.ridx;
    v.score = score; v.cov = cov; v.ref_mean = ref_mean;
    // every output starts at 0: the rows of skipped tasks (n_s == 0, info != 0) stay so
    if (score && rows > 0) hipMemsetAsync(score, 0, sizeof(float) * (size_t)rows * b->T, c.st);
    if (cov && rows > 0) hipMemsetAsync(cov, 0, sizeof(float) * (size_t)rows * b->T * M, c.st);
    return c.ard ? pool_select<true, KgEpilogue>(c, pa, pool, v, k_kg_walk64<true>, have64, k_kg_refs<true>, M)
                 : pool_select<false, KgEpilogue>(c, pa, pool, v, k_kg_walk64<false>, have64, k_kg_refs<false>, M);
}

// adkf_jes_pool: the scratch is the knowledge gradient's reference state for M = S - w [T, S, ns] (and its float64 twin where a
// workspace of this shape can have a float64 region), the entries' feature rows [T, S, d], their means and pool rows [T, S] - then the
// entries' latent variance, 1 / d_s and gain [T, S] each, the task's scale [T], and prediction's candidate lists [T, chunks_max, k].
// It does not depend on rows.
struct JesScratch { RefHead h; float *am, *ov, *invd, *gain, *scale; int64_t* ridx; CandLists cand; size_t bytes; };
inline JesScratch jes_scratch(void* base, int T, int ns, int d, int S, int k) {
    Arena ar{static_cast<char*>(base), 0};
    JesScratch l{};
    l.h = carve_ref_head(ar, T, S, ns, d);
    l.am = ar.floats((size_t)T * S);
    l.ridx = ar.as<int64_t>((size_t)T * S);
    l.ov = ar.floats((size_t)T * S);
    l.invd = ar.floats((size_t)T * S);
    l.gain = ar.floats((size_t)T * S);
    l.scale = ar.floats((size_t)T);
    l.cand = carve_cand(ar, (size_t)T * pm_pool_chunks_max(T) * k);
    l.bytes = ar.off;
    return l;
}

// adkf_jes_pool: isotropic and ARD batches alike (as adkf_kg_pool)
int jes_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* opt_idx, const float* opt_val,
             int32_t S, float cond_noise, const int64_t* excl_idx, const int64_t* excl_off, float* score, float* opt_mean, float* opt_var,
             int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes,
             void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!opt_idx || !opt_val) return ADKF_E_BADARG;
    if (!(cond_noise >= 0.f && cond_noise < INFINITY)) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k == 0 && !score && !opt_mean && !opt_var) return ADKF_E_BADARG;
    if ((rc = check_topk(k, top_idx, top_val))) return rc;
    if (S < 1 || S > ADKF_TS_SAMPLES_MAX) return ADKF_E_SIZE;
    const JesScratch l = jes_scratch(scratch, b->T, b->ns_max, b->d, S, k);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    PmPool pool = pm_pool(excl_idx, excl_off, k, b->T, l.cand.idx, l.cand.val, rows, c.st);
    pool.top_idx = top_idx; pool.top_val = top_val;
    PmArgs pa = pm_args(c, flags, X, rows, info);
    const bool have64 = pm_have64(c, pa);
    JesArgs v{};
    v.S = S; v.opt_idx = opt_idx; v.opt_val = opt_val; v.cond_noise = cond_noise;
    v.W = l.h.W; v.W64 = have64 ? l.h.W64 : nullptr; v.Xp = l.h.Xp; v.am = l.am; v.ov = l.ov; v.invd = l.invd; v.gain = l.gain; v.ridx = l.ridx;
    v.scale = l.scale;
    v.score = score; v.opt_mean = opt_mean; v.opt_var = opt_var;
    // every score starts at 0: the rows of skipped tasks (n_s == 0, info != 0) stay so
    if (score && rows > 0) hipMemsetAsync(score, 0, sizeof(float) * (size_t)rows * b->T, c.st);
    return c.ard ? pool_select<true, JesEpilogue>(c, pa, pool, v, k_jes_walk64<true>, have64, k_jes_refs<true>, S)
                 : pool_select<false, JesEpilogue>(c, pa, pool, v, k_jes_walk64<false>, have64, k_jes_refs<false>, S);
}

// adkf_ipv_pool: the scratch is the entry state - w [T, M + q, ns] (and its float64 twin where a workspace of this shape can have a
// float64 region) and the entries' feature rows [T, M + q, d], targets first - then G [T, q, q] and Lr [T, q, M] (and their twins),
// the targets' effective weights and step-0 variances [T, M], tvar, the pick count and the number of valid targets per task, and one
// (row, score) pair per (task, chunk).  It does not depend on rows.
struct IpvScratch { RefHead h; float *G, *Lr, *wt; double *G64, *Lr64, *v0r, *tv; int32_t *cnt, *nv; CandLists cand; size_t bytes; };
inline IpvScratch ipv_scratch(void* base, int T, int ns, int d, int M, int q) {
    Arena ar{static_cast<char*>(base), 0};
    const size_t g = (size_t)T * q * q, lr = (size_t)T * q * M;
    const bool twin = ns <= R64_MAXN;
    IpvScratch l{};
    l.h = carve_ref_head(ar, T, M + q, ns, d);
    l.G = ar.floats(g);
    l.G64 = ar.as<double>(twin ? g : 0);
    l.Lr = ar.floats(lr);
    l.Lr64 = ar.as<double>(twin ? lr : 0);
    l.wt = ar.floats((size_t)T * M);
    l.v0r = ar.as<double>((size_t)T * M);
    l.tv = ar.as<double>((size_t)T);
    l.cnt = ar.as<int32_t>((size_t)T);
    l.nv = ar.as<int32_t>((size_t)T);
    l.cand = carve_cand(ar, (size_t)T * pm_pool_chunks_max(T));
    l.bytes = ar.off;
    return l;
}

// The launches of a prepared adkf_ipv_pool call: (ARD) the 1 / l pass, the target state, then q chained steps, each the walks with
// IpvEpilogue and one workgroup per task (pool_greedy's shape with this entry's own step kernel)
template <bool ARD>
int ipv_launch(const PmCtx& c, PmArgs& pa, PmPool& pool, IpvArgs& v, bool have64) {
    const int T = c.b.T;
    if constexpr (ARD) launch_ard_il(c);
    k_ipv_refs<ARD><<<dim3(v.M, T), 256, 0, c.st>>>(pm_kargs<ARD, true, IpvEpilogue>(c, pa, &pool, v));
    k_ipv_init<<<ceil_div(T, 256), 256, 0, c.st>>>(v, T);
    pool.grid[2] = pool_grid64(pool, pa.rows, have64);
    for (int j = 0; j < v.q; ++j) {
        v.j = j;
        const int rc = pool_walks<ARD, IpvEpilogue>(c, pa, pool, v, k_ipv_walk64<ARD>);
        if (rc) return rc;
        k_ipv_step<ARD><<<T, 256, 0, c.st>>>(pm_kargs<ARD, true, IpvEpilogue>(c, pa, &pool, v));
    }
    LAUNCH_OK();
    return 0;
}

// adkf_ipv_pool: isotropic and ARD batches alike (as adkf_kg_pool)
int ipv_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* tgt_idx, const float* tgt_w,
             int32_t M, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val, float* tvar,
             int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!tgt_idx || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (M < 1 || q < 1) return ADKF_E_BADARG;
    if ((int64_t)M + q > ADKF_IPV_ENTRIES_MAX) return ADKF_E_SIZE;
    const IpvScratch l = ipv_scratch(scratch, b->T, b->ns_max, b->d, M, q);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    hipStream_t st = c.st;
    const int T = b->T;
    PmArgs pa = pm_args(c, flags, X, rows, info);
    const bool have64 = pm_have64(c, pa);
    PmPool pool = pm_pool(excl_idx, excl_off, 1, T, l.cand.idx, l.cand.val, rows, st);
    IpvArgs v{};
    v.M = M; v.q = q; v.tgt_idx = tgt_idx; v.tgt_w = tgt_w;
    v.W = l.h.W; v.W64 = have64 ? l.h.W64 : nullptr; v.Xp = l.h.Xp;
    v.G = l.G; v.G64 = have64 ? l.G64 : nullptr; v.Lr = l.Lr; v.Lr64 = have64 ? l.Lr64 : nullptr;
    v.wt = l.wt; v.v0r = l.v0r; v.tv = l.tv; v.cnt = l.cnt; v.nv = l.nv;
    v.trace = trace; v.sel_idx = sel_idx; v.sel_val = sel_val; v.tvar = tvar;
    // skipped tasks keep zeros in trace
    if (trace && rows > 0) hipMemsetAsync(trace, 0, sizeof(float) * (size_t)T * q * (size_t)rows, st);
    return c.ard ? ipv_launch<true>(c, pa, pool, v, have64) : ipv_launch<false>(c, pa, pool, v, have64);
}

// adkf_jackknife_pool: the scratch is the leave-one-out state - g, 1 / B_ii and the width factor [T, ns] each, with float64 twins
// (ns <= ADKF_JK_POINTS_MAX, so a workspace of this shape can always have a float64 region), the ranks [T, ADKF_JK_LEVELS_MAX] - and
// prediction's candidate lists [T, chunks_max, k].  It does not depend on rows (nor on L).
struct JkScratch { float *g, *rv, *wd; double *g64, *rv64, *wd64; int32_t* rank; CandLists cand; size_t bytes; };
inline JkScratch jk_scratch(void* base, int T, int ns, int k) {
    Arena ar{static_cast<char*>(base), 0};
    const size_t e = (size_t)T * ns;
    JkScratch l{};
    l.g = ar.floats(e); l.rv = ar.floats(e); l.wd = ar.floats(e);
    l.g64 = ar.as<double>(e); l.rv64 = ar.as<double>(e); l.wd64 = ar.as<double>(e);
    l.rank = ar.as<int32_t>((size_t)T * JK_LV_MAX);
    l.cand = carve_cand(ar, (size_t)T * pm_pool_chunks_max(T) * k);
    l.bytes = ar.off;
    return l;
}

// adkf_jackknife_pool: isotropic and ARD batches alike (as adkf_kg_pool); rows == 0 is the plain leave-one-out diagnostic
int jackknife_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* alpha, int32_t L,
                   const int64_t* excl_idx, const int64_t* excl_off, float* lo, float* hi, float* loo_mean, float* loo_var, float* loo_lpd,
                   int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes,
                   void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~(ADKF_PM_MAXIMIZE | ADKF_PM_JK_SCALED)) return ADKF_E_BADARG;
    if (!alpha) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k == 0 && !lo && !hi && !loo_mean && !loo_var && !loo_lpd) return ADKF_E_BADARG;
    if ((rc = check_topk(k, top_idx, top_val))) return rc;
    if (b->ns_max > ADKF_JK_POINTS_MAX || L < 1 || L > ADKF_JK_LEVELS_MAX) return ADKF_E_SIZE;
    const JkScratch l = jk_scratch(scratch, b->T, b->ns_max, k);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    hipStream_t st = c.st;
    const size_t T = (size_t)b->T, ns = (size_t)b->ns_max;
    PmPool pool = pm_pool(excl_idx, excl_off, k, b->T, l.cand.idx, l.cand.val, rows, st);
    pool.top_idx = top_idx; pool.top_val = top_val;
    PmArgs pa = pm_args(c, flags & ADKF_PM_MAXIMIZE, X, rows, info);
    const bool have64 = pm_have64(c, pa);
    JkArgs v{};
    v.L = L; v.scaled = (flags & ADKF_PM_JK_SCALED) ? 1 : 0; v.alpha = alpha;
    v.g = l.g; v.rv = l.rv; v.wd = l.wd; v.rank = l.rank;
    if (have64) { v.g64 = l.g64; v.rv64 = l.rv64; v.wd64 = l.wd64; }
    v.lo = lo; v.hi = hi; v.loo_mean = loo_mean; v.loo_var = loo_var; v.loo_lpd = loo_lpd;
    // every output starts at 0: the slots beyond n_s and everything of skipped tasks (n_s == 0, info != 0) stay so
    if (lo && rows > 0) hipMemsetAsync(lo, 0, sizeof(float) * T * L * (size_t)rows, st);
    if (hi && rows > 0) hipMemsetAsync(hi, 0, sizeof(float) * T * L * (size_t)rows, st);
    if (loo_mean) hipMemsetAsync(loo_mean, 0, sizeof(float) * T * ns, st);
    if (loo_var) hipMemsetAsync(loo_var, 0, sizeof(float) * T * ns, st);
    if (loo_lpd) hipMemsetAsync(loo_lpd, 0, sizeof(float) * T, st);
    return c.ard ? pool_select<true, JkEpilogue, JK_EPI_LDS>(c, pa, pool, v, k_jk_walk64<true>, have64, k_jk_state<true>, 1)
                 : pool_select<false, JkEpilogue, JK_EPI_LDS>(c, pa, pool, v, k_jk_walk64<false>, have64, k_jk_state<false>, 1);
}

// adkf_gumbel_pool: the scratch is the fixed-point sums [T, 64] (uint64), the probes [T, 64] (float32) and the images of the two
// maxima [T, 2] (uint32) - independent of rows, S and the device
struct GbScratch { unsigned long long* sums; float* probes; unsigned int* mx; size_t bytes; };
inline GbScratch gb_scratch(void* base, int T) {
    Arena ar{static_cast<char*>(base), 0};
    GbScratch l{};
    l.sums = ar.as<unsigned long long>((size_t)T * GB_PROBES);
    l.probes = ar.floats((size_t)T * GB_PROBES);
    l.mx = ar.as<unsigned int>((size_t)T * 2);
    l.bytes = ar.off;
    return l;
}

// kappa = max(1, Phi^-1(1 - 0.25 / rows)): the upper end of the bracket in deviations (gumbel_stream.h), by bisection on erfc
inline float gb_kappa(int64_t rows) {
    const double p = 0.25 / (double)std::max<int64_t>(rows, 1);
    double lo = 0.0, hi = 40.0;
    for (int it = 0; it < 100; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (0.5 * std::erfc(mid * 0.70710678118654752) > p) lo = mid; else hi = mid;
    }
    return (float)std::max(1.0, hi);
}

// The launches of a prepared Gumbel call: three walks (bracket, probe pass 1, probe pass 2), each the walks of prediction with
// GumbelEpilogue and the float64 walk, with one wave per task between them and at the end.  No host synchronisation.
template <bool ARD>
int gb_launch(const PmCtx& c, PmArgs& pa, PmPool& pool, GumbelArgs v, int64_t rows) {
    hipStream_t st = c.st;
    const int T = c.b.T;
    if (rows > 0) {
        if constexpr (ARD) launch_ard_il(c);
        for (int walk = 0; walk < 3; ++walk) {
            v.bracket = walk == 0 ? 1 : 0;
            const int rc = pool_walks<ARD, GumbelEpilogue>(c, pa, pool, v);
            if (rc) return rc;
            // (on the whole of pm64_grid: there are no lists, so pool.grid[2] stays 0 and pool_walks launches no float64 walk)
            if (c.w.w64) k_gumbel_walk64<ARD><<<dim3(pm64_grid(rows), T), PM64_NT, 0, st>>>(pm_kargs<ARD, true, GumbelEpilogue>(c, pa, &pool, v));
            if (walk < 2) k_gumbel_window<<<T, 64, 0, st>>>(v, walk);
        }
    }
    k_gumbel_fit<<<T, 64, 0, st>>>(pa, v);
    LAUNCH_OK();
    return 0;
}

// adkf_gumbel_pool: isotropic and ARD batches alike (as adkf_mes_pool)
int gumbel_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* u, int32_t S,
                float* ystar, float* quant, float* gumbel, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes,
                void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!u || !ystar) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, nullptr, nullptr)) return ADKF_E_BADARG;
    if (S < 1 || S > ADKF_TS_SAMPLES_MAX) return ADKF_E_SIZE;
    if (rows > GB_ROWS_MAX) return ADKF_E_SIZE;
    const GbScratch l = gb_scratch(scratch, b->T);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    PmPool pool = pm_pool(nullptr, nullptr, 0, b->T, nullptr, nullptr, rows, c.st);
    PmArgs pa = pm_args(c, flags, X, rows, info);
    GumbelArgs v{};
    v.probes = l.probes; v.sums = l.sums; v.mx = l.mx;
    v.kappa = gb_kappa(rows);
    v.u = u; v.S = S; v.ystar = ystar; v.quant = quant; v.gumbel = gumbel;
    // the sums and the images of the maxima start at 0 ("no row yet")
    hipMemsetAsync(scratch, 0, l.bytes, c.st);
    return c.ard ? gb_launch<true>(c, pa, pool, v, rows) : gb_launch<false>(c, pa, pool, v, rows);
}

// adkf_ehvi_pool: the scratch is stage A's mean and latent variance of one chunk of the pool, [T, EHVI_CHUNK_ROWS] each, the groups'
// state [G] and the candidate lists, one per (group, walker), at most max(PM_POOL_LISTS, G) of k entries.  It depends on neither rows,
// ns nor d, and it does not shrink when T, G or k grow.
struct EhviScratch { float *m, *v; EhviGroup* grp; CandLists cand; size_t bytes; };
inline EhviScratch ehvi_scratch(void* base, int T, int G, int k) {
    Arena ar{static_cast<char*>(base), 0};
    const size_t mv = (size_t)T * EHVI_CHUNK_ROWS, c = (size_t)std::max(PM_POOL_LISTS, G) * k;
    EhviScratch l{};
    l.m = ar.floats(mv);
    l.v = ar.floats(mv);
    l.grp = ar.as<EhviGroup>((size_t)G);
    l.cand = carve_cand(ar, c);
    l.bytes = ar.off;
    return l;
}
static_assert(EHVI_FRONT_MAX == ADKF_EHVI_FRONT_MAX && EHVI_CONS_MAX == ADKF_EHVI_CONS_MAX && EHVI_CHUNK_ROWS == ADKF_EHVI_CHUNK_ROWS &&
              EHVI_CHUNK_ROWS % PM_TM == 0, "ehvi_stream.h limits");

// The launches of a prepared EHVI call: the groups' state, then per chunk of the pool prediction's own pool launch (latent mean and
// variance into the scratch, no selection) and the scores of that chunk; at the end one wave per group merges the group's lists.
template <bool ARD>
int ehvi_launch(const PmCtx& c, EhviArgs& e, const float* X, int64_t rows, int32_t* info) {
    hipStream_t st = c.st;
    const int T = c.b.T, G = e.G, k = e.s.k;
    if (k > 0) hipMemsetAsync(e.s.cand_idx, 0xff, sizeof(int64_t) * (size_t)G * e.s.chunks_max * k, st);
    // the groups' "cannot be evaluated" flags read info and n_s here, once: pm_prepare has written info, and nothing below writes it
    // again (prediction's walks only read it), so the flags hold for every chunk
    k_ehvi_stair<<<G, 64, 0, st>>>(pm_args(c, 0, X, rows, info), e);
    // one grid for every chunk, so that a list has the same walker throughout
    const int64_t items = (int64_t)G * ((std::min<int64_t>(rows, EHVI_CHUNK_ROWS) + PM_TM - 1) / PM_TM);
    const int grid = pm_persistent_grid(k_ehvi_score, EHVI_NT, 0, std::max<int64_t>(items, 1));
    e.cpg = std::max(1, std::min(grid / G, e.s.chunks_max));
    float* m = const_cast<float*>(e.m);
    float* v = const_cast<float*>(e.v);
    for (int64_t c0 = 0; c0 < rows; c0 += EHVI_CHUNK_ROWS) {
        const int64_t L = std::min<int64_t>(EHVI_CHUNK_ROWS, rows - c0);
        PmPool none = pm_pool(nullptr, nullptr, 0, T, nullptr, nullptr, L, st);
        const PmCall io{ADKF_PM_LATENT, X + (size_t)c0 * c.b.d, nullptr, L, nullptr, m, v, nullptr, info, &none};
        // the whole of prediction's sequence per chunk, the zeroing of [T, L] and (ARD) the 1 / l pass included: a few small launches
        // per 16384 rows, the price of not having a second copy of that sequence to keep equal to it
        const int rc = pm_launch<ARD, true>(c, io);
        if (rc) return rc;
        e.c0 = c0; e.L = L;
        k_ehvi_score<<<grid, EHVI_NT, 0, st>>>(e);
    }
    if (k > 0) k_ehvi_topk<<<G, 64, 0, st>>>(e);
    LAUNCH_OK();
    return 0;
}

// adkf_ehvi_pool: isotropic and ARD batches alike (as adkf_mes_pool)
int ehvi_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, int32_t G, const int32_t* obj,
              const int32_t* obj_max, const float* ref, const float* front, const int32_t* front_n, int32_t P, const int32_t* con,
              const float* con_thr, const int32_t* con_geq, int32_t C, const int64_t* excl_idx, const int64_t* excl_off, float* score,
              float* stair, int32_t* stair_n, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes,
              void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~ADKF_PM_LOG_EI) return ADKF_E_BADARG;
    if (G < 1 || k < 0) return ADKF_E_BADARG;
    if (P < 0 || P > ADKF_EHVI_FRONT_MAX || C < 0 || C > ADKF_EHVI_CONS_MAX || k > ADKF_POOL_TOPK_MAX) return ADKF_E_SIZE;
    if (!obj || !ref || !front_n) return ADKF_E_BADARG;
    if (P > 0 && !front) return ADKF_E_BADARG;
    if (C > 0 && (!con || !con_thr || !con_geq)) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k > 0 && (!top_idx || !top_val)) return ADKF_E_BADARG;
    if (k == 0 && !score && !stair && !stair_n) return ADKF_E_BADARG;
    const EhviScratch l = ehvi_scratch(scratch, b->T, G, k);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    EhviArgs e{};
    e.G = G; e.P = P; e.C = C; e.log = (flags & ADKF_PM_LOG_EI) ? 1 : 0;
    e.obj = obj; e.obj_max = obj_max; e.ref = ref; e.front = front; e.front_n = front_n;
    e.con = con; e.con_thr = con_thr; e.con_geq = con_geq;
    e.stair = stair; e.stair_n = stair_n;
    e.grp = l.grp; e.m = l.m; e.v = l.v;
    e.rows = rows; e.score = score;
    e.s.excl_idx = excl_off ? excl_idx : nullptr; e.s.excl_off = excl_off;
    e.s.k = k; e.s.chunks_max = pm_pool_chunks_max(G);
    e.s.cand_idx = l.cand.idx; e.s.cand_val = l.cand.val;
    e.s.top_idx = top_idx; e.s.top_val = top_val;
    return c.ard ? ehvi_launch<true>(c, e, X, rows, info) : ehvi_launch<false>(c, e, X, rows, info);
}

// adkf_mix_pool: the scratch is stage A's mean, variance and EI (or log EI) of one chunk of the pool, [T, MIX_CHUNK_ROWS] each, the
// groups' state [G] and the candidate lists, one per (group, walker), at most max(PM_POOL_LISTS, G) of k entries.  It depends on
// neither rows, ns, d nor M, and it does not shrink when T, G or k grow.
struct MixScratch { float *m, *v, *e; MixGroup* grp; CandLists cand; size_t bytes; };
inline MixScratch mix_scratch(void* base, int T, int G, int k) {
    Arena ar{static_cast<char*>(base), 0};
    const size_t mv = (size_t)T * MIX_CHUNK_ROWS, c = (size_t)std::max(PM_POOL_LISTS, G) * k;
    MixScratch l{};
    l.m = ar.floats(mv);
    l.v = ar.floats(mv);
    l.e = ar.floats(mv);
    l.grp = ar.as<MixGroup>((size_t)G);
    l.cand = carve_cand(ar, c);
    l.bytes = ar.off;
    return l;
}
static_assert(MIX_MEMBERS_MAX == ADKF_MIX_MEMBERS_MAX && MIX_CHUNK_ROWS == ADKF_MIX_CHUNK_ROWS && MIX_CHUNK_ROWS % PM_TM == 0,
              "mix_stream.h limits");

// The launches of a prepared mixture call: the groups' state, then per chunk of the pool prediction's own pool launch (the members'
// mean and, where something reads them, variance and EI into the scratch, no selection) and the outputs of that chunk; at the end one
// wave per group merges the group's lists.  pm_flags: the caller's LATENT, MAXIMIZE and LOG_EI.
template <bool ARD>
int mix_launch(const PmCtx& c, MixArgs& e, int32_t pm_flags, const float* best_f, const float* X, int64_t rows, int32_t* info) {
    hipStream_t st = c.st;
    const int T = c.b.T, G = e.G, k = e.s.k;
    if (k > 0) hipMemsetAsync(e.s.cand_idx, 0xff, sizeof(int64_t) * (size_t)G * e.s.chunks_max * k, st);
    // the groups' "cannot be evaluated" flags read info and n_s here, once: pm_prepare has written info, and nothing below writes it
    // again (prediction's walks only read it), so the flags hold for every chunk
    k_mix_groups<<<G, 64, 0, st>>>(pm_args(c, 0, X, rows, info), e);
    // one grid for every chunk, so that a list has the same walker throughout
    const int64_t items = (int64_t)G * ((std::min<int64_t>(rows, MIX_CHUNK_ROWS) + PM_TM - 1) / PM_TM);
    const int grid = pm_persistent_grid(k_mix_score, MIX_NT, 0, std::max<int64_t>(items, 1));
    e.cpg = std::max(1, std::min(grid / G, e.s.chunks_max));
    float* m = const_cast<float*>(e.m);
    float* v = const_cast<float*>(e.v);
    float* ei = const_cast<float*>(e.e);
    for (int64_t c0 = 0; c0 < rows; c0 += MIX_CHUNK_ROWS) {
        const int64_t L = std::min<int64_t>(MIX_CHUNK_ROWS, rows - c0);
        PmPool none = pm_pool(nullptr, nullptr, 0, T, nullptr, nullptr, L, st);
        const PmCall io{pm_flags, X + (size_t)c0 * c.b.d, nullptr, L, best_f, m, v, ei, info, &none};
        // the whole of prediction's sequence per chunk, as ehvi_launch runs it and for its reason
        const int rc = pm_launch<ARD, true>(c, io);
        if (rc) return rc;
        e.c0 = c0; e.L = L;
        k_mix_score<<<grid, MIX_NT, 0, st>>>(e);
    }
    if (k > 0) k_mix_topk<<<G, 64, 0, st>>>(e);
    LAUNCH_OK();
    return 0;
}

// adkf_mix_pool: isotropic and ARD batches alike (as adkf_mes_pool)
int mix_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, int32_t G, const int32_t* mem,
             const float* w, int32_t M, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off, float* mean, float* var,
             float* score, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch,
             size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~(ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_SCORE_MEAN | ADKF_PM_LOG_EI | ADKF_PM_SCORE_BALD)) return ADKF_E_BADARG;
    const bool by_mean = flags & ADKF_PM_SCORE_MEAN, by_bald = flags & ADKF_PM_SCORE_BALD, lg = flags & ADKF_PM_LOG_EI;
    if ((by_mean && by_bald) || (lg && (by_mean || by_bald))) return ADKF_E_BADARG;
    if (G < 1 || M < 1 || !mem || k < 0) return ADKF_E_BADARG;
    if (M > ADKF_MIX_MEMBERS_MAX || k > ADKF_POOL_TOPK_MAX) return ADKF_E_SIZE;
    const bool want_score = score || k > 0, want_ei = want_score && !by_mean && !by_bald;
    if (want_ei && !best_f) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k > 0 && (!top_idx || !top_val)) return ADKF_E_BADARG;
    if (k == 0 && !mean && !var && !score) return ADKF_E_BADARG;
    const MixScratch l = mix_scratch(scratch, b->T, G, k);
    if ((rc = check_scratch(scratch, scratch_bytes, l.bytes))) return rc;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    MixArgs e{};
    e.G = G; e.M = M; e.maximize = (flags & ADKF_PM_MAXIMIZE) ? 1 : 0;
    e.kind = by_mean ? MIX_MEAN : by_bald ? MIX_BALD : lg ? MIX_LOG_EI : MIX_EI;
    e.mem = mem; e.w = w;
    e.grp = l.grp; e.m = l.m;
    e.v = (var || (by_bald && want_score)) ? l.v : nullptr;   // stage A writes the planes that something reads
    e.e = want_ei ? l.e : nullptr;
    e.rows = rows; e.mean = mean; e.var = var; e.score = score;
    e.s.excl_idx = excl_off ? excl_idx : nullptr; e.s.excl_off = excl_off;
    e.s.k = k; e.s.chunks_max = pm_pool_chunks_max(G);
    e.s.cand_idx = l.cand.idx; e.s.cand_val = l.cand.val;
    e.s.top_idx = top_idx; e.s.top_val = top_val;
    // prediction's flags: without an EI plane LOG_EI has no reader there (and prediction refuses nothing here: pm_launch checks no flag)
    const int32_t pm_flags = flags & (ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | (want_ei ? ADKF_PM_LOG_EI : 0));
    return c.ard ? mix_launch<true>(c, e, pm_flags, best_f, X, rows, info) : mix_launch<false>(c, e, pm_flags, best_f, X, rows, info);
}

// adkf_rank_pool: the scratch is the score plane of one chunk of the pool [T, RANK_CHUNK_ROWS], two sorted lists per task ([2, T, k]
// rows, then [2, T, k] scores) with the tasks' marks (which list is current, and its length: int32 [2, T]), the refs' rows as a packed
// query set [T * M, d] with prediction's mean and EI of them ([T * M] each) and its offsets [T + 1].  The ranks are counted in
// ref_rank and n_ranked themselves.  Every part is rounded up to 256 bytes; nothing depends on rows or ns.
struct RankScratch { float* plane; int64_t* list_idx; float* list_val; int32_t* mark; float *Xg, *gmean, *gei; int64_t* q_off; size_t bytes; };
inline RankScratch rank_scratch(void* base, int T, int k, int M, int d) {
    Arena ar{static_cast<char*>(base), 0};
    const size_t tm = (size_t)T * M;
    RankScratch l{};
    l.plane = ar.floats((size_t)T * RANK_CHUNK_ROWS);
    l.list_idx = ar.as<int64_t>((size_t)2 * T * k);
    l.list_val = ar.floats((size_t)2 * T * k);
    l.mark = ar.as<int32_t>((size_t)2 * T);
    l.Xg = ar.floats(tm * d);
    l.gmean = ar.floats(tm);
    l.gei = ar.floats(tm);
    l.q_off = ar.as<int64_t>((size_t)T + 1);
    l.bytes = ar.off;
    return l;
}
static_assert(RANK_K_MAX == ADKF_RANK_K_MAX && RANK_REFS_MAX == ADKF_RANK_REFS_MAX && RANK_CHUNK_ROWS == ADKF_RANK_CHUNK_ROWS &&
              RANK_CHUNK_ROWS % PM_TM == 0, "rank_stream.h limits");

// The launches of a prepared ranking call: the refs' rows through prediction's packed launch (M > 0), the tasks' state, then per chunk
// of the pool prediction's own pool launch (the plane the score reads into the scratch, no selection) and k_rank_chunk; at the end
// the lists go to top_*.  pm_flags: the caller's LATENT, MAXIMIZE and LOG_EI; by_mean: the score is +-mean.
template <bool ARD>
int rank_launch(const PmCtx& c, RankArgs& e, int32_t pm_flags, bool by_mean, const float* best_f, int32_t* info) {
    hipStream_t st = c.st;
    const int T = c.b.T;
    const int64_t rows = e.rows;
    if (e.M > 0) {
        k_rank_gather<<<(unsigned)((size_t)T * e.M), 64, 0, st>>>(e);
        const PmCall io{pm_flags, e.Xg, e.q_off, (int64_t)T * e.M, by_mean ? nullptr : best_f, e.gmean, nullptr, by_mean ? nullptr : e.gei, info, nullptr};
        const int rc = pm_launch<ARD, false>(c, io);
        if (rc) return rc;
    }
    // (info and n_s are read here and in every chunk: pm_prepare has written info, and nothing below writes it again)
    const PmArgs pa = pm_args(c, 0, e.X, rows, info);
    k_rank_refs<<<T, RANK_NT, 0, st>>>(pa, e);
    float* plane = const_cast<float*>(e.plane);
    for (int64_t c0 = 0; c0 < rows; c0 += RANK_CHUNK_ROWS) {
        const int64_t L = std::min<int64_t>(RANK_CHUNK_ROWS, rows - c0);
        PmPool none = pm_pool(nullptr, nullptr, 0, T, nullptr, nullptr, L, st);
        const PmCall io{pm_flags, e.X + (size_t)c0 * c.b.d, nullptr, L, by_mean ? nullptr : best_f, by_mean ? plane : nullptr, nullptr,
                        by_mean ? nullptr : plane, info, &none};
        // the whole of prediction's sequence per chunk, as ehvi_launch runs it and for its reason
        const int rc = pm_launch<ARD, true>(c, io);
        if (rc) return rc;
        e.c0 = c0; e.L = L;
        k_rank_chunk<<<T, RANK_NT, 0, st>>>(pa, e);
    }
    if (e.k > 0) k_rank_finish<<<T, RANK_NT, 0, st>>>(e);
    LAUNCH_OK();
    return 0;
}

// adkf_rank_pool: isotropic and ARD batches alike (as adkf_mix_pool)
int rank_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f, const int64_t* excl_idx,
              const int64_t* excl_off, int32_t k, int64_t* top_idx, float* top_val, const int64_t* ref_idx, int32_t M, int64_t* ref_rank,
              float* ref_val, int64_t* n_ranked, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_support_only(b, phi, info, ws, rows);
    if (rc) return rc;
    if (flags & ~(ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_SCORE_MEAN | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    const bool by_mean = flags & ADKF_PM_SCORE_MEAN;
    if (by_mean && (flags & ADKF_PM_LOG_EI)) return ADKF_E_BADARG;   // nothing would read it
    if (k < 0 || M < 0) return ADKF_E_BADARG;
    if (k > ADKF_RANK_K_MAX || M > ADKF_RANK_REFS_MAX) return ADKF_E_SIZE;
    if (!by_mean && !best_f) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k > 0 && (!top_idx || !top_val)) return ADKF_E_BADARG;
    if (M > 0 && (!ref_idx || !ref_rank || !ref_val)) return ADKF_E_BADARG;
    if (k == 0 && M == 0 && !n_ranked) return ADKF_E_BADARG;
    const RankScratch l = rank_scratch(scratch, b->T, k, M, b->d);
    if (!scratch) return ADKF_E_BADARG;
    // (a misaligned scratch is a short one here: its aligned part does not hold the bytes)
    if (scratch_bytes < l.bytes || (reinterpret_cast<uintptr_t>(scratch) & 7u)) return ADKF_E_WORKSPACE;
    PmCtx c;
    rc = pm_prepare(b, phi, info, ws, ws_bytes, stream, c);
    if (rc) return rc;
    RankArgs e{};
    e.T = b->T; e.k = k; e.M = M;
    e.neg = (by_mean && !(flags & ADKF_PM_MAXIMIZE)) ? 1 : 0;
    e.count = (M > 0 || n_ranked) ? 1 : 0;
    e.plane = l.plane; e.rows = rows;
    e.excl_idx = excl_off ? excl_idx : nullptr; e.excl_off = excl_off;
    e.list_idx = l.list_idx; e.list_val = l.list_val; e.cur = l.mark; e.cnt = l.mark + b->T;
    e.ref_idx = ref_idx; e.ref_rank = ref_rank; e.ref_val = ref_val; e.n_ranked = n_ranked;
    e.top_idx = top_idx; e.top_val = top_val;
    e.X = X; e.d = b->d; e.Xg = l.Xg; e.gmean = l.gmean; e.gei = by_mean ? nullptr : l.gei; e.q_off = l.q_off;
    // prediction's flags: the mean score reads no EI plane (and prediction refuses nothing here: pm_launch checks no flag)
    const int32_t pm_flags = flags & (ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI);
    return c.ard ? rank_launch<true>(c, e, pm_flags, by_mean, best_f, info) : rank_launch<false>(c, e, pm_flags, by_mean, best_f, info);
}

}  // namespace
