// Streaming marginal prediction (adkf_predict_marginal): mean, variance and Expected Improvement of PACKED query rows against
// a fitted support set, for query sets of any size, in a workspace that does not depend on the number of rows.
//
// Work items are (task, 64-row query tile); a persistent grid walks them in order, every workgroup finding the task of its
// tile from the row offsets q_off[T + 1] (clamped to [0, rows): bad offsets cannot make it read or write out of bounds).
// Per tile, for each 64-column panel of the support set:
//     D^2 = |q|^2 + |s|^2 - 2 q.s on the FP32 MFMA, the query rows centred with the support column mean (as ProbDist), the row
//           norms summed while the operands are staged;
//     K   = os kappa(D^2 / l^2)                              -> a [64, ns] row tile in LDS (or a global slot, see below)
// then C = K A^-1 panel by panel (A^-1 rows through L2), reduced on the fly to mean_i = sum_j C_ij y_j and
// var_i = os - sum_j C_ij K_ij (as k_predict), EI in the epilogue, 4 to 12 bytes written per row.  Nothing of size rows x ns
// ever goes to HBM.
//
// Tasks that ProbCres / ProbCfix refine in adkf_predict - more than 128 points, or (s + noise) max diag(A^-1) above the float32
// refinement threshold - take REFINE = true: the same one step C' = C + R A^-1 with R = K - C A (A generated from D2ss), applied
// to the two reductions directly:
//     C' y = C y + R (A^-1 y)        and        sum_j C'_ij K_ij = sum_j C_ij K_ij + sum_k R_ik C_ik
// (the second because (R A^-1) K_i^T = R (A^-1 K_i^T) = R C_i^T for the symmetric A^-1; the correction terms are of the size of
// the residual, so this reassociation changes them by a relative eps32 only).  That keeps C as one more row tile and A^-1 y as
// a vector, and saves ProbCfix's product.  The two kinds of task run in two launches of the same kernel (each skips the other's
// tasks), so the common one needs one row tile of LDS only.  Row tiles that do not fit in LDS (beyond 512 points plain, 256
// refined) live in per-workgroup slots carved from workspace regions prediction does not read (host_stream.h: pm_slot_regions);
// the grid is then as large as the number of slots - correct, not tuned.
//
// Per 64-column support panel the 64 x d query tile is streamed (and its norms summed) again: ns / 64 times per tile.  At
// ns <= 64 that is once; beyond, it is the price of not holding a [64, d] tile (512 KB at d = 2048) in LDS.
//
// Rows that belong to no task's range, and the rows of tasks with n_s == 0 or info != 0, are written as 0 (the host zeroes the
// outputs first; the kernels skip such tasks).
//
// Tasks flagged for the float64 path (refine64.h) are skipped here; k_predict_marginal64 evaluates their rows in float64 from the features,
// against the float64 A^-1 and alpha k_refine64 left in the workspace.
//
// ARD batches (adkf_predict_marginal_ard) run the same kernels on the scaled features z~ = (z - mu) / l of ard.h at unit
// lengthscale (ARD = true): the support rows are ard.h's Zt_s, centred and scaled already; the query rows cannot be scaled into a
// buffer (their number is unbounded), so they are scaled while they are staged, (z - mu) * il with il = 1 / l computed once per
// call (k_pm_ard_il; ard_scaled_il).  k_predict_marginal64<true> scales with k_ard_scale's own function, ard_scaled: (z - mu) / l in
// float32, then promoted to float64, so a flagged task's rows see the features ARD adkf_predict would give them.
//
// Shared pool (adkf_predict_pool, POOL = true): every task scores the SAME rows X [rows, d].  An item is (task, pool tile);
// the row source is X + r * d for every task and the destination t * rows + r.  Every workgroup counts the tasks of its
// launch's kind and spreads the grid over them: workgroup w serves the (w % n)-th such task and walks the tiles w / n,
// w / n + C, ... with C = min(grid / n, chunks_max) chunks per task, so the items of one pool tile for different tasks are
// neighbours in time (the tile comes from HBM once) and a workgroup serves one task per walk; with more tasks than workgroups
// it serves several, one after the other.  Nothing depends on that placement but speed.  The arithmetic of an item is the
// packed call's, bit for bit.
//
// Selection (k > 0): the first wave, which holds the tile's 64 scores in the epilogue, keeps the best 64 (score, row) pairs
// of its walk in registers, one per lane, sorted under the total order "larger score first, equal scores by ascending row"
// (pm_list_merge: a threshold test against the k-th entry first, a binary search of the task's exclusion list for the rows that
// pass it, then one shift per accepted row).  At the end of the walk the first k go to the scratch list of (task, chunk) with
// ordinary stores; k_pool_topk, one wave per task after the three walks, merges the task's C lists under the same order.  The
// answer is unique, so it does not depend on the grid.  NaN scores are never selected.
//
// Deterministic: no atomics; a row's result depends on its task's data and its own features only.
//
// Shared with thompson_stream.h, so that "pool = packed", "a task's numbers do not depend on the grid" and "Thompson's K is
// prediction's K" hold by construction: the kernel arguments (PmArgs + the optional groups PmArd and PmPool), the pool walk
// (PmPoolWalk, pm_task_chunks, pm_list_store), the K panel (pm_query_rows, pm_k_panel), and for flagged tasks the preamble of a float64
// kernel (Pm64Task, filled by pm64_task: k_predict_marginal64, k_ts_stream64, k_bv_walk64), the float64 kernel row (pm64_kernel_row:
// k_ts_stream64, and pm64_posterior_row) and the end of a float64 walk (pm64_finish_walk, the three kernels again: the waves' lists
// through the caller's merge - pm_list_merge here and in the believer, a compare of pairs in Thompson - then the store by the first wave).
//
// Shared with believer_stream.h: the float64 posterior of one pool row (pm64_posterior_row: the kernel row, c = k A^-1, c . y and c . k
// summed in one order - k_predict_marginal64 and k_bv_walk64), the merge of a task's lists (pm_merge_task_lists: k_pool_topk at width
// k, k_bv_step at width 1; k_ts_merge is a compare per lane, another shape), and k_predict_marginal itself.  What a tile's rows become once the K row tile and the two reductions
// are in place is the template parameter EPI: PmRowEpilogue (the default) writes prediction's outputs and merges the scores;
// BvEpilogue downdates the variance with the picks made so far before it scores; MesEpilogue (mes_stream.h) scores every row against
// max-value samples with all four waves; GumbelEpilogue (gumbel_stream.h) reduces the tile's rows to two maxima or 64 fixed-point sums
// per task; GibbonEpilogue (gibbon_stream.h) runs the believer's downdate and then MES's four-wave sum of the GIBBON terms.  The instances of the default are the kernels as they were, arithmetic and order.
//
// Shared by every pool acquisition (believer, MES, GIBBON, KG, JES, Gumbel), each described once, where it is defined: the head and
// tail of a tile epilogue (PmTile::mean / ck / var / is_nan, pm_sum4, pm_excl, pm_tile_tail, next to PmTile) and the float64 walk
// (pm64_rows, pm64_pool_walk, next to pm64_finish_walk).  Thompson's float64 kernel stays apart: it merges S lists, and
// Pm64Task::il2 says why its kernel row is not this one's.
#pragma once
#include <type_traits>

#include "refine64.h"

namespace adkf {

constexpr int PM_TM = 64;                   // query rows per tile (and support columns per panel)
constexpr int PM_NT = 256;
constexpr int PM_LDS_BYTES = 160 * 1024;

struct PmArgs {
    const float *Zq, *Zs, *mean_s;          // packed query rows [rows, d]; support [T, ns_ld, d]; support column means [T, d]
    const int64_t* q_off; int64_t rows;
    const int32_t* n_s; int ns_ld, d, kind, T;
    const float *Ainv, *D2ss, *y_s, *scal;
    const float* best_f;
    float *mean, *var, *ei;
    float* slots[2]; int slot_count[2];     // global row-tile slots (GLOBAL instances): two regions, slot_floats each
    size_t slot_floats;
    const int32_t* info;                    // tasks with info != 0 (failed factorisation) are skipped: their rows stay 0
    float refine_thresh, r64_thresh;        // r64_thresh: +inf when the workspace has no float64 region
    int latent, maximize, log_ei, vec;      // log_ei: the ei array and the EI score hold log EI (pm_log_ei)
    int buf_ld;                             // leading dimension of a row tile
    const double* w64; size_t w64_stride;   // the float64 region of refine64.h (the float64 kernels)
};

// the ARD instances: PmArgs::Zs is Zt_s, PmArgs::mean_s the support column means mu of ard.h
struct PmArd { const float *il, *ell; };   // [T, d] each: 1 / l and l
// the shared-pool instances (POOL): PmArgs::Zq is the pool X, q_off unused, mean / var / ei [T, rows] and each nullable
struct PmPool {
    const int64_t *excl_idx, *excl_off;     // nullable: task t may not select rows excl_idx[excl_off[t] .. excl_off[t + 1]), ascending
    int64_t* cand_idx; float* cand_val;     // scratch lists [T, chunks_max, k]
    int k, chunks_max, score_mean;
    int grid[3];                            // the grids of the three walks (pm_task_chunks derives the chunks per task from them)
    int64_t* top_idx; float* top_val;       // the selection [T, k]
    int walked;                             // rows > 0: the walks ran
};
// what a kernel receives: the groups its instance does not have are empty
struct PmNoArd {};
struct PmNoPool {};
struct PmNoEpilogueArgs {};
struct PmRowEpilogue;
// EPI: what a tile's rows become once their two reductions are done (PmRowEpilogue: the outputs of prediction); v: its arguments
template <bool ARD, bool POOL = false, class EPI = PmRowEpilogue>
struct PmArgsOf { PmArgs p; std::conditional_t<ARD, PmArd, PmNoArd> r; std::conditional_t<POOL, PmPool, PmNoPool> s; typename EPI::Args v; };

// il = 1 / l, so that the staging loop of the ARD instances multiplies instead of divides
__global__ __launch_bounds__(256) void k_pm_ard_il(const float* ell, float* il, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) il[i] = 1.f / ell[i];
}

__device__ __forceinline__ int pm_ns(const PmArgs& a, int t) {
    const int n = a.n_s ? a.n_s[t] : a.ns_ld;
    return n < 0 ? 0 : (n > a.ns_ld ? a.ns_ld : n);
}
__device__ __forceinline__ void pm_range(const PmArgs& a, int t, int64_t& lo, int64_t& hi) {
    lo = a.q_off[t]; hi = a.q_off[t + 1];
    lo = lo < 0 ? 0 : (lo > a.rows ? a.rows : lo);
    hi = hi < lo ? lo : (hi > a.rows ? a.rows : hi);
}
// which of the three evaluations owns task t: 0 plain, 1 refined C (the gate of ProbCres / ProbCfix), 2 float64; -1 nobody
__device__ __forceinline__ int pm_kind_of(const PmArgs& a, int t) {
    if (a.info[t] != 0 || pm_ns(a, t) <= 0) return -1;
    const float* sc = a.scal + (size_t)t * NSCAL;
    if (sc[S_PIVR_A] > a.r64_thresh) return 2;
    return (a.ns_ld > 128 || sc[S_CONDA] > a.refine_thresh) ? 1 : 0;
}

// acc[2][2] (this wave's 32 x 32 quarter of a 64 x 64 panel) = sum_k A(i, k) B(j, k), both operands K-contiguous, staged
// through LDS in GK-wide chunks: fa4(i, k, v) / fb4(j, k, v) fill four consecutive k (zero outside their ranges).  SQ: the
// sums of squares of the staged rows of A and B are accumulated in sqa / sqb (ProbDist's norms).
template <bool SQ, class FA, class FB>
__device__ __forceinline__ void pm_mm(f32x4 (&acc)[2][2], int K, float* As, float* Bs, FA fa4, FB fb4, float (&sqa)[2], float (&sqb)[2]) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wr = wv >> 1, wc = wv & 1, fi = lane & 15, fk = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float ra[2][4], rb[2][4];
    auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int r = (tid >> 3) + ps * 32, k = k0 + (tid & 7) * 4;
            fa4(r, k, ra[ps]);
            fb4(r, k, rb[ps]);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += GK) {
#pragma unroll
        for (int ps = 0; ps < 2; ++ps)
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int r = (tid >> 3) + ps * 32;
                As[r * LD_MN + (tid & 7) * 4 + x] = ra[ps][x];
                Bs[r * LD_MN + (tid & 7) * 4 + x] = rb[ps][x];
                if constexpr (SQ) { sqa[ps] = fmaf(ra[ps][x], ra[ps][x], sqa[ps]); sqb[ps] = fmaf(rb[ps][x], rb[ps][x], sqb[ps]); }
            }
        __syncthreads();
        if (k0 + GK < K) fetch(k0 + GK);   // next chunk's loads fly while this one is multiplied
#pragma unroll
        for (int s = 0; s < GK / 4; ++s) {
            float af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = As[(wr * 32 + i * 16 + fi) * LD_MN + 4 * s + fk];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Bs[(wc * 32 + j * 16 + fi) * LD_MN + 4 * s + fk];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
}

// the element (row, column) of a 64 x 64 panel that acc[i][j][r] holds (C/D map of the 16 x 16 MFMA)
__device__ __forceinline__ int pm_row(int i, int r) { const int lane = threadIdx.x & 63, wr = (threadIdx.x >> 6) >> 1; return wr * 32 + i * 16 + (lane >> 4) * 4 + r; }
__device__ __forceinline__ int pm_col(int j) { const int lane = threadIdx.x & 63, wc = (threadIdx.x >> 6) & 1; return wc * 32 + j * 16 + (lane & 15); }

// four consecutive entries of a K-contiguous row (zero beyond k_end); vec: 16-byte loads are legal
__device__ __forceinline__ void pm_ld4(const float* row, int k, int k_end, bool vec, float (&v)[4]) {
    if (vec && k + 3 < k_end) { const float4 q = *reinterpret_cast<const float4*>(row + k); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; return; }
#pragma unroll
    for (int x = 0; x < 4; ++x) v[x] = k + x < k_end ? row[k + x] : 0.f;
}

// EI from the latent variance: sigma (u Phi(u) + phi(u)), u = +-(best_f - mean) / sigma; Phi through erfc (tails keep their digits)
__device__ __forceinline__ float pm_ei(float mean, float var_latent, float best, int maximize) {
    const float sigma = sqrtf(fmaxf(var_latent, 1e-12f));
    const float u = (maximize ? (mean - best) : (best - mean)) / sigma;
    const float cdf = 0.5f * erfcf(-u * 0.70710678118654752f);
    const float pdf = 0.3989422804014327f * expf(-0.5f * u * u);
    return sigma * fmaf(u, cdf, pdf);
}

// log EI = log sigma + log h(u), h(u) = phi(u) + u Phi(u), with pm_ei's sigma and u, never through EI (Ament et al. 2023): finite
// wherever u * u is, -inf where it overflows at u < 0.  h is formed only where it neither cancels nor underflows, u > -1.  Below,
// with a = -u,
//     h(u) = phi(u) b(a),    b(a) = 1 - a sqrt(pi / 2) erfcx(a / sqrt 2) = a^-2 (1 - 3 a^-2 + 15 a^-4 - 105 a^-6 + 945 a^-8 - ...),
// the first form down to u = -12 (b cancels to ~a^-2: an absolute error of a few eps32 a^2 in the logarithm, the size u's own
// rounding gives it), the series beyond (its first omitted term is 1.7e-7 at a = 12).  A NaN mean gives NaN.
// Not inlined: one call per row, and the temporaries of erfcxf and the logarithms stay out of the kernels' register budget (inlined,
// every instance gains 3 VGPRs and the plain ARD pool instance drops from 3 waves per SIMD to 2).
__device__ __noinline__ float pm_log_ei(float mean, float var_latent, float best, int maximize) {
    const float sigma = sqrtf(fmaxf(var_latent, 1e-12f));
    const float u = (maximize ? (mean - best) : (best - mean)) / sigma;
    float lh;
    if (u > -1.f) {
        const float cdf = 0.5f * erfcf(-u * 0.70710678118654752f);
        const float pdf = 0.3989422804014327f * expf(-0.5f * u * u);
        lh = logf(fmaf(u, cdf, pdf));
    } else {
        const float a = -u, a2 = a * a;
        float lb;
        if (u > -12.f) {
            lb = logf(fmaf(-(a * 1.2533141373155003f), erfcxf(a * 0.70710678118654752f), 1.f));
        } else {
            const float w = 1.f / a2;   // 0 once a * a overflows: the series is 1, and -a^2 / 2 = -inf decides
            lb = logf(fmaf(fmaf(fmaf(fmaf(945.f, w, -105.f), w, 15.f), w, -3.f), w, 1.f)) - 2.f * logf(a);
        }
        lh = (lb - 0.9189385332046727f) - 0.5f * a2;
    }
    return logf(sigma) + lh;
}

// ---- shared-pool selection
constexpr int PM_TOPK_MAX = 64;             // one list entry per lane

// (s, r) comes before the list entry (v, i) in the total order; empty entries (i < 0) come last
__device__ __forceinline__ bool pm_beats(float s, long long r, float v, long long i) { return i < 0 || s > v || (s == v && r < i); }

__device__ __forceinline__ bool pm_excluded(const PmPool& s, int t, long long r) {
    if (!s.excl_idx) return false;
    int64_t lo = s.excl_off[t], hi = s.excl_off[t + 1];
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t v = s.excl_idx[mid];
        if (v == r) return true;
        if (v < r) lo = mid + 1; else hi = mid;
    }
    return false;
}

// One wave: (lv, li) is the sorted list, entry `lane` in each lane; every lane offers one candidate (s, r) if `valid`.
// Candidates that do not beat the k-th entry, NaN scores and rows for which excl(r) holds are dropped; the rest are inserted one
// by one (wave-uniform control flow).
template <class EX>
__device__ __forceinline__ void pm_list_merge(float& lv, long long& li, int k, float s, long long r, bool valid, EX excl) {
    const int lane = threadIdx.x & 63;
    // the k-th entry is read by every lane, outside the test: a shuffle behind `valid &&` runs with the invalid lanes switched off, and
    // reads 0 from lane k - 1 when that lane is one of them (fewer candidates than k) - only positive scores then passed
    const float kv = __shfl(lv, k - 1);
    const long long ki = __shfl(li, k - 1);
    bool pass = valid && s == s && pm_beats(s, r, kv, ki);
    if (pass) pass = !excl(r);
    unsigned long long mask = __ballot(pass);
    while (mask) {
        const int l = __ffsll(mask) - 1;
        mask &= mask - 1;
        const float cs = __shfl(s, l);
        const long long cr = __shfl(r, l);
        if (!pm_beats(cs, cr, __shfl(lv, k - 1), __shfl(li, k - 1))) continue;   // the threshold has moved since the test above
        const int pos = __popcll(__ballot(!pm_beats(cs, cr, lv, li)));            // the entries that stay ahead are a prefix
        const float uv = __shfl_up(lv, 1);
        const long long ui = __shfl_up(li, 1);
        if (lane == pos) { lv = cs; li = cr; }
        else if (lane > pos) { lv = uv; li = ui; }
    }
}

// the chunks per task of a walk of `grid` workgroups over n tasks
__device__ __forceinline__ int pm_pool_chunks(int grid, int n, int chunks_max) {
    const int c = n > 0 ? grid / n : 0;
    return c < 1 ? 1 : (c > chunks_max ? chunks_max : c);
}
// a walk serves the tasks whose kind (pm_kind_of) is in the bit mask `kinds`: 1 plain, 2 refined, 3 both (thompson_stream.h)
__device__ __forceinline__ bool pm_owns(const PmArgs& a, int t, int kinds) {
    const int kind = pm_kind_of(a, t);
    return kind >= 0 && ((kinds >> kind) & 1);
}
__device__ __forceinline__ int pm_count_kinds(const PmArgs& a, int kinds) {
    int n = 0;
    for (int u = 0; u < a.T; ++u) n += pm_owns(a, u, kinds) ? 1 : 0;
    return n;
}
// how many of task t's lists were written (0: skipped task, or no walk ran).  split: the float32 tasks were walked by kind, grid[0]
// the plain ones and grid[1] the refined (prediction); otherwise in one walk, grid[0] (Thompson).  grid[2]: the float64 kernel.
__device__ __forceinline__ int pm_task_chunks(const PmArgs& a, const PmPool& s, int t, bool split) {
    const int kind = s.walked ? pm_kind_of(a, t) : -1;
    if (kind < 0) return 0;
    if (kind == 2) return s.grid[2];
    return pm_pool_chunks(s.grid[split ? kind : 0], pm_count_kinds(a, split ? 1 << kind : 3), s.chunks_max);
}
// entry `lane` of the list of (task, chunk), a list of `width` entries (PmPool::k)
__device__ __forceinline__ void pm_list_store(const PmPool& s, int t, int chunk, int lane, int width, float lv, long long li) {
    if (lane < width) {
        const size_t e = ((size_t)t * s.chunks_max + chunk) * width + lane;
        s.cand_idx[e] = li; s.cand_val[e] = lv;
    }
}

// one wave: the `total` scratch entries from `base` on - whole lists of `width` entries - merged under the total order into (lv, li),
// entry `lane` in each lane (nothing listed: -inf / -1).  pm_merge_task_lists: the lists of task t that the walks of prediction wrote
// (a skipped task, and every task when no walk ran, has none)
__device__ __forceinline__ void pm_merge_lists(const PmPool& s, size_t base, int total, int width, float& lv, long long& li) {
    const int lane = threadIdx.x & 63;
    lv = -INFINITY; li = -1;
    for (int e0 = 0; e0 < total; e0 += 64) {
        const int e = e0 + lane;
        const bool in = e < total;
        const long long r = in ? (long long)s.cand_idx[base + e] : -1;
        const float v = in ? s.cand_val[base + e] : 0.f;
        pm_list_merge(lv, li, width, v, r, r >= 0, [](long long) { return false; });
    }
}
__device__ __forceinline__ void pm_merge_task_lists(const PmArgs& a, const PmPool& s, int t, int width, float& lv, long long& li) {
    pm_merge_lists(s, (size_t)t * s.chunks_max * width, pm_task_chunks(a, s, t, true) * width, width, lv, li);
}
// one wave per GROUP of a call that combines tasks (k_ehvi_topk, k_mix_topk): the `lists` lists of k entries that the group's walkers
// wrote (none without rows) merged into top_idx / top_val [G, k] (nothing listed: -1 / -inf)
__device__ __forceinline__ void pm_group_topk(const PmPool& s, int g, int lists) {
    const int lane = threadIdx.x & 63, k = s.k;
    float lv;
    long long li;
    pm_merge_lists(s, (size_t)g * s.chunks_max * k, lists * k, k, lv, li);
    if (lane < k) { s.top_idx[(size_t)g * k + lane] = li; s.top_val[(size_t)g * k + lane] = li >= 0 ? lv : -INFINITY; }
}

// The walk of one workgroup over a shared pool (see the top of the file): a (task, chunk, tile) cursor that only moves forward,
// and the list (lv, li) of the task it is at, one entry per lane of the first wave, which it stores when it leaves the task.
template <int KINDS>
struct PmPoolWalk {
    int pn, pC, pchunk, pj, pt, grid;
    int64_t ptile, pntiles;
    float lv;
    long long li;
    // false: nothing for this workgroup (uniform)
    __device__ __forceinline__ bool start(const PmArgs& a, const PmPool& s) {
        pt = -1; ptile = 0; lv = -INFINITY; li = -1;   // pt < 0 before the first task
        grid = gridDim.x;
        pn = pm_count_kinds(a, KINDS);
        if (pn == 0) return false;
        pC = pm_pool_chunks(grid, pn, s.chunks_max);
        pchunk = blockIdx.x / pn; pj = blockIdx.x % pn;
        pntiles = (a.rows + PM_TM - 1) / PM_TM;
        return pchunk < pC;
    }
    // the next item: task t, first row r0; false at the end of the walk (uniform).  width: the entries of a list (PmPool::k)
    __device__ __forceinline__ bool next(const PmArgs& a, const PmPool& s, int width, int& t, int64_t& r0) {
        while (pt < 0 || ptile >= pntiles) {   // the next task of this walk
            if (pt >= 0) {
                pm_list_store(s, pt, pchunk, threadIdx.x, width, lv, li);
                pj += grid;
            }
            if (pj >= pn) return false;
            int seen = 0;
            for (pt = 0; pt < a.T; ++pt)
                if (pm_owns(a, pt, KINDS) && seen++ == pj) break;
            if (pt >= a.T) return false;   // (cannot happen: pj < pn)
            ptile = pchunk; lv = -INFINITY; li = -1;
        }
        t = pt; r0 = ptile * PM_TM; ptile += pC;
        return true;
    }
};

// ---- the K panel
// the staging of m query rows from r0 on, centred with mu (ARD: and scaled with il), as the A operand of pm_mm
template <bool ARD>
__device__ __forceinline__ auto pm_query_rows(const PmArgs& a, const float* mu, const float* il, int64_t r0, int m) {
    return [&a, mu, il, r0, m](int i, int k, float (&v)[4]) {
        if (i >= m) { v[0] = v[1] = v[2] = v[3] = 0.f; return; }
        const int64_t d = a.d;
        float z[4], c[4];
        pm_ld4(a.Zq + (size_t)(r0 + i) * d, k, a.d, a.vec, z); pm_ld4(mu, k, a.d, a.vec, c);
        if constexpr (ARD) {
            float s[4];
            pm_ld4(il, k, a.d, a.vec, s);
#pragma unroll
            for (int x = 0; x < 4; ++x) v[x] = ard_scaled_il(z[x], c[x], s[x]);
        } else {
#pragma unroll
            for (int x = 0; x < 4; ++x) v[x] = z[x] - c[x];
        }
    };
}

// dst[i * ldd + j] = os kappa(|q_i - s_(j0 + j)|^2 il2) for the [64, 64] panel of query rows r0 .. r0 + m against the support rows
// j0 .. j0 + 64 of Zs [n, d] (zero outside): the centred product and the row norms through pm_mm<true>, the norms of a row summed
// over the eight lanes that staged it (acc: the caller's accumulator tile, free for reuse afterwards).  before_sync() runs between
// the stores of the norms and the barrier that publishes them.
template <bool ARD, class FN>
__device__ __forceinline__ void pm_k_panel(const PmArgs& a, const float* Zs, const float* mu, const float* il, int64_t r0, int m, int n, int j0,
                                           float os, float il2, float* As, float* Bs, float (&rowsq)[2][PM_TM], f32x4 (&acc)[2][2],
                                           float* dst, size_t ldd, FN before_sync) {
    const int tid = threadIdx.x, kind = a.kind;
    const int64_t d = a.d;
    float sqa[2] = {0.f, 0.f}, sqb[2] = {0.f, 0.f};
    pm_mm<true>(acc, a.d, As, Bs, pm_query_rows<ARD>(a, mu, il, r0, m),
        [&](int j, int k, float (&v)[4]) {
            if (j0 + j >= n) { v[0] = v[1] = v[2] = v[3] = 0.f; return; }
            if constexpr (ARD) {   // Zt_s: centred and scaled already
                pm_ld4(Zs + (size_t)(j0 + j) * d, k, a.d, a.vec, v);
            } else {
                float z[4], c[4];
                pm_ld4(Zs + (size_t)(j0 + j) * d, k, a.d, a.vec, z); pm_ld4(mu, k, a.d, a.vec, c);
#pragma unroll
                for (int x = 0; x < 4; ++x) v[x] = z[x] - c[x];
            }
        }, sqa, sqb);
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {   // the eight threads that staged a row are eight adjacent lanes
        float x = sqa[ps], y = sqb[ps];
        x += dpp_f<DPP_XOR1>(x); x += dpp_f<DPP_XOR2>(x); x += dpp_f<DPP_HALF_MIRROR>(x);
        y += dpp_f<DPP_XOR1>(y); y += dpp_f<DPP_XOR2>(y); y += dpp_f<DPP_HALF_MIRROR>(y);
        if ((tid & 7) == 0) { rowsq[0][(tid >> 3) + ps * 32] = x; rowsq[1][(tid >> 3) + ps * 32] = y; }
    }
    before_sync();
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ii = pm_row(i, r), jj = pm_col(j);
                const float d2 = fmaxf(rowsq[0][ii] + rowsq[1][jj] - 2.f * acc[i][j][r], 0.f);
                dst[(size_t)ii * ldd + jj] = (ii < m && j0 + jj < n) ? os * kappa0(kind, d2 * il2) : 0.f;
            }
    __syncthreads();
}

// ---- the outputs of one row (both prediction kernels): mean, the latent variance vl or the observed one vo, EI (PmArgs::log_ei:
// log EI); returns the row's selection score (POOL)
template <bool POOL, class ARGS>
__device__ __forceinline__ float pm_row_out(const ARGS& args, int t, int64_t r, float mean, float vl, float vo) {
    const PmArgs& a = args.p;
    const size_t row = POOL ? (size_t)t * (size_t)a.rows + (size_t)r : (size_t)r;
    if (!POOL || a.mean) a.mean[row] = mean;
    if (a.var) a.var[row] = a.latent ? vl : vo;
    if constexpr (POOL) {
        const bool by_mean = args.s.score_mean != 0;
        float e = 0.f;
        if (a.ei || (args.s.k > 0 && !by_mean))
            e = a.log_ei ? pm_log_ei(mean, vl, a.best_f[t], a.maximize) : pm_ei(mean, vl, a.best_f[t], a.maximize);
        if (a.ei) a.ei[row] = e;
        return by_mean ? (a.maximize ? mean : -mean) : e;
    } else {
        if (a.ei) a.ei[row] = a.log_ei ? pm_log_ei(mean, vl, a.best_f[t], a.maximize) : pm_ei(mean, vl, a.best_f[t], a.maximize);
        return 0.f;
    }
}

// ---- one tile of k_predict_marginal when its epilogue runs: the K row tile and the two reductions are in place
struct PmTile {
    int t; int64_t r0;                      // the task and the tile's first row
    int m, n, nk, ld;                       // rows of the tile, support points, their padded extent, leading dimension of Kb
    float os, noise, il2;
    const float *mu, *il;                   // the centring (ARD: and scaling) of the query rows
    const float* Kb;                        // the K row tile [64, ld], zero beyond (m, n)
    float *As, *Bs;                         // pm_mm's staging buffers, ADJACENT (2 * PM_TM * LD_MN floats from As) and free
    float (*rowsq)[2][PM_TM];
    float (*red)[2][PM_TM];                 // red[wc][0 | 1][row]: the halves of sum_j C_ij y_j and sum_j C_ij K_ij
    // a row's posterior: the mean C . y, the sum C . K alone (NaN exactly when the variance is) and the latent variance os - C . K
    __device__ __forceinline__ float mean(int row) const { return red[0][0][row] + red[1][0][row]; }
    __device__ __forceinline__ float ck(int row) const { return red[0][1][row] + red[1][1][row]; }
    __device__ __forceinline__ float var(int row) const { return os - ck(row); }
    // the row's own mean or variance is NaN: what an epilogue that clamps with fmaxf has to ask, or the row gets a finite score
    __device__ __forceinline__ bool is_nan(int row) const { const float m = mean(row), c = ck(row); return m != m || c != c; }
};

// ---- the head and the tail that the epilogues share.  An epilogue is entered by all 256 threads.  Those that score with every wave
// (MES, GIBBON, KG, JES) give thread tid the row tid & 63 and the terms tid >> 6, + 4, ... of that row; the four partial values of
// a row meet in pm_mm's staging buffers as ps[part * PM_TM + row] (free by then; behind a barrier where a c0 panel was there), and
// thread i < 64 adds them in the order 0, 1, 2, 3:
static_assert(PM_NT == 4 * 64 && 4 * PM_TM <= 2 * PM_TM * LD_MN, "four partial sums per row, in pm_mm's staging buffers");
__device__ __forceinline__ float pm_sum4(const float* ps, int row) { return ((ps[row] + ps[PM_TM + row]) + ps[2 * PM_TM + row]) + ps[3 * PM_TM + row]; }

// task t's exclusion list as the predicate of pm_list_merge
__device__ __forceinline__ auto pm_excl(const PmPool& s, int t) { return [&s, t](long long r) { return pm_excluded(s, t, r); }; }

// The tail of a pool epilogue: thread i < tl.m, which holds the score of row i, writes it to out[plane, r0 + i] (out: nullable,
// [planes, rows]), then the first wave offers the tile's scores to the walk's list of `width` entries, but for the rows excl(r) holds for.
template <class ARGS, class WALK, class EX>
__device__ __forceinline__ void pm_tile_tail(const ARGS& args, const PmTile& tl, WALK& walk, float score, float* out, size_t plane, int width, EX excl) {
    const int tid = threadIdx.x;
    if (out && tid < tl.m) out[plane * (size_t)args.p.rows + (size_t)(tl.r0 + tid)] = score;
    if (width > 0 && (tid >> 6) == 0) pm_list_merge(walk.lv, walk.li, width, score, (long long)(tl.r0 + tid), tid < tl.m, excl);
}

// the epilogue of prediction: the first 64 threads write the outputs of their row (pm_row_out); POOL: the tail, with nothing more to store
struct PmRowEpilogue {
    using Args = PmNoEpilogueArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK& walk, f32x4 (&)[2][2]) {
        const int tid = threadIdx.x;
        [[maybe_unused]] float score = 0.f;
        if (tid < tl.m) {
            const float vl = tl.var(tid);
            score = pm_row_out<POOL>(args, tl.t, tl.r0 + tid, tl.mean(tid), vl, vl + tl.noise);
        }
        if constexpr (POOL) pm_tile_tail(args, tl, walk, score, nullptr, 0, args.s.k, pm_excl(args.s, tl.t));
    }
};

template <bool REFINE, bool GLOBAL, bool ARD = false, bool POOL = false, class EPI = PmRowEpilogue>
__global__ __launch_bounds__(PM_NT) void k_predict_marginal(PmArgsOf<ARD, POOL, EPI> args) {
    const PmArgs& a = args.p;
    extern __shared__ __attribute__((aligned(16))) float pm_lds[];
    __shared__ float ABs[2 * PM_TM * LD_MN];
    float *As = ABs, *Bs = ABs + PM_TM * LD_MN;
    __shared__ float rowsq[2][PM_TM];
    __shared__ float red[2][2][PM_TM];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wc = wv & 1;
    const int ld = a.buf_ld;
    float *Kb, *Cb = nullptr, *wv_s = nullptr;   // row tiles K, C; A^-1 y (REFINE)
    int grid = gridDim.x;
    if (GLOBAL) {
        const int s = blockIdx.x;
        Kb = s < a.slot_count[0] ? a.slots[0] + (size_t)s * a.slot_floats : a.slots[1] + (size_t)(s - a.slot_count[0]) * a.slot_floats;
    } else {
        Kb = pm_lds;
    }
    if (REFINE) { Cb = Kb + (size_t)PM_TM * ld; wv_s = Cb + (size_t)PM_TM * ld; }
    const int64_t d = a.d;
    // persistent walk over the tiles of all tasks, in order: (t, first tile of t) is a cursor that only moves forward
    int t = 0;
    int64_t tile0 = 0;
    [[maybe_unused]] std::conditional_t<POOL, PmPoolWalk<REFINE ? 2 : 1>, PmNoPool> walk;
    if constexpr (POOL)
        if (!walk.start(a, args.s)) return;
    for (int64_t g = blockIdx.x;; g += grid) {
        int64_t lo, hi, r0;
        if constexpr (POOL) {
            lo = 0; hi = a.rows;
            if (!walk.next(a, args.s, args.s.k, t, r0)) return;
        } else {
            for (;;) {
                if (t >= a.T) return;
                pm_range(a, t, lo, hi);
                const int64_t nt = (hi - lo + PM_TM - 1) / PM_TM;
                const bool mine = pm_kind_of(a, t) == (REFINE ? 1 : 0);
                if (g < tile0 + nt && mine) break;
                // next task: the first tile index >= its first tile that this workgroup owns
                tile0 += nt; ++t;
                if (g < tile0) g = tile0 + (((int64_t)blockIdx.x - tile0) % grid + grid) % grid;
            }
            r0 = lo + (g - tile0) * PM_TM;
        }
        const int m = (int)(hi - r0 < PM_TM ? hi - r0 : PM_TM);
        const int n = pm_ns(a, t);
        const float* sc = a.scal + (size_t)t * NSCAL;
        const float os = sc[S_OS], noise = sc[S_NOISE], il2 = 1.f / (sc[S_LS] * sc[S_LS]);
        const int kind = a.kind;
        const float* Zs = a.Zs + (size_t)t * a.ns_ld * d;
        const float* mu = a.mean_s + (size_t)t * d;
        const float* il = nullptr;
        if constexpr (ARD) il = args.r.il + (size_t)t * d;
        const float* Ai = a.Ainv + (size_t)t * a.ns_ld * a.ns_ld;
        const float* ys = a.y_s + (size_t)t * a.ns_ld;
        const int np = (n + PM_TM - 1) / PM_TM;   // support panels
        const int nk = np * PM_TM;                // K extent of the products over the support set (zero-padded)
        f32x4 acc[2][2];
        // ---- K row tile
        for (int p = 0; p < np; ++p) {
            const int j0 = p * PM_TM;
            pm_k_panel<ARD>(a, Zs, mu, il, r0, m, n, j0, os, il2, As, Bs, rowsq, acc, Kb + j0, ld, [] {});
        }
        float s1[2][4], s2[2][4];   // per-lane partial sums of the rows this lane holds: C y and C K
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) { s1[i][r] = 0.f; s2[i][r] = 0.f; }
        float dummy[2];
        auto opK = [&](const float* B) { return [=](int i, int k, float (&v)[4]) {
#pragma unroll
            for (int x = 0; x < 4; ++x) v[x] = B[(size_t)i * ld + k + x];
        }; };
        // ---- C = K A^-1 (A^-1 symmetric: row j of A^-1 is column j, contiguous in k)
        for (int p = 0; p < np; ++p) {
            const int j0 = p * PM_TM;
            pm_mm<false>(acc, nk, As, Bs, opK(Kb),
                [&](int j, int k, float (&v)[4]) {
                    if (j0 + j >= n) { v[0] = v[1] = v[2] = v[3] = 0.f; return; }
                    pm_ld4(Ai + (size_t)(j0 + j) * a.ns_ld, k, n, false, v);
                }, dummy, dummy);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ii = pm_row(i, r), jj = j0 + pm_col(j);
                        if (REFINE) Cb[(size_t)ii * ld + jj] = acc[i][j][r];
                        if (jj < n) { s1[i][r] = fmaf(acc[i][j][r], ys[jj], s1[i][r]); s2[i][r] = fmaf(acc[i][j][r], Kb[(size_t)ii * ld + jj], s2[i][r]); }
                    }
        }
        if (REFINE) {
            // A^-1 y (rows of A^-1, fixed order), then R = K - C A panel by panel, folded into the two sums
            for (int j = tid; j < nk; j += PM_NT) {
                float w = 0.f;
                if (j < n) for (int k = 0; k < n; ++k) w = fmaf(Ai[(size_t)j * a.ns_ld + k], ys[k], w);
                wv_s[j] = w;
            }
            __syncthreads();
            const float* Dss = a.D2ss + (size_t)t * a.ns_ld * a.ns_ld;
            float c1[2][4], c2[2][4];   // the correction terms, summed apart from the main terms and added last
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) { c1[i][r] = 0.f; c2[i][r] = 0.f; }
            for (int p = 0; p < np; ++p) {
                const int j0 = p * PM_TM;
                pm_mm<false>(acc, nk, As, Bs, opK(Cb),
                    [&](int j, int k, float (&v)[4]) {
                        const int jj = j0 + j;
#pragma unroll
                        for (int x = 0; x < 4; ++x)
                            v[x] = (jj < n && k + x < n) ? os * kappa0(kind, Dss[(size_t)jj * a.ns_ld + k + x] * il2) + (k + x == jj ? noise : 0.f) : 0.f;
                    }, dummy, dummy);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ii = pm_row(i, r), jj = j0 + pm_col(j);
                            if (jj < n) {
                                const float res = Kb[(size_t)ii * ld + jj] - acc[i][j][r];
                                c1[i][r] = fmaf(res, wv_s[jj], c1[i][r]); c2[i][r] = fmaf(res, Cb[(size_t)ii * ld + jj], c2[i][r]);
                            }
                        }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) { s1[i][r] += c1[i][r]; s2[i][r] += c2[i][r]; }
        }
        // ---- row reductions: the 16 lanes of a row group, then the two column waves, in a fixed order
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x = s1[i][r], y = s2[i][r];
                x += dpp_f<DPP_XOR1>(x); x += dpp_f<DPP_XOR2>(x); x += dpp_f<DPP_HALF_MIRROR>(x); x += dpp_f<DPP_MIRROR>(x);
                y += dpp_f<DPP_XOR1>(y); y += dpp_f<DPP_XOR2>(y); y += dpp_f<DPP_HALF_MIRROR>(y); y += dpp_f<DPP_MIRROR>(y);
                if ((lane & 15) == 0) { red[wc][0][pm_row(i, r)] = x; red[wc][1][pm_row(i, r)] = y; }
            }
        __syncthreads();
        EPI::template run<ARD, POOL>(args, PmTile{t, r0, m, n, nk, ld, os, noise, il2, mu, il, Kb, As, Bs, &rowsq, red}, walk, acc);
        __syncthreads();   // red / rowsq / the row tiles are rewritten by the next tile
    }
}

// ---- the float64 evaluation of the rows of flagged tasks: one wave per row, difference-form distances from the features,
// k_refine64's float64 A^-1 (region A1) and the kernel row parked in LDS
constexpr int PM64_NT = 256;
constexpr int PM64_WAVES = PM64_NT / 64;

// a flagged task as the float64 kernels see it
struct Pm64Task {
    int n, ld;                              // support points (at most R64_MAXN) and their leading dimension
    double os, noise, ls;
    double il2;                             // 1 / ls^2, the walks of prediction and of the believer.  NOT Thompson's: k_ts_stream64 has always formed
                                            // (1 / ls)^2, which differs in the last bit, and passes that to pm64_kernel_row itself - il2 is a parameter
                                            // there so that a caller states which of the two its bits were built with
    const double* A1;                       // float64 A^-1 [ld, ld] (k_refine64)
    const float *Zs, *ys, *mu, *el;         // ARD: Zs is Zt_s; el, l per dimension, is null otherwise
};
// false: the float64 kernels do not own task t (uniform)
template <bool ARD, class ARGS>
__device__ __forceinline__ bool pm64_task(const ARGS& args, int t, Pm64Task& k) {
    const PmArgs& a = args.p;
    if (pm_kind_of(a, t) != 2) return false;
    k.n = pm_ns(a, t); k.ld = a.ns_ld;
    if (k.n <= 0 || k.n > R64_MAXN) return false;
    const float* sc = a.scal + (size_t)t * NSCAL;
    k.os = sc[S_OS]; k.noise = sc[S_NOISE]; k.ls = sc[S_LS]; k.il2 = 1.0 / (k.ls * k.ls);
    k.A1 = a.w64 + (size_t)t * a.w64_stride;
    k.Zs = a.Zs + (size_t)t * k.ld * a.d;
    k.ys = a.y_s + (size_t)t * k.ld;
    k.mu = a.mean_s + (size_t)t * a.d;
    k.el = nullptr;
    if constexpr (ARD) k.el = args.r.ell + (size_t)t * a.d;
    return true;
}

// one wave: k[j] = os kappa(|zq - zs_j|^2 il2) in float64 for the support rows of the task, published to the wave.  ARD: the query
// element is scaled as k_ard_scale scales it (ard_scaled, in float32) before it is promoted.
template <bool ARD>
__device__ __forceinline__ void pm64_kernel_row(const PmArgs& a, const Pm64Task& tk, const float* zq, double il2, double* k) {
    const int lane = threadIdx.x & 63;
    for (int j = lane; j < tk.n; j += 64) {
        const float* zs = tk.Zs + (size_t)j * a.d;
        double s = 0.0;
        if constexpr (ARD) {
            for (int c = 0; c < a.d; ++c) { const double e = (double)ard_scaled(zq[c], tk.mu[c], tk.el[c]) - (double)zs[c]; s += e * e; }
        } else {
            for (int c = 0; c < a.d; ++c) { const double e = (double)zq[c] - (double)zs[c]; s += e * e; }
        }
        k[j] = tk.os * kappa0(a.kind, s * il2);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// one wave: the float64 posterior of the pool row zq - the kernel row into k, c = k A^-1, then s1 = c . y and s2 = c . k in every lane
// (mean s1, latent variance os - s2).  Every sum has a fixed order.
template <bool ARD>
__device__ __forceinline__ void pm64_posterior_row(const PmArgs& a, const Pm64Task& tk, const float* zq, double* k, double& s1, double& s2) {
    const int lane = threadIdx.x & 63;
    pm64_kernel_row<ARD>(a, tk, zq, tk.il2, k);
    s1 = 0.0; s2 = 0.0;
    for (int j = lane; j < tk.n; j += 64) {
        double c = 0.0;
        for (int q = 0; q < tk.n; ++q) c += k[q] * tk.A1[(size_t)q * tk.ld + j];
        s1 += c * (double)tk.ys[j];
        s2 += c * k[j];
    }
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
}

// the end of a float64 walk: the first wave takes the entry (v, i) that each lane of the other waves holds, wave by wave, through
// merge(v, i) - which updates (lv, li) - and stores its list, `width` entries, as that of (t, blockIdx.x)
template <class M>
__device__ __forceinline__ void pm64_finish_walk(const PmPool& s, int t, int width, float& lv, long long& li, M merge) {
    __shared__ float mv[PM64_WAVES - 1][64];
    __shared__ long long mi[PM64_WAVES - 1][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (wv > 0) { mv[wv - 1][lane] = lv; mi[wv - 1][lane] = li; }
    __syncthreads();
    if (wv == 0) {
        for (int w = 0; w < PM64_WAVES - 1; ++w) merge(mv[w][lane], mi[w][lane]);
        pm_list_store(s, t, blockIdx.x, lane, width, lv, li);
    }
}

// ---- the float64 walk.  Every float64 kernel of a pool call but Thompson's (k_predict_marginal64, k_bv_walk64, k_mes_walk64,
// k_gb_walk64, k_kg_walk64, k_jes_walk64, k_gumbel_walk64) has this shape: kr[PM64_WAVES][R64_MAXN] doubles of LDS, pm64_task
// with a uniform return for a task it does not own, then one of the two functions below with what it does to a row.
//
// The rows of one wave: lo + blockIdx.x * 4 + wave, stride gridDim.x * 4, below hi.  Per row the float64 posterior
// (pm64_posterior_row, the kernel row into k - this wave's row of kr), then row(r, zq, k, s1, s2), entered by the whole wave.
template <bool ARD, class F>
__device__ __forceinline__ void pm64_rows(const PmArgs& a, const Pm64Task& tk, int64_t lo, int64_t hi, double* k, F row) {
    const int wv = threadIdx.x >> 6;
    for (int64_t r = lo + (int64_t)blockIdx.x * PM64_WAVES + wv; r < hi; r += (int64_t)gridDim.x * PM64_WAVES) {
        const float* zq = a.Zq + (size_t)r * a.d;
        double s1, s2;
        pm64_posterior_row<ARD>(a, tk, zq, k, s1, s2);
        row(r, zq, k, s1, s2);
        // the next row overwrites k, which lanes of this wave may still be reading (the products of row(): bv64_c0's k . w); a wave
        // is not lockstep for the compiler, so the barrier keeps the instructions apart and the fence orders the LDS traffic
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

// The walk of workgroup (c, t) of a grid (chunks, T) over the whole pool, keeping a list: every wave offers the score that row()
// returns in lane 0 (row() also does the acquisition's own stores) to its list of `width` entries, but for the rows excl(r) holds for;
// at the end the four lists become that of (t, c) (pm64_finish_walk).  width <= 0 (uniform): no list, the rows are only evaluated.
template <bool ARD, class ARGS, class EX, class F>
__device__ __forceinline__ void pm64_pool_walk(const ARGS& args, const Pm64Task& tk, double* k, int width, EX excl, F row) {
    const int t = blockIdx.y, lane = threadIdx.x & 63;
    float lv = -INFINITY;
    long long li = -1;
    pm64_rows<ARD>(args.p, tk, 0, args.p.rows, k, [&](int64_t r, const float* zq, const double* kq, double s1, double s2) {
        const float score = row(r, zq, kq, s1, s2);
        if (width > 0) pm_list_merge(lv, li, width, score, (long long)r, lane == 0, excl);
    });
    if (width <= 0) return;   // (uniform)
    pm64_finish_walk(args.s, t, width, lv, li, [&](float v, long long i) { pm_list_merge(lv, li, width, v, i, i >= 0, [](long long) { return false; }); });
}

// prediction's own: the rows of the task's range, or (POOL) the pool walk with the score of pm_row_out
template <bool ARD = false, bool POOL = false>
__global__ __launch_bounds__(PM64_NT) void k_predict_marginal64(PmArgsOf<ARD, POOL> args) {
    const PmArgs& a = args.p;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    auto out = [&](int64_t r, const float*, const double*, double s1, double s2) {
        return lane == 0 ? pm_row_out<POOL>(args, t, r, (float)s1, (float)(tk.os - s2), (float)(tk.os - s2 + tk.noise)) : 0.f;
    };
    if constexpr (POOL) {
        pm64_pool_walk<ARD>(args, tk, kr[wv], args.s.k, pm_excl(args.s, t), out);
    } else {
        int64_t lo, hi;
        pm_range(a, t, lo, hi);
        pm64_rows<ARD>(a, tk, lo, hi, kr[wv], out);
    }
}

// ---- the last phase of the selection: one wave per task merges the task's lists and writes top_idx / top_val [T, k]
// (skipped tasks, and every task when no walk ran: -1 / -inf)
__global__ __launch_bounds__(64) void k_pool_topk(PmArgsOf<false, true> args) {
    const PmArgs& a = args.p;
    const PmPool& s = args.s;
    const int t = blockIdx.x, lane = threadIdx.x, k = s.k;
    float lv;
    long long li;
    pm_merge_task_lists(a, s, t, k, lv, li);
    if (lane < k) { s.top_idx[(size_t)t * k + lane] = li; s.top_val[(size_t)t * k + lane] = li >= 0 ? lv : -INFINITY; }
}

}  // namespace adkf
