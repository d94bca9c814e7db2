// Hyperparameter-marginalised prediction and acquisition over a shared pool (adkf_mix_pool; the integrated acquisition of Snoek,
// Larochelle and Adams 2012, BoTorch's average over the MCMC batch of a fully Bayesian model; Riis et al. 2022 and BoTorch's
// qBayesianActiveLearningByDisagreement for the disagreement score).  The T tasks of the batch are MODELS of the same pool rows -
// the same data under different phi, usually.  A group names up to MIX_MEMBERS_MAX member tasks with weights; with wt_i = w_i / W the
// normalised weights of its used entries and m_i, v_i, e_i prediction's mean, variance and EI (or log EI) of member i at a pool row:
//     mean   = sum_i wt_i m_i
//     var    = sum_i wt_i v_i + sum_i wt_i (m_i - mean)^2                     (the law of total variance, from the deviations)
//     score  = sum_i wt_i e_i                                                 (integrated EI)
//            | log sum_i wt_i exp(le_i) = mx + log sum_i wt_i exp(le_i - mx)  (its logarithm, mx = max_i le_i: EI is never formed)
//            | +-mean
//            | (log var_c - sum_i wt_i log vc_i) / 2, vc_i = max(v_i, 1e-12)  (BALD of the Gaussian mixture, var_c from the vc_i)
//
//   stage A   the host walks the pool in chunks of MIX_CHUNK_ROWS rows and runs prediction itself (pm_launch<ARD, true>, the caller's
//             flags and best_f, k = 0) on each: m, v and e [T, chunk] in the scratch are prediction's by construction, for every kind
//             of task.  Tasks that no group names are predicted too.
//   k_mix_groups   one wave per group, lane j the entry j: validity, the compaction of the used entries by ballot and popcount, the
//             weight sum in entry order, wt_i and the "cannot be evaluated" flag go to the scratch.
//   k_mix_score    a persistent grid over (group, 64-row tile of the chunk), a group's tiles spread over the grid as k_ehvi_score
//             spreads them.  256 threads: thread row + 64 part walks the slots part, part + 4, ..; its reads t_i L + row of a plane
//             are coalesced over the 64 rows.  A first pass gives the mean, a second the variances, the score's partials and the
//             maximum of the log form, a third (log form only) the sum of that form.  Four partials are always added in the order
//             0, 1, 2, 3.  The first wave offers the 64 scores to the list of (group, walker), which lives in the scratch across the
//             chunk launches.
//   k_mix_topk     one wave per group merges the group's lists (pm_group_topk, as k_ehvi_topk).
//
// Every sum starts from -0.f, the identity that keeps the sign of a zero term, so a lone term's bits pass through, and is taken over
// 2 wt_i x_i and halved at the end (mix_sum4).  With that a group of one used member has wt = 1 and a group of two used entries that
// name one task with equal weights has wt = 1/2 twice (exact), and either has prediction's bits in mean, var and the EI score -
// subnormal values included - and 0 exactly as BALD score.  The log form weighs exp(le_i - mx) with wt_i instead of adding log wt_i
// to le_i, because that makes the same true of it: the sum is exactly 1, its logarithm 0, and mx is the member's log EI.  (Adding
// log(1/2) to le and log 2 back at the end rounds twice.)  It loses a term only where wt_i exp(le_i - mx) underflows against a sum
// that is at least the weight of the member that holds mx.
//
// Deterministic: no atomics, every sum has a fixed order; a group's bits depend on its own members and their order, its weights,
// best_f, its exclusion list and the pool row only - not on the grid, the other groups or the chunk boundaries.  A group that cannot
// be evaluated (see include/adkf_gp.h) is NaN everywhere and selects nothing.
#pragma once
#include "predict_stream.h"

namespace adkf {

constexpr int MIX_MEMBERS_MAX = 64;
constexpr int MIX_CHUNK_ROWS = 16384;
constexpr int MIX_NT = 256;
enum { MIX_EI = 0, MIX_LOG_EI = 1, MIX_MEAN = 2, MIX_BALD = 3 };

// a group as k_mix_score reads it (written by k_mix_groups); every member is 4 bytes wide
struct MixGroup {
    int bad, n, pad[2];             // n: the used entries, compacted in entry order into the slots 0 .. n - 1
    int t[MIX_MEMBERS_MAX];         // the member task of a slot (0 beyond n)
    float wt[MIX_MEMBERS_MAX];      // its normalised weight (0 beyond n)
};
static_assert(sizeof(MixGroup) % 4 == 0 && sizeof(MixGroup) / 4 <= MIX_NT, "MixGroup: copied to LDS by one pass of the workgroup");

struct MixArgs {
    int G, M, kind, maximize;       // kind: MIX_EI ..
    const int32_t* mem; const float* w;   // [G, M] each; w nullable (every weight 1)
    MixGroup* grp;                  // [G]
    const float *m, *v, *e;         // stage A: [T, L] each; v and e only where something reads them
    int64_t c0, L, rows;            // the chunk's first row and length; the pool's rows
    float *mean, *var, *score;      // each nullable, [G, rows]
    PmPool s;                       // the exclusion lists (per GROUP), the lists [G, chunks_max, k], top_* [G, k]
    int cpg;                        // lists in use per group: min(grid / G, chunks_max), at least 1
};

// ---- one wave per group: the used entries and their weights
__global__ __launch_bounds__(64) void k_mix_groups(PmArgs a, MixArgs e) {
    const int g = blockIdx.x, lane = threadIdx.x, M = e.M, T = a.T;
    const bool have = lane < M;
    const int t = have ? e.mem[(size_t)g * M + lane] : -1;
    const float w = (have && e.w) ? e.w[(size_t)g * M + lane] : 1.f;
    // an entry with mem == -1 is not there: its weight is not read.  Of the others an index outside [0, T) and a negative, NaN or
    // infinite weight spoil the group; a zero weight leaves the entry unused
    const bool named = t != -1;
    bool bad = named && (t < 0 || t >= T || !(w >= 0.f) || w == INFINITY);
    const bool used = named && !bad && w > 0.f;
    if (used && pm_kind_of(a, t) < 0) bad = true;   // a used member with n_s == 0 or info != 0
    const unsigned long long um = __ballot(used);
    const int n = __popcll(um), slot = __popcll(um & ((1ull << lane) - 1ull));
    // W: the used weights added in entry order
    float W = -0.f;
    for (int j = 0; j < 64; ++j) {
        const float wj = __shfl(w, j);
        if ((um >> j) & 1ull) W += wj;
    }
    const bool any_bad = __ballot(bad) != 0ull || n == 0 || !(W < INFINITY);
    MixGroup& s = e.grp[g];
    if (lane >= n) { s.t[lane] = 0; s.wt[lane] = 0.f; }      // (the lanes n .. 63 and the slots 0 .. n - 1 below are disjoint)
    if (used) { s.t[slot] = t; s.wt[slot] = w / W; }
    if (lane == 0) { s.bad = any_bad ? 1 : 0; s.n = n; s.pad[0] = s.pad[1] = 0; }
}

// Four partials of a row, added in the order 0, 1, 2, 3.  The partials are sums of 2 wt_i x_i and the join halves them: scaling by a
// power of two changes no bit of a normal result, and it keeps the anchors exact on subnormal values too (a float32 EI far from best_f
// is one), whose half is not a float: 2 (1/2) x + 2 (1/2) x = 2 x, halved, is x.
__device__ __forceinline__ float mix_sum4(const float (&p)[4][64], int row) { return (((p[0][row] + p[1][row]) + p[2][row]) + p[3][row]) * 0.5f; }

// ---- the outputs and scores of one chunk of the pool
__global__ __launch_bounds__(MIX_NT) void k_mix_score(MixArgs e) {
    // the partials of a row: 0 the mean, then the log form's sum; 1 sum wt v; 2 sum wt dev^2; 3 sum wt vc; 4 sum wt log vc;
    // 5 sum wt e, or the log form's maximum
    __shared__ float red[6][4][64];
    __shared__ MixGroup gs;
    const int tid = threadIdx.x, row = tid & 63, part = tid >> 6;
    const int G = e.G, grid = gridDim.x, k = e.s.k, kind = e.kind;
    const int chunk = blockIdx.x / G;
    if (chunk >= e.cpg) return;   // (uniform)
    const int64_t ntiles = (e.L + 63) / 64;
    const float nan = __builtin_nanf("");
    const bool want_score = e.score || k > 0;
    const bool bald = kind == MIX_BALD && want_score, lin = kind == MIX_EI && want_score, lg = kind == MIX_LOG_EI && want_score;
    const bool want_var = e.var || bald;
    for (int g = blockIdx.x % G; g < G; g += grid) {
        if (tid < (int)(sizeof(MixGroup) / 4)) reinterpret_cast<int*>(&gs)[tid] = reinterpret_cast<const int*>(e.grp + g)[tid];
        __syncthreads();
        // the list of (group, walker) so far: empty at the first chunk (the host fills the indices with -1)
        float lv = -INFINITY;
        long long li = -1;
        if (k > 0 && tid < k) {
            const size_t q = ((size_t)g * e.s.chunks_max + chunk) * k + tid;
            li = e.s.cand_idx[q];
            lv = li >= 0 ? e.s.cand_val[q] : -INFINITY;
        }
        const int bad = gs.bad, n = gs.n;
        for (int64_t tile = chunk; tile < ntiles; tile += e.cpg) {
            const int64_t r0 = tile * 64;
            const int m = (int)(e.L - r0 < 64 ? e.L - r0 : 64);
            const size_t out = (size_t)g * (size_t)e.rows + (size_t)(e.c0 + r0 + row);
            if (bad) {   // (uniform)
                if (tid < m) {
                    if (e.mean) e.mean[out] = nan;
                    if (e.var) e.var[out] = nan;
                    if (e.score) e.score[out] = nan;
                }
                continue;
            }
            const bool in = row < m;
            const size_t q0 = (size_t)(r0 + row);
            if (in) {
                float sm = -0.f;
                for (int i = part; i < n; i += 4) sm = fmaf(2.f * gs.wt[i], e.m[(size_t)gs.t[i] * (size_t)e.L + q0], sm);
                red[0][part][row] = sm;
            }
            __syncthreads();
            const float mean = in ? mix_sum4(red[0], row) : 0.f;
            float mx = -INFINITY;
            if (in) {
                float sv = -0.f, sb = -0.f, sc = -0.f, sl = -0.f, se = -0.f;
                for (int i = part; i < n; i += 4) {
                    const size_t q = (size_t)gs.t[i] * (size_t)e.L + q0;
                    const float wt = 2.f * gs.wt[i];   // (mix_sum4 halves)
                    if (want_var) {
                        const float vi = e.v[q], dev = e.m[q] - mean;
                        sv = fmaf(wt, vi, sv);
                        sb = fmaf(wt * dev, dev, sb);
                        if (bald) {
                            const float vc = vi < 1e-12f ? 1e-12f : vi;   // (a NaN stays one)
                            sc = fmaf(wt, vc, sc);
                            sl = fmaf(wt, logf(vc), sl);
                        }
                    }
                    if (lin) se = fmaf(wt, e.e[q], se);
                    if (lg) mx = fmaxf(mx, e.e[q]);
                }
                red[1][part][row] = sv; red[2][part][row] = sb; red[3][part][row] = sc; red[4][part][row] = sl;
                red[5][part][row] = lg ? mx : se;
            }
            __syncthreads();
            if (lg) {   // (uniform) the maximum of the row, then the weighted sum against it; -inf terms are skipped
                if (in) {
                    mx = fmaxf(fmaxf(fmaxf(red[5][0][row], red[5][1][row]), red[5][2][row]), red[5][3][row]);
                    float sum = -0.f;
                    for (int i = part; i < n; i += 4) {
                        const float le = e.e[(size_t)gs.t[i] * (size_t)e.L + q0];
                        if (le != -INFINITY) sum = fmaf(2.f * gs.wt[i], expf(le - mx), sum);   // (a NaN member: NaN - mx is NaN, whatever mx)
                    }
                    red[0][part][row] = sum;   // (the mean was read before the barrier above)
                }
                __syncthreads();
            }
            float score = 0.f;
            if (tid < m) {
                const float between = mix_sum4(red[2], tid);
                if (e.mean) e.mean[out] = mean;
                if (e.var) e.var[out] = mix_sum4(red[1], tid) + between;
                if (lin) score = mix_sum4(red[5], tid);
                else if (lg) { const float sum = mix_sum4(red[0], tid); score = sum == 0.f ? -INFINITY : mx + logf(sum); }
                else if (bald) score = 0.5f * (logf(mix_sum4(red[3], tid) + between) - mix_sum4(red[4], tid));
                else if (kind == MIX_MEAN) score = e.maximize ? mean : -mean;
                if (e.score) e.score[out] = score;
            }
            if (k > 0 && part == 0)
                pm_list_merge(lv, li, k, score, (long long)(e.c0 + r0 + tid), tid < m, [&](long long r) { return pm_excluded(e.s, g, r); });
            __syncthreads();   // the partials are rewritten by the next tile
        }
        if (k > 0) pm_list_store(e.s, g, chunk, tid, k, lv, li);
        __syncthreads();   // gs is rewritten by the next group
    }
}

// ---- one wave per group: the group's lists merged under the total order, top_idx / top_val [G, k] (nothing listed: -1 / -inf)
__global__ __launch_bounds__(64) void k_mix_topk(MixArgs e) {
    pm_group_topk(e.s, blockIdx.x, e.rows > 0 ? e.cpg : 0);
}

}  // namespace adkf
