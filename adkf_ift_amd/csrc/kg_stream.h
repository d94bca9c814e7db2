// Knowledge-gradient selection over a shared pool (adkf_kg_pool; Frazier, Powell and Dayanik 2009; Scott, Frazier and Powell 2011,
// "KGCP"; the single-step form of BoTorch's qKnowledgeGradient on a discrete set): a pool row x is scored by how much one noisy
// observation at x is expected to raise the best posterior mean over x itself and a reference set R_t = ref_idx[t, 0 .. M), M <= 64.
// With m(.), cov(., .) the latent posterior of prediction, noise the task's, vc = max(v(x), 1e-12) (pm_ei's clamp), s = sqrt(vc + noise)
// and sgn = +1 with ADKF_PM_MAXIMIZE, -1 without:
//     reference line j   a_j = sgn m(r_j),   b_j = cov(x, r_j) / s
//     own line           a_x = sgn m(x),     b_x = vc / s
//     KG(x) = E_Z[max_l (a_l + b_l Z)] - max_l a_l = sum over the lines of the upper envelope, by ascending slope, of
//             (b_next - b_cur) h(-|c|),   c = (a_cur - a_next) / (b_next - b_cur),   h(u) = phi(u) + u Phi(u)
// (Frazier's form: a sum of non-negative terms; E[max] - max a is never formed).  With ADKF_PM_LOG_EI the score is log KG, the
// log-sum-exp of log(b_next - b_cur) + log h(-|c|), log h from pm_log_ei(u, 1, 0, 1); one surviving line gives KG = 0, log KG = -inf.
// Reference entries outside [0, rows) are skipped, a repeated index counts once (its first occurrence), and the entry equal to the
// row's own index is skipped for that row, by index: x always contributes its own line from the tile's mean and variance.
//
// The envelope without a sort: line j keeps lo_j = max over b_i < b_j and hi_j = min over b_i > b_j of (a_j - a_i) / (b_i - b_j); among
// equal slopes the largest intercept survives, exact ties keep the lowest index (the own line has the highest); j is active iff
// lo_j < hi_j; its successor is the active line of the next larger slope, and the crossing of the sum is recomputed from that pair - so
// a line whose interval is empty up to rounding changes the sum by rounding only, kept or dropped (kg_clip, kg_term).  O(M^2) a row.
//
//   k_kg_refs grid (M, T), before the walks: entry j of task t - validity and the first occurrence, then the reference entry of
//             believer_stream.h (bv_ref_entry: the row into Xp, w = A^-1 k(Z_s, x_r) and a_j = w . y).  Skipped entries get zero rows,
//             mean 0 and the index -1.
//   the walk  is k_predict_marginal's tile with KgEpilogue: the believer's c0 panel (bv_c0_panel) with the reference state in the
//             place of the picks is cov(x, r_j) for the tile's 64 rows; it is stored if asked, the absent lines of a row become NaN
//             and vc goes into the panel's pad column 64.  The slopes are never divided out: the envelope is found on the numerators
//             c_l = s b_l (s > 0 scales every crossing alike), and a difference of slopes is (c_next - c_cur) / s, the difference of
//             two float32 inputs, which rounds once.  All 256 threads share the envelope, thread tid the row tid & 63
//             and the lines tid >> 6, + 4, ...: the active flags (a bit mask in a register), behind a barrier NaN over the inactive
//             lines, behind another the successor and the term of each active line; the four partial sums of a row meet where the
//             panel was (pm_sum4, predict_stream.h; log: four (max, sum) pairs, combined here), then the shared tail (pm_tile_tail).
//             No LDS beyond prediction's.
//   float64   tasks take k_kg_walk64, the float64 pool walk (pm64_pool_walk): lane i forms c0(x, i) in float64 (bv64_c0), the mean,
//             variance and covariances are rounded to float32 as the tile holds them, the envelope runs across the lanes with the
//             own line as uniform data, and the terms are added in a fixed butterfly.  A task takes one kind of walk.
//   selection k_pool_topk, unchanged: the candidate lists are prediction's.
//
// NaN is the mark of an absent line in the panel, so a covariance that IS NaN (a reference row with NaN or infinite features: its w
// and mean are NaN too) leaves the envelope of that row as a skipped entry does, and kg_clip's fmaxf / fminf pass over a NaN
// intercept: the other rows are scored without that line, not as NaN (the CPU twin would propagate it; include/adkf_gp.h says so).
// A row whose OWN mean or variance is NaN scores NaN - an explicit test at the end of both walks, since the same fmaxf would
// otherwise hand it a finite score - and NaN is never selected.
//
// Deterministic: no atomics, every sum has a fixed order; a row's score depends on its task's data, the reference set and its own
// features only.
#pragma once
#include "gibbon_stream.h"

namespace adkf {

struct KgArgs {
    int M;                              // reference entries per task
    const int64_t* ref_idx;             // [T, M]: the caller's reference rows
    float* W; double* W64;              // [T, M, ns_ld]: w of entry j (float64 tasks: W64; null without a float64 region)
    float* Xp;                          // [T, M, d]: the entries' feature rows
    float* am;                          // [T, M]: the posterior mean of entry j, natural sign (0: skipped)
    int64_t* ridx;                      // [T, M]: the pool row of entry j, -1: skipped
    float *score, *cov, *ref_mean;      // nullable [T, rows], [T, rows, M], [T, M]
};
struct KgEpilogue;
template <bool ARD>
using KgKargs = PmArgsOf<ARD, true, KgEpilogue>;   // p.Zq: the pool; s: prediction's selection state; ARD: r, the query scaling

// h(u) = phi(u) + u Phi(u) for u <= 0, held at 0 from below (a rounding of the two terms, which cancel in the tail)
__device__ __forceinline__ float kg_h(float u) {
    const float cdf = 0.5f * erfcf(-u * 0.70710678118654752f);
    const float pdf = 0.3989422804014327f * expf(-0.5f * u * u);
    return fmaxf(fmaf(u, cdf, pdf), 0.f);
}
// what the present line i does to line j: the end of j's interval it moves, or j's death among equal slopes.  b: the slopes or, as
// here, their numerators c = s b (the ends are then z / s for every line alike)
__device__ __forceinline__ void kg_clip(float aj, float bj, int j, float ai, float bi, int i, float& lo, float& hi, bool& dead) {
    if (bi < bj) lo = fmaxf(lo, (aj - ai) / (bi - bj));
    else if (bi > bj) hi = fminf(hi, (aj - ai) / (bi - bj));
    else if (i != j && (ai > aj || (ai == aj && i < j))) dead = true;
}
// the term of the active line (aj, cj / s) and its successor (an, cn / s), cn > cj: KG's, or its logarithm
__device__ __forceinline__ float kg_term(float aj, float cj, float an, float cn, float s, int log) {
    const float db = (cn - cj) / s, u = -fabsf((aj - an) / db);
    return log ? logf(db) + pm_log_ei(u, 1.f, 0.f, 1) : db * kg_h(u);
}
// one more logarithmic term t into the running (max, sum of exp(. - max)); -inf adds nothing
__device__ __forceinline__ void kg_lse_add(float t, float& mx, float& sm) {
    if (t == -INFINITY) return;
    if (t > mx) { sm = fmaf(sm, expf(mx - t), 1.f); mx = t; }
    else sm += expf(t - mx);
}

// ---- the reference state: one workgroup per (entry, task)
template <bool ARD>
__global__ __launch_bounds__(256) void k_kg_refs(KgKargs<ARD> args) {
    const PmArgs& a = args.p;
    const KgArgs& v = args.v;
    __shared__ __attribute__((aligned(16))) float fb[3 * TS_NS_MAX];
    __shared__ double red[256];
    const int j = blockIdx.x, t = blockIdx.y, M = v.M, ld = a.ns_ld;
    const size_t o = (size_t)t * M + j;
    const long long idx = v.ref_idx[o];
    bool ok = pm_kind_of(a, t) >= 0 && idx >= 0 && idx < a.rows;
    for (int i = 0; ok && i < j; ++i) ok = v.ref_idx[(size_t)t * M + i] != idx;   // (uniform) the first occurrence counts
    const float mean = (float)bv_ref_entry<ARD>(args, t, ok, idx, v.Xp + o * a.d, v.W + o * ld, v.W64 ? v.W64 + o * ld : nullptr, fb, red);
    if (threadIdx.x == 0) { v.ridx[o] = ok ? idx : -1; v.am[o] = mean; if (v.ref_mean) v.ref_mean[o] = mean; }
}

struct KgEpilogue {
    using Args = KgArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK& walk, f32x4 (&acc)[2][2]) {
        static_assert(POOL, "adkf_kg_pool: a shared pool");
        const PmArgs& a = args.p;
        const KgArgs& v = args.v;
        const int tid = threadIdx.x, row = tid & 63, part = tid >> 6, t = tl.t, M = v.M, log = a.log_ei;
        constexpr int OWN = PM_TM;   // the own line: index 64, its slope in the panel's pad column
        float* C0 = tl.As;           // the c0 panel, then the slopes; at the end [4][64] partial sums (log: [2][4][64])
        const float* am = v.am + (size_t)t * M;
        const int64_t* ridx = v.ridx + (size_t)t * M;
        {
            BvArgs bv{};
            bv.q = M; bv.W = v.W; bv.Xp = v.Xp;
            bv_c0_panel<ARD>(a, bv, tl, acc, M);
        }
        if (v.cov) {
            float* cv = v.cov + ((size_t)t * (size_t)a.rows + (size_t)tl.r0) * M;
            for (int e = tid; e < tl.m * M; e += PM_NT) {
                const int i = e / M, j = e - i * M;
                cv[e] = ridx[j] >= 0 ? C0[i * BV_LDC + j] : 0.f;
            }
            __syncthreads();
        }
        const float sgn = a.maximize ? 1.f : -1.f;
        float* Cr = C0 + row * BV_LDC;
        float ax = 0.f, s = 1.f;
        if (row < tl.m) {   // the numerators of the row's slopes, in place: NaN for an absent line, vc for the own one
            const float vc = fmaxf(tl.var(row), 1e-12f);
            const long long r = tl.r0 + row;
            s = sqrtf(vc + tl.noise);
            ax = sgn * tl.mean(row);
            for (int j = part; j < M; j += PM_NT / 64) {
                const long long rj = ridx[j];
                if (rj < 0 || rj == r) Cr[j] = NAN;
            }
            if (part == 0) Cr[OWN] = vc;
        }
        __syncthreads();
        unsigned act = 0;   // bit q: this thread's q-th line, part + 4 q, is on the envelope
        if (row < tl.m) {
            const float bx = Cr[OWN];
            for (int q = 0, j = part; j <= OWN; ++q, j += PM_NT / 64) {
                if (j >= M && j != OWN) continue;
                const float bj = Cr[j];
                if (bj != bj) continue;
                const float aj = j == OWN ? ax : sgn * am[j];
                float lo = -INFINITY, hi = INFINITY;
                bool dead = false;
                for (int i = 0; i < M; ++i) {
                    const float bi = Cr[i];
                    if (bi == bi) kg_clip(aj, bj, j, sgn * am[i], bi, i, lo, hi, dead);
                }
                kg_clip(aj, bj, j, ax, bx, OWN, lo, hi, dead);
                if (!dead && lo < hi) act |= 1u << q;
            }
        }
        __syncthreads();   // every slope has been read: the inactive lines leave
        if (row < tl.m)
            for (int q = 0, j = part; j <= OWN; ++q, j += PM_NT / 64)
                if ((j < M || j == OWN) && !((act >> q) & 1u)) Cr[j] = NAN;
        __syncthreads();
        float sum = 0.f, mx = -INFINITY;   // plain: the sum of this thread's terms; log: (mx, sum) of kg_lse_add
        if (row < tl.m) {
            const float bx = Cr[OWN];
            for (int q = 0, j = part; j <= OWN; ++q, j += PM_NT / 64) {
                if (!((act >> q) & 1u)) continue;
                const float bj = Cr[j], aj = j == OWN ? ax : sgn * am[j];
                float bn = INFINITY, an = 0.f;   // the active line of the next larger slope
                for (int i = 0; i < M; ++i) {
                    const float bi = Cr[i];
                    if (bi > bj && bi < bn) { bn = bi; an = sgn * am[i]; }
                }
                if (bx > bj && bx < bn) { bn = bx; an = ax; }
                if (bn == INFINITY) continue;   // the steepest line ends the envelope
                const float term = kg_term(aj, bj, an, bn, s, log);
                if (log) kg_lse_add(term, mx, sum); else sum += term;
            }
        }
        __syncthreads();   // the panel is dead: the partial sums may overwrite it
        float* ps = tl.As;
        if (row < tl.m) {
            ps[part * PM_TM + row] = sum;
            if (log) ps[(4 + part) * PM_TM + row] = mx;
        }
        __syncthreads();
        float score = 0.f;
        if (tid < tl.m) {
            if (log) {
                float m4 = fmaxf(fmaxf(ps[4 * PM_TM + tid], ps[5 * PM_TM + tid]), fmaxf(ps[6 * PM_TM + tid], ps[7 * PM_TM + tid]));
                float tot = 0.f;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float mp = ps[(4 + p) * PM_TM + tid];
                    if (mp != -INFINITY) tot += ps[p * PM_TM + tid] * expf(mp - m4);
                }
                score = m4 == -INFINITY ? -INFINITY : m4 + logf(tot);
            } else {
                score = pm_sum4(ps, tid);
            }
            if (tl.is_nan(tid)) score = NAN;   // a NaN mean or variance: NaN, never selected (fmaxf would hide it)
        }
        pm_tile_tail(args, tl, walk, score, v.score, t, args.s.k, pm_excl(args.s, t));
    }
};
static_assert(PM_NT == 4 * 64 && 8 * PM_TM <= 2 * PM_TM * LD_MN && PM_TM * BV_LDC <= 2 * PM_TM * LD_MN,
              "KgEpilogue: the panel with its pad column, then eight partial values per row, in pm_mm's staging buffers");

// ---- flagged tasks: the float64 pool walk (pm64_pool_walk), lane i the reference line i
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_kg_walk64(KgKargs<ARD> args) {
    const PmArgs& a = args.p;
    const KgArgs& v = args.v;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, M = v.M, log = a.log_ei;
    constexpr int OWN = 64;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const double* Wt = v.W64 + (size_t)t * M * tk.ld;
    const float* Xp = v.Xp + (size_t)t * M * a.d;
    const float noise = (float)tk.noise, sgn = a.maximize ? 1.f : -1.f;
    const long long rj = lane < M ? (long long)v.ridx[(size_t)t * M + lane] : -1;
    const float aj = lane < M ? sgn * v.am[(size_t)t * M + lane] : 0.f;
    pm64_pool_walk<ARD>(args, tk, kr[wv], args.s.k, pm_excl(args.s, t), [&](int64_t r, const float* zq, const double* k, double s1, double s2) {
        const float vc = fmaxf((float)(tk.os - s2), 1e-12f), s = sqrtf(vc + noise);
        const float c0 = (float)bv64_c0<ARD>(a, tk, zq, k, Wt, Xp, M, lane);
        if (v.cov && lane < M) v.cov[((size_t)t * (size_t)a.rows + (size_t)r) * M + lane] = rj >= 0 ? c0 : 0.f;
        const float bj = (rj >= 0 && rj != r) ? c0 : NAN;   // the numerator of the lane's slope; NaN: no line in this lane
        const float ax = sgn * (float)s1, bx = vc;
        // the intervals: this lane's line and, in every lane alike, the own line
        float lo = -INFINITY, hi = INFINITY, lox = -INFINITY, hix = INFINITY;
        bool dead = false, deadx = false;
        for (int i = 0; i < M; ++i) {
            const float ai = __shfl(aj, i), bi = __shfl(bj, i);
            if (bi == bi) { kg_clip(aj, bj, lane, ai, bi, i, lo, hi, dead); kg_clip(ax, bx, OWN, ai, bi, i, lox, hix, deadx); }
        }
        kg_clip(aj, bj, lane, ax, bx, OWN, lo, hi, dead);
        const bool act = bj == bj && !dead && lo < hi, actx = !deadx && lox < hix;
        const float ba = act ? bj : NAN;
        // the successors
        float bn = INFINITY, an = 0.f, bnx = INFINITY, anx = 0.f;
        for (int i = 0; i < M; ++i) {
            const float ai = __shfl(aj, i), bi = __shfl(ba, i);
            if (bi > bj && bi < bn) { bn = bi; an = ai; }
            if (bi > bx && bi < bnx) { bnx = bi; anx = ai; }
        }
        if (actx && bx > bj && bx < bn) { bn = bx; an = ax; }
        const bool has = act && bn != INFINITY, hasx = actx && bnx != INFINITY;
        float score;
        if (log) {
            const float tj = has ? kg_term(aj, bj, an, bn, s, 1) : -INFINITY, tx = hasx ? kg_term(ax, bx, anx, bnx, s, 1) : -INFINITY;
            float mx = fmaxf(tj, tx);
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            float e = tj == -INFINITY ? 0.f : expf(tj - mx);
            for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
            if (tx != -INFINITY) e += expf(tx - mx);
            score = mx == -INFINITY ? -INFINITY : mx + logf(e);
        } else {
            float e = has ? kg_term(aj, bj, an, bn, s, 0) : 0.f;
            for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
            score = hasx ? e + kg_term(ax, bx, anx, bnx, s, 0) : e;
        }
        if (s1 != s1 || s2 != s2) score = NAN;   // as the tile: a NaN mean or variance scores NaN
        if (lane == 0 && v.score) v.score[(size_t)t * (size_t)a.rows + (size_t)r] = score;
        return score;
    });
}

}  // namespace adkf
