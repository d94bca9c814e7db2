// Level-set estimation and batch UCB over a shared pool (adkf_levelset_pool; the straddle of Bryan et al. 2005, the classification
// of Gotovos et al. 2013, GP-BUCB of Desautels, Krause and Burdick 2014): q sequential-greedy picks per task against a threshold
// tau[t] with a band of width beta[t], and at every step the class of every pool row and the expected number of actives.  With m(x)
// and v_0(x) the latent posterior of prediction, v_j(x) = v_0(x) - sum_(i<j) ell_i(x)^2 the believer's downdated latent variance
// (the top of believer_stream.h), sigma_j = sqrt(max(v_j, 1e-12)), s = +1 with ADKF_PM_MAXIMIZE and -1 without:
//     z_j(x)        = s (m - tau) / sigma_j
//     straddle_j(x) = beta sigma_j - |m - tau|                   > 0 exactly when the band m +- beta sigma_j holds tau
//     score_j       = straddle_j                                 ADKF_LS_STRADDLE
//                   = log Phi(z_j)                               ADKF_LS_PROB  (unclamped: ls_log_cdf)
//                   = s m + beta sigma_j                         ADKF_LS_BOUND (UCB with MAXIMIZE, -(LCB) without)
//     class         = undecided (2) if straddle_j > 0, otherwise active (0) if s (m - tau) > 0, otherwise inactive (1)
//     hits_j        = sum over the pool rows of Phi(z_j)
// The picks are hallucinated: a GP's variance does not depend on the labels, so the mean never moves and the downdate is the
// believer's.  Counts and hits at steps j > 0 are hallucinated in the same sense.  PROB does NOT diversify: for a row beyond tau the
// probability rises as its variance falls, so its batch is "the rows most certainly active if the earlier picks land on their means".
//
// The state, its layout (bv_scratch) and the step (bv_step with BvBelieveMean) are the believer's: BvArgs::best is carried and
// ignored.  On top of it four unsigned 64-bit accumulators per task, acc [T, 4]: the three class counts and the 2^-31 fixed-point
// sum of the float32 Phi terms (gb_fixed of gumbel_stream.h).  Per step j: the walks of each task kind, then k_ls_step.
//   the walk   is k_predict_marginal's tile with LsEpilogue: with c picks made the believer's c0 panel (bv_c0_panel) and thread
//              i < 64's substitution (bv_downdate) give v_j; at c = 0 none of that runs.  Thread i < tl.m forms the row (ls_row); the
//              first wave counts the three classes by ballot and adds the fixed-point Phi terms by shuffles, then issues at most four
//              integer atomicAdds per tile into acc[t], none for an accumulator the tile adds 0 to.  cls is written at step 0.  Then
//              the shared tail (pm_tile_tail) with the believer's exclusion.  No LDS beyond prediction's.
//   float64    tasks take k_ls_walk64, the float64 pool walk (pm64_pool_walk) with bv64_downdate; the mean and the variance are
//              rounded to float32 and go through the same ls_row.  Each wave keeps its own integer sums over its rows and issues
//              one atomicAdd per accumulator at the end.
//   k_ls_step  first copies acc[t] into counts[t, j] and hits[t, j] (u64 to double to float) and clears acc[t] - also when no row
//              is eligible - then runs the believer's step unchanged.
//
// Whatever the score kind, the class comes from the SAME float32 straddle_j a STRADDLE call stores in trace, formed as
// fmaf(beta, sigma_j, -|m - tau|) in both walks.  Integer addition is associative and commutative, so counts and hits of a task are
// the same bits on any grid, alone or in a batch, and under any permutation of the pool (as gumbel_stream.h).  A Phi term is at most
// 1, so the sum cannot wrap below 2^32 rows; the host refuses rows > 2^31.  No floating-point atomics.
//
// A row whose mean or variance is NaN belongs to no class (cls = -1), adds nothing to hits and has score NaN.  A tau[t] that is not
// finite, or a beta[t] that is NaN, infinite or negative, does that to every row of task t: nothing is picked, the counts are 0.
#pragma once
#include "believer_stream.h"
#include "gumbel_stream.h"

namespace adkf {

constexpr int LS_STRADDLE = 0, LS_PROB = 1, LS_BOUND = 2;   // ADKF_LS_*

// log Phi(z) without a clamp: pm_neg_log_cdf's three pieces, negated.  Finite down to where a^2 / 2 overflows; +inf gives 0, -inf
// gives -inf, NaN gives NaN.  A function of its own, so that pm_neg_log_cdf keeps its bits.  Not inlined, for pm_log_ei's reason.
__device__ __noinline__ float ls_log_cdf(float z) {
    if (z > 0.f) return log1pf(-0.5f * erfcf(z * 0.70710678118654752f));
    if (z > -1.f) return logf(0.5f * erfcf(-z * 0.70710678118654752f));
    const float a = -z;
    return logf(0.5f * erfcxf(a * 0.70710678118654752f)) - 0.5f * a * a;
}

struct LsArgs {
    BvArgs b;                           // the believer's state and outputs (best: carried, ignored)
    const float *tau, *beta;            // [T]
    int kind;                           // LS_*
    int8_t* cls;                        // nullable [T, rows]: the class at step 0
    unsigned long long* acc;            // [T, 4]: active, inactive, undecided, the fixed-point sum of Phi; null when nobody reads them
    int64_t* counts; float* hits;       // k_ls_step: nullable [T, q, 3] and [T, q]
};
struct LsEpilogue;
template <bool ARD>
using LsKargs = PmArgsOf<ARD, true, LsEpilogue>;   // p.Zq: the pool; s.k = 1, s.cand_* [T, chunks_max]; ARD: r, the query scaling

// the threshold and the width of a task, and whether the task can be evaluated by value
struct LsTask { float tau, beta; bool ok; };
__device__ __forceinline__ LsTask ls_task(const LsArgs& v, int t) {
    const float tau = v.tau[t], beta = v.beta[t];
    return {tau, beta, isfinite(tau) && isfinite(beta) && beta >= 0.f};
}

// one row at step j from its float32 mean and downdated latent variance: the score of the kind, the class (-1: none) and Phi(z_j)
struct LsRow { float score; int cls; float phi; };
__device__ __forceinline__ LsRow ls_row(int kind, int maximize, const LsTask& k, float mean, float vj) {
    if (!k.ok || mean != mean || vj != vj) return {NAN, -1, 0.f};
    const float sigma = sqrtf(fmaxf(vj, 1e-12f));
    const float dm = mean - k.tau;
    const float straddle = fmaf(k.beta, sigma, -fabsf(dm));
    const float sd = maximize ? dm : -dm;
    const float z = sd / sigma;
    LsRow r;
    r.cls = straddle > 0.f ? 2 : (sd > 0.f ? 0 : 1);
    r.phi = 0.5f * erfcf(-z * 0.70710678118654752f);
    r.score = kind == LS_STRADDLE ? straddle : (kind == LS_PROB ? ls_log_cdf(z) : fmaf(k.beta, sigma, maximize ? mean : -mean));
    return r;
}

struct LsEpilogue {
    using Args = LsArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK& walk, f32x4 (&acc)[2][2]) {
        static_assert(POOL, "adkf_levelset_pool: a shared pool");
        static_assert(PM_TM == 64, "the first wave holds the tile's rows");
        const PmArgs& a = args.p;
        const LsArgs& L = args.v;
        const BvArgs& v = L.b;
        const int tid = threadIdx.x, t = tl.t, q = v.q;
        const int c = v.cnt[t];   // (uniform) picks made, at most the step
        float* C0 = tl.As;
        if (c > 0) bv_c0_panel<ARD>(a, v, tl, acc, c);
        LsRow r{0.f, -1, 0.f};
        if (tid < tl.m) {
            float vl = tl.var(tid);
            if (c > 0) vl -= bv_downdate(v, t, c, C0 + tid * BV_LDC);
            r = ls_row(L.kind, a.maximize, ls_task(L, t), tl.mean(tid), vl);
            if (L.cls && v.j == 0) L.cls[(size_t)t * (size_t)a.rows + (size_t)(tl.r0 + tid)] = (int8_t)r.cls;
        }
        if (L.acc && (tid >> 6) == 0) {   // the first wave: rows >= tl.m hold class -1 and contribute nothing
            const unsigned long long n0 = __popcll(__ballot(r.cls == 0)), n1 = __popcll(__ballot(r.cls == 1)), n2 = __popcll(__ballot(r.cls == 2));
            unsigned long long x = r.cls >= 0 ? gb_fixed(r.phi) : 0;   // (gb_fixed maps NaN to the clamp: the row's own validity guards it)
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
            if (tid == 0) {
                unsigned long long* ac = L.acc + 4 * (size_t)t;
                if (n0) atomicAdd(ac + 0, n0);
                if (n1) atomicAdd(ac + 1, n1);
                if (n2) atomicAdd(ac + 2, n2);
                if (x) atomicAdd(ac + 3, x);
            }
        }
        pm_tile_tail(args, tl, walk, r.score, v.trace, (size_t)t * q + v.j, 1, bv_excl(args.s, v, t, c));
    }
};

// ---- flagged tasks: the float64 pool walk with k_bv_walk64's downdate; the row from the float32-rounded mean and variance
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_ls_walk64(LsKargs<ARD> args) {
    const PmArgs& a = args.p;
    const LsArgs& L = args.v;
    const BvArgs& v = L.b;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = v.q;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const int c = v.cnt[t];
    const double* Wt = v.W64 + (size_t)t * q * tk.ld;
    const double* G = v.G64 + (size_t)t * q * q;
    const float* Xp = v.Xp + (size_t)t * q * a.d;
    const LsTask k = ls_task(L, t);
    unsigned long long n0 = 0, n1 = 0, n2 = 0, x = 0;   // this wave's sums (the same in every lane)
    pm64_pool_walk<ARD>(args, tk, kr[wv], 1, bv_excl(args.s, v, t, c), [&](int64_t r, const float* zq, const double* kq, double s1, double s2) {
        double vl = tk.os - s2;
        if (c > 0) vl -= bv64_downdate<ARD>(a, tk, zq, kq, Wt, G, Xp, c, q, lane);
        const LsRow w = ls_row(L.kind, a.maximize, k, (float)s1, (float)vl);
        n0 += w.cls == 0; n1 += w.cls == 1; n2 += w.cls == 2;
        if (w.cls >= 0) x += gb_fixed(w.phi);
        if (lane == 0) {
            if (v.trace) v.trace[((size_t)t * q + v.j) * (size_t)a.rows + (size_t)r] = w.score;
            if (L.cls && v.j == 0) L.cls[(size_t)t * (size_t)a.rows + (size_t)r] = (int8_t)w.cls;
        }
        return w.score;
    });
    if (L.acc && lane == 0) {
        unsigned long long* ac = L.acc + 4 * (size_t)t;
        if (n0) atomicAdd(ac + 0, n0);
        if (n1) atomicAdd(ac + 1, n1);
        if (n2) atomicAdd(ac + 2, n2);
        if (x) atomicAdd(ac + 3, x);
    }
}

// the per-task state before step 0: k_bv_init's, an incumbent of 0 (never read), and the cleared accumulators
__global__ __launch_bounds__(256) void k_ls_init(LsArgs v, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    v.b.cnt[t] = 0; v.b.best[t] = 0.f;
    if (v.acc)
        for (int i = 0; i < 4; ++i) v.acc[4 * (size_t)t + i] = 0;
}

// ---- the end of step j: one workgroup per task.  The sums of the step's walks become counts[t, j] and hits[t, j] and the
// accumulators are cleared for the next step - whether or not a row is eligible - then the believer's step.
template <bool ARD>
__global__ __launch_bounds__(256) void k_ls_step(LsKargs<ARD> args) {
    const LsArgs& L = args.v;
    const int t = blockIdx.x;
    if (L.acc && threadIdx.x == 0) {
        unsigned long long* ac = L.acc + 4 * (size_t)t;
        const size_t o = (size_t)t * L.b.q + L.b.j;
        if (L.counts)
            for (int i = 0; i < 3; ++i) L.counts[3 * o + i] = (int64_t)ac[i];
        if (L.hits) L.hits[o] = (float)((double)ac[3] * GB_FIX_UNIT);
        for (int i = 0; i < 4; ++i) ac[i] = 0;
    }
    bv_step<ARD>(args, L.b, BvBelieveMean{});
}

}  // namespace adkf
