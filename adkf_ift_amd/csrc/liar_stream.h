// Constant-liar and label-replay batches over a shared pool (adkf_liar_pool): the believer of believer_stream.h with the believed
// value SUPPLIED - a fixed lie per task (the constant liar of Ginsbourger, Le Riche and Carraro 2010: CL-min, CL-max, CL-mean) or the
// pick's true label out of a table (BoTorch's condition_on_observations at fixed hyperparameters: r sequential iterations of a replay
// in one call).  Pick p_j is conditioned on y_j as a NOISY observation under the task's noise, so the mean moves.  With A, w_i, c0, G
// and ell exactly as at the top of believer_stream.h:
//     y_j      = the first finite of labels[t * label_stride + p_j], lie[t], m_j(x_(p_j))      (the last is the believer's rule)
//     z_j      = (y_j - m_j(x_(p_j))) / G[j, j]                  G[j, j] = sqrt(v_j(x_(p_j)) + noise); 0 under the believer's rule
//     m_j(x)   = m_0(x) + sum_(i<j) ell_i(x) z_i                 v_j(x) = v_0(x) - sum_(i<j) ell_i(x)^2
//     score_j  = EI or log EI (m_j(x), v_j(x), best_j)           best_(j+1) = min(best_j, y_j)   (max with MAXIMIZE)
// The state is the believer's (bv_scratch, BvArgs) plus z [T, q] and its float64 twin; k_bv_init starts it.
//
//   the walk  is the believer's tile with LiarEpilogue: bv_c0_panel and bv_downdate leave ell of the thread's row in place in the
//             panel, so the shift is one dot product of that row with the task's z (uniform loads), added to the row's mean before the
//             score.  No LDS beyond prediction's.  At c = 0 none of this runs and the score is prediction's, bit for bit; with every
//             z_i = 0 (no lie, no label: the believer's rule) the shift is +0 and the scores are adkf_believer_pool's, bit for bit.
//   float64   tasks take k_liar_walk64 on pm64_pool_walk: bv64_downdate's substitution over the lanes, each broadcast ell_i also
//             multiplied into the shift, in float64 against z64.
//   k_liar_step is the believer's step (bv_step) with LiarBelieve for its rule: the value lookup, the pick's shifted mean from the
//             ell the step has just formed for the new row of G, z_j (float32; float64 too for flagged tasks), sel_lie and inc.
//
// Deterministic: no atomics, every sum has a fixed order, nothing of size T x rows is kept unless trace is given.
#pragma once
#include "believer_stream.h"

namespace adkf {

struct LiarArgs {
    BvArgs b;                             // the believer's state and outputs
    const float* lie;                     // nullable [T]
    const float* labels; int64_t stride;  // nullable [rows] (stride 0) or [T, rows] (stride rows)
    float* z; double* z64;                // [T, q]: one scalar per pick (z64: flagged tasks; null without a float64 region)
    float *sel_lie, *inc;                 // nullable [T, q] and [T, q + 1]
};
struct LiarEpilogue;
template <bool ARD>
using LiarKargs = PmArgsOf<ARD, true, LiarEpilogue>;   // p.Zq: the pool; s.k = 1, s.cand_* [T, chunks_max]; ARD: r, the query scaling

struct LiarEpilogue {
    using Args = LiarArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK& walk, f32x4 (&acc)[2][2]) {
        static_assert(POOL, "adkf_liar_pool: a shared pool");
        const PmArgs& a = args.p;
        const BvArgs& v = args.v.b;
        const int tid = threadIdx.x, t = tl.t, q = v.q;
        const int c = v.cnt[t];   // (uniform) picks made, at most the step
        float* C0 = tl.As;
        if (c > 0) bv_c0_panel<ARD>(a, v, tl, acc, c);
        float score = 0.f;
        if (tid < tl.m) {
            float vl = tl.var(tid), mean = tl.mean(tid);
            if (c > 0) {
                float* e = C0 + tid * BV_LDC;
                const float* z = args.v.z + (size_t)t * q;
                vl -= bv_downdate(v, t, c, e);
                float sh = 0.f;
                for (int i = 0; i < c; ++i) sh = fmaf(e[i], z[i], sh);
                mean += sh;
            }
            score = bv_score(a, v, t, mean, vl);
        }
        pm_tile_tail(args, tl, walk, score, v.trace, (size_t)t * q + v.j, 1, bv_excl(args.s, v, t, c));
    }
};

// ---- flagged tasks: the float64 pool walk with the downdate and the shift in float64
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_liar_walk64(LiarKargs<ARD> args) {
    const PmArgs& a = args.p;
    const BvArgs& v = args.v.b;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = v.q;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const int c = v.cnt[t];
    const double* Wt = v.W64 + (size_t)t * q * tk.ld;
    const double* G = v.G64 + (size_t)t * q * q;
    const double* z = args.v.z64 + (size_t)t * q;
    const float* Xp = v.Xp + (size_t)t * q * a.d;
    pm64_pool_walk<ARD>(args, tk, kr[wv], 1, bv_excl(args.s, v, t, c), [&](int64_t r, const float* zq, const double* k, double s1, double s2) {
        double vl = tk.os - s2, mean = s1;
        if (c > 0) {
            double sh = 0.0;
            vl -= bv64_downdate<ARD>(a, tk, zq, k, Wt, G, Xp, c, q, lane, [&](int i, double e) { sh += e * z[i]; });
            mean += sh;
        }
        float score = 0.f;
        if (lane == 0) {
            score = bv_score(a, v, t, (float)mean, (float)vl);
            if (v.trace) v.trace[((size_t)t * q + v.j) * (size_t)a.rows + (size_t)r] = score;
        }
        return score;
    });
}

// the incumbents before step 0 (k_bv_init has the rest of the state)
__global__ __launch_bounds__(256) void k_liar_init(LiarArgs v, const float* best_f, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < T && v.inc) v.inc[(size_t)t * (v.b.q + 1)] = best_f[t];
}

// What bv_step believes about pick c of task t (one thread): the value supplied, and the scalar that moves the mean
struct LiarBelieve {
    const LiarArgs& v;
    int t, maximize;
    bool f64;
    __device__ __forceinline__ size_t inc_slot() const { return (size_t)t * (v.b.q + 1) + v.b.j + 1; }
    __device__ __forceinline__ void none(size_t o) const {
        if (v.sel_lie) v.sel_lie[o] = 0.f;
        if (v.inc) v.inc[inc_slot()] = v.b.best[t];
    }
    __device__ __forceinline__ BvPick pick(size_t o, long long p, double m0, const double* ell, int c, double gd) const {
        const size_t zo = (size_t)t * v.b.q;
        double sh = 0.0;
        for (int i = 0; i < c; ++i) sh += ell[i] * (f64 ? v.z64[zo + i] : (double)v.z[zo + i]);
        const double mj = m0 + sh;
        float y = v.labels ? v.labels[(size_t)t * (size_t)v.stride + (size_t)p] : NAN;
        if (!isfinite(y) && v.lie) y = v.lie[t];
        const bool own = !isfinite(y);
        if (own) y = (float)mj;
        const double zj = own ? 0.0 : ((double)y - mj) / gd;
        v.z[zo + c] = (float)zj;
        if (f64) v.z64[zo + c] = zj;
        if (v.sel_lie) v.sel_lie[o] = y;
        if (v.inc) v.inc[inc_slot()] = maximize ? fmaxf(v.b.best[t], y) : fminf(v.b.best[t], y);
        return {(float)mj, y};
    }
};

// ---- the end of step j: one workgroup per task
template <bool ARD>
__global__ __launch_bounds__(256) void k_liar_step(LiarKargs<ARD> args) {
    const int t = blockIdx.x;
    bv_step<ARD>(args, args.v.b, LiarBelieve{args.v, t, args.p.maximize, pm_kind_of(args.p, t) == 2});
}

}  // namespace adkf
