// GIBBON batch max-value entropy search over a shared pool (adkf_gibbon_pool; Moss, Leslie, Gonzalez and Rayson 2021; BoTorch's
// qLowerBoundMaxValueEntropy): q sequential-greedy picks per task of the lower bound on the information a BATCH of noisy observations
// carries about the task's optimum VALUE, given S samples ystar[t, s] of that value (as adkf_mes_pool takes them).  With m(x) and
// v_0(x) the latent posterior of prediction, noise the task's, sigma = sqrt(max(v_0, 1e-12)) (pm_ei's clamp) and gamma_s = mes_gamma:
//     tau(g)   = phi(g) / Phi(g),    h(g) = tau(g) (g + tau(g))                          0 < h < 1
//     rho2(x)  = max(v_0, 1e-12) / (max(v_0, 1e-12) + noise)
//     a(x)     = -(1 / 2S) sum_s log1p(-rho2 h(gamma_s))                                 the single-point score, >= 0
//     alpha(B) = 1/2 log |R_B| + sum_(i in B) a(x_i)                                     R_B: the predictive correlation of the noisy y_B
// and the greedy increment of adding x to the picks p_0 .. p_(j-1) is exactly
//     score_j(x) = a(x) + 1/2 log((max(v_j(x), 1e-12) + noise) / (max(v_0(x), 1e-12) + noise)),
// v_j(x) = v_0(x) - sum_(i<j) ell_i(x)^2 the believer's downdated latent variance (the top of believer_stream.h).  The mean never
// moves, ystar never changes, there is no incumbent; score_0 = a, later scores may be negative and are valid scores.
//
// The state, its layout (bv_scratch), k_bv_init and k_bv_step<ARD> are the believer's, as they are: BvArgs::best is carried and
// ignored.  Per step j: the walks of each task kind, then k_bv_step.
//   the walk  is k_predict_marginal's tile with GibbonEpilogue: with c picks made the believer's c0 panel (bv_c0_panel) and thread
//             i < 64's substitution (bv_downdate) give v_j, which that thread keeps in ONE register; behind a barrier - the panel is
//             dead - the four-wave sum of the S terms of a(x) where the panel was (pm_sum4, predict_stream.h), then the shared tail
//             (pm_tile_tail).  No LDS beyond prediction's.  At c = 0 nothing of the downdate runs.
//   float64   tasks take k_gb_walk64, the float64 pool walk (pm64_pool_walk): k_bv_walk64's lane-per-pick downdate in float64
//             (bv64_downdate), the mean and the two variances rounded to float32, then k_mes_walk64's lane-per-sample sum with its
//             fixed butterfly.
// trace[j] <= trace[0] bit for bit: a(x) comes out of the same instructions at every step, v_j <= v_0 in float32 (the downdate only
// subtracts a sum of squares; the float64 walk rounds monotonically), a quotient of x <= y is at most 1, its logarithm at most 0,
// and adding a number <= 0 cannot round upwards.
//
// Deterministic: no atomics, every sum has a fixed order, nothing of size T x rows is kept unless trace is given.  A NaN or infinite
// ystar[t, s] makes every score of task t NaN (never selected).
#pragma once
#include "mes_stream.h"

namespace adkf {

// log1p(-rho2 h(gamma)), h = tau (gamma + tau), tau = phi / Phi.  The split is pm_mes_term's:
//   gamma > 0        Phi = 1 - erfc(gamma / sqrt 2) / 2, tau = pdf / (1 - q): the small tail keeps its digits;
//   -1 < gamma <= 0  as written, Phi in [0.15, 0.5], gamma + tau >= 0.52;
//   gamma <= -1      gamma + tau cancels (both ~a).  With a = -gamma, ex = erfcx(a / sqrt 2): tau = sqrt(2 / pi) / ex and
//                    gamma + tau = tau b(a), b(a) = 1 - a sqrt(pi / 2) ex pm_log_ei's bracket, so h = tau^2 b(a); b from erfcxf
//                    down to gamma = -12, its series a^-2 (1 - 3 a^-2 + 15 a^-4 - 105 a^-6 + 945 a^-8) beyond.  h -> 1.
// h is held at 1 from above (a rounding of tau^2 b), so 1 - rho2 h >= 1 - rho2 = noise / (v + noise) > 0.  +-inf and NaN give NaN.
// Not inlined, for pm_log_ei's reason.
__device__ __noinline__ float pm_gibbon_term(float gamma, float rho2) {
    float h;
    if (gamma > -1.f) {
        const float pdf = 0.3989422804014327f * expf(-0.5f * gamma * gamma);
        const float tau = gamma > 0.f ? pdf / (1.f - 0.5f * erfcf(gamma * 0.70710678118654752f)) : pdf / (0.5f * erfcf(-gamma * 0.70710678118654752f));
        h = tau * (gamma + tau);
    } else {
        const float a = -gamma;
        const float ex = erfcxf(a * 0.70710678118654752f);
        float b;
        if (gamma > -12.f) {
            b = fmaf(-(a * 1.2533141373155003f), ex, 1.f);
        } else {
            const float ia = 1.f / a, w = ia * ia;
            b = w * fmaf(fmaf(fmaf(fmaf(945.f, w, -105.f), w, 15.f), w, -3.f), w, 1.f);
        }
        const float tau = 0.7978845608028654f / ex;   // sqrt(2 / pi) / ex
        h = tau * tau * b;
    }
    h = h > 1.f ? 1.f : h;   // (keeps NaN)
    return log1pf(-rho2 * h);
}

struct GibbonArgs {
    BvArgs b;                           // the believer's state and outputs (best: carried, ignored)
    const float* ystar; int S;          // [T, S]: the max-value samples
};
struct GibbonEpilogue;
template <bool ARD>
using GibbonKargs = PmArgsOf<ARD, true, GibbonEpilogue>;   // p.Zq: the pool; s.k = 1, s.cand_* [T, chunks_max]; ARD: r, the query scaling

// score_j from the sum of the S terms, the step-0 variance and the downdated one (equal at c = 0, where the logarithm is skipped)
__device__ __forceinline__ float gb_score(float sum, int S, float v0, float vj, float noise, int c) {
    const float a = sum * (-0.5f / (float)S);
    if (c == 0) return a;
    return a + 0.5f * logf((fmaxf(vj, 1e-12f) + noise) / (fmaxf(v0, 1e-12f) + noise));
}

struct GibbonEpilogue {
    using Args = GibbonArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK& walk, f32x4 (&acc)[2][2]) {
        static_assert(POOL, "adkf_gibbon_pool: a shared pool");
        const PmArgs& a = args.p;
        const BvArgs& v = args.v.b;
        const int tid = threadIdx.x, row = tid & 63, part = tid >> 6, t = tl.t, q = v.q, S = args.v.S;
        const int c = v.cnt[t];   // (uniform) picks made, at most the step
        float* ps = tl.As;        // the c0 panel, then [4][64]: the partial sums
        float vj = 0.f;
        if (c > 0) {
            bv_c0_panel<ARD>(a, v, tl, acc, c);
            if (tid < tl.m) vj = tl.var(tid) - bv_downdate(v, t, c, ps + tid * BV_LDC);
            __syncthreads();   // the panel is dead: the partial sums may overwrite it
        }
        if (row < tl.m) {
            const float v0 = fmaxf(tl.var(row), 1e-12f);
            const float mean = tl.mean(row);
            const float sigma = sqrtf(v0), rho2 = v0 / (v0 + tl.noise);
            const float* ys = args.v.ystar + (size_t)t * S;
            float sum = 0.f;
            for (int s = part; s < S; s += PM_NT / 64) sum += pm_gibbon_term(mes_gamma(a.maximize, ys[s], mean, sigma), rho2);
            ps[part * PM_TM + row] = sum;
        }
        __syncthreads();
        float score = 0.f;
        if (tid < tl.m) score = gb_score(pm_sum4(ps, tid), S, tl.var(tid), vj, tl.noise, c);
        pm_tile_tail(args, tl, walk, score, v.trace, (size_t)t * q + v.j, 1, bv_excl(args.s, v, t, c));
    }
};

// ---- flagged tasks: the float64 pool walk with k_bv_walk64's downdate, then lane s the term of sample s
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_gb_walk64(GibbonKargs<ARD> args) {
    const PmArgs& a = args.p;
    const BvArgs& v = args.v.b;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = v.q, S = args.v.S;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const int c = v.cnt[t];
    const double* Wt = v.W64 + (size_t)t * q * tk.ld;
    const double* G = v.G64 + (size_t)t * q * q;
    const float* Xp = v.Xp + (size_t)t * q * a.d;
    const float noise = (float)tk.noise;
    const float ys = lane < S ? args.v.ystar[(size_t)t * S + lane] : 0.f;
    pm64_pool_walk<ARD>(args, tk, kr[wv], 1, bv_excl(args.s, v, t, c), [&](int64_t r, const float* zq, const double* k, double s1, double s2) {
        const double vl = tk.os - s2;
        const float mean = (float)s1, v0 = (float)vl;
        const float vj = c > 0 ? (float)(vl - bv64_downdate<ARD>(a, tk, zq, k, Wt, G, Xp, c, q, lane)) : v0;
        const float v0c = fmaxf(v0, 1e-12f);
        float g = lane < S ? pm_gibbon_term(mes_gamma(a.maximize, ys, mean, sqrtf(v0c)), v0c / (v0c + noise)) : 0.f;
        for (int o = 32; o > 0; o >>= 1) g += __shfl_xor(g, o);
        const float score = gb_score(g, S, v0, vj, noise, c);
        if (lane == 0 && v.trace) v.trace[((size_t)t * q + v.j) * (size_t)a.rows + (size_t)r] = score;
        return score;
    });
}

}  // namespace adkf
