// Max-value entropy search over a shared pool (adkf_mes_pool; Wang and Jegelka 2017): every pool row is scored by the information
// it carries about the task's optimum VALUE, given S samples ystar[t, s] of that value (an input: the maxima of pathwise posterior
// draws over the pool, adkf_thompson_pool's sel_val, are such samples).  With m(x) and v(x) the latent posterior of prediction and
// sigma = sqrt(max(v, 1e-12)) (pm_ei's clamp):
//     gamma_s  = (ystar[t, s] - m) / sigma   with ADKF_PM_MAXIMIZE (samples of max f),   (m - ystar[t, s]) / sigma   without (of min f)
//     g(gamma) = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma)
//     score(x) = (1 / S) sum_s g(gamma_s)
// g > 0 and strictly decreasing; no incumbent enters.  pm_mes_term forms g without its two hazards (see there).
//
//   the walk  is k_predict_marginal's tile itself with MesEpilogue in the place of prediction's epilogue: the four-wave sum over the
//             samples (pm_sum4, predict_stream.h), scaled by 1 / S, and the shared tail (pm_tile_tail).  m and v are prediction's,
//             bit for bit.  No LDS beyond prediction's.
//   float64   tasks (refine64.h) take k_mes_walk64, the float64 pool walk (pm64_pool_walk): the row's float64 mean and variance
//             rounded to float32 as k_predict_marginal64 hands them to pm_row_out, lane s < S evaluates sample s, and the wave adds
//             the lanes in a fixed butterfly.  A task takes one kind of walk, so the two orders of summation never meet in one task.
//   selection k_pool_topk, unchanged: the candidate lists are prediction's.
//
// Deterministic: no atomics, every sum has a fixed order.  A NaN or infinite ystar[t, s] makes every score of task t NaN (never selected).
#pragma once
#include "believer_stream.h"

namespace adkf {

// g(gamma) = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma).  The hazards are pm_log_ei's, and so is the split:
//   gamma > 0        Phi -> 1: log Phi = log1p(-erfc(gamma / sqrt 2) / 2), which keeps the digits of the small tail;
//   -1 < gamma <= 0  as written, Phi in [0.15, 0.5];
//   gamma <= -1      both terms grow like gamma^2 / 2 and cancel.  With a = -gamma, Phi = exp(-a^2 / 2) erfcx(a / sqrt 2) / 2, so
//                        g = -(a sqrt(2 / pi) b(a) / erfcx(a / sqrt 2)) / 2 - log(erfcx(a / sqrt 2) / 2),
//                    b(a) = 1 - a sqrt(pi / 2) erfcx(a / sqrt 2) pm_log_ei's bracket: a^2 / 2 never appears.  b from erfcxf down to
//                    gamma = -12 (it cancels to ~a^-2: an absolute error of a few eps32 a^2 in a term that tends to -1 / 2), its series
//                    a^-2 (1 - 3 a^-2 + 15 a^-4 - 105 a^-6 + 945 a^-8) beyond.
// +-inf and NaN give NaN.  Not inlined, for pm_log_ei's reason: the temporaries of erfcxf and the logarithms stay out of the walk's
// register budget.
__device__ __noinline__ float pm_mes_term(float gamma) {
    if (gamma > -1.f) {
        const float pdf = 0.3989422804014327f * expf(-0.5f * gamma * gamma);
        if (gamma > 0.f) {
            const float q = 0.5f * erfcf(gamma * 0.70710678118654752f);   // 1 - Phi
            return 0.5f * gamma * pdf / (1.f - q) - log1pf(-q);
        }
        const float cdf = 0.5f * erfcf(-gamma * 0.70710678118654752f);
        return 0.5f * gamma * pdf / cdf - logf(cdf);
    }
    const float a = -gamma;
    const float ex = erfcxf(a * 0.70710678118654752f);
    float ab;   // a b(a)
    if (gamma > -12.f) {
        ab = a * fmaf(-(a * 1.2533141373155003f), ex, 1.f);
    } else {
        const float ia = 1.f / a, w = ia * ia;
        ab = ia * fmaf(fmaf(fmaf(fmaf(945.f, w, -105.f), w, 15.f), w, -3.f), w, 1.f);
    }
    return -(0.3989422804014327f * ab / ex) - logf(0.5f * ex);   // sqrt(2 / pi) / 2 = 1 / sqrt(2 pi)
}

struct MesArgs {
    const float* ystar; int S;          // [T, S]: the max-value samples
    float* score;                       // nullable [T, rows]
};
struct MesEpilogue;
template <bool ARD>
using MesKargs = PmArgsOf<ARD, true, MesEpilogue>;   // p.Zq: the pool; s: prediction's selection state

// gamma of sample ys at a row of mean m and deviation sigma, in the sense of PmArgs::maximize
__device__ __forceinline__ float mes_gamma(int maximize, float ys, float m, float sigma) { return (maximize ? (ys - m) : (m - ys)) / sigma; }

struct MesEpilogue {
    using Args = MesArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK& walk, f32x4 (&)[2][2]) {
        static_assert(POOL, "adkf_mes_pool: a shared pool");
        const PmArgs& a = args.p;
        const MesArgs& v = args.v;
        const int tid = threadIdx.x, row = tid & 63, part = tid >> 6, S = v.S;
        float* ps = tl.As;   // [4][64]: the partial sums (pm_mm's staging buffers are free here)
        if (row < tl.m) {
            const float mean = tl.mean(row), sigma = sqrtf(fmaxf(tl.var(row), 1e-12f));
            const float* ys = v.ystar + (size_t)tl.t * S;
            float sum = 0.f;
            for (int s = part; s < S; s += PM_NT / 64) sum += pm_mes_term(mes_gamma(a.maximize, ys[s], mean, sigma));
            ps[part * PM_TM + row] = sum;
        }
        __syncthreads();
        float score = 0.f;
        if (tid < tl.m) score = pm_sum4(ps, tid) * (1.f / (float)S);
        pm_tile_tail(args, tl, walk, score, v.score, tl.t, args.s.k, pm_excl(args.s, tl.t));
    }
};

// ---- flagged tasks: the float64 pool walk (pm64_pool_walk), lane s the term of sample s
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_mes_walk64(MesKargs<ARD> args) {
    const PmArgs& a = args.p;
    const MesArgs& v = args.v;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, S = v.S;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const float ys = lane < S ? v.ystar[(size_t)t * S + lane] : 0.f;
    pm64_pool_walk<ARD>(args, tk, kr[wv], args.s.k, pm_excl(args.s, t), [&](int64_t r, const float*, const double*, double s1, double s2) {
        const float mean = (float)s1, vl = (float)(tk.os - s2);
        const float sigma = sqrtf(fmaxf(vl, 1e-12f));
        float g = lane < S ? pm_mes_term(mes_gamma(a.maximize, ys, mean, sigma)) : 0.f;
        for (int o = 32; o > 0; o >>= 1) g += __shfl_xor(g, o);
        const float score = g * (1.f / (float)S);
        if (lane == 0 && v.score) v.score[(size_t)t * (size_t)a.rows + (size_t)r] = score;
        return score;
    });
}

}  // namespace adkf
