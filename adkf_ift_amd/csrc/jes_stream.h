// Joint entropy search over a shared pool (adkf_jes_pool; Hvarfner, Hutter and Nardi 2022; BoTorch's qLowerBoundJointEntropySearch at
// q = 1): a pool row x is scored by the information one noisy observation there carries about the task's optimum, LOCATION and VALUE
// together, given S samples (x*_s, f*_s) of that pair - pool rows opt_idx[t, s] and values opt_val[t, s], as adkf_thompson_pool's
// sel_idx / sel_val are.  With m(.), v(.), cov(., .) the latent posterior of prediction, noise the task's and cond_noise >= 0:
//     d_s      = max(v(x*_s), 1e-12) + cond_noise
//     c_s(x)   = cov(x, x*_s)
//     v_s(x)   = max(v(x) - c_s(x)^2 / d_s, 1e-12)                 the latent variance given f(x*_s) = f*_s
//     m_s(x)   = m(x) + c_s(x) (f*_s - m(x*_s)) / d_s
//     gamma_s  = mes_gamma(maximize, f*_s, m_s, sqrt(v_s))         the truncation at the sampled optimum
//     rho2_s   = v_s / (v_s + noise)
//     term_s   = log((vc + noise) / (v_s + noise)) - log1p(-rho2_s h(gamma_s)),   vc = max(v(x), 1e-12),   h: pm_gibbon_term's
//     score(x) = (1 / (2 S_eff)) sum over the valid s of term_s    both parts of a term are >= 0, so is the score
// An entry of opt_idx outside [0, rows) is skipped, S_eff counts the others, and a repeated row is NOT merged: two draws may share a
// location and differ in value.  Nothing is special at x = x*_s: the subtraction in v_s cancels, the clamp catches it, and rho2_s -> 0
// damps whatever gamma_s rounds to.
//
//   k_jes_refs grid (S, T), before the walks: the reference entry of believer_stream.h (bv_ref_entry) as k_kg_refs runs it, without the
//             first-occurrence merge, and with the latent variance at the entry, os - k . w, summed in float64 as the mean is
//             (float32 tasks: less w . (k - A w), which removes the first-order error of the float32 solve; see there).
//             From them 1 / d_s and the gain (f*_s - m(x*_s)) / d_s, once per entry.  The workgroup of entry 0 also leaves the task's
//             scale: -1 / (2 S_eff), or NaN when S_eff = 0 or a valid entry's value is NaN or infinite - every score of the task is then
//             NaN.  Skipped entries get zero rows, zeros in the per-entry arrays and the index -1.
//   the walk  is k_predict_marginal's tile with JesEpilogue: the believer's c0 panel (bv_c0_panel) with that state in the place of the
//             picks is c_s(x) for the tile's 64 rows; then the four-wave sum over the samples (pm_sum4, predict_stream.h) of
//             (log1p part) - (log part) of each term, its partial sums where the panel was once a barrier has declared it dead,
//             times the task's scale, as gb_score does, and the shared tail (pm_tile_tail).  No LDS beyond prediction's.
//   float64   tasks take k_jes_walk64, the float64 pool walk (pm64_pool_walk): lane s forms c_s in float64 (bv64_c0), the mean, the
//             variance and the covariance are rounded to float32 as the tile holds them, lane s forms its term and a fixed butterfly
//             adds them.
//   selection k_pool_topk, unchanged: the candidate lists are prediction's.
//
// With every sample valid and cond_noise so large that c^2 / d_s and the mean's shift round away, v_s = vc and m_s = m bit for bit,
// the logarithm is log 1 = 0 and the score is adkf_gibbon_pool's a(x) for ystar = opt_val, bit for bit, in both walks.
//
// A row whose own mean or variance is NaN scores NaN (an explicit test, as KgEpilogue's); NaN is never selected.  Deterministic: no
// atomics, every sum has a fixed order; a row's score depends on its task's data, the samples and its own features only.
#pragma once
#include "kg_stream.h"

namespace adkf {

struct JesArgs {
    int S;                              // samples per task
    const int64_t* opt_idx;             // [T, S]: the pool rows of the sampled optima
    const float* opt_val;               // [T, S]: their values, natural sign
    float cond_noise;
    float* W; double* W64;              // [T, S, ns_ld]: w of entry s (float64 tasks: W64; null without a float64 region)
    float* Xp;                          // [T, S, d]: the entries' feature rows
    float* am;                          // [T, S]: the posterior mean of entry s (0: skipped)
    float* ov;                          // [T, S]: its latent variance, unclamped
    float* invd;                        // [T, S]: 1 / d_s
    float* gain;                        // [T, S]: (f*_s - m(x*_s)) / d_s
    int64_t* ridx;                      // [T, S]: the pool row of entry s, -1: skipped
    float* scale;                       // [T]: -1 / (2 S_eff), NaN: every score of the task is NaN
    float *score, *opt_mean, *opt_var;  // nullable [T, rows], [T, S], [T, S]
};
struct JesEpilogue;
template <bool ARD>
using JesKargs = PmArgsOf<ARD, true, JesEpilogue>;   // p.Zq: the pool; s: prediction's selection state; ARD: r, the query scaling

// (log1p part) - (log part) of sample s at a row of mean m, latent variance vl (unclamped) and covariance c with the sample: -term_s
__device__ __forceinline__ float jes_term(int maximize, float ys, float m, float vl, float noise, float c, float invd, float gain) {
    const float vc = fmaxf(vl, 1e-12f);
    const float vs = fmaxf(fmaf(-(c * c), invd, vl), 1e-12f);
    const float ms = fmaf(c, gain, m);
    const float lg = logf((vc + noise) / (vs + noise));
    return pm_gibbon_term(mes_gamma(maximize, ys, ms, sqrtf(vs)), vs / (vs + noise)) - lg;
}

// ---- the reference state: one workgroup per (entry, task)
template <bool ARD>
__global__ __launch_bounds__(256) void k_jes_refs(JesKargs<ARD> args) {
    const PmArgs& a = args.p;
    const JesArgs& v = args.v;
    __shared__ __attribute__((aligned(16))) float fb[3 * TS_NS_MAX];
    __shared__ double red[256];
    const int j = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, S = v.S, ld = a.ns_ld;
    const size_t o = (size_t)t * S + j;
    const int kind = pm_kind_of(a, t);
    if (j == 0 && tid < 64) {   // the task's scale: lane s looks at entry s (S <= 64)
        bool valid = false, bad = false;
        if (tid < S) {
            const long long is = v.opt_idx[(size_t)t * S + tid];
            const float fs = v.opt_val[(size_t)t * S + tid];
            valid = kind >= 0 && is >= 0 && is < a.rows;
            bad = valid && !(fabsf(fs) < INFINITY);
        }
        const int n_eff = __popcll(__ballot(valid));
        const bool any_bad = __ballot(bad) != 0ull;
        if (tid == 0) v.scale[t] = (n_eff == 0 || any_bad) ? NAN : -0.5f / (float)n_eff;
    }
    const long long idx = v.opt_idx[o];
    const bool ok = kind >= 0 && idx >= 0 && idx < a.rows;   // (uniform) a repeated row counts again
    const bool f64 = kind == 2;
    const float mean = (float)bv_ref_entry<ARD>(args, t, ok, idx, v.Xp + o * a.d, v.W + o * ld, v.W64 ? v.W64 + o * ld : nullptr, fb, red);
    if (!ok) {   // (uniform)
        if (tid == 0) {
            v.ridx[o] = -1; v.am[o] = 0.f; v.ov[o] = 0.f; v.invd[o] = 0.f; v.gain[o] = 0.f;
            if (v.opt_mean) v.opt_mean[o] = 0.f;
            if (v.opt_var) v.opt_var[o] = 0.f;
        }
        return;
    }
    // k and w as bv_ref_entry has left them in fb: the latent variance at the entry, os - k . w, summed as the mean is
    const int n = pm_ns(a, t);
    const float* sc = a.scal + (size_t)t * NSCAL;
    const double os = sc[S_OS], il2 = 1.0 / ((double)sc[S_LS] * (double)sc[S_LS]);
    const float *rs = fb, *vs = fb + TS_NS_MAX;
    const double *k64 = reinterpret_cast<double*>(fb), *w64 = k64 + R64_MAXN;
    double pk = 0.0;
    for (int i = tid; i < n; i += 256) pk += f64 ? w64[i] * k64[i] : (double)vs[i] * (double)rs[i];
    // float32 tasks: w carries the error dw of a float32 solve, and os - k . w carries k . dw; the symmetric form os - 2 k . w + w . A w =
    // os - k . w - w . (k - A w) is exact to second order in dw.  A is regenerated from D2ss as pm_solve_refined does, here in float64
    double pr = 0.0;
    if (!f64) {
        const float* Dss = a.D2ss + (size_t)t * ld * ld;
        const double noise = sc[S_NOISE];
        for (int i = tid; i < n; i += 256) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += (os * kappa0(a.kind, (double)Dss[(size_t)k * ld + i] * il2) + (k == i ? noise : 0.0)) * (double)vs[k];
            pr += (double)vs[i] * ((double)rs[i] - s);
        }
    }
    const float var = (float)((os - bv_block_sum(pk, red)) - bv_block_sum(pr, red));
    if (tid == 0) {
        const float dd = fmaxf(var, 1e-12f) + v.cond_noise;
        v.ridx[o] = idx; v.am[o] = mean; v.ov[o] = var;
        v.invd[o] = 1.f / dd;
        v.gain[o] = (v.opt_val[o] - mean) / dd;
        if (v.opt_mean) v.opt_mean[o] = mean;
        if (v.opt_var) v.opt_var[o] = var;
    }
}

struct JesEpilogue {
    using Args = JesArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK& walk, f32x4 (&acc)[2][2]) {
        static_assert(POOL, "adkf_jes_pool: a shared pool");
        const PmArgs& a = args.p;
        const JesArgs& v = args.v;
        const int tid = threadIdx.x, row = tid & 63, part = tid >> 6, t = tl.t, S = v.S;
        float* C0 = tl.As;   // the c0 panel; at the end [4][64] partial sums
        {
            BvArgs bv{};
            bv.q = S; bv.W = v.W; bv.Xp = v.Xp;
            bv_c0_panel<ARD>(a, bv, tl, acc, S);
        }
        float sum = 0.f;
        if (row < tl.m) {
            const float vl = tl.var(row), mean = tl.mean(row);
            const size_t o = (size_t)t * S;
            const float* Cr = C0 + row * BV_LDC;
            for (int s = part; s < S; s += PM_NT / 64) {
                if (v.ridx[o + s] < 0) continue;
                sum += jes_term(a.maximize, v.opt_val[o + s], mean, vl, tl.noise, Cr[s], v.invd[o + s], v.gain[o + s]);
            }
        }
        __syncthreads();   // the panel is dead: the partial sums may overwrite it
        float* ps = tl.As;
        if (row < tl.m) ps[part * PM_TM + row] = sum;
        __syncthreads();
        float score = 0.f;
        if (tid < tl.m) {
            score = pm_sum4(ps, tid) * v.scale[t];
            if (tl.is_nan(tid)) score = NAN;   // a NaN mean or variance: NaN, never selected
        }
        pm_tile_tail(args, tl, walk, score, v.score, t, args.s.k, pm_excl(args.s, t));
    }
};

// ---- flagged tasks: the float64 pool walk (pm64_pool_walk), lane s the term of sample s
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_jes_walk64(JesKargs<ARD> args) {
    const PmArgs& a = args.p;
    const JesArgs& v = args.v;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, S = v.S;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const double* Wt = v.W64 + (size_t)t * S * tk.ld;
    const float* Xp = v.Xp + (size_t)t * S * a.d;
    const float noise = (float)tk.noise, scale = v.scale[t];
    const size_t o = (size_t)t * S + (lane < S ? lane : 0);
    const bool on = lane < S && v.ridx[o] >= 0;
    const float ys = v.opt_val[o], invd = v.invd[o], gain = v.gain[o];
    pm64_pool_walk<ARD>(args, tk, kr[wv], args.s.k, pm_excl(args.s, t), [&](int64_t r, const float* zq, const double* k, double s1, double s2) {
        const float mean = (float)s1, vl = (float)(tk.os - s2);
        const float c0 = (float)bv64_c0<ARD>(a, tk, zq, k, Wt, Xp, S, lane);
        float g = on ? jes_term(a.maximize, ys, mean, vl, noise, c0, invd, gain) : 0.f;
        for (int x = 32; x > 0; x >>= 1) g += __shfl_xor(g, x);
        float score = g * scale;
        if (s1 != s1 || s2 != s2) score = NAN;   // as the tile: a NaN mean or variance scores NaN
        if (lane == 0 && v.score) v.score[(size_t)t * (size_t)a.rows + (size_t)r] = score;
        return score;
    });
}

}  // namespace adkf
