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
//   k_jes_refs grid (S, T), before the walks: k_kg_refs over the same parts of k_bv_step (bv_store_row, bv_kernel_col, bv_solve_w) without
//             the first-occurrence merge, and with the latent variance at the entry, os - k . w, summed in float64 as the mean is
//             (float32 tasks: less w . (k - A w), which removes the first-order error of the float32 solve; see there).
//             From them 1 / d_s and the gain (f*_s - m(x*_s)) / d_s, once per entry.  The workgroup of entry 0 also leaves the task's
//             scale: -1 / (2 S_eff), or NaN when S_eff = 0 or a valid entry's value is NaN or infinite - every score of the task is then
//             NaN.  Skipped entries get zero rows, zeros in the per-entry arrays and the index -1.
//   the walk  is k_predict_marginal's tile with JesEpilogue: the believer's c0 panel (bv_c0_panel) with that state in the place of the
//             picks is c_s(x) for the tile's 64 rows; then, as MesEpilogue, thread tid takes the row tid & 63 and the samples tid >> 6,
//             + 4, ... and sums (log1p part) - (log part) of its terms; behind a barrier the panel is dead, the four partial sums meet
//             where it was, and thread i < 64 adds them in the order 0, 1, 2, 3 and multiplies by the task's scale, as gb_score does.
//             No LDS beyond prediction's.
//   float64   tasks take k_jes_walk64, k_kg_walk64's wave-per-row loop: lane s forms c_s in float64 (bv64_c0), the mean, the variance
//             and the covariance are rounded to float32 as the tile holds them, lane s forms its term and a fixed butterfly adds them.
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
    const int j = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, S = v.S, ld = a.ns_ld, d = a.d;
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
    float* Xj = v.Xp + o * d;
    float* Wj = v.W + o * ld;
    if (!ok) {   // (uniform) a skipped entry: nothing of it is read but by the panel, whose column is ignored
        for (int e = tid; e < d; e += 256) Xj[e] = 0.f;
        for (int i = tid; i < ld; i += 256) { Wj[i] = 0.f; if (v.W64) v.W64[o * ld + i] = 0.0; }
        if (tid == 0) {
            v.ridx[o] = -1; v.am[o] = 0.f; v.ov[o] = 0.f; v.invd[o] = 0.f; v.gain[o] = 0.f;
            if (v.opt_mean) v.opt_mean[o] = 0.f;
            if (v.opt_var) v.opt_var[o] = 0.f;
        }
        return;
    }
    const int n = pm_ns(a, t);
    const float* sc = a.scal + (size_t)t * NSCAL;
    const double os = sc[S_OS], il2 = 1.0 / ((double)sc[S_LS] * (double)sc[S_LS]);
    const float* ys = a.y_s + (size_t)t * ld;
    const float* xp = bv_store_row<ARD>(args, t, f64, a.Zq + (size_t)idx * d, Xj);
    const float *rs = fb, *vs = fb + TS_NS_MAX;
    const double *k64 = reinterpret_cast<double*>(fb), *w64 = k64 + R64_MAXN;
    bv_kernel_col(a, a.Zs + (size_t)t * ld * d, xp, n, os, il2, f64, reinterpret_cast<double*>(fb), fb);
    bv_solve_w(a, t, n, f64, fb, Wj, f64 ? v.W64 + o * ld : nullptr);
    for (int i = n + tid; i < ld; i += 256) { Wj[i] = 0.f; if (v.W64) v.W64[o * ld + i] = 0.0; }
    double pm = 0.0, pk = 0.0;
    for (int i = tid; i < n; i += 256) {
        const double wi = f64 ? w64[i] : (double)vs[i], ki = f64 ? k64[i] : (double)rs[i];
        pm += wi * (double)ys[i];
        pk += wi * ki;
    }
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
    const float mean = (float)bv_block_sum(pm, red);
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
            const float vl = tl.os - (tl.red[0][1][row] + tl.red[1][1][row]);
            const float mean = tl.red[0][0][row] + tl.red[1][0][row];
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
            score = (((ps[tid] + ps[PM_TM + tid]) + ps[2 * PM_TM + tid]) + ps[3 * PM_TM + tid]) * v.scale[t];
            const float mean = tl.red[0][0][tid] + tl.red[1][0][tid], vl = tl.red[0][1][tid] + tl.red[1][1][tid];
            if (mean != mean || vl != vl) score = NAN;   // a NaN mean or variance: NaN, never selected
            if (v.score) v.score[(size_t)t * (size_t)a.rows + (size_t)(tl.r0 + tid)] = score;
        }
        if (args.s.k > 0 && (tid >> 6) == 0)
            pm_list_merge(walk.lv, walk.li, args.s.k, score, (long long)(tl.r0 + tid), tid < tl.m, [&](long long r) { return pm_excluded(args.s, t, r); });
    }
};

// ---- flagged tasks: k_kg_walk64's loop (grid (chunks, T), one wave per pool row), lane s the term of sample s
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_jes_walk64(JesKargs<ARD> args) {
    const PmArgs& a = args.p;
    const JesArgs& v = args.v;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    float lv = -INFINITY;
    long long li = -1;
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, S = v.S;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const double* Wt = v.W64 + (size_t)t * S * tk.ld;
    const float* Xp = v.Xp + (size_t)t * S * a.d;
    const float noise = (float)tk.noise, scale = v.scale[t];
    const size_t o = (size_t)t * S + (lane < S ? lane : 0);
    const bool on = lane < S && v.ridx[o] >= 0;
    const float ys = v.opt_val[o], invd = v.invd[o], gain = v.gain[o];
    double* k = kr[wv];
    for (int64_t r = (int64_t)blockIdx.x * PM64_WAVES + wv; r < a.rows; r += (int64_t)gridDim.x * PM64_WAVES) {
        const float* zq = a.Zq + (size_t)r * a.d;
        double s1, s2;
        pm64_posterior_row<ARD>(a, tk, zq, k, s1, s2);
        const float mean = (float)s1, vl = (float)(tk.os - s2);
        const float c0 = (float)bv64_c0<ARD>(a, tk, zq, k, Wt, Xp, S, lane);
        float g = on ? jes_term(a.maximize, ys, mean, vl, noise, c0, invd, gain) : 0.f;
        for (int x = 32; x > 0; x >>= 1) g += __shfl_xor(g, x);
        float score = g * scale;
        if (s1 != s1 || s2 != s2) score = NAN;   // as the tile: a NaN mean or variance scores NaN
        if (lane == 0 && v.score) v.score[(size_t)t * (size_t)a.rows + (size_t)r] = score;
        if (args.s.k > 0) pm_list_merge(lv, li, args.s.k, score, (long long)r, lane == 0, [&](long long q) { return pm_excluded(args.s, t, q); });
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    if (args.s.k <= 0) return;   // (uniform)
    pm64_finish_walk(args.s, t, args.s.k, lv, li, [&](float x, long long i) { pm_list_merge(lv, li, args.s.k, x, i, i >= 0, [](long long) { return false; }); });
}

}  // namespace adkf
