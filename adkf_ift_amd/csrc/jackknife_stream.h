// Leave-one-out checks and jackknife+ prediction intervals over a shared pool (adkf_jackknife_pool; Rasmussen & Williams 2006,
// section 5.4.2, for the leave-one-out forms - GPyTorch's LeaveOneOutPseudoLikelihood, BoTorch's batch_cross_validation; Barber,
// Candes, Ramdas & Tibshirani 2021, "Predictive inference with the jackknife+", for the intervals).  Per task, with n support points
// at the GIVEN phi - the hyperparameters are NOT refitted per fold - A = K_ss + noise I, B = A^-1, alpha = B y (zero prior mean),
// m(x) and v(x) prediction's mean and latent variance of pool row x, c_i(x) = sum_j K(x, z_j) B_ji:
//     g_i          = alpha_i / B_ii                         = y_i - mu_-i(z_i), the leave-one-out residual
//     loo_mean_i   = y_i - g_i,     loo_var_i = 1 / B_ii    (the observed variance, noise included)
//     loo_lpd      = sum_i [ -log(2 pi / B_ii) / 2 - g_i^2 B_ii / 2 ]                      (R&W eq. 5.10), by ascending i
//     mu_-i(x)     = m(x) - c_i(x) g_i                      the prediction at x of the model without point i
//     v_-i(x)      = v(x) + c_i(x)^2 / B_ii                 its latent variance
// Deleting a point needs no refit: both are rank-one updates of the posterior every pool call already holds.  The fold values of a row:
//     plain        a_i = mu_-i(x) - |g_i|,                  b_i = mu_-i(x) + |g_i|
//     scaled       a_i = mu_-i(x) - s_i sd_i(x),            b_i = mu_-i(x) + s_i sd_i(x)          (ADKF_PM_JK_SCALED)
//                  s_i = |g_i| sqrt(B_ii),                  sd_i(x) = sqrt(max(v_-i(x), 1e-12) + noise)
// and for level alpha_l the rank k = floor((double)alpha_l (n + 1)) - the float32 level times a small integer is exact in double, so
// the rank is a function of the bits passed; a level that is NaN, <= 0 or >= 1 has k = 0:
//     lo[t, l, x]  = the k-th smallest a_i,                 hi[t, l, x] = the k-th largest b_i,          -inf / +inf for k = 0.
// [lo, hi] covers a new label with probability >= 1 - 2 alpha for the fixed-phi predictor, whatever the data's distribution; with phi
// fitted on the same points that is a very good approximation, not a theorem.  Order statistics are VALUES, so the answer does not
// depend on how they are found.
//
//   k_jk_state one workgroup per task before the walks (k_kg_refs' role): alpha by the one-step refined solve Thompson and the believer
//              use (pm_solve_refined), B_ii from the float32 A^-1 - flagged tasks: k_refine64's float64 A^-1, alpha = A^-1 y in
//              float64 - then g, 1 / B_ii and the width factor (|g| or s) into the scratch (with float64 twins for flagged tasks),
//              the L ranks, and the three leave-one-out outputs, the density summed in float64 in a fixed order.
//   the walk   is k_predict_marginal's tile with JkEpilogue, so m and v are adkf_predict_pool's bit for bit.  The epilogue needs the
//              row tile C = K B itself, which the tile only holds reduced: it is formed again panel by panel from Kb and A^-1 on the
//              matrix pipe (the product of the tile, operand for operand) into the epilogue's own LDS, [64, 257] floats.  Then ONE
//              WAVE PER ROW, 16 rows each: lane e holds the fold values i = e, e + 64, e + 128, e + 192 as unsigned keys in the
//              order of the values.  The k-th smallest key is the LARGEST T with fewer than k keys below it, and that T is built
//              bit by bit from the top: per bit one compare of each held key against the wave-uniform candidate, a ballot and a
//              scalar count - 32 n / 64 vector instructions per order statistic whatever n is, no LDS, no barrier, no padding to a
//              power of two and no tie-break (equal values give the same answer).  The k-th largest b is the k-th smallest of the
//              complemented keys, and the two searches run in one loop.  Rank-by-counting (n compares per value) and a bitonic
//              network (log^2 n exchanges per value, padded) both cost several times that at n = 128; DESIGN.md has the numbers.
//              The level-0 score (lo with ADKF_PM_MAXIMIZE, -hi without; infinite -> NaN, never selected) goes through pm_tile_tail.
//              With the 66 KB of the epilogue a plain task keeps a resident row tile up to 256 points; refined tasks beyond 128
//              points move to the global slots - correct, not tuned.
//   float64    tasks take k_jk_walk64 (pm64_pool_walk): c = k A^-1 in float64 per lane, the fold values from the float64 twins,
//              rounded to float32, then the same selection.
//
// A row whose own mean or variance is NaN gets NaN bounds and is never selected.  Deterministic: no atomics, every sum in a fixed
// order; a task's outputs do not depend on the grid or on the other tasks.
#pragma once
#include "believer_stream.h"

namespace adkf {

constexpr int JK_NS_MAX = 256;              // support points per task: four fold values per lane
constexpr int JK_LV_MAX = 8;                // levels per call
constexpr int JK_Q = JK_NS_MAX / 64;
constexpr int JK_LDC = JK_NS_MAX + 1;       // leading dimension of the epilogue's C tile
constexpr int JK_EPI_LDS = (PM_TM * JK_LDC + PM_TM) * (int)sizeof(float);

struct JkArgs {
    int L, scaled;
    const float* alpha;                 // [L]: the levels
    float *g, *rv, *wd;                 // [T, ns_ld]: g_i, 1 / B_ii and the width factor (|g_i|, scaled: s_i); 0 beyond n
    double *g64, *rv64, *wd64;          // their float64 twins (flagged tasks; null without a float64 region)
    int32_t* rank;                      // [T, JK_LV_MAX]: the rank of every level, 0: none
    float *lo, *hi;                     // nullable [T, L, rows]
    float *loo_mean, *loo_var, *loo_lpd;   // nullable [T, ns_ld], [T, ns_ld], [T]
};
struct JkEpilogue;
template <bool ARD>
using JkKargs = PmArgsOf<ARD, true, JkEpilogue>;   // p.Zq: the pool; s: prediction's selection state; ARD: r, the query scaling

// the rank of level al among n points
__device__ __forceinline__ int jk_rank(float al, int n) {
    if (!(al > 0.f && al < 1.f) || n <= 0) return 0;
    return (int)floor((double)al * (double)(n + 1));
}

// ---- the leave-one-out state: one workgroup per task (grid (1, T))
template <bool ARD>
__global__ __launch_bounds__(256) void k_jk_state(JkKargs<ARD> args) {
    const PmArgs& a = args.p;
    const JkArgs& v = args.v;
    __shared__ float fb[3 * JK_NS_MAX];
    __shared__ double red[256];
    const int t = blockIdx.y, tid = threadIdx.x, ld = a.ns_ld;
    const int kind = pm_kind_of(a, t);
    const int n = kind >= 0 ? pm_ns(a, t) : 0;
    const size_t so = (size_t)t * ld;
    if (tid < JK_LV_MAX) v.rank[(size_t)t * JK_LV_MAX + tid] = tid < v.L ? jk_rank(v.alpha[tid], n) : 0;
    if (ld > JK_NS_MAX || n <= 0) {   // (uniform; the host refuses ld > JK_NS_MAX) a skipped task: its outputs stay 0
        for (int i = tid; i < ld; i += 256) { v.g[so + i] = 0.f; v.rv[so + i] = 0.f; v.wd[so + i] = 0.f; }
        return;
    }
    const bool f64 = kind == 2;
    const float* ys = a.y_s + so;
    double al = 0.0, bii = 1.0;
    if (f64) {
        const double* A1 = a.w64 + (size_t)t * a.w64_stride;
        if (tid < n) {
            for (int k = 0; k < n; ++k) al += A1[(size_t)k * ld + tid] * (double)ys[k];
            bii = A1[(size_t)tid * ld + tid];
        }
    } else {
        const float* sc = a.scal + (size_t)t * NSCAL;
        const float* Ai = a.Ainv + (size_t)t * ld * ld;
        float *rs = fb, *vs = fb + JK_NS_MAX, *es = fb + 2 * JK_NS_MAX;
        if (tid < n) rs[tid] = ys[tid];
        __syncthreads();
        pm_solve_refined(Ai, a.D2ss + (size_t)t * ld * ld, a.kind, sc[S_OS], sc[S_NOISE], 1.f / (sc[S_LS] * sc[S_LS]), n, ld, rs, vs, es);
        if (tid < n) { al = vs[tid]; bii = Ai[(size_t)tid * ld + tid]; }   // (entry tid of vs is this thread's own)
    }
    double term = 0.0;
    if (tid < ld) {
        const bool in = tid < n;
        const double g = in ? al / bii : 0.0, rv = in ? 1.0 / bii : 0.0;
        const double wd = in ? (v.scaled ? fabs(g) * sqrt(bii) : fabs(g)) : 0.0;
        v.g[so + tid] = (float)g; v.rv[so + tid] = (float)rv; v.wd[so + tid] = (float)wd;
        if (v.g64) { v.g64[so + tid] = g; v.rv64[so + tid] = rv; v.wd64[so + tid] = wd; }
        if (in) {
            if (v.loo_mean) v.loo_mean[so + tid] = (float)((double)ys[tid] - g);
            if (v.loo_var) v.loo_var[so + tid] = (float)rv;
            term = -0.5 * log(6.283185307179586 * rv) - 0.5 * g * g * bii;
        }
    }
    const double lpd = bv_block_sum(term, red);
    if (tid == 0 && v.loo_lpd) v.loo_lpd[t] = (float)lpd;
}

// the image of a float under which the unsigned order is the order of the values (-0 before +0), and back
__device__ __forceinline__ unsigned jk_key(float x) { const unsigned u = __float_as_uint(x); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float jk_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- one wave (all 64 lanes): the k-th smallest of the 64 NQ keys ka (into ta) and of the keys kb (into tb), k >= 1 and uniform.  The
// k-th smallest key is the largest T with fewer than k keys below it, built bit by bit from the top: per bit one compare per held key
// against the uniform candidate, a ballot and a scalar count.  Straight-line code (the two searches give each other's scalar chain
// something to overlap with): a branch per bit costs a wave that runs alone on its SIMD more than the compares do.
template <int NQ>
__device__ __forceinline__ void jk_search(const unsigned (&ka)[JK_Q], const unsigned (&kb)[JK_Q], int k, unsigned& ta, unsigned& tb) {
    ta = 0u; tb = 0u;   // (uniform: every count is a ballot's)
#pragma unroll
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned ca = ta | (1u << bit), cb = tb | (1u << bit);
        int na = 0, nb = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) { na += __popcll(__ballot(ka[q] < ca)); nb += __popcll(__ballot(kb[q] < cb)); }
        ta = na < k ? ca : ta;
        tb = nb < k ? cb : tb;
    }
}

// ---- one wave (all 64 lanes), one pool row r of task t: lane e holds the fold values av[q], bv[q] of the points e + 64 q (anything
// beyond n); lo and hi of every level are written by lane 0; returns the level-0 score.  bad: the row's own mean or variance is NaN.
// The k-th largest b is the k-th smallest complemented key.
__device__ __forceinline__ float jk_select(const PmArgs& a, const JkArgs& v, int t, int64_t r, int n, const float (&av)[JK_Q], const float (&bv)[JK_Q],
                                           bool bad) {
    const int lane = threadIdx.x & 63;
    unsigned ka[JK_Q], kb[JK_Q];    // beyond n: the last key, which is below no candidate
#pragma unroll
    for (int q = 0; q < JK_Q; ++q) {
        const bool in = lane + 64 * q < n;
        ka[q] = in ? jk_key(av[q]) : 0xffffffffu; kb[q] = in ? ~jk_key(bv[q]) : 0xffffffffu;
    }
    float s0 = NAN;
    for (int l = 0; l < v.L; ++l) {
        const int k = v.rank[(size_t)t * JK_LV_MAX + l];   // (uniform)
        float lo = -INFINITY, hi = INFINITY;
        if (k > 0) {
            unsigned ta, tb;
            if (n <= 64) jk_search<1>(ka, kb, k, ta, tb);
            else if (n <= 128) jk_search<2>(ka, kb, k, ta, tb);
            else jk_search<JK_Q>(ka, kb, k, ta, tb);
            lo = jk_unkey(ta); hi = jk_unkey(~tb);
        }
        if (bad) { lo = NAN; hi = NAN; }
        if (lane == 0) {
            const size_t o = ((size_t)t * v.L + l) * (size_t)a.rows + (size_t)r;
            if (v.lo) v.lo[o] = lo;
            if (v.hi) v.hi[o] = hi;
        }
        if (l == 0) s0 = a.maximize ? lo : -hi;
    }
    return fabsf(s0) == INFINITY ? NAN : s0;   // no bound at this level: never selected
}

struct JkEpilogue {
    using Args = JkArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK& walk, f32x4 (&acc)[2][2]) {
        static_assert(POOL, "adkf_jackknife_pool: a shared pool");
        __shared__ float Cj[PM_TM * JK_LDC];                                           // the row tile C = K A^-1
        __shared__ float srow[PM_TM];                                                  // the rows' scores
        const PmArgs& a = args.p;
        const JkArgs& v = args.v;
        const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, t = tl.t, n = tl.n, ld = tl.ld, ns_ld = a.ns_ld;
        if (tl.nk > JK_NS_MAX) return;   // (uniform; the host refuses such batches)
        const float* Ai = a.Ainv + (size_t)t * ns_ld * ns_ld;
        const float* Kb = tl.Kb;
        float dummy[2];
        for (int j0 = 0; j0 < tl.nk; j0 += PM_TM) {   // the tile's own product, operand for operand
            pm_mm<false>(acc, tl.nk, tl.As, tl.Bs,
                [=](int i, int k, float (&x)[4]) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = Kb[(size_t)i * ld + k + e];
                },
                [=](int j, int k, float (&x)[4]) {
                    if (j0 + j >= n) { x[0] = x[1] = x[2] = x[3] = 0.f; return; }
                    pm_ld4(Ai + (size_t)(j0 + j) * ns_ld, k, n, false, x);
                }, dummy, dummy);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Cj[pm_row(i, r) * JK_LDC + j0 + pm_col(j)] = acc[i][j][r];
        }
        __syncthreads();
        const size_t so = (size_t)t * ns_ld;
        float gi[JK_Q], ri[JK_Q], wi[JK_Q];
#pragma unroll
        for (int q = 0; q < JK_Q; ++q) {
            const int i = lane + 64 * q;
            const bool in = i < n;
            gi[q] = in ? v.g[so + i] : 0.f; ri[q] = in ? v.rv[so + i] : 0.f; wi[q] = in ? v.wd[so + i] : 0.f;
        }
        const int nq = tl.nk >> 6;
        for (int row = wv; row < tl.m; row += PM_NT / 64) {
            const float m = tl.mean(row), vl = tl.var(row);
            float av[JK_Q], bv[JK_Q];
#pragma unroll
            for (int q = 0; q < JK_Q; ++q) {
                av[q] = INFINITY; bv[q] = -INFINITY;
                if (q < nq && lane + 64 * q < n) {
                    const float c = Cj[row * JK_LDC + lane + 64 * q];
                    const float mu = fmaf(-c, gi[q], m);
                    float w = wi[q];
                    if (v.scaled) w *= sqrtf(fmaxf(fmaf(c * c, ri[q], vl), 1e-12f) + tl.noise);
                    av[q] = mu - w; bv[q] = mu + w;
                }
            }
            const float s = jk_select(a, v, t, tl.r0 + row, n, av, bv, tl.is_nan(row));
            if (lane == 0) srow[row] = s;
        }
        __syncthreads();
        const float score = tid < tl.m ? srow[tid] : 0.f;
        pm_tile_tail(args, tl, walk, score, nullptr, 0, args.s.k, pm_excl(args.s, t));
    }
};
static_assert(JK_NS_MAX == ADKF_JK_POINTS_MAX && JK_LV_MAX == ADKF_JK_LEVELS_MAX && JK_NS_MAX <= R64_MAXN, "jackknife_stream.h limits");

// ---- flagged tasks: the float64 pool walk (pm64_pool_walk), lane e the points e, e + 64, ...
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_jk_walk64(JkKargs<ARD> args) {
    const PmArgs& a = args.p;
    const JkArgs& v = args.v;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    if (tk.n > JK_NS_MAX || !v.g64) return;     // (uniform; the host refuses such batches)
    const int n = tk.n;
    const size_t so = (size_t)t * tk.ld;
    double gi[JK_Q], ri[JK_Q], wi[JK_Q];
#pragma unroll
    for (int q = 0; q < JK_Q; ++q) {
        const int i = lane + 64 * q;
        const bool in = i < n;
        gi[q] = in ? v.g64[so + i] : 0.0; ri[q] = in ? v.rv64[so + i] : 0.0; wi[q] = in ? v.wd64[so + i] : 0.0;
    }
    pm64_pool_walk<ARD>(args, tk, kr[wv], args.s.k, pm_excl(args.s, t), [&](int64_t r, const float*, const double* k, double s1, double s2) {
        const double vl = tk.os - s2;
        float av[JK_Q], bv[JK_Q];
#pragma unroll
        for (int q = 0; q < JK_Q; ++q) {
            const int i = lane + 64 * q;
            av[q] = INFINITY; bv[q] = -INFINITY;
            if (i < n) {
                double c = 0.0;   // (pm64_posterior_row's c, which it does not keep)
                for (int p = 0; p < n; ++p) c += k[p] * tk.A1[(size_t)p * tk.ld + i];
                const double mu = s1 - c * gi[q];
                double w = wi[q];
                if (v.scaled) w *= sqrt(fmax(vl + c * c * ri[q], 1e-12) + tk.noise);
                av[q] = (float)(mu - w); bv[q] = (float)(mu + w);
            }
        }
        return jk_select(a, v, t, r, n, av, bv, s1 != s1 || s2 != s2);
    });
}

}  // namespace adkf
