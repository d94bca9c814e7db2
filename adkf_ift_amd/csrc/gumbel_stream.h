// Gumbel max-value sampling over a shared pool (adkf_gumbel_pool; Wang and Jegelka 2017, section 3.1; BoTorch's
// _sample_max_value_Gumbel): samples of a task's optimum VALUE over the pool from the pool's posterior marginals alone.  The marginals
// are taken as independent, so with m_i, v_i the latent posterior of prediction, sigma_i = sqrt(max(v_i, 1e-12)) and mu_i = +-m_i
// (the score's sense: +f with ADKF_PM_MAXIMIZE, -f without)
//     Pr[max_i h_i < z] = prod_i Phi((z - mu_i) / sigma_i),    L(z) = sum_i -log Phi((z - mu_i) / sigma_i) = -log Pr.
// The quartiles of that distribution are found, a Gumbel is fitted to them and S values are drawn from it through the caller's
// uniforms.  No basis, no per-sample solve; the call is a REDUCTION of the whole pool per task, in three walks:
//   bracket   lo = max_i (mu_i - sigma_i), hi = max_i (mu_i + kappa sigma_i), kappa = max(1, Phi^-1(1 - 0.25 / rows)) from the host.
//             The maximising row alone gives log P(lo) <= log Phi(-1) < log 0.25, and the union bound gives 1 - P(hi) <=
//             rows (1 - Phi(kappa)) <= 0.25: all three quartiles lie in [lo, hi].
//   pass 1    GB_PROBES = 64 probes z_g = lo + (hi - lo) g / 63, L(z_g) for every g; k_gumbel_window takes g_lo, the largest g with
//             -L <= log 0.25, and g_hi, the smallest with -L >= log 0.75, and makes [z_g_lo, z_g_hi] the next window.
//   pass 2    the same 64 probes on that window; k_gumbel_fit finds, per quartile, the cell that brackets log q, interpolates -L
//             linearly in z (the left end where the cell is flat or empty), fits b = (q75 - q25) / (log log 4 - log log(4 / 3)),
//             a = q50 + b log log 2, and draws ystar_h = a - b log(-log u).
// A walk is k_predict_marginal's tile with GumbelEpilogue in the place of prediction's epilogue (m and v are prediction's, bit for
// bit), and k_gumbel_walk64 for float64 tasks (the float64 row loop, pm64_rows of predict_stream.h).
//
// Independent of the grid.  A float sum over a walk's chunk would depend on how many chunks a task has, which depends on the grid
// and on the other tasks.  Every term -log Phi is therefore turned into an unsigned 64-bit fixed-point number and added with
// integer adds only - inside the wave through shuffles, then ONE integer atomicAdd per probe and tile (float64 walk: per probe and
// wave) into sums [T, 64].  Integer addition is associative and commutative, so neither the order nor the atomics can change a
// bit; the project's rule is "no floating-point atomics" (large.h and large_fused.h use integer atomics already).  The two maxima
// go through the order-preserving integer image of a float and atomicMax.  Hence quant, gumbel and ystar of a task are the same
// bits alone or in a batch, and under any permutation of the pool's rows.
//     format      a term t in [0, GB_CLAMP = 32] becomes round-to-nearest-even(t 2^31): absolute resolution 2^-31 (4.7e-10), the
//                 error of a term at most 2^-32, so that of a sum at most rows 2^-32;
//     no wrap     rows GB_CLAMP 2^31 <= 2^63 for rows <= GB_ROWS_MAX = 2^27; more rows are refused (ADKF_E_SIZE).
// A probe whose sum reaches 32 has P < 1e-13 and only ever serves as "below the 25 % quantile", which is why the clamp is harmless.
// A NaN term (a NaN mean) counts as the clamp, and NaN rows are left out of the maxima.
#pragma once
#include "mes_stream.h"

namespace adkf {

constexpr int GB_PROBES = 64;                         // ADKF_GUMBEL_PROBES
constexpr float GB_CLAMP = 32.f;
constexpr float GB_FIX_SCALE = 2147483648.f;          // 2^31
constexpr double GB_FIX_UNIT = 1.0 / 2147483648.0;
constexpr int64_t GB_ROWS_MAX = (int64_t)1 << 27;
static_assert(GB_PROBES == 64, "one probe per lane");

// -log Phi(gamma), relative accuracy on both sides (the pieces of pm_mes_term and pm_log_ei):
//   gamma > 0        -log1p(-erfc(gamma / sqrt 2) / 2): the small tail keeps its digits;
//   -1 < gamma <= 0  as written, Phi in [0.15, 0.5];
//   gamma <= -1      a = -gamma: a^2 / 2 - log(erfcx(a / sqrt 2) / 2), no underflow of Phi.
// Clamped from above at GB_CLAMP (-inf gives the clamp, +inf gives 0).  NaN gives NaN.  Not inlined, for pm_log_ei's reason.
__device__ __noinline__ float pm_neg_log_cdf(float gamma) {
    float t;
    if (gamma > 0.f) t = -log1pf(-0.5f * erfcf(gamma * 0.70710678118654752f));
    else if (gamma > -1.f) t = -logf(0.5f * erfcf(-gamma * 0.70710678118654752f));
    else {
        const float a = -gamma;
        t = a > 16.f ? GB_CLAMP : 0.5f * a * a - logf(0.5f * erfcxf(a * 0.70710678118654752f));
    }
    return t > GB_CLAMP ? GB_CLAMP : t;
}

// the fixed-point image of a term (NaN: the clamp's)
__device__ __forceinline__ unsigned long long gb_fixed(float t) {
    return __float2ull_rn((t == t ? t : GB_CLAMP) * GB_FIX_SCALE);
}
// the order-preserving image of a float (never 0: 0 is "no row yet") and back
__device__ __forceinline__ unsigned int gb_image(float x) {
    const unsigned int u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gb_unimage(unsigned int u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

struct GumbelArgs {
    float* probes;                      // [T, 64]: the probes of the pass (probe mode)
    unsigned long long* sums;           // [T, 64]: the fixed-point sums (probe mode)
    unsigned int* mx;                   // [T, 2]: the images of lo and hi (bracket mode)
    float kappa; int bracket;           // bracket != 0: the walk takes the two maxima; otherwise the 64 sums
    const float* u; int S;              // k_gumbel_fit: the uniforms [T, S]
    float *ystar, *quant, *gumbel;      // k_gumbel_fit: [T, S], nullable [T, 3], nullable [T, 2]
};
struct GumbelEpilogue;
template <bool ARD>
using GumbelKargs = PmArgsOf<ARD, true, GumbelEpilogue>;   // p.Zq: the pool; s: an empty selection (k = 0)

// All 256 threads work: thread tid takes the row tid & 63 and the probes (tid >> 6), (tid >> 6) + 4, ...; a wave holds the 64 rows of the
// tile for its 16 probes, adds their fixed-point terms by shuffles and issues one atomicAdd per probe.  Rows >= tl.m contribute nothing.
struct GumbelEpilogue {
    using Args = GumbelArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK&, f32x4 (&)[2][2]) {
        static_assert(POOL, "adkf_gumbel_pool: a shared pool");
        const PmArgs& a = args.p;
        const GumbelArgs& v = args.v;
        const int tid = threadIdx.x, row = tid & 63, part = tid >> 6;
        const bool in = row < tl.m;
        float mu = 0.f, sigma = 1.f;
        if (in) {
            const float mean = tl.mean(row);
            sigma = sqrtf(fmaxf(tl.var(row), 1e-12f));
            mu = a.maximize ? mean : -mean;
        }
        if (v.bracket) {
            if (part != 0) return;
            float lo = in ? mu - sigma : -INFINITY, hi = in ? fmaf(v.kappa, sigma, mu) : -INFINITY;
            if (!(lo == lo) || !(hi == hi)) { lo = -INFINITY; hi = -INFINITY; }
            for (int o = 32; o > 0; o >>= 1) { lo = fmaxf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
            if (row == 0) {
                atomicMax(v.mx + 2 * (size_t)tl.t, gb_image(lo));
                atomicMax(v.mx + 2 * (size_t)tl.t + 1, gb_image(hi));
            }
            return;
        }
        const float* pr = v.probes + (size_t)tl.t * GB_PROBES;
        unsigned long long* sm = v.sums + (size_t)tl.t * GB_PROBES;
#pragma unroll 1
        for (int g = part; g < GB_PROBES; g += PM_NT / 64) {
            unsigned long long x = 0;
            if (in) x = gb_fixed(pm_neg_log_cdf((pr[g] - mu) / sigma));
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
            if (row == 0 && x) atomicAdd(sm + g, x);
        }
    }
};

// ---- flagged tasks: the float64 row loop over the whole pool (pm64_rows: grid (chunks, T), no list); lane g owns probe g and keeps its
// own integer sum over the wave's rows, one atomicAdd per lane at the end.  Bracket mode: the wave's two maxima.
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_gumbel_walk64(GumbelKargs<ARD> args) {
    const PmArgs& a = args.p;
    const GumbelArgs& v = args.v;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const float z = v.bracket ? 0.f : v.probes[(size_t)t * GB_PROBES + lane];
    unsigned long long acc = 0;
    float lo = -INFINITY, hi = -INFINITY;
    pm64_rows<ARD>(a, tk, 0, a.rows, kr[wv], [&](int64_t, const float*, const double*, double s1, double s2) {
        const float mean = (float)s1, vl = (float)(tk.os - s2);
        const float sigma = sqrtf(fmaxf(vl, 1e-12f));
        const float mu = a.maximize ? mean : -mean;
        if (v.bracket) {
            const float l = mu - sigma, h = fmaf(v.kappa, sigma, mu);
            if (l == l && h == h) { lo = fmaxf(lo, l); hi = fmaxf(hi, h); }
        } else {
            acc += gb_fixed(pm_neg_log_cdf((z - mu) / sigma));
        }
    });
    if (v.bracket) {
        if (lane == 0) {
            atomicMax(v.mx + 2 * (size_t)t, gb_image(lo));
            atomicMax(v.mx + 2 * (size_t)t + 1, gb_image(hi));
        }
    } else if (acc) {
        atomicAdd(v.sums + (size_t)t * GB_PROBES + lane, acc);
    }
}

// the 64 probes of the window [lo, hi]: both ends exact
__device__ __forceinline__ float gb_probe(float lo, float hi, int g) { return g == GB_PROBES - 1 ? hi : fmaf(hi - lo, (float)g / (float)(GB_PROBES - 1), lo); }

constexpr double GB_LOG_Q25 = -1.3862943611198906, GB_LOG_Q50 = -0.6931471805599453, GB_LOG_Q75 = -0.2876820724517809;

// ---- one wave per task, lane g the probe g.  pass 0: the window is the bracket (the two maxima); pass 1: the cell range of the pass-1
// sums that holds the three quartiles.  Writes probes [T, 64] of the next walk and zeroes the sums.
__global__ __launch_bounds__(64) void k_gumbel_window(GumbelArgs v, int pass) {
    const int t = blockIdx.x, g = threadIdx.x;
    float lo, hi;
    if (pass == 0) {
        const unsigned int il = v.mx[2 * (size_t)t], ih = v.mx[2 * (size_t)t + 1];
        lo = il ? gb_unimage(il) : 0.f;      // no row: a skipped task (k_gumbel_fit writes its outputs)
        hi = ih ? gb_unimage(ih) : 0.f;
    } else {
        const float z = v.probes[(size_t)t * GB_PROBES + g];
        const double nl = -(double)v.sums[(size_t)t * GB_PROBES + g] * GB_FIX_UNIT;
        const unsigned long long below = __ballot(nl <= GB_LOG_Q25), above = __ballot(nl >= GB_LOG_Q75);
        const int g_lo = below ? 63 - __clzll(below) : 0;
        int g_hi = above ? __ffsll(above) - 1 : GB_PROBES - 1;
        if (g_hi < g_lo) g_hi = g_lo;
        lo = __shfl(z, g_lo); hi = __shfl(z, g_hi);
    }
    v.probes[(size_t)t * GB_PROBES + g] = gb_probe(lo, hi, g);
    v.sums[(size_t)t * GB_PROBES + g] = 0;
}

// the quartile log q from the probes z and the sums nl = -L of pass 2 (lane g holds probe g): the cell whose right end is the first probe
// with -L >= log q, -L interpolated linearly in z; the left end where the cell is flat; the window's end where no cell brackets log q
__device__ __forceinline__ double gb_quartile(double z, double nl, double lq) {
    const unsigned long long above = __ballot(nl >= lq);
    const int g1 = above ? __ffsll(above) - 1 : GB_PROBES - 1;
    const int g0 = g1 > 0 ? g1 - 1 : 0;
    const double z0 = __shfl(z, g0), z1 = __shfl(z, g1), n0 = __shfl(nl, g0), n1 = __shfl(nl, g1);
    if (!above) return z1;
    if (g1 == 0 || n1 == n0 || z1 == z0) return z0;
    return z0 + (z1 - z0) * ((lq - n0) / (n1 - n0));
}

// ---- one wave per task: the three quartiles from the pass-2 sums, the Gumbel fit and the S draws (lane s the sample s).  Skipped tasks
// (n_s == 0, info != 0) and every task of an empty pool: quant = gumbel = -inf, ystar = -inf with ADKF_PM_MAXIMIZE and +inf without.
__global__ __launch_bounds__(64) void k_gumbel_fit(PmArgs a, GumbelArgs v) {
    const int t = blockIdx.x, g = threadIdx.x;
    const bool skipped = a.rows <= 0 || pm_kind_of(a, t) < 0;
    float fa = -INFINITY, fb = -INFINITY, f25 = -INFINITY, f50 = -INFINITY, f75 = -INFINITY;
    if (!skipped) {
        const double z = (double)v.probes[(size_t)t * GB_PROBES + g];
        const double nl = -(double)v.sums[(size_t)t * GB_PROBES + g] * GB_FIX_UNIT;
        const double q25 = gb_quartile(z, nl, GB_LOG_Q25), q50 = gb_quartile(z, nl, GB_LOG_Q50), q75 = gb_quartile(z, nl, GB_LOG_Q75);
        // log log 4 - log log(4 / 3) and log log 2
        double b = (q75 - q25) / 1.5725335836855194;
        if (!(b > 0.0)) b = 0.0;
        const double al = q50 + b * -0.36651292058166435;
        fa = (float)al; fb = (float)b;
        f25 = (float)q25; f50 = (float)q50; f75 = (float)q75;
    }
    if (g < 3 && v.quant) v.quant[(size_t)t * 3 + g] = g == 0 ? f25 : (g == 1 ? f50 : f75);
    if (g < 2 && v.gumbel) v.gumbel[(size_t)t * 2 + g] = g == 0 ? fa : fb;
    if (g < v.S) {
        float h = -INFINITY;
        if (!skipped) {
            const float uc = fminf(fmaxf(v.u[(size_t)t * v.S + g], 5.9604644775390625e-8f), 1.f - 5.9604644775390625e-8f);
            h = fa - fb * logf(-logf(uc));
        }
        v.ystar[(size_t)t * v.S + g] = a.maximize ? h : -h;
    }
}

}  // namespace adkf
