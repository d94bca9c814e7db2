// Feature gradients of streaming prediction (adkf_predict_grad): the vector-Jacobian product of adkf_predict_marginal(_ard) with
// respect to the PACKED query rows,
//     dZq[r, :] = d/dZq[r, :] ( g_mean[r] mean[r] + g_var[r] var[r] + g_ei[r] ei[r] ),
// in the workspace of the packed call, whatever the number of rows.  With k_i = os kappa(u_i), u_i = |x - z_i|^2 / l^2,
// G_i = os kappa'(u_i) (kappa3's k1 = d kappa / du), c = k A^-1 and alpha = A^-1 y:
//     a_m = g_mean + g_ei dE/dmean,     a_v = g_var + g_ei dE/dvar            (gd_coef; var is the latent variance: the noise is a constant)
//     W_i = G_i (a_m alpha_i - 2 a_v c_i)
//     dZq[r, :] = (2 / l^2) ( (sum_i W_i) (x - mu) - sum_i W_i (z_i - mu) )    (the centred features of the K panel)
// ARD: the same on the scaled features at unit lengthscale, then one more factor 1 / l_c per dimension (the gradient is the raw row's).
//
// k_predict_grad_tile - the matrix pipe, plain tasks (pm_kind_of == 0, so at most 128 points): prediction's walk over (task, 64-row
// tile).  Three row tiles [64, ld] stay in LDS: K, G (both from the same D^2 of pm_mm<true>) and C = K A^-1 (pm_mm, A^-1 through L2),
// reduced on the fly to the mean and the variance as in k_predict_marginal; alpha = A^-1 y is one more vector.  The first 64 threads
// turn the two reductions and the row's cotangents into (a_m, a_v); W overwrites G, four threads per row, which also sum it; then the
// third product W (Z_s - mu) runs through pm_mm in 64-column chunks of d (tail chunk and d % 4 != 0 included: the operand loads are
// guarded element by element), the (sum_i W_i) (x - mu) term joins in the epilogue, and a [64, 64] block of dZq is stored per chunk.
// LDS: 3 x 64 x 132 floats + 128 = 99.5 KB dynamic at 128 points, 18.5 KB static - one workgroup per CU.
//
// k_predict_grad_row - everything else (refined tasks, more than 128 points, tasks flagged for float64), one workgroup per row, correct
// and not tuned.  Float32 tasks: k and G from difference-form distances, c and alpha through pm_solve_refined (one refinement step with
// A regenerated from D2ss).  Flagged tasks: the float64 kernel row of pm64_kernel_row's arithmetic, c and alpha against k_refine64's
// float64 A^-1.  Both: the two reductions, the coefficients and the sums over the support points in float64, rounded once.
//
// Rows of no task's range and rows of tasks with n_s == 0 or info != 0 stay 0 (the host zeroes dZq first).  A row whose cotangents
// are all zero is written as +0.  No atomics; a row's result depends on its task and its own features only; every sum has a fixed order.
#pragma once
#include "thompson_stream.h"

namespace adkf {

struct PgArgs {
    const float *g_mean, *g_var, *g_ei;     // [rows] each, nullable
    float* dZq;                             // [rows, d]
    int row_kinds;                          // the kinds (bit mask over pm_kind_of) that k_predict_grad_row serves
};
template <bool ARD>
struct PgArgsOf { PmArgs p; std::conditional_t<ARD, PmArd, PmNoArd> r; PgArgs g; };

// Phi(u) / h(u) and phi(u) / h(u), h = phi + u Phi, float32: h directly for u > -1; below, with a = -u and q = sqrt(pi / 2) erfcx(a / sqrt 2),
// Phi = phi q and h = phi b, b = 1 - a q (pm_log_ei's b: it cancels to ~a^-2, a relative 64 eps32 at a = 8); beyond a = 8 the series
// b = a^-2 (1 - 3 a^-2 + 15 a^-4 - 105 a^-6 + 945 a^-8 - 10395 a^-10), first omitted term 2e-6, and Phi = phi (1 - b) / a.
__device__ __noinline__ void gd_ei_ratios(float u, float& cdf_h, float& pdf_h) {
    if (u > -1.f) {
        const float cdf = 0.5f * erfcf(-u * 0.70710678118654752f);
        const float pdf = 0.3989422804014327f * expf(-0.5f * u * u);
        const float h = fmaf(u, cdf, pdf);
        cdf_h = cdf / h; pdf_h = pdf / h;
        return;
    }
    const float a = -u;
    float b;
    if (u > -8.f) {
        const float q = 1.2533141373155003f * erfcxf(a * 0.70710678118654752f);
        b = fmaf(-a, q, 1.f);
        cdf_h = q / b;
    } else {
        const float w = 1.f / (a * a);
        b = w * fmaf(fmaf(fmaf(fmaf(fmaf(-10395.f, w, 945.f), w, -105.f), w, 15.f), w, -3.f), w, 1.f);
        cdf_h = (1.f - b) / (a * b);
    }
    pdf_h = 1.f / b;
}
// float64: h directly down to u = -20 (the cancellation costs a^2 eps64), the series summed while its terms shrink below
__device__ __noinline__ void gd_ei_ratios(double u, double& cdf_h, double& pdf_h) {
    if (u > -20.0) {
        const double cdf = 0.5 * erfc(-u * 0.70710678118654752), pdf = 0.3989422804014327 * exp(-0.5 * u * u);
        const double h = pdf + u * cdf;
        cdf_h = cdf / h; pdf_h = pdf / h;
        return;
    }
    const double a = -u, w = 1.0 / (a * a);
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 64; ++k) {
        const double next = -term * (2 * k + 1) * w;
        if (fabs(next) >= fabs(term)) break;
        sum += term = next;
    }
    const double b = w * sum;
    pdf_h = 1.0 / b; cdf_h = (1.0 - b) / (a * b);
}
__device__ __forceinline__ float gd_cdf(float u) { return 0.5f * erfcf(-u * 0.70710678118654752f); }
__device__ __forceinline__ double gd_cdf(double u) { return 0.5 * erfc(-u * 0.70710678118654752); }
__device__ __forceinline__ float gd_pdf(float u) { return 0.3989422804014327f * expf(-0.5f * u * u); }
__device__ __forceinline__ double gd_pdf(double u) { return 0.3989422804014327 * exp(-0.5 * u * u); }

// (a_m, a_v) of row r of task t from its mean and latent variance, in R = float or double.  pm_ei's sigma and u; where the clamp of
// sigma is active the derivative through sigma is 0.
template <class R>
__device__ __forceinline__ void gd_coef(const PmArgs& a, const PgArgs& g, int t, int64_t r, R mean, R vl, R& am, R& av) {
    am = g.g_mean ? (R)g.g_mean[r] : (R)0;
    av = g.g_var ? (R)g.g_var[r] : (R)0;
    if (!g.g_ei) return;
    const R ge = (R)g.g_ei[r], best = (R)a.best_f[t];
    const bool live = vl > (R)1e-12;
    const R sigma = sqrt(live ? vl : (R)1e-12), sgn = a.maximize ? (R)1 : (R)-1;
    const R u = sgn * (mean - best) / sigma;
    if (a.log_ei) {
        R ch, ph;
        gd_ei_ratios(u, ch, ph);
        am += ge * (sgn * ch / sigma);
        if (live) av += ge * (ph / ((R)2 * vl));
    } else {
        am += ge * (sgn * gd_cdf(u));
        if (live) av += ge * (gd_pdf(u) / ((R)2 * sigma));
    }
}

// pm_k_panel with two destinations: K = os kappa and G = os kappa' of the same D^2 (kappa3), zero outside (m, n)
template <bool ARD>
__device__ __forceinline__ void gd_kg_panel(const PmArgs& a, const float* Zs, const float* mu, const float* il, int64_t r0, int m, int n, int j0,
                                            float os, float il2, float* As, float* Bs, float (&rowsq)[2][PM_TM], f32x4 (&acc)[2][2],
                                            float* Kd, float* Gd, size_t ldd) {
    const int tid = threadIdx.x, kind = a.kind;
    const int64_t d = a.d;
    float sqa[2] = {0.f, 0.f}, sqb[2] = {0.f, 0.f};
    pm_mm<true>(acc, a.d, As, Bs, pm_query_rows<ARD>(a, mu, il, r0, m),
        [&](int j, int k, float (&v)[4]) {
            if (j0 + j >= n) { v[0] = v[1] = v[2] = v[3] = 0.f; return; }
            if constexpr (ARD) {
                pm_ld4(Zs + (size_t)(j0 + j) * d, k, a.d, a.vec, v);
            } else {
                float z[4], c[4];
                pm_ld4(Zs + (size_t)(j0 + j) * d, k, a.d, a.vec, z); pm_ld4(mu, k, a.d, a.vec, c);
#pragma unroll
                for (int x = 0; x < 4; ++x) v[x] = z[x] - c[x];
            }
        }, sqa, sqb);
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        float x = sqa[ps], y = sqb[ps];
        x += dpp_f<DPP_XOR1>(x); x += dpp_f<DPP_XOR2>(x); x += dpp_f<DPP_HALF_MIRROR>(x);
        y += dpp_f<DPP_XOR1>(y); y += dpp_f<DPP_XOR2>(y); y += dpp_f<DPP_HALF_MIRROR>(y);
        if ((tid & 7) == 0) { rowsq[0][(tid >> 3) + ps * 32] = x; rowsq[1][(tid >> 3) + ps * 32] = y; }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ii = pm_row(i, r), jj = pm_col(j);
                const float d2 = fmaxf(rowsq[0][ii] + rowsq[1][jj] - 2.f * acc[i][j][r], 0.f);
                float k0, k1, k2;
                kappa3(kind, d2 * il2, k0, k1, k2);
                const bool in = ii < m && j0 + jj < n;
                Kd[(size_t)ii * ldd + jj] = in ? os * k0 : 0.f;
                Gd[(size_t)ii * ldd + jj] = in ? os * k1 : 0.f;
            }
    __syncthreads();
}

template <bool ARD>
__global__ __launch_bounds__(PM_NT) void k_predict_grad_tile(PgArgsOf<ARD> args) {
    const PmArgs& a = args.p;
    const PgArgs& g = args.g;
    extern __shared__ __attribute__((aligned(16))) float pg_lds[];
    __shared__ float ABs[2 * PM_TM * LD_MN];
    float *As = ABs, *Bs = ABs + PM_TM * LD_MN;
    __shared__ float rowsq[2][PM_TM];
    __shared__ float red[2][2][PM_TM];
    __shared__ float coef[3][PM_TM];   // a_m, a_v, sum_i W_i of the tile's rows
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wc = wv & 1;
    const int ld = a.buf_ld;
    float *Kb = pg_lds, *Gb = Kb + (size_t)PM_TM * ld, *Cb = Gb + (size_t)PM_TM * ld, *al = Cb + (size_t)PM_TM * ld;
    const int grid = gridDim.x;
    const int64_t d = a.d;
    // prediction's walk over the tiles of all tasks, in order: (t, first tile of t) is a cursor that only moves forward
    int t = 0;
    int64_t tile0 = 0;
    for (int64_t w = blockIdx.x;; w += grid) {
        int64_t lo, hi;
        for (;;) {
            if (t >= a.T) return;
            pm_range(a, t, lo, hi);
            const int64_t nt = (hi - lo + PM_TM - 1) / PM_TM;
            const bool mine = pm_kind_of(a, t) == 0;
            if (w < tile0 + nt && mine) break;
            tile0 += nt; ++t;
            if (w < tile0) w = tile0 + (((int64_t)blockIdx.x - tile0) % grid + grid) % grid;
        }
        const int64_t r0 = lo + (w - tile0) * PM_TM;
        const int m = (int)(hi - r0 < PM_TM ? hi - r0 : PM_TM);
        const int n = pm_ns(a, t);
        const float* sc = a.scal + (size_t)t * NSCAL;
        const float os = sc[S_OS], il2 = 1.f / (sc[S_LS] * sc[S_LS]);
        const float* Zs = a.Zs + (size_t)t * a.ns_ld * d;
        const float* mu = a.mean_s + (size_t)t * d;
        const float* il = nullptr;
        if constexpr (ARD) il = args.r.il + (size_t)t * d;
        const float* Ai = a.Ainv + (size_t)t * a.ns_ld * a.ns_ld;
        const float* ys = a.y_s + (size_t)t * a.ns_ld;
        const int np = (n + PM_TM - 1) / PM_TM;
        const int nk = np * PM_TM;   // <= ld - 4
        f32x4 acc[2][2];
        // ---- K and G row tiles
        for (int p = 0; p < np; ++p) {
            const int j0 = p * PM_TM;
            gd_kg_panel<ARD>(a, Zs, mu, il, r0, m, n, j0, os, il2, As, Bs, rowsq, acc, Kb + j0, Gb + j0, ld);
        }
        // ---- alpha = A^-1 y (rows of the symmetric A^-1, fixed order), zero beyond n; published by the barriers of the product below
        for (int j = tid; j < nk; j += PM_NT) {
            float s = 0.f;
            if (j < n) for (int k = 0; k < n; ++k) s = fmaf(Ai[(size_t)j * a.ns_ld + k], ys[k], s);
            al[j] = s;
        }
        float s1[2][4], s2[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) { s1[i][r] = 0.f; s2[i][r] = 0.f; }
        float dummy[2];
        auto opK = [&](const float* B) { return [=](int i, int k, float (&v)[4]) {
#pragma unroll
            for (int x = 0; x < 4; ++x) v[x] = B[(size_t)i * ld + k + x];
        }; };
        // ---- C = K A^-1, kept, and its two reductions (as k_predict_marginal)
        for (int p = 0; p < np; ++p) {
            const int j0 = p * PM_TM;
            pm_mm<false>(acc, nk, As, Bs, opK(Kb),
                [&](int j, int k, float (&v)[4]) {
                    if (j0 + j >= n) { v[0] = v[1] = v[2] = v[3] = 0.f; return; }
                    pm_ld4(Ai + (size_t)(j0 + j) * a.ns_ld, k, n, false, v);
                }, dummy, dummy);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ii = pm_row(i, r), jj = j0 + pm_col(j);
                        Cb[(size_t)ii * ld + jj] = acc[i][j][r];
                        if (jj < n) { s1[i][r] = fmaf(acc[i][j][r], ys[jj], s1[i][r]); s2[i][r] = fmaf(acc[i][j][r], Kb[(size_t)ii * ld + jj], s2[i][r]); }
                    }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x = s1[i][r], y = s2[i][r];
                x += dpp_f<DPP_XOR1>(x); x += dpp_f<DPP_XOR2>(x); x += dpp_f<DPP_HALF_MIRROR>(x); x += dpp_f<DPP_MIRROR>(x);
                y += dpp_f<DPP_XOR1>(y); y += dpp_f<DPP_XOR2>(y); y += dpp_f<DPP_HALF_MIRROR>(y); y += dpp_f<DPP_MIRROR>(y);
                if ((lane & 15) == 0) { red[wc][0][pm_row(i, r)] = x; red[wc][1][pm_row(i, r)] = y; }
            }
        __syncthreads();
        // ---- the coefficients of the tile's rows
        if (tid < PM_TM) {
            float am = 0.f, av = 0.f;
            if (tid < m) {
                const float mean = red[0][0][tid] + red[1][0][tid], vl = os - (red[0][1][tid] + red[1][1][tid]);
                gd_coef<float>(a, g, t, r0 + tid, mean, vl, am, av);
            }
            coef[0][tid] = am; coef[1][tid] = av;
        }
        __syncthreads();
        // ---- W over G: four adjacent lanes per row, columns c, c + 4, ...; their sums meet in a fixed order
        {
            const int i = tid >> 2, c = tid & 3;
            const float am = coef[0][i], av2 = 2.f * coef[1][i];
            float sw = 0.f;
            for (int j = c; j < nk; j += 4) {
                const size_t e = (size_t)i * ld + j;
                const float wij = Gb[e] * (am * al[j] - av2 * Cb[e]);
                Gb[e] = wij;
                sw += wij;
            }
            sw += dpp_f<DPP_XOR1>(sw); sw += dpp_f<DPP_XOR2>(sw);
            if (c == 0) coef[2][i] = sw;
        }
        __syncthreads();
        // ---- dZq = 2 il2 ( (sum_i W_i) (x - mu) - W (Z_s - mu) ), one [64, 64] block per chunk of d
        for (int c0 = 0; c0 < a.d; c0 += PM_TM) {
            pm_mm<false>(acc, nk, As, Bs, opK(Gb),
                [&](int j, int k, float (&v)[4]) {
                    const int col = c0 + j;
                    if (col >= a.d) { v[0] = v[1] = v[2] = v[3] = 0.f; return; }
                    const float cm = ARD ? 0.f : mu[col];   // (ARD: Zt_s is centred and scaled already)
#pragma unroll
                    for (int x = 0; x < 4; ++x) v[x] = k + x < n ? Zs[(size_t)(k + x) * d + col] - cm : 0.f;
                }, dummy, dummy);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ii = pm_row(i, r), col = c0 + pm_col(j);
                        if (ii < m && col < a.d) {
                            const size_t e = (size_t)(r0 + ii) * d + col;
                            float xc, out;
                            if constexpr (ARD) xc = ard_scaled_il(a.Zq[e], mu[col], il[col]); else xc = a.Zq[e] - mu[col];
                            out = 2.f * il2 * (coef[2][ii] * xc - acc[i][j][r]);
                            if constexpr (ARD) out *= il[col];
                            g.dZq[e] = (coef[0][ii] == 0.f && coef[1][ii] == 0.f) ? 0.f : out;
                        }
                    }
        }
        __syncthreads();   // coef / red / the row tiles are rewritten by the next tile
    }
}

// ---- the row kernel: grid (workgroups per task, T); workgroup (x, t) serves the rows lo + x, lo + x + gridDim.x, ... of task t
constexpr int PG_NT = 256;

// sum over the workgroup in a fixed order; every thread gets the total (two barriers)
__device__ __forceinline__ double pg_sum(double v, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// the LDS of a workgroup at leading dimension ld: five float arrays (float32 tasks) or four double arrays (flagged tasks)
__host__ __device__ inline size_t pg_row_lds(int ld, bool have64) {
    const size_t f32 = (size_t)5 * ld * sizeof(float), f64 = have64 ? (size_t)4 * ld * sizeof(double) : 0;
    return f32 > f64 ? f32 : f64;
}

template <bool ARD>
__global__ __launch_bounds__(PG_NT) void k_predict_grad_row(PgArgsOf<ARD> args) {
    const PmArgs& a = args.p;
    const PgArgs& g = args.g;
    extern __shared__ __attribute__((aligned(16))) double pg_row_mem[];
    __shared__ double red[PG_NT / 64];
    const int t = blockIdx.y, tid = threadIdx.x;
    const int kind = pm_kind_of(a, t);
    if (kind < 0 || !((g.row_kinds >> kind) & 1)) return;   // (uniform)
    const bool f64 = kind == 2;
    const int n = pm_ns(a, t), ld = a.ns_ld, d = a.d;
    if (f64 && n > R64_MAXN) return;   // (cannot happen: no float64 region beyond R64_MAXN points, so nothing is flagged there)
    int64_t lo, hi;
    pm_range(a, t, lo, hi);
    if (lo + blockIdx.x >= hi) return;
    const float* sc = a.scal + (size_t)t * NSCAL;
    const float osf = sc[S_OS], noisef = sc[S_NOISE], il2f = 1.f / (sc[S_LS] * sc[S_LS]);
    const double os = sc[S_OS], il2 = 1.0 / ((double)sc[S_LS] * (double)sc[S_LS]);
    const float* Zs = a.Zs + (size_t)t * ld * d;
    const float* ys = a.y_s + (size_t)t * ld;
    const float* mu = a.mean_s + (size_t)t * d;
    const float* el = nullptr;
    if constexpr (ARD) el = args.r.ell + (size_t)t * d;
    const float* Ai = a.Ainv + (size_t)t * ld * ld;
    const float* Dss = a.D2ss + (size_t)t * ld * ld;
    const double* A1 = f64 ? a.w64 + (size_t)t * a.w64_stride : nullptr;
    // float32 tasks: k, c, e (pm_solve_refined's scratch), alpha, G / W;  flagged: k, G / W, c, alpha
    float *kf = reinterpret_cast<float*>(pg_row_mem), *cf = kf + ld, *ef = cf + ld, *alf = ef + ld, *gf = alf + ld;
    double *kd = pg_row_mem, *gd = kd + ld, *cd = gd + ld, *ald = cd + ld;
    // ---- alpha, once per workgroup
    if (f64) {
        for (int j = tid; j < n; j += PG_NT) {
            double s = 0.0;
            for (int q = 0; q < n; ++q) s += (double)ys[q] * A1[(size_t)q * ld + j];
            ald[j] = s;
        }
    } else {
        for (int j = tid; j < n; j += PG_NT) kf[j] = ys[j];
        __syncthreads();
        pm_solve_refined(Ai, Dss, a.kind, osf, noisef, il2f, n, ld, kf, cf, ef);
        __syncthreads();
        for (int j = tid; j < n; j += PG_NT) alf[j] = cf[j];
    }
    __syncthreads();
    for (int64_t r = lo + blockIdx.x; r < hi; r += gridDim.x) {
        const float* zq = a.Zq + (size_t)r * d;
        // ---- the kernel row and its derivative from difference-form distances (flagged: pm64_kernel_row's arithmetic)
        for (int j = tid; j < n; j += PG_NT) {
            const float* zs = Zs + (size_t)j * d;
            double s = 0.0;
            if constexpr (ARD) {
                for (int c = 0; c < d; ++c) { const double e = (double)ard_scaled(zq[c], mu[c], el[c]) - (double)zs[c]; s += e * e; }
            } else {
                for (int c = 0; c < d; ++c) { const double e = (double)zq[c] - (double)zs[c]; s += e * e; }
            }
            if (f64) {
                double k0, k1, k2;
                kappa3_d(a.kind, s * il2, k0, k1, k2);
                kd[j] = os * k0; gd[j] = os * k1;
            } else {
                float k0, k1, k2;
                kappa3(a.kind, (float)(s * il2), k0, k1, k2);
                kf[j] = osf * k0; gf[j] = osf * k1;
            }
        }
        __syncthreads();
        // ---- c = k A^-1
        if (f64) {
            for (int j = tid; j < n; j += PG_NT) {
                double s = 0.0;
                for (int q = 0; q < n; ++q) s += kd[q] * A1[(size_t)q * ld + j];
                cd[j] = s;
            }
        } else {
            pm_solve_refined(Ai, Dss, a.kind, osf, noisef, il2f, n, ld, kf, cf, ef);
        }
        __syncthreads();
        double p1 = 0.0, p2 = 0.0;
        for (int j = tid; j < n; j += PG_NT) {
            const double cj = f64 ? cd[j] : (double)cf[j], kj = f64 ? kd[j] : (double)kf[j];
            p1 += cj * (double)ys[j]; p2 += cj * kj;
        }
        const double mean = pg_sum(p1, red), ck = pg_sum(p2, red);
        double am, av;
        gd_coef<double>(a, g, t, r, mean, os - ck, am, av);   // (uniform: every thread holds the same sums)
        // ---- W over G
        for (int j = tid; j < n; j += PG_NT) {
            if (f64) gd[j] = gd[j] * (am * ald[j] - 2.0 * av * cd[j]);
            else gf[j] = (float)((double)gf[j] * (am * (double)alf[j] - 2.0 * av * (double)cf[j]));
        }
        __syncthreads();
        // ---- dZq[r, c] = 2 il2 sum_i W_i (x_c - z_ic), in float64, rounded once
        const bool zero = am == 0.0 && av == 0.0;
        for (int c = tid; c < d; c += PG_NT) {
            double x, s = 0.0;
            if constexpr (ARD) x = (double)ard_scaled(zq[c], mu[c], el[c]); else x = (double)zq[c];
            for (int i = 0; i < n; ++i) s += (f64 ? gd[i] : (double)gf[i]) * (x - (double)Zs[(size_t)i * d + c]);
            s *= 2.0 * il2;
            if constexpr (ARD) s /= (double)el[c];
            g.dZq[(size_t)r * d + c] = zero ? 0.f : (float)s;
        }
        __syncthreads();   // the next row overwrites k and G
    }
}

}  // namespace adkf
