// Thompson sampling over a shared pool (adkf_thompson_pool): S pathwise posterior draws per task (Matheron's rule on a
// random-Fourier-feature prior draw), each reduced on the fly to its best eligible pool row.  One pass over the pool, work per
// (task, 64-row pool tile), a scratch that does not depend on the number of rows.
//
// With (noise, s, l) the task's hyper-parameters, mu its support column mean, (omega [m, d], phase [m]) the caller's basis at unit
// lengthscale, w [T, S, m] and eps [T, S, ns] the caller's standard normal draws, sample q of task t is
//     phi_j(x) = sqrt(2 s / m) cos(omega_j . (x - mu) / l + phase_j)         g(x) = sum_j w[t, q, j] phi_j(x)
//     r_i = y_i - g(z_i) - sqrt(noise) eps[t, q, i]                           v = A^-1 r
//     f(x) = g(x) + sum_i k(x, z_i) v_i
// Four phases, ordered by launch boundaries (no atomics anywhere; every sum has a fixed order, so the result is reproducible to
// the bit and a task's numbers do not depend on the grid or on the other tasks of the batch):
//   k_ts_resid   per (task, support row): the m features of the row (one per thread, the feature row of omega streamed), then
//                g for the S samples (one wave per sample, butterfly sum) and r into V [T, S, ns];
//   k_ts_solve   per (task, sample): v = A^-1 r, then ONE refinement step v += A^-1 (r - A v) with A regenerated from D2ss (as
//                ProbCres does), in place in V (pm_solve_refined).  That step is why this call has no plain / refined distinction
//                (pm_kind_of);
//   k_ts_stream  per (task, pool tile), a persistent grid placed over tasks and tiles by the pool walk of predict_stream.h
//                (PmPoolWalk, over the plain and the refined tasks at once): per 64-feature chunk P = (X - mu) Omega^T on the
//                FP32 MFMA (pm_mm with pm_query_rows, the operand staging of the distance product), sqrt(2 s / m)
//                cos(P / l + phase) on the vector ALU into an LDS panel, F += panel W^T on the MFMA; then per 64-column support
//                panel the K panel of prediction (pm_k_panel: centred D^2 with the norms summed while staging, then kappa)
//                and F += K_panel V_panel^T.  Only K v is needed, not K A^-1: no [64, ns] row tile is kept, so any ns runs
//                through this one instance with 53 KB of static LDS.  The X Omega^T product is computed per task (NOT shared
//                across tasks): the centred form keeps the argument of the cosine at the size of (x - mu) / l.  Epilogue: the
//                [64, S] tile goes through LDS, optionally to `paths`, and lane q of the first wave keeps sample q's best
//                (score, row) of the walk under the total order of pm_beats, with the exclusion test of pm_excluded; at the
//                end of the walk one pair per (task, chunk, sample) goes to scratch with ordinary stores;
//   k_ts_merge   one wave per task: lane q reduces the chunks' pairs of sample q under the same order.
// Tasks flagged for the float64 path (refine64.h: their K v cancels beyond float32) take the <true> instances of the first two
// kernels - the features and r in float64, v from k_refine64's float64 A^-1 - and k_ts_stream64 (one wave per pool row; the task
// preamble, the kernel row and the end of the walk are k_predict_marginal64's: pm64_task, pm64_kernel_row, pm64_finish_walk) instead
// of k_ts_stream.  The cosine there is cosf of the argument reduced to [-pi, pi] in float64.
//
// ARD batches (adkf_thompson_pool_ard, ARD = true) are the same call on the scaled features x~ = (x - mu) / l of ard.h at unit
// lengthscale, with the one basis (omega, phase) every task shares: the support rows are ard.h's Zt_s, centred and scaled already,
// so k_ts_resid takes omega_j . z~_i as it stands; the pool rows are scaled while they are staged ((x - mu) * il, the il = 1 / l of
// k_pm_ard_il, as ARD streaming prediction does), for the feature product and the K panel alike, and the feature epilogue has
// no lengthscale left to apply.  k_ts_stream64<true> scales with k_ard_scale's function (ard_scaled: (x - mu) / l in float32) before
// promoting to float64 (the rule of k_predict_marginal64<true>).  k_ts_solve and k_ts_merge are the isotropic instances: the scaled batch's
// scalars and D2ss are those of the unit-lengthscale pipeline that built A^-1 (scal[S_LS] = softplus(RAW_ONE) = 1, ard.h).
//
// Shared with qei_stream.h (adkf_qei_pool): k_ts_resid, k_ts_solve and the tile itself (ts_tile, with NB sample blocks of 64; k_ts_stream is
// its NB = 1 instance, bit for bit what it was before the tile was a function).
// Shared with believer_stream.h: pm_solve_refined, the float32 solve with its refinement step (k_ts_solve<false> copies v to V, k_bv_step
// to W and goes on with it).
#pragma once
#include <type_traits>

#include "predict_stream.h"

namespace adkf {

constexpr int TS_LDP = PM_TM + 4;      // leading dimension of the two LDS panels of k_ts_stream
constexpr int TS_M_MAX = 4096;         // ADKF_TS_FEATURES_MAX
constexpr int TS_S_MAX = 64;           // ADKF_TS_SAMPLES_MAX: one sample per lane
constexpr int TS_NS_MAX = 4096;        // the largest support set of the library

struct TsArgs {
    PmArgs p;                           // Zq: the pool X; q_off, best_f, mean / var / ei, the slots unused
    PmPool s;                           // k = S; cand_* [T, chunks_max, S]; top_* = sel_idx / sel_val [T, S]; grid[0], grid[2]
    const float *omega, *phase, *w, *eps;   // [m, d], [m], [T, S, m], [T, S, ns_ld]
    int m, S, vec_om;                   // vec_om: 16-byte loads of the rows of omega are legal
    float* V;                           // [T, S, ns_ld]: r, then v (float32 tasks)
    double* V64;                        // the same for flagged tasks (null without a float64 region)
    float* paths;                       // nullable [T, S, rows]
};
// what a kernel receives: the ARD instances carry the query scaling as well (PmArgs::Zs is Zt_s, PmArgs::mean_s is mu); the
// isotropic instances' arguments are TsArgs itself
struct TsArgsArd : TsArgs { PmArd r; };
template <bool ARD>
using TsArgsOf = std::conditional_t<ARD, TsArgsArd, TsArgs>;

// does the float32 (F64 = false: plain and refined tasks alike) or the float64 (true) instance own task t
constexpr int TS_KINDS32 = 3;
template <bool F64>
__device__ __forceinline__ bool ts_mine(const PmArgs& a, int t) { return F64 ? pm_kind_of(a, t) == 2 : pm_owns(a, t, TS_KINDS32); }

__device__ __forceinline__ float ts_cos(float x) { return cosf(x); }
__device__ __forceinline__ double ts_cos(double x) {   // reduced in float64, evaluated in float32
    x -= 6.283185307179586 * rint(x * 0.15915494309189535);
    return (double)cosf((float)x);
}

// ---- r = y - g(Z_s) - sqrt(noise) eps, per (task, support row): grid (ns_ld, T)
template <bool F64, bool ARD = false>
__global__ __launch_bounds__(256) void k_ts_resid(TsArgs args) {
    using R = std::conditional_t<F64, double, float>;
    const PmArgs& a = args.p;
    __shared__ R cs[TS_M_MAX];
    const int t = blockIdx.y, i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (!ts_mine<F64>(a, t)) return;   // (uniform)
    if (i >= pm_ns(a, t)) return;
    const float* sc = a.scal + (size_t)t * NSCAL;
    const R amp = sqrt((R)2 * (R)sc[S_OS] / (R)args.m), sigma = sqrt((R)sc[S_NOISE]);
    const float* z = a.Zs + ((size_t)t * a.ns_ld + i) * a.d;   // ARD: a row of Zt_s, centred and scaled already
    for (int j = tid; j < args.m; j += 256) {
        const float* om = args.omega + (size_t)j * a.d;
        R s = 0;
        if constexpr (ARD) {
            for (int c = 0; c < a.d; ++c) {
                if constexpr (F64) s = fma((double)om[c], (double)z[c], s);
                else s = fmaf(om[c], z[c], s);
            }
            cs[j] = amp * ts_cos(s + (R)args.phase[j]);
        } else {
            const R il = (R)1 / (R)sc[S_LS];
            const float* mu = a.mean_s + (size_t)t * a.d;
            for (int c = 0; c < a.d; ++c) {
                if constexpr (F64) s = fma((double)om[c], (double)z[c] - (double)mu[c], s);
                else s = fmaf(om[c], z[c] - mu[c], s);
            }
            cs[j] = amp * ts_cos(s * il + (R)args.phase[j]);
        }
    }
    __syncthreads();
    for (int q = wv; q < args.S; q += 4) {
        const float* wq = args.w + ((size_t)t * args.S + q) * args.m;
        R g = 0;
        for (int j = lane; j < args.m; j += 64) g += (R)wq[j] * cs[j];
        for (int o = 32; o > 0; o >>= 1) g += __shfl_xor(g, o);
        if (lane == 0) {
            const size_t e = ((size_t)t * args.S + q) * a.ns_ld + i;
            const R r = (R)a.y_s[(size_t)t * a.ns_ld + i] - g - sigma * (R)args.eps[e];
            if constexpr (F64) args.V64[e] = r; else args.V[e] = r;
        }
    }
}

// One workgroup of 256 threads, float32: v = A^-1 r, then ONE refinement step v += A^-1 (r - A v) with A = os kappa(D2ss il2) + noise I
// regenerated from Dss (as ProbCres does).  Ai: the symmetric A^-1 (column i is row i); rs, vs, es: LDS arrays of n floats of the
// caller, r in rs (published), v left in vs - entry i by thread i % 256, no barrier after it - and es used up.
__device__ __forceinline__ void pm_solve_refined(const float* Ai, const float* Dss, int kind, float os, float noise, float il2, int n, int ld,
                                                 const float* rs, float* vs, float* es) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += 256) {
        float s = 0.f;
        for (int k = 0; k < n; ++k) s = fmaf(Ai[(size_t)k * ld + i], rs[k], s);
        vs[i] = s;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        float s = 0.f;
        for (int k = 0; k < n; ++k) s = fmaf(os * kappa0(kind, Dss[(size_t)k * ld + i] * il2) + (k == i ? noise : 0.f), vs[k], s);
        es[i] = rs[i] - s;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        float s = 0.f;
        for (int k = 0; k < n; ++k) s = fmaf(Ai[(size_t)k * ld + i], es[k], s);
        vs[i] += s;
    }
}

// ---- v = A^-1 r (+ one refinement step in float32), per (task, sample), in place: grid (S, T).  Serves ARD batches unchanged: their
// scalars, D2ss and A^-1 are those of the scaled batch at unit lengthscale (scal[S_LS] = 1)
template <bool F64>
__global__ __launch_bounds__(256) void k_ts_solve(TsArgs args) {
    const PmArgs& a = args.p;
    const int t = blockIdx.y, q = blockIdx.x, tid = threadIdx.x;
    if (!ts_mine<F64>(a, t)) return;   // (uniform)
    const int n = pm_ns(a, t), ld = a.ns_ld;
    const size_t base = ((size_t)t * args.S + q) * ld;
    if constexpr (F64) {
        __shared__ double rs[R64_MAXN];
        if (n > R64_MAXN) return;
        const double* A1 = a.w64 + (size_t)t * a.w64_stride;   // float64 A^-1 [ld, ld] (symmetric)
        for (int i = tid; i < n; i += 256) rs[i] = args.V64[base + i];
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += A1[(size_t)k * ld + i] * rs[k];
            args.V64[base + i] = s;
        }
    } else {
        __shared__ float rs[TS_NS_MAX], vs[TS_NS_MAX], es[TS_NS_MAX];
        const float* sc = a.scal + (size_t)t * NSCAL;
        for (int i = tid; i < n; i += 256) rs[i] = args.V[base + i];
        __syncthreads();
        pm_solve_refined(a.Ainv + (size_t)t * ld * ld, a.D2ss + (size_t)t * ld * ld, a.kind, sc[S_OS], sc[S_NOISE], 1.f / (sc[S_LS] * sc[S_LS]), n, ld,
                         rs, vs, es);
        for (int i = tid; i < n; i += 256) args.V[base + i] = vs[i];
    }
}

// F (this wave's 32 x 32 quarter of the [64 rows, 64 samples] tile) += A B^T for two LDS panels [64, 64] (leading dimension
// TS_LDP, K-contiguous).  Column blocks at or beyond S hold zeros and are skipped (wave-uniform).
__device__ __forceinline__ void ts_mm(f32x4 (&F)[2][2], const float* A, const float* B, int S) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1, fi = lane & 15, fk = lane >> 4;
#pragma unroll
    for (int s = 0; s < PM_TM / 4; ++s) {
        float af[2], bf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = A[(wr * 32 + i * 16 + fi) * TS_LDP + 4 * s + fk];
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = B[(wc * 32 + j * 16 + fi) * TS_LDP + 4 * s + fk];
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (wc * 32 + j * 16 < S) {
#pragma unroll
                for (int i = 0; i < 2; ++i) F[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], F[i][j], 0, 0, 0);
            }
    }
}

// B panel: Bp[s][k] = src[(t S + s) ld + k0 + k] for s < S and k0 + k < k_end, else 0
__device__ __forceinline__ void ts_stage(float* Bp, const float* src, size_t ld, int S, int k0, int k_end) {
    for (int e = threadIdx.x; e < PM_TM * PM_TM; e += PM_NT) {
        const int s = e >> 6, k = e & 63;
        Bp[s * TS_LDP + k] = (s < S && k0 + k < k_end) ? src[(size_t)s * ld + k0 + k] : 0.f;
    }
}

// ---- the [64 rows, 64 NB samples] tile of draws of task t at the pool rows r0 .. r0 + mr, for k_ts_stream (NB = 1) and k_qei_stream
// (qei_stream.h; NB sample blocks of 64): F[bk] is this wave's 32 x 32 quarter of block bk, samples 64 bk .. 64 bk + 63.  The feature
// product, the cosine panel and the K panel are computed once per feature chunk / support panel; per block only the B panel (W, then
// V) is staged and multiplied.  What a sample gets does not depend on S, NB or its block: block bk, column s is the tile of NB = 1 on
// the draws of sample 64 bk + s alone, bit for bit.  ril (ARD): the task's 1 / l.  All 256 threads; the LDS arrays are the caller's
// (As, Bs: pm_mm's staging buffers; Pp, Bp: [64, TS_LDP] panels), free when it returns (behind a barrier).  The tile comes back in Fout.
template <bool ARD, int NB>
__device__ __forceinline__ void ts_tile(const TsArgs& args, const float* ril, int t, int64_t r0, int mr, float* As, float* Bs, float* Pp, float* Bp,
                                        float (&rowsq)[2][PM_TM], f32x4 (&Fout)[NB][2][2]) {
    const PmArgs& a = args.p;
    const int S = args.S;
    const int64_t d = a.d;
    const int n = pm_ns(a, t);
    const float* sc = a.scal + (size_t)t * NSCAL;
    const float os = sc[S_OS], il2 = 1.f / (sc[S_LS] * sc[S_LS]), amp = sqrtf(2.f * os / (float)args.m);
    [[maybe_unused]] const float il = 1.f / sc[S_LS];   // (isotropic: the scaling of the cosine's argument)
    const float* Zs = a.Zs + (size_t)t * a.ns_ld * d;
    const float* mu = a.mean_s + (size_t)t * d;
    const int np = (n + PM_TM - 1) / PM_TM;
    // the accumulators are locals, handed over once at the end: accumulated through the reference, the tile is moved between the
    // accumulator and the vector registers around every product
    f32x4 acc[2][2], F[NB][2][2];
#pragma unroll
    for (int bk = 0; bk < NB; ++bk)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) F[bk][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // the centred (ARD: and scaled) pool rows of the tile, for the feature part (by reference, once per tile: the functor
    // itself held across the feature loop costs 22 VGPRs)
    auto fx = [&](int i, int k, float (&v)[4]) { pm_query_rows<ARD>(a, mu, ril, r0, mr)(i, k, v); };
    float dummy[2];
    // ---- feature part: F = sqrt(2 s / m) cos((X - mu) Omega^T / l + phase) W^T (ARD: X~ Omega^T + phase)
    for (int j0 = 0; j0 < args.m; j0 += PM_TM) {
        pm_mm<false>(acc, a.d, As, Bs, fx,
            [&](int j, int k, float (&v)[4]) { pm_ld4(args.omega + (size_t)(j0 + j) * d, k, a.d, args.vec_om, v); }, dummy, dummy);
        ts_stage(Bp, args.w + (size_t)t * S * args.m, args.m, S, j0, args.m);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int jj = pm_col(j);
            const float ph = args.phase[j0 + jj];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ii = pm_row(i, r);
                    float arg;
                    if constexpr (ARD) arg = acc[i][j][r] + ph;
                    else arg = fmaf(acc[i][j][r], il, ph);
                    Pp[ii * TS_LDP + jj] = ii < mr ? amp * ts_cos(arg) : 0.f;
                }
        }
        __syncthreads();
        ts_mm(F[0], Pp, Bp, S);
        __syncthreads();
#pragma unroll
        for (int bk = 1; bk < NB; ++bk)
            if (bk * TS_S_MAX < S) {   // (uniform) the same cosine panel against the next block of W
                ts_stage(Bp, args.w + ((size_t)t * S + bk * TS_S_MAX) * args.m, args.m, S - bk * TS_S_MAX, j0, args.m);
                __syncthreads();
                ts_mm(F[bk], Pp, Bp, S - bk * TS_S_MAX);
                __syncthreads();
            }
    }
    // ---- update part: F += K V^T; the V panel is staged while the norms of the K panel are on their way
    for (int p = 0; p < np; ++p) {
        const int j0 = p * PM_TM;
        pm_k_panel<ARD>(a, Zs, mu, ril, r0, mr, n, j0, os, il2, As, Bs, rowsq, acc, Pp, TS_LDP,
                          [&] { ts_stage(Bp, args.V + (size_t)t * S * a.ns_ld, a.ns_ld, S, j0, n); });
        ts_mm(F[0], Pp, Bp, S);
        __syncthreads();
#pragma unroll
        for (int bk = 1; bk < NB; ++bk)
            if (bk * TS_S_MAX < S) {   // (uniform) the same K panel against the next block of V
                ts_stage(Bp, args.V + ((size_t)t * S + bk * TS_S_MAX) * a.ns_ld, a.ns_ld, S - bk * TS_S_MAX, j0, n);
                __syncthreads();
                ts_mm(F[bk], Pp, Bp, S - bk * TS_S_MAX);
                __syncthreads();
            }
    }
#pragma unroll
    for (int bk = 0; bk < NB; ++bk)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) Fout[bk][i][j] = F[bk][i][j];
}
// one block of the tile as [sample][row] into an LDS panel (the caller publishes it)
__device__ __forceinline__ void ts_tile_to_lds(float* Pp, const f32x4 (&F)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) Pp[pm_col(j) * TS_LDP + pm_row(i, r)] = F[i][j][r];
}

template <bool ARD = false>
__global__ __launch_bounds__(PM_NT) void k_ts_stream(TsArgsOf<ARD> args) {
    const PmArgs& a = args.p;
    __shared__ float As[PM_TM * LD_MN], Bs[PM_TM * LD_MN];
    __shared__ float Pp[PM_TM * TS_LDP], Bp[PM_TM * TS_LDP];   // the A panel (features or K) and the B panel (W or V)
    __shared__ float rowsq[2][PM_TM];
    const int tid = threadIdx.x, wv = tid >> 6;
    const int S = args.S;
    PmPoolWalk<TS_KINDS32> walk;   // first wave, lane q: (walk.lv, walk.li) is the best (score, row) of sample q in this walk
    if (!walk.start(a, args.s)) return;
    for (;;) {
        int t;
        int64_t r0;
        if (!walk.next(a, args.s, S, t, r0)) return;
        const int mr = (int)(a.rows - r0 < PM_TM ? a.rows - r0 : PM_TM);
        const float* ril = nullptr;                         // ARD: 1 / l per dimension, applied while the pool rows are staged
        if constexpr (ARD) ril = args.r.il + (size_t)t * a.d;
        f32x4 F[1][2][2];
        ts_tile<ARD, 1>(args, ril, t, r0, mr, As, Bs, Pp, Bp, rowsq, F);
        // ---- epilogue: the tile as [sample][row] through LDS
        ts_tile_to_lds(Pp, F[0]);
        __syncthreads();
        if (args.paths)
            for (int e = tid; e < S * PM_TM; e += PM_NT) {
                const int q = e >> 6, r = e & 63;
                if (r < mr) args.paths[((size_t)t * S + q) * (size_t)a.rows + (size_t)(r0 + r)] = Pp[q * TS_LDP + r];
            }
        if (wv == 0 && tid < S)
            for (int r = 0; r < mr; ++r) {
                const float f = Pp[tid * TS_LDP + r], s = a.maximize ? f : -f;
                const long long row = r0 + r;
                if (s == s && pm_beats(s, row, walk.lv, walk.li) && !pm_excluded(args.s, t, row)) { walk.lv = s; walk.li = row; }
            }
        __syncthreads();   // the panels are rewritten by the next tile
    }
}

// ---- flagged tasks: one wave per pool row in float64, grid (chunks, T); workgroup (c, t) walks the rows c * 4 + wave, stride
// chunks * 4; lane q carries sample q
template <bool ARD = false>
__global__ __launch_bounds__(PM64_NT) void k_ts_stream64(TsArgsOf<ARD> args) {
    const PmArgs& a = args.p;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, S = args.S, m = args.m;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const int n = tk.n, ld = tk.ld;
    [[maybe_unused]] const double il = 1.0 / tk.ls, il2 = il * il, amp = sqrt(2.0 * tk.os / (double)m);   // (il2 not Pm64Task's 1 / ls^2: this kernel's bits)
    const int ql = lane < S ? lane : S - 1;   // (lanes beyond S compute sample S - 1 again and store nothing)
    const float* wq = args.w + ((size_t)t * S + ql) * m;
    const double* vq = args.V64 + ((size_t)t * S + ql) * ld;
    double* k = kr[wv];
    float lv = -INFINITY;
    long long li = -1;
    for (int64_t r = (int64_t)blockIdx.x * PM64_WAVES + wv; r < a.rows; r += (int64_t)gridDim.x * PM64_WAVES) {
        const float* zq = a.Zq + (size_t)r * a.d;
        pm64_kernel_row<ARD>(a, tk, zq, il2, k);
        double f = 0.0;
        for (int j0 = 0; j0 < m; j0 += 64) {   // (m is a multiple of 64) one feature per lane, then every lane adds its sample's 64 terms
            const float* om = args.omega + (size_t)(j0 + lane) * a.d;
            double s = 0.0;
            double cv;
            if constexpr (ARD) {   // the float32 feature of k_ard_scale (ard_scaled), promoted as pm64_kernel_row<true> promotes it
                for (int c = 0; c < a.d; ++c) s = fma((double)om[c], (double)ard_scaled(zq[c], tk.mu[c], tk.el[c]), s);
                cv = amp * ts_cos(s + (double)args.phase[j0 + lane]);
            } else {
                for (int c = 0; c < a.d; ++c) s = fma((double)om[c], (double)zq[c] - (double)tk.mu[c], s);
                cv = amp * ts_cos(s * il + (double)args.phase[j0 + lane]);
            }
            for (int jj = 0; jj < 64; ++jj) f = fma((double)wq[j0 + jj], __shfl(cv, jj), f);
        }
        double u = 0.0;
        for (int j = 0; j < n; ++j) u = fma(k[j], vq[j], u);
        f += u;
        if (lane < S) {
            const float ff = (float)f, s = a.maximize ? ff : -ff;
            if (args.paths) args.paths[((size_t)t * S + lane) * (size_t)a.rows + (size_t)r] = ff;
            if (s == s && pm_beats(s, (long long)r, lv, li) && !pm_excluded(args.s, t, (long long)r)) { lv = s; li = r; }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    pm64_finish_walk(args.s, t, S, lv, li, [&](float v, long long i) { if (i >= 0 && pm_beats(v, i, lv, li)) { lv = v; li = i; } });
}

// ---- one wave per task: lane q reduces the pairs of sample q over the task's chunks (skipped tasks, and every task when no
// walk ran: -1 / -inf)
__global__ __launch_bounds__(64) void k_ts_merge(TsArgs args) {
    const PmArgs& a = args.p;
    const int t = blockIdx.x, lane = threadIdx.x, S = args.S;
    const int C = pm_task_chunks(a, args.s, t, false);
    if (lane >= S) return;
    float lv = -INFINITY;
    long long li = -1;
    for (int c = 0; c < C; ++c) {
        const size_t e = ((size_t)t * args.s.chunks_max + c) * S + lane;
        const long long r = args.s.cand_idx[e];
        const float v = args.s.cand_val[e];
        if (r >= 0 && pm_beats(v, r, lv, li)) { lv = v; li = r; }
    }
    args.s.top_idx[(size_t)t * S + lane] = li;
    args.s.top_val[(size_t)t * S + lane] = li >= 0 ? lv : -INFINITY;
}

}  // namespace adkf
