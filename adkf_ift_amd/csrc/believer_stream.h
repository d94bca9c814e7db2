// Kriging-believer batch selection over a shared pool (adkf_believer_pool): q sequential-greedy EI picks per task, each pick
// "believed" at its posterior mean (Ginsbourger, Le Riche and Carraro 2010).  The mean never changes; the latent variance of every
// pool row shrinks by a rank-one downdate per pick, and the incumbent moves to the believed value.  With p_0 .. p_(j-1) the picks of
// task t so far (x_p their pool rows), A = K_ss + noise I:
//     w_i      = A^-1 k(Z_s, x_(p_i))
//     c0(x, i) = k(x, x_(p_i)) - k(x, Z_s) . w_i                 posterior covariance of x and pick i
//     G G^T    = [c0(x_(p_i), l)] + noise I                      G lower triangular, one new row per pick
//     ell(x)   = G^-1 c0(x, .)                                   forward substitution, i ascending
//     v_j(x)   = v_0(x) - sum_(i<j) ell_i(x)^2                   score_j(x) = EI(m(x), v_j(x), best_j) (pm_ei / pm_log_ei)
// Per step j: the pool walks of prediction (plain, refined, float64 - pm_kind_of), then one workgroup per task (k_bv_step).  The
// launch boundaries order the steps; nothing is atomic, every sum has a fixed order, and nothing of size T x rows is kept.
//
//   the walk  is k_predict_marginal's tile itself (K row tile, C = K A^-1, the two reductions, REFINE's correction) with
//             BvEpilogue in the place of prediction's epilogue.  With c picks made, it adds F = K_tile W^T (pm_mm over the row tile,
//             W the picks' w rows, [q, ns]) and the kernel panel of the tile against the picks (pm_k_panel with the picks' stored
//             feature rows as its "support"); c0 = Kxp - F goes into pm_mm's two staging buffers, which are adjacent and free by then
//             (a [64, 65] panel in 2 * 64 * 34 floats), so the instance needs NO LDS beyond prediction's: its row tiles move to the
//             global slots at prediction's sizes (host_stream.h derives both from the same expression).  Thread i < 64 then runs the
//             substitution of row i against G (uniform loads), takes v_j and the score, and the shared tail (pm_tile_tail) offers the
//             scores to the walk's one-entry list; the exclusion test also scans the picks made so far (bv_excl).  At c = 0 none of
//             this runs and the row's score is prediction's, bit for bit.
//   float64   tasks (refine64.h) take k_bv_walk64, the float64 pool walk (pm64_pool_walk, predict_stream.h) with float64 w and G: lane
//             i forms c0(x, i), the substitution runs over the lanes (row i of G against the ell broadcast so far).
//   k_bv_step merges the chunks' pairs under pm_beats (pm_merge_task_lists, k_pool_topk's merge at width 1), writes sel_*, forms
//             k(Z_s, x_p) from the features in float64 (refine64.h's float64 kappa0, as the float64 walk), solves w = A^-1 k (float32
//             tasks: pm_solve_refined, k_ts_solve's product and ONE refinement step with A regenerated from D2ss; flagged tasks:
//             k_refine64's float64 A^-1), takes the pick's mean w . y and variance s - k . w - |ell|^2 from it, and stores the pick's
//             feature row, the new row of G (G[j, :j] = ell, G[j, j] = sqrt(v_j + noise)), the new incumbent and the pick count.  With
//             no eligible row it reports -1 / -inf and changes nothing, so every later step does the same.
//
// ARD batches (adkf_believer_pool_ard, ARD = true) run the same kernels on the scaled features x~ = (x - mu) / l of ard.h at unit
// lengthscale: the walk's tile is prediction's ARD tile (pool rows scaled while they are staged, a.Zs = Zt_s), and the pick panel is
// pm_k_panel<true>, which expects its "support" centred and scaled already - so k_bv_step<true> stores the pick's SCALED row in Xp,
// through the function the walk of that task's kind applies to the same pool row: ard_scaled_il, (x - mu) * il, for float32 tasks
// (pm_query_rows<true>); ard_scaled, k_ard_scale's (x - mu) / l in float32, for flagged ones (pm64_kernel_row<true>, k_bv_walk64<true>).
// A pool row and its stored copy are the same float32 numbers because both come out of one function (device_utils.h), not because two
// expressions were kept alike; only one kind of kernel reads a task's Xp, so one buffer serves both.  The scalars, D2ss and
// A^-1 are those of the unit-lengthscale pipeline (scal[S_LS] = softplus(RAW_ONE) = 1), so the solve, G and the state are unchanged.
//
// The c0 panel, the substitution of one row and the float64 downdate are functions (bv_c0_panel, bv_downdate, bv64_downdate) because
// adkf_gibbon_pool (gibbon_stream.h) downdates the same variance with the same state, k_bv_init and k_bv_step, under another score.
// The float64 c0 of a lane (bv64_c0) and the first parts of k_bv_step - the stored row, k(Z_s, x) and w = A^-1 k (bv_store_row,
// bv_kernel_col, bv_solve_w) - are functions because adkf_kg_pool and adkf_jes_pool (kg_stream.h, jes_stream.h) build the same state
// for a fixed reference set, one (entry, task) workgroup each: bv_ref_entry.  k_bv_step's body is a function too (bv_step), with
// what is believed about the pick as a parameter, because adkf_liar_pool (liar_stream.h) runs the same step with a supplied value;
// bv64_downdate shows each ell_i to a functor for the same entry's mean shift.
#pragma once
#include "thompson_stream.h"

namespace adkf {

constexpr int BV_LDC = PM_TM + 1;      // leading dimension of the c0 panel (a thread per row walks it: no bank conflicts)
static_assert(PM_TM * BV_LDC <= 2 * PM_TM * LD_MN, "the c0 panel lives in pm_mm's staging buffers");

struct BvArgs {
    int q, j;                           // picks per task; the step of this launch
    float* W; double* W64;              // [T, q, ns_ld]: w of pick i (float64 tasks: W64; null without a float64 region)
    float* Xp;                          // [T, q, d]: the picks' feature rows
    float* G; double* G64;              // [T, q, q] lower triangular
    float* best; int32_t* cnt;          // [T]: the incumbent and the picks made
    float* trace;                       // nullable [T, q, rows]
    int64_t* sel_idx; float *sel_val, *sel_mean, *sel_var;   // [T, q]; the last two nullable
};
struct BvEpilogue;
template <bool ARD>
using BvKargs = PmArgsOf<ARD, true, BvEpilogue>;   // p.Zq: the pool; s.k = 1, s.cand_* [T, chunks_max]; ARD: r, the query scaling

__device__ __forceinline__ bool bv_picked(const BvArgs& v, int t, int c, long long r) {
    for (int i = 0; i < c; ++i)
        if (v.sel_idx[(size_t)t * v.q + i] == r) return true;
    return false;
}
// what task t may not select with c picks made: its exclusion list and the picks
__device__ __forceinline__ auto bv_excl(const PmPool& s, const BvArgs& v, int t, int c) {
    return [&s, &v, t, c](long long r) { return pm_excluded(s, t, r) || bv_picked(v, t, c, r); };
}
__device__ __forceinline__ float bv_score(const PmArgs& a, const BvArgs& v, int t, float mean, float vl) {
    return a.log_ei ? pm_log_ei(mean, vl, v.best[t], a.maximize) : pm_ei(mean, vl, v.best[t], a.maximize);
}

// ---- with c > 0 picks made (uniform): F = K_tile W^T over the row tile, then the kernel panel against the picks; c0 = Kxp - F is left
// in pm_mm's staging buffers ([64, BV_LDC] from tl.As), behind a barrier.  All 256 threads.
template <bool ARD>
__device__ __forceinline__ void bv_c0_panel(const PmArgs& a, const BvArgs& v, const PmTile& tl, f32x4 (&acc)[2][2], int c) {
    const int t = tl.t, q = v.q;
    float* C0 = tl.As;
    const float* Wt = v.W + (size_t)t * q * a.ns_ld;
    const float* Kb = tl.Kb;
    const int ld = tl.ld, n = tl.n, ns_ld = a.ns_ld;
    float dummy[2];
    pm_mm<false>(acc, tl.nk, tl.As, tl.Bs,
        [=](int i, int k, float (&x)[4]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = Kb[(size_t)i * ld + k + e];
        },
        [=](int i, int k, float (&x)[4]) {
            if (i >= c) { x[0] = x[1] = x[2] = x[3] = 0.f; return; }
            pm_ld4(Wt + (size_t)i * ns_ld, k, n, false, x);
        }, dummy, dummy);
    f32x4 F[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) F[i][j] = acc[i][j];
    pm_k_panel<ARD>(a, v.Xp + (size_t)t * q * a.d, tl.mu, tl.il, tl.r0, tl.m, c, 0, tl.os, tl.il2, tl.As, tl.Bs, *tl.rowsq, acc,
                      C0, BV_LDC, [] {});
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) C0[pm_row(i, r) * BV_LDC + pm_col(j)] -= F[i][j][r];   // (this thread's own elements)
    __syncthreads();
}
// ell = G^-1 c0 of one row of the panel, in place, i ascending; returns |ell|^2, what the row's latent variance loses
__device__ __forceinline__ float bv_downdate(const BvArgs& v, int t, int c, float* e) {
    const int q = v.q;
    const float* G = v.G + (size_t)t * q * q;
    float ss = 0.f;
    for (int i = 0; i < c; ++i) {
        float s = e[i];
        for (int l = 0; l < i; ++l) s = fmaf(-G[i * q + l], e[l], s);
        s /= G[i * q + i];
        e[i] = s;
        ss = fmaf(s, s, ss);
    }
    return ss;
}

struct BvEpilogue {
    using Args = BvArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK& walk, f32x4 (&acc)[2][2]) {
        static_assert(POOL, "adkf_believer_pool(_ard): a shared pool");
        const PmArgs& a = args.p;
        const BvArgs& v = args.v;
        const int tid = threadIdx.x, t = tl.t, q = v.q;
        const int c = v.cnt[t];   // (uniform) picks made, at most the step
        float* C0 = tl.As;
        if (c > 0) bv_c0_panel<ARD>(a, v, tl, acc, c);
        float score = 0.f;
        if (tid < tl.m) {
            float vl = tl.var(tid);
            if (c > 0) vl -= bv_downdate(v, t, c, C0 + tid * BV_LDC);
            score = bv_score(a, v, t, tl.mean(tid), vl);
        }
        pm_tile_tail(args, tl, walk, score, v.trace, (size_t)t * q + v.j, 1, bv_excl(args.s, v, t, c));
    }
};

// lane i < c of a wave: c0(x, i) in float64 for the pool row zq (kernel row k) against the stored row i of Xp and its w (0 in the other lanes)
template <bool ARD>
__device__ __forceinline__ double bv64_c0(const PmArgs& a, const Pm64Task& tk, const float* zq, const double* k, const double* Wt, const float* Xp,
                                          int c, int lane) {
    const int n = tk.n, ld = tk.ld;
    double c0 = 0.0;
    if (lane < c) {
        const float* xp = Xp + (size_t)lane * a.d;
        double s = 0.0, f = 0.0;
        if constexpr (ARD) {   // the float32 feature of k_ard_scale against the stored one (k_bv_step<true>: ard_scaled, both)
            for (int e = 0; e < a.d; ++e) { const double df = (double)ard_scaled(zq[e], tk.mu[e], tk.el[e]) - (double)xp[e]; s += df * df; }
        } else {
            for (int e = 0; e < a.d; ++e) { const double df = (double)zq[e] - (double)xp[e]; s += df * df; }
        }
        for (int i = 0; i < n; ++i) f += k[i] * Wt[(size_t)lane * ld + i];
        c0 = tk.os * kappa0(a.kind, s * tk.il2) - f;
    }
    return c0;
}

// the float64 downdate of one pool row zq (kernel row k) with c > 0 picks made, over the lanes of a wave: lane i forms c0(x, i), the
// substitution runs over the lanes (row i of G against the ell broadcast so far); returns |ell|^2 to every lane.  each(i, ell_i)
// sees every entry as it is broadcast (adkf_liar_pool's mean shift, liar_stream.h).
template <bool ARD, class EACH>
__device__ __forceinline__ double bv64_downdate(const PmArgs& a, const Pm64Task& tk, const float* zq, const double* k, const double* Wt,
                                                const double* G, const float* Xp, int c, int q, int lane, EACH each) {
    const double c0 = bv64_c0<ARD>(a, tk, zq, k, Wt, Xp, c, lane);   // lane i: c0(x, i)
    double part = 0.0, ss = 0.0;   // lane i: sum_(l < i) G[i, l] ell_l so far
    for (int i = 0; i < c; ++i) {
        double e = lane == i ? (c0 - part) / G[(size_t)i * q + i] : 0.0;
        e = __shfl(e, i);
        if (lane > i && lane < c) part += G[(size_t)lane * q + i] * e;
        ss += e * e;
        each(i, e);
    }
    return ss;
}
template <bool ARD>
__device__ __forceinline__ double bv64_downdate(const PmArgs& a, const Pm64Task& tk, const float* zq, const double* k, const double* Wt,
                                                const double* G, const float* Xp, int c, int q, int lane) {
    return bv64_downdate<ARD>(a, tk, zq, k, Wt, G, Xp, c, q, lane, [](int, double) {});
}

// ---- flagged tasks: the float64 pool walk (pm64_pool_walk) with the downdate in float64
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_bv_walk64(BvKargs<ARD> args) {
    const PmArgs& a = args.p;
    const BvArgs& v = args.v;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = v.q;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const int c = v.cnt[t];
    const double* Wt = v.W64 + (size_t)t * q * tk.ld;
    const double* G = v.G64 + (size_t)t * q * q;
    const float* Xp = v.Xp + (size_t)t * q * a.d;
    pm64_pool_walk<ARD>(args, tk, kr[wv], 1, bv_excl(args.s, v, t, c), [&](int64_t r, const float* zq, const double* k, double s1, double s2) {
        double vl = tk.os - s2;
        if (c > 0) vl -= bv64_downdate<ARD>(a, tk, zq, k, Wt, G, Xp, c, q, lane);
        float score = 0.f;
        if (lane == 0) {
            score = bv_score(a, v, t, (float)s1, (float)vl);
            if (v.trace) v.trace[((size_t)t * q + v.j) * (size_t)a.rows + (size_t)r] = score;
        }
        return score;
    });
}

// the per-task state before step 0
__global__ __launch_bounds__(256) void k_bv_init(BvArgs v, const float* best_f, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < T) { v.cnt[t] = 0; v.best[t] = best_f[t]; }
}

// the sum of x over the workgroup's 256 threads in a fixed order, to every thread
__device__ __forceinline__ double bv_block_sum(double x, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = x;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// ---- the parts of k_bv_step that k_kg_refs (kg_stream.h) runs on a reference row: one workgroup of 256 threads each
// the pool row xp of task t into dst [d] - ARD: scaled by the function the walk of the task's kind applies (see the top of the file),
// published - and the row everything after reads: the stored copy (ARD) or xp itself
template <bool ARD, class ARGS>
__device__ __forceinline__ const float* bv_store_row(const ARGS& args, int t, bool f64, const float* xp, float* dst) {
    const PmArgs& a = args.p;
    const int tid = threadIdx.x, d = a.d;
    if constexpr (ARD) {   // the row as the walk of this task's kind scales it; everything below reads the stored copy
        const float *mu = a.mean_s + (size_t)t * d, *il = args.r.il + (size_t)t * d, *el = args.r.ell + (size_t)t * d;
        for (int e = tid; e < d; e += 256) dst[e] = f64 ? ard_scaled(xp[e], mu[e], el[e]) : ard_scaled_il(xp[e], mu[e], il[e]);
        __syncthreads();
        return dst;
    } else {
        for (int e = tid; e < d; e += 256) dst[e] = xp[e];
        return xp;
    }
}
// k(Z_s, x_p) from the features, in float64, into k64 (flagged tasks) or rs (rounded); published
__device__ __forceinline__ void bv_kernel_col(const PmArgs& a, const float* Zs, const float* xp, int n, double os, double il2, bool f64,
                                              double* k64, float* rs) {
    const int d = a.d;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float* zs = Zs + (size_t)i * d;
        double sq = 0.0;
        for (int e = 0; e < d; ++e) { const double df = (double)xp[e] - (double)zs[e]; sq += df * df; }
        const double kv = os * kappa0(a.kind, sq * il2);
        if (f64) k64[i] = kv; else rs[i] = (float)kv;
    }
    __syncthreads();
}
// w = A^-1 k, published: flagged tasks through k_refine64's float64 A^-1 (k in fb as doubles, w behind it at R64_MAXN, and in Wn64),
// float32 tasks through pm_solve_refined (k in fb, w in fb + TS_NS_MAX, and in Wn; the third array is used up)
__device__ __forceinline__ void bv_solve_w(const PmArgs& a, int t, int n, bool f64, float* fb, float* Wn, double* Wn64) {
    const int tid = threadIdx.x, ld = a.ns_ld;
    if (f64) {
        double *k64 = reinterpret_cast<double*>(fb), *w64 = k64 + R64_MAXN;
        const double* A1 = a.w64 + (size_t)t * a.w64_stride;
        for (int i = tid; i < n; i += 256) {
            double x = 0.0;
            for (int k = 0; k < n; ++k) x += A1[(size_t)k * ld + i] * k64[k];
            w64[i] = x; Wn64[i] = x;
        }
    } else {   // k_ts_solve's solve
        const float* sc = a.scal + (size_t)t * NSCAL;
        float *rs = fb, *vs = fb + TS_NS_MAX, *es = fb + 2 * TS_NS_MAX;
        pm_solve_refined(a.Ainv + (size_t)t * ld * ld, a.D2ss + (size_t)t * ld * ld, a.kind, sc[S_OS], sc[S_NOISE], 1.f / (sc[S_LS] * sc[S_LS]), n, ld,
                         rs, vs, es);
        for (int i = tid; i < n; i += 256) Wn[i] = vs[i];
    }
    __syncthreads();
}

// ---- one (entry, task) workgroup of a reference kernel (k_kg_refs, k_jes_refs): the pool row idx as a fixed "pick" of task t, with
// the caller's verdict ok (uniform) and the entry's slots Xj [d], Wj [ns_ld] and W64j [ns_ld] (null without a float64 region).
// A skipped entry gets zero rows - nothing of it is read but by the c0 panel, whose column is ignored - and the answer 0.  Otherwise
// the row goes into Xj (bv_store_row), k(Z_s, x) and w = A^-1 k into fb as bv_kernel_col and bv_solve_w leave them (float32 tasks:
// k in fb, w at fb + TS_NS_MAX; flagged: doubles, k in fb, w behind it at R64_MAXN), w into its slot, zero beyond n, and the entry's
// posterior mean w . y comes back, summed in float64 in a fixed order.  fb: 3 * TS_NS_MAX floats, 16-byte aligned; red: 256 doubles.
template <bool ARD, class ARGS>
__device__ __forceinline__ double bv_ref_entry(const ARGS& args, int t, bool ok, long long idx, float* Xj, float* Wj, double* W64j, float* fb, double* red) {
    const PmArgs& a = args.p;
    const int tid = threadIdx.x, ld = a.ns_ld, d = a.d;
    if (!ok) {
        for (int e = tid; e < d; e += 256) Xj[e] = 0.f;
        for (int i = tid; i < ld; i += 256) { Wj[i] = 0.f; if (W64j) W64j[i] = 0.0; }
        return 0.0;
    }
    const bool f64 = pm_kind_of(a, t) == 2;
    const int n = pm_ns(a, t);
    const float* sc = a.scal + (size_t)t * NSCAL;
    const double os = sc[S_OS], il2 = 1.0 / ((double)sc[S_LS] * (double)sc[S_LS]);
    const float* ys = a.y_s + (size_t)t * ld;
    const float* xp = bv_store_row<ARD>(args, t, f64, a.Zq + (size_t)idx * d, Xj);
    const float* vs = fb + TS_NS_MAX;
    const double* w64 = reinterpret_cast<double*>(fb) + R64_MAXN;
    bv_kernel_col(a, a.Zs + (size_t)t * ld * d, xp, n, os, il2, f64, reinterpret_cast<double*>(fb), fb);
    bv_solve_w(a, t, n, f64, fb, Wj, W64j);
    for (int i = n + tid; i < ld; i += 256) { Wj[i] = 0.f; if (W64j) W64j[i] = 0.0; }
    double pm = 0.0;
    for (int i = tid; i < n; i += 256) pm += (f64 ? w64[i] : (double)vs[i]) * (double)ys[i];
    return bv_block_sum(pm, red);
}

// What a greedy entry believes about a pick - the one part of the step its entries do not share.  The believer's and GIBBON's: the
// pick's posterior mean, which never moves.  adkf_liar_pool's (liar_stream.h) supplies the value and moves the mean.
//   none(o)                       no eligible row at output slot o (one thread)
//   pick(o, p, m0, ell, c, gd)    row p is pick c: m0 its mean from the support set, ell [c] = G^-1 c0(x_p, .), gd = G[c, c]; returns
//                                 the mean to report and the value believed, which moves the incumbent (one thread)
struct BvPick { float mean, believed; };
struct BvBelieveMean {
    __device__ __forceinline__ void none(size_t) const {}
    __device__ __forceinline__ BvPick pick(size_t, long long, double m0, const double*, int, double) const {
        const float mf = (float)m0;
        return {mf, mf};
    }
};

// ---- the end of step j: one workgroup per task (see the top of the file), on the believer's arguments v with the entry's rule
template <bool ARD, class ARGS, class BELIEVE>
__device__ __forceinline__ void bv_step(const ARGS& args, const BvArgs& v, const BELIEVE& believe) {
    const PmArgs& a = args.p;
    const PmPool& s = args.s;
    __shared__ __attribute__((aligned(16))) float fb[3 * TS_NS_MAX];
    __shared__ double red[256];
    __shared__ double c0s[PM_TOPK_MAX];
    __shared__ long long pick_s;
    __shared__ float val_s;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = v.q;
    const size_t o = (size_t)t * q + v.j;
    if (wv == 0) {   // the task's lists under the total order (skipped tasks, and every task when no walk ran, have none)
        float lv;
        long long li;
        pm_merge_task_lists(a, s, t, 1, lv, li);
        if (lane == 0) { pick_s = li; val_s = lv; }
    }
    __syncthreads();
    const long long p = pick_s;
    if (p < 0) {   // (uniform) no eligible row: the state stays as it is
        if (tid == 0) {
            v.sel_idx[o] = -1; v.sel_val[o] = -INFINITY;
            if (v.sel_mean) v.sel_mean[o] = 0.f;
            if (v.sel_var) v.sel_var[o] = 0.f;
            believe.none(o);
        }
        return;
    }
    const bool f64 = pm_kind_of(a, t) == 2;
    const int n = pm_ns(a, t), ld = a.ns_ld, d = a.d, c = v.cnt[t];
    const float* sc = a.scal + (size_t)t * NSCAL;
    const double os = sc[S_OS], noise = sc[S_NOISE], il2 = 1.0 / ((double)sc[S_LS] * (double)sc[S_LS]);
    const float* xp = a.Zq + (size_t)p * d;
    const float* Zs = a.Zs + (size_t)t * ld * d;
    const float* ys = a.y_s + (size_t)t * ld;
    float* Xt = v.Xp + (size_t)t * q * d;
    xp = bv_store_row<ARD>(args, t, f64, xp, Xt + (size_t)c * d);
    float *rs = fb, *vs = fb + TS_NS_MAX;   // float32 tasks: k, then w in vs (bv_solve_w)
    double *k64 = reinterpret_cast<double*>(fb), *w64 = k64 + R64_MAXN;   // float64 tasks (n <= R64_MAXN): k and w
    bv_kernel_col(a, Zs, xp, n, os, il2, f64, k64, rs);
    bv_solve_w(a, t, n, f64, fb, v.W + ((size_t)t * q + c) * ld, f64 ? v.W64 + ((size_t)t * q + c) * ld : nullptr);
    // ---- the pick's mean w . y and prior-step variance s - k . w
    double pm = 0.0, pk = 0.0;
    for (int i = tid; i < n; i += 256) {
        const double wi = f64 ? w64[i] : (double)vs[i], ki = f64 ? k64[i] : (double)rs[i];
        pm += wi * (double)ys[i];
        pk += wi * ki;
    }
    const double mean = bv_block_sum(pm, red), v0 = os - bv_block_sum(pk, red);
    // ---- c0(x_p, i) for the earlier picks: one wave per pick
    for (int i = wv; i < c; i += 4) {
        const float* xi = Xt + (size_t)i * d;
        double sq = 0.0, f = 0.0;
        for (int e = lane; e < d; e += 64) { const double df = (double)xp[e] - (double)xi[e]; sq += df * df; }
        for (int k = lane; k < n; k += 64)
            f += f64 ? k64[k] * v.W64[((size_t)t * q + i) * ld + k] : (double)rs[k] * (double)v.W[((size_t)t * q + i) * ld + k];
        for (int x = 32; x > 0; x >>= 1) { sq += __shfl_xor(sq, x); f += __shfl_xor(f, x); }
        if (lane == 0) c0s[i] = os * kappa0(a.kind, sq * il2) - f;
    }
    __syncthreads();
    if (tid == 0) {   // the new row of G, the outputs and the state
        double ss = 0.0;
        for (int i = 0; i < c; ++i) {
            double x = c0s[i];
            for (int l = 0; l < i; ++l) x -= (f64 ? v.G64[((size_t)t * q + i) * q + l] : (double)v.G[((size_t)t * q + i) * q + l]) * c0s[l];
            x /= f64 ? v.G64[((size_t)t * q + i) * q + i] : (double)v.G[((size_t)t * q + i) * q + i];
            c0s[i] = x;
            ss += x * x;
        }
        const double vj = v0 - ss, gd = sqrt(fmax(vj + noise, 1e-30));
        for (int i = 0; i <= c; ++i) {
            const double g = i < c ? c0s[i] : gd;
            if (f64) v.G64[((size_t)t * q + c) * q + i] = g; else v.G[((size_t)t * q + c) * q + i] = (float)g;
        }
        const BvPick b = believe.pick(o, p, mean, c0s, c, gd);
        v.sel_idx[o] = p; v.sel_val[o] = val_s;
        if (v.sel_mean) v.sel_mean[o] = b.mean;
        if (v.sel_var) v.sel_var[o] = (float)vj;
        v.best[t] = a.maximize ? fmaxf(v.best[t], b.believed) : fminf(v.best[t], b.believed);
        v.cnt[t] = c + 1;
    }
}
template <bool ARD>
__global__ __launch_bounds__(256) void k_bv_step(BvKargs<ARD> args) {
    bv_step<ARD>(args, args.v, BvBelieveMean{});
}

}  // namespace adkf
