// Target-variance batch selection over a shared pool (adkf_ipv_pool; Cohn 1996, "ALC"; Gramacy and Apley 2015; BoTorch's
// qNegIntegratedPosteriorVariance; Huebotter et al. 2024, "VTL"): q sequential-greedy picks per task, each the pool row whose noisy
// observation lowers the weighted posterior variance at the task's TARGET rows r_1 .. r_M (pool rows tgt_idx[t, .], weights wt_m) the
// most.  The posterior variance of a GP does not depend on the labels, so the whole batch is chosen before anything is measured.
// With p_0 .. p_(j-1) the picks of task t so far, A = K_ss + noise I, an ENTRY e a target or a pick and w_e = A^-1 k(Z_s, x_e):
//     c0(x, e)     = k(x, x_e) - k(x, Z_s) . w_e
//     G G^T        = [c0(x_(p_i), p_l)] + noise I                 the believer's G (believer_stream.h), one new row per pick
//     ell(x)       = G^-1 c0(x, picks)                            forward substitution, i ascending (bv_downdate)
//     v_j(x)       = v_0(x) - sum_(i<j) ell_i(x)^2
//     cov_j(x,r_m) = c0(x, r_m) - sum_(i<j) ell_i(x) ell_i(r_m)   ell(r_m): the state Lr [T, q, M], one new row per pick
//     score_j(x)   = sum_m wt_m cov_j(x, r_m)^2 / (max(v_j(x), 1e-12) + noise)
//     tvar_j       = sum_m wt_m v_j(r_m),   v_j(r_m) = v_0(r_m) - sum_(i<j) ell_i(r_m)^2
// score_j(x) is what one noisy observation at x takes off tvar_j, so tvar_j - tvar_(j+1) = score_j(p_j).  A target entry is skipped
// if it lies outside [0, rows), repeats the index of an earlier entry of the list (by index alone, as adkf_kg_pool), or has a weight
// that is <= 0 or NaN.  Targets are eligible like any other row: observing a target is the best single pick, and a caller who cannot
// measure the targets lists them in the exclusions.
//
// One entry list per task, targets first (0 .. M), picks after (M .. M + j): both kinds share W [T, M + q, ns_ld], Xp [T, M + q, d]
// and the float64 twin of W, so ONE bv_c0_panel call with M + j columns gives the tile's covariances with everything at once.
// M + q <= 64 is the capacity of that panel ([64, BV_LDC] in pm_mm's staging buffers); a two-panel form is not built.
//
//   k_ipv_refs grid (M, T), before the walks: k_kg_refs' shape on bv_ref_entry, with the weight test; the target's row and w into its
//              entry slot, its effective weight (0: skipped) and v_0(r_m) = s - k . w (float64 sum, fixed order) into the state.
//   k_ipv_init a thread per task: the pick count 0, the number of valid targets and tvar_0 (by ascending m).
//   the walk   is k_predict_marginal's tile with IpvEpilogue, in all three kinds and ARD or not: (1) the panel; (2) thread i < 64:
//              the substitution of row i against G over the pick columns, in place, and the row's denominator max(v_j, 1e-12) +
//              noise into the panel's pad column; (3) ALL 256 THREADS, thread tid the row tid & 63 and the targets tid >> 6, + 4,
//              ...: cov_j(x, r_m) by ascending pick (one fma each, Lr read uniformly per wave) and its weighted square added by
//              ascending m; the four partial sums of a row meet where the panel was and are added in the order 0, 1, 2, 3
//              (pm_sum4).  A thread per row, as the believer has it, would leave three waves idle over j M multiply-adds a row -
//              up to 1024 - where the believer has j; MES and KG split their terms the same way.  (4) pm_tile_tail with the
//              believer's exclusion over this entry's sel_idx.  No LDS beyond prediction's: the row tiles move to the global slots
//              at prediction's sizes.  A task with no valid target is still WALKED - the walk owns its tasks by kind, and its tile
//              (K, C = K A^-1, the reductions) runs at every step - but the epilogue returns before the panel: no score, its
//              trace stays 0 and nothing is listed.  The same tile work is spent on a task that has run out of eligible rows.
//   float64    tasks take k_ipv_walk64 (pm64_pool_walk): lane i forms c0(x, entry i) in float64 (bv64_c0) and rounds it to float32
//              as the tile holds it; the substitution against G64 runs across the pick lanes, the products with Lr64 in the target
//              lanes, in float64; the variance is rounded to float32 before the clamp, and the weighted squares are added in a
//              fixed butterfly.  A task takes one kind of walk.
//   k_ipv_step one workgroup per task per step, from the believer's functions: the merge of the task's lists at width 1, the
//              pick's row, k(Z_s, x_p) and w into entry slot M + c (bv_store_row, bv_kernel_col, bv_solve_w), c0(x_p, e) for
//              every entry e < M + c from the stored rows and W in float64 (one wave per entry), then the new row of G as
//              k_bv_step forms it, the new row of Lr, ell_c(r_m) = (c0(r_m, p) - sum_(l<c) G[c, l] ell_l(r_m)) / G[c, c] - from
//              G and Lr as stored: float32 for float32 tasks, float64 for flagged ones - and tvar_(c+1), summed by ascending m by
//              one thread.  With no eligible row it reports -1 / -inf and changes nothing, so every later step does the same.
//
// A target row with NaN or infinite features has NaN w and covariances, so every score of its task is NaN and nothing is selected
// (include/adkf_gp.h says so): keep such rows out of tgt_idx.  A row whose own mean or variance is NaN scores NaN.
//
// Deterministic: no atomics, every sum has a fixed order; a task's result does not depend on the grid or on the other tasks.
#pragma once
#include "jes_stream.h"

namespace adkf {

struct IpvArgs {
    int M, q, j;                        // target entries and picks per task; the step of this launch
    const int64_t* tgt_idx;             // [T, M]: the caller's target rows
    const float* tgt_w;                 // nullable [T, M]: their weights (null: 1)
    float* W; double* W64;              // [T, M + q, ns_ld]: w of entry e (float64 tasks: W64; null without a float64 region)
    float* Xp;                          // [T, M + q, d]: the entries' feature rows
    float* G; double* G64;              // [T, q, q] lower triangular
    float* Lr; double* Lr64;            // [T, q, M]: ell_i(r_m)
    float* wt;                          // [T, M]: the weight of target m, 0: skipped
    double* v0r;                        // [T, M]: v_0(r_m)
    double* tv;                         // [T]: tvar after the picks made
    int32_t *cnt, *nv;                  // [T]: the picks made; the valid targets
    float* trace;                       // nullable [T, q, rows]
    int64_t* sel_idx; float* sel_val;   // [T, q]
    float* tvar;                        // nullable [T, q + 1]
};
struct IpvEpilogue;
template <bool ARD>
using IpvKargs = PmArgsOf<ARD, true, IpvEpilogue>;   // p.Zq: the pool; s.k = 1, s.cand_* [T, chunks_max]; ARD: r, the query scaling

// the believer's view of the state: the entry list as "picks" of the c0 panel, and G with sel_idx for the substitution and the exclusion
__device__ __forceinline__ BvArgs ipv_entries(const IpvArgs& v) {
    BvArgs b{};
    b.q = v.M + v.q; b.W = v.W; b.W64 = v.W64; b.Xp = v.Xp;
    return b;
}
__device__ __forceinline__ BvArgs ipv_picks(const IpvArgs& v) {
    BvArgs b{};
    b.q = v.q; b.j = v.j; b.G = v.G; b.G64 = v.G64; b.sel_idx = v.sel_idx;
    return b;
}

// ---- the target state: one workgroup per (entry, task)
template <bool ARD>
__global__ __launch_bounds__(256) void k_ipv_refs(IpvKargs<ARD> args) {
    const PmArgs& a = args.p;
    const IpvArgs& v = args.v;
    __shared__ __attribute__((aligned(16))) float fb[3 * TS_NS_MAX];
    __shared__ double red[256];
    const int m = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, M = v.M, E = M + v.q, ld = a.ns_ld;
    const size_t o = (size_t)t * M + m, e = (size_t)t * E + m;
    const long long idx = v.tgt_idx[o];
    const float w = v.tgt_w ? v.tgt_w[o] : 1.f;
    bool ok = pm_kind_of(a, t) >= 0 && idx >= 0 && idx < a.rows && w > 0.f;   // (a NaN weight fails the comparison)
    for (int i = 0; ok && i < m; ++i) ok = v.tgt_idx[(size_t)t * M + i] != idx;   // (uniform) the first occurrence counts
    bv_ref_entry<ARD>(args, t, ok, idx, v.Xp + e * a.d, v.W + e * ld, v.W64 ? v.W64 + e * ld : nullptr, fb, red);
    double v0 = 0.0;
    if (ok) {   // (uniform) k and w are where bv_ref_entry left them
        const bool f64 = pm_kind_of(a, t) == 2;
        const int n = pm_ns(a, t);
        const float *rs = fb, *vs = fb + TS_NS_MAX;
        const double *k64 = reinterpret_cast<double*>(fb), *w64 = k64 + R64_MAXN;
        double pk = 0.0;
        for (int i = tid; i < n; i += 256) pk += f64 ? w64[i] * k64[i] : (double)vs[i] * (double)rs[i];
        v0 = (double)a.scal[(size_t)t * NSCAL + S_OS] - bv_block_sum(pk, red);
    }
    if (tid == 0) { v.wt[o] = ok ? w : 0.f; v.v0r[o] = v0; }
}

// ---- the per-task state before step 0: a thread per task (k_bv_init's shape)
__global__ __launch_bounds__(256) void k_ipv_init(IpvArgs v, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x, M = v.M;
    if (t >= T) return;
    int nv = 0;
    double tv = 0.0;
    for (int m = 0; m < M; ++m) {
        const float w = v.wt[(size_t)t * M + m];
        if (w > 0.f) { ++nv; tv += (double)w * v.v0r[(size_t)t * M + m]; }
    }
    v.cnt[t] = 0; v.nv[t] = nv; v.tv[t] = tv;
    if (v.tvar) v.tvar[(size_t)t * (v.q + 1)] = (float)tv;
}

struct IpvEpilogue {
    using Args = IpvArgs;
    template <bool ARD, bool POOL, class ARGS, class WALK>
    static __device__ __forceinline__ void run(const ARGS& args, const PmTile& tl, WALK& walk, f32x4 (&acc)[2][2]) {
        static_assert(POOL, "adkf_ipv_pool: a shared pool");
        const PmArgs& a = args.p;
        const IpvArgs& v = args.v;
        const int tid = threadIdx.x, row = tid & 63, part = tid >> 6, t = tl.t, M = v.M, q = v.q;
        if (v.nv[t] == 0) return;   // (uniform) no valid target: nothing is scored or listed
        const int c = v.cnt[t];     // (uniform) picks made, at most the step
        constexpr int DEN = PM_TM;  // the pad column of the panel: the row's denominator
        float* C0 = tl.As;          // the c0 panel [64, BV_LDC]: targets 0 .. M, picks M .. M + c; at the end [4][64] partial sums
        const BvArgs bp = ipv_picks(v);
        bv_c0_panel<ARD>(a, ipv_entries(v), tl, acc, M + c);
        if (tid < tl.m) {
            float vl = tl.var(tid);
            if (c > 0) vl -= bv_downdate(bp, t, c, C0 + tid * BV_LDC + M);
            C0[tid * BV_LDC + DEN] = fmaxf(vl, 1e-12f) + tl.noise;
        }
        __syncthreads();
        const float* Cr = C0 + row * BV_LDC;
        const float* Lr = v.Lr + (size_t)t * q * M;
        const float* wt = v.wt + (size_t)t * M;
        const float den = Cr[DEN];
        float sum = 0.f;
        for (int m = part; m < M; m += PM_NT / 64) {   // (m is uniform over a wave: wt and Lr are read once per wave)
            const float w = wt[m];
            if (!(w > 0.f)) continue;
            float cv = Cr[m];
            for (int i = 0; i < c; ++i) cv = fmaf(-Cr[M + i], Lr[(size_t)i * M + m], cv);
            sum = fmaf(w * cv, cv, sum);
        }
        __syncthreads();   // the panel is dead: the partial sums may overwrite it
        float* ps = tl.As;
        ps[part * PM_TM + row] = sum;
        __syncthreads();
        float score = 0.f;
        if (tid < tl.m) {
            score = pm_sum4(ps, tid) / den;
            if (tl.is_nan(tid)) score = NAN;   // a NaN mean or variance: NaN, never selected (fmaxf would hide it)
        }
        pm_tile_tail(args, tl, walk, score, v.trace, (size_t)t * q + v.j, 1, bv_excl(args.s, bp, t, c));
    }
};
static_assert(ADKF_IPV_ENTRIES_MAX == PM_TM && PM_TM < BV_LDC, "IpvEpilogue: one c0 panel for targets and picks, its pad column the denominator");

// ---- flagged tasks: the float64 pool walk (pm64_pool_walk), lane e the entry e
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_ipv_walk64(IpvKargs<ARD> args) {
    const PmArgs& a = args.p;
    const IpvArgs& v = args.v;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, M = v.M, q = v.q, E = M + q;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    if (v.nv[t] == 0) return;                   // (uniform) no valid target
    const int c = v.cnt[t];
    const double* Wt = v.W64 + (size_t)t * E * tk.ld;
    const double* G = v.G64 + (size_t)t * q * q;
    const double* Lr = v.Lr64 + (size_t)t * q * M;
    const float* Xp = v.Xp + (size_t)t * E * a.d;
    const BvArgs bp = ipv_picks(v);
    const double w = lane < M ? (double)v.wt[(size_t)t * M + lane] : 0.0;
    const float noise = (float)tk.noise;
    pm64_pool_walk<ARD>(args, tk, kr[wv], 1, bv_excl(args.s, bp, t, c), [&](int64_t r, const float* zq, const double* k, double s1, double s2) {
        const double c0 = (double)(float)bv64_c0<ARD>(a, tk, zq, k, Wt, Xp, M + c, lane);   // lane e: c0(x, e), as the tile holds it
        double part = 0.0, ss = 0.0, cv = c0;   // pick lanes: sum_(l < i) G[i, l] ell_l so far; target lanes: cov_j(x, r_lane)
        for (int i = 0; i < c; ++i) {
            double e = lane == M + i ? (c0 - part) / G[(size_t)i * q + i] : 0.0;
            e = __shfl(e, M + i);
            if (lane > M + i && lane < M + c) part += G[(size_t)(lane - M) * q + i] * e;
            if (lane < M) cv -= e * Lr[(size_t)i * M + lane];
            ss += e * e;
        }
        double term = w > 0.0 ? w * cv * cv : 0.0;
        for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o);
        const float vl = (float)(tk.os - s2 - ss);
        float score = (float)(term / (double)(fmaxf(vl, 1e-12f) + noise));
        if (s1 != s1 || s2 != s2) score = NAN;   // as the tile: a NaN mean or variance scores NaN
        if (lane == 0 && v.trace) v.trace[((size_t)t * q + v.j) * (size_t)a.rows + (size_t)r] = score;
        return score;
    });
}

// ---- the end of step j: one workgroup per task (see the top of the file)
template <bool ARD>
__global__ __launch_bounds__(256) void k_ipv_step(IpvKargs<ARD> args) {
    const PmArgs& a = args.p;
    const PmPool& s = args.s;
    const IpvArgs& v = args.v;
    __shared__ __attribute__((aligned(16))) float fb[3 * TS_NS_MAX];
    __shared__ double red[256];
    __shared__ double c0s[ADKF_IPV_ENTRIES_MAX];
    __shared__ long long pick_s;
    __shared__ float val_s;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, M = v.M, q = v.q, E = M + q;
    const size_t o = (size_t)t * q + v.j;
    if (wv == 0) {   // the task's lists under the total order (skipped tasks, and every task when no walk ran, have none)
        float lv;
        long long li;
        pm_merge_task_lists(a, s, t, 1, lv, li);
        if (lane == 0) { pick_s = v.nv[t] > 0 ? li : -1; val_s = lv; }
    }
    __syncthreads();
    const long long p = pick_s;
    if (p < 0) {   // (uniform) no eligible row: the state stays as it is
        if (tid == 0) {
            v.sel_idx[o] = -1; v.sel_val[o] = -INFINITY;
            if (v.tvar) v.tvar[(size_t)t * (q + 1) + v.j + 1] = (float)v.tv[t];
        }
        return;
    }
    const bool f64 = pm_kind_of(a, t) == 2;
    const int n = pm_ns(a, t), ld = a.ns_ld, d = a.d, c = v.cnt[t];
    const float* sc = a.scal + (size_t)t * NSCAL;
    const double os = sc[S_OS], noise = sc[S_NOISE], il2 = 1.0 / ((double)sc[S_LS] * (double)sc[S_LS]);
    const float* xp = a.Zq + (size_t)p * d;
    const float* Zs = a.Zs + (size_t)t * ld * d;
    float* Xt = v.Xp + (size_t)t * E * d;
    const size_t we = (size_t)t * E * ld;   // the task's first entry in W / W64
    xp = bv_store_row<ARD>(args, t, f64, xp, Xt + (size_t)(M + c) * d);
    float *rs = fb, *vs = fb + TS_NS_MAX;   // float32 tasks: k, then w in vs (bv_solve_w)
    double *k64 = reinterpret_cast<double*>(fb), *w64 = k64 + R64_MAXN;   // float64 tasks (n <= R64_MAXN): k and w
    bv_kernel_col(a, Zs, xp, n, os, il2, f64, k64, rs);
    bv_solve_w(a, t, n, f64, fb, v.W + we + (size_t)(M + c) * ld, f64 ? v.W64 + we + (size_t)(M + c) * ld : nullptr);
    // ---- the pick's prior-step variance s - k . w
    double pk = 0.0;
    for (int i = tid; i < n; i += 256) pk += f64 ? w64[i] * k64[i] : (double)vs[i] * (double)rs[i];
    const double v0 = os - bv_block_sum(pk, red);
    // ---- c0(x_p, e) for the targets and the earlier picks: one wave per entry (a skipped target's is never read)
    for (int e = wv; e < M + c; e += 4) {
        const float* xi = Xt + (size_t)e * d;
        double sq = 0.0, f = 0.0;
        for (int x = lane; x < d; x += 64) { const double df = (double)xp[x] - (double)xi[x]; sq += df * df; }
        for (int k = lane; k < n; k += 64)
            f += f64 ? k64[k] * v.W64[we + (size_t)e * ld + k] : (double)rs[k] * (double)v.W[we + (size_t)e * ld + k];
        for (int x = 32; x > 0; x >>= 1) { sq += __shfl_xor(sq, x); f += __shfl_xor(f, x); }
        if (lane == 0) c0s[e] = os * kappa0(a.kind, sq * il2) - f;
    }
    __syncthreads();
    const size_t go = ((size_t)t * q + c) * q;   // the new row of G
    if (tid == 0) {   // (k_bv_step's)
        double* ep = c0s + M;
        double ss = 0.0;
        for (int i = 0; i < c; ++i) {
            double x = ep[i];
            for (int l = 0; l < i; ++l) x -= (f64 ? v.G64[((size_t)t * q + i) * q + l] : (double)v.G[((size_t)t * q + i) * q + l]) * ep[l];
            x /= f64 ? v.G64[((size_t)t * q + i) * q + i] : (double)v.G[((size_t)t * q + i) * q + i];
            ep[i] = x;
            ss += x * x;
        }
        const double vj = v0 - ss, gd = sqrt(fmax(vj + noise, 1e-30));
        for (int i = 0; i <= c; ++i) {
            const double g = i < c ? ep[i] : gd;
            if (f64) v.G64[go + i] = g; else v.G[go + i] = (float)g;
            ep[i] = f64 ? g : (double)(float)g;   // as stored: what the walks will read
        }
        v.sel_idx[o] = p; v.sel_val[o] = val_s;
    }
    __syncthreads();
    // ---- the new row of Lr and the targets' variances after it: thread m the target m
    double vm = 0.0;
    if (tid < M && v.wt[(size_t)t * M + tid] > 0.f) {
        const int m = tid;
        const double* ep = c0s + M;
        double x = c0s[m], used = 0.0;
        for (int l = 0; l < c; ++l) {
            const double e = f64 ? v.Lr64[((size_t)t * q + l) * M + m] : (double)v.Lr[((size_t)t * q + l) * M + m];
            x -= ep[l] * e;
            used += e * e;
        }
        x /= ep[c];
        if (f64) v.Lr64[((size_t)t * q + c) * M + m] = x; else { v.Lr[((size_t)t * q + c) * M + m] = (float)x; x = (double)(float)x; }
        vm = (double)v.wt[(size_t)t * M + m] * (v.v0r[(size_t)t * M + m] - (used + x * x));
    } else if (tid < M) {
        if (f64) v.Lr64[((size_t)t * q + c) * M + tid] = 0.0; else v.Lr[((size_t)t * q + c) * M + tid] = 0.f;
    }
    if (tid < ADKF_IPV_ENTRIES_MAX) red[tid] = vm;
    __syncthreads();
    if (tid == 0) {
        double tv = 0.0;
        for (int m = 0; m < M; ++m) tv += red[m];
        v.tv[t] = tv;
        if (v.tvar) v.tvar[(size_t)t * (q + 1) + v.j + 1] = (float)tv;
        v.cnt[t] = c + 1;
    }
}

}  // namespace adkf
