// Monte-Carlo (noisy) q-EI over a shared pool (adkf_qei_pool): q sequential-greedy picks per task, each scored jointly with the picks
// before it by a sample average over S pathwise posterior draws (Wilson, Hutter and Deisenroth 2018; Balandat et al. 2020; the noisy
// incumbent of Letham et al. 2019).  The paths f_s are Thompson's (thompson_stream.h: the same basis, draws, residual and solve), so
// the call is a deterministic function of its arguments.  Per task, with b_s the incumbent of path s (minimisation; ADKF_PM_MAXIMIZE
// flips the difference and min becomes max):
//     b_s^0      = min_(i < n_s) f_s(z_i)   (best_f NULL: noisy q-EI)   or   best_f[t]   (plain q-EI)
//     score_j(x) = (1 / S) sum_s max(0, b_s^j - f_s(x))
//     p_j        = the best eligible row under pm_beats (not excluded, not an earlier pick, score not NaN)
//     b_s^(j+1)  = min(b_s^j, f_s(p_j))
// The noisy incumbent needs no product: A v = r and K_ss = A - noise I give f_s(z_i) = y_i - sqrt(noise) eps_(s,i) - noise v_(s,i),
// whose error is the residual of the solve (k_qei_init; flagged tasks in float64 from V64).
//
// Launches, ordered by launch boundaries (no atomics; every sum has a fixed order that does not depend on the grid or on T):
//   k_ts_resid, k_ts_solve   once per call, Thompson's kernels as they are, S up to 256;
//   k_qei_init               b^0, inc row 0 and the pick count;
//   q times:
//     k_qei_stream<ARD, NB>  Thompson's walk and tile (ts_tile) with NB = 1, 2 or 4 sample blocks of 64: the feature product, the cosine
//                            panel and the K panel are computed once per chunk / panel, only the staging of W or V and the MFMA repeat per
//                            block, into F[NB][2][2].  Block bk, lane-sample s is what adkf_thompson_pool computes for sample 64 bk + s
//                            alone, bit for bit.  Epilogue: block by block the tile goes through the LDS panel as [sample][row]; thread
//                            (row, quarter) adds the clipped differences of the samples quarter, quarter + 4, ... of each block against b
//                            (in LDS, staged once per task visit); the four quarters meet in pm_mm's staging buffer (pm_sum4) and the sum
//                            is divided by S.  pm_tile_tail stores the trace and offers the scores to the walk's one-entry list under
//                            qe_excl.  When the entry changes, the tile goes through the panel once more and the new row's S path values
//                            go to the candidate slot of this (task, chunk) with ordinary stores;
//     k_qei_stream64<ARD>    flagged tasks, after k_ts_stream64: one wave per pool row, lane l carries the samples l + 64 bk, the kernel
//                            row and each feature computed once; the clipped differences are summed in float64 (butterfly) and rounded
//                            once; each wave keeps its best row's values in registers and the workgroup's best wave stores them;
//     k_qei_step             one workgroup per task: merges the chunks' pairs (pm_merge_lists), writes sel_*[j], finds the chunk that
//                            holds the winner, moves b by that candidate's stored path values - the numbers that were scored - and
//                            writes inc row j + 1 and the count.  No eligible row: -1 / -inf, the state stays, and every later step
//                            does the same (the believer's rule).
#pragma once
#include "believer_stream.h"

namespace adkf {

constexpr int QE_S_MAX = 256;          // ADKF_QEI_SAMPLES_MAX: four blocks of 64
constexpr int QE_Q_MAX = 64;           // ADKF_QEI_PICKS_MAX
constexpr int QE_NB_MAX = QE_S_MAX / TS_S_MAX;

struct QeArgs : TsArgs {                // p.Zq: the pool; s.k = 1, s.cand_* [T, chunks_max]; paths and top_* unused
    int q, j;                           // picks per task; the step of this launch
    float* b; int32_t* cnt;             // [T, S]: the incumbents; [T]: the picks made
    float* slots;                       // [T, chunks_max, S]: the path values of each (task, chunk) candidate
    const float* best_f;                // nullable [T]: null - the noisy incumbent
    float *trace, *inc;                 // nullable [T, q, rows], [T, q + 1, S]
    int64_t* sel_idx; float* sel_val;   // [T, q]
};
struct QeArgsArd : QeArgs { PmArd r; };
template <bool ARD>
using QeArgsOf = std::conditional_t<ARD, QeArgsArd, QeArgs>;

// what task t may not select with c picks made: its exclusion list and the picks (the believer's rule)
__device__ __forceinline__ auto qe_excl(const QeArgs& v, int t, int c) {
    return [&v, t, c](long long r) {
        if (pm_excluded(v.s, t, r)) return true;
        for (int i = 0; i < c; ++i)
            if (v.sel_idx[(size_t)t * v.q + i] == r) return true;
        return false;
    };
}
// one term of the score: NaN stays NaN (a NaN path value makes the row's score NaN, which is never selected)
__device__ __forceinline__ float qe_clip(float imp) { return imp < 0.f ? 0.f : imp; }

// ---- b^0, inc row 0 and the count: one workgroup per task, thread s the samples s, s + 256, ...
__global__ __launch_bounds__(256) void k_qei_init(QeArgs v) {
    const PmArgs& a = v.p;
    const int t = blockIdx.x, S = v.S, ld = a.ns_ld;
    const int kind = pm_kind_of(a, t);
    const int n = pm_ns(a, t);
    const float* sc = a.scal + (size_t)t * NSCAL;
    const float* ys = a.y_s + (size_t)t * ld;
    if (threadIdx.x == 0) v.cnt[t] = 0;
    for (int s = threadIdx.x; s < S; s += 256) {
        float b0 = 0.f;   // (a skipped task: nothing reads it)
        if (v.best_f) {
            b0 = v.best_f[t];
        } else if (kind >= 0) {
            const size_t base = ((size_t)t * S + s) * ld;
            if (kind == 2) {
                const double noise = sc[S_NOISE], sigma = sqrt(noise);
                double m = 0.0;
                for (int i = 0; i < n; ++i) {
                    const double f = (double)ys[i] - sigma * (double)v.eps[base + i] - noise * v.V64[base + i];
                    m = i == 0 ? f : (a.maximize ? fmax(m, f) : fmin(m, f));
                }
                b0 = (float)m;
            } else {
                const float noise = sc[S_NOISE], sigma = sqrtf(noise);
                for (int i = 0; i < n; ++i) {
                    const float f = fmaf(-noise, v.V[base + i], fmaf(-sigma, v.eps[base + i], ys[i]));
                    b0 = i == 0 ? f : (a.maximize ? fmaxf(b0, f) : fminf(b0, f));
                }
            }
        }
        v.b[(size_t)t * S + s] = b0;
        if (v.inc) v.inc[(size_t)t * (v.q + 1) * S + s] = b0;
    }
}

// ---- the walk of the float32 tasks (plain and refined alike, as k_ts_stream)
template <bool ARD, int NB>
__global__ __launch_bounds__(PM_NT) void k_qei_stream(QeArgsOf<ARD> args) {
    const QeArgs& v = args;
    const TsArgs& ts = v;
    const PmArgs& a = ts.p;
    __shared__ float As[PM_TM * LD_MN], Bs[PM_TM * LD_MN];
    __shared__ float Pp[PM_TM * TS_LDP], Bp[PM_TM * TS_LDP];
    __shared__ float rowsq[2][PM_TM];
    __shared__ float bs[QE_S_MAX];
    __shared__ int win_s;
    static_assert(4 * PM_TM <= PM_TM * LD_MN, "the four partial sums of a row fit in one staging buffer");
    const int tid = threadIdx.x, wv = tid >> 6, row = tid & 63;
    const int S = ts.S;
    PmPoolWalk<TS_KINDS32> walk;
    if (!walk.start(a, ts.s)) return;
    int cur_t = -1, c = 0;
    for (;;) {
        int t;
        int64_t r0;
        if (!walk.next(a, ts.s, 1, t, r0)) return;
        const int mr = (int)(a.rows - r0 < PM_TM ? a.rows - r0 : PM_TM);
        if (t != cur_t) {   // (uniform) the incumbents and the pick count of the task; published by the barriers of the tile
            cur_t = t;
            c = v.cnt[t];
            for (int s = tid; s < S; s += PM_NT) bs[s] = v.b[(size_t)t * S + s];
        }
        const float* ril = nullptr;
        if constexpr (ARD) ril = args.r.il + (size_t)t * a.d;
        f32x4 F[NB][2][2];
        ts_tile<ARD, NB>(ts, ril, t, r0, mr, As, Bs, Pp, Bp, rowsq, F);
        // ---- the score: thread (row, wv) adds the samples wv, wv + 4, ... of every block, blocks ascending
        float part = 0.f;
#pragma unroll
        for (int bk = 0; bk < NB; ++bk) {
            if (bk * TS_S_MAX < S) {   // (uniform)
                ts_tile_to_lds(Pp, F[bk]);
                __syncthreads();
                const int sb = S - bk * TS_S_MAX < TS_S_MAX ? S - bk * TS_S_MAX : TS_S_MAX;
                for (int s = wv; s < sb; s += 4) {
                    const float f = Pp[s * TS_LDP + row], bb = bs[bk * TS_S_MAX + s];
                    part += qe_clip(a.maximize ? f - bb : bb - f);
                }
                __syncthreads();
            }
        }
        As[wv * PM_TM + row] = part;
        long long li0 = 0;
        if (tid == 0) li0 = walk.li;
        __syncthreads();
        const float score = tid < mr ? pm_sum4(As, tid) / (float)S : 0.f;
        PmTile tl{};
        tl.t = t; tl.r0 = r0; tl.m = mr;
        pm_tile_tail(ts, tl, walk, score, v.trace, (size_t)t * v.q + v.j, 1, qe_excl(v, t, c));
        // ---- a new best row of this (task, chunk): its S path values to the candidate slot
        if (tid == 0) win_s = walk.li != li0 ? (int)(walk.li - r0) : -1;
        __syncthreads();
        const int win = win_s;
        if (win >= 0) {   // (uniform)
            float* slot = v.slots + ((size_t)t * ts.s.chunks_max + walk.pchunk) * S;
#pragma unroll
            for (int bk = 0; bk < NB; ++bk) {
                if (bk * TS_S_MAX < S) {
                    ts_tile_to_lds(Pp, F[bk]);
                    __syncthreads();
                    if (tid < TS_S_MAX && bk * TS_S_MAX + tid < S) slot[bk * TS_S_MAX + tid] = Pp[tid * TS_LDP + win];
                    __syncthreads();
                }
            }
        }
        __syncthreads();   // the panels, the partial sums and win_s are rewritten by the next tile
    }
}

// ---- flagged tasks: one wave per pool row in float64, grid (chunks, T), the rows of k_ts_stream64; lane l carries the samples l + 64 bk
template <bool ARD>
__global__ __launch_bounds__(PM64_NT) void k_qei_stream64(QeArgsOf<ARD> args) {
    const QeArgs& v = args;
    const TsArgs& ts = v;
    const PmArgs& a = ts.p;
    __shared__ double kr[PM64_WAVES][R64_MAXN];
    __shared__ float wave_v[PM64_WAVES];
    __shared__ long long wave_i[PM64_WAVES];
    const int t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, S = ts.S, m = ts.m;
    Pm64Task tk;
    if (!pm64_task<ARD>(args, t, tk)) return;   // (uniform)
    const int n = tk.n, ld = tk.ld;
    [[maybe_unused]] const double il = 1.0 / tk.ls, il2 = il * il, amp = sqrt(2.0 * tk.os / (double)m);   // (k_ts_stream64's il2: its bits)
    const int nb = (S + TS_S_MAX - 1) / TS_S_MAX, c = v.cnt[t];
    const float* wq[QE_NB_MAX];
    const double* vq[QE_NB_MAX];
    float bb[QE_NB_MAX], keep[QE_NB_MAX];
#pragma unroll
    for (int bk = 0; bk < QE_NB_MAX; ++bk) {
        const int s = bk * TS_S_MAX + lane, ql = s < S ? s : S - 1;   // (lanes beyond S compute sample S - 1 again and add nothing)
        wq[bk] = ts.w + ((size_t)t * S + ql) * m;
        vq[bk] = ts.V64 + ((size_t)t * S + ql) * ld;
        bb[bk] = v.b[(size_t)t * S + ql];
        keep[bk] = 0.f;
    }
    double* k = kr[wv];
    float lv = -INFINITY;
    long long li = -1;
    const auto excl = qe_excl(v, t, c);
    for (int64_t r = (int64_t)blockIdx.x * PM64_WAVES + wv; r < a.rows; r += (int64_t)gridDim.x * PM64_WAVES) {
        const float* zq = a.Zq + (size_t)r * a.d;
        pm64_kernel_row<ARD>(a, tk, zq, il2, k);
        double f[QE_NB_MAX] = {0.0, 0.0, 0.0, 0.0};
        for (int j0 = 0; j0 < m; j0 += 64) {   // one feature per lane, then every lane adds its samples' 64 terms (k_ts_stream64's order)
            const float* om = ts.omega + (size_t)(j0 + lane) * a.d;
            double s = 0.0;
            double cv;
            if constexpr (ARD) {
                for (int e = 0; e < a.d; ++e) s = fma((double)om[e], (double)ard_scaled(zq[e], tk.mu[e], tk.el[e]), s);
                cv = amp * ts_cos(s + (double)ts.phase[j0 + lane]);
            } else {
                for (int e = 0; e < a.d; ++e) s = fma((double)om[e], (double)zq[e] - (double)tk.mu[e], s);
                cv = amp * ts_cos(s * il + (double)ts.phase[j0 + lane]);
            }
            for (int jj = 0; jj < 64; ++jj) {
                const double cj = __shfl(cv, jj);
#pragma unroll
                for (int bk = 0; bk < QE_NB_MAX; ++bk)
                    if (bk < nb) f[bk] = fma((double)wq[bk][j0 + jj], cj, f[bk]);
            }
        }
        double sum = 0.0;
        float ff[QE_NB_MAX];
#pragma unroll
        for (int bk = 0; bk < QE_NB_MAX; ++bk) {
            ff[bk] = 0.f;
            if (bk < nb) {
                double u = 0.0;
                for (int j = 0; j < n; ++j) u = fma(k[j], vq[bk][j], u);
                ff[bk] = (float)(f[bk] + u);
                if (bk * TS_S_MAX + lane < S) {
                    const double imp = a.maximize ? (double)ff[bk] - (double)bb[bk] : (double)bb[bk] - (double)ff[bk];
                    sum += imp < 0.0 ? 0.0 : imp;
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        const float score = (float)(sum / (double)S);
        if (lane == 0 && v.trace) v.trace[((size_t)t * v.q + v.j) * (size_t)a.rows + (size_t)r] = score;
        const long long before = __shfl(li, 0);
        pm_list_merge(lv, li, 1, score, (long long)r, lane == 0, excl);
        if (__shfl(li, 0) != before) {   // (wave-uniform) this row is the wave's best so far: keep its values
#pragma unroll
            for (int bk = 0; bk < QE_NB_MAX; ++bk) keep[bk] = ff[bk];
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    // ---- the workgroup's best wave under the total order stores the pair and its values as those of (t, blockIdx.x)
    if (lane == 0) { wave_v[wv] = lv; wave_i[wv] = li; }
    __syncthreads();
    int best = 0;
    for (int w = 1; w < PM64_WAVES; ++w)
        if (wave_i[w] >= 0 && pm_beats(wave_v[w], wave_i[w], wave_v[best], wave_i[best])) best = w;
    if (wv != best) return;
    pm_list_store(ts.s, t, blockIdx.x, lane, 1, lv, li);
    if (__shfl(li, 0) >= 0) {
        float* slot = v.slots + ((size_t)t * ts.s.chunks_max + blockIdx.x) * S;
#pragma unroll
        for (int bk = 0; bk < QE_NB_MAX; ++bk)
            if (bk * TS_S_MAX + lane < S) slot[bk * TS_S_MAX + lane] = keep[bk];
    }
}

// ---- the end of step j: one workgroup per task (see the top of the file)
__global__ __launch_bounds__(256) void k_qei_step(QeArgs v) {
    const TsArgs& ts = v;
    const PmArgs& a = ts.p;
    const PmPool& s = ts.s;
    __shared__ long long pick_s;
    __shared__ float val_s;
    __shared__ int chunk_s;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, S = ts.S, q = v.q;
    const size_t o = (size_t)t * q + v.j;
    const int C = pm_task_chunks(a, s, t, false);   // (one walk serves the plain and the refined tasks, as Thompson's)
    if (wv == 0) {
        float lv;
        long long li;
        pm_merge_lists(s, (size_t)t * s.chunks_max, C, 1, lv, li);
        if (lane == 0) { pick_s = li; val_s = lv; chunk_s = -1; }
    }
    __syncthreads();
    const long long p = pick_s;
    if (p >= 0)   // (uniform) the chunk whose candidate won: the chunks walk disjoint rows
        for (int ch = tid; ch < C; ch += 256)
            if (s.cand_idx[(size_t)t * s.chunks_max + ch] == p) chunk_s = ch;
    __syncthreads();
    const int ch = chunk_s;
    float* inc = v.inc ? v.inc + ((size_t)t * (q + 1) + v.j + 1) * S : nullptr;
    if (p < 0 || ch < 0) {   // (uniform) no eligible row: the state stays as it is
        if (tid == 0) { v.sel_idx[o] = -1; v.sel_val[o] = -INFINITY; }
        if (inc)
            for (int e = tid; e < S; e += 256) inc[e] = v.b[(size_t)t * S + e];
        return;
    }
    const float* slot = v.slots + ((size_t)t * s.chunks_max + ch) * S;
    for (int e = tid; e < S; e += 256) {
        const float b0 = v.b[(size_t)t * S + e], f = slot[e];
        const float b1 = a.maximize ? fmaxf(b0, f) : fminf(b0, f);
        v.b[(size_t)t * S + e] = b1;
        if (inc) inc[e] = b1;
    }
    if (tid == 0) { v.sel_idx[o] = p; v.sel_val[o] = val_s; v.cnt[t] = v.cnt[t] + 1; }
}

}  // namespace adkf
