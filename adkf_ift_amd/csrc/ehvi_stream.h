// Constrained expected hypervolume improvement ACROSS tasks over a shared pool (adkf_ehvi_pool; Emmerich, Deutz and Klinkenberg 2011,
// Yang et al. 2019 for the exact two-objective form; Schonlau 1998, Gardner et al. 2014 for the feasibility weight).  A group names
// one or two objective tasks and up to four constraint tasks of the same batch.  With m_t, v_t the latent posterior of prediction at a
// pool row, s_t = sqrt(max(v_t, 1e-12)) (pm_ei's clamp), every objective turned into minimisation (a maximised one is negated: mean,
// front column, reference coordinate) and psi_t(c) = E[(c - y_t)+] = pm_ei(m_t, v_t, c, 0), psi_t(-inf) = 0:
//     two objectives   EHVI = sum_{i = 0 .. P} [psi_1(a_(i+1)) - psi_1(a_i)] psi_2(b_i)
//                      over the staircase (a_1, b_1) .. (a_P, b_P) of the group's front (a ascending, b descending), a_0 = -inf,
//                      b_0 = r2, a_(P+1) = r1, r the reference point;
//     one objective    EHVI = psi_1(r1): EI with best_f = r1;
//     constraints      PoF = prod_c Phi(z_c), z_c = (thr_c - m_c) / s_c ("f <= thr") or (m_c - thr_c) / s_c ("f >= thr");
//     score            EHVI PoF, or log EHVI + sum_c log Phi(z_c) formed in log space throughout (ADKF_PM_LOG_EI).
//
//   stage A   the host walks the pool in chunks of EHVI_CHUNK_ROWS rows and runs prediction itself (pm_launch<ARD, true>, latent, k = 0)
//             on each: m and v [T, chunk] in the scratch are prediction's by construction, for every kind of task.
//   k_ehvi_stair   one wave per group, lane i the front point i: validity, dominance by shuffles, rank by counting; the staircase,
//             its count, the senses, the reference point, the constraints and the "cannot be evaluated" flag go to the scratch.
//   k_ehvi_score   a persistent grid over (group, 64-row tile of the chunk), a group's tiles spread over chunks of the grid as
//             PmPoolWalk spreads a task's.  256 threads: all four waves fill two [P + 1][64] LDS panels with the edge values - every
//             psi_1(a_i) and psi_2(b_i) of a row once - then thread row + 64 part sums the strips part, part + 4, ..; the four
//             partials are added in the order 0, 1, 2, 3 (as MesEpilogue).  Thread (row, c) evaluates constraint c.  The first wave
//             offers the 64 scores to the list of (group, walker), which lives in the scratch across the chunk launches.
//   k_ehvi_topk    one wave per group merges the group's lists (pm_merge_task_lists' logic over groups).
//
// Log form: per edge l = pm_log_ei; a strip's weight l_hi + log(1 - exp(l_lo - l_hi)) (the first strip: l_hi itself); the strips by a
// log-sum-exp with a fixed-order maximum and a fixed-order sum; -inf terms are skipped, all -inf gives -inf.
//
// Deterministic: no atomics, every sum has a fixed order; a group's bits depend on its own tasks, front, reference, constraints and
// the pool row only - not on the grid, the other groups or the chunk boundaries.  A group that cannot be evaluated (see
// include/adkf_gp.h) scores NaN everywhere and selects nothing.
#pragma once
#include "mes_stream.h"

namespace adkf {

constexpr int EHVI_FRONT_MAX = 64;
constexpr int EHVI_CONS_MAX = 4;
constexpr int EHVI_CHUNK_ROWS = 16384;
constexpr int EHVI_NT = 256;

// a group as k_ehvi_score reads it (written by k_ehvi_stair); every member is 4 bytes wide
struct EhviGroup {
    int bad, two, P, pad;
    int t[2];                       // the objective tasks
    float sg[2];                    // +1: minimised, -1: maximised
    float r[2];                     // the reference point, in the minimisation sense
    int ct[EHVI_CONS_MAX];          // the constraint tasks, -1: unused
    float cthr[EHVI_CONS_MAX];
    int cgeq[EHVI_CONS_MAX];
    float a[EHVI_FRONT_MAX], b[EHVI_FRONT_MAX];   // the staircase, in the minimisation sense
};
static_assert(sizeof(EhviGroup) % 4 == 0 && sizeof(EhviGroup) / 4 <= EHVI_NT, "EhviGroup: copied to LDS by one pass of the workgroup");

struct EhviArgs {
    int G, P, C, log;
    const int32_t *obj, *obj_max; const float *ref, *front; const int32_t* front_n;   // [G, 2], [G, 2] nullable, [G, 2], [G, P, 2], [G]
    const int32_t* con; const float* con_thr; const int32_t* con_geq;                 // [G, C] each
    float* stair; int32_t* stair_n;                                                   // nullable [G, P, 2], [G]
    EhviGroup* grp;                                                                   // [G]
    const float *m, *v;             // stage A: [T, L] each
    int64_t c0, L, rows;            // the chunk's first row and length; the pool's rows
    float* score;                   // nullable [G, rows]
    PmPool s;                       // the exclusion lists (per GROUP), the lists [G, chunks_max, k], top_* [G, k]
    int cpg;                        // lists in use per group: min(grid / G, chunks_max), at least 1
};

// psi(c) = E[(c - y)+], y ~ N(m, v): pm_ei for minimisation; psi(-inf) = 0.  Not inlined, as pm_log_ei and for its reason.
__device__ __noinline__ float ehvi_psi(float m, float v, float c) {
    if (c == -INFINITY) return 0.f;
    return pm_ei(m, v, c, 0);
}
// log(1 - exp(d)), d < 0: through expm1 near 0, where 1 - exp(d) cancels
__device__ __noinline__ float ehvi_log1mexp(float d) {
    return d > -0.6931472f ? logf(-expm1f(d)) : log1pf(-expf(d));
}
// log Phi(z), pm_mes_term's three-way split: log1p where Phi -> 1, as written on (-1, 0], through erfcx below (a^2 / 2 apart)
__device__ __noinline__ float ehvi_log_phi(float z) {
    if (z > 0.f) return log1pf(-0.5f * erfcf(z * 0.70710678118654752f));
    if (z > -1.f) return logf(0.5f * erfcf(-z * 0.70710678118654752f));
    const float a = -z;
    return logf(0.5f * erfcxf(a * 0.70710678118654752f)) - 0.5f * a * a;
}

// ---- one wave per group: the staircase and the group's state
__global__ __launch_bounds__(64) void k_ehvi_stair(PmArgs a, EhviArgs e) {
    const int g = blockIdx.x, lane = threadIdx.x, P = e.P, C = e.C, T = a.T;
    const int o1 = e.obj[2 * g], o2 = e.obj[2 * g + 1];
    const bool two = o2 != -1;
    bool bad = o1 < 0 || o1 >= T || (two && (o2 < 0 || o2 >= T || o2 == o1));
    const float sg1 = (e.obj_max && e.obj_max[2 * g] != 0) ? -1.f : 1.f, sg2 = (e.obj_max && e.obj_max[2 * g + 1] != 0) ? -1.f : 1.f;
    const float r1 = sg1 * e.ref[2 * g], r2 = two ? sg2 * e.ref[2 * g + 1] : 0.f;
    bad = bad || r1 != r1 || r2 != r2;
    if (!bad) bad = pm_kind_of(a, o1) < 0 || (two && pm_kind_of(a, o2) < 0);
    int ct = -1, cgeq = 0;
    float cthr = 0.f;
    for (int c = 0; c < EHVI_CONS_MAX; ++c) {
        int t = -1, q = 0;
        float thr = 0.f;
        if (c < C) {
            t = e.con[g * C + c];
            if (t != -1) {
                thr = e.con_thr[g * C + c]; q = e.con_geq[g * C + c] != 0 ? 1 : 0;
                if (t < 0 || t >= T) { bad = true; t = -1; }
                else if (thr != thr || pm_kind_of(a, t) < 0) bad = true;
            }
        }
        if (lane == c) { ct = t; cthr = thr; cgeq = q; }
    }
    // the front, turned into minimisation: NaN points and points not strictly better than r in both coordinates leave
    int n = two ? e.front_n[g] : 0;
    n = n < 0 ? 0 : (n > P ? P : n);
    float fa = 0.f, fb = 0.f;
    if (lane < n) { fa = sg1 * e.front[((size_t)g * P + lane) * 2]; fb = sg2 * e.front[((size_t)g * P + lane) * 2 + 1]; }
    const int valid = (lane < n && fa == fa && fb == fb && fa < r1 && fb < r2) ? 1 : 0;
    // weakly dominated points leave; of exact duplicates the lowest index stays
    int keep = valid;
    for (int j = 0; j < 64; ++j) {
        const float aj = __shfl(fa, j), bj = __shfl(fb, j);
        const int vj = __shfl(valid, j);
        if (vj && j != lane && aj <= fa && bj <= fb && (aj < fa || bj < fb || j < lane)) keep = 0;
    }
    // the rank by the first coordinate (distinct among the points that stay), then entry `lane` of the staircase into lane `lane`
    int rank = 0;
    for (int j = 0; j < 64; ++j) {
        const float aj = __shfl(fa, j);
        const int kj = __shfl(keep, j);
        if (kj && aj < fa) ++rank;
    }
    const int cnt = __popcll(__ballot(keep != 0));
    float ma = 0.f, mb = 0.f;
    for (int j = 0; j < 64; ++j) {
        const float aj = __shfl(fa, j), bj = __shfl(fb, j);
        const int kj = __shfl(keep, j), rj = __shfl(rank, j);
        if (kj && rj == lane) { ma = aj; mb = bj; }
    }
    EhviGroup& s = e.grp[g];
    s.a[lane] = ma; s.b[lane] = mb;
    if (lane < EHVI_CONS_MAX) { s.ct[lane] = ct; s.cthr[lane] = cthr; s.cgeq[lane] = cgeq; }
    if (lane == 0) {
        s.bad = bad ? 1 : 0; s.two = two ? 1 : 0; s.P = cnt; s.pad = 0;
        s.t[0] = o1; s.t[1] = o2; s.sg[0] = sg1; s.sg[1] = sg2; s.r[0] = r1; s.r[1] = r2;
        if (e.stair_n) e.stair_n[g] = cnt;
    }
    if (e.stair && lane < P) {   // in the caller's units and sense, zero beyond the count
        e.stair[((size_t)g * P + lane) * 2] = lane < cnt ? sg1 * ma : 0.f;
        e.stair[((size_t)g * P + lane) * 2 + 1] = lane < cnt ? sg2 * mb : 0.f;
    }
}

// ---- the scores of one chunk of the pool
__global__ __launch_bounds__(EHVI_NT) void k_ehvi_score(EhviArgs e) {
    __shared__ float pan[2][EHVI_FRONT_MAX + 1][64];   // pan[0][j]: the edge a_(j+1) (j = P: r1); pan[1][j]: the edge b_j (j = 0: r2)
    __shared__ float red[4][64];                       // the four partials of a row
    __shared__ float pcon[EHVI_CONS_MAX][64];          // Phi(z_c) (log form: log Phi) of a row
    __shared__ EhviGroup gs;
    const int tid = threadIdx.x, row = tid & 63, part = tid >> 6;
    const int G = e.G, grid = gridDim.x, k = e.s.k, lg = e.log;
    const int chunk = blockIdx.x / G;
    if (chunk >= e.cpg) return;   // (uniform)
    const int64_t ntiles = (e.L + 63) / 64;
    const float nan = __builtin_nanf("");
    for (int g = blockIdx.x % G; g < G; g += grid) {
        if (tid < (int)(sizeof(EhviGroup) / 4)) reinterpret_cast<int*>(&gs)[tid] = reinterpret_cast<const int*>(e.grp + g)[tid];
        __syncthreads();
        // the list of (group, walker) so far: empty at the first chunk (the host fills the indices with -1)
        float lv = -INFINITY;
        long long li = -1;
        if (k > 0 && tid < k) {
            const size_t q = ((size_t)g * e.s.chunks_max + chunk) * k + tid;
            li = e.s.cand_idx[q];
            lv = li >= 0 ? e.s.cand_val[q] : -INFINITY;
        }
        const int bad = gs.bad, two = gs.two, P = gs.P;
        const int n1 = P + 1, ne = two ? 2 * n1 : n1;   // edges of the first objective; all edges
        for (int64_t tile = chunk; tile < ntiles; tile += e.cpg) {
            const int64_t r0 = tile * 64;
            const int m = (int)(e.L - r0 < 64 ? e.L - r0 : 64);
            const size_t out = (size_t)g * (size_t)e.rows + (size_t)(e.c0 + r0 + row);
            if (bad) {   // (uniform)
                if (e.score && tid < m) e.score[out] = nan;
                continue;
            }
            const bool in = row < m;
            if (in) {
                const size_t q1 = (size_t)gs.t[0] * (size_t)e.L + (size_t)(r0 + row);
                const float m1 = gs.sg[0] * e.m[q1], v1 = e.v[q1];
                float m2 = 0.f, v2 = 0.f;
                if (two) { const size_t q2 = (size_t)gs.t[1] * (size_t)e.L + (size_t)(r0 + row); m2 = gs.sg[1] * e.m[q2]; v2 = e.v[q2]; }
                for (int q = part; q < ne; q += 4) {
                    const bool first = q < n1;
                    const int j = first ? q : q - n1;
                    const float c = first ? (j < P ? gs.a[j] : gs.r[0]) : (j == 0 ? gs.r[1] : gs.b[j - 1]);
                    const float mm = first ? m1 : m2, vv = first ? v1 : v2;
                    pan[first ? 0 : 1][j][row] = lg ? pm_log_ei(mm, vv, c, 0) : ehvi_psi(mm, vv, c);
                }
                // constraint `part` of the row
                float pc = lg ? -0.f : 1.f;
                const int t = gs.ct[part];
                if (t >= 0) {
                    const size_t qc = (size_t)t * (size_t)e.L + (size_t)(r0 + row);
                    const float mc = e.m[qc], sc = sqrtf(fmaxf(e.v[qc], 1e-12f)), thr = gs.cthr[part];
                    const float z = (gs.cgeq[part] ? (mc - thr) : (thr - mc)) / sc;
                    pc = lg ? ehvi_log_phi(z) : 0.5f * erfcf(-z * 0.70710678118654752f);
                }
                pcon[part][row] = pc;
            }
            __syncthreads();
            float score = 0.f;
            if (!lg) {
                if (in) {
                    float sum = -0.f;   // the identity that keeps the sign of a zero term: a lone strip's bits pass through the sums
                    for (int i = part; i < n1; i += 4) {
                        const float w = i > 0 ? pan[0][i][row] - pan[0][i - 1][row] : pan[0][0][row];
                        sum = two ? fmaf(w, pan[1][i][row], sum) : sum + w;
                    }
                    red[part][row] = sum;
                }
                __syncthreads();
                if (tid < m) {
                    const float ehvi = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
                    float pof = 1.f;
                    for (int c = 0; c < EHVI_CONS_MAX; ++c) pof *= pcon[c][tid];
                    score = ehvi * pof;
                }
            } else {
                // a strip's term, in the place of its second factor (read by this strip only); then the maximum
                float mx = -INFINITY;
                if (in) {
                    for (int i = part; i < n1; i += 4) {
                        const float hi = pan[0][i][row];
                        float w = hi;
                        if (i > 0 && hi != -INFINITY) {
                            const float d = pan[0][i - 1][row] - hi;
                            w = d >= 0.f ? -INFINITY : hi + ehvi_log1mexp(d);
                        }
                        const float term = two ? w + pan[1][i][row] : w;
                        pan[1][i][row] = term;
                        mx = fmaxf(mx, term);
                    }
                    red[part][row] = mx;
                }
                __syncthreads();
                if (in) mx = fmaxf(fmaxf(fmaxf(red[0][row], red[1][row]), red[2][row]), red[3][row]);
                __syncthreads();
                if (in) {
                    float sum = 0.f;
                    for (int i = part; i < n1; i += 4) {
                        const float term = pan[1][i][row];
                        if (term != -INFINITY) sum += expf(term - mx);
                    }
                    red[part][row] = sum;
                }
                __syncthreads();
                if (tid < m) {
                    const float sum = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
                    const float lehvi = sum == 0.f ? -INFINITY : mx + logf(sum);
                    float lp = -0.f;
                    for (int c = 0; c < EHVI_CONS_MAX; ++c) lp += pcon[c][tid];
                    score = lehvi + lp;
                }
            }
            if (e.score && tid < m) e.score[out] = score;
            if (k > 0 && part == 0)
                pm_list_merge(lv, li, k, score, (long long)(e.c0 + r0 + tid), tid < m, [&](long long r) { return pm_excluded(e.s, g, r); });
            __syncthreads();   // the panels and the partials are rewritten by the next tile
        }
        if (k > 0) pm_list_store(e.s, g, chunk, tid, k, lv, li);
        __syncthreads();   // gs is rewritten by the next group
    }
}

// ---- one wave per group: the group's lists merged under the total order, top_idx / top_val [G, k] (nothing listed: -1 / -inf)
__global__ __launch_bounds__(64) void k_ehvi_topk(EhviArgs e) {
    pm_group_topk(e.s, blockIdx.x, e.rows > 0 ? e.cpg : 0);
}

}  // namespace adkf
