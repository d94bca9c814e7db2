// Host side of the GP pipeline: the workspace and its carve, the distance stage, the inner fit (register-resident and blocked),
// the float64 path of ill-conditioned tasks, the outer / hypergradient pipeline and prediction on a query block.
#pragma once
#include "host_common.h"

namespace {

// Feature dimensions below one K chunk stay on the FP32 form: nothing to gain there (the chunk is mostly padding), and the stress
// suite's low-dimensional clustered tasks (d = 2, 3: cond 2e2 .. 6e2, where the float32 restatement of the reference itself is
// 1e-4 .. 3e-4 from float64) keep the arithmetic their tolerances were measured with.
inline bool x3_for(int d) { return d >= GK; }

struct Workspace {
    float *mean, *D2ss, *D2qs, *D2qq, *Ainv, *P, *C, *S, *OC, *Wss, *Wqs, *Wqq, *vecs, *scal, *part_oc, *part_ma, *l0;
    // blocked path only (max(ns, nq) > REG_POINTS)
    float *lg_Dinv, *lg_C, *lg_F, *lg_logdet, *lg_part, *lg_pext;   // lg_Dinv: [2, T, LB, LB] (the fused block step alternates between the two)
    int32_t *lg_info, *lg_med, *lg_cnt;  // lg_med: prefix[T], rank[T], hist[T, 256]; lg_cnt: [T] arrival counters of large_fused.h
    FitShared* lg_fit;
    double* w64; size_t w64_stride;   // float64 region of the ill-conditioned-task path (refine64.h); null beyond R64_MAXN points
    int vld, nt_oc, nt_ma;
    int lg_mode;       // ADKF_BATCH_LG_UNFUSED / ADKF_BATCH_LG_FUSED of the batch this view was carved for: -1 three launches, +1 fused, 0 by size
    size_t bytes;
};

Workspace carve(void* base, int T, int ns, int nq, int d) {
    Workspace w{};   // (the regions a shape does not have stay null, lg_mode 0)
    Arena ar{static_cast<char*>(base), 0};
    const size_t Tz = (size_t)T;
    w.vld = ns > nq ? ns : nq;
    w.nt_oc = nq > 0 ? tiles_of(nq, ns) : 0;   // per-tile partial reductions of ProbOC / ProbMA
    w.nt_ma = tiles_of(ns, ns);
    w.mean = ar.floats(Tz * d);
    w.D2ss = ar.floats(Tz * ns * ns);
    w.D2qs = ar.floats(Tz * nq * ns);
    w.D2qq = ar.floats(Tz * nq * nq);
    w.Ainv = ar.floats(Tz * ns * ns);
    w.P = ar.floats(Tz * ns * ns);
    w.C = ar.floats(Tz * nq * ns);
    w.S = ar.floats(Tz * nq * nq);
    w.OC = ar.floats(Tz * nq * ns);
    w.Wss = ar.floats(Tz * ns * ns);
    w.Wqs = ar.floats(Tz * nq * ns);
    w.Wqq = ar.floats(Tz * nq * nq);
    w.vecs = ar.floats(Tz * NVEC * w.vld);
    w.scal = ar.floats(Tz * NSCAL);
    w.part_oc = ar.floats(Tz * (w.nt_oc > 0 ? w.nt_oc : 1) * 4);
    w.part_ma = ar.floats(Tz * w.nt_ma * 4);
    w.l0 = ar.floats(Tz);
    if (w.vld > REG_POINTS) {
        w.lg_Dinv = ar.floats(2 * Tz * LB * LB);
        w.lg_C = ar.floats(Tz * LB * w.vld);
        w.lg_F = ar.floats(Tz * LB * w.vld);
        w.lg_logdet = ar.floats(Tz);
        w.lg_pext = ar.floats(Tz * 2);
        const size_t tq = (size_t)((nq + GT - 1) / GT) * ((nq + GT - 1) / GT);
        const size_t ts = (size_t)((ns + GT - 1) / GT) * ((ns + GT - 1) / GT);
        w.lg_part = ar.floats(Tz * (ts > tq ? ts : tq) * 8);
        w.lg_info = ar.as<int32_t>(Tz);
        w.lg_cnt = ar.as<int32_t>(Tz);
        w.lg_med = ar.as<int32_t>(Tz * 258);
        static_assert(sizeof(FitShared) % sizeof(float) == 0, "FitShared is carved as whole floats");
        w.lg_fit = ar.as<FitShared>(Tz);
    }
    // the float64 region of refine64.h is carved for EVERY task (any of them may turn out ill-conditioned): 8 refine64_doubles(ns, nq)
    // bytes per task - 1.3 MB at 128 points, 5.2 MB at 256, 82 MB at 1024 (1.7 x the float32 part of the workspace); r64_maxn() is the
    // largest batch that gets one
    if (w.vld <= r64_maxn()) {
        w.w64_stride = refine64_doubles(ns, nq);
        w.w64 = ar.as<double>(Tz * w.w64_stride);
    }
    w.bytes = ar.off;
    return w;
}

Workspace carve_for(const adkf_batch_t* b, void* ws) {
    Workspace w = carve(ws, b->T, b->ns_max, b->nq_max, b->d);
    w.lg_mode = (b->flags & ADKF_BATCH_LG_UNFUSED) ? -1 : (b->flags & ADKF_BATCH_LG_FUSED) ? 1 : 0;
    return w;
}

int check_batch(const adkf_batch_t* b, bool need_query) {
    (void)hipGetLastError();  // a stale error left by another library on this thread must not be blamed on our launches
    if (!b || b->T <= 0 || b->ns_max <= 0 || b->d <= 0 || !b->Z_s) return ADKF_E_BADARG;
    if (b->kernel != ADKF_KERNEL_RBF && b->kernel != ADKF_KERNEL_MATERN52) return ADKF_E_BADARG;
    if (b->ns_max > MAX_POINTS) return ADKF_E_SIZE;
    if (need_query) {
        if (b->nq_max <= 0 || !b->Z_q) return ADKF_E_BADARG;
        if (b->nq_max > MAX_POINTS) return ADKF_E_SIZE;
    }
    return 0;
}

// 16-byte vector loads are legal when every leading dimension is a multiple of 4 floats and every base is aligned
// (the workspace carve keeps 256-byte alignment; per-task offsets are then multiples of 16 bytes too).
bool vec_ok(const adkf_batch_t* b, const Workspace& w) {
    if ((b->ns_max & 3) || (b->nq_max & 3) || (b->d & 3) || (w.vld & 3)) return false;
    return aligned16(b->Z_s) && aligned16(b->Z_q) && aligned16(w.mean);
}

TaskView make_tv(const adkf_batch_t* b, const Workspace& w, bool with_query) {
    TaskView tv;
    tv.n_s = b->n_s; tv.n_q = with_query ? b->n_q : nullptr;
    tv.ns_ld = b->ns_max; tv.nq_ld = with_query ? b->nq_max : 0; tv.vld = w.vld; tv.kind = b->kernel;
    tv.scal = w.scal; tv.vecs = w.vecs;
    tv.vec = vec_ok(b, w);
    return tv;
}

inline bool has_query(const adkf_batch_t* b) { return b->nq_max > 0 && b->Z_q != nullptr; }
inline bool is_ard(const adkf_batch_t* b) { return (b->flags & ADKF_BATCH_ARD) != 0; }

// Stage A: centring, squared distances.  Skipped when the caller promises (ADKF_BATCH_REUSE_DIST) that
// this workspace already holds them for exactly this batch.
// parts: 1 = the support block (mean, norms, D2ss), 2 = the query blocks (needs the support mean / norms in place),
// 4 = the features are already centred and w.mean holds zeros (ARD: Z~ = (Z - mu) / l has zero column mean by construction).
// (The squared row norms are summed inside the distance GEMM while it stages its operands: no separate pass.)
//
// Fast path (dist_task.h: one workgroup per task, every row loaded, centred and split once; bit-identical to the generic launch; for
// adkf_median_lengthscale / adkf_init_params the median select and the initialisation ride in the same launch): a FULL
// batch of 128 support and 128 query points - parts == 3 with a query set, ns_max == nq_max == 128, no n_s and no n_q, d a multiple of
// the K chunk (which implies x3_for(d)), 16-byte loads legal (vec_ok), the LDS opt-in granted, no REUSE_DIST.  Every other batch
// (ragged, other sizes, support only, ARD's parts bits, other d, misaligned Z) keeps the generic launch.
bool use_dist_task(const adkf_batch_t* b, const Workspace& w, bool with_query, int parts) {
    static const bool optin = lds_optin(DT_LDS_BYTES, {kernel_ptr(&k_dist_task<false>), kernel_ptr(&k_dist_task<true>)});
    // (d <= 2^22: the kernel's 32-bit byte offsets inside a task's block of 64 rows)
    return optin && parts == 3 && with_query && b->ns_max == DT_N && b->nq_max == DT_N && !b->n_s && !b->n_q && (b->d % GK) == 0 &&
           b->d <= (1 << 22) && vec_ok(b, w);
}

// l0 / init / selected (median_core): the median heuristic the caller wants next.  The fast path runs it inside its launch (l0[t], and
// init_params_task when init->phi is set) and says so through *selected; every other way out leaves it to k_median.
int stage_dist(const adkf_batch_t* b, const Workspace& w, bool with_query, hipStream_t st, int parts = 3, float* l0 = nullptr,
               const InitArgs* init = nullptr, bool* selected = nullptr) {
    if (selected) *selected = false;
    if (b->flags & ADKF_BATCH_REUSE_DIST) return 0;
    const int T = b->T, ns = b->ns_max, nq = with_query ? b->nq_max : 0, d = b->d;
    if (!(parts & 2)) with_query = false;
    if ((parts & 1) && !(parts & 4)) k_colmean<<<dim3(ceil_div(d, 64), T), 256, 0, st>>>(b->Z_s, b->n_s, ns, d, w.mean, T);
    if (use_dist_task(b, w, with_query, parts)) {
        const DistTaskArgs a{b->Z_s, b->Z_q, w.mean, w.D2ss, w.D2qs, w.D2qq, d, T, l0, init ? *init : InitArgs{0, 0, nullptr, nullptr}};
        if (l0 && selected) k_dist_task<true><<<grid_for(T, 1), DT_NT, DT_LDS_BYTES, st>>>(a);
        else k_dist_task<false><<<grid_for(T, 1), DT_NT, DT_LDS_BYTES, st>>>(a);
        LAUNCH_OK();
        if (l0 && selected) *selected = true;
        return 0;
    }
    ProbDist p;
    p.mean = w.mean; p.d = d; p.vec = vec_ok(b, w);
    ProbDistMulti pm;
    pm.vec = p.vec; pm.end0 = pm.end1 = 0; pm.tn0 = pm.tn1 = pm.tn2 = 1;
    int nblk = 0, total = 0;
    auto add = [&](const ProbDist& q, int M, int N) {
        const int tn = ceil_div(N, GT), tiles = ceil_div(M, GT) * tn;
        if (nblk == 0) { pm.s0 = q; pm.tn0 = tn; pm.end0 = pm.end1 = total + tiles; pm.s1 = pm.s2 = q; }
        else if (nblk == 1) { pm.s1 = q; pm.tn1 = tn; pm.end1 = total + tiles; pm.s2 = q; }
        else { pm.s2 = q; pm.tn2 = tn; }
        total += tiles; ++nblk;
    };
    if (parts & 1) {
        p.X = b->Z_s; p.Y = b->Z_s; p.n_x = b->n_s; p.n_y = b->n_s; p.x_ld = ns; p.y_ld = ns; p.symmetric = true; p.D2 = w.D2ss;
        add(p, ns, ns);
    }
    if (with_query) {
        p.X = b->Z_q; p.Y = b->Z_s; p.n_x = b->n_q; p.n_y = b->n_s; p.x_ld = nq; p.y_ld = ns; p.symmetric = false; p.D2 = w.D2qs;
        add(p, nq, ns);
        p.X = b->Z_q; p.Y = b->Z_q; p.n_x = b->n_q; p.n_y = b->n_q; p.x_ld = nq; p.y_ld = nq; p.symmetric = true; p.D2 = w.D2qq;
        add(p, nq, nq);
    }
    if (nblk > 0) {
        if (x3_for(d)) k_bgemm3<ProbDistMulti, GT, 256><<<grid_for(T, total), 256, 0, st>>>(pm, T, 1, total);
        else k_bgemm<ProbDistMulti, GT><<<grid_for(T, total), 256, 0, st>>>(pm, T, 1, total);
    }
    LAUNCH_OK();
    return 0;
}

template <int NMAX, int NT, bool LOW>
void launch_inner_kl(const InnerArgs& a, hipStream_t st) {
    constexpr size_t cache_bytes = sizeof(float) * NMAX * NMAX;   // the kappa' u cache of inner.h (one float per matrix element), or D^2 (LOW)
    // 64 KB of dynamic LDS on top of the static part needs the opt-in (a refusal shows as the launch's own error)
    static const bool optin = lds_optin(cache_bytes, {kernel_ptr(&k_inner<NMAX, NT, 0, LOW>), kernel_ptr(&k_inner<NMAX, NT, 1, LOW>)});
    (void)optin;
    if (a.kind == ADKF_KERNEL_RBF) k_inner<NMAX, NT, 0, LOW><<<grid_for(a.T, 1), NT, cache_bytes, st>>>(a);
    else k_inner<NMAX, NT, 1, LOW><<<grid_for(a.T, 1), NT, cache_bytes, st>>>(a);
}

// The two-tasks-per-CU variant of the 128-point fit is taken when the batch has more tasks than the chip has CUs (up to that every
// task has a CU to itself and the resident variant is 20 % faster; beyond it the resident variant needs a second round of
// workgroups, the low-register one runs two tasks per CU side by side)
template <int NMAX, int NT>
void launch_inner_k(const InnerArgs& a, hipStream_t st) {
    if constexpr (NMAX == 128) {
        if (a.T > num_cus()) { launch_inner_kl<NMAX, NT, true>(a, st); return; }
    }
    launch_inner_kl<NMAX, NT, false>(a, st);
}

// The update of block step k and the sweep of block step k + 1 share a launch (large_fused.h) from four block steps on
// (tools/lgf_bench.hip, profiles/r05_lgf_bench.txt: 8 x 1024 points 0.85 x the time of the three launches, 16 x 1024 0.90 x; but
// 64 x 256, 5 x 515 and 3 x 300 points 1.06 - 1.10 x: with two or three block steps the sweep that rides in the update launch is
// most of that launch)
inline bool lg_fused_by_size(int ld) { return ld >= 4 * LB; }

LgMat lg_mat(const Workspace& w, float* M, int ld, const int32_t* n_arr, const FitShared* fit, int T) {
    LgMat m;
    m.M = M; m.ld = ld; m.n_arr = n_arr; m.fit = fit;
    m.Dinv = w.lg_Dinv; m.Cbuf = w.lg_C; m.Fbuf = w.lg_F; m.logdet = w.lg_logdet; m.pext = w.lg_pext; m.info = w.lg_info;
    const bool fused = w.lg_mode > 0 || (w.lg_mode == 0 && lg_fused_by_size(ld));
    m.cnt = fused ? w.lg_cnt : nullptr;
    m.T = T; m.vec = (ld & 3) == 0;
    return m;
}

// M -> -(M^-1) in place by 128-pivot block steps (large.h; large_fused.h)
void lg_sweep(const LgMat& m0, hipStream_t st) {
    const int nb = ceil_div(m0.ld, LB), tn = ceil_div(m0.ld, GT);
    LgMat m = m0;
    if (m.cnt) {
        // D(0) | P(0) | U(0) + D(1) | P(1) | U(1) + D(2) | ... | P(nb - 1) | U(nb - 1): 2 nb + 1 launches instead of 3 nb
        float* dinv[2] = {m0.Dinv, m0.Dinv + (size_t)m0.T * LB * LB};
        const int npair = lgf_npair(tn);
        k_lg_diag<<<grid_for(m.T, 1), 512, 0, st>>>(m, 0);
        for (int step = 0; step < nb; ++step) {
            m.Dinv = dinv[step & 1];
            ProbLgPanel pp; pp.m = m; pp.step = step;
            k_bgemm<ProbLgPanel><<<grid_for(m.T, 2 * tn), 256, 0, st>>>(pp, m.T, 2, tn);
            LgStepArgs sa{m, dinv[(step + 1) & 1], m.cnt, step, tn, npair, step + 1 < nb ? 1 : 0};
            k_lg_update_sweep<<<grid_for(m.T, npair), LGF_NT, 0, st>>>(sa);
        }
        return;
    }
    for (int step = 0; step < nb; ++step) {
        k_lg_diag<<<grid_for(m.T, 1), 512, 0, st>>>(m, step);
        ProbLgPanel pp; pp.m = m; pp.step = step;
        k_bgemm<ProbLgPanel><<<grid_for(m.T, 2 * tn), 256, 0, st>>>(pp, m.T, 2, tn);
        ProbLgUpdate pu; pu.m = m; pu.step = step; pu.tri = tn * (tn + 1) / 2;   // workgroups for the tiles on or above the diagonal only
        k_bgemm<ProbLgUpdate><<<grid_for(m.T, pu.tri), 256, 0, st>>>(pu, m.T, tn, tn);
    }
}

// Convergence-mode early exit for the fits that are a sequence of launches (blocked path, ARD): every POLL_EVERY
// evaluations the number of unfinished tasks goes to pinned host memory and the stream is synchronised, so a fit that
// converges after 15 evaluations does not enqueue the other 185 rounds of (skipped) kernels.  Never in exact-evals mode
// (deterministic work, no synchronisation) and never while the stream is being captured into a graph.
constexpr int POLL_EVERY = 8;

__global__ void k_count_unfinished(const char* base, size_t stride, size_t phase_offset, int T, int done_value, int32_t* out) {
    int c = 0;
    for (int t = threadIdx.x; t < T; t += blockDim.x) c += *reinterpret_cast<const int*>(base + (size_t)t * stride + phase_offset) != done_value;
    c = wave_sum_i(c);
    if (threadIdx.x == 0) *out = c;
}

struct FitPoll {
    bool enabled = false;
    int32_t* host = nullptr;
    int32_t* dev;
    FitPoll(bool convergence_mode, int max_evals, int32_t* dev_counter, hipStream_t st) : dev(dev_counter) {
        if (!convergence_mode || max_evals <= 2 * POLL_EVERY) return;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return;
        thread_local int32_t* pinned = nullptr;
        if (!pinned && hipHostMalloc(reinterpret_cast<void**>(&pinned), sizeof(int32_t), hipHostMallocDefault) != hipSuccess) return;
        host = pinned;
        enabled = true;
    }
    // true when every task has finished (call after the advance kernel of evaluation e).  every_after: once POLL_EVERY rounds are
    // through, poll every that many (the CG loop: a round of empty launches costs more than a poll once most tasks have converged)
    bool finished(int e, const void* state, size_t stride, size_t phase_offset, int T, hipStream_t st, int done_value = PH_DONE, int every_after = POLL_EVERY) {
        if (!enabled) return false;
        if (e + 1 < POLL_EVERY || (e + 1 - POLL_EVERY) % every_after != 0) return false;
        k_count_unfinished<<<1, 64, 0, st>>>(static_cast<const char*>(state), stride, phase_offset, T, done_value, dev);
        if (hipMemcpyAsync(host, dev, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess) return false;
        if (hipStreamSynchronize(st) != hipSuccess) return false;
        return *host == 0;
    }
};

int launch_inner_large(const InnerArgs& a, const Workspace& w, hipStream_t st) {
    LgInner li;
    li.in = a; li.fit = w.lg_fit; li.part = w.lg_part;
    li.tiles_1d = ceil_div(a.ld, GT); li.ntiles = li.tiles_1d * li.tiles_1d;
    li.mat = lg_mat(w, a.Ainv, a.ld, a.n_s, w.lg_fit, a.T);
    LgMatvecArgs mv{li.mat, a.y_s, (size_t)a.ld, a.vecs + (size_t)V_ALPHA * a.vld, (size_t)NVEC * a.vld, -1.f};
    k_lg_begin<<<ceil_div(a.T, 64), 64, 0, st>>>(li);
    const int n_evals = a.max_evals > 0 ? a.max_evals : 1;
    FitPoll poll(a.max_evals > 0 && !a.exact_evals, a.max_evals, w.lg_info, st);   // lg_info[0] is free between block sweeps
    for (int e = 0; e < n_evals; ++e) {
        k_lg_build<<<grid_for(a.T, li.ntiles), 256, 0, st>>>(li);
        lg_sweep(li.mat, st);
        k_lg_matvec<<<dim3(ceil_div(a.ld, 4), a.T), 256, 0, st>>>(mv);
        k_lg_traces<<<grid_for(a.T, li.ntiles), 256, 0, st>>>(li);
        k_lg_advance<<<a.T, 256, 0, st>>>(li);
        if (poll.finished(e, w.lg_fit, sizeof(FitShared), offsetof(FitShared, phase), a.T, st)) break;
    }
    LAUNCH_OK();
    return 0;
}

// Stage B (and the fit): dispatch on the padded support size.
int launch_inner(InnerArgs a, const Workspace& w, hipStream_t st) {
    if (a.ld > REG_POINTS) return launch_inner_large(a, w, st);
    if (a.ld <= 16) launch_inner_k<16, 256>(a, st);
    else if (a.ld <= 32) launch_inner_k<32, 256>(a, st);
    else if (a.ld <= 64) launch_inner_k<64, 256>(a, st);
    else launch_inner_k<128, 512>(a, st);
    LAUNCH_OK();
    return 0;
}

void launch_alpha_refine(const TaskView& tv, const adkf_batch_t* b, const Workspace& w, hipStream_t st) {
    AlphaRefineArgs aa{tv, w.Ainv, w.D2ss, b->y_s, w.vecs, refine32_threshold(), b->T};
    k_alpha_refine<<<grid_for(b->T, 1), SMALL_NT, 0, st>>>(aa);
}

// C = K_qs A^-1 followed, for the tasks that need it, by one refinement step (R lives in w.OC, which ProbOC fills later)
void launch_c(const TaskView& tv, const adkf_batch_t* b, const Workspace& w, hipStream_t st) {
    const int T = b->T, ns = b->ns_max, nq = b->nq_max;
    ProbC pc; pc.tv = tv; pc.Ainv = w.Ainv; pc.D2qs = w.D2qs; pc.C = w.C;
    launch_gemm(pc, T, nq, ns, st);
    ProbCres pr; pr.tv = tv; pr.C = w.C; pr.D2ss = w.D2ss; pr.D2qs = w.D2qs; pr.R = w.OC; pr.thresh = refine32_threshold();
    launch_gemm(pr, T, nq, ns, st);
    ProbCfix pf; pf.tv = tv; pf.R = w.OC; pf.Ainv = w.Ainv; pf.C = w.C; pf.thresh = refine32_threshold();
    launch_gemm(pf, T, nq, ns, st);
}

bool refine64_lds_optin() {
    // up to R64_LDS_POINTS points the float64 inverses run in LDS: 128 KB of dynamic shared memory (one workgroup per CU then; the
    // kernels are a two-scalar test for everybody but the flagged tasks).  Without the opt-in the inverses work in global memory.
    static const bool ok = lds_optin(sizeof(double) * R64_LDS_POINTS * R64_LDS_POINTS, {kernel_ptr(&k_refine64), kernel_ptr(&k_tail64)});
    return ok;
}

Refine64Args refine_args(const TaskView& tv, const adkf_batch_t* b, const Workspace& w, bool with_hessian, int level, float* f_out,
                         int32_t* info, float* f_in, float* g_in, float* gnorm, size_t& lds_bytes) {
    const bool lds_inv = refine64_lds_optin();   // (beyond R64_LDS_POINTS the diagonal blocks of the blocked inverse live there)
    // (always the full R64_LDS_POINTS^2 doubles - 128 KB: the staged products of refine64.h work in blocks of that edge whatever the
    // batch size; one workgroup per CU, which is what this path runs at anyway)
    lds_bytes = lds_inv ? sizeof(double) * (size_t)R64_LDS_POINTS * R64_LDS_POINTS : 0;
    return Refine64Args{tv, b->Z_s, b->Z_q, b->d, b->y_s, b->y_q, b->priors, w.Ainv, with_hessian ? w.P : nullptr, level >= 1 ? w.C : nullptr,
                        level >= 2 ? w.S : nullptr, w.vecs, w.scal, f_out, info, f_in, g_in, gnorm, w.w64, w.w64_stride, r64_threshold(), b->T,
                        with_hessian ? 1 : 0, level, lds_inv ? 1 : 0};
}

// Ill-conditioned tasks redo the factorisation-type stages in float64 (refine64.h); everybody else leaves the kernel after
// reading two scalars.  level: 0 = inner quantities (A^-1, alpha, scalars), 1 = + C, mu (prediction).  (Level 2 - + S^-1, e, f_out -
// runs inside k_tail64 at the end of the hypergradient pipeline.)
void launch_refine(const TaskView& tv, const adkf_batch_t* b, const Workspace& w, bool with_hessian, int level, float* f_out,
                   int32_t* info, hipStream_t st, float* f_in = nullptr, float* g_in = nullptr, float* gnorm = nullptr) {
    if (!w.w64) return;
    size_t lds_bytes;
    const Refine64Args ra = refine_args(tv, b, w, with_hessian, level, f_out, info, f_in, g_in, gnorm, lds_bytes);
    k_refine64<<<b->T, R64_NT, lds_bytes, st>>>(ra);
}

// max(support, query) <= 128: the outer / hypergradient stage of a task runs as ONE workgroup (hyper.h).  The sixteen-launch
// pipeline takes the larger batches, and every batch on a device that refuses the LDS opt-in.
bool use_fused_outer(int ns, int nq) {
    // (the small shapes - C1, 16 / 32 / 64-shot tasks - go through the ragged instance too: one launch instead of sixteen)
    static const bool optin = lds_optin(HY_LDS_BYTES, {kernel_ptr(&k_hyper<true, 0>), kernel_ptr(&k_hyper<true, 1>),
                                                       kernel_ptr(&k_hyper<false, 0>), kernel_ptr(&k_hyper<false, 1>)});
    const int hi = ns > nq ? ns : nq;
    return optin && hi >= 1 && hi <= HY_N;
}

int launch_outer_factor(const OuterArgs& a, const Workspace& w, int nq, hipStream_t st) {
    if (nq > REG_POINTS) {
        k_lg_resid<<<dim3(ceil_div(nq, 4), a.T), 256, 0, st>>>(a);
        LgMat m = lg_mat(w, a.S, a.tv.nq_ld, a.tv.n_q, nullptr, a.T);
        lg_sweep(m, st);
        LgMatvecArgs mv{m, a.vecs + (size_t)V_R * a.tv.vld, (size_t)NVEC * a.tv.vld, a.vecs + (size_t)V_E * a.tv.vld, (size_t)NVEC * a.tv.vld, -1.f};
        k_lg_matvec<<<dim3(ceil_div(nq, 4), a.T), 256, 0, st>>>(mv);
        const int tn = ceil_div(nq, GT);
        k_lg_negate<<<grid_for(a.T, tn * tn), 256, 0, st>>>(m, tn);
        LgColsumArgs cs{a.C, a.tv.ns_ld, (size_t)a.tv.nq_ld * a.tv.ns_ld, a.tv.n_q, a.tv.nq_ld, a.tv.n_s, a.tv.ns_ld,
                        a.vecs + (size_t)V_E * a.tv.vld, (size_t)NVEC * a.tv.vld, a.vecs + (size_t)V_CTE * a.tv.vld, (size_t)NVEC * a.tv.vld};
        k_lg_colsum<<<dim3(ceil_div(a.tv.ns_ld, 64), a.T), 1024, 0, st>>>(cs);
        LgOuterFin fin{a, w.lg_logdet, w.lg_info, w.lg_pext};
        k_lg_outer_fin<<<a.T, 64, 0, st>>>(fin);
        LAUNCH_OK();
        return 0;
    }
    if (nq <= 16) k_outer_factor<16, 256><<<grid_for(a.T, 1), 256, 0, st>>>(a);
    else if (nq <= 32) k_outer_factor<32, 256><<<grid_for(a.T, 1), 256, 0, st>>>(a);
    else if (nq <= 64) k_outer_factor<64, 256><<<grid_for(a.T, 1), 256, 0, st>>>(a);
    else k_outer_factor<128, 512><<<grid_for(a.T, 1), 512, 0, st>>>(a);
    LAUNCH_OK();
    return 0;
}


InnerArgs inner_args(const adkf_batch_t* b, const Workspace& w, float* phi, int32_t* info) {
    InnerArgs a{};
    a.D2ss = w.D2ss; a.y_s = b->y_s; a.n_s = b->n_s; a.phi = phi; a.priors = b->priors;
    a.Ainv = w.Ainv; a.vecs = w.vecs; a.scal = w.scal; a.info = info;
    a.T = b->T; a.ld = b->ns_max; a.vld = w.vld; a.kind = b->kernel;
    a.max_evals = 0; a.exact_evals = 0; a.gtol = 0.f; a.ftol = 0.f;
    return a;
}

// Stage B at phi - unless the batch says (ADKF_BATCH_REUSE_INNER) that this workspace holds it already.  info[] is then zeroed
// for the callers none of whose later kernels writes it (zero_info_on_reuse).
int inner_stage(const adkf_batch_t* b, const Workspace& w, const float* phi, int32_t* info, bool zero_info_on_reuse, hipStream_t st) {
    if (!(b->flags & ADKF_BATCH_REUSE_INNER)) return launch_inner(inner_args(b, w, const_cast<float*>(phi), info), w, st);
    if (zero_info_on_reuse) hipMemsetAsync(info, 0, sizeof(int32_t) * (size_t)b->T, st);
    return 0;
}

// dL/dZ of a full batch in one launch (dz_task.h: one workgroup per task, bit-identical to the two tiled launches on the BF16 pipe):
// use_dist_task's conditions on the shape - ns_max == nq_max == 128, no n_s and no n_q, d a multiple of the K chunk, 16-byte loads legal,
// the LDS opt-in granted - with both cotangents requested in 16-byte aligned rows, and no ADKF_BATCH_DZ_TILED.
bool dz_task_ok(const adkf_batch_t* b, const Workspace& w, const float* dZ_s, const float* dZ_q) {
    static const bool optin = lds_optin(DT_LDS_BYTES, {kernel_ptr(&k_dz_task)});
    // (d <= 2^22: a lane offset of 100 d bytes fits 32 bits)
    return optin && dZ_s && dZ_q && !(b->flags & ADKF_BATCH_DZ_TILED) && b->ns_max == DT_N && b->nq_max == DT_N && !b->n_s && !b->n_q &&
           (b->d % GK) == 0 && b->d <= (1 << 22) && vec_ok(b, w) && aligned16(dZ_s) && aligned16(dZ_q);
}

// Stage D..G shared by adkf_outer_nll_value_grad (with_hessian = false) and adkf_ift_hypergrad.
int outer_pipeline(const adkf_batch_t* b, const Workspace& w, const float* phi, int flags, bool with_hessian, float* f_out,
                   float* dZ_s, float* dZ_q, float* g_phi_out, float* v_out, float* H_out, int32_t* info, hipStream_t st) {
    const int T = b->T, ns = b->ns_max, nq = b->nq_max, d = b->d;
    int rc = stage_dist(b, w, true, st);
    if (rc) return rc;
    const bool reuse_inner = (b->flags & ADKF_BATCH_REUSE_INNER) != 0;
    rc = inner_stage(b, w, phi, info, false, st);   // (reused: info[] is written by k_hyper / the outer factor below)
    if (rc) return rc;
    TaskView tv = make_tv(b, w, true);
    const int tms = ceil_div(ns, GT), tmq = ceil_div(nq, GT);
    const float dirscale = (flags & ADKF_IGNORE_DIRECT_GRAD) ? 0.f : 1.f;
    const float corrscale = (with_hessian && !(flags & ADKF_IGNORE_GRAD_CORRECTION)) ? 1.f : 0.f;
    if (use_fused_outer(ns, nq)) {
        // (reused inner stage: A^-1, alpha and the scalars of phi are in the workspace, info[] is written by this kernel)
        HyperArgs ha{tv, w.Ainv, w.D2ss, w.D2qs, w.D2qq, b->y_s, b->y_q, b->priors, w.Wss, w.Wqs, w.Wqq, w.vecs, w.scal, f_out, info,
                     g_phi_out, v_out, H_out, T, reuse_inner ? 1 : 0, with_hessian ? 1 : 0, flags, dirscale, corrscale, refine32_threshold()};
        // FULL: every task has exactly 128 support and 128 query points in 16-byte aligned rows (affine addresses, no clamps)
        const bool full = ns == HY_N && nq == HY_N && !b->n_s && !b->n_q && tv.vec;
        const bool rbf = b->kernel == ADKF_KERNEL_RBF;
        if (full && rbf) k_hyper<true, 0><<<grid_for(T, 1), HY_NT, HY_LDS_BYTES, st>>>(ha);
        else if (full) k_hyper<true, 1><<<grid_for(T, 1), HY_NT, HY_LDS_BYTES, st>>>(ha);
        else if (rbf) k_hyper<false, 0><<<grid_for(T, 1), HY_NT, HY_LDS_BYTES, st>>>(ha);
        else k_hyper<false, 1><<<grid_for(T, 1), HY_NT, HY_LDS_BYTES, st>>>(ha);
    } else {
    launch_alpha_refine(tv, b, w, st);
    if (with_hessian) {
        ProbP pp; pp.tv = tv; pp.Ainv = w.Ainv; pp.D2ss = w.D2ss; pp.P = w.P;
        launch_gemm(pp, T, ns, ns, st);
        HessArgs ha{tv, w.Ainv, w.P, w.D2ss, b->y_s, b->priors, w.scal, w.vecs, T};
        if (ns > REG_POINTS) {
            k_lg_hess_mv<<<dim3(ceil_div(ns, 4), T), 256, 0, st>>>(ha);
            LgMat am = lg_mat(w, w.Ainv, ns, b->n_s, nullptr, T);
            LgMatvecArgs mv{am, w.vecs + (size_t)V_BETA * w.vld, (size_t)NVEC * w.vld, w.vecs + (size_t)V_DELTA * w.vld, (size_t)NVEC * w.vld, 1.f};
            k_lg_matvec<<<dim3(ceil_div(ns, 4), T), 256, 0, st>>>(mv);
            LgHessTr ht{ha, w.lg_part, tms * tms, tms};
            k_lg_hess_tr<<<grid_for(T, tms * tms), 256, 0, st>>>(ht);
            k_lg_hess_fin<<<T, 64, 0, st>>>(ht);
        } else {
            k_hess<<<grid_for(T, 1), SMALL_NT, 0, st>>>(ha);
        }
    }
    launch_c(tv, b, w, st);
    ProbS ps; ps.tv = tv; ps.C = w.C; ps.D2qs = w.D2qs; ps.D2qq = w.D2qq; ps.S = w.S;
    launch_gemm(ps, T, nq, nq, st);
    // (reused inner stage: A^-1, alpha and the scalars of phi are in the workspace, info[] is written by the outer factor)
    OuterArgs oa{tv, w.C, w.S, b->y_s, b->y_q, w.vecs, w.scal, f_out, info, T, reuse_inner ? 1 : 0};
    rc = launch_outer_factor(oa, w, nq, st);
    if (rc) return rc;
    ProbOC po; po.tv = tv; po.Sinv = w.S; po.C = w.C; po.D2qs = w.D2qs; po.OC = w.OC; po.Wqs = w.Wqs; po.part = w.part_oc; po.ntiles = w.nt_oc; po.dirscale = dirscale;
    launch_gemm(po, T, nq, ns, st);
    ProbMA pm; pm.tv = tv; pm.C = w.C; pm.OC = w.OC; pm.D2ss = w.D2ss; pm.Wss = w.Wss; pm.part = w.part_ma; pm.ntiles = w.nt_ma; pm.dirscale = dirscale;
    launch_gemm(pm, T, ns, ns, st);
    SolveArgs sa{tv, w.scal, w.vecs, w.part_oc, w.part_ma, w.nt_oc, w.nt_ma, flags, g_phi_out, v_out, H_out, T, with_hessian ? 1 : 0};
    WqqArgs wq{tv, w.S, w.D2qq, w.Wqq, w.scal, dirscale, T, 0, sa};
    if (nq > REG_POINTS) {
        LgWqq lw{wq, w.lg_part, tmq * tmq, tmq};
        k_lg_wqq<<<grid_for(T, tmq * tmq), 256, 0, st>>>(lw);
        k_lg_wqq_fin<<<T, 64, 0, st>>>(lw);
        k_solve_v<<<T, 64, 0, st>>>(sa);
    } else {
        wq.do_solve = 1;   // g_out, v and w in the tail of the same workgroup
        k_wqq<<<grid_for(T, 1), SMALL_NT, 0, st>>>(wq);
    }
    if (corrscale != 0.f) {
        ProbMixed px; px.tv = tv; px.Ainv = w.Ainv; px.P = w.P; px.D2ss = w.D2ss; px.Wss = w.Wss; px.corrscale = corrscale;
        launch_gemm(px, T, ns, ns, st);
    }
    }
    if (dZ_s || dZ_q) {
        if (dZ_s && b->n_s) hipMemsetAsync(dZ_s, 0, (size_t)T * ns * d * sizeof(float), st);   // padded rows only exist in ragged batches
        if (dZ_q && b->n_q) hipMemsetAsync(dZ_q, 0, (size_t)T * nq * d * sizeof(float), st);
        ProbDZ<false> pzs; pzs.tv = tv; pzs.Wss = w.Wss; pzs.Wqs = w.Wqs; pzs.Wqq = w.Wqq; pzs.Zs = b->Z_s; pzs.Zq = b->Z_q; pzs.dZ = dZ_s; pzs.d = d;
        ProbDZ<true> pzq; pzq.tv = tv; pzq.Wss = w.Wss; pzq.Wqs = w.Wqs; pzq.Wqq = w.Wqq; pzq.Zs = b->Z_s; pzq.Zq = b->Z_q; pzq.dZ = dZ_q; pzq.d = d;
        // Full batches: one launch, one workgroup per task (dz_task.h).  Measured at C2 (profiles/dz_task_bench.json: six alternating
        // runs per library on one box): the step 0.8664 -> 0.8195 ms, ranges 8.4 and 5.9 us.  Earlier forms, measured and dropped: both
        // cotangents in ONE tiled launch behind a run-time switch, 139.8 us against 62.6 + 56.4 for the two launches; one workgroup per
        // task on the FP32 pipe with both operands in LDS and no pipeline (k_dz in tools/variants/dz.h at 4c3bc9b), 135 us.
        if (dz_task_ok(b, w, dZ_s, dZ_q)) {
            k_dz_task<<<grid_for(T, 1), DT_NT, DT_LDS_BYTES, st>>>(DzTaskArgs{w.Wss, w.Wqs, w.Wqq, b->Z_s, b->Z_q, dZ_s, dZ_q, d, T});
        } else {
            // the split form by a rule of this product's own: its contraction runs over the points, not over d
            const bool x3 = ns == DT_N && nq == DT_N;
            if (dZ_s) launch_gemm(pzs, T, ns, d, st, x3);
            if (dZ_q) launch_gemm(pzq, T, nq, d, st, x3);
        }
    }
    if (w.w64) {
        // flagged (ill-conditioned) tasks, ONE launch at the very end: the factorisation-type stages (A^-1, alpha, P, the Hessian, C,
        // Sigma_q^-1, e, f_out) and then the cotangent algebra and dL/dZ, in float64, over what the kernels above wrote for them
        size_t lds_bytes;
        const Refine64Args ra = refine_args(tv, b, w, with_hessian, 2, f_out, info, nullptr, nullptr, nullptr, lds_bytes);
        Cot64Args ca{tv, b->Z_s, b->Z_q, dZ_s, dZ_q, d, w.vecs, w.scal, w.w64, w.w64_stride, r64_threshold(), T,
                     with_hessian ? 1 : 0, flags, dirscale, corrscale, g_phi_out, v_out, H_out, lds_bytes ? 1 : 0};
        k_tail64<<<T, R64_NT, lds_bytes, st>>>(ra, ca);
    }
    LAUNCH_OK();
    return 0;
}

// C = K_qs A^-1, predictive mean / variance (/ covariance) from the distances, A^-1 and scalars in the workspace
int predict_core(const adkf_batch_t* b, const Workspace& w, float* mean, float* var, float* cov, int32_t* info, hipStream_t st) {
    TaskView tv = make_tv(b, w, true);
    const int T = b->T;
    launch_alpha_refine(tv, b, w, st);
    launch_c(tv, b, w, st);
    launch_refine(tv, b, w, false, 1, nullptr, info, st);
    PredArgs pa{tv, w.C, w.D2qs, b->y_s, mean, var, w.scal, T};
    k_predict<<<grid_for(T, 1), 256, 0, st>>>(pa);
    if (cov) {
        hipMemsetAsync(cov, 0, (size_t)T * b->nq_max * b->nq_max * sizeof(float), st);
        ProbS ps; ps.tv = tv; ps.C = w.C; ps.D2qs = w.D2qs; ps.D2qq = w.D2qq; ps.S = cov;
        launch_gemm(ps, T, b->nq_max, b->nq_max, st);
    }
    LAUNCH_OK();
    return 0;
}

}  // namespace
