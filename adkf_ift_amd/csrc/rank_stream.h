// Large-k selection and row ranks over a shared pool (adkf_rank_pool): per task the first k eligible rows of the pool, k up to
// RANK_K_MAX, under the total order of every selection here (pm_beats: larger score first, equal scores by ascending row, -0 and +0
// tie, NaN and excluded rows never listed), the 0-based rank of up to RANK_REFS_MAX named rows in that order, and the number of rows
// ranked.  The score is adkf_predict_pool's: EI, log EI or +-mean.
//
//   pre-pass       (M > 0) k_rank_gather copies the named rows into the scratch as a packed query set [T * M, d], q_off = t * M; the
//                  host runs prediction's packed launch on it (pm_launch<ARD, false>, the caller's flags and best_f); k_rank_refs
//                  turns what it wrote into ref_val and the start of the counters: 0, or -1 / NaN for an entry outside the pool, a
//                  NaN score or a skipped task.  The refs' scores are known before the walk, so counting costs no second walk.
//   the walk       the host walks the pool in chunks of RANK_CHUNK_ROWS rows, each through prediction's own pool launch
//                  (pm_launch<ARD, true>, k = 0, the one plane the score reads, [T, chunk] in the scratch): the scores are
//                  prediction's by construction, for every kind of task, and nothing here forms a kernel value.
//   k_rank_chunk   one workgroup per task, after the chunk's prediction.  It walks the chunk's rows 256 at a time: eligibility (the
//                  exclusion list is searched for every row when something is counted, otherwise only for rows that pass the
//                  threshold, as pm_list_merge does), one ballot per wave into an LDS bit mask and into n_ranked, and the SURVIVORS -
//                  eligible rows that beat the task's current k-th entry, every eligible row while the list is short - compacted
//                  into an LDS slice of RANK_SLICE 64-bit keys (order-preserving score bits, inverted, -0 as +0; then the row's
//                  offset in the chunk).  A full slice, and the last one, is sorted by a bitonic network in LDS and merged with the
//                  task's sorted list in global memory into the task's OTHER list, truncated to k: a merge-path partition gives every
//                  thread its own run of the output.  Then the task's mark flips and the threshold is read again, so later slices
//                  keep fewer rows.  A chunk without survivors touches neither list.  At the end a thread per ref counts the
//                  chunk's eligible rows that beat (ref_val, ref_row) into ref_rank, a wave taking 64 rows' scores at a time: plain
//                  integer adds, one workgroup owns a task and the chunks' launches are ordered on the stream.
//   k_rank_finish  the task's current list to top_idx / top_val, -1 / -inf beyond its length.
//
// top_val is read back from the plane by the key's row offset, so it carries the score's own bits, the sign of a zero included; the
// key only orders.  The selection is the first k of a set under a total order and a count is a sum of integers: neither depends on
// the slices, the chunk boundaries, the grid or the other tasks.  No floating-point atomics (the only atomics are integer adds in LDS).
#pragma once
#include "predict_stream.h"

namespace adkf {

constexpr int RANK_K_MAX = 65536;
constexpr int RANK_REFS_MAX = 1024;
constexpr int RANK_CHUNK_ROWS = 16384;
constexpr int RANK_NT = 256;
constexpr int RANK_SLICE = 4096;            // survivors sorted at a time: 32 KB of static LDS, no opt-in, several workgroups per CU
static_assert(RANK_CHUNK_ROWS % RANK_NT == 0 && RANK_CHUNK_ROWS % 64 == 0 && RANK_SLICE % RANK_NT == 0 && RANK_SLICE >= 2 * RANK_NT, "rank_stream.h tiling");

struct RankArgs {
    int T, k, M, neg;                       // neg: the score is -plane (the mean score of a minimisation)
    int count;                              // M > 0 or n_ranked given: every row's eligibility is needed
    const float* plane;                     // [T, L]: the chunk's EI, log EI or mean, prediction's own
    int64_t c0, L, rows;                    // the chunk's first row and length; the pool's rows
    const int64_t *excl_idx, *excl_off;     // as PmPool's
    int64_t* list_idx; float* list_val;     // [2, T, k] each: a task's two sorted lists
    int32_t *cur, *cnt;                     // [T] each: which list is current, and its length
    const int64_t* ref_idx;                 // [T, M]
    int64_t* ref_rank; float* ref_val;      // [T, M]: the counters (-1: not counted) and the refs' scores
    int64_t* n_ranked;                      // [T], nullable
    int64_t* top_idx; float* top_val;       // [T, k]
    // the pre-pass
    const float* X; int d;
    float *Xg, *gmean, *gei;                // [T * M, d], [T * M], [T * M] (gei: nullable, the EI scores)
    int64_t* q_off;                         // [T + 1]
};

// the order as an integer: ascending key = descending score, -0 as +0 (on the bits: no arithmetic touches a subnormal); never a NaN
__device__ __forceinline__ unsigned rank_key32(float s) {
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;
    return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
// (key, row) comes before (key2, row2)
__device__ __forceinline__ bool rank_before(unsigned ka, long long ra, unsigned kb, long long rb) { return ka < kb || (ka == kb && ra < rb); }

__device__ __forceinline__ bool rank_excluded(const RankArgs& e, int t, long long r) {
    PmPool s{};
    s.excl_idx = e.excl_idx; s.excl_off = e.excl_off;
    return pm_excluded(s, t, r);
}
__device__ __forceinline__ float rank_score(const RankArgs& e, int t, int i) {
    const float v = e.plane[(size_t)t * (size_t)e.L + (size_t)i];
    return e.neg ? -v : v;
}

// ---- the pre-pass: the named rows as a packed query set (zeros for an entry outside the pool), and its offsets
__global__ __launch_bounds__(64) void k_rank_gather(RankArgs e) {
    const size_t q = blockIdx.x;            // t * M + j
    const int64_t r = e.ref_idx[q];
    const bool in = r >= 0 && r < e.rows;
    for (int c = threadIdx.x; c < e.d; c += 64) e.Xg[q * e.d + c] = in ? e.X[(size_t)r * e.d + c] : 0.f;
    if (q == 0)
        for (int t = threadIdx.x; t <= e.T; t += 64) e.q_off[t] = (int64_t)t * e.M;
}

// ---- the state of every task before the walk: empty lists, nothing ranked, and the refs' scores and counters
__global__ __launch_bounds__(RANK_NT) void k_rank_refs(PmArgs a, RankArgs e) {
    const int t = blockIdx.x, tid = threadIdx.x;
    const bool skip = pm_kind_of(a, t) < 0;
    if (tid == 0) {
        e.cur[t] = 0; e.cnt[t] = 0;
        if (e.n_ranked) e.n_ranked[t] = 0;
    }
    for (int j = tid; j < e.M; j += RANK_NT) {
        const size_t q = (size_t)t * e.M + j;
        const int64_t r = e.ref_idx[q];
        float v = __builtin_nanf("");
        if (!skip && r >= 0 && r < e.rows) {
            const float g = e.gei ? e.gei[q] : e.gmean[q];
            v = e.neg ? -g : g;
        }
        e.ref_val[q] = v;
        e.ref_rank[q] = v == v ? 0 : -1;
    }
}

// ---- one chunk of the pool, one workgroup per task
__global__ __launch_bounds__(RANK_NT) void k_rank_chunk(PmArgs a, RankArgs e) {
    __shared__ unsigned long long keys[RANK_SLICE];
    __shared__ unsigned long long elig[RANK_CHUNK_ROWS / 64];
    __shared__ int wcount[RANK_NT / 64];
    __shared__ int s_cur, s_cnt, s_nr;
    __shared__ unsigned s_thr_key;
    __shared__ long long s_thr_row;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (pm_kind_of(a, t) < 0) return;       // (uniform) a skipped task: the fills
    const int k = e.k, L = (int)e.L;
    const size_t Tk = (size_t)e.T * k;
    // the threshold: the k-th entry of the current list once it is full
    auto load_state = [&](int cur, int cnt) {
        s_cur = cur; s_cnt = cnt;
        if (cnt == k && k > 0) {
            const size_t q = (size_t)cur * Tk + (size_t)t * k + (k - 1);
            s_thr_key = rank_key32(e.list_val[q]); s_thr_row = e.list_idx[q];
        }
    };
    if (tid == 0) { load_state(e.cur[t], e.cnt[t]); s_nr = 0; }
    __syncthreads();

    // n survivors in keys[]: sorted, merged with the current list into the other one, and the mark flipped
    auto flush = [&](int n) {
        int N = 2;
        while (N < n) N <<= 1;
        for (int i = n + tid; i < N; i += RANK_NT) keys[i] = ~0ull;
        __syncthreads();
        for (int size = 2; size <= N; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int p = tid; p < (N >> 1); p += RANK_NT) {
                    const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1)), l = i + stride;
                    const unsigned long long x = keys[i], y = keys[l];
                    if ((x > y) == ((i & size) == 0)) { keys[i] = y; keys[l] = x; }
                }
                __syncthreads();
            }
        const int cur = s_cur, cnt = s_cnt;
        const int64_t* Ai = e.list_idx + (size_t)cur * Tk + (size_t)t * k;
        const float* Av = e.list_val + (size_t)cur * Tk + (size_t)t * k;
        int64_t* Bi = e.list_idx + (size_t)(cur ^ 1) * Tk + (size_t)t * k;
        float* Bv = e.list_val + (size_t)(cur ^ 1) * Tk + (size_t)t * k;
        const int out_n = cnt + n < k ? cnt + n : k;
        const int per = (out_n + RANK_NT - 1) / RANK_NT;
        const int d0 = tid * per < out_n ? tid * per : out_n, d1 = d0 + per < out_n ? d0 + per : out_n;
        auto s_key = [&](int j) { return (unsigned)(keys[j] >> 32); };
        auto s_row = [&](int j) { return (long long)e.c0 + (long long)(unsigned)keys[j]; };
        if (d0 < d1) {
            // the merge path: the output positions before d0 hold i entries of the list and d0 - i survivors
            int lo = d0 - n > 0 ? d0 - n : 0, hi = d0 < cnt ? d0 : cnt;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1, j = d0 - 1 - mid;
                if (rank_before(rank_key32(Av[mid]), Ai[mid], s_key(j), s_row(j))) lo = mid + 1; else hi = mid;
            }
            int i = lo, j = d0 - lo;
            float av = 0.f; long long ai = 0; unsigned ak = 0;
            if (i < cnt) { av = Av[i]; ai = Ai[i]; ak = rank_key32(av); }
            for (int o = d0; o < d1; ++o) {
                const bool take_a = j >= n || (i < cnt && rank_before(ak, ai, s_key(j), s_row(j)));
                if (take_a) {
                    Bi[o] = ai; Bv[o] = av;
                    if (++i < cnt) { av = Av[i]; ai = Ai[i]; ak = rank_key32(av); }
                } else {
                    const int off = (int)(unsigned)keys[j];
                    Bi[o] = e.c0 + off; Bv[o] = rank_score(e, t, off);
                    ++j;
                }
            }
        }
        __threadfence_block();
        __syncthreads();
        if (tid == 0) { load_state(cur ^ 1, out_n); e.cur[t] = cur ^ 1; e.cnt[t] = out_n; }
        __syncthreads();
    };

    int n_buf = 0;
    long long ranked = 0;
    for (int b0 = 0; b0 < L; b0 += RANK_NT) {
        const int i = b0 + tid;
        const bool in = i < L;
        const float s = in ? rank_score(e, t, i) : 0.f;
        const long long r = e.c0 + i;
        bool ok = in && s == s;
        if (e.count) {
            if (ok) ok = !rank_excluded(e, t, r);
            const unsigned long long m = __ballot(ok);
            if (lane == 0) elig[(b0 >> 6) + wv] = m;
            ranked += __popcll(m);
        }
        bool surv = ok && k > 0 && (s_cnt < k || rank_before(rank_key32(s), r, s_thr_key, s_thr_row));
        if (!e.count && surv) surv = !rank_excluded(e, t, r);
        const unsigned long long sm = __ballot(surv);
        if (lane == 0) wcount[wv] = __popcll(sm);
        __syncthreads();
        int base = n_buf, total = 0;
        for (int w = 0; w < RANK_NT / 64; ++w) { if (w < wv) base += wcount[w]; total += wcount[w]; }
        if (surv) keys[base + __popcll(sm & ((1ull << lane) - 1ull))] = ((unsigned long long)rank_key32(s) << 32) | (unsigned)i;
        n_buf += total;
        __syncthreads();
        if (n_buf + RANK_NT > RANK_SLICE) { flush(n_buf); n_buf = 0; }   // (uniform) the next 256 rows might not fit
    }
    if (n_buf > 0) flush(n_buf);

    if (!e.count) return;
    if (e.n_ranked) {
        if (lane == 0) atomicAdd(&s_nr, (int)ranked);
        __syncthreads();
        if (tid == 0) e.n_ranked[t] += s_nr;
    }
    // the ranks: W threads hold a ref each, 256 / W of them share its rows; the partial counts meet in LDS (keys[] is free now)
    int* part_cnt = reinterpret_cast<int*>(keys);
    for (int j0 = 0; j0 < e.M; j0 += RANK_NT) {
        // W >= 64, so a wave holds 64 refs and one share of the chunk's 64-row blocks: it loads a block's scores once, a lane each, and
        // every lane compares all 64 with its own ref by readlane - the inner loop touches no memory
        int W = 64;
        while (W < RANK_NT && W < e.M - j0) W <<= 1;
        const int P = RANK_NT / W, jj = tid & (W - 1), part = tid / W, j = j0 + jj;
        const size_t q = (size_t)t * e.M + (j < e.M ? j : 0);
        const bool have = j < e.M && e.ref_rank[q] >= 0;
        const float rv = have ? e.ref_val[q] : 0.f;
        const long long rr = have ? (long long)e.ref_idx[q] : 0;
        __syncthreads();
        if (tid < W) part_cnt[tid] = 0;
        __syncthreads();
        int c = 0;
        for (int blk = part; blk < ((L + 63) >> 6); blk += P) {   // (uniform in a wave, which the shuffles need)
            const int i = (blk << 6) + lane;
            const float sc = i < L ? rank_score(e, t, i) : 0.f;
            const unsigned long long m = elig[blk];               // (rows beyond L are not eligible)
            const long long r0 = e.c0 + (blk << 6);
#pragma unroll 8
            for (int l = 0; l < 64; ++l) {
                const float s = __shfl(sc, l);
                c += (((m >> l) & 1ull) && pm_beats(s, r0 + l, rv, rr)) ? 1 : 0;
            }
        }
        if (have) atomicAdd(&part_cnt[jj], c);
        __syncthreads();
        if (have && part == 0) e.ref_rank[q] += part_cnt[jj];
    }
}

// ---- the task's current list to top_idx / top_val [T, k], -1 / -inf beyond its length (a skipped task: all of it)
__global__ __launch_bounds__(RANK_NT) void k_rank_finish(RankArgs e) {
    const int t = blockIdx.x, k = e.k;
    const int cur = e.cur[t], cnt = e.cnt[t];
    const size_t src = ((size_t)cur * e.T + t) * k, dst = (size_t)t * k;
    for (int q = threadIdx.x; q < k; q += RANK_NT) {
        e.top_idx[dst + q] = q < cnt ? e.list_idx[src + q] : -1;
        e.top_val[dst + q] = q < cnt ? e.list_val[src + q] : -INFINITY;
    }
}

}  // namespace adkf
