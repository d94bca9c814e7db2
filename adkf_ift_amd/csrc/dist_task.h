// k_dist_task: the distance stage of a FULL batch of 128 support and 128 query points - D2ss, D2qs, D2qq of one task by ONE workgroup,
// bit for bit what k_bgemm3<ProbDistMulti, 64, 256> writes (kernels.h, gemm_x3.h).
//
// The generic launch runs the ten active 64 x 64 tiles of a task as ten workgroups; each loads, centres and three-way splits both of its
// operands, so every 64-row group of Z_s and Z_q is fetched and split five times, and each tile pays its own first load, its sixteen
// barriers and its row-norm reduction.  Here a task's 128 x 32 slice of Z_s and of Z_q is loaded, centred and split ONCE per K chunk:
//   * 512 lanes, 2 x 4 waves of 64 x 32 (the fragment layout of k_bgemm3<..., 128, 512> / k_dense3), K chunks of 32, the staging map of
//     X3Cfg<128, 512> (eight lanes per row, four k each, rows 80 bytes apart), LDS double-buffered: two buffers x (Z_s, Z_q) x three planes
//     = 122 880 bytes (dense_x3.h's size; needs the opt-in), one barrier per chunk;
//   * two chunks of operand loads in flight per lane (16 registers each: two float4 of each operand; the mean's float4, which comes from
//     L2, one chunk ahead): one chunk ahead is bound by load latency at K = 256 (dense_x3.h), a third set does not fit the registers;
//   * pass 1 over K forms D2ss and D2qs (both have Z_s as their column operand: one set of B fragments, 128 accumulator registers),
//     pass 2 forms D2qq (64) from Z_q alone, re-read through L2; its first loads are issued before the stores of pass 1, which drain
//     under it.  All three blocks at once do not fit 256 registers.
// Arithmetic, kept from the generic launch term by term: Z - mean before the split; per 16 x 16 tile and chunk small += a0 b2, a2 b0,
// a1 b1; acc += a0 b0; small += a0 b1, a1 b0 (a: the row operand - Z_q for D2qs, row i <= j of a symmetric block), acc + small once at
// the end; the squared row norms from x3_stage<..., SQ = 1> (fmaf over the four k of a lane's slot and over the chunks, then the
// XOR1 / XOR2 / HALF_MIRROR tree over the row's eight lanes); ProbDist::value; symmetric blocks: diagonal 0, entries i < j computed and
// also stored as their mirror image.  The MFMA takes the column operand first (d3_multiply's transposed 16 x 16 block: the same products in
// the same order), so a lane holds four consecutive columns of one row: D2qs and the upper halves go out as 16-byte stores.
// Waves (wr, wc) = (1, 0), (1, 1) hold the 64 x 64 quadrant below the diagonal of a symmetric block and issue no MFMA for it.
// The median heuristic in the same launch (SELECT instance; adkf_median_lengthscale / adkf_init_params on a batch that takes this path):
// between the passes, once pass 1's stores are issued, the entries above the diagonal of D2ss go - still in registers, 32 keys per lane,
// none in the waves (1, 0) and (1, 1) - through median_select.h's histogram select; the histograms (26 368 bytes) lie in the staging
// buffers, which are free there.  Lane 0 writes l0 and calls init_params_task, as k_median does, and such a step launches no k_median.
// First tried with k_median's 31-step select on the same registers: 65.3 us against 46.6 us without it, i.e. 18.7 us inside the launch
// for what k_median did in 19.0 us as a launch of its own - nothing.  Neither select is bound by its barriers: it is bound by its
// instructions per held key (the 31 steps: four per key and step; the histogram form: a few dozen per key and digit, most of them the
// tie handling), so four barriers instead of thirty-two bought less than their count suggests.  Measured (MI355X, C2, rocprofv3 trace
// averages, profiles/dist_fused_kernel_stats{_parent,}.csv): 58.6 us against 43.5 + 19.1 us for k_dist_task and k_median as two
// launches, i.e. the select costs 15.1 us inside the launch (4.0 us saved).  The C2 step: profiles/dist_fused_bench.json.
#pragma once
#include "kernels.h"
#include "gemm_x3.h"

namespace adkf {

constexpr int DT_N = 128, DT_NT = 512, DT_PLANE = DT_N * X3_RS, DT_OPER = 3 * DT_PLANE, DT_BUF = 2 * DT_OPER;
constexpr int DT_LDS_BYTES = 2 * DT_BUF * (int)sizeof(unsigned short);   // 122 880

struct DistTaskArgs {
    const float *Zs, *Zq, *mean;      // [T, 128, d], [T, 128, d], [T, d] (k_colmean's); 16-byte aligned, d a multiple of 32
    float *D2ss, *D2qs, *D2qq;        // [T, 128, 128] each
    int d, T;
    float* l0;                        // SELECT instance: [T], sqrt(median / 2) of the task's D2ss
    InitArgs init;                    // SELECT instance: phi != null -> init_params_task with that l0
};

static_assert(MedianSelect<MEDIAN_W>::WORDS * (int)sizeof(uint32_t) <= DT_LDS_BYTES, "the select's histograms live in the staging buffers");

extern __shared__ __attribute__((aligned(16))) unsigned short dt_lds[];

template <bool SELECT>   // SELECT: the median heuristic (and a4) on the D2ss values between the passes; without it l0 and init are not read
__global__ __launch_bounds__(DT_NT) void k_dist_task(DistTaskArgs a) {
    constexpr int MI = 4, MJ = 2, IH = 1;   // IH: row tiles whose fragments are held at once (block_terms)
    int t, tile;
    if (!task_tile(a.T, 1, t, tile)) return;
    __shared__ float rowsq[2][DT_N];   // squared norms of the centred rows: [0] Z_s, [1] Z_q
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // waves wv and wv + 4 share a SIMD: the second row of waves is turned by two columns, so that the waves (1, 0) and (1, 1), which have
    // no part in a symmetric block, sit beside (0, 2) and (0, 3), and every SIMD has one wave's worth of each symmetric block (a quarter
    // fewer MFMAs on the busiest SIMD; no measurable change at C2, where the products are not what the other waves wait for)
    const int wr = wv >> 2, wc = (wv & 3) ^ (wr << 1), fi = lane & 15, fk = lane >> 4;
    const int d = a.d, nc = d / GK, last = nc - 1;
    const bool sym_on = !(wr == 1 && wc < 2);   // (wave-uniform) this wave's part of a symmetric block has entries on or above the diagonal

    const int sr = tid >> 3, sk = (tid & 7) * 4;   // staging: rows sr and sr + 64, k = sk .. sk + 3 of every chunk
    // (every load is a uniform base - the task's rows 0 .. 63 or 64 .. 127, advanced by the chunk - plus ONE 32-bit byte offset per lane;
    // a row block is 256 d bytes, which the host keeps below 2^31)
    const char* const zs = reinterpret_cast<const char*>(a.Zs + (size_t)t * DT_N * d);
    const char* const zq = reinterpret_cast<const char*>(a.Zq + (size_t)t * DT_N * d);
    const char* const mu = reinterpret_cast<const char*>(a.mean + (size_t)t * d);
    const size_t hi = (size_t)256 * d;
    const uint32_t off = 4u * (uint32_t)(sr * d + sk), off_mu = 4u * (uint32_t)sk;
    auto ldb = [](const char* base, uint32_t o) __attribute__((always_inline)) { return *reinterpret_cast<const float4*>(base + o); };
    const int frag_a = (wr * 64 + fi) * X3_RS + 8 * fk, frag_b = (wc * 32 + fi) * X3_RS + 8 * fk;

    float4 rs[2][2], rq[2][2], rm;   // (the mean's eight float4 per chunk come from L2: one chunk ahead is enough)
    float sqs[2] = {0.f, 0.f}, sqq[2] = {0.f, 0.f};
    auto fetch = [&](auto with_s, int set, int c) __attribute__((always_inline)) {
        const size_t k = (size_t)(4 * GK) * c;
        if constexpr (decltype(with_s)::value) { rs[set][0] = ldb(zs + k, off); rs[set][1] = ldb(zs + hi + k, off); }
        rq[set][0] = ldb(zq + k, off); rq[set][1] = ldb(zq + hi + k, off);
    };
    auto fetch_mean = [&](int c) __attribute__((always_inline)) { rm = ldb(mu + (size_t)(4 * GK) * c, off_mu); };
    // Z - mean of one float4.  The loaded values pass through an identity DPP move (quad_perm 0, 1, 2, 3) first: hipcc otherwise pairs
    // entries of DIFFERENT loads for its packed arithmetic (the two rows' norm chains) and builds those pairs by copies placed right
    // behind the loads, with a wait for each - the prefetch was then as good as synchronous (s_waitcnt vmcnt(1) at the end of the very
    // iteration that issued it).  The move folds into the subtraction.
    auto centre = [](const float4& r, const float4& m, float (&v)[4]) __attribute__((always_inline)) {
        constexpr int DPP_IDENTITY = 0xE4;
        v[0] = dpp_f<DPP_IDENTITY>(r.x) - m.x; v[1] = dpp_f<DPP_IDENTITY>(r.y) - m.y;
        v[2] = dpp_f<DPP_IDENTITY>(r.z) - m.z; v[3] = dpp_f<DPP_IDENTITY>(r.w) - m.w;
    };
    // `commit`: the chunk exists (the pipeline stages once past the last chunk rather than branch around a stage and its loads); a
    // staging pass that does not count leaves the norms alone
    auto stage = [&](auto with_s, int buf, int set, bool commit) __attribute__((always_inline)) {
        constexpr bool S = decltype(with_s)::value;
        unsigned short* B = dt_lds + buf * DT_BUF;
        float v[2][4], ts[2] = {sqs[0], sqs[1]}, tq[2] = {sqq[0], sqq[1]};
        if constexpr (S) {
            centre(rs[set][0], rm, v[0]); centre(rs[set][1], rm, v[1]);
            x3_stage<true, DT_N, DT_NT, 1>(B, v, ts);
        }
        centre(rq[set][0], rm, v[0]); centre(rq[set][1], rm, v[1]);
        x3_stage<true, DT_N, DT_NT, S ? 1 : 0>(B + DT_OPER, v, tq);   // (the norms of Z_q are summed in pass 1 only)
        if constexpr (S) {
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) { sqs[ps] = commit ? ts[ps] : sqs[ps]; sqq[ps] = commit ? tq[ps] : sqq[ps]; }
        }
    };

    // one block's terms of one chunk: Ab = the row operand's fragments, b = the column operand's (three planes)
    auto block_terms = [&](const unsigned short* Ab, const unsigned short* Bb, const bf16x8 (&b)[2][MJ], f32x4 (&acc)[MI][MJ], f32x4 (&small)[MI][MJ]) __attribute__((always_inline)) {
        // IH row tiles at a time: the fragment registers of all four at once do not fit
#define ADKF_DT_LOADA(dst_, q_) _Pragma("unroll") for (int i = 0; i < IH; ++i) dst_[i] = *reinterpret_cast<const bf16x8*>(Ab + (q_) * DT_PLANE + (ih + i) * 16 * X3_RS);
#define ADKF_DT_TERM(dst_, av_, bq_)                                                                       \
    _Pragma("unroll") for (int i = 0; i < IH; ++i) _Pragma("unroll") for (int j = 0; j < MJ; ++j)        \
        dst_[ih + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq_[j], av_[i], dst_[ih + i][j], 0, 0, 0);
#pragma unroll
        for (int ih = 0; ih < MI; ih += IH) {
            bf16x8 a0[IH], ax[IH], b2[MJ];   // (plane 2 of the column operand has one use: read here, not held beside the other two)
#pragma unroll
            for (int j = 0; j < MJ; ++j) b2[j] = *reinterpret_cast<const bf16x8*>(Bb + 2 * DT_PLANE + j * 16 * X3_RS);
            ADKF_DT_LOADA(a0, 0) ADKF_DT_TERM(small, a0, b2)                         // a0 b2
            ADKF_DT_LOADA(ax, 2) ADKF_DT_TERM(small, ax, b[0])                       // a2 b0
            ADKF_DT_LOADA(ax, 1) ADKF_DT_TERM(small, ax, b[1])                       // a1 b1
            ADKF_DT_TERM(acc, a0, b[0])                                              // a0 b0: the leading term, alone in its accumulator
            ADKF_DT_TERM(small, a0, b[1]) ADKF_DT_TERM(small, ax, b[0])              // a0 b1, a1 b0
        }
#undef ADKF_DT_TERM
#undef ADKF_DT_LOADA
    };
    auto load_b = [&](const unsigned short* Bb, bf16x8 (&b)[2][MJ]) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < MJ; ++j) b[q][j] = *reinterpret_cast<const bf16x8*>(Bb + q * DT_PLANE + j * 16 * X3_RS);
    };
    // The chunk pipeline of one pass, two chunks per trip (register set and LDS buffer = chunk & 1); sets 0 and 1 hold the loads of
    // chunks 0 and 1 on entry.  Inside the loop nothing is conditional: every fetch goes out (beyond the last chunk it re-reads the last
    // one and is dropped) and so does the stage after an even count's last chunk.  With a branch around a stage or a load hipcc's
    // s_waitcnt for a set counts no younger load (on SOME path through the branches there is none) and waits for everything in flight.
    auto run_pass = [&](auto with_s, auto&& multiply) __attribute__((always_inline)) {
        auto advance = [&](int c, int nbuf, int nset, bool commit) __attribute__((always_inline)) {   // chunk c + 1 to LDS, c + 3 on its way
            stage(with_s, nbuf, nset, commit);
            fetch_mean(min(c + 2, last));
            __builtin_amdgcn_sched_barrier(0);   // (the counter retires loads in order: the mean, wanted one chunk sooner, goes first)
            fetch(with_s, nset, min(c + 3, last));
        };
        // Every wave multiplies first, then stages (measured at T = 256, d = 256: 44.4 us; k_dense3's ping-pong order - waves 0 - 3 staging
        // first - 47.8 us, as in k_dense3_sk).  One barrier per chunk: buffer nbuf was last read before the previous one.
        stage(with_s, 0, 0, true);
        fetch_mean(min(1, last));
        __builtin_amdgcn_sched_barrier(0);
        fetch(with_s, 0, min(2, last));
        __syncthreads();
        int c = 0;
        for (; c + 1 < nc; c += 2) {
            multiply(0); advance(c, 1, 1, true); __syncthreads();
            multiply(1); advance(c + 1, 0, 0, c + 2 < nc); __syncthreads();
        }
        if (c < nc) { multiply(0); __syncthreads(); }   // an odd count's last chunk
    };
    auto zero = [](f32x4 (&x)[MI][MJ]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < MJ; ++j) x[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    };
    // ProbDist::value on this lane's four consecutive columns of row gi (transposed block: row = lane & 15, columns 4 (lane >> 4) + reg)
    auto values = [&](const f32x4& acc, const float* nrow, const float* ncol, int gi, int gj0, float (&v)[4]) __attribute__((always_inline)) {
        const float nx = nrow[gi];
        const float4 ny = *reinterpret_cast<const float4*>(ncol + gj0);
        v[0] = fmaxf(nx + ny.x - 2.f * acc[0], 0.f); v[1] = fmaxf(nx + ny.y - 2.f * acc[1], 0.f);
        v[2] = fmaxf(nx + ny.z - 2.f * acc[2], 0.f); v[3] = fmaxf(nx + ny.w - 2.f * acc[3], 0.f);
    };
    // a symmetric block's 16 x 16 tile (row tile rt, column tile ct): nothing below the diagonal, the diagonal 0, every entry above it
    // and its mirror image; v: the lane's four values (those on or below the diagonal included)
    auto store_sym = [&](float* D, const f32x4& acc, const float* nrm, int rt, int ct, float (&v)[4]) __attribute__((always_inline)) {
        const int gi = rt * 16 + fi, gj0 = ct * 16 + fk * 4;
        values(acc, nrm, nrm, gi, gj0, v);
        if (rt < ct) {   // (wave-uniform)
            *reinterpret_cast<float4*>(D + (size_t)gi * DT_N + gj0) = make_float4(v[0], v[1], v[2], v[3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) D[(size_t)(gj0 + r) * DT_N + gi] = v[r];
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gj = gj0 + r;
                if (gi == gj) D[(size_t)gi * DT_N + gj] = 0.f;
                else if (gi < gj) { D[(size_t)gi * DT_N + gj] = v[r]; D[(size_t)gj * DT_N + gi] = v[r]; }
            }
        }
    };

    const std::true_type pass1{};
    const std::false_type pass2{};
    float* const Dss = a.D2ss + (size_t)t * DT_N * DT_N;
    float* const Dqs = a.D2qs + (size_t)t * DT_N * DT_N;
    float* const Dqq = a.D2qq + (size_t)t * DT_N * DT_N;

    // ---- pass 1: D2ss and D2qs ----
    fetch_mean(0);
    __builtin_amdgcn_sched_barrier(0);
    fetch(pass1, 0, 0); fetch(pass1, 1, min(1, last));
    {
        f32x4 acc_s[MI][MJ], small_s[MI][MJ], acc_q[MI][MJ], small_q[MI][MJ];
        zero(acc_s); zero(small_s); zero(acc_q); zero(small_q);
        run_pass(pass1, [&](int buf) __attribute__((always_inline)) {
            const unsigned short* S = dt_lds + buf * DT_BUF;
            bf16x8 b[2][MJ];
            load_b(S + frag_b, b);
            if (sym_on) block_terms(S + frag_a, S + frag_b, b, acc_s, small_s);
            __builtin_amdgcn_sched_barrier(0);   // (the second block's fragments are not loaded over the first's: registers)
            block_terms(S + DT_OPER + frag_a, S + frag_b, b, acc_q, small_q);
        });
        // pass 2's first loads go out ahead of the stores below
        fetch_mean(0);
        __builtin_amdgcn_sched_barrier(0);
        fetch(pass2, 0, 0); fetch(pass2, 1, min(1, last));
        // the eight lanes that staged a row sit side by side: three DPP steps (k_bgemm3's tree)
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            float s = sqs[ps], q = sqq[ps];
            s += dpp_f<DPP_XOR1>(s); s += dpp_f<DPP_XOR2>(s); s += dpp_f<DPP_HALF_MIRROR>(s);
            q += dpp_f<DPP_XOR1>(q); q += dpp_f<DPP_XOR2>(q); q += dpp_f<DPP_HALF_MIRROR>(q);
            if ((tid & 7) == 0) { rowsq[0][sr + ps * 64] = s; rowsq[1][sr + ps * 64] = q; }
        }
        __syncthreads();
        // the select's keys: the entries above the diagonal of D2ss, as k_median takes them from memory (0: not a candidate)
        uint32_t key[SELECT ? MI * MJ * 4 : 1];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < MJ; ++j) {
                const int rt = wr * 4 + i, ct = wc * 2 + j;
                float v[4];
                values(acc_q[i][j] + small_q[i][j], rowsq[1], rowsq[0], rt * 16 + fi, ct * 16 + fk * 4, v);
                *reinterpret_cast<float4*>(Dqs + (size_t)(rt * 16 + fi) * DT_N + ct * 16 + fk * 4) = make_float4(v[0], v[1], v[2], v[3]);
                if (rt <= ct) store_sym(Dss, acc_s[i][j] + small_s[i][j], rowsq[0], rt, ct, v);
                if constexpr (SELECT) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        key[(i * MJ + j) * 4 + r] = (rt <= ct && rt * 16 + fi < ct * 16 + fk * 4 + r) ? __float_as_uint(v[r]) : 0u;
                }
            }
        // The staging buffers are free between the passes (every wave is past the barrier that follows its last multiply) and hold the
        // histograms; the stores above drain under the select.  The barrier behind it keeps pass 2's staging off the last scan.
        if constexpr (SELECT) {
            const uint32_t bits = median_select<DT_NT, MI * MJ * 4, MEDIAN_W>(key, reinterpret_cast<uint32_t*>(dt_lds));
            __syncthreads();
            if (tid == 0) median_finish(a.init, t, a.l0, bits);   // (behind the barrier: the other waves do not wait for its logarithms)
        }
    }

    // ---- pass 2: D2qq (Z_q alone, from L2) ----
    {
        f32x4 acc_g[MI][MJ], small_g[MI][MJ];
        zero(acc_g); zero(small_g);
        run_pass(pass2, [&](int buf) __attribute__((always_inline)) {
            if (sym_on) {
                const unsigned short* Q = dt_lds + buf * DT_BUF + DT_OPER;
                bf16x8 b[2][MJ];
                load_b(Q + frag_b, b);
                block_terms(Q + frag_a, Q + frag_b, b, acc_g, small_g);
            }
        });
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < MJ; ++j) {
                const int rt = wr * 4 + i, ct = wc * 2 + j;
                float v[4];
                if (rt <= ct) store_sym(Dqq, acc_g[i][j] + small_g[i][j], rowsq[1], rt, ct, v);
            }
    }
}

}  // namespace adkf
