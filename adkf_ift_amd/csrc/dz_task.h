// k_dz_task: dL/dZ of a FULL batch of 128 support and 128 query points - both cotangents of one task by ONE workgroup, bit for bit what
// k_bgemm3<ProbDZ<false>, 64, 256> and k_bgemm3<ProbDZ<true>, 64, 256> write (problems.h, gemm_x3.h).
//
//     Wfull = [[4 W_ss, 2 W_qs^T], [2 W_qs, 4 W_qq]]  (256 x 256),  Z = [Z_s; Z_q]  (256 x d),  dZ = rowsum(Wfull) o Z - Wfull Z
//
// The generic launches run 2 x 2 (d / 64) tiles of 64 x 64 per task; each stages a 64 x 256 panel of the weights and a 256 x 64 panel of Z,
// 128 KB per tile, three times the compulsory bytes out of L2 / MALL, and pays its own first load, sixteen barriers and row-sum
// reduction.  Here the output is cut into 128 x 128 tiles - the column panels of 128 features (the last one may hold 32, 64 or 96), the
// support rows and then the query rows of each - and a tile is one pass of dist_task.h's pipeline over the 256 points:
//   * 512 lanes, 2 x 4 waves of 64 x 32, eight K chunks of 32, LDS double-buffered: two buffers x (weights, Z) x three planes = 122 880
//     bytes (DT_LDS_BYTES; needs the opt-in), one barrier per chunk, two chunks of operand loads in flight per lane (16 registers each);
//   * the K-contiguous weight segments (W_ss; W_qs and W_qq for the query rows) by X3Cfg<128, 512>'s K-contiguous map - eight lanes per
//     row, four k each, 16-byte loads; the segments strided along the contraction (Z; W_qs for the support rows, where the contraction
//     runs over the ROWS of W_qs) by its MN-contiguous map - a column per lane, eight scalar row loads, each a coalesced segment across
//     the wave: no operand is fetched with a stride;
//   * the chunk loop is unrolled over its eight chunks, so which map a chunk takes is known at compile time: nothing in it is
//     conditional, and in its last chunks the loads in flight are those of the NEXT tile's first two chunks (after the last tile: the
//     same addresses again, dropped), which arrive while this tile's stores drain.
// Arithmetic, kept from the generic launch term by term: per 16 x 16 tile and chunk small += a0 b2, a2 b0, a1 b1; acc += a0 b0;
// small += a0 b1, a1 b0 (a: the weights), acc + small once at the end, rs[i] z - (acc + small) (ProbDZ::epi's expression).  The
// coefficient rs[i] = sum_k Wfull[i, k] is summed as the generic launch's staging map sums it: eight chains per row - chain j takes
// k = 32 c + 4 j .. + 3 of every chunk c, in order - combined as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)), which is what the
// XOR1 / XOR2 / HALF_MIRROR steps give lane 0 of the row (the additions commute).  For the support rows the chains change hands after
// chunk 3: the K-contiguous map's lane (row, j) parks its chain in LDS and the MN-contiguous map's lane (row, k run 8 q .. 8 q + 7) goes
// on with chains 2 q and 2 q + 1.  The MFMA takes Z first (the transposed 16 x 16 block, as in k_dist_task: the same products in the
// same order), so a lane holds four consecutive features of one row: 16-byte loads of Z and stores of dZ in the epilogue.
#pragma once
#include "kernels.h"
#include "gemm_x3.h"
#include "dist_task.h"

namespace adkf {

struct DzTaskArgs {
    const float *Wss, *Wqs, *Wqq;     // [T, 128, 128] each
    const float *Zs, *Zq;             // [T, 128, d]; 16-byte aligned, d a multiple of 32
    float *dZs, *dZq;                 // [T, 128, d]; 16-byte aligned
    int d, T;
};

extern __shared__ __attribute__((aligned(16))) unsigned short dz_lds[];

__global__ __launch_bounds__(DT_NT) void k_dz_task(DzTaskArgs a) {
    constexpr int MI = 4, MJ = 2, NCH = 2 * DT_N / GK;   // eight chunks: four of support points, four of query points
    constexpr int DPP_IDENTITY = 0xE4;
    int t, tile;
    if (!task_tile(a.T, 1, t, tile)) return;
    __shared__ float chain[DT_N][8];   // support rows: the eight row-sum chains after the W_ss chunks
    __shared__ __attribute__((aligned(16))) float pairs[DT_N][4];   // support rows: s0 + s1, s2 + s3, s4 + s5, s6 + s7
    __shared__ float rowsum[DT_N];     // query rows
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = wv >> 2, wc = wv & 3, fi = lane & 15, fk = lane >> 4;
    const int d = a.d, npanel = (d + DT_N - 1) / DT_N;

    const int sr = tid >> 3, sj = tid & 7;      // K-contiguous map: rows sr and sr + 64, k = 4 sj .. + 3 of every chunk
    const int mc = tid & (DT_N - 1), mq = tid >> 7;   // MN-contiguous map: column mc, k = 8 mq .. + 7 of every chunk
    // (every load is a uniform base plus ONE 32-bit byte offset per lane; the host keeps 100 d bytes below 2^32)
    const char* const wss = reinterpret_cast<const char*>(a.Wss + (size_t)t * DT_N * DT_N);
    const char* const wqs = reinterpret_cast<const char*>(a.Wqs + (size_t)t * DT_N * DT_N);
    const char* const wqq = reinterpret_cast<const char*>(a.Wqq + (size_t)t * DT_N * DT_N);
    const char* const zs = reinterpret_cast<const char*>(a.Zs + (size_t)t * DT_N * d);
    const char* const zq = reinterpret_cast<const char*>(a.Zq + (size_t)t * DT_N * d);
    const uint32_t off_k = 4u * (uint32_t)(sr * DT_N + 4 * sj), off_m = 4u * (uint32_t)(8 * mq * DT_N + mc);
    // a column beyond d (last panel) is read as column d - 1: its products land in output columns that are not stored
    auto z_off = [&](int panel) __attribute__((always_inline)) { return 4u * ((uint32_t)(8 * mq) * (uint32_t)d + (uint32_t)min(panel * DT_N + mc, d - 1)); };
    auto ld4 = [](const char* base, uint32_t o) __attribute__((always_inline)) { return *reinterpret_cast<const float4*>(base + o); };
    auto ld1 = [](const char* base, uint32_t o) __attribute__((always_inline)) { return *reinterpret_cast<const float*>(base + o); };
    // A lane offset goes through an empty asm statement wherever a group of loads or stores uses it.  With every chunk known at compile
    // time hipcc otherwise folds base + offset into one 64-bit pointer per lane, matrix and row block, keeps them all - and the
    // epilogue's, advanced per panel - in registers from the top of the kernel, and spills (392 bytes of scratch).
    auto fresh = [](uint32_t o) __attribute__((always_inline)) { asm volatile("" : "+v"(o)); return o; };
    const int frag_a = (wr * 64 + fi) * X3_RS + 8 * fk, frag_b = DT_OPER + (wc * 32 + fi) * X3_RS + 8 * fk;

    float ra[2][8], rb[2][8];   // two chunks of loads in flight: the weights' and Z's
    float sq[2];                // row-sum chains of this lane (K-contiguous map: rows sr, sr + 64; MN-contiguous: chains 2 mq, 2 mq + 1)

    // which staging map chunk C of the weights takes, and the factor its segment carries (ProbDZ::a)
    auto fetch_a = [&](auto query, auto chunk, int set) __attribute__((always_inline)) {
        constexpr bool Q = decltype(query)::value;
        constexpr int C = decltype(chunk)::value;
        if constexpr (Q || C < NCH / 2) {
            const char* W = (Q ? (C < NCH / 2 ? wqs : wqq) : wss) + 4 * GK * (C % (NCH / 2));
            const uint32_t o = fresh(off_k);
            const float4 r0 = ld4(W, o), r1 = ld4(W + 4 * 64 * DT_N, o);
            ra[set][0] = r0.x; ra[set][1] = r0.y; ra[set][2] = r0.z; ra[set][3] = r0.w;
            ra[set][4] = r1.x; ra[set][5] = r1.y; ra[set][6] = r1.z; ra[set][7] = r1.w;
        } else {   // W_qs^T: the contraction runs over the rows of W_qs
            const char* W = wqs + 4 * GK * DT_N * (C - NCH / 2);
            const uint32_t o = fresh(off_m);
#pragma unroll
            for (int x = 0; x < 8; ++x) ra[set][x] = ld1(W + 4 * DT_N * x, o);
        }
    };
    auto fetch_b = [&](auto chunk, int set, uint32_t off_z) __attribute__((always_inline)) {
        constexpr int C = decltype(chunk)::value;
        const char* Z = (C < NCH / 2 ? zs : zq) + (size_t)(4 * GK * (C % (NCH / 2))) * d;
        const uint32_t o = fresh(off_z);
#pragma unroll
        for (int x = 0; x < 8; ++x) rb[set][x] = ld1(Z + (size_t)(4 * x) * d, o);
    };
    // (the loaded weights pass through an identity DPP move, which folds into the multiplication: dist_task.h, `centre`)
    auto stage_a = [&](auto query, auto chunk, int buf, int set) __attribute__((always_inline)) {
        constexpr bool Q = decltype(query)::value;
        constexpr int C = decltype(chunk)::value;
        constexpr float f = (Q == (C < NCH / 2)) ? 2.f : 4.f;   // W_qs carries 2, W_ss and W_qq carry 4
        unsigned short* S = dz_lds + buf * DT_BUF;
        float v[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int x = 0; x < 4; ++x) v[h][x] = dpp_f<DPP_IDENTITY>(ra[set][4 * h + x]) * f;
        if constexpr (Q || C < NCH / 2) {
            x3_stage<true, DT_N, DT_NT, 2>(S, v, sq);
            if constexpr (!Q && C == NCH / 2 - 1) { chain[sr][sj] = sq[0]; chain[sr + 64][sj] = sq[1]; }
        } else {
            if constexpr (C == NCH / 2) { sq[0] = chain[mc][2 * mq]; sq[1] = chain[mc][2 * mq + 1]; }   // (written before the last barrier)
            x3_stage<false, DT_N, DT_NT, 0>(S, v, nullptr);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int x = 0; x < 4; ++x) sq[h] += v[h][x];
        }
    };
    auto stage_b = [&](int buf, int set) __attribute__((always_inline)) {
        float v[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int x = 0; x < 4; ++x) v[h][x] = rb[set][4 * h + x];
        x3_stage<false, DT_N, DT_NT, 0>(dz_lds + buf * DT_BUF + DT_OPER, v, nullptr);
    };

    f32x4 acc[MI][MJ], small[MI][MJ];
    auto multiply = [&](int buf) __attribute__((always_inline)) {
        const unsigned short* Ab = dz_lds + buf * DT_BUF + frag_a;
        const unsigned short* Bb = dz_lds + buf * DT_BUF + frag_b;
        bf16x8 b[2][MJ];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < MJ; ++j) b[q][j] = *reinterpret_cast<const bf16x8*>(Bb + q * DT_PLANE + j * 16 * X3_RS);
#define ADKF_DZ_LOADA(dst_, q_) dst_ = *reinterpret_cast<const bf16x8*>(Ab + (q_) * DT_PLANE + i * 16 * X3_RS);
#define ADKF_DZ_TERM(dst_, av_, bq_) \
    _Pragma("unroll") for (int j = 0; j < MJ; ++j) dst_[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq_[j], av_, dst_[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MI; ++i) {   // the fragments of one row tile at a time (dist_task.h)
            bf16x8 a0, ax, b2[MJ];
#pragma unroll
            for (int j = 0; j < MJ; ++j) b2[j] = *reinterpret_cast<const bf16x8*>(Bb + 2 * DT_PLANE + j * 16 * X3_RS);
            ADKF_DZ_LOADA(a0, 0) ADKF_DZ_TERM(small, a0, b2)                         // a0 b2
            ADKF_DZ_LOADA(ax, 2) ADKF_DZ_TERM(small, ax, b[0])                       // a2 b0
            ADKF_DZ_LOADA(ax, 1) ADKF_DZ_TERM(small, ax, b[1])                       // a1 b1
            ADKF_DZ_TERM(acc, a0, b[0])                                              // a0 b0: the leading term, alone in its accumulator
            ADKF_DZ_TERM(small, a0, b[1]) ADKF_DZ_TERM(small, ax, b[0])              // a0 b1, a1 b0
        }
#undef ADKF_DZ_TERM
#undef ADKF_DZ_LOADA
    };

    // One 128 x 128 output tile: rows of the support (QUERY = false) or query half, features panel * 128 .. + 127.  On entry the register
    // sets 0 and 1 hold the loads of its chunks 0 and 1; on exit those of the tile that follows (off_next: its Z offsets).
    auto run_tile = [&](auto query, int panel, uint32_t off_z, uint32_t off_next) __attribute__((always_inline)) {
        constexpr bool Q = decltype(query)::value;
        const std::integral_constant<bool, !Q> next{};
        const bool cols_on = panel * DT_N + wc * 32 < d;   // (wave-uniform; d is a multiple of 32) this wave's features exist
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < MJ; ++j) { acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; small[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        sq[0] = 0.f; sq[1] = 0.f;
        // every wave multiplies first, then stages; one barrier per chunk: buffer (C + 1) & 1 was last read before the previous one
        auto step = [&](auto chunk) __attribute__((always_inline)) {
            constexpr int C = decltype(chunk)::value, N1 = (C + 1) & 1;
            if (cols_on) multiply(C & 1);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (C + 1 < NCH) {
                stage_a(query, std::integral_constant<int, (C + 1) % NCH>{}, N1, N1);
                __builtin_amdgcn_sched_barrier(0);
                stage_b(N1, N1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (C + 3 < NCH) {
                fetch_a(query, std::integral_constant<int, (C + 3) % NCH>{}, N1); fetch_b(std::integral_constant<int, (C + 3) % NCH>{}, N1, off_z);
            } else if constexpr (C + 3 < NCH + 2) {
                fetch_a(next, std::integral_constant<int, (C + 3) % NCH>{}, N1); fetch_b(std::integral_constant<int, (C + 3) % NCH>{}, N1, off_next);
            }
            __syncthreads();
        };
        stage_a(query, std::integral_constant<int, 0>{}, 0, 0); stage_b(0, 0);
        fetch_a(query, std::integral_constant<int, 2>{}, 0); fetch_b(std::integral_constant<int, 2>{}, 0, off_z);
        __syncthreads();
        step(std::integral_constant<int, 0>{}); step(std::integral_constant<int, 1>{}); step(std::integral_constant<int, 2>{});
        step(std::integral_constant<int, 3>{}); step(std::integral_constant<int, 4>{}); step(std::integral_constant<int, 5>{});
        step(std::integral_constant<int, 6>{}); step(std::integral_constant<int, 7>{});

        if constexpr (Q) {   // the eight lanes that staged a row sit side by side: three DPP steps (k_bgemm3's tree)
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                float s = sq[ps];
                s += dpp_f<DPP_XOR1>(s); s += dpp_f<DPP_XOR2>(s); s += dpp_f<DPP_HALF_MIRROR>(s);
                if (sj == 0) rowsum[sr + ps * 64] = s;
            }
        } else {
            pairs[mc][mq] = sq[0] + sq[1];
        }
        __syncthreads();
        if (cols_on) {
            const char* Zr = Q ? zq : zs;
            char* out = reinterpret_cast<char*>((Q ? a.dZq : a.dZs) + (size_t)t * DT_N * d);
            // row wr * 64 + fi of the half, this wave's 32 features, four of them per lane: below 2^31 bytes (d <= 2^22)
            const uint32_t eo = fresh(4u * ((uint32_t)(wr * 64 + fi) * (uint32_t)d + (uint32_t)(panel * DT_N + wc * 32 + fk * 4)));
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int gi = (wr * 4 + i) * 16 + fi;
                float rs;
                if constexpr (Q) rs = rowsum[gi];
                else { const float4 p = *reinterpret_cast<const float4*>(&pairs[gi][0]); rs = (p.x + p.y) + (p.z + p.w); }
#pragma unroll
                for (int j = 0; j < MJ; ++j) {
                    const size_t at = (size_t)(4 * 16 * i) * d + 4 * 16 * j;   // (uniform)
                    const f32x4 v = acc[i][j] + small[i][j];
                    const float4 z = ld4(Zr + at, eo);
                    *reinterpret_cast<float4*>(out + at + eo) = make_float4(rs * z.x - v[0], rs * z.y - v[1], rs * z.z - v[2], rs * z.w - v[3]);
                }
            }
        }
    };

    const std::false_type support{};
    const std::true_type query{};
    uint32_t off_z = z_off(0);
    fetch_a(support, std::integral_constant<int, 0>{}, 0); fetch_b(std::integral_constant<int, 0>{}, 0, off_z);
    fetch_a(support, std::integral_constant<int, 1>{}, 1); fetch_b(std::integral_constant<int, 1>{}, 1, off_z);
    for (int panel = 0; panel < npanel; ++panel) {
        const uint32_t off_next = z_off(min(panel + 1, npanel - 1));
        run_tile(support, panel, off_z, off_z);
        run_tile(query, panel, off_z, off_next);
        off_z = off_next;
    }
}

}  // namespace adkf
