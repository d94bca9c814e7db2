// median_select: the exact lower median of the positive keys a workgroup holds in registers (K per lane, 0 = not a candidate), by a
// histogram radix select on the bit patterns (positive floats order like their bits).  k_median (kernels.h) and k_dist_task
// (dist_task.h) both end in it.
//   1. count, minimum and maximum of the candidates: one LDS hop across the waves.  The leading bits min and max share are the
//      answer's; all-equal candidates are finished here.  rank = (count - 1) / 2 (torch.median).
//   2. the remaining bits in digits of at most W, most significant first, one histogram of 2^W bins per digit.  All histograms are
//      zeroed before the barrier of step 1, so a pass is: integer LDS adds, ONE barrier, then EVERY wave scans the whole histogram by
//      itself (2^W / 64 consecutive bins per lane, a DPP scan over the lanes) and arrives at the same bin and the same rank inside it:
//      no second barrier and no broadcast.  Three passes at most for W = 11: four barriers in all where the one-bit-per-step select
//      has thirty-two.
// Ties: before its own add each key is compared with the wave's first candidate of the same register; the lanes that agree are
// counted with one population count and added by one lane.  Thousands of equal keys are then one add per wave and register instead of
// 64 adds queueing on one LDS address.  Integer adds only: the result does not depend on any order of arrival.
// Every lane of the workgroup must call; the keys are below 2^31; nothing here reads or writes outside `lds`.
#pragma once
#include "device_utils.h"

namespace adkf {

template <int W>
struct MedianSelect {
    static_assert(W >= 7 && W <= 13, "2^W bins, at least two per lane of a scanning wave");
    static constexpr int NB = 1 << W, BPL = NB / 64;          // bins; consecutive bins of one lane of the scan
    static constexpr int HIST = NB + 64;                        // bin b sits at b + b / BPL: a lane's bins start BPL + 1 words apart
    static constexpr int PASSES = (31 + W - 1) / W;
    static constexpr int HEAD = 64 * 4;                         // {count, min, max} per wave, 16 waves at most
    static constexpr int WORDS = HEAD + PASSES * HIST;          // 32-bit words of LDS, 16-byte aligned
    __device__ static constexpr int slot(int b) { return b + b / BPL; }
};

// inclusive sum over the lanes 0 .. lane of the wave (every lane active)
__device__ __forceinline__ int wave_scan_i(int v) {
    constexpr int ROW_SHR = 0x110;   // row_shr:n reads lane - n of the same row of 16; lanes without a source read 0 (bound_ctrl)
    v += dpp_i<ROW_SHR + 1>(v);
    v += dpp_i<ROW_SHR + 2>(v);
    v += dpp_i<ROW_SHR + 4>(v);
    v += dpp_i<ROW_SHR + 8>(v);
    const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31), t2 = __builtin_amdgcn_readlane(v, 47);
    const int row = (threadIdx.x & 63) >> 4;
    return v + (row >= 1 ? t0 : 0) + (row >= 2 ? t1 : 0) + (row >= 3 ? t2 : 0);
}
__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
    v = min(v, (uint32_t)dpp_i<DPP_XOR1>((int)v)); v = min(v, (uint32_t)dpp_i<DPP_XOR2>((int)v));
    v = min(v, (uint32_t)dpp_i<DPP_HALF_MIRROR>((int)v)); v = min(v, (uint32_t)dpp_i<DPP_MIRROR>((int)v));
    const int b = (int)v;
    return min(min((uint32_t)__builtin_amdgcn_readlane(b, 0), (uint32_t)__builtin_amdgcn_readlane(b, 16)),
               min((uint32_t)__builtin_amdgcn_readlane(b, 32), (uint32_t)__builtin_amdgcn_readlane(b, 48)));
}
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) { return ~wave_umin(~v); }

// -> the bit pattern of the lower median of the non-zero keys, 0 without one (the same value in every lane)
template <int NT, int K, int W>
__device__ __forceinline__ uint32_t median_select(const uint32_t (&key)[K], uint32_t* lds) {
    using M = MedianSelect<W>;
    constexpr int NW = NT / 64;
    static_assert(NW <= 16 && NT % 64 == 0, "the header has room for sixteen waves");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t* const hist = lds + M::HEAD;

    // ---- 1. count, min, max; the histograms are zeroed under the same barrier ----
    int count = 0;   // wave-uniform
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        count += __popcll(__ballot(key[r] != 0u));
        lo = min(lo, key[r] != 0u ? key[r] : 0xFFFFFFFFu);
        hi = max(hi, key[r]);
    }
    lo = wave_umin(lo); hi = wave_umax(hi);
    if (lane == 0) { lds[4 * wv] = (uint32_t)count; lds[4 * wv + 1] = lo; lds[4 * wv + 2] = hi; }
    for (int i = tid * 4; i < M::PASSES * M::HIST; i += NT * 4) *reinterpret_cast<uint4*>(hist + i) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    int total = 0;
    lo = 0xFFFFFFFFu; hi = 0u;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const uint4 h = *reinterpret_cast<const uint4*>(lds + 4 * i);
        total += (int)h.x; lo = min(lo, h.y); hi = max(hi, h.z);
    }
    if (total == 0) return 0u;
    if (lo == hi) return lo;
    int rank = (total - 1) / 2;   // torch.median: the lower median
    int nb = min(32 - __clz((int)(lo ^ hi)), 31);   // bits still open: the candidates agree in every bit from nb up
    uint32_t prefix = (lo >> nb) << nb;

    // ---- 2. one digit per pass ----
    for (int p = 0; nb > 0; ++p) {   // at most PASSES trips: nb <= 31 falls by W per trip
        const int w = min(W, nb), shift = nb - w;
        const uint32_t dmask = (1u << w) - 1u;
        uint32_t* const h = hist + p * M::HIST;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const bool live = key[r] != 0u && (key[r] >> nb) == (prefix >> nb);
            const unsigned long long act = __ballot(live);
            if (act == 0ull) continue;   // (wave-uniform)
            const int dg = (int)((key[r] >> shift) & dmask);
            const int first = __ffsll(act) - 1;
            const int d0 = __builtin_amdgcn_readlane(dg, first);
            const unsigned long long same = __ballot(live && dg == d0);
            if (lane == first) atomicAdd(h + M::slot(d0), (uint32_t)__popcll(same));
            else if (live && dg != d0) atomicAdd(h + M::slot(dg), 1u);
        }
        __syncthreads();
        // every wave: the bin that holds `rank`, and the rank inside it
        int c[M::BPL], s = 0;
#pragma unroll
        for (int j = 0; j < M::BPL; ++j) c[j] = (int)h[lane * (M::BPL + 1) + j];
        __builtin_amdgcn_sched_barrier(0);   // (all reads in flight before the first sum: hipcc otherwise waits for each in turn)
#pragma unroll
        for (int j = 0; j < M::BPL; ++j) s += c[j];
        const int incl = wave_scan_i(s), excl = incl - s;
        const int local = rank - excl;                       // the rank among this lane's bins, if it lies there
        int below = 0, bin = 0, cum = 0;
#pragma unroll
        for (int j = 0; j < M::BPL; ++j) {
            cum += c[j];
            const bool under = cum <= local;                 // bin j ends at or before the rank
            bin += under ? 1 : 0;
            below = under ? cum : below;
        }
        const unsigned long long own = __ballot(local >= 0 && local < s);   // exactly one lane: 0 <= rank < the sum of all bins
        const int o = __ffsll(own) - 1;
        const int digit = __builtin_amdgcn_readlane(lane * M::BPL + bin, o);
        rank = __builtin_amdgcn_readlane(local - below, o);
        prefix |= ((uint32_t)digit & dmask) << shift;
        nb = shift;
    }
    return prefix;
}

}  // namespace adkf
