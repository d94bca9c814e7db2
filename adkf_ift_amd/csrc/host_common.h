// Host side, shared by every subsystem: grid arithmetic, the launch check, the batched-GEMM launch, the values read from the
// environment, the dynamic-LDS opt-in and the cursor that carves workspaces.  Like host_gp.h, host_ard.h, host_stream.h, host_gnn.h
// and host_dense.h a part of the one translation unit adkf_gp.hip, which includes the public header and the kernel headers first.
#pragma once
#include <initializer_list>

using namespace adkf;

namespace {

constexpr int MAX_POINTS = 4096;  // <= 128: register-resident sweep (inner.h); above: blocked sweep through L2/HBM (large.h)
constexpr int REG_POINTS = 128;

inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

inline int grid_for(int T, int tiles) { return ((T + 7) / 8) * 8 * tiles; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Output tiles of the batched GEMMs: 64 x 64 (GT, four co-resident workgroups per CU) throughout.  The 128 x 128 tile halves the
// operand traffic but leaves one wave per SIMD: measured slower at every stage of C2 (ProbDist 33 -> 49 us, ProbP 22 -> 32 us,
// profiles/ notes in DESIGN.md).
inline int tiles_of(int M, int N) { return ceil_div(M, GT) * ceil_div(N, GT); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

thread_local hipError_t g_last_hip_error = hipSuccess;  // diagnostics only: what ADKF_E_LAUNCH was about (adkf_last_hip_error)
#define LAUNCH_OK() do { const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { g_last_hip_error = e_; return ADKF_E_LAUNCH; } } while (0)

int num_cus() {
    static const int n = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        return cus;
    }();
    return n;
}

// Which problems run on the BF16 matrix pipe (gemm_x3.h: FP32 products out of three-way split operands).
template <class P> struct use_x3 : std::false_type {};
template <> struct use_x3<ProbDistMulti> : std::true_type {};
// ProbDZ: as tiled launches the split form takes the same time as the FP32 form (62.5 + 54.4 against 61 + 56.5 us at C2: 64 x 64 tiles
// wait for their operands, not for the matrix pipe).  It is on this list for its arithmetic: full batches of 128 + 128 points run
// k_dz_task (dz_task.h), which writes what k_bgemm3<ProbDZ> writes, and every other batch of that padded size (ragged, misaligned,
// other d, one cotangent only) has to round as they do.  The caller asks for it by a rule of ProbDZ's own (host_gp.h::outer_pipeline);
// the support-only call sites never do.
template <bool QUERY> struct use_x3<ProbDZ<QUERY>> : std::true_type {};
// (The N^3 products of the multi-launch outer stage beyond 128 points - ProbP, ProbC, ProbS, ProbOC, ProbMA, ProbMixed - were tried on
// it as well: the same 1.99 ms for the eleven products of a C5 step, profiles/r05_c5_x3_kernel_stats.csv - at 64 x 64 tiles and
// K = 1024 they wait for their operands, 6.9 TB/s out of L2 / MALL, not for the matrix pipe.)

template <class P>
void launch_gemm(const P& p, int T, int M, int N, hipStream_t st, bool x3 = false) {
    const int tm = ceil_div(M, GT), tn = ceil_div(N, GT);
    if constexpr (use_x3<P>::value) {
        if (x3) { k_bgemm3<P, GT, 256><<<((T + 7) / 8) * 8 * tm * tn, 256, 0, st>>>(p, T, tm, tn); return; }
    }
    k_bgemm<P, GT><<<((T + 7) / 8) * 8 * tm * tn, 256, 0, st>>>(p, T, tm, tn);
}

// ----------------------------------------------------------------------------------------------------------------------
// Everything the library reads from the environment: three numbers, each read once at first use.  None of them selects a
// code path by name; every path is chosen from the shapes, the device and the batch flags.
//   ADKF_R64_THRESHOLD      pivot ratio of a task's sweep above which it redoes the factorisation-type stages in float64
//                           (refine64.h).  Default R64_THRESHOLD (30); 0 sends every task there, a huge value none.  The
//                           streaming-prediction tests move it, in a child process, to reach the refined branch.
//   ADKF_REFINE32_THRESHOLD (s + noise) max_i (A^-1)_ii above which C and alpha get one step of float32 iterative
//                           refinement.  Default 3.  Moved by the same tests.
//   ADKF_R64_MAXN           largest batch, in points, whose workspace gets a float64 region: the memory knob documented in
//                           include/adkf_gp.h.  Default and upper limit R64_MAXN (1024); tasks of larger batches stay on the
//                           float32 path whatever their conditioning.
// ----------------------------------------------------------------------------------------------------------------------
float r64_threshold() {
    static const float thresh = [] { const char* e = getenv("ADKF_R64_THRESHOLD"); return e ? (float)atof(e) : R64_THRESHOLD; }();
    return thresh;
}
float refine32_threshold() {
    static const float thresh = [] { const char* e = getenv("ADKF_REFINE32_THRESHOLD"); return e ? (float)atof(e) : 3.f; }();
    return thresh;
}
int r64_maxn() {
    static const int n = [] { const char* e = getenv("ADKF_R64_MAXN"); const int v = e ? atoi(e) : R64_MAXN; return v < R64_MAXN ? v : R64_MAXN; }();
    return n;
}

// More dynamic LDS than the 64 KB default needs an opt-in per kernel.  True when every kernel took it (no error is left behind
// otherwise); call it from a function-local `static const bool`, and let the caller decide what a refusal means.
template <class K> const void* kernel_ptr(K* k) { return reinterpret_cast<const void*>(k); }
bool lds_optin(size_t bytes, std::initializer_list<const void*> kernels) {
    bool ok = true;
    for (const void* k : kernels) ok = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess && ok;
    if (!ok) (void)hipGetLastError();
    return ok;
}

// Carves consecutive regions, each padded to 256 bytes, out of a caller's buffer; base == nullptr only measures (off is the size).
struct Arena {
    char* base;
    size_t off;
    template <class T> T* as(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += align_up(count * sizeof(T));
        return p;
    }
    float* floats(size_t n) { return as<float>(n); }
};

}  // namespace
