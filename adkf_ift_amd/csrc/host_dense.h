// Host side and entry points of the dense layers on the BF16 matrix pipe (plane split, forward product, weight gradient) and of the
// optimiser step (sum of squares, clip + Adam).
#pragma once
#include "host_common.h"

extern "C" {

int adkf_split_planes(const float* x, uint16_t* planes, int64_t rows, int64_t K, void* stream) {
    (void)hipGetLastError();
    if (!x || !planes || rows <= 0 || K <= 0 || (K & 1)) return ADKF_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(x) & 7) || (reinterpret_cast<uintptr_t>(planes) & 15) || ((rows * K) & 7)) return ADKF_E_BADARG;
    const size_t pairs = (size_t)rows * (size_t)K / 2;
    if (pairs > (size_t)0x7fffffff * 256) return ADKF_E_SIZE;
    k_split3<<<(unsigned)((pairs + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(x, planes, pairs, (size_t)rows * (size_t)K);
    LAUNCH_OK();
    return 0;
}

int adkf_split_planes_t(const float* w, uint16_t* planes, int64_t K, int64_t N, void* stream) {
    (void)hipGetLastError();
    if (!w || !planes || K <= 0 || N <= 0 || (K & 1)) return ADKF_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(w) & 3) || (reinterpret_cast<uintptr_t>(planes) & 15) || ((N * K) & 7)) return ADKF_E_BADARG;
    if (K > 0x7fffffffLL || N > 0x7fffffffLL) return ADKF_E_SIZE;
    const size_t pairs = (size_t)(K / 2) * (size_t)N;
    if (pairs > (size_t)0x7fffffff * 256) return ADKF_E_SIZE;
    k_split3_t<<<(unsigned)((pairs + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(w, planes, (int)K, (int)N);
    LAUNCH_OK();
    return 0;
}

int adkf_dense_forward(const float* x, int32_t ldx, const uint16_t* w_planes, const float* bias, float* y, int32_t ldy, int32_t M,
                       int32_t N, int32_t K, void* stream) {
    (void)hipGetLastError();
    if (!x || !w_planes || !y || M <= 0 || N <= 0 || K <= 0 || ldx < K || ldy < N) return ADKF_E_BADARG;
    if ((K % GK) || (ldx & 3)) return ADKF_E_SIZE;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_planes)) & 15) return ADKF_E_BADARG;
    static const bool optin = lds_optin(D3_LDS_BYTES, {kernel_ptr(&k_dense3)});
    if (!optin) { g_last_hip_error = hipErrorInvalidValue; return ADKF_E_LAUNCH; }
    const long long tiles = (long long)ceil_div(M, D3_TM) * ceil_div(N, D3_TN);
    if (tiles > 0x7fffffffLL) return ADKF_E_SIZE;
    Dense3Args a{x, ldx, w_planes, (size_t)N * (size_t)K, bias, y, ldy, M, N, K};
    // short contractions over many rows: the persistent form that keeps a row tile's whole K extent in registers (bit-identical
    // results; 79 -> 63 us at 65 536 x 256 x 256, tools/x3_stream_bench.hip)
    const int tiles_m = ceil_div(M, D3_TM);
    if ((K == 64 || K == 128 || K == 256) && tiles_m >= num_cus()) {
        static const bool optin_sk = lds_optin(D3_LDS_BYTES, {kernel_ptr(&k_dense3_sk<2>), kernel_ptr(&k_dense3_sk<4>), kernel_ptr(&k_dense3_sk<8>)});
        if (optin_sk) {
            const unsigned grid = (unsigned)num_cus();
            hipStream_t st = static_cast<hipStream_t>(stream);
            if (K == 256) k_dense3_sk<8><<<grid, D3_NT, D3_LDS_BYTES, st>>>(a);
            else if (K == 128) k_dense3_sk<4><<<grid, D3_NT, D3_LDS_BYTES, st>>>(a);
            else k_dense3_sk<2><<<grid, D3_NT, D3_LDS_BYTES, st>>>(a);
            LAUNCH_OK();
            return 0;
        }
    }
    k_dense3<<<(unsigned)tiles, D3_NT, D3_LDS_BYTES, static_cast<hipStream_t>(stream)>>>(a);
    LAUNCH_OK();
    return 0;
}

// row ranges of the weight gradient: enough workgroups for ~4 rounds of the chip, ranges a multiple of the chunk, at most 64 of them
static int dense_tn_splits(int M, int N, int K, int* rows_per_split) {
    const long long tiles = (long long)ceil_div(N, D3_TM) * ceil_div(K, D3_TN);
    long long s = (4LL * num_cus() + tiles - 1) / tiles;
    const long long max_s = (M + 4 * GK - 1) / (4 * GK);          // at least four chunks per range
    if (s > max_s) s = max_s;
    if (s > 64) s = 64;
    if (s < 1) s = 1;
    int rps = (int)((M + s - 1) / s);
    rps = (rps + GK - 1) / GK * GK;
    *rows_per_split = rps;
    return ceil_div(M, rps);
}

size_t adkf_dense_weight_grad_scratch_bytes(int32_t M, int32_t N, int32_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    int rps;
    const int splits = dense_tn_splits(M, N, K, &rps);
    return sizeof(float) * (size_t)splits * (size_t)N * (size_t)K;
}

int adkf_dense_weight_grad(const float* g, int32_t ldg, const float* x, int32_t ldx, float* dw, int32_t M, int32_t N, int32_t K,
                           void* scratch, size_t scratch_bytes, void* stream) {
    (void)hipGetLastError();
    if (!g || !x || !dw || !scratch || M <= 0 || N <= 0 || K <= 0 || ldg < N || ldx < K) return ADKF_E_BADARG;
    if (scratch_bytes < adkf_dense_weight_grad_scratch_bytes(M, N, K)) return ADKF_E_WORKSPACE;
    static const bool optin = lds_optin(D3_LDS_BYTES, {kernel_ptr(&k_dense3_tn)});
    if (!optin) { g_last_hip_error = hipErrorInvalidValue; return ADKF_E_LAUNCH; }
    int rps;
    const int splits = dense_tn_splits(M, N, K, &rps);
    const long long tiles = (long long)ceil_div(N, D3_TM) * ceil_div(K, D3_TN);
    if (tiles * splits > 0x7fffffffLL) return ADKF_E_SIZE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Dense3TnArgs a{g, ldg, x, ldx, static_cast<float*>(scratch), M, N, K, rps};
    k_dense3_tn<<<dim3((unsigned)tiles, (unsigned)splits), D3_NT, D3_LDS_BYTES, st>>>(a);
    const size_t n = (size_t)N * (size_t)K;
    k_dense3_reduce<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(static_cast<const float*>(scratch), dw, n, splits);
    LAUNCH_OK();
    return 0;
}

int adkf_grad_sumsq(const float* g, int64_t n, float* partials, void* stream) {
    (void)hipGetLastError();
    if (!g || !partials || n <= 0 || (reinterpret_cast<uintptr_t>(g) & 15)) return ADKF_E_BADARG;
    k_grad_sumsq<<<SUMSQ_PARTS, STEP_NT, 0, static_cast<hipStream_t>(stream)>>>(g, (long)n, partials);
    LAUNCH_OK();
    return 0;
}

// The update's constants, with the bias corrections in double on the host, as torch.optim.Adam does for a python-number step
static AdamArgs adam_args(float* p, float* g, float* m, float* v, int64_t n, const float* partials, int32_t n_partials, float scale, float clip,
                          double lr, double beta1, double beta2, double eps, double weight_decay, int32_t step) {
    const double bias1 = 1.0 - pow(beta1, (double)step);
    const double bias2_sqrt = sqrt(1.0 - pow(beta2, (double)step));
    return AdamArgs{p, g, m, v, (long)n, partials, n_partials, scale, clip, (float)(lr / bias1), (float)(1.0 - beta1), (float)beta2,
                    (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)bias2_sqrt};
}

int adkf_clip_adam_step(float* p, float* g, float* m, float* v, int64_t n, const float* partials, int32_t n_partials, float scale,
                        float clip, double lr, double beta1, double beta2, double eps, double weight_decay, int32_t step, void* stream) {
    (void)hipGetLastError();
    if (!p || !g || !m || !v || !partials || n <= 0 || n_partials <= 0 || step <= 0) return ADKF_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15)
        return ADKF_E_BADARG;
    const AdamArgs a = adam_args(p, g, m, v, n, partials, n_partials, scale, clip, lr, beta1, beta2, eps, weight_decay, step);
    const long n4 = (n + 3) / 4;
    int grid = (int)((n4 + STEP_NT - 1) / STEP_NT);
    grid = grid < 1 ? 1 : (grid > 2048 ? 2048 : grid);
    k_clip_adam<<<grid, STEP_NT, 0, static_cast<hipStream_t>(stream)>>>(a);
    LAUNCH_OK();
    return 0;
}

int adkf_clip_adam_step_one(float* p, float* g, float* m, float* v, int64_t n, float scale, float clip, double lr, double beta1, double beta2,
                            double eps, double weight_decay, int32_t step, uint16_t* planes_t, int32_t K, int32_t N, void* stream) {
    (void)hipGetLastError();
    if (!p || !g || !m || !v || n <= 0 || step <= 0) return ADKF_E_BADARG;
    if (n > CLIP_ADAM_ONE_MAX) return ADKF_E_SIZE;
    if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15)
        return ADKF_E_BADARG;
    if (planes_t && (K <= 0 || N <= 0 || (int64_t)K * N != n || (K % STEP1_TILE) || (N % STEP1_TILE) || (reinterpret_cast<uintptr_t>(planes_t) & 3))) return ADKF_E_BADARG;
    const AdamOneArgs o{adam_args(p, g, m, v, n, nullptr, 0, scale, clip, lr, beta1, beta2, eps, weight_decay, step), planes_t, K, N};
    const long n4 = (n + 3) / 4;
    int grid = (int)((n4 + STEP1_NT - 1) / STEP1_NT);
    if (grid < 1) grid = 1;
    if (planes_t) grid = (K / STEP1_TILE) * (N / STEP1_TILE);
    k_clip_adam_one<<<grid, STEP1_NT, 0, static_cast<hipStream_t>(stream)>>>(o);
    LAUNCH_OK();
    return 0;
}

}  // extern "C"
