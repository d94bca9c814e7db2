// libadkf_gp_cpu.so - the CPU twin of the GP entry points of include/adkf_gp.h ("CPU twins of each for
// testing without a GPU"; section 8(d)(ii): the second CPU baseline, so that GPU-vs-CPU is not only GPU vs slow Python).
//
// Same C ABI, HOST pointers: adkf_batch_t, priors, phi layouts, info codes and flags exactly as in the header; `ws` /
// `ws_bytes` / `stream` / `scratch` are accepted and ignored (adkf_workspace_bytes and every *_scratch_bytes return 0 here).  Batches
// of any size.  The fit, prediction and hypergradient entries (adkf_median_lengthscale, adkf_init_params, adkf_mll_value_grad,
// adkf_fit, adkf_predict, adkf_outer_nll_value_grad, adkf_ift_hypergrad) take non-ARD batches only.  The streaming entries on a
// support-only batch take ARD batches too - they centre and scale the features by the per-dimension lengthscales and run the
// isotropic code at unit lengthscale (csrc/ard.h, prepare_task below): adkf_predict_marginal_ard, adkf_thompson_pool_ard and
// adkf_believer_pool_ard take ARD batches only and their plain namesakes refuse them, as the library does; adkf_predict_pool,
// adkf_mes_pool, adkf_gumbel_pool, adkf_gibbon_pool, adkf_liar_pool, adkf_levelset_pool, adkf_kg_pool, adkf_ipv_pool, adkf_jes_pool, adkf_jackknife_pool, adkf_ehvi_pool
// and adkf_mix_pool take either kind.  What the pool entries share is the pool kit (after pm_task).
// Plain loops, OpenMP over the tasks of a batch, float64 arithmetic inside and float32 at the boundary - a Cholesky-based
// restatement of the same staged closed-form algebra the HIP kernels run (stage names as in DESIGN.md section 3 and
// oracle/closed_form.py): kernel matrices from difference-form squared distances, A = L L^T, A^-1, the analytic 3 x 3 Hessian,
// the joint predictive NLL with its cotangents Omega, M_A, M_B, v = H^-1 grad f_out, the mixed-partial weights and the chain
// through D^2 to dL/dZ.  The inner fit is the same quasi-Newton state machine as csrc/inner.h (BFGS, Armijo backtracking
// with safeguarded quadratic interpolation, the reference's gtol / ftol rules).
//
// Test and baseline infrastructure only: bench.py's cpu_baseline leg (entry "kind": "twin") times it, tests/test_cpu_twin.py pins it
// to the golden fixtures, every tests/test_*_pool_cpu.py, tests/test_predict_marginal*_cpu.py and tests/test_log_ei_cpu.py holds an
// entry against its float64 reference, some GPU tests hold the library against it (tests/test_gpu_believer_pool*.py, test_gpu_gibbon_pool.py,
// test_gpu_ipv_pool.py) and tools/twin_bits.py compares two builds of it bit for bit; the product package (adkf_ift_amd.gp_ops)
// never loads it and keeps refusing CPU tensors.
//   g++ -O3 -fopenmp -shared -fPIC -std=c++17 -I include adkf_ift_amd/csrc/cpu/adkf_gp_cpu.cpp -o adkf_ift_amd/libadkf_gp_cpu.so
#include <algorithm>
#include <functional>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "adkf_gp.h"

namespace {

using Mat = std::vector<double>;   // row-major
constexpr double NOISE_LB = 1e-4, LOG_2PI = 1.8378770664093453, SQRT5 = 2.23606797749979;

inline double softplus(double x) { return x > 30.0 ? x : std::log1p(std::exp(x)); }
inline double sigmoid(double x) { return 1.0 / (1.0 + std::exp(-x)); }
inline double inv_softplus(double y) { return y > 30.0 ? y : y + std::log(-std::expm1(-y)); }

inline void kappa(int kind, double u, double& k0, double& k1, double& k2) {
    if (kind == ADKF_KERNEL_RBF) { k0 = std::exp(-0.5 * u); k1 = -0.5 * k0; k2 = 0.25 * k0; return; }
    const double r = std::sqrt(u), e = std::exp(-SQRT5 * r);
    k0 = (1.0 + SQRT5 * r + (5.0 / 3.0) * u) * e; k1 = -(5.0 / 6.0) * (1.0 + SQRT5 * r) * e; k2 = (25.0 / 12.0) * e;
}

// D2[i][j] = |x_i - y_j|^2 (difference form: exact zero on the diagonal of a matrix with itself)
template <class F>
Mat sqdist(const F* X, int n, const F* Y, int m, int d) {
    Mat D((size_t)n * m);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            double s = 0.0;
            const F *x = X + (size_t)i * d, *y = Y + (size_t)j * d;
            for (int k = 0; k < d; ++k) { const double t = (double)x[k] - (double)y[k]; s += t * t; }
            D[(size_t)i * m + j] = s;
        }
    return D;
}

// in-place lower Cholesky; returns 0 or (index + 1) of the first non-positive pivot; logdet = log|A|
int cholesky(Mat& A, int n, double& logdet) {
    logdet = 0.0;
    for (int j = 0; j < n; ++j) {
        double p = A[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) p -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
        if (!(p > 0.0)) return j + 1;
        const double l = std::sqrt(p);
        A[(size_t)j * n + j] = l;
        logdet += 2.0 * std::log(l);
        for (int i = j + 1; i < n; ++i) {
            double s = A[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
            A[(size_t)i * n + j] = s / l;
        }
    }
    return 0;
}

// A^-1 from its Cholesky factor L (lower, in `L`): X = L^-T L^-1
Mat inverse_from_chol(const Mat& L, int n) {
    Mat Li((size_t)n * n, 0.0);   // L^-1, lower
    for (int j = 0; j < n; ++j) {
        Li[(size_t)j * n + j] = 1.0 / L[(size_t)j * n + j];
        for (int i = j + 1; i < n; ++i) {
            double s = 0.0;
            for (int k = j; k < i; ++k) s -= L[(size_t)i * n + k] * Li[(size_t)k * n + j];
            Li[(size_t)i * n + j] = s / L[(size_t)i * n + i];
        }
    }
    Mat X((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int k = i; k < n; ++k) s += Li[(size_t)k * n + i] * Li[(size_t)k * n + j];
            X[(size_t)i * n + j] = s; X[(size_t)j * n + i] = s;
        }
    return X;
}

Mat matmul(const Mat& A, int n, int k, const Mat& B, int m) {   // [n,k] x [k,m]
    Mat C((size_t)n * m, 0.0);
    for (int i = 0; i < n; ++i)
        for (int p = 0; p < k; ++p) {
            const double a = A[(size_t)i * k + p];
            if (a == 0.0) continue;
            const double* b = &B[(size_t)p * m];
            double* c = &C[(size_t)i * m];
            for (int j = 0; j < m; ++j) c[j] += a * b[j];
        }
    return C;
}
Mat matmul_nt(const Mat& A, int n, int k, const Mat& B, int m) {   // [n,k] x [m,k]^T
    Mat C((size_t)n * m);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            double s = 0.0;
            const double *a = &A[(size_t)i * k], *b = &B[(size_t)j * k];
            for (int p = 0; p < k; ++p) s += a[p] * b[p];
            C[(size_t)i * m + j] = s;
        }
    return C;
}
std::vector<double> matvec(const Mat& A, int n, int m, const std::vector<double>& x) {
    std::vector<double> y(n, 0.0);
    for (int i = 0; i < n; ++i) { double s = 0.0; for (int j = 0; j < m; ++j) s += A[(size_t)i * m + j] * x[j]; y[i] = s; }
    return y;
}
std::vector<double> matvec_t(const Mat& A, int n, int m, const std::vector<double>& x) {   // A^T x
    std::vector<double> y(m, 0.0);
    for (int i = 0; i < n; ++i) for (int j = 0; j < m; ++j) y[j] += A[(size_t)i * m + j] * x[i];
    return y;
}
inline double dot(const std::vector<double>& a, const std::vector<double>& b) { double s = 0.0; for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i]; return s; }
inline double frob(const Mat& A, const Mat& B) { double s = 0.0; for (size_t i = 0; i < A.size(); ++i) s += A[i] * B[i]; return s; }

void lognormal_terms(double x, double loc, double scale, double& lp, double& d1, double& d2) {
    const double lx = std::log(x), z = (lx - loc) / (scale * scale);
    lp = -lx - std::log(scale) - 0.5 * LOG_2PI - 0.5 * (lx - loc) * z;
    d1 = (-1.0 - z) / x;
    d2 = (1.0 + z - 1.0 / (scale * scale)) / (x * x);
}

struct Inner {
    int n = 0, info = 0;
    double noise, s, l, d1[3], d2[3], f_in, g_in[3], H[9], logdet;
    Mat Ainv, K, G, u, k1, k2, P;
    std::vector<double> alpha, gamma, beta, delta;
};

// oracle/closed_form.py::inner_stage
Inner inner_stage(const Mat& D2, const float* y_, int n, const double* phi, const float* pri, int kind, bool want_hess, bool want_mats) {
    Inner o; o.n = n;
    for (int q = 0; q < 3; ++q) { const double sg = sigmoid(phi[q]); o.d1[q] = sg; o.d2[q] = sg * (1.0 - sg); }
    o.noise = softplus(phi[0]) + NOISE_LB; o.s = softplus(phi[1]); o.l = softplus(phi[2]);
    const double il2 = 1.0 / (o.l * o.l);
    std::vector<double> y(n);
    for (int i = 0; i < n; ++i) y[i] = y_[i];
    o.u.resize((size_t)n * n); o.k1.resize((size_t)n * n); o.k2.resize((size_t)n * n); o.K.resize((size_t)n * n); o.G.resize((size_t)n * n);
    Mat A((size_t)n * n);
    for (size_t e = 0; e < (size_t)n * n; ++e) {
        const double u = D2[e] * il2;
        double k0, k1, k2; kappa(kind, u, k0, k1, k2);
        o.u[e] = u; o.k1[e] = k1; o.k2[e] = k2; o.K[e] = o.s * k0; o.G[e] = o.s * k1 * (-2.0 * u / o.l);
        A[e] = o.K[e];
    }
    for (int i = 0; i < n; ++i) A[(size_t)i * n + i] += o.noise;
    o.info = cholesky(A, n, o.logdet);
    if (o.info) { o.f_in = std::numeric_limits<double>::infinity(); for (double& g : o.g_in) g = 0.0; return o; }
    o.Ainv = inverse_from_chol(A, n);
    o.alpha = matvec(o.Ainv, n, n, y);
    const double ya = dot(y, o.alpha), aa = dot(o.alpha, o.alpha);
    const double nll = 0.5 * ya + 0.5 * o.logdet + 0.5 * n * LOG_2PI;
    double lpn = 0, dpn = 0, d2pn = 0, lpl = 0, dpl = 0, d2pl = 0;
    if (pri[1] > 0.f) lognormal_terms(o.noise, pri[0], pri[1], lpn, dpn, d2pn);
    if (pri[3] > 0.f) lognormal_terms(o.l, pri[2], pri[3], lpl, dpl, d2pl);
    o.f_in = (nll - lpn - lpl) / n;
    double trAinv = 0.0;
    for (int i = 0; i < n; ++i) trAinv += o.Ainv[(size_t)i * n + i];
    const double trAinvG = frob(o.Ainv, o.G);
    o.beta = matvec(o.G, n, n, o.alpha);
    const double aGa = dot(o.alpha, o.beta);
    const double g_noise = 0.5 * trAinv - 0.5 * aa;
    const double g_s = (0.5 * (n - o.noise * trAinv) - 0.5 * (ya - o.noise * aa)) / o.s;
    const double g_l = 0.5 * trAinvG - 0.5 * aGa;
    o.g_in[0] = (g_noise - dpn) * o.d1[0] / n; o.g_in[1] = g_s * o.d1[1] / n; o.g_in[2] = (g_l - dpl) * o.d1[2] / n;
    if (!want_hess) { if (!want_mats) { o.u.clear(); o.k2.clear(); } return o; }
    o.P = matmul(o.Ainv, n, n, o.G, n);
    o.gamma = matvec(o.Ainv, n, n, o.alpha);
    o.delta = matvec(o.Ainv, n, n, o.beta);
    double trA2 = frob(o.Ainv, o.Ainv), trPA = frob(o.P, o.Ainv), trPP = 0.0;
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) trPP += o.P[(size_t)i * n + j] * o.P[(size_t)j * n + i];
    const double ag = dot(o.alpha, o.gamma), bg = dot(o.beta, o.gamma), bd = dot(o.beta, o.delta), ab = dot(o.alpha, o.beta);
    double trAinvKll = 0.0, aKlla = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const size_t e = (size_t)i * n + j;
            const double kll = o.s * (o.k2[e] * 4.0 * o.u[e] * o.u[e] * il2 + o.k1[e] * 6.0 * o.u[e] * il2);
            trAinvKll += o.Ainv[e] * kll; aKlla += o.alpha[i] * kll * o.alpha[j];
        }
    double h[3][3];
    const double noise = o.noise, s = o.s;
    h[0][0] = ag - 0.5 * trA2 - d2pn;
    h[0][1] = ((aa - noise * ag) - 0.5 * (trAinv - noise * trA2)) / s;
    h[0][2] = bg - 0.5 * trPA;
    h[1][1] = ((ya - 2 * noise * aa + noise * noise * ag) - 0.5 * (n - 2 * noise * trAinv + noise * noise * trA2)) / (s * s);
    h[1][2] = ((ab - noise * bg) - 0.5 * (trAinvG - noise * trPA)) / s - (0.5 * aGa - 0.5 * trAinvG) / s;
    h[2][2] = bd - 0.5 * aKlla - 0.5 * trPP + 0.5 * trAinvKll - d2pl;
    h[1][0] = h[0][1]; h[2][0] = h[0][2]; h[2][1] = h[1][2];
    const double gt[3] = {g_noise - dpn, g_s, g_l - dpl};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) o.H[i * 3 + j] = (h[i][j] * o.d1[i] * o.d1[j] + (i == j ? gt[i] * o.d2[i] : 0.0)) / n;
    return o;
}

struct Outer {
    int info = 0;
    double f_out, g_out[3];
    Mat W_ss, W_qs, W_qq, S, C;
    std::vector<double> mean;
};

// oracle/closed_form.py::outer_stage  (level 1: mean / covariance only)
Outer outer_stage(const Mat& D2qs, const Mat& D2qq, const float* yq_, int m, const Inner& in, int kind, bool want_grads) {
    Outer o;
    const int n = in.n;
    const double il2 = 1.0 / (in.l * in.l), s = in.s, l = in.l;
    Mat B((size_t)m * n), kqs1((size_t)m * n), uqs((size_t)m * n);
    for (size_t e = 0; e < (size_t)m * n; ++e) { double k0, k1, k2; uqs[e] = D2qs[e] * il2; kappa(kind, uqs[e], k0, k1, k2); B[e] = s * k0; kqs1[e] = k1; }
    o.C = matmul(B, m, n, in.Ainv, n);
    o.mean = matvec(B, m, n, in.alpha);
    Mat CBt = matmul_nt(o.C, m, n, B, m);
    Mat Kqq((size_t)m * m), kqq1((size_t)m * m), uqq((size_t)m * m);
    o.S.resize((size_t)m * m);
    for (size_t e = 0; e < (size_t)m * m; ++e) { double k0, k1, k2; uqq[e] = D2qq[e] * il2; kappa(kind, uqq[e], k0, k1, k2); Kqq[e] = s * k0; kqq1[e] = k1; o.S[e] = Kqq[e] - CBt[e]; }
    for (int i = 0; i < m; ++i) o.S[(size_t)i * m + i] += in.noise;
    for (int i = 0; i < m; ++i) for (int j = 0; j < i; ++j) { const double a = 0.5 * (o.S[(size_t)i * m + j] + o.S[(size_t)j * m + i]); o.S[(size_t)i * m + j] = a; o.S[(size_t)j * m + i] = a; }
    if (!yq_) return o;
    Mat L = o.S;
    double logdetS;
    const int bad = cholesky(L, m, logdetS);
    if (bad) { o.info = ADKF_INFO_OUTER_BASE + bad; o.f_out = std::numeric_limits<double>::infinity(); return o; }
    Mat Sinv = inverse_from_chol(L, m);
    std::vector<double> r(m);
    for (int i = 0; i < m; ++i) r[i] = (double)yq_[i] - o.mean[i];
    std::vector<double> e = matvec(Sinv, m, m, r);
    o.f_out = 0.5 * dot(r, e) + 0.5 * logdetS + 0.5 * m * LOG_2PI;
    if (!want_grads) return o;
    Mat Om((size_t)m * m);
    for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) Om[(size_t)i * m + j] = 0.5 * (Sinv[(size_t)i * m + j] - e[i] * e[j]);
    Mat OC = matmul(Om, m, m, o.C, n);
    Mat M_B((size_t)m * n);
    for (int i = 0; i < m; ++i) for (int j = 0; j < n; ++j) M_B[(size_t)i * n + j] = -2.0 * OC[(size_t)i * n + j] - e[i] * in.alpha[j];
    std::vector<double> Cte = matvec_t(o.C, m, n, e);
    Mat M_A((size_t)n * n, 0.0);
    for (int p = 0; p < m; ++p)
        for (int i = 0; i < n; ++i) {
            const double c = o.C[(size_t)p * n + i];
            for (int j = 0; j < n; ++j) M_A[(size_t)i * n + j] += c * OC[(size_t)p * n + j];
        }
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) M_A[(size_t)i * n + j] += 0.5 * (Cte[i] * in.alpha[j] + in.alpha[i] * Cte[j]);
    double trOm = 0.0, trMA = 0.0;
    for (int i = 0; i < m; ++i) trOm += Om[(size_t)i * m + i];
    for (int i = 0; i < n; ++i) trMA += M_A[(size_t)i * n + i];
    double g_s = frob(M_A, in.K) + frob(M_B, B) + frob(Om, Kqq), g_l = frob(M_A, in.G);
    for (size_t q = 0; q < (size_t)m * n; ++q) g_l += M_B[q] * (s * kqs1[q] * (-2.0 * uqs[q] / l));
    for (size_t q = 0; q < (size_t)m * m; ++q) g_l += Om[q] * (s * kqq1[q] * (-2.0 * uqq[q] / l));
    o.g_out[0] = (trOm + trMA) * in.d1[0]; o.g_out[1] = g_s / s * in.d1[1]; o.g_out[2] = g_l * in.d1[2];
    o.W_ss.resize((size_t)n * n); o.W_qs.resize((size_t)m * n); o.W_qq.resize((size_t)m * m);
    for (size_t q = 0; q < (size_t)n * n; ++q) o.W_ss[q] = M_A[q] * s * in.k1[q] * il2;
    for (size_t q = 0; q < (size_t)m * n; ++q) o.W_qs[q] = M_B[q] * s * kqs1[q] * il2;
    for (size_t q = 0; q < (size_t)m * m; ++q) o.W_qq[q] = Om[q] * s * kqq1[q] * il2;
    return o;
}

// oracle/closed_form.py::mixed_stage
Mat mixed_stage(const double* v, const Inner& in) {
    const int n = in.n;
    const double noise = in.noise, s = in.s, l = in.l, il2 = 1.0 / (l * l);
    const double cn = v[0] * in.d1[0], cs = v[1] * in.d1[1] / s, cl = v[2] * in.d1[2];
    Mat X((size_t)n * n);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) {
        const size_t e = (size_t)i * n + j;
        X[e] = cn * in.Ainv[e] + cs * ((i == j ? 1.0 : 0.0) - noise * in.Ainv[e]) + cl * in.P[e];
    }
    std::vector<double> w(n);
    for (int i = 0; i < n; ++i) w[i] = cn * in.gamma[i] + cs * (in.alpha[i] - noise * in.gamma[i]) + cl * in.delta[i];
    Mat XA = matmul(X, n, n, in.Ainv, n);
    Mat W((size_t)n * n);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) {
        const size_t e = (size_t)i * n + j;
        const double dg_dA = (-0.5 * XA[e] + 0.5 * (w[i] * in.alpha[j] + in.alpha[i] * w[j])) / n;
        const double Q = 0.5 * (in.Ainv[e] - in.alpha[i] * in.alpha[j]) / n;
        const double dBv_du = cs * s * in.k1[e] + cl * s * (-2.0 / l) * (in.k1[e] + in.u[e] * in.k2[e]);
        W[e] = dg_dA * s * in.k1[e] * il2 + Q * dBv_du * il2;
    }
    return W;
}

// oracle/closed_form.py::dz_from_weights: D2_ij = |z_i - z_j|^2
void dz_from_weights(const float* Zs, int n, const float* Zq, int m, int d, const Mat* W_ss, const Mat* W_qs, const Mat* W_qq,
                     float* dZs, float* dZq, int ld_d) {
    (void)ld_d;
    if (dZs) {
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < d; ++k) {
                double s = 0.0;
                if (W_ss) for (int j = 0; j < n; ++j) s += 2.0 * ((*W_ss)[(size_t)i * n + j] + (*W_ss)[(size_t)j * n + i]) * ((double)Zs[(size_t)i * d + k] - (double)Zs[(size_t)j * d + k]);
                if (W_qs) for (int p = 0; p < m; ++p) s += 2.0 * (*W_qs)[(size_t)p * n + i] * ((double)Zs[(size_t)i * d + k] - (double)Zq[(size_t)p * d + k]);
                dZs[(size_t)i * d + k] = (float)s;
            }
    }
    if (dZq) {
        for (int p = 0; p < m; ++p)
            for (int k = 0; k < d; ++k) {
                double s = 0.0;
                if (W_qs) for (int j = 0; j < n; ++j) s += 2.0 * (*W_qs)[(size_t)p * n + j] * ((double)Zq[(size_t)p * d + k] - (double)Zs[(size_t)j * d + k]);
                if (W_qq) for (int q = 0; q < m; ++q) s += 2.0 * ((*W_qq)[(size_t)p * m + q] + (*W_qq)[(size_t)q * m + p]) * ((double)Zq[(size_t)p * d + k] - (double)Zq[(size_t)q * d + k]);
                dZq[(size_t)p * d + k] = (float)s;
            }
    }
}

bool solve3(const double* H, const double* b, double* x) {   // partial pivoting
    double a[3][4];
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) a[i][j] = H[i * 3 + j]; a[i][3] = b[i]; }
    for (int c = 0; c < 3; ++c) {
        int p = c;
        for (int r = c + 1; r < 3; ++r) if (std::fabs(a[r][c]) > std::fabs(a[p][c])) p = r;
        if (a[p][c] == 0.0) return false;
        if (p != c) for (int j = 0; j < 4; ++j) std::swap(a[p][j], a[c][j]);
        for (int r = c + 1; r < 3; ++r) { const double f = a[r][c] / a[c][c]; for (int j = c; j < 4; ++j) a[r][j] -= f * a[c][j]; }
    }
    for (int r = 2; r >= 0; --r) { double s = a[r][3]; for (int j = r + 1; j < 3; ++j) s -= a[r][j] * x[j]; x[r] = s / a[r][r]; }
    return true;
}

double median_l0(const Mat& D2, int n) {
    std::vector<double> v;
    v.reserve((size_t)n * (n - 1) / 2);
    for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) { const double x = (double)(float)D2[(size_t)i * n + j]; if (x > 0.0) v.push_back(x); }
    if (v.empty()) return 0.0;
    const size_t k = (v.size() - 1) / 2;
    std::nth_element(v.begin(), v.begin() + k, v.end());
    return std::sqrt(0.5 * v[k]);
}

int check(const adkf_batch_t* b, bool need_q, bool ard_ok = false) {
    if (!b || b->T <= 0 || b->ns_max <= 0 || b->nq_max < 0 || b->d <= 0 || !b->Z_s) return ADKF_E_BADARG;
    if (b->kernel != ADKF_KERNEL_RBF && b->kernel != ADKF_KERNEL_MATERN52) return ADKF_E_BADARG;
    if (!ard_ok && (b->flags & ADKF_BATCH_ARD)) return ADKF_E_BADARG;
    if (need_q && (b->nq_max <= 0 || !b->Z_q)) return ADKF_E_BADARG;
    return 0;
}
inline int ns_of(const adkf_batch_t* b, int t) { return b->n_s ? b->n_s[t] : b->ns_max; }

// log h(u), h(u) = phi(u) + u Phi(u) (ADKF_PM_LOG_EI): through erfc down to u = -8; below that, with a = -u,
// h(u) = phi(u) a^-2 (1 - 3 a^-2 + 15 a^-4 - ...), the asymptotic series summed while its terms shrink (the smallest is below
// 2e-13 at a = 8)
double log_h(double u) {
    if (u > -8.0) return std::log(std::exp(-0.5 * u * u) / std::sqrt(2.0 * M_PI) + u * 0.5 * std::erfc(-u / std::sqrt(2.0)));
    const double w = 1.0 / (u * u);
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 64; ++k) {
        const double next = -term * (2 * k + 1) * w;
        if (std::fabs(next) >= std::fabs(term)) break;
        sum += term = next;
    }
    return -0.5 * u * u - 0.5 * std::log(2.0 * M_PI) + std::log(w) + std::log(sum);
}

// EI (ADKF_PM_LOG_EI: log EI) of a row from its mean and latent variance
float pm_ei(double mu, double vl, double bf, int flags) {
    const double sg = std::sqrt(std::max(vl, 1e-12));
    const double u = ((flags & ADKF_PM_MAXIMIZE) ? (mu - bf) : (bf - mu)) / sg;
    if (flags & ADKF_PM_LOG_EI) return (float)(std::log(sg) + log_h(u));
    return (float)(sg * (u * 0.5 * std::erfc(-u / std::sqrt(2.0)) + std::exp(-0.5 * u * u) / std::sqrt(2.0 * M_PI)));
}

// The posterior of one row from its squared distances D [n] to the support set of a task: k = s kappa(D / l^2) into kr [n] (row_k),
// c = k A^-1 into c [n] unless it is null, mu = c . y and q = c . k (the latent variance is s - q).  The only place that forms them;
// the variance clamp, ADKF_PM_LATENT and the noise stay with the callers.
inline void row_k(const Inner& in, int kind, const double* D, double* kr) {
    const double il2 = 1.0 / (in.l * in.l);
    for (int j = 0; j < in.n; ++j) { double k0, k1, k2; kappa(kind, D[j] * il2, k0, k1, k2); kr[j] = in.s * k0; }
}
struct MuQ { double mu, q; };
MuQ row_posterior(const Inner& in, int kind, const double* D, const float* y, double* kr, double* c) {
    const int n = in.n;
    row_k(in, kind, D, kr);
    double mu = 0.0, q = 0.0;
    for (int j = 0; j < n; ++j) {
        double cj = 0.0;
        for (int i = 0; i < n; ++i) cj += kr[i] * in.Ainv[(size_t)i * n + j];
        if (c) c[j] = cj;
        mu += cj * (double)y[j];
        q += cj * kr[j];
    }
    return {mu, q};
}

// adkf_predict_marginal(_ard): mean, variance and EI (ADKF_PM_LOG_EI: log EI) of row r from its squared distances D [n] to the
// support set of a task
void pm_row(const Inner& in, int kind, const double* D, const float* y, int flags, const float* best_f, int t, int64_t r, float* mean,
            float* var, float* ei) {
    std::vector<double> k(in.n);
    const MuQ p = row_posterior(in, kind, D, y, k.data(), nullptr);
    const double vl = in.s - p.q;
    mean[r] = (float)p.mu;
    if (var) var[r] = (float)((flags & ADKF_PM_LATENT) ? vl : vl + in.noise);
    if (ei) ei[r] = pm_ei(p.mu, vl, best_f[t], flags);
}

// What every streaming entry prepares of a task: inner_stage on the support set.  ARD: on z~ = (z - mu) / l with mu the support column
// mean and l = softplus(raw_lengthscale) per dimension, at unit lengthscale (phi3 = (raw_noise, raw_outputscale, softplus^-1(1)),
// no lengthscale prior), as csrc/ard.h does; otherwise mu = 0 and l = 1, which change no bit.  mean: the support column mean, for
// ARD batches and where with_mean asks for it (Thompson centres its random features with it in both kinds); otherwise 0.
struct TaskPrep {
    int n = 0;
    std::vector<double> mean, mu, l;   // mu, l: the centring and the scaling of the distance operands
    Mat Zt;                            // the support rows, centred and scaled
    Inner in;
};
// Sets info[t]; false when there is nothing to evaluate (n_s == 0 or info != 0).
bool prepare_task(const adkf_batch_t* b, const float* phi, int t, bool with_mean, int32_t* info, TaskPrep& p) {
    const bool ard = (b->flags & ADKF_BATCH_ARD) != 0;
    const int d = b->d, n = p.n = std::min(ns_of(b, t), b->ns_max);
    info[t] = 0;
    if (n <= 0) return false;
    const float* Zs = b->Z_s + (size_t)t * b->ns_max * d;
    const float* x = phi + (size_t)t * (ard ? 2 + d : 3);
    p.mean.assign(d, 0.0); p.l.assign(d, 1.0);
    if (ard || with_mean) {
        for (int i = 0; i < n; ++i) for (int c = 0; c < d; ++c) p.mean[c] += Zs[(size_t)i * d + c];
        for (int c = 0; c < d; ++c) p.mean[c] /= n;
    }
    if (ard) for (int c = 0; c < d; ++c) p.l[c] = softplus(x[2 + c]);
    p.mu = ard ? p.mean : std::vector<double>(d, 0.0);
    p.Zt.resize((size_t)n * d);
    for (int i = 0; i < n; ++i) for (int c = 0; c < d; ++c) p.Zt[(size_t)i * d + c] = ((double)Zs[(size_t)i * d + c] - p.mu[c]) / p.l[c];
    const double x3[3] = {x[0], x[1], ard ? std::log(std::expm1(1.0)) : (double)x[2]};
    const float pri[4] = {b->priors[t * 4], b->priors[t * 4 + 1], ard ? 0.f : b->priors[t * 4 + 2], ard ? -1.f : b->priors[t * 4 + 3]};
    p.in = inner_stage(sqdist(p.Zt.data(), n, p.Zt.data(), n, d), b->y_s + (size_t)t * b->ns_max, n, x3, pri, b->kernel, false, false);
    info[t] = p.in.info;
    return p.in.info == 0;
}
// the squared distances [n] of the row x [d] to the prepared support set
Mat task_row_dist(const TaskPrep& p, const float* x, int d) {
    std::vector<double> zt(d);
    for (int c = 0; c < d; ++c) zt[c] = ((double)x[c] - p.mu[c]) / p.l[c];
    return sqdist(zt.data(), 1, p.Zt.data(), p.n, d);
}

// One task of adkf_predict_marginal(_ard) and of every pool entry but Thompson's: prepare_task, then row(r, in, D) for the rows
// lo <= r < hi of Zq, D [n] the squared distances of row r to the support set.  Sets info[t]; false when no row was evaluated
// (n_s == 0 or info != 0).
// state(in): called once per evaluated task before its rows (adkf_jackknife_pool: the leave-one-out state, with or without rows).
template <class STATE, class ROW>
bool pm_task_state(const adkf_batch_t* b, const float* phi, int t, const float* Zq, int64_t lo, int64_t hi, int32_t* info, STATE state, ROW row) {
    TaskPrep p;
    if (!prepare_task(b, phi, t, false, info, p)) return false;
    state(p.in);
    for (int64_t r = lo; r < hi; ++r) row(r, p.in, task_row_dist(p, Zq + (size_t)r * b->d, b->d).data());
    return true;
}
template <class ROW>
bool pm_task(const adkf_batch_t* b, const float* phi, int t, const float* Zq, int64_t lo, int64_t hi, int32_t* info, ROW row) {
    return pm_task_state(b, phi, t, Zq, lo, hi, info, [](const Inner&) {}, row);
}

// ---- The pool kit: what the entries over a shared pool have in common.  An entry writes its own flags and arguments, its fills and its
// arithmetic per row; the rest is here:
//   check_support_only, pool_args_ok   every entry (named as in csrc/host_stream.h); check_topk: those with a top-k selection
//   row_posterior (above)              pm_row (predict_marginal, predict_pool, gumbel, mix), mes, jackknife, ehvi, and pool_state
//   PoolState, pool_state, c0_col      believer / gibbon, kg, ipv, jes: K, K A^-1, mean and latent variance of every row, c0(x_r, x_p)
//   excl_range (Excl::has)             select_topk, greedy_pick and Thompson's per-row test
//   init_topk, select_topk             predict_pool, mes, kg, jes, jackknife, ehvi and mix (per group), rank (alone without check_topk's cap); init_topk also the sel_* fills
//   greedy_pick, append_pick           believer / gibbon / liar (step j) and ipv (pick c)
//   valid_entry                        kg (references) and ipv (targets)
//   prepare_task, task_row_dist        pm_task_state and PathDraws (thompson_pool, qei_pool)
enum { ARD_EITHER = -1 };   // check_support_only's ard_mode; 0 / 1: the batch must not / must be an ARD batch
int check_support_only(const adkf_batch_t* b, const float* phi, const int32_t* info, int64_t rows, int ard_mode) {
    if (int rc = check(b, false, ard_mode != 0)) return rc;
    const bool kind_ok = ard_mode == ARD_EITHER || ((b->flags & ADKF_BATCH_ARD) != 0) == (ard_mode != 0);
    if (!kind_ok || b->nq_max != 0 || b->Z_q || b->y_q) return ADKF_E_BADARG;
    if (!phi || !info || !b->y_s || !b->priors || rows < 0) return ADKF_E_BADARG;
    return 0;
}
// a pool where there are rows, and exclusion lists only with their offsets
inline bool pool_args_ok(const float* X, int64_t rows, const int64_t* excl_idx, const int64_t* excl_off) {
    return !(rows > 0 && !X) && !(excl_idx && !excl_off);
}
// the selection of k rows per task: k itself and the two outputs it needs
inline int check_topk(int k, const int64_t* top_idx, const float* top_val) {
    if (k < 0 || (k > 0 && (!top_idx || !top_val))) return ADKF_E_BADARG;
    return k > ADKF_POOL_TOPK_MAX ? ADKF_E_SIZE : 0;
}

// the sorted exclusion list of task (group) t
struct Excl {
    const int64_t *lo = nullptr, *hi = nullptr;
    bool has(int64_t r) const { return lo && std::binary_search(lo, hi, r); }
};
inline Excl excl_range(const int64_t* excl_idx, const int64_t* excl_off, int t) {
    return excl_idx ? Excl{excl_idx + excl_off[t], excl_idx + excl_off[t + 1]} : Excl{};
}
// the k slots of task (group) t before anything is selected: -1 / -inf
inline void init_topk(int64_t* top_idx, float* top_val, int t, int k) {
    for (int q = 0; q < k; ++q) { top_idx[(size_t)t * k + q] = -1; top_val[(size_t)t * k + q] = -std::numeric_limits<float>::infinity(); }
}
// The selection of every pool entry: the k eligible rows (not NaN, not excluded) under the total order "larger score first, equal
// scores by ascending row"; slots beyond the eligible rows keep what init_topk wrote.
void select_topk(const std::vector<float>& sc, int64_t rows, int k, const Excl& excl, int64_t* top_idx, float* top_val) {
    std::vector<int64_t> cand;
    for (int64_t r = 0; r < rows; ++r)
        if (sc[r] == sc[r] && !excl.has(r)) cand.push_back(r);
    const size_t kk = std::min<size_t>(k, cand.size());
    std::partial_sort(cand.begin(), cand.begin() + kk, cand.end(), [&](int64_t a, int64_t c) { return sc[a] > sc[c] || (sc[a] == sc[c] && a < c); });
    for (size_t q = 0; q < kk; ++q) { top_idx[q] = cand[q]; top_val[q] = sc[cand[q]]; }
}
// One step of a greedy batch: the row of largest score among those not NaN, not taken and not excluded, the lower index on a tie; -1
// when there is none
int64_t greedy_pick(const std::vector<float>& score, int64_t rows, const std::vector<char>& taken, const Excl& excl) {
    int64_t p = -1;
    for (int64_t r = 0; r < rows; ++r) {
        if (score[r] != score[r] || taken[r] || excl.has(r)) continue;
        if (p < 0 || score[r] > score[p]) p = r;   // (rows ascend: a tie keeps the lower index)
    }
    return p;
}
// entry j of idx when it is a row of the pool and its first occurrence, else -1
int64_t valid_entry(const int64_t* idx, int j, int64_t rows) {
    const int64_t p = idx[j];
    if (p < 0 || p >= rows) return -1;
    for (int i = 0; i < j; ++i) if (idx[i] == p) return -1;
    return p;
}

// The state of a task over the whole pool: K [R, n], K A^-1 [R, n], the mean and the latent variance of every row, and for ARD batches
// the pool rows over l (the distances between pool rows are taken on x / l: mu cancels).
struct PoolState {
    int n = 0;
    size_t R = 0;
    double s = 0.0, noise = 0.0, il2 = 0.0;
    Mat Kr, Cr, mu, v, Xl;
};
// through pm_task; false when no row was evaluated
bool pool_state(const adkf_batch_t* b, const float* phi, int t, const float* X, int64_t rows, int32_t* info, PoolState& st) {
    const int n = st.n = std::min(ns_of(b, t), b->ns_max), d = b->d;
    const size_t R = st.R = (size_t)rows;
    st.Kr.resize(R * std::max(n, 0)); st.Cr.resize(R * std::max(n, 0)); st.mu.resize(R); st.v.resize(R);
    const float* y = b->y_s + (size_t)t * b->ns_max;
    const bool done = pm_task(b, phi, t, X, 0, rows, info, [&](int64_t r, const Inner& in, const double* D) {
        st.s = in.s; st.noise = in.noise; st.il2 = 1.0 / (in.l * in.l);
        const MuQ p = row_posterior(in, b->kernel, D, y, &st.Kr[(size_t)r * n], &st.Cr[(size_t)r * n]);
        st.mu[r] = p.mu; st.v[r] = in.s - p.q;
    });
    if (done && (b->flags & ADKF_BATCH_ARD)) {
        const float* x0 = phi + (size_t)t * (2 + d);
        st.Xl.resize(R * d);
        for (size_t r = 0; r < R; ++r) for (int c = 0; c < d; ++c) st.Xl[r * d + c] = (double)X[r * d + c] / softplus(x0[2 + c]);
    }
    return done;
}
// c0(x_r, x_p), the posterior covariance of row p with every row r, into out [R]
void c0_col(const PoolState& st, const adkf_batch_t* b, const float* X, int64_t p, double* out) {
    const int n = st.n, d = b->d;
    const Mat Dp = (b->flags & ADKF_BATCH_ARD) ? sqdist(st.Xl.data() + (size_t)p * d, 1, st.Xl.data(), (int)st.R, d) : sqdist(X + (size_t)p * d, 1, X, (int)st.R, d);
    for (size_t r = 0; r < st.R; ++r) {
        double k0, k1, k2;
        kappa(b->kernel, Dp[r] * st.il2, k0, k1, k2);
        double c0 = st.s * k0;
        for (int i = 0; i < n; ++i) c0 -= st.Kr[r * n + i] * st.Cr[(size_t)p * n + i];
        out[r] = c0;
    }
}
// Row p joins a greedy batch as its entry c (of at most q): the new row of G, column c of ell for every row (the forward substitution
// of the header, one row of G at a time; col [R] is scratch) and the downdate of every row's variance, the picked one included.
void append_pick(PoolState& st, const adkf_batch_t* b, const float* X, int64_t p, int c, int q, Mat& G, Mat& L, Mat& col) {
    for (int l = 0; l < c; ++l) G[(size_t)c * q + l] = L[(size_t)p * q + l];
    G[(size_t)c * q + c] = std::sqrt(st.v[p] + st.noise);
    c0_col(st, b, X, p, col.data());
    for (size_t r = 0; r < st.R; ++r) {
        double c0 = col[r];
        for (int l = 0; l < c; ++l) c0 -= G[(size_t)c * q + l] * L[r * q + l];
        const double e = c0 / G[(size_t)c * q + c];
        L[r * q + c] = e;
        st.v[r] -= e * e;
    }
}

int predict_marginal(bool ard, const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows,
                     const float* best_f, float* mean, float* var, float* ei, int32_t* info) {
    if (int rc = check_support_only(b, phi, info, rows, ard)) return rc;
    if (!q_off) return ADKF_E_BADARG;
    if (rows > 0 && (!Zq || !mean)) return ADKF_E_BADARG;
    if (ei && !best_f) return ADKF_E_BADARG;
    if (flags & ~(ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    if ((flags & ADKF_PM_LOG_EI) && !ei) return ADKF_E_BADARG;
    // rows outside every task's range and those of tasks with n_s == 0 or info != 0 stay 0 (as on the GPU)
    if (rows > 0) {
        std::fill(mean, mean + rows, 0.f);
        if (var) std::fill(var, var + rows, 0.f);
        if (ei) std::fill(ei, ei + rows, 0.f);
    }
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const int64_t lo = std::min(std::max<int64_t>(q_off[t], 0), rows), hi = std::min(std::max<int64_t>(q_off[t + 1], lo), rows);
        pm_task(b, phi, t, Zq, lo, hi, info, [&](int64_t r, const Inner& in, const double* D) {
            pm_row(in, b->kernel, D, b->y_s + (size_t)t * b->ns_max, flags, best_f, t, r, mean, var, ei);
        });
    }
    return 0;
}
// Phi(u) / h(u) and phi(u) / h(u), h(u) = phi(u) + u Phi(u): the two ratios behind the derivatives of log EI.  Directly while
// h keeps its digits in float64 (u > -20: the cancellation costs a^2 eps); below, with a = -u, h = phi b(a) and Phi = phi (1 - b) / a
// from the series of log_h.
void ei_ratios(double u, double& cdf_h, double& pdf_h) {
    if (u > -20.0) {
        const double cdf = 0.5 * std::erfc(-u / std::sqrt(2.0)), pdf = std::exp(-0.5 * u * u) / std::sqrt(2.0 * M_PI);
        const double h = pdf + u * cdf;
        cdf_h = cdf / h; pdf_h = pdf / h;
        return;
    }
    const double a = -u, w = 1.0 / (a * a);
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 64; ++k) {
        const double next = -term * (2 * k + 1) * w;
        if (std::fabs(next) >= std::fabs(term)) break;
        sum += term = next;
    }
    const double bb = w * sum;
    pdf_h = 1.0 / bb; cdf_h = (1.0 - bb) / (a * bb);
}

// adkf_predict_grad: the coefficients a_m = d(sum of cotangent x output) / d mean and a_v = the same by the latent variance of a row
// (include/adkf_gp.h).  Where the variance clamp is active the derivative through sigma is 0.
struct GradCoef { double am, av; };
GradCoef grad_coef(double mu, double vl, double bf, int flags, double gm, double gv, double ge, bool with_ei) {
    GradCoef c{gm, gv};
    if (!with_ei) return c;
    const bool live = vl > 1e-12;
    const double sg = std::sqrt(std::max(vl, 1e-12)), sgn = (flags & ADKF_PM_MAXIMIZE) ? 1.0 : -1.0;
    const double u = sgn * (mu - bf) / sg;
    if (flags & ADKF_PM_LOG_EI) {
        double ch, ph;
        ei_ratios(u, ch, ph);
        c.am += ge * sgn * ch / sg;
        if (live) c.av += ge * ph / (2.0 * vl);
    } else {
        c.am += ge * sgn * 0.5 * std::erfc(-u / std::sqrt(2.0));
        if (live) c.av += ge * std::exp(-0.5 * u * u) / std::sqrt(2.0 * M_PI) / (2.0 * sg);
    }
    return c;
}

// adkf_predict_grad: dZq [rows, d] = the vector-Jacobian product of streaming prediction by the packed rows, in float64 on the scaled
// features of prepare_task, rounded once.
int predict_grad(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows,
                 const float* best_f, const float* g_mean, const float* g_var, const float* g_ei, float* dZq, int32_t* info) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (!q_off) return ADKF_E_BADARG;
    if (rows > 0 && (!Zq || !dZq)) return ADKF_E_BADARG;
    if (!g_mean && !g_var && !g_ei) return ADKF_E_BADARG;
    if (g_ei && !best_f) return ADKF_E_BADARG;
    if (flags & ~(ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    if ((flags & ADKF_PM_LOG_EI) && !g_ei) return ADKF_E_BADARG;
    const int d = b->d;
    if (rows > 0) std::fill(dZq, dZq + (size_t)rows * d, 0.f);
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const int64_t lo = std::min(std::max<int64_t>(q_off[t], 0), rows), hi = std::min(std::max<int64_t>(q_off[t + 1], lo), rows);
        TaskPrep p;
        if (!prepare_task(b, phi, t, false, info, p)) continue;
        const Inner& in = p.in;
        const int n = in.n;
        const float* y = b->y_s + (size_t)t * b->ns_max;
        const double il2 = 1.0 / (in.l * in.l);
        std::vector<double> kr(n), c(n), zt(d), W(n);
        for (int64_t r = lo; r < hi; ++r) {
            const float* x = Zq + (size_t)r * d;
            for (int q = 0; q < d; ++q) zt[q] = ((double)x[q] - p.mu[q]) / p.l[q];
            const Mat D = sqdist(zt.data(), 1, p.Zt.data(), n, d);
            const MuQ pq = row_posterior(in, b->kernel, D.data(), y, kr.data(), c.data());
            const GradCoef gc = grad_coef(pq.mu, in.s - pq.q, g_ei ? best_f[t] : 0.0, flags, g_mean ? g_mean[r] : 0.0, g_var ? g_var[r] : 0.0,
                                          g_ei ? g_ei[r] : 0.0, g_ei != nullptr);
            for (int i = 0; i < n; ++i) {
                double k0, k1, k2;
                kappa(b->kernel, D[i] * il2, k0, k1, k2);
                W[i] = in.s * k1 * (gc.am * in.alpha[i] - 2.0 * gc.av * c[i]);
            }
            for (int q = 0; q < d; ++q) {
                double s = 0.0;
                for (int i = 0; i < n; ++i) s += W[i] * (zt[q] - p.Zt[(size_t)i * d + q]);
                dZq[(size_t)r * d + q] = (float)(2.0 * il2 * s / p.l[q]);
            }
        }
    }
    return 0;
}
inline int nq_of(const adkf_batch_t* b, int t) { return b->n_q ? b->n_q[t] : b->nq_max; }

// The quasi-Newton driver of csrc/inner.h (Bfgs + fit_advance), in float64.
struct Bfgs {
    double x[3], f, g[3], Hi[3][3], p[3], gp, step; int bt; bool first;
    void reset_H() { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Hi[i][j] = i == j; first = true; }
    bool direction() {
        for (int i = 0; i < 3; ++i) p[i] = -(Hi[i][0] * g[0] + Hi[i][1] * g[1] + Hi[i][2] * g[2]);
        gp = g[0] * p[0] + g[1] * p[1] + g[2] * p[2];
        if (!(gp < 0.0)) { reset_H(); for (int i = 0; i < 3; ++i) p[i] = -g[i]; gp = -(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]); if (!(gp < 0.0)) return false; }
        step = first ? std::min(1.0, 1.0 / (std::fabs(g[0]) + std::fabs(g[1]) + std::fabs(g[2]))) : 1.0;
        step = std::min(step, 16.0 / std::max(std::max(std::fabs(p[0]), std::fabs(p[1])), std::max(std::fabs(p[2]), 1e-30)));
        bt = 0;
        return true;
    }
    void accept(const double* xn, double fn, const double* gn) {
        double s[3], yv[3];
        for (int i = 0; i < 3; ++i) { s[i] = xn[i] - x[i]; yv[i] = gn[i] - g[i]; x[i] = xn[i]; g[i] = gn[i]; }
        f = fn;
        const double sy = s[0] * yv[0] + s[1] * yv[1] + s[2] * yv[2], yy = yv[0] * yv[0] + yv[1] * yv[1] + yv[2] * yv[2], ss = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
        if (sy > 1e-10 * std::sqrt(ss * yy) && yy > 0.0) {
            if (first) { const double sc = sy / yy; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Hi[i][j] = i == j ? sc : 0.0; first = false; }
            const double rho = 1.0 / sy;
            double Hy[3];
            for (int i = 0; i < 3; ++i) Hy[i] = Hi[i][0] * yv[0] + Hi[i][1] * yv[1] + Hi[i][2] * yv[2];
            const double yHy = yv[0] * Hy[0] + yv[1] * Hy[1] + yv[2] * Hy[2];
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Hi[i][j] += -rho * (s[i] * Hy[j] + Hy[i] * s[j]) + rho * (rho * yHy + 1.0) * s[i] * s[j];
        }
    }
};

}  // namespace

extern "C" {

const char* adkf_version(void) { return "adkf_gp_cpu 0.1 (float64 inside, OpenMP over tasks)"; }
const char* adkf_last_hip_error(void) { return "no HIP in the CPU twin"; }
int adkf_max_points(void) { return 1 << 20; }
size_t adkf_workspace_bytes(int32_t, int32_t, int32_t, int32_t) { return 0; }

int adkf_median_lengthscale(const adkf_batch_t* b, float* l0, void*, size_t, void*) {
    if (int rc = check(b, false)) return rc;
    if (!l0) return ADKF_E_BADARG;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const int n = ns_of(b, t);
        const float* Z = b->Z_s + (size_t)t * b->ns_max * b->d;
        l0[t] = n > 1 ? (float)median_l0(sqdist(Z, n, Z, n, b->d), n) : 0.f;
    }
    return 0;
}

int adkf_init_params(const adkf_batch_t* b, int32_t numeric, int32_t use_ls_prior, float* phi, float* priors, float* l0, void*, size_t, void*) {
    if (int rc = check(b, false)) return rc;
    if (!phi || !priors) return ADKF_E_BADARG;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const int n = ns_of(b, t);
        const float* Z = b->Z_s + (size_t)t * b->ns_max * b->d;
        const float l = n > 1 ? (float)median_l0(sqdist(Z, n, Z, n, b->d), n) : 0.f;
        if (l0) l0[t] = l;
        const double scale = 0.25, mode = numeric ? 0.01 : 0.1;
        phi[t * 3 + 0] = (float)inv_softplus(mode - NOISE_LB); phi[t * 3 + 1] = 0.f; phi[t * 3 + 2] = (float)inv_softplus((double)l);
        priors[t * 4 + 0] = (float)(std::log(mode) + scale * scale); priors[t * 4 + 1] = (float)scale;
        priors[t * 4 + 2] = use_ls_prior ? (float)(std::log((double)l) + scale * scale) : 0.f; priors[t * 4 + 3] = use_ls_prior ? (float)scale : -1.f;
    }
    return 0;
}

int adkf_mll_value_grad(const adkf_batch_t* b, const float* phi, float* f_in, float* g_phi, float* dZ_s, int32_t* info, void*, size_t, void*) {
    if (int rc = check(b, false)) return rc;
    if (!phi || !f_in || !info || !b->y_s || !b->priors) return ADKF_E_BADARG;
    const int d = b->d;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const int n = ns_of(b, t);
        const float* Z = b->Z_s + (size_t)t * b->ns_max * d;
        const double p[3] = {phi[t * 3], phi[t * 3 + 1], phi[t * 3 + 2]};
        Inner in = inner_stage(sqdist(Z, n, Z, n, d), b->y_s + (size_t)t * b->ns_max, n, p, b->priors + t * 4, b->kernel, false, true);
        info[t] = in.info; f_in[t] = (float)in.f_in;
        if (g_phi) for (int q = 0; q < 3; ++q) g_phi[t * 3 + q] = (float)in.g_in[q];
        if (dZ_s) {
            float* out = dZ_s + (size_t)t * b->ns_max * d;
            std::memset(out, 0, sizeof(float) * (size_t)b->ns_max * d);
            if (!in.info) {
                Mat W((size_t)n * n);
                const double il2 = 1.0 / (in.l * in.l);
                for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { const size_t e = (size_t)i * n + j; W[e] = 0.5 * (in.Ainv[e] - in.alpha[i] * in.alpha[j]) / n * in.s * in.k1[e] * il2; }
                dz_from_weights(Z, n, nullptr, 0, d, &W, nullptr, nullptr, out, nullptr, d);
            }
        }
    }
    return 0;
}

int adkf_fit(const adkf_batch_t* b, float* phi, const adkf_fit_options_t* opt, float* f_final, float* gnorm, int32_t* n_evals, int32_t* info,
             void*, size_t, void*) {
    if (int rc = check(b, false)) return rc;
    if (!phi || !opt || !info || !b->y_s || !b->priors || opt->max_evals < 1) return ADKF_E_BADARG;
    const int d = b->d;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const int n = ns_of(b, t);
        const float* Z = b->Z_s + (size_t)t * b->ns_max * d;
        const Mat D2 = sqdist(Z, n, Z, n, d);
        const float* y = b->y_s + (size_t)t * b->ns_max;
        const float* pri = b->priors + t * 4;
        auto eval = [&](const double* x, double& f, double* g) { Inner in = inner_stage(D2, y, n, x, pri, b->kernel, false, false); f = in.f_in; for (int q = 0; q < 3; ++q) g[q] = in.g_in[q]; return in.info; };
        Bfgs st;
        for (int q = 0; q < 3; ++q) st.x[q] = phi[t * 3 + q];
        st.reset_H();
        double xe[3] = {st.x[0], st.x[1], st.x[2]}, fe, ge[3];
        int evals = 0, ie = eval(xe, fe, ge);
        ++evals;
        st.f = fe; for (int q = 0; q < 3; ++q) st.g[q] = ge[q];
        const int budget = opt->max_evals - 1;
        bool stop = ie != 0 || std::max(std::fabs(ge[0]), std::max(std::fabs(ge[1]), std::fabs(ge[2]))) <= opt->gtol || !st.direction();
        while (!stop && evals < budget) {
            for (int q = 0; q < 3; ++q) xe[q] = st.x[q] + st.step * st.p[q];
            ie = eval(xe, fe, ge);
            ++evals;
            if (ie == 0 && fe <= st.f + 1e-4 * st.step * st.gp) {
                const double fprev = st.f;
                st.accept(xe, fe, ge);
                const double gmax = std::max(std::fabs(ge[0]), std::max(std::fabs(ge[1]), std::fabs(ge[2])));
                if (gmax <= opt->gtol || std::fabs(fprev - fe) <= opt->ftol * std::max(std::max(std::fabs(fprev), std::fabs(fe)), 1.0)) stop = true;
                else if (!st.direction()) stop = true;
            } else {
                const double denom = 2.0 * (fe - st.f - st.gp * st.step);
                const double sq = (denom > 0.0 && std::isfinite(fe)) ? (-st.gp * st.step * st.step / denom) : 0.5 * st.step;
                st.step = std::min(std::max(sq, 0.1 * st.step), 0.5 * st.step);
                if (++st.bt >= 12) stop = true;
            }
        }
        double ff, gf[3];
        const int inf = eval(st.x, ff, gf);     // the output evaluation at the accepted point
        ++evals;
        for (int q = 0; q < 3; ++q) phi[t * 3 + q] = (float)st.x[q];
        info[t] = inf;
        if (f_final) f_final[t] = (float)ff;
        if (gnorm) gnorm[t] = (float)std::max(std::fabs(gf[0]), std::max(std::fabs(gf[1]), std::fabs(gf[2])));
        if (n_evals) n_evals[t] = opt->exact_evals ? opt->max_evals : evals;
    }
    return 0;
}

int adkf_predict(const adkf_batch_t* b, const float* phi, float* mean, float* var, float* cov, int32_t* info, void*, size_t, void*) {
    if (int rc = check(b, true)) return rc;
    if (!phi || !mean || !info || !b->y_s || !b->priors) return ADKF_E_BADARG;
    const int d = b->d;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const int n = ns_of(b, t), m = nq_of(b, t);
        const float *Zs = b->Z_s + (size_t)t * b->ns_max * d, *Zq = b->Z_q + (size_t)t * b->nq_max * d;
        const double p[3] = {phi[t * 3], phi[t * 3 + 1], phi[t * 3 + 2]};
        Inner in = inner_stage(sqdist(Zs, n, Zs, n, d), b->y_s + (size_t)t * b->ns_max, n, p, b->priors + t * 4, b->kernel, false, false);
        info[t] = in.info;
        float* mu = mean + (size_t)t * b->nq_max;
        std::fill(mu, mu + b->nq_max, 0.f);
        if (var) std::fill(var + (size_t)t * b->nq_max, var + (size_t)(t + 1) * b->nq_max, 0.f);
        if (cov) std::fill(cov + (size_t)t * b->nq_max * b->nq_max, cov + (size_t)(t + 1) * b->nq_max * b->nq_max, 0.f);
        if (in.info) continue;
        Outer o = outer_stage(sqdist(Zq, m, Zs, n, d), sqdist(Zq, m, Zq, m, d), nullptr, m, in, b->kernel, false);
        for (int i = 0; i < m; ++i) {
            mu[i] = (float)o.mean[i];
            if (var) var[(size_t)t * b->nq_max + i] = (float)o.S[(size_t)i * m + i];
            if (cov) for (int j = 0; j < m; ++j) cov[((size_t)t * b->nq_max + i) * b->nq_max + j] = (float)o.S[(size_t)i * m + j];
        }
    }
    return 0;
}

int adkf_predict_marginal(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows,
                          const float* best_f, float* mean, float* var, float* ei, int32_t* info, void*, size_t, void*) {
    return predict_marginal(false, b, phi, flags, Zq, q_off, rows, best_f, mean, var, ei, info);
}

int adkf_predict_grad(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows,
                      const float* best_f, const float* g_mean, const float* g_var, const float* g_ei, float* dZq, int32_t* info, void*, size_t, void*) {
    return predict_grad(b, phi, flags, Zq, q_off, rows, best_f, g_mean, g_var, g_ei, dZq, info);
}

int adkf_predict_marginal_ard(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows,
                              const float* best_f, float* mean, float* var, float* ei, int32_t* info, void*, size_t, void*) {
    return predict_marginal(true, b, phi, flags, Zq, q_off, rows, best_f, mean, var, ei, info);
}

size_t adkf_predict_pool_scratch_bytes(int32_t, int32_t) { return 0; }

// One pool for every task (include/adkf_gp.h).  The selection ranks the float32 values the call returns (or would return), under
// the total order "larger score first, equal scores by ascending row".
int adkf_predict_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                      const int64_t* excl_idx, const int64_t* excl_off, float* mean, float* var, float* ei, int32_t k, int64_t* top_idx,
                      float* top_val, int32_t* info, void*, size_t, void*, size_t, void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~(ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_SCORE_MEAN | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    const bool by_mean = (flags & ADKF_PM_SCORE_MEAN) != 0, want_e = ei || (k > 0 && !by_mean);
    if ((flags & ADKF_PM_LOG_EI) && !want_e) return ADKF_E_BADARG;   // nothing would read it
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (want_e && !best_f) return ADKF_E_BADARG;
    if (!mean && !var && !ei && k == 0) return ADKF_E_BADARG;
    if (int rc = check_topk(k, top_idx, top_val)) return rc;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const size_t o = (size_t)t * (size_t)rows;
        if (mean) std::fill(mean + o, mean + o + rows, 0.f);
        if (var) std::fill(var + o, var + o + rows, 0.f);
        if (ei) std::fill(ei + o, ei + o + rows, 0.f);
        init_topk(top_idx, top_val, t, k);
        std::vector<float> score(k > 0 ? (size_t)rows : 0);
        const bool done = pm_task(b, phi, t, X, 0, rows, info, [&](int64_t r, const Inner& in, const double* D) {
            float m1, v1, e1 = 0.f;
            pm_row(in, b->kernel, D, b->y_s + (size_t)t * b->ns_max, flags, best_f, t, 0, &m1, &v1, want_e ? &e1 : nullptr);
            if (mean) mean[o + r] = m1;
            if (var) var[o + r] = v1;
            if (ei) ei[o + r] = e1;
            if (k > 0) score[r] = by_mean ? ((flags & ADKF_PM_MAXIMIZE) ? m1 : -m1) : e1;
        });
        if (done && k > 0) select_topk(score, rows, k, excl_range(excl_idx, excl_off, t), top_idx + (size_t)t * k, top_val + (size_t)t * k);
    }
    return 0;
}

// g(gamma) = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma) of adkf_mes_pool in float64: log1p where Phi -> 1; as written down to
// gamma = -8 (the two terms cancel from ~a^2 / 2 <= 32: a few 1e-15); below that through Mills' ratio, with a = -gamma, w = a^-2 and
// Phi(-a) = phi(a) M / a, M = 1 + w U, U = -1 + 3 w - 15 w^2 + ... (summed while its terms shrink, as log_h):
//     g = U / (2 M) + log(2 pi) / 2 + log a - log M,
// in which a^2 / 2 never appears.  +-inf and NaN give NaN.
static double mes_term(double g) {
    if (!std::isfinite(g)) return std::numeric_limits<double>::quiet_NaN();
    if (g > -8.0) {
        const double pdf = std::exp(-0.5 * g * g) / std::sqrt(2.0 * M_PI);
        if (g > 0.0) {
            const double q = 0.5 * std::erfc(g / std::sqrt(2.0));
            return 0.5 * g * pdf / (1.0 - q) - std::log1p(-q);
        }
        const double cdf = 0.5 * std::erfc(-g / std::sqrt(2.0));
        return 0.5 * g * pdf / cdf - std::log(cdf);
    }
    const double a = -g, w = (1.0 / a) / a;
    double U = -1.0, term = -1.0;
    for (int k = 1; k < 64; ++k) {
        const double next = -term * (2 * k + 1) * w;
        if (std::fabs(next) >= std::fabs(term)) break;
        U += term = next;
    }
    const double M = 1.0 + w * U;
    return 0.5 * U / M + 0.5 * std::log(2.0 * M_PI) + std::log(a) - std::log(M);
}

// Max-value entropy search over a shared pool (include/adkf_gp.h): the posterior of adkf_predict_pool and mes_term in float64,
// the score rounded to float32 at the boundary; the selection ranks those float32 values under adkf_predict_pool's total order.
int adkf_mes_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* ystar, int32_t S,
                  const int64_t* excl_idx, const int64_t* excl_off, float* score, int32_t k, int64_t* top_idx, float* top_val, int32_t* info,
                  void*, size_t, void*, size_t, void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!ystar) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k == 0 && !score) return ADKF_E_BADARG;
    if (int rc = check_topk(k, top_idx, top_val)) return rc;
    if (S < 1 || S > ADKF_TS_SAMPLES_MAX) return ADKF_E_SIZE;
    const bool maximize = (flags & ADKF_PM_MAXIMIZE) != 0;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const size_t o = (size_t)t * (size_t)rows;
        if (score) std::fill(score + o, score + o + rows, 0.f);
        init_topk(top_idx, top_val, t, k);
        std::vector<float> sc((size_t)rows);
        std::vector<double> kr(b->ns_max);
        const float* y = b->y_s + (size_t)t * b->ns_max;
        const bool done = pm_task(b, phi, t, X, 0, rows, info, [&](int64_t r, const Inner& in, const double* D) {
            const MuQ p = row_posterior(in, b->kernel, D, y, kr.data(), nullptr);
            const double sg = std::sqrt(std::max(in.s - p.q, 1e-12));
            double sum = 0.0;
            for (int s = 0; s < S; ++s) {
                const double ys = ystar[(size_t)t * S + s];
                sum += mes_term((maximize ? (ys - p.mu) : (p.mu - ys)) / sg);
            }
            sc[r] = (float)(sum / S);
            if (score) score[o + r] = sc[r];
        });
        if (done && k > 0) select_topk(sc, rows, k, excl_range(excl_idx, excl_off, t), top_idx + (size_t)t * k, top_val + (size_t)t * k);
    }
    return 0;
}

size_t adkf_gumbel_pool_scratch_bytes(int32_t) { return 0; }

// -log Phi(gamma) of adkf_gumbel_pool in float64, clamped at 32 (csrc/gumbel_stream.h): log1p where Phi -> 1; erfc itself below 0 (it
// does not underflow before the clamp is reached, at gamma ~ -7.6).  NaN gives NaN.
static double neg_log_cdf(double g) {
    if (g != g) return g;
    if (g > 0.0) return -std::log1p(-0.5 * std::erfc(g / std::sqrt(2.0)));
    if (g < -9.0) return 32.0;
    return std::min(32.0, -std::log(0.5 * std::erfc(-g / std::sqrt(2.0))));
}

// Gumbel max-value sampling over a shared pool (include/adkf_gp.h), the scheme of csrc/gumbel_stream.h on host pointers: the float64
// posterior of adkf_predict_pool rounded to float32, the float32 probes, the clamp, the 2^-31 fixed point summed in integers, the
// interpolation and the fit in float64, the draw in float32.
int adkf_gumbel_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* u, int32_t S,
                     float* ystar, float* quant, float* gumbel, int32_t* info, void*, size_t, void*, size_t, void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!u || !ystar) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, nullptr, nullptr)) return ADKF_E_BADARG;
    if (S < 1 || S > ADKF_TS_SAMPLES_MAX) return ADKF_E_SIZE;
    if (rows > ((int64_t)1 << 27)) return ADKF_E_SIZE;
    constexpr int G = ADKF_GUMBEL_PROBES;
    const float ninf = -std::numeric_limits<float>::infinity();
    const bool maximize = (flags & ADKF_PM_MAXIMIZE) != 0;
    double klo = 0.0, khi = 40.0;   // kappa = max(1, Phi^-1(1 - 0.25 / rows)) by bisection
    for (int it = 0; it < 100; ++it) {
        const double mid = 0.5 * (klo + khi);
        if (0.5 * std::erfc(mid / std::sqrt(2.0)) > 0.25 / (double)std::max<int64_t>(rows, 1)) klo = mid; else khi = mid;
    }
    const float kappa = (float)std::max(1.0, khi);
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        std::vector<float> mu((size_t)rows), sg((size_t)rows);
        const float* y = b->y_s + (size_t)t * b->ns_max;
        const bool done = pm_task(b, phi, t, X, 0, rows, info, [&](int64_t r, const Inner& in, const double* D) {
            float m1, v1;
            pm_row(in, b->kernel, D, y, ADKF_PM_LATENT, nullptr, t, 0, &m1, &v1, nullptr);
            mu[r] = maximize ? m1 : -m1;
            sg[r] = std::sqrt(std::max(v1, 1e-12f));
        });
        float fa = ninf, fb = ninf, fq[3] = {ninf, ninf, ninf};
        if (done && rows > 0) {
            float lo = ninf, hi = ninf;
            for (int64_t r = 0; r < rows; ++r) {
                const float l = mu[r] - sg[r], h = std::fma(kappa, sg[r], mu[r]);
                if (l == l && h == h) { lo = std::max(lo, l); hi = std::max(hi, h); }
            }
            float z[G];
            double nl[G];
            auto pass = [&] {
                for (int g = 0; g < G; ++g) {
                    z[g] = g == G - 1 ? hi : std::fma(hi - lo, (float)g / (float)(G - 1), lo);
                    uint64_t sum = 0;
                    for (int64_t r = 0; r < rows; ++r) {
                        const double term = neg_log_cdf((double)((z[g] - mu[r]) / sg[r]));
                        sum += (uint64_t)std::llrint((term == term ? term : 32.0) * 2147483648.0);
                    }
                    nl[g] = -(double)sum / 2147483648.0;
                }
            };
            pass();
            int g_lo = 0, g_hi = G - 1;
            for (int g = 0; g < G; ++g) if (nl[g] <= std::log(0.25)) g_lo = g;
            for (int g = G - 1; g >= 0; --g) if (nl[g] >= std::log(0.75)) g_hi = g;
            if (g_hi < g_lo) g_hi = g_lo;
            lo = z[g_lo]; hi = z[g_hi];
            pass();
            const double lq[3] = {std::log(0.25), std::log(0.5), std::log(0.75)};
            double q[3];
            for (int i = 0; i < 3; ++i) {
                int g1 = -1;
                for (int g = 0; g < G; ++g) if (nl[g] >= lq[i]) { g1 = g; break; }
                if (g1 < 0) q[i] = z[G - 1];
                else if (g1 == 0 || nl[g1] == nl[g1 - 1] || z[g1] == z[g1 - 1]) q[i] = z[g1 > 0 ? g1 - 1 : 0];
                else q[i] = (double)z[g1 - 1] + ((double)z[g1] - (double)z[g1 - 1]) * ((lq[i] - nl[g1 - 1]) / (nl[g1] - nl[g1 - 1]));
            }
            double bb = (q[2] - q[0]) / (std::log(std::log(4.0)) - std::log(std::log(4.0 / 3.0)));
            if (!(bb > 0.0)) bb = 0.0;
            fa = (float)(q[1] + bb * std::log(std::log(2.0))); fb = (float)bb;
            for (int i = 0; i < 3; ++i) fq[i] = (float)q[i];
        }
        if (quant) for (int i = 0; i < 3; ++i) quant[(size_t)t * 3 + i] = fq[i];
        if (gumbel) { gumbel[(size_t)t * 2] = fa; gumbel[(size_t)t * 2 + 1] = fb; }
        for (int s = 0; s < S; ++s) {
            float h = ninf;
            if (done && rows > 0) {
                const float uc = std::min(std::max(u[(size_t)t * S + s], 5.9604644775390625e-8f), 1.f - 5.9604644775390625e-8f);
                h = fa - fb * std::log(-std::log(uc));
            }
            ystar[(size_t)t * S + s] = maximize ? h : -h;
        }
    }
    return 0;
}

// The pathwise posterior draws of a prepared task (prepare_task with_mean), for adkf_thompson_pool(_ard) and adkf_qei_pool: the features
// phi_j(x) = sqrt(2 s / m) cos(omega_j . ((x - mean) / l_dim) / l + phase_j), the prior draws g_q = w_q . phi, r = y - g(Z_s) - sqrt(noise) eps
// and v = A^-1 r (V [S, n]).  row(x) prepares the features and the kernel row of x; value(q) is then f_q(x) = g_q(x) + k(x, Z_s) . v_q.
struct PathDraws {
    const TaskPrep& tp;
    const Inner& in;
    const float *omega, *phase, *wt;
    int kind, d, m, S, n;
    double amp, sigma;
    std::vector<double> ft, k;
    Mat V;
    PathDraws(const adkf_batch_t* b, int t, const TaskPrep& tp_, const float* omega_, const float* phase_, int m_, const float* w, const float* eps, int S_)
        : tp(tp_), in(tp_.in), omega(omega_), phase(phase_), wt(w + (size_t)t * S_ * m_), kind(b->kernel), d(b->d), m(m_), S(S_), n(tp_.n),
          amp(std::sqrt(2.0 * tp_.in.s / m_)), sigma(std::sqrt(tp_.in.noise)), ft(m_), k(tp_.n), V((size_t)S_ * tp_.n) {
        const int ld = b->ns_max;
        const float* Zs = b->Z_s + (size_t)t * ld * d;
        const float* ys = b->y_s + (size_t)t * ld;
        Mat R((size_t)S * n);
        for (int i = 0; i < n; ++i) {
            features(Zs + (size_t)i * d);
            for (int q = 0; q < S; ++q) R[(size_t)q * n + i] = (double)ys[i] - prior(q) - sigma * (double)eps[((size_t)t * S + q) * ld + i];
        }
        for (int q = 0; q < S; ++q)
            for (int i = 0; i < n; ++i) {
                double v = 0.0;
                for (int kk = 0; kk < n; ++kk) v += in.Ainv[(size_t)i * n + kk] * R[(size_t)q * n + kk];
                V[(size_t)q * n + i] = v;
            }
    }
    void features(const float* x) {   // phi_j(x), j < m
        for (int j = 0; j < m; ++j) {
            double a = 0.0;
            const float* om = omega + (size_t)j * d;
            for (int c = 0; c < d; ++c) a += (double)om[c] * (((double)x[c] - tp.mean[c]) / tp.l[c]);
            ft[j] = amp * std::cos(a / in.l + (double)phase[j]);
        }
    }
    double prior(int q) const { double g = 0.0; const float* wq = wt + (size_t)q * m; for (int j = 0; j < m; ++j) g += (double)wq[j] * ft[j]; return g; }
    void row(const float* x) { features(x); row_k(in, kind, task_row_dist(tp, x, d).data(), k.data()); }
    double value(int q) const { double f = prior(q); for (int j = 0; j < n; ++j) f += k[j] * V[(size_t)q * n + j]; return f; }
};

size_t adkf_thompson_pool_scratch_bytes(int32_t, int32_t, int32_t, int32_t) { return 0; }

// Thompson sampling over a shared pool (include/adkf_gp.h): the pathwise posterior draws in float64, rounded to float32 at the
// boundary; the selection ranks those float32 values under "larger score first, equal scores by ascending row".  ARD
// (adkf_thompson_pool_ard): on z~ = (z - mu) / l at unit lengthscale, by prepare_task as for every entry; otherwise the features are
// centred with the support column mean (prepare_task's with_mean), the distances are taken from the rows as they are and l = 1, which changes no bit of the isotropic call.
static int thompson_pool(bool ard, const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega,
                         const float* phase, int32_t m, const float* w, const float* eps, int32_t S, const int64_t* excl_idx,
                         const int64_t* excl_off, float* paths, int64_t* sel_idx, float* sel_val, int32_t* info) {
    if (int rc = check_support_only(b, phi, info, rows, ard)) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!omega || !phase || !w || !eps || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (S < 1 || S > ADKF_TS_SAMPLES_MAX) return ADKF_E_SIZE;
    if (m < 64 || m > ADKF_TS_FEATURES_MAX || (m & 63)) return ADKF_E_SIZE;
    const int d = b->d;
    const float ninf = -std::numeric_limits<float>::infinity();
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        init_topk(sel_idx, sel_val, t, S);
        if (paths && rows > 0) std::fill(paths + (size_t)t * S * rows, paths + (size_t)(t + 1) * S * rows, 0.f);
        TaskPrep tp;
        if (!prepare_task(b, phi, t, true, info, tp)) continue;
        PathDraws pd(b, t, tp, omega, phase, m, w, eps, S);
        std::vector<float> bv(S, ninf);
        std::vector<int64_t> bi(S, -1);
        const Excl excl = excl_range(excl_idx, excl_off, t);
        for (int64_t r = 0; r < rows; ++r) {
            pd.row(X + (size_t)r * d);
            const bool excluded = excl.has(r);
            for (int q = 0; q < S; ++q) {
                const float ff = (float)pd.value(q), sc = (flags & ADKF_PM_MAXIMIZE) ? ff : -ff;
                if (paths) paths[((size_t)t * S + q) * rows + r] = ff;
                if (sc == sc && !excluded && (bi[q] < 0 || sc > bv[q])) { bv[q] = sc; bi[q] = r; }   // (rows ascend: a tie keeps the lower index)
            }
        }
        for (int q = 0; q < S; ++q) { sel_idx[(size_t)t * S + q] = bi[q]; sel_val[(size_t)t * S + q] = bi[q] >= 0 ? bv[q] : ninf; }
    }
    return 0;
}

int adkf_thompson_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega,
                       const float* phase, int32_t m, const float* w, const float* eps, int32_t S, const int64_t* excl_idx,
                       const int64_t* excl_off, float* paths, int64_t* sel_idx, float* sel_val, int32_t* info, void*, size_t, void*, size_t,
                       void*) {
    return thompson_pool(false, b, phi, flags, X, rows, omega, phase, m, w, eps, S, excl_idx, excl_off, paths, sel_idx, sel_val, info);   // (refuses ARD batches)
}

int adkf_thompson_pool_ard(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega,
                           const float* phase, int32_t m, const float* w, const float* eps, int32_t S, const int64_t* excl_idx,
                           const int64_t* excl_off, float* paths, int64_t* sel_idx, float* sel_val, int32_t* info, void*, size_t, void*, size_t,
                           void*) {
    return thompson_pool(true, b, phi, flags, X, rows, omega, phase, m, w, eps, S, excl_idx, excl_off, paths, sel_idx, sel_val, info);
}

size_t adkf_qei_pool_scratch_bytes(int32_t, int32_t, int32_t, int32_t) { return 0; }

// Monte-Carlo (noisy) q-EI over a shared pool (include/adkf_gp.h), for either kind of batch: Thompson's paths (PathDraws) in float64,
// rounded to float32 at the boundary as adkf_thompson_pool's paths are; the incumbents are float32 values; a row's score is the float64
// sum of its clipped differences, divided by S and rounded once; the selection is greedy_pick's.  The noisy incumbent is taken as the
// header states it: y_i - sqrt(noise) eps_(s,i) - noise v_(s,i).
int adkf_qei_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega, const float* phase,
                  int32_t m, const float* w, const float* eps, int32_t S, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off,
                  int32_t q, float* trace, float* inc, int64_t* sel_idx, float* sel_val, int32_t* info, void*, size_t, void*, size_t, void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!omega || !phase || !w || !eps || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (S < 1 || S > ADKF_QEI_SAMPLES_MAX) return ADKF_E_SIZE;
    if (m < 64 || m > ADKF_TS_FEATURES_MAX || (m & 63)) return ADKF_E_SIZE;
    if (q < 1 || q > ADKF_QEI_PICKS_MAX) return ADKF_E_SIZE;
    const int d = b->d, ld = b->ns_max;
    const bool mx = (flags & ADKF_PM_MAXIMIZE) != 0;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        init_topk(sel_idx, sel_val, t, q);
        if (trace && rows > 0) std::fill(trace + (size_t)t * q * rows, trace + (size_t)(t + 1) * q * rows, 0.f);
        float* inct = inc ? inc + (size_t)t * (q + 1) * S : nullptr;
        if (inct) std::fill(inct, inct + (size_t)(q + 1) * S, best_f ? best_f[t] : 0.f);
        TaskPrep tp;
        if (!prepare_task(b, phi, t, true, info, tp)) continue;
        PathDraws pd(b, t, tp, omega, phase, m, w, eps, S);
        const int n = tp.n;
        const size_t R = (size_t)rows;
        std::vector<float> F((size_t)S * R), bs(S), score(R);
        for (size_t r = 0; r < R; ++r) {
            pd.row(X + r * d);
            for (int s = 0; s < S; ++s) F[(size_t)s * R + r] = (float)pd.value(s);
        }
        const float* ys = b->y_s + (size_t)t * ld;
        for (int s = 0; s < S; ++s) {
            if (best_f) { bs[s] = best_f[t]; continue; }
            double best = 0.0;
            for (int i = 0; i < n; ++i) {
                const double f = (double)ys[i] - pd.sigma * (double)eps[((size_t)t * S + s) * ld + i] - tp.in.noise * pd.V[(size_t)s * n + i];
                best = i == 0 ? f : (mx ? std::max(best, f) : std::min(best, f));
            }
            bs[s] = (float)best;
        }
        if (inct) std::copy(bs.begin(), bs.end(), inct);
        const Excl excl = excl_range(excl_idx, excl_off, t);
        std::vector<char> taken(R, 0);
        for (int j = 0; j < q; ++j) {
            for (size_t r = 0; r < R; ++r) {
                double sum = 0.0;
                for (int s = 0; s < S; ++s) {
                    const double imp = mx ? (double)F[(size_t)s * R + r] - (double)bs[s] : (double)bs[s] - (double)F[(size_t)s * R + r];
                    sum += imp < 0.0 ? 0.0 : imp;   // (NaN stays NaN)
                }
                score[r] = (float)(sum / S);
                if (trace) trace[((size_t)t * q + j) * R + r] = score[r];
            }
            const int64_t p = greedy_pick(score, rows, taken, excl);
            if (p >= 0) {   // (no eligible row: this step and all later ones keep -1 / -inf, the state stays)
                sel_idx[(size_t)t * q + j] = p; sel_val[(size_t)t * q + j] = score[p];
                taken[p] = 1;
                for (int s = 0; s < S; ++s) bs[s] = mx ? std::max(bs[s], F[(size_t)s * R + p]) : std::min(bs[s], F[(size_t)s * R + p]);
            }
            if (inct) std::copy(bs.begin(), bs.end(), inct + (size_t)(j + 1) * S);
        }
    }
    return 0;
}

size_t adkf_believer_pool_scratch_bytes(int32_t, int32_t, int32_t, int32_t) { return 0; }

// log1p(-rho2 h(gamma)) of adkf_gibbon_pool in float64, h = tau (gamma + tau), tau = phi / Phi: as written down to gamma = -8 (gamma + tau
// cancels from ~8 to ~0.12: a few 1e-15); below that through Mills' ratio as mes_term, with a = -gamma, w = a^-2, Phi(-a) = phi(a) M / a,
// M = 1 + w U: tau = a / M and gamma + tau = -a w U / M, so h = -U / M^2.  +-inf and NaN give NaN.
static double gibbon_term(double g, double rho2) {
    if (!std::isfinite(g)) return std::numeric_limits<double>::quiet_NaN();
    double h;
    if (g > -8.0) {
        const double pdf = std::exp(-0.5 * g * g) / std::sqrt(2.0 * M_PI);
        const double tau = g > 0.0 ? pdf / (1.0 - 0.5 * std::erfc(g / std::sqrt(2.0))) : pdf / (0.5 * std::erfc(-g / std::sqrt(2.0)));
        h = tau * (g + tau);
    } else {
        const double a = -g, w = (1.0 / a) / a;
        double U = -1.0, term = -1.0;
        for (int k = 1; k < 64; ++k) {
            const double next = -term * (2 * k + 1) * w;
            if (std::fabs(next) >= std::fabs(term)) break;
            U += term = next;
        }
        const double M = 1.0 + w * U;
        h = -U / (M * M);
    }
    return std::log1p(-rho2 * std::min(h, 1.0));
}

// Kriging-believer batch selection (include/adkf_gp.h): the mean, the latent variance and K A^-1 of every pool row once, then per
// step one more column of ell (the forward substitution of the header, one row of G at a time) and the scores in float32, ranked
// under "larger score first, equal scores by ascending row".  ARD (adkf_believer_pool_ard): pm_task prepares the support set and the
// pool rows on z~ = (z - mu) / l at unit lengthscale, and the distances between pool rows are taken on x / l (mu cancels); otherwise
// l = 1 and the rows are taken as they are, which changes no bit of the isotropic call.
// GIBBON (adkf_gibbon_pool: ystar given, S samples per task, no best_f): the same greedy loop and downdate with the score
// a(x) + 1/2 log((max(v_j, 1e-12) + noise) / (max(v_0, 1e-12) + noise)), a(x) from gibbon_term, computed once per row; the mean and
// the variances enter the score in float64 (the device rounds them to float32 first).
// The constant liar and label replay (adkf_liar_pool: liar given): the pick is conditioned on y_j, the first finite of its label, the
// task's lie and its own mean, so after append_pick - whose column of ell is the one the mean moves along - every row's mean gains
// ell_j(x) z_j, z_j = (y_j - m_j(x_p)) / G[j, j]; the incumbent follows y_j.
struct Liar {
    const float *lie, *labels; int64_t stride;
    float *sel_lie, *inc;
};
static int believer_pool(bool ard, const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                         const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val,
                         float* sel_mean, float* sel_var, int32_t* info, const float* ystar = nullptr, int32_t S = 0, bool gibbon = false,
                         const Liar* liar = nullptr) {
    if (int rc = check_support_only(b, phi, info, rows, ard)) return rc;
    if (flags & ~(gibbon ? ADKF_PM_MAXIMIZE : (ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI))) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!(gibbon ? ystar : best_f) || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (liar && !liar->lie && !liar->labels) return ADKF_E_BADARG;
    if (liar && liar->stride != 0 && (liar->stride != rows || !liar->labels)) return ADKF_E_BADARG;
    if (q < 1 || (gibbon && S < 1)) return ADKF_E_BADARG;
    if (q > ADKF_POOL_TOPK_MAX || (gibbon && S > ADKF_TS_SAMPLES_MAX)) return ADKF_E_SIZE;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        init_topk(sel_idx, sel_val, t, q);
        if (liar && liar->sel_lie) std::fill(liar->sel_lie + (size_t)t * q, liar->sel_lie + (size_t)(t + 1) * q, 0.f);
        if (liar && liar->inc) std::fill(liar->inc + (size_t)t * (q + 1), liar->inc + (size_t)(t + 1) * (q + 1), best_f[t]);
        if (sel_mean) std::fill(sel_mean + (size_t)t * q, sel_mean + (size_t)(t + 1) * q, 0.f);
        if (sel_var) std::fill(sel_var + (size_t)t * q, sel_var + (size_t)(t + 1) * q, 0.f);
        if (trace && rows > 0) std::fill(trace + (size_t)t * q * rows, trace + (size_t)(t + 1) * q * rows, 0.f);
        PoolState st;
        if (!pool_state(b, phi, t, X, rows, info, st)) continue;
        const size_t R = st.R;
        Mat& mu = st.mu;       // (the liar moves it)
        const Mat& v = st.v;   // (append_pick downdates it)
        const double noise = st.noise;
        const Excl excl = excl_range(excl_idx, excl_off, t);
        std::vector<char> taken(R, 0);
        std::vector<float> score(R);
        Mat G((size_t)q * q, 0.0), L(R * q), col(R);
        double best = gibbon ? 0.0 : best_f[t];
        Mat v0(gibbon ? v : Mat()), ax(gibbon ? R : 0);   // GIBBON: the step-0 variance and a(x)
        if (gibbon)
            for (size_t r = 0; r < R; ++r) {
                const double vc = std::max(v0[r], 1e-12), sg = std::sqrt(vc), rho2 = vc / (vc + noise);
                double sum = 0.0;
                for (int k = 0; k < S; ++k) {
                    const double ys = ystar[(size_t)t * S + k];
                    sum += gibbon_term(((flags & ADKF_PM_MAXIMIZE) ? (ys - mu[r]) : (mu[r] - ys)) / sg, rho2);
                }
                ax[r] = -0.5 * sum / S;
            }
        for (int j = 0; j < q; ++j) {
            for (int64_t r = 0; r < rows; ++r) {
                score[r] = gibbon ? (float)(ax[r] + 0.5 * std::log((std::max(v[r], 1e-12) + noise) / (std::max(v0[r], 1e-12) + noise)))
                                  : pm_ei(mu[r], v[r], best, flags);
                if (trace) trace[((size_t)t * q + j) * R + r] = score[r];
            }
            const int64_t p = greedy_pick(score, rows, taken, excl);
            if (p < 0) continue;   // no eligible row: this step and all later ones keep -1 / -inf, the state (hence trace) stays
            const size_t o = (size_t)t * q + j;
            sel_idx[o] = p; sel_val[o] = score[p];
            if (sel_mean) sel_mean[o] = (float)mu[p];
            if (sel_var) sel_var[o] = (float)v[p];
            const double mjp = mu[p];
            append_pick(st, b, X, p, j, q, G, L, col);   // (a step without a pick ends the batch, so step j is entry j)
            taken[p] = 1;
            double mp = (double)(float)mjp;
            if (liar) {
                float y = liar->labels ? liar->labels[(size_t)t * (size_t)liar->stride + (size_t)p] : std::numeric_limits<float>::quiet_NaN();
                if (!std::isfinite(y) && liar->lie) y = liar->lie[t];
                if (std::isfinite(y)) {
                    mp = y;
                    const double z = ((double)y - mjp) / G[(size_t)j * q + j];
                    for (size_t r = 0; r < R; ++r) mu[r] += L[r * q + j] * z;
                }
                if (liar->sel_lie) liar->sel_lie[o] = (float)mp;
            }
            best = (flags & ADKF_PM_MAXIMIZE) ? std::max(best, mp) : std::min(best, mp);
            if (liar && liar->inc) std::fill(liar->inc + (size_t)t * (q + 1) + j + 1, liar->inc + (size_t)(t + 1) * (q + 1), (float)best);
        }
    }
    return 0;
}

int adkf_believer_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                       const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val,
                       float* sel_mean, float* sel_var, int32_t* info, void*, size_t, void*, size_t, void*) {
    return believer_pool(false, b, phi, flags, X, rows, best_f, excl_idx, excl_off, q, trace, sel_idx, sel_val, sel_mean, sel_var, info);   // (refuses ARD batches)
}

int adkf_believer_pool_ard(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                           const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val,
                           float* sel_mean, float* sel_var, int32_t* info, void*, size_t, void*, size_t, void*) {
    return believer_pool(true, b, phi, flags, X, rows, best_f, excl_idx, excl_off, q, trace, sel_idx, sel_val, sel_mean, sel_var, info);
}

// GIBBON batch max-value entropy search (include/adkf_gp.h): believer_pool's loop with the GIBBON score, for either kind of batch
int adkf_gibbon_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* ystar, int32_t S,
                     const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val,
                     float* sel_mean, float* sel_var, int32_t* info, void*, size_t, void*, size_t, void*) {
    const bool ard = b && (b->flags & ADKF_BATCH_ARD) != 0;
    return believer_pool(ard, b, phi, flags, X, rows, nullptr, excl_idx, excl_off, q, trace, sel_idx, sel_val, sel_mean, sel_var, info, ystar, S, true);
}

size_t adkf_liar_pool_scratch_bytes(int32_t, int32_t, int32_t, int32_t) { return 0; }

// Constant-liar and label-replay batches (include/adkf_gp.h): believer_pool's loop with the believed value supplied, for either kind of batch
int adkf_liar_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f, const float* lie,
                   const float* labels, int64_t label_stride, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace,
                   int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, float* sel_lie, float* inc, int32_t* info, void*, size_t,
                   void*, size_t, void*) {
    const bool ard = b && (b->flags & ADKF_BATCH_ARD) != 0;
    const Liar liar{lie, labels, label_stride, sel_lie, inc};
    return believer_pool(ard, b, phi, flags, X, rows, best_f, excl_idx, excl_off, q, trace, sel_idx, sel_val, sel_mean, sel_var, info, nullptr, 0,
                         false, &liar);
}

size_t adkf_levelset_pool_scratch_bytes(int32_t, int32_t, int32_t, int32_t) { return 0; }

static double log_cdf(double z);

// Level-set estimation and batch UCB (include/adkf_gp.h): believer_pool's greedy loop and downdate with the mean held fixed and no
// incumbent.  The posterior, z and the scores are float64, rounded to float32 at the boundary; the class of a row is taken from the
// float32-rounded straddle - the value a STRADDLE call stores in trace - so that the counts are comparable with the device's; hits
// is the device's 2^-31 fixed-point sum of the float32-rounded Phi terms, integer adds only (csrc/levelset_stream.h).
int adkf_levelset_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* tau, const float* beta,
                       int32_t kind, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int8_t* cls, int64_t* counts,
                       float* hits, int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, int32_t* info, void*, size_t, void*,
                       size_t, void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (kind < ADKF_LS_STRADDLE || kind > ADKF_LS_BOUND) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!tau || !beta || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (q < 1) return ADKF_E_BADARG;
    if (q > ADKF_POOL_TOPK_MAX) return ADKF_E_SIZE;
    if ((counts || hits) && rows > ((int64_t)1 << 31)) return ADKF_E_SIZE;
    const bool maximize = (flags & ADKF_PM_MAXIMIZE) != 0;
    const float nan = std::numeric_limits<float>::quiet_NaN();
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        init_topk(sel_idx, sel_val, t, q);
        if (sel_mean) std::fill(sel_mean + (size_t)t * q, sel_mean + (size_t)(t + 1) * q, 0.f);
        if (sel_var) std::fill(sel_var + (size_t)t * q, sel_var + (size_t)(t + 1) * q, 0.f);
        if (trace && rows > 0) std::fill(trace + (size_t)t * q * rows, trace + (size_t)(t + 1) * q * rows, 0.f);
        if (cls && rows > 0) std::fill(cls + (size_t)t * rows, cls + (size_t)(t + 1) * rows, (int8_t)-1);
        if (counts) std::fill(counts + (size_t)t * q * 3, counts + (size_t)(t + 1) * q * 3, (int64_t)0);
        if (hits) std::fill(hits + (size_t)t * q, hits + (size_t)(t + 1) * q, 0.f);
        PoolState st;
        if (!pool_state(b, phi, t, X, rows, info, st)) continue;
        const size_t R = st.R;
        const Mat &mu = st.mu, &v = st.v;   // (append_pick downdates v)
        const double tf = tau[t], bf = beta[t];
        const bool ok = std::isfinite(tf) && std::isfinite(bf) && bf >= 0.0;
        const Excl excl = excl_range(excl_idx, excl_off, t);
        std::vector<char> taken(R, 0);
        std::vector<float> score(R);
        Mat G((size_t)q * q, 0.0), L(R * q), col(R);
        for (int j = 0; j < q; ++j) {
            const size_t o = (size_t)t * q + j;
            uint64_t n[3] = {0, 0, 0}, fixed = 0;
            for (size_t r = 0; r < R; ++r) {
                int c = -1;
                score[r] = nan;
                if (ok && mu[r] == mu[r] && v[r] == v[r]) {
                    const double sg = std::sqrt(std::max(v[r], 1e-12)), dm = mu[r] - tf, sd = maximize ? dm : -dm, z = sd / sg;
                    const double straddle = bf * sg - std::fabs(dm);
                    c = (float)straddle > 0.f ? 2 : (sd > 0.0 ? 0 : 1);
                    const double Phi = z > 0.0 ? 1.0 - 0.5 * std::erfc(z / std::sqrt(2.0)) : 0.5 * std::erfc(-z / std::sqrt(2.0));
                    fixed += (uint64_t)std::llrint((double)(float)Phi * 2147483648.0);
                    ++n[c];
                    score[r] = (float)(kind == ADKF_LS_STRADDLE ? straddle : (kind == ADKF_LS_PROB ? log_cdf(z) : (maximize ? mu[r] : -mu[r]) + bf * sg));
                }
                if (trace) trace[o * R + r] = score[r];
                if (cls && j == 0) cls[(size_t)t * R + r] = (int8_t)c;
            }
            if (counts) for (int c = 0; c < 3; ++c) counts[o * 3 + c] = (int64_t)n[c];
            if (hits) hits[o] = (float)((double)fixed / 2147483648.0);
            const int64_t p = greedy_pick(score, rows, taken, excl);
            if (p < 0) continue;   // no eligible row: this step and all later ones keep -1 / -inf, the state (hence the counts) stays
            sel_idx[o] = p; sel_val[o] = score[p];
            if (sel_mean) sel_mean[o] = (float)mu[p];
            if (sel_var) sel_var[o] = (float)v[p];
            append_pick(st, b, X, p, j, q, G, L, col);
            taken[p] = 1;
        }
    }
    return 0;
}

size_t adkf_kg_pool_scratch_bytes(int32_t, int32_t, int32_t, int32_t, int32_t) { return 0; }

// KG or log KG of the lines (a_l, b_l) in float64, Frazier's sorted form: the lines by ascending slope (equal slopes: the largest
// intercept only), the upper envelope by a stack of breakpoints, then the sum of (b_next - b_cur) h(-|c|) over consecutive survivors
// (h through log_h: the tail keeps its digits), or its log-sum-exp.  One surviving line: 0 / -inf.
static double kg_value(std::vector<std::pair<double, double>> ln, bool want_log) {   // (b, a) pairs
    const double ninf = -std::numeric_limits<double>::infinity();
    std::sort(ln.begin(), ln.end(), [](const std::pair<double, double>& x, const std::pair<double, double>& y) { return x.first < y.first || (x.first == y.first && x.second > y.second); });
    std::vector<std::pair<double, double>> hull;   // survivors, ascending slope
    std::vector<double> start;                     // start[i]: from where survivor i is on top
    for (const auto& l : ln) {
        if (!hull.empty() && hull.back().first == l.first) continue;   // an equal slope with a smaller (or equal) intercept
        double z = ninf;
        while (!hull.empty()) {
            z = (hull.back().second - l.second) / (l.first - hull.back().first);
            if (z > start.back()) break;
            hull.pop_back(); start.pop_back();
            z = ninf;
        }
        hull.push_back(l); start.push_back(hull.size() == 1 ? ninf : z);
    }
    std::vector<double> lt;
    for (size_t i = 0; i + 1 < hull.size(); ++i) lt.push_back(std::log(hull[i + 1].first - hull[i].first) + log_h(-std::fabs(start[i + 1])));
    if (lt.empty()) return want_log ? ninf : 0.0;
    const double mx = *std::max_element(lt.begin(), lt.end());
    if (mx == ninf) return want_log ? ninf : 0.0;
    double sum = 0.0;
    for (double x : lt) sum += std::exp(x - mx);
    return want_log ? mx + std::log(sum) : std::exp(mx) * sum;
}

// Knowledge-gradient selection over a shared pool (include/adkf_gp.h): the mean, the latent variance and K A^-1 of every pool row
// once, the covariance of every row with every valid reference entry from them, then kg_value per row in float64, rounded to float32
// at the boundary; the selection ranks those float32 values under adkf_predict_pool's total order.  ARD: pm_task prepares the
// support set and the pool rows on z~ = (z - mu) / l, and the distances between pool rows are taken on x / l (mu cancels).
int adkf_kg_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* ref_idx, int32_t M,
                 const int64_t* excl_idx, const int64_t* excl_off, float* score, float* cov, float* ref_mean, int32_t k, int64_t* top_idx,
                 float* top_val, int32_t* info, void*, size_t, void*, size_t, void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~(ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    if (!ref_idx) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k == 0 && !score && !cov && !ref_mean) return ADKF_E_BADARG;
    if (int rc = check_topk(k, top_idx, top_val)) return rc;
    if (M < 1 || M > ADKF_KG_REFS_MAX) return ADKF_E_SIZE;
    const bool want_log = (flags & ADKF_PM_LOG_EI) != 0;
    const double sgn = (flags & ADKF_PM_MAXIMIZE) ? 1.0 : -1.0;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const size_t R = (size_t)rows, o = (size_t)t * R;
        if (score) std::fill(score + o, score + o + R, 0.f);
        if (cov) std::fill(cov + o * M, cov + (o + R) * M, 0.f);
        if (ref_mean) std::fill(ref_mean + (size_t)t * M, ref_mean + (size_t)(t + 1) * M, 0.f);
        init_topk(top_idx, top_val, t, k);
        PoolState st;
        if (!pool_state(b, phi, t, X, rows, info, st)) continue;
        const Mat &mu = st.mu, &v = st.v;
        std::vector<int64_t> ref(M);   // the valid entries, -1 for the others
        Mat C(R * M, 0.0), col(R);     // cov(x_r, entry j)
        for (int j = 0; j < M; ++j) {
            const int64_t p = ref[j] = valid_entry(ref_idx + (size_t)t * M, j, rows);
            if (p < 0) continue;
            if (ref_mean) ref_mean[(size_t)t * M + j] = (float)mu[p];
            c0_col(st, b, X, p, col.data());
            for (size_t r = 0; r < R; ++r) {
                C[r * M + j] = col[r];
                if (cov) cov[(o + r) * M + j] = (float)col[r];
            }
        }
        std::vector<float> sc(R);
        for (size_t r = 0; r < R; ++r) {
            const double vc = std::max(v[r], 1e-12), sd = std::sqrt(vc + st.noise);
            std::vector<std::pair<double, double>> ln;
            for (int j = 0; j < M; ++j)
                if (ref[j] >= 0 && ref[j] != (int64_t)r) ln.emplace_back(C[r * M + j] / sd, sgn * mu[ref[j]]);
            ln.emplace_back(vc / sd, sgn * mu[r]);
            sc[r] = (mu[r] == mu[r] && v[r] == v[r]) ? (float)kg_value(ln, want_log) : std::numeric_limits<float>::quiet_NaN();   // a NaN row: NaN
            if (score) score[o + r] = sc[r];
        }
        if (k > 0) select_topk(sc, rows, k, excl_range(excl_idx, excl_off, t), top_idx + (size_t)t * k, top_val + (size_t)t * k);
    }
    return 0;
}

size_t adkf_ipv_pool_scratch_bytes(int32_t, int32_t, int32_t, int32_t, int32_t) { return 0; }

// Target-variance batch selection over a shared pool (include/adkf_gp.h): the latent variance and K A^-1 of every pool row once, the
// covariance of every row with every valid target from them, then per step the scores in float64, rounded to float32 at the
// boundary and ranked under "larger score first, equal scores by ascending row", and one more column of ell for every row (the
// believer's substitution, one row of G at a time); the targets' ell are the rows' own, read at the targets' indices.  ARD: pm_task
// prepares the support set and the pool rows on z~ = (z - mu) / l, and the distances between pool rows are taken on x / l.
int adkf_ipv_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* tgt_idx, const float* tgt_w,
                  int32_t M, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val,
                  float* tvar, int32_t* info, void*, size_t, void*, size_t, void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (!tgt_idx || !sel_idx || !sel_val) return ADKF_E_BADARG;
    if (M < 1 || q < 1) return ADKF_E_BADARG;
    if ((int64_t)M + q > ADKF_IPV_ENTRIES_MAX) return ADKF_E_SIZE;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        init_topk(sel_idx, sel_val, t, q);
        if (tvar) std::fill(tvar + (size_t)t * (q + 1), tvar + (size_t)(t + 1) * (q + 1), 0.f);
        if (trace && rows > 0) std::fill(trace + (size_t)t * q * rows, trace + (size_t)(t + 1) * q * rows, 0.f);
        PoolState st;
        if (!pool_state(b, phi, t, X, rows, info, st)) continue;
        const size_t R = st.R;
        const Mat& v = st.v;   // (append_pick downdates it)
        // the valid targets with a weight > 0; Ct: cov_j(x_r, target), downdated with the rows
        std::vector<int64_t> tg;
        std::vector<double> wt;
        for (int m = 0; m < M; ++m) {
            const int64_t p = valid_entry(tgt_idx + (size_t)t * M, m, rows);
            const float w = tgt_w ? tgt_w[(size_t)t * M + m] : 1.f;
            if (p >= 0 && w > 0.f) { tg.push_back(p); wt.push_back(w); }
        }
        const size_t nt = tg.size();
        if (nt == 0) continue;
        Mat Ct(nt * R);
        for (size_t m = 0; m < nt; ++m) c0_col(st, b, X, tg[m], &Ct[m * R]);
        auto total = [&] { double x = 0.0; for (size_t m = 0; m < nt; ++m) x += wt[m] * v[tg[m]]; return x; };
        if (tvar) tvar[(size_t)t * (q + 1)] = (float)total();
        const Excl excl = excl_range(excl_idx, excl_off, t);
        std::vector<char> taken(R, 0);
        std::vector<float> score(R);
        Mat G((size_t)q * q, 0.0), L(R * q), col(R);
        int c = 0;   // picks made
        for (int j = 0; j < q; ++j) {
            for (int64_t r = 0; r < rows; ++r) {
                double sum = 0.0;
                for (size_t m = 0; m < nt; ++m) sum += wt[m] * Ct[m * R + r] * Ct[m * R + r];
                score[r] = (float)(sum / (std::max(v[r], 1e-12) + st.noise));
                if (trace) trace[((size_t)t * q + j) * R + r] = score[r];
            }
            const int64_t p = greedy_pick(score, rows, taken, excl);
            if (p >= 0) {   // (no eligible row: this step and all later ones keep -1 / -inf, the state stays)
                sel_idx[(size_t)t * q + j] = p; sel_val[(size_t)t * q + j] = score[p];
                append_pick(st, b, X, p, c, q, G, L, col);
                for (size_t m = 0; m < nt; ++m) {   // the targets' ell are the rows' own
                    const double em = L[(size_t)tg[m] * q + c];
                    for (size_t r = 0; r < R; ++r) Ct[m * R + r] -= L[r * q + c] * em;
                }
                taken[p] = 1;
                ++c;
            }
            if (tvar) tvar[(size_t)t * (q + 1) + j + 1] = (float)total();
        }
    }
    return 0;
}

size_t adkf_jes_pool_scratch_bytes(int32_t, int32_t, int32_t, int32_t, int32_t) { return 0; }

// Joint entropy search over a shared pool (include/adkf_gp.h): the mean, the latent variance and K A^-1 of every pool row once, the
// covariance of every row with every valid sample's row from them (a repeated row is computed again: it counts again), then the S
// terms per row in float64 (gibbon_term), rounded to float32 at the boundary; the selection ranks those float32 values under
// adkf_predict_pool's total order.  ARD: as adkf_kg_pool.
int adkf_jes_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* opt_idx,
                  const float* opt_val, int32_t S, float cond_noise, const int64_t* excl_idx, const int64_t* excl_off, float* score,
                  float* opt_mean, float* opt_var, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void*, size_t, void*, size_t,
                  void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~ADKF_PM_MAXIMIZE) return ADKF_E_BADARG;
    if (!opt_idx || !opt_val) return ADKF_E_BADARG;
    if (!(cond_noise >= 0.f) || !std::isfinite(cond_noise)) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k == 0 && !score && !opt_mean && !opt_var) return ADKF_E_BADARG;
    if (int rc = check_topk(k, top_idx, top_val)) return rc;
    if (S < 1 || S > ADKF_TS_SAMPLES_MAX) return ADKF_E_SIZE;
    const bool maximize = (flags & ADKF_PM_MAXIMIZE) != 0;
    const float fnan = std::numeric_limits<float>::quiet_NaN();
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const size_t R = (size_t)rows, o = (size_t)t * R;
        if (score) std::fill(score + o, score + o + R, 0.f);
        if (opt_mean) std::fill(opt_mean + (size_t)t * S, opt_mean + (size_t)(t + 1) * S, 0.f);
        if (opt_var) std::fill(opt_var + (size_t)t * S, opt_var + (size_t)(t + 1) * S, 0.f);
        init_topk(top_idx, top_val, t, k);
        PoolState st;
        if (!pool_state(b, phi, t, X, rows, info, st)) continue;
        const Mat &mu = st.mu, &v = st.v;
        const double noise = st.noise;
        int s_eff = 0;
        bool bad = false;
        Mat sum(R, 0.0), col(R);
        for (int j = 0; j < S; ++j) {
            const int64_t p = opt_idx[(size_t)t * S + j];
            if (p < 0 || p >= rows) continue;
            ++s_eff;
            const double fs = opt_val[(size_t)t * S + j];
            if (!std::isfinite(fs)) bad = true;
            if (opt_mean) opt_mean[(size_t)t * S + j] = (float)mu[p];
            if (opt_var) opt_var[(size_t)t * S + j] = (float)v[p];
            const double dd = std::max(v[p], 1e-12) + (double)cond_noise, gain = (fs - mu[p]) / dd;
            c0_col(st, b, X, p, col.data());
            for (size_t r = 0; r < R; ++r) {
                const double c0 = col[r];
                const double vc = std::max(v[r], 1e-12), vs = std::max(v[r] - c0 * c0 / dd, 1e-12), ms = mu[r] + c0 * gain;
                const double g = (maximize ? (fs - ms) : (ms - fs)) / std::sqrt(vs);
                sum[r] += std::log((vc + noise) / (vs + noise)) - gibbon_term(g, vs / (vs + noise));
            }
        }
        std::vector<float> sc(R);
        for (size_t r = 0; r < R; ++r) {
            const bool nan = s_eff == 0 || bad || mu[r] != mu[r] || v[r] != v[r];
            sc[r] = nan ? fnan : (float)(0.5 * sum[r] / s_eff);
            if (score) score[o + r] = sc[r];
        }
        if (k > 0) select_topk(sc, rows, k, excl_range(excl_idx, excl_off, t), top_idx + (size_t)t * k, top_val + (size_t)t * k);
    }
    return 0;
}

size_t adkf_jackknife_pool_scratch_bytes(int32_t, int32_t, int32_t, int32_t) { return 0; }

// Leave-one-out checks and jackknife+ intervals over a shared pool (include/adkf_gp.h), in float64 throughout: the leave-one-out state
// from A^-1 and alpha, per row c = k A^-1, the fold values, and the two order statistics per level by a partial sort; everything is
// rounded to float32 at the boundary, and the selection ranks the float32 level-0 score under adkf_predict_pool's total order.
int adkf_jackknife_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* alpha, int32_t L,
                        const int64_t* excl_idx, const int64_t* excl_off, float* lo, float* hi, float* loo_mean, float* loo_var, float* loo_lpd,
                        int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void*, size_t, void*, size_t, void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~(ADKF_PM_MAXIMIZE | ADKF_PM_JK_SCALED)) return ADKF_E_BADARG;
    if (!alpha) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k == 0 && !lo && !hi && !loo_mean && !loo_var && !loo_lpd) return ADKF_E_BADARG;
    if (int rc = check_topk(k, top_idx, top_val)) return rc;
    if (b->ns_max > ADKF_JK_POINTS_MAX || L < 1 || L > ADKF_JK_LEVELS_MAX) return ADKF_E_SIZE;
    const float ninf = -std::numeric_limits<float>::infinity(), pinf = std::numeric_limits<float>::infinity();
    const bool maximize = (flags & ADKF_PM_MAXIMIZE) != 0, scaled = (flags & ADKF_PM_JK_SCALED) != 0;
    const size_t ld = (size_t)b->ns_max, R = (size_t)rows;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        if (lo && rows > 0) std::fill(lo + (size_t)t * L * R, lo + (size_t)(t + 1) * L * R, 0.f);
        if (hi && rows > 0) std::fill(hi + (size_t)t * L * R, hi + (size_t)(t + 1) * L * R, 0.f);
        if (loo_mean) std::fill(loo_mean + t * ld, loo_mean + (t + 1) * ld, 0.f);
        if (loo_var) std::fill(loo_var + t * ld, loo_var + (t + 1) * ld, 0.f);
        if (loo_lpd) loo_lpd[t] = 0.f;
        init_topk(top_idx, top_val, t, k);
        const float* y = b->y_s + t * ld;
        std::vector<double> g, bii, wd, a, bb, kr, c;
        std::vector<int> rank(L, 0);
        std::vector<float> sc(R);
        const bool done = pm_task_state(b, phi, t, X, 0, rows, info,
            [&](const Inner& in) {
                const int n = in.n;
                g.resize(n); bii.resize(n); wd.resize(n); a.resize(n); bb.resize(n); kr.resize(n); c.resize(n);
                double lpd = 0.0;
                for (int i = 0; i < n; ++i) {
                    bii[i] = in.Ainv[(size_t)i * n + i];
                    g[i] = in.alpha[i] / bii[i];
                    wd[i] = scaled ? std::fabs(g[i]) * std::sqrt(bii[i]) : std::fabs(g[i]);
                    if (loo_mean) loo_mean[t * ld + i] = (float)((double)y[i] - g[i]);
                    if (loo_var) loo_var[t * ld + i] = (float)(1.0 / bii[i]);
                    lpd += -0.5 * std::log(2.0 * M_PI / bii[i]) - 0.5 * g[i] * g[i] * bii[i];
                }
                if (loo_lpd) loo_lpd[t] = (float)lpd;
                for (int l = 0; l < L; ++l) {
                    const float al = alpha[l];
                    rank[l] = (al > 0.f && al < 1.f) ? (int)std::floor((double)al * (double)(n + 1)) : 0;
                }
            },
            [&](int64_t r, const Inner& in, const double* D) {
                const int n = in.n;
                const MuQ p = row_posterior(in, b->kernel, D, y, kr.data(), c.data());
                const double mu = p.mu, qf = p.q, v = in.s - qf;
                for (int i = 0; i < n; ++i) {
                    const double mi = mu - c[i] * g[i];
                    const double w = scaled ? wd[i] * std::sqrt(std::max(v + c[i] * c[i] / bii[i], 1e-12) + in.noise) : wd[i];
                    a[i] = mi - w; bb[i] = mi + w;
                }
                const bool bad = mu != mu || qf != qf;
                float s0 = 0.f;
                for (int l = 0; l < L; ++l) {
                    float lv = ninf, hv = pinf;
                    if (const int kk = rank[l]; kk > 0) {
                        std::nth_element(a.begin(), a.begin() + (kk - 1), a.end());
                        std::nth_element(bb.begin(), bb.begin() + (kk - 1), bb.end(), std::greater<double>());
                        lv = (float)a[kk - 1]; hv = (float)bb[kk - 1];
                    }
                    if (bad) lv = hv = std::numeric_limits<float>::quiet_NaN();
                    if (lo) lo[((size_t)t * L + l) * R + r] = lv;
                    if (hi) hi[((size_t)t * L + l) * R + r] = hv;
                    if (l == 0) s0 = maximize ? lv : -hv;
                }
                sc[r] = std::isinf(s0) ? std::numeric_limits<float>::quiet_NaN() : s0;
            });
        if (done && k > 0) select_topk(sc, rows, k, excl_range(excl_idx, excl_off, t), top_idx + (size_t)t * k, top_val + (size_t)t * k);
    }
    return 0;
}

size_t adkf_ehvi_pool_scratch_bytes(int32_t, int32_t, int32_t) { return 0; }

// log(1 - exp(d)), d < 0
static double log1mexp(double d) { return d > -M_LN2 ? std::log(-std::expm1(d)) : std::log1p(-std::exp(d)); }

// log Phi(z): log1p where Phi -> 1, through erfc down to z = -30, Mills' ratio below
static double log_cdf(double z) {
    if (z > 0.0) return std::log1p(-0.5 * std::erfc(z / std::sqrt(2.0)));
    if (z > -30.0) return std::log(0.5 * std::erfc(-z / std::sqrt(2.0)));
    const double w = 1.0 / (z * z);
    return -0.5 * z * z - std::log(-z) - 0.5 * std::log(2.0 * M_PI) + std::log1p(w * (-1.0 + w * (3.0 - 15.0 * w)));
}

// Constrained expected hypervolume improvement across tasks over a shared pool (include/adkf_gp.h): the mean and the latent variance
// of every task at every pool row first, then per group the staircase (the device's cleaning rule, on the float32 values) and the score
// in float64 - the log form in log space throughout - rounded to float32 at the boundary; the selection ranks those float32 values
// under adkf_predict_pool's total order.
int adkf_ehvi_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, int32_t G, const int32_t* obj,
                   const int32_t* obj_max, const float* ref, const float* front, const int32_t* front_n, int32_t P, const int32_t* con,
                   const float* con_thr, const int32_t* con_geq, int32_t C, const int64_t* excl_idx, const int64_t* excl_off, float* score,
                   float* stair, int32_t* stair_n, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void*, size_t, void*, size_t,
                   void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~ADKF_PM_LOG_EI) return ADKF_E_BADARG;
    if (G < 1 || k < 0) return ADKF_E_BADARG;
    if (P < 0 || P > ADKF_EHVI_FRONT_MAX || C < 0 || C > ADKF_EHVI_CONS_MAX || k > ADKF_POOL_TOPK_MAX) return ADKF_E_SIZE;
    if (!obj || !ref || !front_n) return ADKF_E_BADARG;
    if (P > 0 && !front) return ADKF_E_BADARG;
    if (C > 0 && (!con || !con_thr || !con_geq)) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (int rc = check_topk(k, top_idx, top_val)) return rc;   // (the sizes come first here: only the two outputs are left to ask for)
    if (k == 0 && !score && !stair && !stair_n) return ADKF_E_BADARG;
    const bool want_log = (flags & ADKF_PM_LOG_EI) != 0;
    const int T = b->T;
    const size_t R = (size_t)rows;
    const float fnan = std::numeric_limits<float>::quiet_NaN();
    const double dinf = std::numeric_limits<double>::infinity();
    Mat mu((size_t)T * R), vl((size_t)T * R);
    std::vector<char> done(T, 0);
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < T; ++t) {
        const float* y = b->y_s + (size_t)t * b->ns_max;
        std::vector<double> kr(b->ns_max);
        done[t] = pm_task(b, phi, t, X, 0, rows, info, [&](int64_t r, const Inner& in, const double* D) {
            const MuQ p = row_posterior(in, b->kernel, D, y, kr.data(), nullptr);
            mu[(size_t)t * R + r] = p.mu; vl[(size_t)t * R + r] = in.s - p.q;
        }) ? 1 : 0;
    }
    auto psi = [&](double m, double s, double c, bool lg) {
        if (c == -dinf) return lg ? -dinf : 0.0;
        const double z = (c - m) / s;
        if (lg) return std::log(s) + log_h(z);
        return s * (z * 0.5 * std::erfc(-z / std::sqrt(2.0)) + std::exp(-0.5 * z * z) / std::sqrt(2.0 * M_PI));
    };
#pragma omp parallel for schedule(dynamic)
    for (int g = 0; g < G; ++g) {
        const int o1 = obj[2 * g], o2 = obj[2 * g + 1];
        const bool two = o2 != -1;
        bool bad = o1 < 0 || o1 >= T || (two && (o2 < 0 || o2 >= T || o2 == o1));
        const float sg1 = (obj_max && obj_max[2 * g]) ? -1.f : 1.f, sg2 = (obj_max && obj_max[2 * g + 1]) ? -1.f : 1.f;
        const float r1 = sg1 * ref[2 * g], r2 = two ? sg2 * ref[2 * g + 1] : 0.f;
        bad = bad || r1 != r1 || r2 != r2;
        if (!bad) bad = !done[o1] || (two && !done[o2]);
        int ct[ADKF_EHVI_CONS_MAX];
        for (int c = 0; c < ADKF_EHVI_CONS_MAX; ++c) {
            ct[c] = c < C ? con[(size_t)g * C + c] : -1;
            if (ct[c] == -1) continue;
            if (ct[c] < 0 || ct[c] >= T) { bad = true; ct[c] = -1; continue; }
            const float thr = con_thr[(size_t)g * C + c];
            if (thr != thr || !done[ct[c]]) bad = true;
        }
        // the staircase
        int n = two ? front_n[g] : 0;
        n = std::min(std::max(n, 0), (int)P);
        std::vector<float> fa(n), fb(n);
        std::vector<char> keep(n);
        for (int i = 0; i < n; ++i) {
            fa[i] = sg1 * front[((size_t)g * P + i) * 2]; fb[i] = sg2 * front[((size_t)g * P + i) * 2 + 1];
            keep[i] = fa[i] == fa[i] && fb[i] == fb[i] && fa[i] < r1 && fb[i] < r2;
        }
        const std::vector<char> valid = keep;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n && keep[i]; ++j)
                if (valid[j] && j != i && fa[j] <= fa[i] && fb[j] <= fb[i] && (fa[j] < fa[i] || fb[j] < fb[i] || j < i)) keep[i] = 0;
        std::vector<std::pair<float, float>> st;
        for (int i = 0; i < n; ++i) if (keep[i]) st.emplace_back(fa[i], fb[i]);
        std::sort(st.begin(), st.end());
        const int Pg = (int)st.size();
        if (stair_n) stair_n[g] = Pg;
        if (stair)
            for (int i = 0; i < P; ++i) {
                stair[((size_t)g * P + i) * 2] = i < Pg ? sg1 * st[i].first : 0.f;
                stair[((size_t)g * P + i) * 2 + 1] = i < Pg ? sg2 * st[i].second : 0.f;
            }
        init_topk(top_idx, top_val, g, k);
        std::vector<float> sc(R, fnan);
        if (!bad) {
            for (size_t r = 0; r < R; ++r) {
                const double m1 = (double)sg1 * mu[(size_t)o1 * R + r], s1 = std::sqrt(std::max(vl[(size_t)o1 * R + r], 1e-12));
                double val;   // EHVI or its logarithm
                if (!two) {
                    val = psi(m1, s1, r1, want_log);
                } else {
                    const double m2 = (double)sg2 * mu[(size_t)o2 * R + r], s2 = std::sqrt(std::max(vl[(size_t)o2 * R + r], 1e-12));
                    std::vector<double> term(Pg + 1);
                    double lo = want_log ? -dinf : 0.0;
                    for (int i = 0; i <= Pg; ++i) {
                        const double hi = psi(m1, s1, i < Pg ? st[i].first : r1, want_log);
                        const double f2 = psi(m2, s2, i == 0 ? r2 : st[i - 1].second, want_log);
                        if (want_log) {
                            double w = hi;
                            if (i > 0 && hi != -dinf) w = lo - hi >= 0.0 ? -dinf : hi + log1mexp(lo - hi);
                            term[i] = w + f2;
                        } else {
                            term[i] = (hi - lo) * f2;
                        }
                        lo = hi;
                    }
                    if (want_log) {
                        double mx = -dinf, sum = 0.0;
                        bool nan = false;
                        for (double x : term) { if (x != x) nan = true; else mx = std::max(mx, x); }
                        for (double x : term) if (x != -dinf) sum += std::exp(x - mx);
                        val = nan ? std::numeric_limits<double>::quiet_NaN() : (sum == 0.0 ? -dinf : mx + std::log(sum));
                    } else {
                        val = 0.0;
                        for (double x : term) val += x;
                    }
                }
                double w = want_log ? 0.0 : 1.0;
                for (int c = 0; c < ADKF_EHVI_CONS_MAX; ++c) {
                    if (ct[c] < 0) continue;
                    const double mc = mu[(size_t)ct[c] * R + r], sd = std::sqrt(std::max(vl[(size_t)ct[c] * R + r], 1e-12));
                    const double thr = con_thr[(size_t)g * C + c];
                    const double z = (con_geq[(size_t)g * C + c] ? (mc - thr) : (thr - mc)) / sd;
                    if (want_log) w += log_cdf(z); else w *= 0.5 * std::erfc(-z / std::sqrt(2.0));
                }
                sc[r] = (float)(want_log ? val + w : val * w);
            }
        }
        if (score) std::copy(sc.begin(), sc.end(), score + (size_t)g * R);
        if (!bad && k > 0) select_topk(sc, rows, k, excl_range(excl_idx, excl_off, g), top_idx + (size_t)g * k, top_val + (size_t)g * k);
    }
    return 0;
}

size_t adkf_rank_pool_scratch_bytes(int32_t, int32_t, int32_t, int32_t) { return 0; }

// Large-k selection and row ranks (include/adkf_gp.h): adkf_predict_pool's score on every row, select_topk without the cap of 64, and
// for a named row the number of eligible rows that come before it in select_topk's order.
int adkf_rank_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f,
                   const int64_t* excl_idx, const int64_t* excl_off, int32_t k, int64_t* top_idx, float* top_val, const int64_t* ref_idx,
                   int32_t M, int64_t* ref_rank, float* ref_val, int64_t* n_ranked, int32_t* info, void*, size_t, void*, size_t, void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~(ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_SCORE_MEAN | ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    const bool by_mean = (flags & ADKF_PM_SCORE_MEAN) != 0;
    if (by_mean && (flags & ADKF_PM_LOG_EI)) return ADKF_E_BADARG;
    if (k < 0 || M < 0) return ADKF_E_BADARG;
    if (k > ADKF_RANK_K_MAX || M > ADKF_RANK_REFS_MAX) return ADKF_E_SIZE;
    if (!by_mean && !best_f) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (k > 0 && (!top_idx || !top_val)) return ADKF_E_BADARG;
    if (M > 0 && (!ref_idx || !ref_rank || !ref_val)) return ADKF_E_BADARG;
    if (k == 0 && M == 0 && !n_ranked) return ADKF_E_BADARG;
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        init_topk(top_idx, top_val, t, k);
        for (int j = 0; j < M; ++j) { ref_rank[(size_t)t * M + j] = -1; ref_val[(size_t)t * M + j] = std::numeric_limits<float>::quiet_NaN(); }
        if (n_ranked) n_ranked[t] = 0;
        std::vector<float> sc((size_t)rows);
        const bool done = pm_task(b, phi, t, X, 0, rows, info, [&](int64_t r, const Inner& in, const double* D) {
            float m1, e1 = 0.f;
            pm_row(in, b->kernel, D, b->y_s + (size_t)t * b->ns_max, flags, best_f, t, 0, &m1, nullptr, by_mean ? nullptr : &e1);
            sc[r] = by_mean ? ((flags & ADKF_PM_MAXIMIZE) ? m1 : -m1) : e1;
        });
        if (!done) continue;
        const Excl excl = excl_range(excl_idx, excl_off, t);
        if (k > 0) select_topk(sc, rows, k, excl, top_idx + (size_t)t * k, top_val + (size_t)t * k);
        std::vector<char> ok((size_t)rows);
        int64_t n = 0;
        for (int64_t r = 0; r < rows; ++r) n += (ok[r] = sc[r] == sc[r] && !excl.has(r));
        if (n_ranked) n_ranked[t] = n;
        for (int j = 0; j < M; ++j) {
            const int64_t p = ref_idx[(size_t)t * M + j];
            if (p < 0 || p >= rows || sc[p] != sc[p]) continue;
            int64_t c = 0;
            for (int64_t r = 0; r < rows; ++r) c += ok[r] && (sc[r] > sc[p] || (sc[r] == sc[p] && r < p));
            ref_rank[(size_t)t * M + j] = c; ref_val[(size_t)t * M + j] = sc[p];
        }
    }
    return 0;
}

size_t adkf_mix_pool_scratch_bytes(int32_t, int32_t, int32_t) { return 0; }

// Hyperparameter-marginalised prediction and acquisition over a shared pool (include/adkf_gp.h): the members' mean, variance and EI
// (log EI) of every task at every pool row first - adkf_predict_pool's float32 values, which is what the header defines the
// mixture on - then per group the mixture in float64, rounded to float32 at the boundary; the selection ranks those float32 values
// under adkf_predict_pool's total order.
int adkf_mix_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, int32_t G, const int32_t* mem,
                  const float* w, int32_t M, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off, float* mean,
                  float* var, float* score, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void*, size_t, void*, size_t,
                  void*) {
    if (int rc = check_support_only(b, phi, info, rows, ARD_EITHER)) return rc;
    if (flags & ~(ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_SCORE_MEAN | ADKF_PM_LOG_EI | ADKF_PM_SCORE_BALD)) return ADKF_E_BADARG;
    const bool by_mean = (flags & ADKF_PM_SCORE_MEAN) != 0, by_bald = (flags & ADKF_PM_SCORE_BALD) != 0, lg = (flags & ADKF_PM_LOG_EI) != 0;
    if ((by_mean && by_bald) || (lg && (by_mean || by_bald))) return ADKF_E_BADARG;
    if (G < 1 || M < 1 || !mem || k < 0) return ADKF_E_BADARG;
    if (M > ADKF_MIX_MEMBERS_MAX || k > ADKF_POOL_TOPK_MAX) return ADKF_E_SIZE;
    const bool want_score = score || k > 0, want_e = want_score && !by_mean && !by_bald;
    if (want_e && !best_f) return ADKF_E_BADARG;
    if (!pool_args_ok(X, rows, excl_idx, excl_off)) return ADKF_E_BADARG;
    if (int rc = check_topk(k, top_idx, top_val)) return rc;   // (the sizes come first here: only the two outputs are left to ask for)
    if (k == 0 && !mean && !var && !score) return ADKF_E_BADARG;
    const int T = b->T;
    const size_t R = (size_t)rows;
    const float fnan = std::numeric_limits<float>::quiet_NaN();
    const double dinf = std::numeric_limits<double>::infinity();
    const int pm_flags = flags & (ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI);
    std::vector<float> mu((size_t)T * R), vr((size_t)T * R), ei(want_e ? (size_t)T * R : 0);
    std::vector<char> done(T, 0);
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < T; ++t)
        done[t] = pm_task(b, phi, t, X, 0, rows, info, [&](int64_t r, const Inner& in, const double* D) {
            float e1 = 0.f;
            pm_row(in, b->kernel, D, b->y_s + (size_t)t * b->ns_max, pm_flags, best_f, t, 0, &mu[(size_t)t * R + r], &vr[(size_t)t * R + r],
                   want_e ? &e1 : nullptr);
            if (want_e) ei[(size_t)t * R + r] = e1;
        }) ? 1 : 0;
#pragma omp parallel for schedule(dynamic)
    for (int g = 0; g < G; ++g) {
        // the used entries in entry order, W their float32 sum in that order
        std::vector<int> ts;
        std::vector<float> ws;
        bool bad = false;
        float W = -0.f;
        for (int j = 0; j < M; ++j) {
            const int t = mem[(size_t)g * M + j];
            if (t == -1) continue;
            const float wj = w ? w[(size_t)g * M + j] : 1.f;
            if (t < 0 || t >= T || !(wj >= 0.f) || std::isinf(wj)) { bad = true; continue; }
            if (!(wj > 0.f)) continue;
            if (!done[t]) bad = true;
            ts.push_back(t); ws.push_back(wj); W += wj;
        }
        bad = bad || ts.empty() || !std::isfinite(W);
        const int n = (int)ts.size();
        std::vector<double> wt(n);
        for (int i = 0; i < n; ++i) wt[i] = (double)(ws[i] / W);
        init_topk(top_idx, top_val, g, k);
        std::vector<float> sc(R, fnan);
        for (size_t r = 0; r < R; ++r) {
            const size_t o = (size_t)g * R + r;
            if (bad) {
                if (mean) mean[o] = fnan;
                if (var) var[o] = fnan;
                continue;
            }
            double m1 = 0.0, within = 0.0, between = 0.0, wc = 0.0, sl = 0.0, se = 0.0, mx = -dinf;
            for (int i = 0; i < n; ++i) m1 += wt[i] * (double)mu[(size_t)ts[i] * R + r];
            for (int i = 0; i < n; ++i) {
                const size_t q = (size_t)ts[i] * R + r;
                const double vi = vr[q], dev = (double)mu[q] - m1, vc = vi < 1e-12 ? 1e-12 : vi;
                within += wt[i] * vi; between += wt[i] * dev * dev;
                wc += wt[i] * vc; sl += wt[i] * std::log(vc);
                if (want_e) { const double e1 = ei[q]; if (lg) { if (e1 == e1) mx = std::max(mx, e1); } else se += wt[i] * e1; }
            }
            if (mean) mean[o] = (float)m1;
            if (var) var[o] = (float)(within + between);
            if (!want_score) continue;
            double val;
            if (by_mean) val = (flags & ADKF_PM_MAXIMIZE) ? m1 : -m1;
            else if (by_bald) val = 0.5 * (std::log(wc + between) - sl);
            else if (!lg) val = se;
            else {
                double sum = 0.0;
                for (int i = 0; i < n; ++i) { const double e1 = ei[(size_t)ts[i] * R + r]; if (e1 != -dinf) sum += wt[i] * std::exp(e1 - mx); }
                val = sum == 0.0 ? -dinf : mx + std::log(sum);
            }
            sc[r] = (float)val;
        }
        if (score) std::copy(sc.begin(), sc.end(), score + (size_t)g * R);
        if (!bad && k > 0) select_topk(sc, rows, k, excl_range(excl_idx, excl_off, g), top_idx + (size_t)g * k, top_val + (size_t)g * k);
    }
    return 0;
}

static int outer_common(const adkf_batch_t* b, const float* phi, int flags, bool with_hessian, float* f_out, float* g_phi, float* dZ_s, float* dZ_q,
                        float* v_out, float* H_out, int32_t* info) {
    const int d = b->d;
    const bool direct = !(flags & ADKF_IGNORE_DIRECT_GRAD), corr = with_hessian && !(flags & ADKF_IGNORE_GRAD_CORRECTION);
#pragma omp parallel for schedule(dynamic)
    for (int t = 0; t < b->T; ++t) {
        const int n = ns_of(b, t), m = nq_of(b, t);
        const float *Zs = b->Z_s + (size_t)t * b->ns_max * d, *Zq = b->Z_q + (size_t)t * b->nq_max * d;
        const double p[3] = {phi[t * 3], phi[t * 3 + 1], phi[t * 3 + 2]};
        Inner in = inner_stage(sqdist(Zs, n, Zs, n, d), b->y_s + (size_t)t * b->ns_max, n, p, b->priors + t * 4, b->kernel, with_hessian, true);
        info[t] = in.info;
        if (dZ_s) std::memset(dZ_s + (size_t)t * b->ns_max * d, 0, sizeof(float) * (size_t)b->ns_max * d);
        if (dZ_q) std::memset(dZ_q + (size_t)t * b->nq_max * d, 0, sizeof(float) * (size_t)b->nq_max * d);
        if (in.info) { f_out[t] = std::numeric_limits<float>::infinity(); continue; }
        Outer o = outer_stage(sqdist(Zq, m, Zs, n, d), sqdist(Zq, m, Zq, m, d), b->y_q + (size_t)t * b->nq_max, m, in, b->kernel, true);
        f_out[t] = (float)o.f_out;
        if (o.info) { info[t] = o.info; continue; }
        if (g_phi) for (int q = 0; q < 3; ++q) g_phi[t * 3 + q] = (float)o.g_out[q];
        double v[3] = {0, 0, 0};
        if (with_hessian) {
            solve3(in.H, o.g_out, v);
            if (v_out) for (int q = 0; q < 3; ++q) v_out[t * 3 + q] = (float)v[q];
            if (H_out) for (int q = 0; q < 9; ++q) H_out[t * 9 + q] = (float)in.H[q];
        }
        Mat Wss((size_t)n * n, 0.0);
        if (direct) Wss = o.W_ss;
        if (corr) { Mat Wm = mixed_stage(v, in); for (size_t q = 0; q < Wss.size(); ++q) Wss[q] -= Wm[q]; }
        dz_from_weights(Zs, n, Zq, m, d, &Wss, direct ? &o.W_qs : nullptr, direct ? &o.W_qq : nullptr,
                        dZ_s ? dZ_s + (size_t)t * b->ns_max * d : nullptr, dZ_q ? dZ_q + (size_t)t * b->nq_max * d : nullptr, d);
    }
    return 0;
}

int adkf_outer_nll_value_grad(const adkf_batch_t* b, const float* phi, float* f_out, float* g_phi, float* dZ_s, float* dZ_q, int32_t* info,
                              void*, size_t, void*) {
    if (int rc = check(b, true)) return rc;
    if (!phi || !f_out || !info || !b->y_s || !b->y_q || !b->priors) return ADKF_E_BADARG;
    return outer_common(b, phi, 0, false, f_out, g_phi, dZ_s, dZ_q, nullptr, nullptr, info);
}

int adkf_ift_hypergrad(const adkf_batch_t* b, const float* phi, int32_t flags, float* f_out, float* dZ_s, float* dZ_q, float* g_phi_out, float* v,
                       float* H, int32_t* info, void*, size_t, void*) {
    if (int rc = check(b, true)) return rc;
    if (!phi || !f_out || !dZ_s || !dZ_q || !info || !b->y_s || !b->y_q || !b->priors) return ADKF_E_BADARG;
    return outer_common(b, phi, flags, true, f_out, g_phi_out, dZ_s, dZ_q, v, H, info);
}

}  // extern "C"
