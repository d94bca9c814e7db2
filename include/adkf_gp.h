/*
 * adkf_gp.h - C ABI of libadkf_gp.so: the MI355X (gfx950) batched exact-GP / IFT-hypergradient path of
 * ADKF-IFT's inner loop.
 *
 * The reference (Wenlin-Chen/ADKF-IFT) is pure Python and has NO foreign-function interface for this
 * path: every GP operation is a GPyTorch/BoTorch call made from fs_mol/models/adaptive_dkt.py and
 * fs_mol/utils/adaptive_dkt_utils.py.  Each entry point below names the reference call site(s) it
 * replaces; INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions:
 *   - plain `extern "C"`, no exceptions, no ownership transfer: the caller allocates every input, output
 *     and the workspace (device memory, e.g. torch tensors' data_ptr()) and passes raw pointers + sizes;
 *   - all matrices are contiguous row-major float32: Z_s [T, ns_max, d], Z_q [T, nq_max, d],
 *     y_s [T, ns_max], y_q [T, nq_max], phi [T, 3], priors [T, 4];  per-task true sizes n_s[T], n_q[T]
 *     (int32, device; NULL = every task uses ns_max / nq_max).  Rows >= n are padding and are ignored on
 *     input and written as 0 on output;
 *   - phi[t] = (raw_noise, raw_outputscale, raw_lengthscale) in the reference's gp_params() order
 *     (fs_mol/models/adaptive_dkt.py:81-86); noise = softplus(raw)+1e-4, outputscale / lengthscale =
 *     softplus(raw);
 *   - priors[t] = (noise_loc, noise_scale, ls_loc, ls_scale): LogNormal priors of
 *     fs_mol/models/adaptive_dkt.py:94-100,112-119; a scale <= 0 disables that prior (DKLModel has no
 *     noise prior, fs_mol/models/dkl.py:86; use_lengthscale_prior=False);
 *   - every function is ASYNCHRONOUS on `stream` (a hipStream_t passed as void*), re-entrant across
 *     streams, and performs no allocation; no synchronisation either, with ONE documented exception: the
 *     multi-launch fits (more than 128 points; ARD) poll a convergence counter every few evaluations in
 *     convergence mode - never in exact-evals mode and never while the stream is being captured - so every
 *     sequence may be captured into a hipGraph.  State kept across calls: a thread-local last-HIP-error
 *     (adkf_last_hip_error), the outcome of the dynamic-LDS opt-ins (asked once per process; see
 *     adkf_path_info) and read-once environment switches for experiments (ADKF_* in DESIGN.md section 1);
 *     nothing a call leaves behind changes what a later call computes;
 *   - return value: 0 = enqueued, < 0 = rejected argument (ADKF_E_*).  Numerical failure is reported
 *     per task in the device array info[T]: 0 = ok, k > 0 = the k-th pivot of a Cholesky factorisation was
 *     not positive (the reference's NotPSDError after jitter retries; this library never adds jitter),
 *     with ADKF_INFO_OUTER_BASE added when it was the N_q x N_q predictive covariance.  For a task the call
 *     sent through the float64 path (ill-conditioned: DESIGN.md section 3.5) info[] is the verdict of the float64
 *     factorisations, which produced everything the call returns for it - not of the float32 sweeps before them.
 *     adkf_check_info() synchronises and folds info[] into one status (index+1 of the first bad task).
 */
#ifndef ADKF_GP_H
#define ADKF_GP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADKF_KERNEL_RBF 0      /* gpytorch ScaleKernel(RBFKernel)            fs_mol/utils/gp_utils.py:26-27 */
#define ADKF_KERNEL_MATERN52 1 /* gpytorch ScaleKernel(MaternKernel nu=2.5)  fs_mol/utils/gp_utils.py:29-30 */

#define ADKF_E_BADARG (-1)
#define ADKF_E_SIZE (-2)      /* a dimension is outside what this build supports (see adkf_max_points) */
#define ADKF_E_WORKSPACE (-3) /* workspace too small */
#define ADKF_E_LAUNCH (-4)    /* the HIP runtime refused a launch */

#define ADKF_INFO_OUTER_BASE 100000

/* adkf_batch_t.flags: promises that let consecutive calls on the SAME batch (same pointers, shape, kernel) and the
 * SAME workspace skip work that is already there.  The usual meta-step sequence is
 *   adkf_init_params (flags 0) -> adkf_fit (REUSE_DIST) -> adkf_ift_hypergrad (REUSE_DIST | REUSE_INNER). */
#define ADKF_BATCH_REUSE_DIST 1  /* squared distances (incl. query blocks when Z_q was given) are in the workspace */
#define ADKF_BATCH_REUSE_INNER 2 /* A^-1, alpha and the scalars of exactly this phi are in the workspace (adkf_fit
                                    leaves them for its result; adkf_mll_value_grad for its argument) */

#define ADKF_BATCH_DEFER_REFINE 8 /* adkf_fit only: skip the float64 re-evaluation of ill-conditioned tasks at phi* (csrc/refine64.h) - the
                                    caller goes on to adkf_ift_hypergrad / adkf_outer_nll_value_grad / adkf_predict with REUSE_INNER on
                                    this workspace, which redo those tasks in float64 themselves; f_final / gnorm of such tasks are
                                    then the float32 values */

#define ADKF_BATCH_LG_UNFUSED 16 /* more than 128 points only, A/B runs and tests: the blocked sweep as three launches per block step
                                    (k_lg_diag, panel, update: csrc/large.h) instead of the update of step k and the diagonal sweep of
                                    step k + 1 in one launch (csrc/large_fused.h).  Both give bit-identical results. */
#define ADKF_BATCH_LG_FUSED 32   /* ... and the fused form whatever the size (without either flag: fused from 512 points on, where it is faster) */
#define ADKF_BATCH_DZ_TILED 64   /* A/B runs and tests: dL/dZ by the tiled launches whatever the shape (without it a full batch of 128 support
                                    and 128 query points takes one launch, csrc/dz_task.h).  Both give bit-identical results. */

/* ARD kernel (``use_ard``: fs_mol/models/adaptive_dkt.py:107-108 -> gpytorch ``ard_num_dims``): one lengthscale per
 * feature dimension.  With this flag EVERY phi / g_phi / v argument has h = 2 + d entries per task, laid out
 * (raw_noise, raw_outputscale, raw_lengthscale[0..d)); priors stay [T,4] (the lengthscale prior applies to each
 * dimension and is summed, as gpytorch does); the workspace must have adkf_workspace_bytes_ard() bytes; the h x h
 * Hessian is never formed (pass H = NULL): adkf_ift_hypergrad solves H v = grad f_out by conjugate gradients on
 * closed-form Hessian-vector products.  REUSE_DIST is ignored (distances depend on the lengthscales). */
#define ADKF_BATCH_ARD 4
#define ADKF_CG_DEFAULT_MAXITER 48
#define ADKF_CG_DEFAULT_TOL 1e-6f
#define ADKF_INFO_CG_BASE 200000 /* info = 200000 + k: CG met non-positive curvature at iteration k (H not PD) */

/* flags of adkf_ift_hypergrad: fs_mol/utils/cauchy_hypergradient.py:11-13 */
#define ADKF_IGNORE_GRAD_CORRECTION 1
#define ADKF_IGNORE_DIRECT_GRAD 2

typedef struct adkf_batch {
    int32_t T;          /* tasks */
    int32_t ns_max;     /* padded support rows */
    int32_t nq_max;     /* padded query rows (0 when no query set is involved) */
    int32_t d;          /* feature dimension */
    int32_t kernel;     /* ADKF_KERNEL_* */
    int32_t flags;      /* ADKF_BATCH_* reuse promises (0 = recompute everything) */
    const int32_t* n_s; /* [T] or NULL */
    const int32_t* n_q; /* [T] or NULL */
    const float* Z_s;   /* [T, ns_max, d] */
    const float* y_s;   /* [T, ns_max] */
    const float* Z_q;   /* [T, nq_max, d] or NULL */
    const float* y_q;   /* [T, nq_max] or NULL */
    const float* priors; /* [T, 4] */
} adkf_batch_t;

typedef struct adkf_fit_options {
    int32_t max_evals; /* hard cap on MLL value+gradient evaluations per task (SciPy maxfun) */
    int32_t exact_evals; /* != 0: spend exactly max_evals evaluations (benchmark mode, deterministic work): same stopping
                          * rules, but a converged task re-evaluates at its optimum until the budget is used up */
    float gtol;        /* stop when max|grad| <= gtol          (SciPy L-BFGS-B pgtol, default 1e-5) */
    float ftol;        /* stop when rel. decrease <= ftol      (SciPy factr*eps: 2.22e-9 is the reference setting) */
    void* ev_start;    /* optional hipEvent_t recorded on `stream` immediately before the optimiser kernel */
    void* ev_stop;     /* optional hipEvent_t recorded immediately after it (roofline timing in bench.py) */
} adkf_fit_options_t;

const char* adkf_version(void);

/* Diagnostics: the HIP runtime's description of the error behind the calling thread's last ADKF_E_LAUNCH. */
const char* adkf_last_hip_error(void);

/* Diagnostics: which kernels a batch padded to (ns_max, nq_max) takes ON THIS DEVICE (needs a GPU: it asks the runtime for the
 * dynamic-LDS opt-ins exactly as the entry points do), as a mask of ADKF_PATH_* bits, or ADKF_E_SIZE.  The library never computes
 * anything else than what the header promises, but two of its fast paths depend on an opt-in the runtime may refuse, and then the
 * slower pipeline runs silently: this is where a caller (bench.py prints it) sees which one is live. */
#define ADKF_PATH_FUSED_OUTER 1    /* 64 < max(ns, nq) <= 128: the outer / hypergradient stage of a task as ONE kernel (csrc/hyper.h, 159 KB of
                                      dynamic LDS); clear: the sixteen-launch pipeline */
#define ADKF_PATH_BLOCKED 2        /* max(ns, nq) > 128: blocked sweep through L2 / HBM (csrc/large.h) */
#define ADKF_PATH_BLOCKED_FUSED 4  /* ... with update k + sweep k + 1 in one launch (csrc/large_fused.h: from 512 points on); clear: the three launches */
#define ADKF_PATH_R64_REGION 8     /* the workspace of this shape carries the float64 region of the ill-conditioned-task path (csrc/refine64.h) */
#define ADKF_PATH_R64_LDS 16       /* that path's inverses run in 128 KB of dynamic LDS; clear: in global memory */
int adkf_path_info(int32_t ns_max, int32_t nq_max);

/* Largest support/query set this build handles in its LDS-resident factorisation. */
int adkf_max_points(void);

/* Bytes of device workspace every call below needs for a batch of this shape: per task 4 (4 ns^2 + 4 nq ns + 3 nq^2) bytes of
 * float32 matrices (+ three 128-row panels beyond 128 points) and, up to 1024 points, the float64 region of the ill-conditioned-task
 * path (csrc/refine64.h; about 1.7 x the float32 part: 1.3 MB per task at 128 points, 82 MB at 1024 - every task has one, any of
 * them may be flagged).  Environment ADKF_R64_MAXN=<points> (read once) lowers the batch size up to which that region is carved;
 * larger batches then stay in float32 whatever their conditioning. */
size_t adkf_workspace_bytes(int32_t T, int32_t ns_max, int32_t nq_max, int32_t d);

/* a3: ADKTModel.compute_median_lengthscale_init (fs_mol/models/adaptive_dkt.py:128-131):
 * l0[t] = sqrt(0.5 * lower_median{ |z_i - z_j|^2 : i<j, > 0 }). */
int adkf_median_lengthscale(const adkf_batch_t* b, float* l0, void* ws, size_t ws_bytes, void* stream);

/* a4: ADKTModel.reinit_gp_params / __create_tail_GP (fs_mol/models/adaptive_dkt.py:88-126) and
 * ExactGPLayer.__init__ (fs_mol/utils/gp_utils.py:14-17): fresh per-task phi and priors.
 * noise0 = 0.1 (classification) or 0.01 (numeric labels); writes phi [T,3], priors [T,4], l0 [T] (nullable). */
int adkf_init_params(const adkf_batch_t* b, int32_t use_numeric_labels, int32_t use_lengthscale_prior,
                     float* phi, float* priors, float* l0, void* ws, size_t ws_bytes, void* stream);

/* a5+a6: -ExactMarginalLogLikelihood of the support set = f_inner (fs_mol/models/adaptive_dkt.py:173-176;
 * DKLModel.compute_loss fs_mol/models/dkl.py:155-157): f_in [T], optional d f_in/d phi [T,3] and
 * d f_in/d Z_s [T, ns_max, d]. */
int adkf_mll_value_grad(const adkf_batch_t* b, const float* phi, float* f_in, float* g_phi, float* dZ_s,
                        int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* a7: botorch.optim.fit.fit_gpytorch_scipy(model.mll) (fs_mol/utils/adaptive_dkt_utils.py:91): minimise
 * f_inner over phi, all tasks at once, on the device (quasi-Newton with the exact analytic gradient).
 * phi [T,3] in/out ([T, 2 + d] for ARD batches); f_final [T], gnorm [T] (max|grad| at the result), n_evals [T] are
 * nullable.  Up to 128 support points the whole optimisation is ONE kernel launch.  Larger sets and ARD batches are a
 * sequence of launches per evaluation; there, in convergence mode (exact_evals == 0, max_evals > 16) and outside
 * stream capture, the call synchronises the stream every 8 evaluations to stop enqueueing once every task has
 * finished - with exact_evals != 0 nothing is ever synchronised. */
int adkf_fit(const adkf_batch_t* b, float* phi, const adkf_fit_options_t* opt, float* f_final, float* gnorm,
             int32_t* n_evals, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* a8 (eval branch): gp_likelihood(gp_model(x_q)) (fs_mol/models/adaptive_dkt.py:198-203;
 * fs_mol/models/dkl.py:143-151): posterior mean [T, nq_max], variance diag incl. noise [T, nq_max]
 * (nullable) and full covariance incl. noise [T, nq_max, nq_max] (nullable). */
int adkf_predict(const adkf_batch_t* b, const float* phi, float* mean, float* var, float* cov, int32_t* info,
                 void* ws, size_t ws_bytes, void* stream);

/* Streaming marginal prediction: the predictive mean, variance and Expected Improvement of query rows of ANY number, in a
 * workspace of exactly adkf_workspace_bytes(T, ns_max, 0, d) bytes whatever `rows` is (csrc/predict_stream.h).
 *   b      the support set only: nq_max == 0, Z_q == y_q == NULL (ADKF_E_BADARG otherwise, and for ARD batches, which
 *          go to adkf_predict_marginal_ard below);
 *          REUSE_INNER after adkf_fit on the same batch and workspace (with or without DEFER_REFINE) reuses A^-1, alpha and
 *          the scalars, otherwise they are evaluated at phi as adkf_predict does; REUSE_DIST covers D2ss;
 *   Zq     packed query rows [rows, d]; task t owns rows [q_off[t], q_off[t+1]) (q_off: [T+1] int64, device); every range
 *          is clamped to [0, rows);
 *   mean   [rows]; var [rows] (nullable) includes the noise unless ADKF_PM_LATENT; ei [rows] (nullable, needs best_f [T]):
 *          Expected Improvement sigma (u Phi(u) + phi(u)) on the LATENT variance, u = (best_f - mean) / sigma for
 *          minimisation, (mean - best_f) / sigma with ADKF_PM_MAXIMIZE; info [T] as adkf_predict.  Rows that belong to no
 *          task's range, and the rows of tasks with n_s == 0 or info != 0, are written as 0.
 *          In float32 that EI is 0, or a negative denormal, from about u <= -14.  With ADKF_PM_LOG_EI (needs ei, ADKF_E_BADARG
 *          without) the ei array holds log EI instead: log sigma + log h(u), h(u) = phi(u) + u Phi(u), with the same
 *          sigma = sqrt(max(var_latent, 1e-12)), u, best_f and ADKF_PM_MAXIMIZE sense, evaluated without ever forming EI (Ament et
 *          al., NeurIPS 2023; csrc/predict_stream.h: pm_log_ei).  It is finite for every finite (mean, var, best_f) whose u * u
 *          does not overflow float32 (-inf where it overflows at u < 0), NaN for a NaN mean, and exp of it is the EI above
 *          wherever that one is accurate.  The rows written as 0 stay 0 under the flag: that 0 is the fill value, not a
 *          logarithm. */
#define ADKF_PM_LATENT 1   /* var without the observation noise: the latent f, what BoTorch's analytic EI reads */
#define ADKF_PM_MAXIMIZE 2 /* ei for maximisation (default: minimisation, as bayes_opt.run_gp_ei_bo) */
#define ADKF_PM_LOG_EI 16  /* ei holds log EI, which does not underflow; adkf_predict_pool ranks by it (bit 8 is not a flag) */
int adkf_predict_marginal(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows, const float* best_f, float* mean, float* var, float* ei, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* The same for ARD batches (one lengthscale per feature dimension); exactly the parameters of adkf_predict_marginal.
 *   b      must carry ADKF_BATCH_ARD and be support-only (nq_max == 0, Z_q == y_q == NULL); anything else is ADKF_E_BADARG,
 *          as are a missing Zq with rows > 0, ei without best_f, ADKF_PM_LOG_EI without ei and flag bits other than
 *          ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI.
 *          Every argument is checked before anything is launched;
 *   phi    [T, 2 + d] in the ARD layout (raw_noise, raw_outputscale, raw_lengthscale[0..d));
 *   ws     exactly adkf_workspace_bytes_ard(T, ns_max, 0, d) bytes whatever `rows` is (less: ADKF_E_WORKSPACE);
 *          REUSE_INNER after an ARD adkf_fit on the same batch and workspace reuses the fit's state (mu, the scaled support
 *          features, D2ss, A^-1, alpha, the scalars - the state ARD adkf_predict reuses); otherwise the call evaluates at phi.
 *          REUSE_DIST is ignored, as for every ARD call.
 * Outputs, zeroed rows and info as adkf_predict_marginal; info as ARD adkf_predict reports it. */
int adkf_predict_marginal_ard(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows, const float* best_f, float* mean, float* var, float* ei, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* Feature gradients of streaming prediction: the vector-Jacobian product of adkf_predict_marginal(_ard) with respect to the packed
 * query rows (csrc/grad_stream.h),
 *     dZq[r, :] = d/dZq[r, :] ( g_mean[r] mean[r] + g_var[r] var[r] + g_ei[r] ei[r] ),
 * for saliency at the feature layer, losses on the predictive moments of a query set, and ascent of an acquisition in feature space.
 *   b      support-only as for adkf_predict_marginal; with ADKF_BATCH_ARD in b->flags the call behaves as
 *          adkf_predict_marginal_ard (phi [T, 2 + d], ws of adkf_workspace_bytes_ard(T, ns_max, 0, d) bytes), without it as
 *          adkf_predict_marginal (adkf_workspace_bytes(T, ns_max, 0, d)).  REUSE_DIST / REUSE_INNER mean what they mean there.
 *          The workspace does not depend on rows; every size the library accepts is served.
 *   Zq, q_off, rows, best_f   as adkf_predict_marginal;
 *   flags  ADKF_PM_LATENT | ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI, as there.  The noise is a constant of the row, so ADKF_PM_LATENT changes no
 *          gradient; with ADKF_PM_LOG_EI g_ei is the cotangent of log EI;
 *   g_mean, g_var, g_ei   [rows] each, nullable (a missing one is a cotangent of 0);
 *   dZq    [rows, d], overwritten: the gradient with respect to the RAW row (ARD: the 1 / l of the scaling included).  Rows that
 *          belong to no task's range, and the rows of tasks with n_s == 0 or info != 0, are 0.  A row whose three cotangents are 0 is
 *          exactly 0; a NaN in a row's features or cotangents stays in that row.  With k_i = os kappa(u_i), u_i = |x - z_i|^2 / l^2,
 *          c = k A^-1, alpha = A^-1 y, sigma = sqrt(max(var_latent, 1e-12)):
 *              a_m = g_mean + g_ei dE/dmean,   a_v = g_var + g_ei dE/dvar,   W_i = os kappa'(u_i) (a_m alpha_i - 2 a_v c_i),
 *              dZq[r, :] = (2 / l^2) ( (sum_i W_i) x - sum_i W_i z_i ),
 *          dEI/dmean = -+Phi(u), dEI/dvar = phi(u) / (2 sigma); d log EI/dmean = -+Phi / (sigma h), d log EI/dvar = (phi / h) / (2 var),
 *          the ratios Phi / h and phi / h formed without cancellation for u << 0.  Where the clamp of sigma is active
 *          (var_latent <= 1e-12) the derivative through sigma is 0.
 * ADKF_E_BADARG, before anything is launched: a batch with a query set, rows < 0, rows > 0 without Zq or dZq, no cotangent at all,
 * g_ei without best_f, ADKF_PM_LOG_EI without g_ei, any other flag bit.  A short workspace is ADKF_E_WORKSPACE.
 * Asynchronous, no allocation, capturable, no atomics; a row's result depends on its task and its own features only. */
int adkf_predict_grad(const adkf_batch_t* b, const float* phi, int32_t flags, const float* Zq, const int64_t* q_off, int64_t rows, const float* best_f, const float* g_mean, const float* g_var, const float* g_ei, float* dZq, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* Shared-pool prediction: every task of the batch scores the SAME rows X [rows, d], and the call can return each task's best k
 * rows itself, so that nothing of size T x rows has to exist unless the caller asks for it (Bayesian-optimisation replicates
 * over one candidate pool, virtual screening).
 *   b      support-only as for adkf_predict_marginal; with ADKF_BATCH_ARD in b->flags the call behaves as
 *          adkf_predict_marginal_ard (phi [T, 2 + d], ws of adkf_workspace_bytes_ard(T, ns_max, 0, d) bytes), without it as
 *          adkf_predict_marginal (adkf_workspace_bytes(T, ns_max, 0, d)).  REUSE_DIST / REUSE_INNER mean what they mean there.
 *          The workspace size depends neither on rows nor on k.
 *   flags  ADKF_PM_LATENT, ADKF_PM_MAXIMIZE, ADKF_PM_SCORE_MEAN, ADKF_PM_LOG_EI; any other bit is ADKF_E_BADARG.
 *   mean, var, ei   each nullable, [T, rows] row-major (task t, row r at t * rows + r); the values of the packed call: var
 *          includes the noise unless ADKF_PM_LATENT, ei (needs best_f [T]) is on the latent variance and holds log EI with
 *          ADKF_PM_LOG_EI.  With all three NULL the kernels write nothing per row.
 *   k, top_idx, top_val   k == 0: no selection.  Otherwise ([T, k] each) the score of row r for task t is its ei value (its log EI
 *          with ADKF_PM_LOG_EI: the same maximiser, and an order where float32 EI is 0 on every row), or with
 *          ADKF_PM_SCORE_MEAN +mean under ADKF_PM_MAXIMIZE and -mean without; top_idx[t, 0..k) are the k eligible rows of largest
 *          score in descending score, equal scores in ascending row index (a total order: the answer is unique and independent of
 *          the grid), top_val their scores.  A row is eligible unless it is listed in excl_idx[excl_off[t] .. excl_off[t + 1])
 *          (nullable; int64, each task's range sorted ascending) or its score is NaN.  With fewer than k eligible rows the tail is
 *          top_idx = -1, top_val = -inf.
 *   Tasks with n_s == 0 or info != 0: their [rows] slices are 0 (as the packed call zeroes such rows; under ADKF_PM_LOG_EI too,
 *          where that 0 is the fill value, not a logarithm), their selection -1 / -inf.
 *   scratch   adkf_predict_pool_scratch_bytes(T, k) bytes, 8-byte aligned: the candidate lists of the selection.  It depends
 *          on T and k only (at most 3 MB), never on rows; 0 for k == 0.  Nothing for the caller to initialise.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: a batch with a query set; rows < 0; rows > 0 without X; ei
 * without best_f; k > 0 ranking by ei without best_f; k < 0; k > 0 without top_idx or top_val; no output at all (mean, var, ei
 * NULL and k == 0); ADKF_PM_LOG_EI with nothing that reads it (ei NULL and either k == 0 or ADKF_PM_SCORE_MEAN); excl_idx without
 * excl_off; k > ADKF_POOL_TOPK_MAX (ADKF_E_SIZE); a scratch or a workspace that is too small (ADKF_E_WORKSPACE). */
#define ADKF_PM_SCORE_MEAN 4 /* adkf_predict_pool only: rank by the posterior mean instead of ei (no best_f needed) */
/* ADKF_PM_LOG_EI (16, defined above): ei [T, rows], the EI score and so top_val are log EI; eligibility, order and tail unchanged */
#define ADKF_POOL_TOPK_MAX 64
size_t adkf_predict_pool_scratch_bytes(int32_t T, int32_t k);
int adkf_predict_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off, float* mean, float* var, float* ei, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Thompson sampling over a shared pool from pathwise posterior draws (csrc/thompson_stream.h): every task of the batch draws S
 * functions from its posterior (Matheron's rule on a random-Fourier-feature prior draw; Wilson et al. 2020), and each function
 * picks its own best row of the SAME pool X [rows, d].  The S picks of a task are a diverse batch by construction, no best_f is
 * involved and no tail probability is evaluated.  One pass over the pool; nothing of size rows is kept unless `paths` is given.
 * No reference-side counterpart: the reference has analytic EI only.
 *   The quantity.  With (noise, s, l) from phi[t] under the library's transforms, mu the support column mean of task t, k the
 *          batch's kernel and A = K_ss + noise I, sample q < S of task t is
 *              phi_j(x) = sqrt(2 s / m) cos(omega_j . (x - mu) / l + phase_j)    (j < m),    g(x) = sum_j w[t, q, j] phi_j(x),
 *              r_i = y_i - g(z_i) - sqrt(noise) eps[t, q, i]    (i < n_s[t]),    v = A^-1 r,
 *              f(x) = g(x) + sum_i k(x, z_i) v_i,
 *          and score(x) = +f(x) with ADKF_PM_MAXIMIZE, -f(x) without.  Given the arrays below f is a deterministic function; its
 *          mean over standard normal w, eps is exactly the posterior mean K A^-1 y, whatever m is.
 *   The caller supplies all randomness: omega [m, d] and phase [m], a random-Fourier basis of the kernel AT UNIT LENGTHSCALE shared
 *          by all tasks (RBF: rows N(0, I); Matern-5/2: multivariate Student-t with 5 degrees of freedom; phase uniform on
 *          [0, 2 pi)); w [T, S, m] and eps [T, S, ns_max] standard normal (entries at i >= n_s[t] are ignored).
 *   b      support-only as for adkf_predict_pool, workspace of adkf_workspace_bytes(T, ns_max, 0, d) bytes; REUSE_DIST / REUSE_INNER
 *          mean what they mean there (the inner quantities at phi, or the fit's, plus the float64 A^-1 of flagged tasks).  ARD
 *          batches are refused (ADKF_E_BADARG): they go to adkf_thompson_pool_ard below.
 *   flags  ADKF_PM_MAXIMIZE only.
 *   sel_idx, sel_val   [T, S]: sel_idx[t, q] is the eligible pool row of largest score of sample q, equal scores going to the
 *          lowest row index (the total order of adkf_predict_pool: the answer is unique and independent of the grid), sel_val its
 *          score.  A row is eligible unless it is listed in excl_idx[excl_off[t] .. excl_off[t + 1]) (nullable; as
 *          adkf_predict_pool) or its score is NaN.  With no eligible row: -1 / -inf.
 *   paths  nullable, [T, S, rows] with element (t, q, r) at (t S + q) rows + r: the values f (not the scores), for tests and
 *          diagnostics.  With paths == NULL the call writes T S pairs and nothing per row.
 *   Tasks with n_s == 0 or info != 0: -1 / -inf in every sample, zeros in paths.
 *   scratch   adkf_thompson_pool_scratch_bytes(T, ns_max, S, m) bytes, 8-byte aligned: v [T, S, ns_max] (and its float64 twin for
 *          flagged tasks up to 1024 points) and the per-chunk candidate pairs.  A function of (T, ns_max, S, m) only, never of
 *          rows.  Nothing for the caller to initialise.
 * Asynchronous on `stream`, no allocation, no synchronisation, capturable.  No atomics: the result is reproducible to the bit, and
 * a task's paths and selection depend on that task's data, its w / eps slices, the basis and the pool only - not on the other
 * tasks of the batch.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: a batch with a query set; an ARD batch; any flag bit other
 * than ADKF_PM_MAXIMIZE; rows < 0; rows > 0 without X; a missing omega, phase, w, eps, sel_idx, sel_val, info or ws; excl_idx
 * without excl_off; S < 1 or S > ADKF_TS_SAMPLES_MAX (ADKF_E_SIZE); m < 64, m > ADKF_TS_FEATURES_MAX or m not a multiple of 64
 * (ADKF_E_SIZE); a workspace or a scratch that is too small (ADKF_E_WORKSPACE); a scratch that is not 8-byte aligned. */
#define ADKF_TS_SAMPLES_MAX 64
#define ADKF_TS_FEATURES_MAX 4096
size_t adkf_thompson_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t S, int32_t m);
int adkf_thompson_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega, const float* phase, int32_t m, const float* w, const float* eps, int32_t S, const int64_t* excl_idx, const int64_t* excl_off, float* paths, int64_t* sel_idx, float* sel_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* The same for ARD batches (one lengthscale per feature dimension); exactly the parameters of adkf_thompson_pool.
 *   The quantity.  With phi[t] = (raw_noise, raw_outputscale, raw_lengthscale[0..d)), l_c = softplus(raw_lengthscale[c]), mu the
 *          support column mean of task t and x~ = (x - mu) / l element-wise, sample q of task t is the isotropic definition on the
 *          scaled features at unit lengthscale (as csrc/ard.h treats every ARD call):
 *              phi_j(x) = sqrt(2 s / m) cos(omega_j . x~ + phase_j),    g(x) = sum_j w[t, q, j] phi_j(x),
 *              r_i = y_i - g(z_i) - sqrt(noise) eps[t, q, i],    v = A^-1 r,    A = s kappa(|z~_i - z~_k|^2) + noise I,
 *              f(x) = g(x) + sum_i s kappa(|x~ - z~_i|^2) v_i.
 *          (omega, phase) is still ONE basis of the kernel at unit lengthscale, shared by all tasks.  With all l_c equal f is
 *          adkf_thompson_pool's f.  The score, the eligibility rule, the total order and the -1 / -inf conventions are unchanged.
 *   b      must carry ADKF_BATCH_ARD and be support-only (nq_max == 0, Z_q == y_q == NULL); anything else is ADKF_E_BADARG;
 *   phi    [T, 2 + d] in the ARD layout;
 *   ws     exactly adkf_workspace_bytes_ard(T, ns_max, 0, d) bytes whatever `rows` is (less: ADKF_E_WORKSPACE); REUSE_INNER after an
 *          ARD adkf_fit on the same batch and workspace reuses the fit's state, as adkf_predict_marginal_ard documents; otherwise
 *          the call evaluates at phi.  REUSE_DIST is ignored, as for every ARD call;
 *   scratch   adkf_thompson_pool_scratch_bytes(T, ns_max, S, m) bytes (it does not depend on d).
 * Every other argument, check, return code and their order, the outputs, and the guarantees (asynchronous, capturable, no atomics,
 * reproducible to the bit, a task's result independent of the other tasks of the batch) are those of adkf_thompson_pool; every
 * check runs before anything is launched. */
int adkf_thompson_pool_ard(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega, const float* phase, int32_t m, const float* w, const float* eps, int32_t S, const int64_t* excl_idx, const int64_t* excl_off, float* paths, int64_t* sel_idx, float* sel_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Kriging-believer batch selection over a shared pool (csrc/believer_stream.h; Ginsbourger, Le Riche and Carraro 2010): q
 * sequential-greedy EI picks per task from the SAME pool X [rows, d] in one call.  Each pick is "believed" at its posterior mean, so
 * the mean of every row stays what it is, the latent variance shrinks by a rank-one downdate per pick, and the incumbent moves to
 * the believed value.  The k rows of largest EI (adkf_predict_pool) are neighbours of the winner; these q rows are a batch.
 *   The quantity.  (noise, s, l) from phi[t], A = K_ss + noise I, m(x) and v_0(x) adkf_predict_pool's mean and latent variance.
 *          After picks p_0 .. p_(j-1) of task t, x_p the pool row of pick p:
 *              w_i      = A^-1 k(Z_s, x_(p_i)),      c0(x, i) = k(x, x_(p_i)) - k(x, Z_s) . w_i      (i < j),
 *              G G^T    = [c0(x_(p_i), l)]_(i,l<j) + noise I,  G lower triangular,    ell(x) = G^-1 c0(x, .),
 *              v_j(x)   = v_0(x) - sum_(i<j) ell_i(x)^2,
 *              best_0   = best_f[t],    best_(j+1) = min(best_j, m(x_(p_j)))   (max with ADKF_PM_MAXIMIZE),
 *              score_j(x) = EI(m(x), v_j(x), best_j)   (log EI with ADKF_PM_LOG_EI), on sqrt(max(v, 1e-12)) as everywhere.
 *          p_j is the eligible row of largest score_j, equal scores going to the lowest row index (the total order of
 *          adkf_predict_pool).  A row is eligible unless it is listed in excl_idx[excl_off[t] .. excl_off[t + 1]) (nullable; as
 *          adkf_predict_pool), it is one of p_0 .. p_(j-1), or its score is NaN.  With no eligible row at step j, that step and all
 *          later ones report -1 / -inf (0 in sel_mean / sel_var) and the state stops changing.  The noise stays in G: a picked row
 *          keeps the latent variance v noise / (v + noise) > 0.  Step 0 is adkf_predict_pool with k = 1, bit for bit.
 *   b      support-only, workspace of adkf_workspace_bytes(T, ns_max, 0, d) bytes whatever rows and q are; REUSE_DIST / REUSE_INNER
 *          mean what they mean for adkf_predict_pool.  ARD batches are refused (ADKF_E_BADARG).
 *   flags  ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI; any other bit is ADKF_E_BADARG.
 *   sel_idx, sel_val   [T, q], required: the pick of each step and its score.
 *   sel_mean, sel_var  [T, q], each nullable: m(x_(p_j)), the believed value, and v_j(x_(p_j)).
 *   trace  nullable, [T, q, rows] with element (t, j, r) at (t q + j) rows + r: score_j of every row, eligible or not, for tests
 *          and diagnostics.  With trace == NULL the call writes T q tuples and nothing per row.
 *   Tasks with n_s == 0 or info != 0: -1 / -inf in every step, zeros in sel_mean, sel_var and trace.
 *   scratch   adkf_believer_pool_scratch_bytes(T, ns_max, d, q) bytes, 8-byte aligned: w [T, q, ns_max] (and its float64 twin for
 *          flagged tasks up to 1024 points), the picks' feature rows [T, q, d], G [T, q, q] (and its twin), the incumbent and the
 *          pick count per task, the per-chunk candidate pairs.  A function of (T, ns_max, d, q) only, never of rows.  Nothing for
 *          the caller to initialise.
 * Asynchronous on `stream`, no allocation, no synchronisation, no atomics: reproducible to the bit, and a task's result depends on
 * that task's data, the pool and its exclusion list only - not on the grid or on the other tasks of the batch.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: a batch with a query set; an ARD batch; any other flag bit;
 * rows < 0; rows > 0 without X; a missing best_f, sel_idx, sel_val, info or ws; excl_idx without excl_off; q < 1;
 * q > ADKF_POOL_TOPK_MAX (ADKF_E_SIZE); a workspace or a scratch that is too small (ADKF_E_WORKSPACE); a scratch that is not 8-byte
 * aligned. */
size_t adkf_believer_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t q);
int adkf_believer_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* adkf_believer_pool for ARD batches (one lengthscale per feature dimension, phi [T, 2 + d]: adkf_workspace_bytes_ard).
 *   The quantity.  (noise, s, l_1 .. l_d) from phi[t], mu the support column mean, x~ = (x - mu) / l elementwise; every kernel value
 *          of adkf_believer_pool's recurrence is taken on the scaled features at unit lengthscale,
 *              k(x, x') = s kappa(|x~ - x'~|^2),
 *          for pool rows, support rows and picks alike; m(x) and v_0(x) are ARD adkf_predict_pool's.  With all l_c equal the picks
 *          are adkf_believer_pool's.  Eligibility, the total order, the incumbent rule and the -1 / -inf conventions are unchanged,
 *          and step 0 is ARD adkf_predict_pool with k = 1, bit for bit.
 *   b      must carry ADKF_BATCH_ARD and be support-only (nq_max == 0, Z_q == y_q == NULL); anything else is ADKF_E_BADARG;
 *   phi    [T, 2 + d] in the ARD layout;
 *   ws     exactly adkf_workspace_bytes_ard(T, ns_max, 0, d) bytes whatever rows and q are (less: ADKF_E_WORKSPACE); REUSE_INNER after
 *          an ARD adkf_fit on the same batch and workspace reuses the fit's state, as adkf_predict_marginal_ard documents; otherwise
 *          the call evaluates at phi.  REUSE_DIST is ignored, as for every ARD call;
 *   scratch   adkf_believer_pool_scratch_bytes(T, ns_max, d, q) bytes: the layout does not depend on the kind of batch (the picks'
 *          rows [T, q, d] hold the SCALED rows here).
 * Every other argument, check, return code and their order, the outputs, and the guarantees (asynchronous, capturable, no atomics,
 * reproducible to the bit, a task's result independent of the other tasks of the batch) are those of adkf_believer_pool; every
 * check runs before anything is launched. */
int adkf_believer_pool_ard(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Max-value entropy search over a shared pool (csrc/mes_stream.h; Wang and Jegelka 2017): every task of the batch scores the SAME
 * rows X [rows, d] by the information each row carries about the VALUE of the task's optimum, and the call can return each task's
 * best k rows itself.  The information-theoretic member of the pool family: no incumbent best_f is involved.
 *   The quantity.  m(x) and v(x) adkf_predict_pool's mean and latent variance, sigma = sqrt(max(v, 1e-12)) as everywhere, and S
 *          samples ystar[t, 0..S) of the optimum value of task t:
 *              gamma_s  = (ystar[t, s] - m) / sigma   with ADKF_PM_MAXIMIZE (ystar: samples of max f),
 *              gamma_s  = (m - ystar[t, s]) / sigma   without                (ystar: samples of min f),
 *              g(gamma) = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma),
 *              score(x) = (1 / S) sum_s g(gamma_s).
 *          g is positive and strictly decreasing.  It is formed without its cancellation at gamma <= -1 (both terms grow like
 *          gamma^2 / 2) and with log1p where Phi -> 1, so a float32 score is good to a few eps32 (1 + gamma^2); the S terms of a row
 *          are added in a fixed order.
 *   ystar  [T, S], an input: given it the call is a deterministic function.  The maxima over the pool of pathwise posterior draws are
 *          such samples - adkf_thompson_pool's sel_val without exclusions is max f with ADKF_PM_MAXIMIZE and -min f without (negate
 *          it).  A NaN or infinite ystar[t, s] makes every score of task t NaN: not skipped, not clamped, never selected.
 *   b      support-only as for adkf_predict_pool, of either kind: with ADKF_BATCH_ARD in b->flags phi is [T, 2 + d] and ws has
 *          adkf_workspace_bytes_ard(T, ns_max, 0, d) bytes, without it [T, 3] and adkf_workspace_bytes(T, ns_max, 0, d).  REUSE_DIST /
 *          REUSE_INNER mean what they mean there.  The workspace size depends on neither rows, S nor k.
 *   flags  ADKF_PM_MAXIMIZE only.
 *   score  nullable, [T, rows] (task t, row r at t * rows + r).  With score == NULL nothing of size T x rows is written.
 *   k, top_idx, top_val   k == 0: no selection.  Otherwise ([T, k] each) the k eligible rows of largest score in descending score,
 *          equal scores in ascending row index (the total order of adkf_predict_pool), and their scores; a row is eligible unless it
 *          is listed in excl_idx[excl_off[t] .. excl_off[t + 1]) (nullable; as adkf_predict_pool) or its score is NaN.  With fewer
 *          than k eligible rows, and with rows == 0, the tail is top_idx = -1, top_val = -inf.
 *   Tasks with n_s == 0 or info != 0: their [rows] slice of score is 0 (the fill value), their selection -1 / -inf.
 *   scratch   adkf_predict_pool_scratch_bytes(T, k) bytes, 8-byte aligned: the candidate lists of adkf_predict_pool (0 for k == 0).
 * Asynchronous on `stream`, no allocation, no synchronisation, no atomics: reproducible to the bit, and a task's scores and selection
 * depend on that task's data, its ystar row, the pool and its exclusion list only - not on the grid or the other tasks of the batch.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: a batch with a query set; any flag bit other than
 * ADKF_PM_MAXIMIZE; ystar == NULL; rows < 0; rows > 0 without X; excl_idx without excl_off; k < 0; k > 0 without top_idx or top_val;
 * k == 0 without score; S < 1 or S > ADKF_TS_SAMPLES_MAX (ADKF_E_SIZE); k > ADKF_POOL_TOPK_MAX (ADKF_E_SIZE); a scratch or a
 * workspace that is too small (ADKF_E_WORKSPACE); a scratch that is not 8-byte aligned. */
int adkf_mes_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* ystar, int32_t S, const int64_t* excl_idx, const int64_t* excl_off, float* score, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Gumbel max-value sampling over a shared pool (csrc/gumbel_stream.h; Wang and Jegelka 2017, section 3.1; BoTorch's
 * _sample_max_value_Gumbel): S samples of the VALUE of each task's optimum over the rows X [rows, d], as adkf_mes_pool takes them in
 * ystar, from the pool's posterior marginals alone - no random-Fourier basis, no per-sample solve, S uniforms per task.
 *   The quantity.  m_i and v_i adkf_predict_pool's mean and latent variance of row i, sigma_i = sqrt(max(v_i, 1e-12)), and in the
 *          score's sense h = +f with ADKF_PM_MAXIMIZE and h = -f without (mu_i = +-m_i).  The marginals are taken as independent:
 *              Pr[max_i h_i < z] = prod_i Phi((z - mu_i) / sigma_i).
 *          Its quartiles are bracketed by lo = max_i (mu_i - sigma_i) and hi = max_i (mu_i + kappa sigma_i), kappa = max(1,
 *          Phi^-1(1 - 0.25 / rows)), and located by two passes of ADKF_GUMBEL_PROBES = 64 equidistant probes of log Pr with linear
 *          interpolation in the bracketing cell (within about 2e-4 b of the exact quartiles).  A Gumbel is fitted to them,
 *              b = (q75 - q25) / (log log 4 - log log(4 / 3)),   a = q50 + b log log 2,
 *          and ystar_h[t, s] = a - b log(-log u[t, s]), u clamped to [2^-24, 1 - 2^-24].  Three walks of the pool per call.
 *   u      [T, S] uniforms in (0, 1), an input: given them the call is a deterministic function.
 *   ystar  [T, S]: samples of max f with ADKF_PM_MAXIMIZE (ystar_h), of min f without (-ystar_h).
 *   quant  nullable, [T, 3]: the quartiles q25, q50, q75 in the score's sense.   gumbel  nullable, [T, 2]: (a, b), the same sense.
 *   b, ws  support-only, of either kind (ADKF_BATCH_ARD or not), as for adkf_mes_pool.   flags  ADKF_PM_MAXIMIZE only.
 *   Tasks with n_s == 0 or info != 0, and every task when rows == 0: quant = gumbel = -inf, ystar = -inf with ADKF_PM_MAXIMIZE and
 *          +inf without (adkf_mes_pool turns such samples into NaN scores, which are never selected).
 *   scratch   adkf_gumbel_pool_scratch_bytes(T) bytes, 8-byte aligned; the size depends on neither rows, S nor the device.
 * The terms -log Phi are summed as unsigned 64-bit fixed-point numbers (2^-31 per unit, each term clamped at 32) with integer adds and
 * integer atomics only, the two maxima through an order-preserving integer image: no floating-point atomics, and a task's quant,
 * gumbel and ystar are the same bits alone or in a batch, on any grid, and under any permutation of the pool's rows.  The sums
 * cannot wrap for rows <= 2^27; the rounding of a sum is at most rows 2^-32.  Asynchronous on `stream`, no allocation, no
 * synchronisation, capturable.  Rejected before anything is launched, ADKF_E_BADARG unless noted: a batch with a query set; any flag
 * bit other than ADKF_PM_MAXIMIZE; u, ystar, info or ws == NULL; rows < 0; rows > 0 without X; S < 1 or S > ADKF_TS_SAMPLES_MAX
 * (ADKF_E_SIZE); rows > 2^27 (ADKF_E_SIZE); a scratch or a workspace that is too small (ADKF_E_WORKSPACE); a scratch that is not
 * 8-byte aligned. */
#define ADKF_GUMBEL_PROBES 64
size_t adkf_gumbel_pool_scratch_bytes(int32_t T);
int adkf_gumbel_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* u, int32_t S, float* ystar, float* quant, float* gumbel, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* GIBBON batch max-value entropy search over a shared pool (csrc/gibbon_stream.h; Moss, Leslie, Gonzalez and Rayson 2021; BoTorch's
 * qLowerBoundMaxValueEntropy): q sequential-greedy picks per task from the SAME pool X [rows, d] in one call, of the lower bound on
 * the information a BATCH of noisy observations carries about the VALUE of the task's optimum.  The batch form of adkf_mes_pool: its k
 * best rows are neighbours of the winner and carry almost the same information; these q rows are a batch.
 *   The quantity.  m(x) and v_0(x) adkf_predict_pool's mean and latent variance, noise the task's, sigma = sqrt(max(v_0, 1e-12)) as
 *          everywhere, S samples ystar[t, 0..S) of the optimum value of task t and gamma_s as adkf_mes_pool forms it
 *          ((ystar[t, s] - m) / sigma with ADKF_PM_MAXIMIZE, (m - ystar[t, s]) / sigma without):
 *              tau(g)   = phi(g) / Phi(g),      h(g) = tau(g) (g + tau(g))                 0 < h < 1,
 *              rho2(x)  = max(v_0, 1e-12) / (max(v_0, 1e-12) + noise),
 *              a(x)     = -(1 / 2S) sum_s log1p(-rho2 h(gamma_s))                          the single-point GIBBON score, >= 0.
 *          The batch criterion is alpha(B) = 1/2 log |R_B| + sum_(i in B) a(x_i), R_B the predictive correlation matrix of the noisy
 *          observations at B, and the greedy increment of adding x to the picks p_0 .. p_(j-1) is exactly
 *              score_j(x) = a(x) + 1/2 log((max(v_j(x), 1e-12) + noise) / (max(v_0(x), 1e-12) + noise)),
 *          v_j(x) = v_0(x) - sum_(i<j) ell_i(x)^2 the downdated latent variance of adkf_believer_pool (w_i, c0, G and ell as there;
 *          G G^T carries the noise on its diagonal).  The mean never moves, ystar never changes between steps and there is no
 *          incumbent.  score_0 = a; later scores may be negative and are valid scores; score_j(x) <= score_0(x) for every row.
 *          h is formed without the cancellation of g + tau at gamma <= -1 (h = tau^2 b(a), a = -gamma, b the bracket of log EI, its
 *          series beyond gamma = -12) and with the complement of the tail where Phi -> 1; 1 - rho2 h >= noise / (v_0 + noise) > 0,
 *          always through log1p.  The S terms of a row are added in a fixed order.
 *          p_j is the eligible row of largest score_j, equal scores going to the lowest row index (the total order of
 *          adkf_predict_pool).  A row is eligible unless it is listed in excl_idx[excl_off[t] .. excl_off[t + 1]) (nullable), it is one
 *          of p_0 .. p_(j-1), or its score is NaN.  With no eligible row at step j, that step and all later ones report -1 / -inf (0
 *          in sel_mean / sel_var) and the state stops changing.  A pick counts when its index is not -1 and its value is finite.
 *   ystar  [T, S], an input, as for adkf_mes_pool.  A NaN or infinite ystar[t, s] makes every score of task t NaN: no pick.
 *   b      support-only, of either kind: with ADKF_BATCH_ARD in b->flags phi is [T, 2 + d], ws has adkf_workspace_bytes_ard(T, ns_max,
 *          0, d) bytes and every kernel value is taken on the scaled features (the picks' rows are stored scaled, as
 *          adkf_believer_pool_ard stores them); without it [T, 3] and adkf_workspace_bytes(T, ns_max, 0, d).
 *   flags  ADKF_PM_MAXIMIZE only.
 *   q, S   1 <= q <= ADKF_POOL_TOPK_MAX, 1 <= S <= ADKF_TS_SAMPLES_MAX.
 *   sel_idx, sel_val   [T, q], required: the pick of each step and its score.
 *   sel_mean, sel_var  [T, q], each nullable: m(x_(p_j)) and v_j(x_(p_j)).
 *   trace  nullable, [T, q, rows] with element (t, j, r) at (t q + j) rows + r: score_j of every row, eligible or not.  With
 *          trace == NULL the call writes T q tuples and nothing per row.
 *   Tasks with n_s == 0 or info != 0: -1 / -inf in every step, zeros in sel_mean, sel_var and trace.
 *   scratch   adkf_believer_pool_scratch_bytes(T, ns_max, d, q) bytes, 8-byte aligned: the believer's state with the believer's layout.
 * Asynchronous on `stream`, no allocation, no synchronisation, no atomics: reproducible to the bit, and a task's result depends on
 * that task's data, its ystar row, the pool and its exclusion list only - not on the grid or on the other tasks of the batch.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: a batch with a query set; any flag bit other than
 * ADKF_PM_MAXIMIZE; rows < 0; rows > 0 without X; a missing ystar, sel_idx, sel_val, info or ws; excl_idx without excl_off; q < 1;
 * S < 1; q > ADKF_POOL_TOPK_MAX or S > ADKF_TS_SAMPLES_MAX (ADKF_E_SIZE); a workspace or a scratch that is too small
 * (ADKF_E_WORKSPACE); a scratch that is not 8-byte aligned. */
int adkf_gibbon_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* ystar, int32_t S, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Constant-liar and label-replay batches over a shared pool (csrc/liar_stream.h; the constant liar of Ginsbourger, Le Riche and
 * Carraro 2010, the sibling of the Kriging believer; conditioning on real labels without a refit is BoTorch's
 * condition_on_observations): adkf_believer_pool with the believed value SUPPLIED.  Per task q sequential-greedy picks by EI (log EI
 * with ADKF_PM_LOG_EI) from the SAME pool X [rows, d]; after pick p_j is chosen it is conditioned on y_j as a NOISY observation
 * under the task's own noise, so the posterior mean moves inside the call.  y_j is the first finite value of
 *              labels[t * label_stride + p_j]    if labels is given,
 *              lie[t]                            if lie is given,
 *              m_j(x_(p_j))                      the pick's own posterior mean, which is the believer's rule.
 *          With A, w_i, c0, G and ell exactly as for adkf_believer_pool:
 *              z_j      = (y_j - m_j(x_(p_j))) / G[j, j]          G[j, j] = sqrt(v_j(x_(p_j)) + noise)
 *              m_j(x)   = m_0(x) + sum_(i<j) ell_i(x) z_i         v_j(x) = v_0(x) - sum_(i<j) ell_i(x)^2
 *              score_j  = EI or log EI (m_j(x), v_j(x), best_j)   best_(j+1) = min(best_j, y_j)   (max with ADKF_PM_MAXIMIZE)
 *          which is the posterior of the support set with the picks appended as labelled points at the same phi.  A constant lie
 *          (CL-min, CL-max, CL-mean of the observed labels) is the dial on batch diversity the believer lacks; a label table plays
 *          q iterations of a replay at fixed phi in one call.  Step 0 is adkf_predict_pool(k = 1) bit for bit; with every y_j from the
 *          third rule (a lie of NaN) every output is adkf_believer_pool's bit for bit.
 *          Eligibility, the total order and "no eligible row at step j: -1 / -inf from there on, the state stops changing" are
 *          adkf_believer_pool's; such a step has 0 in sel_lie and repeats the incumbent in inc.
 *   b      support-only, of either kind (as adkf_gibbon_pool): with ADKF_BATCH_ARD phi is [T, 2 + d] and ws an ARD workspace.
 *   flags  ADKF_PM_MAXIMIZE, ADKF_PM_LOG_EI.
 *   best_f [T], required: best_0.
 *   lie    nullable [T].  labels  nullable; label_stride 0: one table [rows] shared by all tasks (replicates over one pool);
 *          label_stride == rows: [T, rows].  At least one of lie and labels.
 *   q      1 <= q <= ADKF_POOL_TOPK_MAX.
 *   sel_idx, sel_val   [T, q], required: the pick of each step and its score.
 *   sel_mean, sel_var  [T, q], each nullable: m_j and the latent v_j at the pick, before it is conditioned on.
 *   sel_lie   [T, q], nullable: the y_j actually used.    inc  [T, q + 1], nullable: best_0 .. best_q.
 *   trace  nullable, [T, q, rows] as for adkf_believer_pool.  With trace == NULL nothing of size T x rows is written or kept.
 *   Tasks with n_s == 0 or info != 0: -1 / -inf in every step, zeros in sel_mean, sel_var, sel_lie and trace, best_f[t] in inc.
 *   scratch   adkf_liar_pool_scratch_bytes(T, ns_max, d, q) bytes, 8-byte aligned, independent of rows: the believer's state with the
 *          believer's layout, then z [T, q] and its float64 twin.
 * Asynchronous on `stream`, no allocation, no synchronisation, no atomics: reproducible to the bit, and a task's result depends on
 * that task's data, its lie, its labels, the pool and its exclusion list only.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: a batch with a query set; any flag bit other than the two
 * above; rows < 0; rows > 0 without X; a missing best_f, sel_idx, sel_val, info or ws; lie and labels both NULL (that call is
 * adkf_believer_pool); a label_stride other than 0 and rows; a non-zero label_stride without labels; excl_idx without excl_off;
 * q < 1; q > ADKF_POOL_TOPK_MAX (ADKF_E_SIZE); a workspace or a scratch that is too small (ADKF_E_WORKSPACE); a scratch that is not
 * 8-byte aligned. */
size_t adkf_liar_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t q);
int adkf_liar_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f, const float* lie, const float* labels, int64_t label_stride, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, float* sel_lie, float* inc, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Level-set estimation and batch UCB over a shared pool (csrc/levelset_stream.h; the straddle of Bryan et al. 2005, the classification
 * of Gotovos et al. 2013, GP-BUCB of Desautels, Krause and Burdick 2014): per task, against a threshold tau[t] with a confidence band
 * of width beta[t], which rows of the SAME pool X [rows, d] are on the active side of tau, how many actives the pool is expected to
 * hold, and q sequential-greedy picks of what to measure next.  It also supplies the two acquisitions that take a parameter instead
 * of an incumbent: probability of improvement over a threshold, and the upper / lower confidence bound.
 *   The quantity.  m(x) and v_0(x) adkf_predict_pool's mean and latent variance; v_j(x) = v_0(x) - sum_(i<j) ell_i(x)^2 the downdated
 *          latent variance of adkf_believer_pool after the picks p_0 .. p_(j-1) (w_i, c0, G and ell as there); sigma_j =
 *          sqrt(max(v_j, 1e-12)) as everywhere; s = +1 with ADKF_PM_MAXIMIZE (active means f > tau) and -1 without (active means
 *          f < tau, the minimisation default of every other entry); z_j(x) = s (m - tau) / sigma_j.
 *              straddle_j(x) = beta sigma_j - |m - tau|         > 0 exactly when the band m +- beta sigma_j holds tau
 *              ADKF_LS_STRADDLE   score_j = straddle_j
 *              ADKF_LS_PROB       score_j = log Phi(z_j)        unclamped: the ranking survives where float32 Phi is 0, as log EI does
 *              ADKF_LS_BOUND      score_j = s m + beta sigma_j  UCB with ADKF_PM_MAXIMIZE, -(LCB) without
 *          The class of a row at step j, in this order: undecided if straddle_j > 0; otherwise active if s (m - tau) > 0; otherwise
 *          inactive.  Whatever the score, the class is decided from the same float32 straddle_j that an ADKF_LS_STRADDLE call
 *          stores in trace, formed as fmaf(beta, sigma_j, -|m - tau|) (tasks on the float64 path: from the float32-rounded mean and
 *          variance by the same function).  hits_j = sum over the pool rows of Phi(z_j) is the expected number of actives.
 *          A row whose mean or variance is NaN belongs to no class, adds nothing to hits and has score NaN.
 *          The picks are hallucinated: a GP's variance does not depend on the labels, so the mean never moves and every pick only
 *          downdates the variance.  Counts and hits at steps j > 0 are hallucinated in the same sense: "if the earlier picks land on
 *          their means".  ADKF_LS_PROB does NOT diversify: for a row beyond tau the probability rises as its variance falls, so its
 *          batch is the rows most certainly active given the earlier picks, not a spread over the pool.
 *          p_j is the eligible row of largest score_j, equal scores going to the lowest row index (the total order of
 *          adkf_predict_pool).  A row is eligible unless it is listed in excl_idx[excl_off[t] .. excl_off[t + 1]) (nullable), it is one
 *          of p_0 .. p_(j-1), or its score is NaN.  With no eligible row at step j, that step and all later ones report -1 / -inf (0
 *          in sel_mean / sel_var) and the state stops changing.  A pick counts when its index is not -1 and its value is finite.
 *   b      support-only, of either kind (as adkf_gibbon_pool): with ADKF_BATCH_ARD in b->flags phi is [T, 2 + d] and ws has
 *          adkf_workspace_bytes_ard(T, ns_max, 0, d) bytes; without it [T, 3] and adkf_workspace_bytes(T, ns_max, 0, d).  REUSE_DIST /
 *          REUSE_INNER mean what they mean for adkf_predict_pool.
 *   flags  ADKF_PM_MAXIMIZE only.  The variance is always the latent one: ADKF_PM_LATENT is refused like any other bit.
 *   tau, beta   [T], required.  A tau[t] that is not finite, or a beta[t] that is NaN, infinite or negative, cannot be refused by the
 *          host (the values live on the device): every score of task t is NaN, nothing is picked, its counts and hits are 0 and
 *          its cls is -1.
 *   score  ADKF_LS_STRADDLE, ADKF_LS_PROB or ADKF_LS_BOUND.
 *   q      1 <= q <= ADKF_POOL_TOPK_MAX.  A caller who wants the counts AFTER a batch of q asks for q + 1 steps and drops the last pick.
 *   trace  nullable, [T, q, rows] with element (t, j, r) at (t q + j) rows + r: score_j of every row, eligible or not.
 *   cls    nullable, [T, rows] int8: the class at step 0.  0 = active, 1 = inactive, 2 = undecided, -1 = not evaluated (a NaN row, and
 *          the whole slice of a skipped task).
 *   counts nullable, [T, q, 3] int64: at step j the number of active, inactive and undecided pool rows given the picks before it.  It
 *          covers ALL rows: excluded and picked rows are counted too.
 *   hits   nullable, [T, q]: hits_j, the 2^-31 fixed-point sum (adkf_gumbel_pool's format) of the float32 Phi terms, integer adds
 *          only, converted once at the end (u64 to double to float).  The rounding of the sum is at most rows 2^-32.
 *   sel_idx, sel_val   [T, q], required: the pick of each step and its score.
 *   sel_mean, sel_var  [T, q], each nullable: m(x_(p_j)), which never moves, and v_j(x_(p_j)).
 *   Tasks with n_s == 0 or info != 0: -1 / -inf in every step, zeros in sel_mean, sel_var, trace, counts and hits, cls = -1.
 *   scratch   adkf_levelset_pool_scratch_bytes(T, ns_max, d, q) bytes, 8-byte aligned, a function of (T, ns_max, d, q) only: the
 *          believer's state with the believer's layout, then four 64-bit accumulators per task.
 * Nothing of size T x rows exists unless trace or cls is given.  Asynchronous on `stream`, no allocation, no synchronisation,
 * capturable.  The class counts and the Phi sum are accumulated with integer adds and integer atomics only - no floating-point
 * atomics - so the call is reproducible to the bit, and a task's counts and hits are the same bits alone or in a batch, on any grid,
 * and under any permutation of the pool's rows.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: a batch with a query set; any flag bit other than
 * ADKF_PM_MAXIMIZE; score outside 0 .. 2; rows < 0; rows > 0 without X; a missing tau, beta, sel_idx, sel_val, info or ws; excl_idx
 * without excl_off; q < 1; q > ADKF_POOL_TOPK_MAX (ADKF_E_SIZE); rows > 2^31 with counts or hits (ADKF_E_SIZE: below that the
 * fixed-point sum cannot wrap); a workspace or a scratch that is too small (ADKF_E_WORKSPACE); a scratch that is not 8-byte aligned. */
#define ADKF_LS_STRADDLE 0
#define ADKF_LS_PROB 1
#define ADKF_LS_BOUND 2
size_t adkf_levelset_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t q);
int adkf_levelset_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* tau, const float* beta, int32_t score, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int8_t* cls, int64_t* counts, float* hits, int64_t* sel_idx, float* sel_val, float* sel_mean, float* sel_var, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Knowledge-gradient selection over a shared pool (csrc/kg_stream.h; Frazier, Powell and Dayanik 2009; Scott, Frazier and Powell
 * 2011, "KGCP"; the single-step form of BoTorch's qKnowledgeGradient on a discrete set): every row of the SAME pool X [rows, d] is
 * scored, per task, by how much one noisy observation there is expected to raise the best posterior mean over the row itself and a
 * reference set of at most ADKF_KG_REFS_MAX other pool rows.  It prices the observation noise, and needs neither an incumbent nor
 * max-value samples.
 *   The quantity.  m(.), cov(., .) the latent posterior of adkf_predict_pool, noise the task's, R_t = ref_idx[t, 0 .. M) the reference
 *          rows.  For a pool row x: vc = max(v(x), 1e-12) (the clamp of EI), s = sqrt(vc + noise), sgn = +1 with ADKF_PM_MAXIMIZE and
 *          -1 without (the slopes keep their sign, Z being symmetric), and
 *              reference line j   a_j = sgn m(r_j),   b_j = cov(x, r_j) / s,
 *              own line           a_x = sgn m(x),     b_x = vc / s,
 *              KG(x) = E_Z[max_l (a_l + b_l Z)] - max_l a_l >= 0,   Z standard normal.
 *          Reference entries outside [0, rows) are skipped, so a top_idx of adkf_predict_pool with its -1 tail can be passed as it
 *          is; a repeated index counts once, its first occurrence being the one kept.  x always contributes its own line from its own
 *          mean and variance, and a reference entry equal to x's own index is skipped for that row - exactly, by index, so no pair
 *          of nearly coincident lines is ever created.
 *          KG is evaluated in Frazier's form, a sum of non-negative terms over the lines of the upper envelope in ascending slope,
 *              sum (b_next - b_cur) h(-|c|),   c = (a_cur - a_next) / (b_next - b_cur),   h(u) = phi(u) + u Phi(u);
 *          E[max] is never formed and max a never subtracted.  With ADKF_PM_LOG_EI the score is log KG, the log-sum-exp of
 *          log(b_next - b_cur) + log h(-|c|) with log h as log EI forms it: finite where KG underflows.  One surviving line gives
 *          KG = 0 and log KG = -inf (a row that is the only valid reference entry of its task, for instance).  The set of lines
 *          judged active may differ from the exact one only by lines whose interval is empty up to rounding; each crossing is
 *          recomputed from the pair of consecutive active lines, so such a line changes the sum by rounding only.
 *   b      support-only, of either kind, as for adkf_mes_pool; REUSE_DIST / REUSE_INNER and info as for adkf_predict_pool.
 *   flags  ADKF_PM_MAXIMIZE | ADKF_PM_LOG_EI.
 *   ref_idx   [T, M] pool row indices, 1 <= M <= ADKF_KG_REFS_MAX.
 *   score  nullable, [T, rows]: KG or log KG.
 *   cov    nullable, [T, rows, M] (task t, row r, entry j at (t * rows + r) * M + j): the latent posterior covariance of each row with
 *          each reference entry, 0 for skipped entries (the own-index entry of a row is NOT skipped here: it holds v(x)).
 *   ref_mean  nullable, [T, M]: the posterior mean of each reference entry in its natural sign, 0 for skipped entries.
 *   k, top_idx, top_val, excl_idx, excl_off   the selection of adkf_predict_pool on the score: its unique order, its exclusion lists,
 *          its -1 / -inf tail; a NaN score is never selected.
 *   Tasks with n_s == 0 or info != 0: zero slices of score, cov and ref_mean, and a -1 / -inf selection.
 *   Non-finite data.  A pool row whose own mean or variance is NaN scores NaN and is never selected.  A line whose covariance with the
 *          row is NaN is left out of that row's envelope as a skipped entry is, and a NaN intercept does not move the interval of
 *          another line: a reference row with NaN or infinite features (its w, mean and covariances are then NaN, and cov / ref_mean
 *          report them) lowers no score to NaN - the other rows are scored without it.  Keep such rows out of ref_idx.
 *   scratch   adkf_kg_pool_scratch_bytes(T, ns_max, d, M, k) bytes, 8-byte aligned: the reference state (w = A^-1 k(Z_s, r_j) [T, M,
 *          ns_max], its float64 copy where the workspace has a float64 region, the stored rows [T, M, d], the means and the entries'
 *          indices) and the candidate lists of adkf_predict_pool.  It depends on neither rows nor the device.
 * Asynchronous on `stream`, no allocation, no synchronisation, no atomics: reproducible to the bit, and a task's score, cov, ref_mean
 * and selection depend on that task's data, its reference rows, the pool and its exclusion list only - not on the grid or on the other
 * tasks of the batch.  Rejected before anything is launched, ADKF_E_BADARG unless noted: M < 1, M > ADKF_KG_REFS_MAX or
 * k > ADKF_POOL_TOPK_MAX (ADKF_E_SIZE); ref_idx == NULL; a batch with a query set; rows < 0; rows > 0 without X; any flag bit other
 * than the two; k < 0; k > 0 without top_idx or top_val; excl_idx without excl_off; no output at all (k == 0 and score, cov and
 * ref_mean all NULL); a scratch or a workspace that is too small (ADKF_E_WORKSPACE); a scratch that is not 8-byte aligned. */
#define ADKF_KG_REFS_MAX 64
size_t adkf_kg_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t M, int32_t k);
int adkf_kg_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* ref_idx, int32_t M, const int64_t* excl_idx, const int64_t* excl_off, float* score, float* cov, float* ref_mean, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Joint entropy search over a shared pool (csrc/jes_stream.h; Hvarfner, Hutter and Nardi 2022; BoTorch's
 * qLowerBoundJointEntropySearch at q = 1): every row of the SAME pool X [rows, d] is scored, per task, by the information one noisy
 * observation there carries about the task's optimum - its LOCATION and VALUE together - given S samples of that pair.
 * adkf_thompson_pool's sel_idx / sel_val are such samples and can be passed as they are (sel_val in its natural sign).
 *   The quantity.  m(.), v(.), cov(., .) the latent posterior of adkf_predict_pool, noise the task's, (x*_s, f*_s) = (pool row
 *          opt_idx[t, s], opt_val[t, s]) the samples; f*_s is a maximum with ADKF_PM_MAXIMIZE and a minimum without.  Per valid s:
 *              d_s      = max(v(x*_s), 1e-12) + cond_noise,
 *              c_s(x)   = cov(x, x*_s),
 *              v_s(x)   = max(v(x) - c_s(x)^2 / d_s, 1e-12)           the latent variance given f(x*_s) = f*_s,
 *              m_s(x)   = m(x) + c_s(x) (f*_s - m(x*_s)) / d_s,
 *              gamma_s  = (f*_s - m_s) / sqrt(v_s) with ADKF_PM_MAXIMIZE, (m_s - f*_s) / sqrt(v_s) without,
 *              rho2_s   = v_s / (v_s + noise),
 *              term_s   = log((vc + noise) / (v_s + noise)) - log1p(-rho2_s h(gamma_s)),   vc = max(v(x), 1e-12),
 *              score(x) = (1 / (2 S_eff)) sum over the valid s of term_s,
 *          h(g) = tau (g + tau), tau = phi / Phi, formed as adkf_gibbon_pool forms it.  The score is the entropy of the noisy
 *          observation at x minus the mean over the samples of its moment-matched entropy given the sample; both parts of every
 *          term are >= 0, so score >= 0.  The S terms of a row are added in a fixed order.
 *          An entry of opt_idx outside [0, rows) is a skipped sample (adkf_thompson_pool's -1 included) and S_eff counts the valid
 *          ones.  A repeated row is NOT merged: two draws may share a location and differ in value, so each counts (unlike
 *          adkf_kg_pool's first-occurrence rule).  S_eff == 0 makes every score of the task NaN, and nothing is selected.  A NaN or
 *          infinite opt_val[t, s] on a valid entry makes every score of task t NaN (adkf_mes_pool's rule).  A pool row whose own mean
 *          or variance is NaN scores NaN and is never selected.  Nothing is special, by index, at x = x*_s: the subtraction in v_s
 *          cancels there, the clamp catches it, and the term stays well conditioned because rho2_s -> 0 damps whatever gamma_s
 *          rounds to.
 *          With every sample valid and cond_noise so large that c_s^2 / d_s and c_s (f*_s - m(x*_s)) / d_s round away, the score is
 *          adkf_gibbon_pool's step-0 score a(x) for ystar = opt_val, bit for bit.
 *   b      support-only, of either kind, as for adkf_mes_pool; REUSE_DIST / REUSE_INNER and info as for adkf_predict_pool.
 *   flags  ADKF_PM_MAXIMIZE only.
 *   opt_idx, opt_val   [T, S], required, 1 <= S <= ADKF_TS_SAMPLES_MAX.
 *   cond_noise   the noise variance under which the optimum is conditioned on; finite and >= 0.
 *   score  nullable, [T, rows].
 *   opt_mean, opt_var  [T, S], each nullable: m(x*_s) and the unclamped latent v(x*_s), 0 for skipped samples.
 *   k, top_idx, top_val, excl_idx, excl_off   the selection of adkf_predict_pool on the score: its unique order, its exclusion lists,
 *          its -1 / -inf tail; a NaN score is never selected.
 *   Tasks with n_s == 0 or info != 0: zero slices of score, opt_mean and opt_var, and a -1 / -inf selection.
 *   scratch   adkf_jes_pool_scratch_bytes(T, ns_max, d, S, k) bytes, 8-byte aligned: adkf_kg_pool's reference state for M = S, the
 *          entries' v(x*_s), 1 / d_s and (f*_s - m(x*_s)) / d_s [T, S] each, one scale per task and the candidate lists of
 *          adkf_predict_pool.  It depends on neither rows nor the device.
 * Asynchronous on `stream`, no allocation, no synchronisation, no atomics: reproducible to the bit, and a task's result depends on
 * that task's data, its samples, the pool and its exclusion list only - not on the grid or on the other tasks of the batch.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: S < 1, S > ADKF_TS_SAMPLES_MAX or k > ADKF_POOL_TOPK_MAX
 * (ADKF_E_SIZE); opt_idx == NULL or opt_val == NULL; a negative, NaN or infinite cond_noise; a batch with a query set; rows < 0;
 * rows > 0 without X; any flag bit other than ADKF_PM_MAXIMIZE; k < 0; k > 0 without top_idx or top_val; excl_idx without excl_off;
 * no output at all (k == 0 and score, opt_mean and opt_var all NULL); a scratch or a workspace that is too small
 * (ADKF_E_WORKSPACE); a scratch that is not 8-byte aligned. */
size_t adkf_jes_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t S, int32_t k);
int adkf_jes_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* opt_idx, const float* opt_val, int32_t S, float cond_noise, const int64_t* excl_idx, const int64_t* excl_off, float* score, float* opt_mean, float* opt_var, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Target-variance batch selection over a shared pool (csrc/ipv_stream.h; Cohn 1996, "ALC"; Gramacy and Apley 2015; BoTorch's
 * qNegIntegratedPosteriorVariance with the targets as its mc_points; Huebotter et al. 2024, "VTL"): transductive active learning.
 * Per task, q rows of the SAME pool X [rows, d] are chosen, one after the other, so that noisy observations there lower the weighted
 * posterior variance at the task's TARGET rows as far as possible.  The posterior variance of a GP does not depend on the labels,
 * so the whole batch is chosen before anything is measured, and y_s enters only through the fit that gave phi.
 *   The quantity.  v_0, cov_0(., .) the latent posterior of adkf_predict_pool, noise the task's, r_m = pool row tgt_idx[t, m] the
 *          targets with weights wt_m = tgt_w[t, m] (tgt_w == NULL: 1), p_0 .. p_(j-1) the picks so far, w_e = A^-1 k(Z_s, x_e):
 *              c0(x, e)     = k(x, x_e) - k(x, Z_s) . w_e                  e a target or a pick
 *              G G^T        = [c0(x_(p_i), p_l)]_(i,l<j) + noise I         adkf_believer_pool's G
 *              ell(x)       = G^-1 c0(x, picks)
 *              v_j(x)       = v_0(x) - sum_(i<j) ell_i(x)^2
 *              cov_j(x,r_m) = c0(x, r_m) - sum_(i<j) ell_i(x) ell_i(r_m)
 *              score_j(x)   = sum_m wt_m cov_j(x, r_m)^2 / (max(v_j(x), 1e-12) + noise)      >= 0
 *              tvar_j       = sum_m wt_m v_j(r_m)
 *          score_j(x) is exactly what one noisy observation at x takes off tvar_j: tvar_j - tvar_(j+1) = score_j(p_j).  p_j is the
 *          eligible row of largest score_j under adkf_predict_pool's total order (score, then ascending row); a row is eligible
 *          unless it is in the task's exclusion list, is an earlier pick, or scores NaN.
 *          A target entry is skipped if it lies outside [0, rows), if an earlier entry of the task's list has the same index (by
 *          index alone, as adkf_kg_pool: the first occurrence is the one looked at), or if its weight is <= 0 or NaN.
 *          THE TARGETS ARE ELIGIBLE unless the caller excludes them: observing a target is the best single pick.  A caller who cannot
 *          measure the targets lists them in excl_idx.
 *   b      support-only, of either kind, as for adkf_kg_pool; REUSE_DIST / REUSE_INNER and info as for adkf_predict_pool.
 *   flags  0.
 *   tgt_idx   [T, M] pool row indices; tgt_w nullable, [T, M].  M >= 1, q >= 1 and M + q <= ADKF_IPV_ENTRIES_MAX: targets and picks
 *          share one 64-column covariance panel per row tile.  A form with two panels is not built.
 *   trace  nullable, [T, q, rows]: score_j of every row at every step (as adkf_believer_pool's).
 *   sel_idx, sel_val   [T, q], required: the picks in pick order and their scores at the step they were picked.  With no eligible
 *          row at step j, that step and all later ones report -1 / -inf and the state stops changing.
 *   tvar   nullable, [T, q + 1]: tvar_0 .. tvar_q (a step without a pick repeats the value before it).
 *   Tasks with n_s == 0, info != 0 or no valid target entry: -1 / -inf at every step, zero slices of tvar and trace.
 *   Non-finite data.  A target row with NaN or infinite features makes its own w and covariances NaN, and with them every score of
 *          the task: nothing is selected.  Keep such rows out of tgt_idx.  A pool row whose own mean or variance is NaN scores NaN
 *          and is never selected.
 *   scratch   adkf_ipv_pool_scratch_bytes(T, ns_max, d, M, q) bytes, 8-byte aligned: w and the stored row of every entry [T, M + q,
 *          ns_max] and [T, M + q, d] (w with a float64 copy where the workspace has a float64 region), G [T, q, q] and ell(r_m) [T, q,
 *          M] with their copies, per-target and per-task scalars, and one candidate pair per (task, chunk).  A function of (T, ns_max,
 *          d, M, q) only.
 * Asynchronous on `stream` and capturable, no allocation, no synchronisation, no atomics, every sum in a fixed order: reproducible to
 * the bit, and a task's result depends on that task's data, its targets, the pool and its exclusion list only - not on the grid or on
 * the other tasks of the batch.  Rejected before anything is launched, ADKF_E_BADARG unless noted: M < 1; q < 1;
 * M + q > ADKF_IPV_ENTRIES_MAX (ADKF_E_SIZE); tgt_idx, sel_idx, sel_val, info or ws NULL; a batch with a query set; any flag bit;
 * rows < 0; rows > 0 without X; excl_idx without excl_off; a scratch or a workspace that is too small (ADKF_E_WORKSPACE); a scratch
 * that is not 8-byte aligned. */
#define ADKF_IPV_ENTRIES_MAX 64      /* M + q */
size_t adkf_ipv_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t d, int32_t M, int32_t q);
int adkf_ipv_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const int64_t* tgt_idx, const float* tgt_w, int32_t M, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, int64_t* sel_idx, float* sel_val, float* tvar, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Leave-one-out checks and jackknife+ prediction intervals over a shared pool (csrc/jackknife_stream.h; Rasmussen and Williams 2006,
 * section 5.4.2, GPyTorch's LeaveOneOutPseudoLikelihood and BoTorch's batch_cross_validation for the leave-one-out forms; Barber,
 * Candes, Ramdas and Tibshirani 2021, "Predictive inference with the jackknife+", for the intervals).  How far the predictions of a
 * task with a handful of labels can be trusted, without holding any label out and without resting on the GP variance.
 *   Fixed phi.  Everything below is at the phi passed: the hyperparameters are NOT refitted per fold.  The coverage theorem holds for
 *          that fixed-phi predictor; with phi fitted on the same points it is a very good approximation, not a guarantee.
 *   The quantities.  A = K_ss + noise I, B = A^-1, alpha = B y, os and noise exactly what adkf_predict_pool reads (zero prior mean);
 *          m(x), v(x) its mean and latent variance of pool row x; c_i(x) = sum_j K(x, z_j) B_ji; n = n_s[t].  For i < n:
 *              g_i           = alpha_i / B_ii                    (= y_i - mu_-i(z_i), the leave-one-out residual)
 *              loo_mean[t,i] = y_i - g_i,    loo_var[t,i] = 1 / B_ii   (the observed variance, noise included)
 *              loo_lpd[t]    = sum_i [ -log(2 pi / B_ii) / 2 - g_i^2 B_ii / 2 ]   (R&W eq. 5.10), summed by ascending i
 *              mu_-i(x)      = m(x) - c_i(x) g_i,                v_-i(x) = v(x) + c_i(x)^2 / B_ii
 *          (deleting point i is a rank-one update: no refactorisation).  Slots i >= n hold 0.  The fold values of a row:
 *              plain         a_i = mu_-i(x) - |g_i|,             b_i = mu_-i(x) + |g_i|
 *              scaled        a_i = mu_-i(x) - s_i sd_i(x),       b_i = mu_-i(x) + s_i sd_i(x)       (ADKF_PM_JK_SCALED: locally
 *                            s_i = |g_i| sqrt(B_ii),             sd_i(x) = sqrt(max(v_-i(x), 1e-12) + noise)      adaptive widths)
 *   alpha  [L] float32 on the device, shared by all tasks, 1 <= L <= ADKF_JK_LEVELS_MAX.  The rank of level l in task t is
 *          k = floor((double)alpha[l] * (n + 1)) - exact in double, so a function of the bits passed; a level that is NaN, <= 0 or
 *          >= 1 has k = 0.  lo[t, l, x] is the k-th smallest a_i, hi[t, l, x] the k-th largest b_i; k = 0 gives -inf / +inf: the
 *          support set is too small for that level.  [lo, hi] covers a new label with probability >= 1 - 2 alpha[l].  Order
 *          statistics are values: the answer is unique.
 *   lo, hi   nullable, [T, L, rows].     loo_mean, loo_var, loo_lpd   nullable, [T, ns_max], [T, ns_max], [T].
 *   k, top_idx, top_val   the selection of adkf_predict_pool ([T, k], its total order, exclusion lists and -1 / -inf tail) on the
 *          level-0 score: lo with ADKF_PM_MAXIMIZE, -hi without - conservative screening, by the bound one can rely on.  A row
 *          whose score is infinite or NaN is never selected.
 *   b      support-only, of either kind, as for adkf_kg_pool, with ns_max <= ADKF_JK_POINTS_MAX (beyond: ADKF_E_SIZE; with that many
 *          labels use a held-out split).  rows == 0 is valid: the plain leave-one-out diagnostic.
 *   flags  ADKF_PM_MAXIMIZE | ADKF_PM_JK_SCALED.
 *   Tasks with n_s == 0 or info != 0: zeros everywhere and -1 / -inf selections.  A pool row whose own mean or variance is NaN has
 *          NaN bounds and is never selected.
 *   scratch   adkf_jackknife_pool_scratch_bytes(T, ns_max, L, k) bytes, 8-byte aligned: g, 1 / B_ii and the width factor [T, ns_max]
 *          (with float64 copies), the ranks and the candidate lists.  A function of (T, ns_max, k) only, 0 for arguments out of
 *          range; nothing of size T x rows exists unless lo or hi is asked for.
 * Asynchronous on `stream` and capturable, no allocation, no synchronisation, no atomics, every sum in a fixed order: reproducible to
 * the bit, and a task's result depends on that task's data, the levels, the pool and its exclusion list only - not on the grid or on
 * the other tasks of the batch.  Rejected before anything is launched, ADKF_E_BADARG unless noted: ns_max > ADKF_JK_POINTS_MAX, L < 1
 * or L > ADKF_JK_LEVELS_MAX, k > ADKF_POOL_TOPK_MAX (ADKF_E_SIZE); alpha, info or ws NULL; a batch with a query set; a flag bit other
 * than the two above; rows < 0; rows > 0 without X; excl_idx without excl_off; k < 0; k > 0 without top_idx or top_val; no output at
 * all; a scratch or a workspace that is too small (ADKF_E_WORKSPACE); a scratch that is not 8-byte aligned. */
#define ADKF_PM_JK_SCALED 64         /* adkf_jackknife_pool only: fold widths scaled by the leave-one-out predictive deviation */
#define ADKF_JK_POINTS_MAX 256       /* FS-Mol's largest support size */
#define ADKF_JK_LEVELS_MAX 8
size_t adkf_jackknife_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t L, int32_t k);
int adkf_jackknife_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* alpha, int32_t L, const int64_t* excl_idx, const int64_t* excl_off, float* lo, float* hi, float* loo_mean, float* loo_var, float* loo_lpd, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Constrained expected hypervolume improvement ACROSS tasks over a shared pool (csrc/ehvi_stream.h; Emmerich, Deutz and Klinkenberg
 * 2011 and Yang et al. 2019 for the exact two-objective form, BoTorch's analytic ExpectedHypervolumeImprovement; Schonlau 1998 and
 * Gardner et al. 2014 for the feasibility weight, BoTorch's ConstrainedExpectedImprovement; ADKF_PM_LOG_EI: their log forms).  It
 * replaces a adkf_predict_pool call for mean and var [T, rows] combined on the host.  The T tasks of the batch are properties of the
 * SAME pool rows X [rows, d]; a GROUP g names one or two objective tasks and up to ADKF_EHVI_CONS_MAX constraint tasks among them (a
 * task may serve in several groups), and every pool row gets one score per group.
 *   The quantity.  m_t, v_t the latent posterior of adkf_predict_pool at the row, s_t = sqrt(max(v_t, 1e-12)).  An objective with
 *          obj_max != 0 is maximised: its mean, its column of the front and its reference coordinate are negated, so that everything
 *          below minimises.  psi_t(c) = E[(c - y_t)+] = s_t (z Phi(z) + phi(z)), z = (c - m_t) / s_t, psi_t(-inf) = 0: the ei of
 *          adkf_predict_pool with ADKF_PM_LATENT and best_f = c.
 *          Two objectives: the reference point r = ref[g] and the front[g] points of index below front_n[g] (clamped to [0, P]) are
 *          cleaned into a STAIRCASE: points with a NaN leave, then points not strictly better than r in both coordinates, then points
 *          weakly dominated by another one (of exact duplicates the one of lowest index stays); the rest is sorted by the first
 *          coordinate ascending (the second is then strictly descending): (a_1, b_1) .. (a_P', b_P').  With a_0 = -inf, b_0 = r2 and
 *          a_(P'+1) = r1,
 *              EHVI = sum_{i = 0 .. P'} [psi_1(a_(i+1)) - psi_1(a_i)] psi_2(b_i).
 *          One objective (obj[g, 1] == -1): EHVI = psi_1(r1), EI with best_f = r1; the front is not read.
 *          Constraints: PoF = prod_c Phi(z_c) in the order of the list, z_c = (thr_c - m_c) / s_c with con_geq == 0 (feasible when
 *          f <= thr) and (m_c - thr_c) / s_c otherwise, on the latent f.  An entry con[g, c] == -1 is unused.
 *          score = EHVI PoF; with ADKF_PM_LOG_EI, log EHVI + sum_c log Phi(z_c), formed in log space throughout (log psi as the log EI
 *          of adkf_predict_pool, the strips joined by a fixed-order log-sum-exp), which keeps an order where the linear score is 0.
 *          A single-objective group without constraints has, on every row, the bits of adkf_predict_pool's ei (ADKF_PM_LATENT, the
 *          objective's sense, best_f = ref[g, 0]), and its selection.
 *          A group cannot be evaluated when a task index is outside [0, T) (other than the -1 of "unused"), obj[g, 0] < 0, both
 *          objectives are the same task, a member task has n_s == 0 or info != 0, a used coordinate of ref[g] is NaN, or a used
 *          threshold is NaN: every score of the group is NaN and it selects nothing (top_idx -1, top_val -inf).  A pool row whose
 *          mean is NaN scores NaN in the groups whose tasks see it, and is never selected.
 *   b      support-only, of either kind, as for adkf_mes_pool; REUSE_DIST / REUSE_INNER and info [T] as for adkf_predict_pool.
 *   flags  ADKF_PM_LOG_EI only (the senses are per objective: ADKF_PM_MAXIMIZE is a bad argument here).
 *   G      groups, at least 1.  obj [G, 2] (int32), obj_max [G, 2] (0 | 1; NULL: all 0), ref [G, 2].
 *   front  [G, P, 2] with front_n [G], 0 <= P <= ADKF_EHVI_FRONT_MAX; NULL if and only if P == 0.
 *   con, con_thr, con_geq   [G, C] each, 0 <= C <= ADKF_EHVI_CONS_MAX; required when C > 0.
 *   excl_idx, excl_off   as for adkf_predict_pool, but per GROUP: excl_off is [G + 1].
 *   score  nullable, [G, rows].
 *   stair, stair_n   each nullable, [G, P, 2] and [G]: the cleaned staircase in the caller's units and sense, zero beyond stair_n[g]
 *          (0 points for a single-objective group).
 *   k, top_idx, top_val   the selection of adkf_predict_pool on the score, per group: [G, k], k <= ADKF_POOL_TOPK_MAX, its unique
 *          order, its -1 / -inf tail; a NaN score is never selected.
 *   scratch   adkf_ehvi_pool_scratch_bytes(T, G, k) bytes, 8-byte aligned: the mean and latent variance of one chunk of
 *          ADKF_EHVI_CHUNK_ROWS pool rows, [T, chunk] each (the pool is walked in such chunks, each through prediction's own launch,
 *          so m and v are adkf_predict_pool's bit for bit), the groups' state and the candidate lists.  It depends on neither rows,
 *          ns_max nor d; the size function returns 0 for T < 1, G < 1, k < 0 or k > ADKF_POOL_TOPK_MAX.
 * Asynchronous on `stream`, no allocation, no synchronisation, no atomics: reproducible to the bit, and a group's result depends on
 * its own tasks, front, reference, constraints, exclusion list and the pool only - not on the grid, on the other groups of the call
 * or on where the chunk boundaries fall.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: G < 1; P < 0 or P > ADKF_EHVI_FRONT_MAX, C < 0 or
 * C > ADKF_EHVI_CONS_MAX, k > ADKF_POOL_TOPK_MAX (ADKF_E_SIZE); obj, ref or front_n == NULL; P > 0 without front; C > 0 without con,
 * con_thr or con_geq; any flag bit other than ADKF_PM_LOG_EI; a batch with a query set; rows < 0; rows > 0 without X; k < 0; k > 0
 * without top_idx or top_val; excl_idx without excl_off; no output at all (k == 0 and score, stair and stair_n all NULL); a scratch or
 * a workspace that is too small (ADKF_E_WORKSPACE); a scratch that is not 8-byte aligned. */
#define ADKF_EHVI_FRONT_MAX 64
#define ADKF_EHVI_CONS_MAX 4
#define ADKF_EHVI_CHUNK_ROWS 16384 /* a multiple of 64: 128 KB of scratch per task, 8 bytes of traffic per (task, row) against ~2 ns d flops */
size_t adkf_ehvi_pool_scratch_bytes(int32_t T, int32_t G, int32_t k);
int adkf_ehvi_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, int32_t G, const int32_t* obj, const int32_t* obj_max, const float* ref, const float* front, const int32_t* front_n, int32_t P, const int32_t* con, const float* con_thr, const int32_t* con_geq, int32_t C, const int64_t* excl_idx, const int64_t* excl_off, float* score, float* stair, int32_t* stair_n, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Hyperparameter-marginalised prediction and acquisition over a shared pool (csrc/mix_stream.h; the integrated acquisition of Snoek,
 * Larochelle and Adams 2012, BoTorch's average over the MCMC batch of a fully Bayesian model; Riis et al. 2022 and BoTorch's
 * qBayesianActiveLearningByDisagreement for ADKF_PM_SCORE_BALD).  It replaces a adkf_predict_pool call for mean, var and ei [T, rows]
 * on M replicas of every task, combined and selected on the host.  The T tasks of the batch are MODELS of the SAME pool rows
 * X [rows, d] - usually the same data under M samples of phi; a GROUP g names up to ADKF_MIX_MEMBERS_MAX member tasks mem[g, 0..M)
 * (a task may serve in several groups; a task repeated inside a group counts each time) with weights w[g, 0..M) (NULL: all 1), and
 * every pool row gets one mean, variance and score per group.
 *   Used entries.  An entry is USED when mem != -1 and its weight is > 0 (the weight of an entry with mem == -1 is not read).  The
 *          used entries are compacted in entry order into the slots 0 .. n - 1; W is the float32 sum of their weights in that
 *          order and wt_i = w_i / W.
 *   The quantities.  m_i, v_i, e_i: adkf_predict_pool's mean, var and ei of member i at the row under the caller's flags - var with
 *          the member's own noise unless ADKF_PM_LATENT, ei on the latent variance with best_f[t_i] in the ADKF_PM_MAXIMIZE sense,
 *          log EI with ADKF_PM_LOG_EI.
 *              mean  = sum_i wt_i m_i
 *              var   = sum_i wt_i v_i + sum_i wt_i (m_i - mean)^2     (total variance; the second term from the deviations, not
 *                                                                      as E[m^2] - mean^2)
 *              score = sum_i wt_i e_i                                 (default: the integrated EI)
 *                    = log sum_i wt_i exp(le_i)                       (ADKF_PM_LOG_EI: its logarithm, as mx + log sum_i wt_i
 *                                                                      exp(le_i - mx), mx = max_i le_i, in a fixed order; EI is
 *                                                                      never formed, -inf terms are skipped, all -inf gives -inf)
 *                    = +mean with ADKF_PM_MAXIMIZE, -mean without     (ADKF_PM_SCORE_MEAN)
 *                    = (log var_c - sum_i wt_i log vc_i) / 2          (ADKF_PM_SCORE_BALD: vc_i = max(v_i, 1e-12), var_c the
 *                                                                      variance above from the vc_i; not clamped at 0, it may round
 *                                                                      a few ulp of the logarithms below 0)
 *          Every sum is taken over four interleaved partials (slots p, p + 4, ..) that start from -0 and are joined in the order
 *          0, 1, 2, 3.  ANCHORS: a group with one used member, and a group of two used entries that name the same task with equal
 *          weights, have on every row the bits of adkf_predict_pool's mean, var and ei (log EI) of that task under the same flags,
 *          and its selection; their BALD score is exactly 0.  A group's bits depend on the ORDER of its members, by rounding only.
 *          A group cannot be evaluated when an index is outside [0, T) other than -1, a weight of an entry with mem != -1 is
 *          negative, NaN or infinite, no entry is used, the weights do not sum to a finite number, or a used member has n_s == 0 or
 *          info != 0: mean, var and score of the group are NaN on every row and it selects nothing (top_idx -1, top_val -inf); the
 *          other groups keep their bits.  A pool row whose members are NaN is NaN, and never selected.
 *   b      support-only, of either kind, as for adkf_mes_pool; REUSE_DIST / REUSE_INNER and info [T] as for adkf_predict_pool.  Every
 *          task of the batch is predicted, whether a group names it or not.
 *   flags  ADKF_PM_LATENT, ADKF_PM_MAXIMIZE, and at most one of ADKF_PM_SCORE_MEAN, ADKF_PM_LOG_EI, ADKF_PM_SCORE_BALD.
 *   G, mem, w, M   G >= 1 groups; mem [G, M] (int32), w [G, M] nullable, 1 <= M <= ADKF_MIX_MEMBERS_MAX.
 *   best_f [T], per member task: needed when the EI or log-EI score is read (score != NULL or k > 0).
 *   excl_idx, excl_off   as for adkf_predict_pool, but per GROUP: excl_off is [G + 1].
 *   mean, var, score   each nullable, [G, rows].
 *   k, top_idx, top_val   the selection of adkf_predict_pool on the score, per group: [G, k], k <= ADKF_POOL_TOPK_MAX, its
 *          eligibility, its unique order (score, then row index), its -1 / -inf tail; a NaN score is never selected.
 *   scratch   adkf_mix_pool_scratch_bytes(T, G, k) bytes, 8-byte aligned and a multiple of 8: three planes [T, ADKF_MIX_CHUNK_ROWS]
 *          (the pool is walked in such chunks, each through prediction's own launch, so m, v and e are adkf_predict_pool's bit for
 *          bit), the groups' state and the candidate lists.  It depends on neither rows, ns_max, d nor M; the size function returns
 *          0 for T < 1, G < 1, k < 0 or k > ADKF_POOL_TOPK_MAX.
 * Asynchronous on `stream`, no allocation, no synchronisation, no atomics: reproducible to the bit, and a group's result depends on
 * its own members, weights, best_f, exclusion list and the pool row only - not on the grid, on the other groups of the call or on
 * where the chunk boundaries fall.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: G < 1; M < 1; mem == NULL; k < 0; M > ADKF_MIX_MEMBERS_MAX or
 * k > ADKF_POOL_TOPK_MAX (ADKF_E_SIZE); a flag bit other than the five above; ADKF_PM_SCORE_MEAN with ADKF_PM_SCORE_BALD;
 * ADKF_PM_LOG_EI with either; the EI or log-EI score read without best_f; k > 0 without top_idx or top_val; no output at all (k == 0
 * and mean, var and score all NULL); a batch with a query set; rows < 0; rows > 0 without X; excl_idx without excl_off; a scratch
 * or a workspace that is too small (ADKF_E_WORKSPACE); a scratch that is not 8-byte aligned. */
#define ADKF_PM_SCORE_BALD 32      /* adkf_mix_pool only: rank by the disagreement of the members */
#define ADKF_MIX_MEMBERS_MAX 64
#define ADKF_MIX_CHUNK_ROWS 16384  /* a multiple of 64: 192 KB of scratch per task */
size_t adkf_mix_pool_scratch_bytes(int32_t T, int32_t G, int32_t k);
int adkf_mix_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, int32_t G, const int32_t* mem, const float* w, int32_t M, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off, float* mean, float* var, float* score, int32_t k, int64_t* top_idx, float* top_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Large-k selection and row ranks over a shared pool (csrc/rank_stream.h): what a virtual screen asks beyond a BO batch.  Every task
 * ranks the SAME pool X [rows, d] by adkf_predict_pool's score and returns its first k rows, k up to ADKF_RANK_K_MAX instead of
 * ADKF_POOL_TOPK_MAX, the rank of up to ADKF_RANK_REFS_MAX named rows (known actives: enrichment factors and every retrospective
 * screening metric) and the number of rows ranked.  Nothing of size T x rows exists.
 *   score  adkf_predict_pool's, bit for bit: EI on the latent variance against best_f[t] in the ADKF_PM_MAXIMIZE sense, log EI with
 *          ADKF_PM_LOG_EI, +mean (ADKF_PM_MAXIMIZE) or -mean with ADKF_PM_SCORE_MEAN.  A row is ELIGIBLE when its score is not NaN and
 *          it is not in the task's exclusion list (excl_idx / excl_off as adkf_predict_pool).  THE ORDER: larger score first, equal
 *          scores by ascending row; -0 and +0 tie; a score of -inf is eligible and comes last.
 *   flags  ADKF_PM_LATENT (accepted, no score reads it), ADKF_PM_MAXIMIZE, ADKF_PM_SCORE_MEAN, ADKF_PM_LOG_EI (not with SCORE_MEAN);
 *          any other bit is ADKF_E_BADARG.  best_f [T] is required unless the score is the mean.
 *   k, top_idx, top_val   [T, k], 0 <= k <= ADKF_RANK_K_MAX: the first k eligible rows in the order, -1 / -inf where fewer are
 *          eligible.  top_val has the score's own bits, the sign of a zero included.  The first min(k, 64) entries are
 *          adkf_predict_pool's selection.  k == 0 needs M > 0 or n_ranked.
 *   ref_idx, M, ref_rank, ref_val   [T, M], 0 <= M <= ADKF_RANK_REFS_MAX (ref_idx nullable with M == 0): ref_rank[t, j] is the number
 *          of eligible pool rows that come strictly before row ref_idx[t, j] in the order - 0-based, counted whether or not the row
 *          itself is excluded (an excluded row gets the position it would take) - and ref_val[t, j] that row's score.  An eligible
 *          row with ref_rank < k is top_idx[t, ref_rank].  An entry outside [0, rows) or a row with a NaN score gives -1 / NaN;
 *          repeated entries are independent.
 *   n_ranked   [T], nullable: the eligible rows of the task, the denominator of every percentile.
 *   b, ws  support-only, of either kind (ADKF_BATCH_ARD or not), plain, refined and float64 tasks, as for adkf_mix_pool; REUSE_DIST /
 *          REUSE_INNER and info [T] as for adkf_predict_pool.  Tasks with n_s == 0 or info != 0: top_idx -1, top_val -inf,
 *          ref_rank -1, ref_val NaN, n_ranked 0.
 *   scratch   adkf_rank_pool_scratch_bytes(T, k, M, d) bytes, 8-byte aligned.  With r(x) = x rounded up to a multiple of 256:
 *              r(4 T ADKF_RANK_CHUNK_ROWS)                 the score plane of one chunk (the pool is walked in such chunks, each
 *                                                          through prediction's own launch, so the scores are adkf_predict_pool's)
 *            + r(16 T k) + r(8 T k) + r(8 T)               two sorted lists per task, rows and scores, and which one is current
 *            + r(4 T M d) + 2 r(4 T M) + r(8 (T + 1))      the refs' rows as a packed query set, prediction's outputs on them and
 *                                                          its offsets (the refs' scores are known before the walk: prediction's
 *                                                          packed launch on T M rows, which has the pool launch's bits)
 *          It depends on neither rows nor ns_max; the size function returns 0 for T < 1, d < 1, k or M out of range.  The ranks are
 *          counted in ref_rank and n_ranked themselves.
 * Asynchronous on `stream`, no allocation, no synchronisation, no device-to-host read, no floating-point atomics: capturable, and
 * reproducible to the bit; a task's result depends on its own data, best_f, exclusion list, refs and the pool only - not on the grid,
 * on the other tasks or on where the chunk boundaries fall.
 * Rejected before anything is launched, ADKF_E_BADARG unless noted: a batch with a query set; rows < 0; rows > 0 without X; a flag
 * bit other than the four above; ADKF_PM_LOG_EI with ADKF_PM_SCORE_MEAN; k < 0; M < 0; k > ADKF_RANK_K_MAX or M > ADKF_RANK_REFS_MAX
 * (ADKF_E_SIZE); the EI or log-EI score without best_f; excl_idx without excl_off; k > 0 without top_idx or top_val; M > 0 without
 * ref_idx, ref_rank or ref_val; nothing asked for (k == 0, M == 0 and n_ranked NULL); scratch NULL; a scratch that is too small or
 * not 8-byte aligned, or a workspace that is too small (ADKF_E_WORKSPACE). */
#define ADKF_RANK_K_MAX 65536
#define ADKF_RANK_REFS_MAX 1024
#define ADKF_RANK_CHUNK_ROWS 16384 /* as ADKF_EHVI_CHUNK_ROWS / ADKF_MIX_CHUNK_ROWS: 64 KB of scratch per task */
size_t adkf_rank_pool_scratch_bytes(int32_t T, int32_t k, int32_t M, int32_t d);
int adkf_rank_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off, int32_t k, int64_t* top_idx, float* top_val, const int64_t* ref_idx, int32_t M, int64_t* ref_rank, float* ref_val, int64_t* n_ranked, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Monte-Carlo q-EI and noisy q-EI over a shared pool: a batch of q rows per task, chosen by sequential-greedy maximisation of the
 * sample-average joint improvement over S pathwise posterior draws (Wilson, Hutter and Deisenroth 2018, "Maximizing acquisition
 * functions for Bayesian optimization"; Balandat et al. 2020, BoTorch; the noisy incumbent of Letham et al. 2019, "Constrained
 * Bayesian optimization with noisy experiments").  Replaces BoTorch's qNoisyExpectedImprovement (best_f NULL) or
 * qExpectedImprovement (best_f given) under optimize_acqf_discrete's sequential greedy with fixed base samples.
 *
 * Isotropic and ARD batches alike (ADKF_BATCH_ARD, as adkf_mes_pool); the batch is support-only.  All per task t, with the
 * paths f_s of adkf_thompson_pool on the same arguments (omega [m, d], phase [m], w [T, S, m], eps [T, S, ns_max]; m under
 * Thompson's limits, 1 <= S <= ADKF_QEI_SAMPLES_MAX), so the call is a deterministic function of its arguments:
 *     f_s(x) = g_s(x) + k(x, Z_s) v_s,  v_s = A^-1 r_s,  r_s = y - g_s(Z_s) - sqrt(noise) eps_s
 * Minimisation by default: imp_s(x) = b_s - f_s(x) and incumbents move by min; ADKF_PM_MAXIMIZE (the only flag accepted) flips both.
 *   incumbent   best_f NULL:  b_s^0 = min_(i < n_s[t]) f_s(z_i), the best value of path s over the task's own support rows, taken as
 *               y_i - sqrt(noise) eps_(s,i) - noise v_(s,i) (A v = r and K_ss = A - noise I: no further product);
 *               best_f [T]:   b_s^0 = best_f[t] for every s.
 *   step j      score_j(x) = (1 / S) sum_s max(0, imp_s^j(x)); the pick p_j is the eligible row of largest score, equal scores by
 *               the lower row index; eligible: not in the task's exclusion list (excl_idx / excl_off as adkf_predict_pool) and not an
 *               earlier pick; NaN scores are never selected.  Then b_s^(j+1) = min(b_s^j, f_s(p_j)).  With no eligible row the step
 *               reports -1 / -inf, leaves the state unchanged, and every later step does the same (adkf_believer_pool's rule).
 * Hence score_(j+1)(x) <= score_j(x) for every row, and sum_j score_j(p_j) = (1 / S) sum_s (b_s^0 - b_s^q), the MC q-EI of the batch.
 * Outputs: sel_idx, sel_val [T, q] (1 <= q <= ADKF_QEI_PICKS_MAX); inc [T, q + 1, S] (nullable): the incumbents b_s^j, row 0 the
 * starting ones; trace [T, q, rows] (nullable): every row's score at every step (zeros for skipped tasks).  With trace and inc
 * NULL nothing of size T x rows exists; the scratch does not depend on rows: V [T, S, ns_max] (and its float64 twin where the
 * workspace of this shape can have a float64 region), the incumbents [T, S], a pick count per task, and per (task, chunk) one
 * candidate: (row, score) and that row's S path values.  Flags other than ADKF_PM_MAXIMIZE: BADARG; S, m or q out of range: SIZE
 * (adkf_qei_pool_scratch_bytes returns 0 for them); a short scratch: WORKSPACE; a misaligned one: BADARG. */
#define ADKF_QEI_SAMPLES_MAX 256
#define ADKF_QEI_PICKS_MAX 64
size_t adkf_qei_pool_scratch_bytes(int32_t T, int32_t ns_max, int32_t S, int32_t m);
int adkf_qei_pool(const adkf_batch_t* b, const float* phi, int32_t flags, const float* X, int64_t rows, const float* omega, const float* phase, int32_t m, const float* w, const float* eps, int32_t S, const float* best_f, const int64_t* excl_idx, const int64_t* excl_off, int32_t q, float* trace, float* inc, int64_t* sel_idx, float* sel_val, int32_t* info, void* ws, size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* a8 (training branch) = f_outer (fs_mol/models/adaptive_dkt.py:183-191): joint predictive NLL of the query
 * set, with gradients: f_out [T], g_phi [T,3] (nullable), dZ_s, dZ_q (nullable). */
int adkf_outer_nll_value_grad(const adkf_batch_t* b, const float* phi, float* f_out, float* g_phi, float* dZ_s,
                              float* dZ_q, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* a9/a10: cauchy_hypergradient / cauchy_hypergradient_jvp (fs_mol/utils/cauchy_hypergradient.py:5-163,
 * cauchy_hypergradient_jvp.py:5-156) at the feature-matrix level, all tasks at once:
 *   dL/dZ = d f_out/dZ - d( v^T grad_phi f_in )/dZ,  v = H^-1 grad_phi f_out,  H = d2 f_in / d phi2.
 * Outputs: f_out [T]; dZ_s [T,ns_max,d]; dZ_q [T,nq_max,d]; g_phi_out [T,3] (what the reference leaves in
 * phi.grad); v [T,3] and H [T,9] (nullable, diagnostics).  One backward pass of the caller's feature
 * extractor with (dZ_s, dZ_q) as cotangents then yields exactly theta.grad of the reference. */
int adkf_ift_hypergrad(const adkf_batch_t* b, const float* phi, int32_t flags, float* f_out, float* dZ_s,
                       float* dZ_q, float* g_phi_out, float* v, float* H, int32_t* info, void* ws,
                       size_t ws_bytes, void* stream);

/* Diagnostic: flagged[t] = 1 if task t took the float64 path (ill-conditioned: pivot ratio of the sweep of A or of
 * Sigma_q above the threshold, csrc/refine64.h) in the last adkf_ift_hypergrad / adkf_outer_nll_value_grad on this
 * workspace, else 0.  Non-ARD batches.  No reference counterpart (GPyTorch has one precision); bench.py --regression
 * reports the fraction (fs_mol/utils/gp_utils.py:17: noise 0.01 for numeric labels is where such tasks come from). */
int adkf_double_path_tasks(const adkf_batch_t* b, int32_t* flagged, void* ws, size_t ws_bytes, void* stream);

/* Workspace size for batches that carry ADKF_BATCH_ARD (a superset of adkf_workspace_bytes). */
size_t adkf_workspace_bytes_ard(int32_t T, int32_t ns_max, int32_t nq_max, int32_t d);

/* adkf_ift_hypergrad for ARD batches with explicit conjugate-gradient controls (the north-star's "HVP + CG"):
 * at most cg_maxiter iterations, stop at |r| <= cg_tol |grad f_out|; cg_iters [T] (nullable) receives the iterations
 * each task used.  Converged tasks drop out of the products; outside stream capture (and for cg_maxiter > 16) the call
 * synchronises the stream every 8 iterations to stop enqueueing once every task has converged. */
int adkf_ift_hypergrad_cg(const adkf_batch_t* b, const float* phi, int32_t flags, int32_t cg_maxiter, float cg_tol,
                          float* f_out, float* dZ_s, float* dZ_q, float* g_phi_out, float* v, int32_t* cg_iters,
                          int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* a1 (message functions of RelationalMP, fs_mol/modules/gnn.py:95-148, for the default depth-1 message MLP): all towers of ALL
 * edge types in one batched GEMM with the source / target node states gathered on the fly:
 *   msgs[e_off(t) + e, h, :] = relu(cat(x[src_e, h, :], x[tgt_e, h, :]) W_t[h] + bias_t[h])   for edge e of edge type t,
 * x [V, H, in], W_t [H, 2 in, out], bias_t [H, out], msgs [E_all, H, out]; the edge types' rows follow one another in msgs in
 * the order of `ets` (e_off = number of edges of the types before); at most 4 edge types.
 * The backward is reproducible to the bit - no floating-point atomics (the reference's scatter ops and PyTorch's index_add_
 * are, on a GPU): d cat[e, h, :] = (d msgs . [msgs > 0]) W[h]^T is written once per edge into dcat [E_all, H, 2 in]; dx [V, H, in]
 * is then the sum over each node's outgoing edges of the first half of d cat and over its incoming edges of the second half, in
 * the order of the two CSR lists (perm_*: edge ids of the concatenated edge list sorted stably by source / target node,
 * rowptr_* [V + 1]); every edge type's dW [H, 2 in, out] and db [H, out] are sums over fixed chunks of its edges (partials in
 * `scratch`, at least adkf_msg_backward_scratch_bytes() bytes), added in a fixed order.  Nothing needs initialising; an edge type
 * without edges gets exact zeros.  msgs = NULL in the backward: d_msgs is already the gradient in front of the ReLU
 * (adkf_pna_aggregate_backward_relu below) and no mask is applied.
 * A batch without a single edge (E_all = 0) is legal: nothing of msgs / d_msgs / dcat / perm_* is read or written, the forward
 * launches nothing, the backward writes zeros to every dW, db and dx.  The pointers must still be non-NULL (a NULL argument is
 * ADKF_E_BADARG here and in adkf_pna_aggregate*): a caller whose empty tensors have no address passes any valid one. */
typedef struct adkf_msg_et {
    const int64_t* src; /* [E] source node of every edge */
    const int64_t* tgt; /* [E] target node */
    const float* W;     /* [H, 2 in, out] */
    const float* bias;  /* [H, out] (forward) */
    float* dW;          /* [H, 2 in, out] (backward: output) */
    float* db;          /* [H, out]       (backward: output) */
    int32_t E;
} adkf_msg_et_t;
int adkf_msg_forward(const float* x, const adkf_msg_et_t* ets, int32_t n_et, int32_t H, int32_t in, int32_t out, float* msgs,
                     void* stream);
size_t adkf_msg_backward_scratch_bytes(const adkf_msg_et_t* ets, int32_t n_et, int32_t H, int32_t in, int32_t out);
int adkf_msg_backward(const float* x, const adkf_msg_et_t* ets, int32_t n_et, int32_t H, int32_t in, int32_t out, const float* msgs,
                      const float* d_msgs, const int64_t* perm_src, const int64_t* rowptr_src, const int64_t* perm_tgt,
                      const int64_t* rowptr_tgt, int32_t V, float* dcat, float* dx, void* scratch, size_t scratch_bytes,
                      void* stream);

/* a1 (per-graph pooling of CombinedGraphReadout, fs_mol/modules/graph_readout.py:119-177: the weighted-mean head's
 * scatter_softmax + index_add_ :238-252, the weighted-sum head's sigmoid weights :236, the max pooler's scatter :289) between
 * the node-level MLPs and the combination layers, every per-graph sum in the fixed order of the graph's node list:
 *   w_mean = segment-softmax(s_mean), g_mean[g] = sum_v w_mean[v] v_mean[v];  w_sum = sigmoid(s_sum), g_sum likewise;
 *   g_max[g] = max_v emb[v] (0 and argmax -1 for a graph without nodes; first maximum in list order).
 * s_* [V, nh], v_* [V, nh, hd], emb [V, D]; perm [V] node ids sorted stably by graph, rowptr [G + 1]; nh <= 64.  Outputs w_*
 * [V, nh] (kept for the backward), g_mean / g_sum [G, nh hd], g_max / argmax [G, D].  The backward writes every element of
 * d_s_* [V, nh], d_v_* [V, nh hd], d_emb [V, D] exactly once (no scatter). */
int adkf_readout_pool(const float* s_mean, const float* v_mean, const float* s_sum, const float* v_sum, const float* emb,
                      const int64_t* perm, const int64_t* rowptr, int32_t V, int32_t G, int32_t nh, int32_t hd, int32_t D,
                      float* w_mean, float* w_sum, float* g_mean, float* g_sum, float* g_max, int32_t* argmax, void* stream);
int adkf_readout_pool_backward(const float* v_mean, const float* v_sum, const float* w_mean, const float* w_sum,
                               const float* g_mean, const int32_t* argmax, const int64_t* node_to_graph, const float* dg_mean,
                               const float* dg_sum, const float* dg_max, int32_t V, int32_t G, int32_t nh, int32_t hd, int32_t D,
                               float* d_s_mean, float* d_v_mean, float* d_s_sum, float* d_v_sum, float* d_emb, void* stream);

/* The same pooling taken BEFORE the last layer of the two value MLPs (graph_readout.py:219-223: _transformation_mlp = Linear . ReLU .
 * Linear; :242-252 pools its output).  Pooling is linear in that last layer, so
 *     g[g, h, :] = W2[h] p[h, g, :] + b2[h] wtot[g, h],   p[h, g, :] = sum_v w[v, h] r_v,   wtot[g, h] = sum_v w[v, h],
 * with r_v [K] the hidden activations: the caller multiplies nh small [G, K] x [K, hd] products instead of [V, K] x [K, nh hd].
 * h_mean / h_sum: rows of K floats with row stride ldh (column blocks of one activation tensor), K <= 1024; p_* [nh, G, K];
 * wtot_mean (1, or 0 for an empty graph) and wtot_sum [G, nh]; everything else as adkf_readout_pool.  The backward takes dp_*
 * [nh, G, K], dwtot_sum [G, nh], dg_max and writes d_s_* [V, nh], d_h_* [V, K] (contiguous), d_emb [V, D], every element once. */
int adkf_readout_pool_hidden(const float* s_mean, const float* h_mean, const float* s_sum, const float* h_sum, int32_t ldh,
                             const float* emb, const int64_t* perm, const int64_t* rowptr, int32_t V, int32_t G, int32_t nh,
                             int32_t K, int32_t D, float* w_mean, float* w_sum, float* p_mean, float* p_sum, float* wtot_mean,
                             float* wtot_sum, float* g_max, int32_t* argmax, void* stream);
int adkf_readout_pool_hidden_backward(const float* h_mean, const float* h_sum, int32_t ldh, const float* w_mean, const float* w_sum,
                                      const int32_t* argmax, const int64_t* perm, const int64_t* rowptr, const float* dp_mean,
                                      const float* dp_sum, const float* dwtot_sum, const float* dg_max, int32_t V, int32_t G,
                                      int32_t nh, int32_t K, int32_t D, float* d_s_mean, float* d_h_mean, float* d_s_sum,
                                      float* d_h_sum, float* d_emb, void* stream);

/* a1 (aggregation inside RelationalMultiAggrMP._aggregate_messages, fs_mol/modules/gnn.py:197-265; torch_scatter's
 * scatter_sum / scatter_mean / scatter_max there): SUM | MEAN | STD | MAX of the incoming messages of every target
 * node in one pass.  msgs [E, H, 3m] post-ReLU messages (per tower: sum-part | mean/std-part | max-part), perm [E] the
 * message ids sorted by target, rowptr [V+1]; agg [V, H, 4m], argmax [V, H, m] (message id of the maximum, -1 for an
 * empty segment, whose aggregates are 0).  The backward writes every element of d_msgs [E, H, 3m] exactly once. */
int adkf_pna_aggregate(const float* msgs, const int64_t* perm, const int64_t* rowptr, int32_t V, int32_t H, int32_t m,
                       float* agg, int32_t* argmax, void* stream);
int adkf_pna_aggregate_backward(const float* msgs, const int64_t* perm, const int64_t* rowptr, const float* agg,
                                const int32_t* argmax, const float* d_agg, int32_t V, int32_t H, int32_t m,
                                float* d_msgs, void* stream);
/* The same with the ReLU in front of the messages folded in (msgs are the ReLU OUTPUTS of the message functions, gnn.py:141):
 * d_pre = d_msgs . [msgs > 0], the gradient in front of that ReLU.  adkf_msg_backward takes it with msgs = NULL and then reads one
 * [E, H, 3m] tensor per product instead of gradient + mask (its three products are bound by exactly that traffic). */
int adkf_pna_aggregate_backward_relu(const float* msgs, const int64_t* perm, const int64_t* rowptr, const float* agg,
                                     const int32_t* argmax, const float* d_agg, int32_t V, int32_t H, int32_t m, float* d_pre,
                                     void* stream);

/* a1 (the element-wise middle of GNNBlock.forward, fs_mol/modules/gnn.py:477-515, between the output projection of the message
 * passing and the BOOM MLP):   new = p0 + amp[v] p1 + att[v] p2 + bias  (p = [p0 | p1 | p2] [V, 3 hid]: the projected unscaled
 * aggregates; amp / att [V]: the PNA scalers),   x1 = x + alpha new  (ReZero),   h = LayerNorm(x1; gamma, beta, eps).
 * x1 is formed as ((p0 + amp p1) + att p2) + bias, then x + alpha new, every product and every sum rounded on its own (no fused
 * multiply-add): bit for bit the numbers of the float32 PyTorch expression of adkf_ift_amd/gnn.py::GNNBlock.
 * Outputs x1, h [V, hid] and the row statistics mu, rstd [V] the backward needs.  hid a multiple of 64, at most 256 (else
 * ADKF_E_SIZE: the caller keeps its own path).  The backward takes the gradients arriving at x1 (g_x1) and h (g_h) and writes d_p
 * [V, 3 hid], d_x [V, hid] and the parameter gradients d_bias, d_gamma, d_beta [hid], d_alpha [1], reduced over the nodes in a fixed
 * order (per-workgroup partials in `scratch`, adkf_block_combine_scratch_bytes(V, hid) bytes): bit-reproducible. */
int adkf_block_combine(const float* p, const float* x, const float* amp, const float* att, const float* bias, const float* alpha,
                       const float* gamma, const float* beta, float eps, int32_t V, int32_t hid, float* x1, float* h, float* mu,
                       float* rstd, void* stream);
size_t adkf_block_combine_scratch_bytes(int32_t V, int32_t hid);
int adkf_block_combine_backward(const float* p, const float* x1, const float* amp, const float* att, const float* bias,
                                const float* alpha, const float* gamma, const float* mu, const float* rstd, const float* g_x1,
                                const float* g_h, int32_t V, int32_t hid, float* d_p, float* d_x, float* d_bias, float* d_alpha,
                                float* d_gamma, float* d_beta, void* scratch, size_t scratch_bytes, void* stream);

/* H (outer update of ADKTModelTrainer.train_loop, fs_mol/utils/adaptive_dkt_utils.py:402-413: task-mean of the
 * accumulated gradients, torch.nn.utils.clip_grad_norm_, torch.optim.Adam.step) for a handful of parameter tensors.
 *   adkf_grad_sumsq      partials[0 .. ADKF_SUMSQ_PARTS) = per-workgroup sums of g^2 (fixed partition: deterministic).
 *   adkf_clip_adam_step  with |g| = sqrt(sum of the n_partials partials, i.e. those of ALL tensors laid side by side):
 *                        g <- g * scale * min(1, clip / (scale |g| + 1e-6));  then Adam step number `step` (1-based;
 *                        exp_avg m, exp_avg_sq v, no amsgrad, weight_decay added to g as torch does).  clip = +inf
 *                        disables clipping.  Hyper-parameters are doubles: 1 - beta and lr / (1 - beta1^step) are formed in double
 *                        and rounded once, as torch does.  All pointers 16-byte aligned, n elements each.
 *   adkf_clip_adam_step_one  the two calls above as ONE launch for ONE tensor of at most ADKF_CLIP_ADAM_ONE_MAX elements (every
 *                        workgroup re-adds the whole gradient's squares in the same fixed order: deterministic, identical on every rank;
 *                        ADKF_E_SIZE beyond the limit).  planes_t (or NULL): the tensor is a row-major weight w[K][N] (n = K * N, K and N
 *                        multiples of 64) and the three bfloat16 pieces of every UPDATED weight are also written as planes[q][n][k] - what
 *                        adkf_split_planes_t(w) would give after the step, bit for bit - so that the next adkf_dense_forward of y = x w
 *                        needs no split launch. */
#define ADKF_SUMSQ_PARTS 256
#define ADKF_CLIP_ADAM_ONE_MAX 131072
int adkf_grad_sumsq(const float* g, int64_t n, float* partials, void* stream);
int adkf_clip_adam_step(float* p, float* g, float* m, float* v, int64_t n, const float* partials, int32_t n_partials,
                        float scale, float clip, double lr, double beta1, double beta2, double eps, double weight_decay,
                        int32_t step, void* stream);
int adkf_clip_adam_step_one(float* p, float* g, float* m, float* v, int64_t n, float scale, float clip, double lr, double beta1,
                            double beta2, double eps, double weight_decay, int32_t step, uint16_t* planes_t, int32_t K, int32_t N,
                            void* stream);

/* a1 / a2 (the dense layers of the feature extractor and of the fc head: torch.nn.Linear, fs_mol/modules/gnn.py:477-515,
 * fs_mol/modules/graph_readout.py, fs_mol/models/adaptive_dkt.py:50-65) with FP32 products on the BF16 matrix pipe (csrc/dense_x3.h,
 * csrc/gemm_x3.h: a float is the exact sum of three bfloat16 values; six BF16 MFMAs per product block; errors below the FP32 GEMM's).
 *   adkf_split_planes         planes[q][r][k], q = 0..2: the three bfloat16 pieces of x[r][k] (x0 = bf16(x), x1 = bf16(x - x0), x2 = the rest,
 *                       every cut rounding to nearest even: their sum is x exactly for |x| >= 2^-108 and for 0; below that a piece is a
 *                       bfloat16 denormal and nothing is promised).  `planes`: 3 * rows * K uint16, 16-byte aligned; K even; rows * K a
 *                       multiple of 8; x 8-byte aligned.
 *   adkf_split_planes_t       the same from the transpose: w[K][N] (a weight stored input-major, as torch.matmul(x, w) takes it) ->
 *                       planes[q][n][k], i.e. the planes adkf_dense_forward wants for y = x w.  K even; N * K a multiple of 8.
 *   adkf_dense_forward  y[M, N] = x[M, K] w[N, K]^T (+ bias[N]): torch's F.linear, with w given as the planes adkf_split_planes wrote
 *                       (weights are split once per update, activations on the fly).  K a multiple of 32; ldx, ldy the row strides
 *                       of x, y in floats (ldx a multiple of 4); x and w_planes 16-byte aligned, y 4-byte aligned (the stores are 16-byte wide where y and ldy
 *                       allow it).  A row of x that holds a non-finite value - or a finite one above bfloat16's largest finite value,
 *                       3.3895e38, whose first piece is inf - gives non-finite outputs in that row of y and nowhere else; the same holds
 *                       for a row of w and its column of y.  The backward product with respect to x is
 *                       the same call on the planes of w^T.  Returns ADKF_E_LAUNCH when the device refuses the kernel's 120 KB of
 *                       dynamic LDS.  Short contractions over many rows (K = 64, 128 or 256 and at least one 128-row tile per CU) take a
 *                       persistent form of the kernel (k_dense3_sk: a row tile's whole K extent in registers); the results are the same bits. */
int adkf_split_planes(const float* x, uint16_t* planes, int64_t rows, int64_t K, void* stream);
int adkf_split_planes_t(const float* w, uint16_t* planes, int64_t K, int64_t N, void* stream);
int adkf_dense_forward(const float* x, int32_t ldx, const uint16_t* w_planes, const float* bias, float* y, int32_t ldy, int32_t M,
                       int32_t N, int32_t K, void* stream);
 /*   adkf_dense_weight_grad  dw[N, K] = g[M, N]^T x[M, K] (torch: g.t() @ x), the contraction over the rows cut into row ranges whose
 *                       partial products are added in a fixed order (bit-reproducible); `scratch`: adkf_dense_weight_grad_scratch_bytes(M, N, K)
 *                       bytes.  Any M, N, K; ldg, ldx the row strides of g, x in floats. */
size_t adkf_dense_weight_grad_scratch_bytes(int32_t M, int32_t N, int32_t K);
int adkf_dense_weight_grad(const float* g, int32_t ldg, const float* x, int32_t ldx, float* dw, int32_t M, int32_t N, int32_t K,
                           void* scratch, size_t scratch_bytes, void* stream);

/* Synchronises `stream`, then returns 0 or (index+1) of the first task with info != 0. */
int adkf_check_info(const int32_t* info, int32_t T, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADKF_GP_H */
