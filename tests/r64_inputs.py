"""Seeded inputs of the tests of the float64 path of ill-conditioned tasks (csrc/refine64.h: k_refine64, k_tail64 and their float64 products,
inverses and mat-vecs), built on the CPU, each with its float64 reference and a bound that comes from the reference alone.
tests/test_gpu_float64_path.py runs the library on them, tests/test_r64_inputs.py checks (without a GPU) that they have the properties the
comparisons rely on: every task sits a factor of two on its side of the path's threshold, every flagged task would fail if it were silently
left on the float32 path, every bound is at least three times sharper than the suite's 1e-4 x slack.

A case is a small ragged batch at a phi chosen directly (float32 raw values: noise 0.003 .. 0.01 for the flagged tasks, 0.1 for the
controls, outputscale 1, a lengthscale chosen with the features).  Features of a flagged task: one common row plus a spread that puts the
typical scaled squared distance at ``u`` (0.01 .. 0.05: K is close to s 1 1^T, the last pivots of the sweep close to the noise); labels: one
draw from the GP itself, so that alpha, e and the weights have the sizes the model expects.  Rows >= n of Z and y hold finite JUNK.

Reference: oracle.gp_oracle.full_reference_quantities (+ predict) in float64 at the float32 phi, with the batch's float32 priors.
Error of output k: max |got - ref| / max |ref|.  Bound: 2 (S_k + R slack_k), where
  S_k      the largest change of output k of the reference, in the same measure, when ONE transformed hyper-parameter moves by +-4 float32
           ulps (six evaluations; the raw parameter moves by 4 2^-23 value / sigmoid(raw)).  The transformed hyper-parameters are the
           only float32 ingredient of the path (log1pf(expf(x)) at 1 ulp each, plus the added noise floor);
  R        2^-23: the output is rounded to float32 once - at most half an ulp of its largest element, doubled;
  slack_k  the cancellation slack of tests/_stress_oracle.py for f_out, grad_phi f_out and v (1 elsewhere).  It multiplies R alone: S_k is
           measured on the output itself and carries its own cancellation; what the slack stands for here is the one rounding of the
           INGREDIENTS that are outputs themselves (v = H^-1 g from the float32 H the caller gets);
  2        the margin for the device's float64 summation order (float64 round-off is 1e-9 below everything else here).

Nothing here may be modified by a test: cases and references are cached."""
import functools
import math

import numpy as np
import torch

from oracle import gp_oracle as O

R = 2.0 ** -23
ULPS = 4.0
JUNK_ZS, JUNK_YS, JUNK_ZQ, JUNK_YQ = 7.5, -3.0, -2.5, 9.0
THRESHOLD = 30.0                     # csrc/refine64.h R64_THRESHOLD
FLAG_MIN, UNFLAG_MAX = 60.0, 15.0    # a factor of two either side of it
RBF, MATERN = O.KERNEL_RBF, O.KERNEL_MATERN52

# task: (n, m, recipe, noise, lengthscale, u, flag).  recipe "cluster": see above; "pair": two points u apart in one dimension and one query
# next to them; "far": three support points 3 lengthscales apart, the queries clustered 2 lengthscales from the first; "control": standard
# normal features.  flag: "A" (flagged through the sweep of A), "S" (through Sigma_q alone) or None (stays on the float32 path).
CASES = {
    "tiny": dict(kernel=RBF, d=1, ld=(2, 1), tasks=[(2, 1, "pair", 0.003, 1.0, 1e-3, "A")]),
    "tiny_matern": dict(kernel=MATERN, d=1, ld=(2, 1), tasks=[(2, 1, "pair", 0.003, 0.7, 1e-3, "A")]),
    "odd": dict(kernel=MATERN, d=5, ld=(40, 24), tasks=[(33, 20, "cluster", 0.003, 1.3, 0.02, "A"), (32, 17, "cluster", 0.005, 0.8, 0.02, "A")]),
    "full": dict(kernel=RBF, d=3, ld=(128, 128), tasks=[(128, 128, "cluster", 0.01, 1.5, 0.02, "A")]),
    "wide_d": dict(kernel=RBF, d=130, ld=(33, 20), tasks=[(33, 20, "cluster", 0.003, 40.0, 0.02, "A"), (31, 20, "cluster", 0.005, 25.0, 0.02, "A")]),
    "leftover_a": dict(kernel=MATERN, d=5, ld=(130, 129), tasks=[(130, 129, "cluster", 0.01, 1.1, 0.02, "A")]),
    "leftover_b": dict(kernel=RBF, d=3, ld=(129, 20), tasks=[(129, 20, "cluster", 0.01, 0.9, 0.02, "A"), (127, 19, "cluster", 0.01, 2.0, 0.02, "A")]),
    "mixed_a": dict(kernel=RBF, d=3, ld=(128, 130), seed=3, tasks=[(128, 130, "cluster", 0.01, 0.8, 0.03, "A")]),
    "mixed_b": dict(kernel=MATERN, d=3, ld=(130, 20), tasks=[(130, 20, "cluster", 0.01, 1.7, 0.02, "A"), (100, 20, "cluster", 0.01, 0.6, 0.02, "A")]),
    "three_blocks": dict(kernel=MATERN, d=3, ld=(257, 3), tasks=[(257, 3, "cluster", 0.01, 1.4, 0.02, "A")]),
    "sigma_only": dict(kernel=RBF, d=2, ld=(3, 40), tasks=[(3, 40, "far", 0.01, 1.0, 0.02, "S")]),
    "neighbours_128": dict(kernel=RBF, d=3, ld=(64, 40), tasks=[(50, 40, "control", 0.1, 1.5, None, None), (64, 17, "cluster", 0.005, 1.2, 0.02, "A"),
                                                                (33, 30, "control", 0.1, 2.0, None, None)]),
    "neighbours_130": dict(kernel=MATERN, d=3, ld=(130, 33), tasks=[(100, 20, "control", 0.1, 1.5, None, None), (130, 33, "cluster", 0.01, 1.3, 0.02, "A"),
                                                                   (64, 7, "control", 0.1, 2.0, None, None)]),
    # the second flagged case of the shape of "odd" (the workspace-state test runs the two in turn on one workspace)
    "odd_twin": dict(kernel=MATERN, d=5, ld=(40, 24), tasks=[(33, 20, "cluster", 0.005, 0.9, 0.03, "A"), (32, 17, "cluster", 0.003, 1.6, 0.015, "A")]),
}
ACCURACY_CASES = [c for c in CASES if c != "odd_twin"]
ENTRY_CASES = ["odd", "wide_d", "leftover_a", "sigma_only"]
NEIGHBOUR_CASES = ["neighbours_128", "neighbours_130"]
IFT_KEYS = ("H", "f_out", "g_out", "v", "dZs_total", "dZq_total")
SLACK_KEYS = ("f_out", "g_out", "v")


def _raw(value):
    return float(O.inv_softplus(value))


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(Z_s [T, ld, d], y_s, Z_q, y_q, n_s, n_q, phi [T, 3], kernel, flags [T] (the tasks meant to take the float64 path in
    ift_hypergrad), flag_by): float32 tensors on the CPU."""
    spec = CASES[name]
    d, (ld, ldq), kind = spec["d"], spec["ld"], spec["kernel"]
    T = len(spec["tasks"])
    g = torch.Generator().manual_seed(6400 + 97 * sorted(CASES).index(name) + spec.get("seed", 0))
    Zs, ys = torch.full((T, ld, d), JUNK_ZS), torch.full((T, ld), JUNK_YS)
    Zq, yq = torch.full((T, ldq, d), JUNK_ZQ), torch.full((T, ldq), JUNK_YQ)
    phi = torch.zeros(T, 3)
    for t, (n, m, recipe, noise, ls, u, _) in enumerate(spec["tasks"]):
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        if recipe == "cluster":
            centre, spread = rn(d), ls * math.sqrt(u / (2.0 * d))
            zs, zq = centre + spread * rn(n, d), centre + spread * rn(m, d)
        elif recipe == "pair":
            x0 = rn(1)
            zs = torch.stack((x0, x0 + ls * math.sqrt(u)))
            zq = (x0 + 0.4 * ls * math.sqrt(u)).reshape(1, 1)
        elif recipe == "far":
            zs = 3.0 * ls * torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], dtype=torch.float64) + rn(d)
            zq = zs[0] + ls * torch.tensor([-1.4, -1.4], dtype=torch.float64) + ls * math.sqrt(u / (2.0 * d)) * rn(m, d)
        else:
            zs, zq = rn(n, d), rn(m, d)
        zs, zq = zs.float(), zq.float()
        phi[t] = torch.tensor([_raw(noise - O.NOISE_LOWER_BOUND), _raw(1.0), _raw(ls)])
        # the labels: one draw from the model at the float32 phi
        nz, os_, l_ = O.transform_phi(phi[t].double())
        zz = torch.cat((zs, zq)).double()
        K = O.kernel_matrix(zz, zz, os_, l_, kind) + nz * torch.eye(n + m, dtype=torch.float64)
        y = (torch.linalg.cholesky(K) @ rn(n + m)).float()
        Zs[t, :n], ys[t, :n], Zq[t, :m], yq[t, :m] = zs, y[:n], zq, y[n:]
    return dict(name=name, Z_s=Zs, y_s=ys, Z_q=Zq, y_q=yq, phi=phi, kernel=kind, d=d,
                n_s=tuple(s[0] for s in spec["tasks"]), n_q=tuple(s[1] for s in spec["tasks"]),
                flags=tuple(1 if s[6] else 0 for s in spec["tasks"]), flag_by=tuple(s[6] for s in spec["tasks"]))


def task_slices(c, t):
    """(zs, ys, zq, yq) of task t without the padding."""
    n, m = c["n_s"][t], c["n_q"][t]
    return c["Z_s"][t, :n].contiguous(), c["y_s"][t, :n].contiguous(), c["Z_q"][t, :m].contiguous(), c["y_q"][t, :m].contiguous()


def single_task(c, t):
    """Task t alone, at the padded sizes of its batch (a shallow case dict with T = 1)."""
    out = dict(c)
    for k in ("Z_s", "y_s", "Z_q", "y_q", "phi"):
        out[k] = c[k][t:t + 1].contiguous()
    for k in ("n_s", "n_q", "flags", "flag_by"):
        out[k] = c[k][t:t + 1]
    return out


def host_priors(name, t):
    """The priors adkf_init_params would fill in for task t (regression labels, lengthscale prior), restated on the CPU and rounded to
    float32: what the CPU checks use.  The GPU tests pass the batch's own priors, read back."""
    c = case(name)
    _, p = O.init_phi(task_slices(c, t)[0].double(), True, True)
    return tuple(float(np.float32(v)) for v in p.as_array())


# ---- conditioning -----------------------------------------------------------------------------------------------------------------------
def pivot_ratio(M):
    """max pivot / min pivot of the LDL^T factorisation of a float64 SPD matrix (the pivots of Gauss-Jordan without pivoting:
    csrc/refine64.h r64_inverse)."""
    piv = torch.diagonal(torch.linalg.cholesky(torch.as_tensor(M, dtype=torch.float64))) ** 2
    return float(piv.max() / piv.min())


@functools.lru_cache(maxsize=None)
def pivot_ratios(name, t):
    """(ratio of A, ratio of Sigma_q) of task t in float64."""
    c = case(name)
    zs, ys, zq, _ = task_slices(c, t)
    phi = c["phi"][t].double()
    noise, os_, ls = O.transform_phi(phi)
    A = O.kernel_matrix(zs.double(), zs.double(), os_, ls, c["kernel"]) + noise * torch.eye(zs.shape[0], dtype=torch.float64)
    _, cov = O.predict(zs.double(), ys.double(), zq.double(), phi, c["kernel"])
    return pivot_ratio(A), pivot_ratio(cov)


# ---- reference and bounds ---------------------------------------------------------------------------------------------------------------
def rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def combine(q, direct=True, correction=True):
    """dL/dZ_s and dL/dZ_q of a reference with the direct part and the correction part switched as ADKF_IGNORE_DIRECT_GRAD /
    ADKF_IGNORE_GRAD_CORRECTION switch them, and v (zero without the correction)."""
    dzs = (q["dZs_direct"] if direct else 0.0 * q["dZs_direct"]) - (q["mixed_Zs"] if correction else 0.0 * q["mixed_Zs"])
    dzq = q["dZq_direct"] if direct else 0.0 * q["dZq_direct"]
    return dzs, dzq, (q["v"] if correction else 0.0 * q["v"])


def _quantities(zs, ys, zq, yq, phi, pri, kind):
    q = O.full_reference_quantities(zs, ys, zq, yq, phi, O.Priors(*pri), kind)
    return {k: np.asarray(v) for k, v in q.items() if k != "l0"}


def _slack(q, m):
    """tests/_stress_oracle.py's cancellation slack: f_out against its three terms, grad_phi f_out against 1e-2 |f_out|, v against
    |H^-1|_inf times what grad_phi f_out is allowed."""
    g_floor = 1e-2 * abs(float(q["f_out"]))
    ld_q = float(np.linalg.slogdet(q["pred_cov"])[1])
    quad = 2.0 * float(q["f_out"]) - ld_q - m * O.LOG_2PI
    terms = 0.5 * (abs(quad) + abs(ld_q) + m * O.LOG_2PI)
    gmax = float(np.abs(q["g_out"]).max())
    return {"f_out": max(1.0, terms / abs(float(q["f_out"]))), "g_out": max(1.0, g_floor / gmax),
            "v": max(1.0, float(np.abs(np.linalg.inv(q["H"])).sum(1).max()) * max(g_floor, gmax) / float(np.abs(q["v"]).max()))}


@functools.lru_cache(maxsize=None)
def reference(name, t, pri=None):
    """dict(q: the float64 reference of task t at the float32 phi, moved: the six references with one transformed hyper-parameter 4 float32
    ulps off, slack).  pri: the four float32 priors of the task as a tuple (default: host_priors)."""
    c = case(name)
    pri = host_priors(name, t) if pri is None else tuple(float(v) for v in pri)
    zs, ys, zq, yq = task_slices(c, t)
    phi = c["phi"][t].double()
    q = _quantities(zs, ys, zq, yq, phi, pri, c["kernel"])
    values = [float(v) for v in O.transform_phi(phi)]
    moved = []
    for i in range(3):
        step = ULPS * R * values[i] / float(torch.sigmoid(phi[i]))
        for sign in (-1.0, 1.0):
            p = phi.clone()
            p[i] += sign * step
            moved.append(_quantities(zs, ys, zq, yq, p, pri, c["kernel"]))
    return dict(q=q, moved=moved, slack=_slack(q, zq.shape[0]), pri=pri)


def sensitivity(ref, key=None, fn=None):
    """S_k of an output (``key``) or of a function of the reference dict (``fn``: for the combinations of ``combine``)."""
    fn = fn or (lambda q: q[key])
    base = fn(ref["q"])
    return max(rel(fn(p), base) for p in ref["moved"])


def bound(ref, key, fn=None, slack_key=None):
    """2 (S_k + R slack_k): see the module docstring."""
    return 2.0 * (sensitivity(ref, key, fn) + R * ref["slack"].get(slack_key or key, 1.0))


def old_tolerance(ref, key):
    """What tests/test_gpu_stress.py holds the same output to."""
    return 1e-4 * ref["slack"].get(key, 1.0)


@functools.lru_cache(maxsize=None)
def float32_restatement_errors(name, t):
    """{output: error of the reference restated in float32} (O.DT = float32, as tests/_stress_oracle.py does): what a task left on a
    float32 path of the same formulas would show."""
    c = case(name)
    zs, ys, zq, yq = task_slices(c, t)
    ref = reference(name, t)
    O.DT = torch.float32
    try:
        q32 = _quantities(zs, ys, zq, yq, c["phi"][t], ref["pri"], c["kernel"])
    finally:
        O.DT = torch.float64
    return {k: rel(q32[k], ref["q"][k]) for k in IFT_KEYS + ("f_in", "g_in", "pred_mean")}


# ---- the float32 step adkf_predict keeps ------------------------------------------------------------------------------------------------
def _kappa32(kind, u):
    """kappa in float32, operation by operation as csrc/device_utils.h kappa0 does."""
    u = u.astype(np.float32)
    if kind == RBF:
        return np.exp(np.float32(-0.5) * u)
    r = np.sqrt(u)
    s5 = np.float32(2.23606797749979)
    return (np.float32(1.0) + s5 * r + np.float32(5.0 / 3.0) * u) * np.exp(-s5 * r)


def _gemm_d2(X, Y, mu):
    """|x|^2 + |y|^2 - 2 x.y of the centred rows in float32, clamped at zero: the float32 distance stage."""
    X, Y = X - mu, Y - mu
    nx, ny = (X * X).sum(1, dtype=np.float32), (Y * Y).sum(1, dtype=np.float32)
    return np.maximum((nx[:, None] + ny[None, :]) - np.float32(2) * (X @ Y.T), np.float32(0))


@functools.lru_cache(maxsize=None)
def predict_float32_step(name, t):
    """The part of adkf_predict that stays in float32 for a flagged task, applied to the float64 reference: level 1 of k_refine64 hands
    C = K_qs A^-1 back ROUNDED to float32 and the float32 kernels finish - k_predict (csrc/kernels.h): mean_i = sum_j C_ij y_j,
    var_i = s - sum_j C_ij s kappa(D2qs_ij / l^2) + noise, and ProbS for the covariance: K_qq + noise I - C K_sq, from the float32
    distances of the float32 stage.  Returns {pred_mean, pred_var, pred_cov: error of this emulation against the reference}."""
    c = case(name)
    zs, ys, zq, _ = task_slices(c, t)
    ref = reference(name, t)["q"]
    kind = c["kernel"]
    phi = c["phi"][t].double()
    noise, os_, ls = O.transform_phi(phi)
    A = O.kernel_matrix(zs.double(), zs.double(), os_, ls, kind) + noise * torch.eye(zs.shape[0], dtype=torch.float64)
    C32 = (O.kernel_matrix(zq.double(), zs.double(), os_, ls, kind) @ torch.linalg.inv(A)).numpy().astype(np.float32)
    f = lambda v: np.float32(float(v))
    noise, os_, ls = f(noise), f(os_), f(ls)
    il2 = np.float32(1.0) / (ls * ls)
    X, Q = zs.numpy(), zq.numpy()
    mu = X.astype(np.float64).mean(0).astype(np.float32)
    Kqs = os_ * _kappa32(kind, _gemm_d2(Q, X, mu) * il2)
    Kqq = os_ * _kappa32(kind, _gemm_d2(Q, Q, mu) * il2)
    mean = C32 @ ys.numpy()
    var = (os_ - (C32 * Kqs).sum(1, dtype=np.float32)) + noise
    cov = Kqq + noise * np.eye(Q.shape[0], dtype=np.float32) - C32 @ Kqs.T
    return {"pred_mean": rel(mean, ref["pred_mean"]), "pred_var": rel(var, ref["pred_var"]), "pred_cov": rel(cov, ref["pred_cov"])}
