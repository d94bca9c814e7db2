"""The float64 reference of adkf_predict_grad: torch.autograd through oracle.gp_oracle (kernel_matrix, transform_phi) of
sum(g_mean m + g_var v + g_ei E) with respect to the query rows - not a hand-written closed form, so a wrong sign or factor in the
library fails.  An ARD phi (raw noise, raw outputscale, d raw lengthscales) goes through the same code: transform_phi returns the d
lengthscales and kernel_matrix divides the features by them."""
import math

import numpy as np
import torch

TOL = 1e-4   # the project's bound: max |got - ref| <= TOL * max |ref| over a task's [rows_t, d] block


def rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def posterior(zs, ys, zq, phi, kind):
    """Mean [rows], LATENT variance [rows] and the outputscale of the rows zq (float64 tensors; differentiable in zq)."""
    from oracle import gp_oracle as O

    noise, os_, ls = O.transform_phi(phi)
    A = O.kernel_matrix(zs, zs, os_, ls, kind) + noise * torch.eye(zs.shape[0], dtype=torch.float64)
    L = torch.linalg.cholesky(A)
    alpha = torch.cholesky_solve(ys[:, None], L)[:, 0]
    K = O.kernel_matrix(zq, zs, os_, ls, kind)
    W = torch.linalg.solve_triangular(L, K.T, upper=False)
    return K @ alpha, os_ - (W * W).sum(0), os_


def acquisition(m, v, best, maximize, log_ei):
    """EI (log_ei: log EI) on the latent variance with the library's sigma = sqrt(max(v, 1e-12)) and u; returns (E, u)."""
    sigma = torch.sqrt(torch.clamp(v, min=1e-12))
    u = ((m - best) if maximize else (best - m)) / sigma
    if not log_ei:
        cdf = 0.5 * torch.erfc(-u / math.sqrt(2.0))
        pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        return sigma * (u * cdf + pdf), u
    # log h(u), h = phi + u Phi: directly for u > -1; below through erfcx, h = phi (1 - a sqrt(pi / 2) erfcx(a / sqrt 2)), a = -u (in
    # float64 the cancellation costs a^2 eps: 1e-13 at a = 25).  Each branch sees a harmless argument where the other one is taken.
    hi = u > -1.0
    u_hi = torch.where(hi, u, torch.zeros_like(u))
    a_lo = torch.where(hi, torch.ones_like(u), -u)
    lh_hi = torch.log(torch.exp(-0.5 * u_hi * u_hi) / math.sqrt(2.0 * math.pi) + u_hi * 0.5 * torch.erfc(-u_hi / math.sqrt(2.0)))
    lh_lo = (-0.5 * a_lo * a_lo - 0.5 * math.log(2.0 * math.pi)
             + torch.log(1.0 - a_lo * math.sqrt(math.pi / 2.0) * torch.special.erfcx(a_lo / math.sqrt(2.0))))
    return torch.log(sigma) + torch.where(hi, lh_hi, lh_lo), u


def predict_grad_ref(zs, ys, zq, phi, kind, g_mean=None, g_var=None, g_ei=None, best=None, maximize=False, log_ei=False):
    """d/dzq sum(g_mean m + g_var v + g_ei E) by autograd: (dZq [rows, d], m, v, u, os) as float64 numpy arrays (u: None without
    g_ei).  zs [n, d], ys [n], zq [rows, d], phi [3] or [2 + d]; the cotangents are [rows] arrays or None."""
    f64 = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64))
    zs, ys, phi = f64(zs), f64(ys), f64(phi)
    zq = f64(zq).clone().requires_grad_(True)
    m, v, os_ = posterior(zs, ys, zq, phi, kind)
    total = torch.zeros((), dtype=torch.float64)
    u = None
    if g_mean is not None:
        total = total + (f64(g_mean) * m).sum()
    if g_var is not None:
        total = total + (f64(g_var) * v).sum()
    if g_ei is not None:
        E, u = acquisition(m, v, float(best), maximize, log_ei)
        total = total + (f64(g_ei) * E).sum()
    (dz,) = torch.autograd.grad(total, zq)
    return dz.numpy(), m.detach().numpy(), v.detach().numpy(), None if u is None else u.detach().numpy(), float(os_)


# The cotangent sets every test walks: each cotangent alone, all together, EI and log EI, both senses.
COMBOS = [  # (name, uses g_mean, g_var, g_ei, maximize, log_ei)
    ("mean", True, False, False, False, False), ("var", False, True, False, False, False),
    ("ei-min", False, False, True, False, False), ("ei-max", False, False, True, True, False),
    ("logei-min", False, False, True, False, True), ("logei-max", False, False, True, True, True),
    ("all-ei-min", True, True, True, False, False), ("all-logei-max", True, True, True, True, True),
]


def cotangents(rows, seed):
    """Three seeded cotangent vectors [rows] of order one, none near zero (float32)."""
    g = np.random.default_rng(seed)
    return [(np.sign(g.standard_normal(rows)) * (0.5 + g.random(rows))).astype(np.float32) for _ in range(3)]
