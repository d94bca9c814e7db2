"""Batched GP operators on the HIP library: thin torch-tensor front end of include/adkf_gp.h.

All tensors live on one ROCm device, float32, contiguous.  Shapes: ``Z_s [T,N,d]``, ``y_s [T,N]``,
``Z_q [T,Nq,d]``, ``y_q [T,Nq]``, ``phi [T,h]`` (h = 3, or 2 + d for ``ard=True`` batches), ``priors [T,4]``,
optional ragged sizes ``n_s [T]``, ``n_q [T]`` (int32).  PyTorch is used for device memory and streams only; every number comes from the
hand-written kernels in ``csrc/``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import KERNEL_MATERN52, KERNEL_RBF, Batch, FitOptions, ptr, stream

KERNELS = {"rbf": KERNEL_RBF, "RBF": KERNEL_RBF, "matern": KERNEL_MATERN52}
REUSE_DIST = 1
REUSE_INNER = 2
LG_UNFUSED = 16     # blocked path: three launches per block step (A/B; include/adkf_gp.h)
LG_FUSED = 32       # ... the fused block step whatever the size
DZ_TILED = 64       # dL/dZ by the tiled launches whatever the shape (A/B; include/adkf_gp.h)
DEFER_REFINE = 8   # adkf_fit: leave the float64 re-evaluation of ill-conditioned tasks to the next call (include/adkf_gp.h)
ARD = 4


def kernel_id(kernel) -> int:
    if isinstance(kernel, int):
        return kernel
    if kernel not in KERNELS:
        # same message shape as fs_mol/utils/gp_utils.py:43; the other kernels of that file are out of scope
        raise ValueError("[ERROR] the kernel '" + str(kernel) + "' is not supported!")
    return KERNELS[kernel]


# SciPy's L-BFGS-B default ftol (factr * eps = 2.22e-9), which is what botorch's fit_gpytorch_scipy runs with
# (SURVEY App. A7).  On an fp32 objective of magnitude ~1 it means "stop when an accepted step does not lower f at all";
# 1e-7 (one ulp) looked equivalent and was not: it stopped fits that were still creeping along the lengthscale valley.
FTOL_DEFAULT = 2.22e-9


def _f32(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU: the GP path has no CPU fallback")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


@dataclass
class GPBatch:
    """A meta-batch of tasks in the library's layout."""

    Z_s: torch.Tensor
    y_s: torch.Tensor
    priors: torch.Tensor
    kernel: int = KERNEL_RBF
    Z_q: Optional[torch.Tensor] = None
    y_q: Optional[torch.Tensor] = None
    n_s: Optional[torch.Tensor] = None
    n_q: Optional[torch.Tensor] = None
    flags: int = 0  # REUSE_DIST / REUSE_INNER promises for consecutive calls on this batch (include/adkf_gp.h)
    ard: bool = False  # one lengthscale per feature dimension: phi has 2 + d entries per task (ADKF_BATCH_ARD)

    def __post_init__(self):
        self.kernel = kernel_id(self.kernel)
        self.Z_s = _f32(self.Z_s, "Z_s")
        self.y_s = _f32(self.y_s, "y_s")
        self.priors = _f32(self.priors, "priors")
        self.Z_q = _f32(self.Z_q, "Z_q")
        self.y_q = _f32(self.y_q, "y_q")
        if self.Z_s.dim() != 3:
            raise ValueError("Z_s must be [T, N, d]")
        T, N, d = self.Z_s.shape
        # The library trusts the sizes of adkf_batch_t: every tensor is checked against them HERE (a [T, 3] phi on an ARD
        # batch, or labels of another meta-batch, would otherwise be read and written out of bounds on the device).
        if tuple(self.y_s.shape) != (T, N):
            raise ValueError(f"y_s must be [T, N] = [{T}, {N}], got {tuple(self.y_s.shape)}")
        if tuple(self.priors.shape) != (T, 4):
            raise ValueError(f"priors must be [T, 4] = [{T}, 4], got {tuple(self.priors.shape)}")
        if (self.Z_q is None) != (self.y_q is None) and self.Z_q is None:
            raise ValueError("y_q given without Z_q")
        if self.Z_q is not None:
            if self.Z_q.dim() != 3 or self.Z_q.shape[0] != T or self.Z_q.shape[2] != d:
                raise ValueError(f"Z_q must be [T, N_q, d] = [{T}, N_q, {d}], got {tuple(self.Z_q.shape)}")
            if self.y_q is not None and tuple(self.y_q.shape) != tuple(self.Z_q.shape[:2]):
                raise ValueError(f"y_q must be [T, N_q] = {tuple(self.Z_q.shape[:2])}, got {tuple(self.y_q.shape)}")
        for name, limit in (("n_s", N), ("n_q", self.nq)):
            v = getattr(self, name)
            if v is not None:
                if v.numel() != T:
                    raise ValueError(f"{name} must have T = {T} entries, got {v.numel()}")
                if not v.is_cuda:     # host-side sizes can be range-checked without a device synchronisation
                    lo, hi = int(v.min()), int(v.max())
                    if lo < (1 if name == "n_s" else 0) or hi > limit:
                        raise ValueError(f"{name} out of range: [{lo}, {hi}] for a padded size of {limit}")
                setattr(self, name, v.to(device=self.Z_s.device, dtype=torch.int32).contiguous().view(T))
        for name in ("y_s", "priors", "Z_q", "y_q"):
            v = getattr(self, name)
            if v is not None and v.device != self.Z_s.device:
                raise ValueError(f"{name} lives on {v.device}, Z_s on {self.Z_s.device}: one batch, one device")
        self._ws = None

    @property
    def T(self):
        return self.Z_s.shape[0]

    @property
    def ns(self):
        return self.Z_s.shape[1]

    @property
    def nq(self):
        return 0 if self.Z_q is None else self.Z_q.shape[1]

    @property
    def d(self):
        return self.Z_s.shape[2]

    @property
    def device(self):
        return self.Z_s.device

    @property
    def h(self):
        return 2 + self.d if self.ard else 3

    def c_struct(self) -> Batch:
        b = Batch()
        flags = int(self.flags) | (ARD if self.ard else 0)
        b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = self.T, self.ns, self.nq, self.d, self.kernel, flags
        b.n_s, b.n_q = ptr(self.n_s), ptr(self.n_q)
        b.Z_s, b.y_s, b.Z_q, b.y_q, b.priors = ptr(self.Z_s), ptr(self.y_s), ptr(self.Z_q), ptr(self.y_q), ptr(self.priors)
        return b

    def workspace(self) -> Tuple[torch.Tensor, int]:
        """The caller-owned workspace of THIS batch.  It belongs to the batch object (not to a per-stream cache) because
        the REUSE_DIST / REUSE_INNER promises refer to what earlier calls on this batch left in it; torch's caching allocator
        makes the per-batch allocation cheap."""
        lib = _lib.load()
        need = (lib.adkf_workspace_bytes_ard if self.ard else lib.adkf_workspace_bytes)(self.T, self.ns, self.nq, self.d)
        if self._ws is None or self._ws.numel() < need:
            if self._ws is not None and (self.flags & (REUSE_DIST | REUSE_INNER)):
                raise RuntimeError("the workspace of this batch would have to grow while REUSE flags are set: the data they refer to would be lost")
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws, need

    def check_phi(self, phi: torch.Tensor, name: str = "phi") -> torch.Tensor:
        phi = _f32(phi, name)
        if tuple(phi.shape) != (self.T, self.h):
            raise ValueError(f"{name} must be [T, h] = [{self.T}, {self.h}] for this batch, got {tuple(phi.shape)}")
        if phi.device != self.device:
            raise ValueError(f"{name} lives on {phi.device}, the batch on {self.device}")
        return phi


def _new(b: GPBatch, *shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=b.device)


def check_info(info: torch.Tensor, what: str = "GP factorisation"):
    """Raises like gpytorch's NotPSDError would in the reference (SURVEY 8b error convention)."""
    lib = _lib.load()
    rc = lib.adkf_check_info(ptr(info), info.numel(), stream(info.device))
    if rc > 0:
        code = int(info[rc - 1].item())
        if code >= 200000:   # ADKF_INFO_CG_BASE
            raise RuntimeError(f"{what}: conjugate gradients met non-positive curvature for task {rc - 1} at iteration "
                               f"{code - 200000}: the inner Hessian is not positive definite (is the inner fit converged?)")
        where = "predictive covariance" if code >= _lib.INFO_OUTER_BASE else "K + noise*I"
        raise RuntimeError(f"{what}: matrix not positive definite for task {rc - 1} ({where}, pivot {code % _lib.INFO_OUTER_BASE})")
    if rc < 0:
        _lib.check(rc, "adkf_check_info")


def median_lengthscale(b: GPBatch) -> torch.Tensor:
    lib = _lib.load()
    l0 = _new(b, b.T)
    ws, nb = b.workspace()
    cb = b.c_struct()
    _lib.check(lib.adkf_median_lengthscale(C.byref(cb), ptr(l0), ptr(ws), nb, stream(b.device)), "adkf_median_lengthscale")
    return l0


def init_params(Z_s: torch.Tensor, use_numeric_labels: bool = False, use_lengthscale_prior: bool = True,
                n_s: Optional[torch.Tensor] = None):
    """Returns (phi [T,3], priors [T,4], l0 [T]) exactly as ``reinit_gp_params`` would initialise every task."""
    lib = _lib.load()
    Z_s = _f32(Z_s, "Z_s")
    dummy = torch.zeros(Z_s.shape[0], 4, device=Z_s.device)
    b = GPBatch(Z_s, torch.zeros(Z_s.shape[:2], device=Z_s.device), dummy, KERNEL_RBF, n_s=n_s)
    phi, priors, l0 = _new(b, b.T, 3), _new(b, b.T, 4), _new(b, b.T)
    ws, nb = b.workspace()
    cb = b.c_struct()
    _lib.check(lib.adkf_init_params(C.byref(cb), int(use_numeric_labels), int(use_lengthscale_prior), ptr(phi),
                                    ptr(priors), ptr(l0), ptr(ws), nb, stream(b.device)), "adkf_init_params")
    return phi, priors, l0


def init_params_batch(b: GPBatch, use_numeric_labels: bool = False, use_lengthscale_prior: bool = True):
    """Like ``init_params`` but on an existing batch: fills ``b.priors`` in place and returns (phi0, l0).  The
    squared distances it computes stay in the workspace, so the caller may set ``b.flags |= REUSE_DIST`` for the
    following ``fit`` / ``ift_hypergrad`` calls on the same batch."""
    lib = _lib.load()
    phi, l0 = _new(b, b.T, b.h), _new(b, b.T)
    ws, nb = b.workspace()
    cb = b.c_struct()
    _lib.check(lib.adkf_init_params(C.byref(cb), int(use_numeric_labels), int(use_lengthscale_prior), ptr(phi),
                                    ptr(b.priors), ptr(l0), ptr(ws), nb, stream(b.device)), "adkf_init_params")
    return phi, l0


def mll_value_grad(b: GPBatch, phi: torch.Tensor, want_grad_phi=True, want_dZ=False):
    lib = _lib.load()
    phi = b.check_phi(phi)
    f = _new(b, b.T)
    g = _new(b, b.T, b.h) if want_grad_phi else None
    dZ = _new(b, b.T, b.ns, b.d) if want_dZ else None
    info = _new(b, b.T, dtype=torch.int32)
    ws, nb = b.workspace()
    cb = b.c_struct()
    _lib.check(lib.adkf_mll_value_grad(C.byref(cb), ptr(phi), ptr(f), ptr(g), ptr(dZ), ptr(info), ptr(ws), nb,
                                       stream(b.device)), "adkf_mll_value_grad")
    return f, g, dZ, info


def fit(b: GPBatch, phi0: torch.Tensor, max_evals: int = 200, gtol: float = 1e-5, ftol: float = FTOL_DEFAULT,
        exact_evals: bool = False, events: Optional[Tuple[torch.cuda.Event, torch.cuda.Event]] = None,
        inplace: bool = False):
    """Batched inner optimisation; returns (phi*, f_final, gnorm, n_evals, info).  ``events`` = a pair of
    already-created timing events recorded right around the optimiser kernel (bench.py's roofline clock).
    ``inplace``: the library optimises ``phi0`` where it lies (the meta-step's freshly initialised parameters have no
    other reader: one copy kernel less per step); otherwise ``phi0`` is left untouched."""
    lib = _lib.load()
    phi = b.check_phi(phi0, "phi0")
    if not inplace:
        phi = phi.clone()
    f, gn = _new(b, b.T), _new(b, b.T)
    ne, info = _new(b, b.T, dtype=torch.int32), _new(b, b.T, dtype=torch.int32)
    opt = FitOptions(int(max_evals), int(exact_evals), float(gtol), float(ftol),
                     events[0].cuda_event if events else None, events[1].cuda_event if events else None)
    ws, nb = b.workspace()
    cb = b.c_struct()
    _lib.check(lib.adkf_fit(C.byref(cb), ptr(phi), C.byref(opt), ptr(f), ptr(gn), ptr(ne), ptr(info), ptr(ws), nb,
                            stream(b.device)), "adkf_fit")
    return phi, f, gn, ne, info


def predict(b: GPBatch, phi: torch.Tensor, want_var=True, want_cov=False):
    lib = _lib.load()
    phi = b.check_phi(phi)
    mean = _new(b, b.T, b.nq)
    var = _new(b, b.T, b.nq) if want_var else None
    cov = _new(b, b.T, b.nq, b.nq) if want_cov else None
    info = _new(b, b.T, dtype=torch.int32)
    ws, nb = b.workspace()
    cb = b.c_struct()
    _lib.check(lib.adkf_predict(C.byref(cb), ptr(phi), ptr(mean), ptr(var), ptr(cov), ptr(info), ptr(ws), nb,
                                stream(b.device)), "adkf_predict")
    return mean, var, cov, info


def pack_rows(Z_q: torch.Tensor, n_q: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Padded query rows ``Z_q [T, Nq, d]`` (true sizes ``n_q [T]``, default all ``Nq``) -> packed ``Zq [rows, d]`` and the row
    offsets ``q_off [T + 1]`` (int64: task t owns rows ``q_off[t]:q_off[t+1]``), on ``Z_q``'s device.  Pure torch; runs on
    CPU tensors too."""
    if Z_q.dim() != 3:
        raise ValueError("Z_q must be [T, N_q, d]")
    T, nq, d = Z_q.shape
    if n_q is None:
        n = torch.full((T,), nq, dtype=torch.int64, device=Z_q.device)
    else:
        n = n_q.to(device=Z_q.device, dtype=torch.int64).reshape(T).clamp(0, nq)
    q_off = torch.zeros(T + 1, dtype=torch.int64, device=Z_q.device)
    q_off[1:] = torch.cumsum(n, 0)
    mask = torch.arange(nq, device=Z_q.device)[None, :] < n[:, None]
    return Z_q[mask].reshape(-1, d).contiguous(), q_off


def unpack_rows(x: torch.Tensor, q_off: torch.Tensor, nq: int) -> torch.Tensor:
    """Per-row results ``x [rows]`` -> ``[T, nq]`` (zeros in the padding): the inverse of ``pack_rows`` for outputs."""
    T = q_off.numel() - 1
    n = (q_off[1:] - q_off[:-1]).to(x.device)
    out = torch.zeros(T, nq, dtype=x.dtype, device=x.device)
    mask = torch.arange(nq, device=x.device)[None, :] < n[:, None]
    out[mask] = x
    return out


def predict_marginal(b: GPBatch, phi: torch.Tensor, Zq: torch.Tensor, q_off: torch.Tensor, latent: bool = False,
                     best_f: Optional[torch.Tensor] = None, maximize: bool = False, want_var: bool = True, log_ei: bool = False):
    """Marginal posterior of packed query rows (``pack_rows``) against the support set of ``b`` (which carries no query set):
    returns (mean [rows], var [rows] or None, ei [rows] or None, info [T]).  ``var`` includes the observation noise unless
    ``latent``; ``ei`` (only with ``best_f [T]``) is Expected Improvement on the latent variance, for minimisation unless
    ``maximize``.  With ``log_ei`` (needs ``best_f``) ``ei`` holds log EI instead, evaluated without forming EI: finite where
    float32 EI underflows to 0 (from about 14 posterior standard deviations short of ``best_f``); rows the call leaves at 0 stay 0.
    No size cap and a workspace independent of the number of rows (include/adkf_gp.h).  ARD batches (``phi``
    [T, 2 + d]) go through ``adkf_predict_marginal_ard``."""
    lib = _lib.load()
    if log_ei and best_f is None:
        raise ValueError("log_ei needs best_f [T]")
    if b.nq != 0:
        raise ValueError("predict_marginal takes a support-only batch (no Z_q / y_q): the query rows come packed in Zq")
    phi = b.check_phi(phi)
    Zq = _f32(Zq, "Zq")
    if Zq.dim() != 2 or Zq.shape[1] != b.d:
        raise ValueError(f"Zq must be [rows, d] = [rows, {b.d}], got {tuple(Zq.shape)}")
    if not q_off.is_cuda or q_off.dtype != torch.int64 or q_off.numel() != b.T + 1:
        raise ValueError(f"q_off must be int64 [T + 1] = [{b.T + 1}] on the GPU")
    q_off = q_off.contiguous()
    if best_f is not None:
        best_f = _f32(best_f, "best_f").reshape(-1)
        if best_f.numel() != b.T:
            raise ValueError(f"best_f must have T = {b.T} entries")
    for name, t in (("Zq", Zq), ("q_off", q_off), ("best_f", best_f)):
        if t is not None and t.device != b.device:
            raise ValueError(f"{name} lives on {t.device}, the batch on {b.device}")
    rows = Zq.shape[0]
    mean = _new(b, rows)
    var = _new(b, rows) if want_var else None
    ei = _new(b, rows) if best_f is not None else None
    info = _new(b, b.T, dtype=torch.int32)
    flags = (_lib.PM_LATENT if latent else 0) | (_lib.PM_MAXIMIZE if maximize else 0) | (_lib.PM_LOG_EI if log_ei else 0)
    ws, nb = b.workspace()
    cb = b.c_struct()
    name = "adkf_predict_marginal_ard" if b.ard else "adkf_predict_marginal"
    _lib.check(getattr(lib, name)(C.byref(cb), ptr(phi), flags, ptr(Zq), ptr(q_off), rows, ptr(best_f), ptr(mean), ptr(var),
                                  ptr(ei), ptr(info), ptr(ws), nb, stream(b.device)), name)
    return mean, var, ei, info


def predict_grad(b: GPBatch, phi: torch.Tensor, Zq: torch.Tensor, q_off: torch.Tensor, *, g_mean: Optional[torch.Tensor] = None,
                 g_var: Optional[torch.Tensor] = None, g_ei: Optional[torch.Tensor] = None, best_f: Optional[torch.Tensor] = None,
                 maximize: bool = False, log_ei: bool = False):
    """The vector-Jacobian product of ``predict_marginal`` with respect to the packed query rows, in one ``adkf_predict_grad`` call:
    returns (dZq [rows, d], info [T]) with ``dZq[r] = d/dZq[r] (g_mean[r] mean[r] + g_var[r] var[r] + g_ei[r] ei[r])``.  The
    cotangents are ``[rows]`` each and at least one must be given; ``g_ei`` needs ``best_f [T]`` and is the cotangent of log EI with
    ``log_ei`` (``maximize`` as in ``predict_marginal``; the noise is a constant, so ``latent`` would change nothing and is not an
    argument).  The support set and ``phi`` are constants of the call.  Rows of no task's range, and rows of tasks with no support
    points or ``info != 0``, get 0.  Autograd-free, like the rest of this module (``models.predict_marginal_diff`` is the bridge).
    Isotropic and ARD batches alike."""
    lib = _lib.load()
    if g_mean is None and g_var is None and g_ei is None:
        raise ValueError("predict_grad needs at least one of g_mean, g_var, g_ei")
    if g_ei is not None and best_f is None:
        raise ValueError("g_ei needs best_f [T]")
    if log_ei and g_ei is None:
        raise ValueError("log_ei needs g_ei (the cotangent of log EI)")
    if b.nq != 0:
        raise ValueError("predict_grad takes a support-only batch (no Z_q / y_q): the query rows come packed in Zq")
    phi = b.check_phi(phi)
    Zq = _f32(Zq, "Zq")
    if Zq.dim() != 2 or Zq.shape[1] != b.d:
        raise ValueError(f"Zq must be [rows, d] = [rows, {b.d}], got {tuple(Zq.shape)}")
    if not q_off.is_cuda or q_off.dtype != torch.int64 or q_off.numel() != b.T + 1:
        raise ValueError(f"q_off must be int64 [T + 1] = [{b.T + 1}] on the GPU")
    q_off = q_off.contiguous()
    rows = Zq.shape[0]
    cot = {}
    for name, t in (("g_mean", g_mean), ("g_var", g_var), ("g_ei", g_ei)):
        if t is not None:
            t = _f32(t, name).reshape(-1)
            if t.numel() != rows:
                raise ValueError(f"{name} must have rows = {rows} entries, got {t.numel()}")
        cot[name] = t
    if best_f is not None:
        best_f = _f32(best_f, "best_f").reshape(-1)
        if best_f.numel() != b.T:
            raise ValueError(f"best_f must have T = {b.T} entries")
    for name, t in (("Zq", Zq), ("q_off", q_off), ("best_f", best_f), *cot.items()):
        if t is not None and t.device != b.device:
            raise ValueError(f"{name} lives on {t.device}, the batch on {b.device}")
    dZq = _new(b, rows, b.d)
    info = _new(b, b.T, dtype=torch.int32)
    flags = (_lib.PM_MAXIMIZE if maximize else 0) | (_lib.PM_LOG_EI if log_ei else 0)
    ws, nb = b.workspace()
    cb = b.c_struct()
    _lib.check(lib.adkf_predict_grad(C.byref(cb), ptr(phi), flags, ptr(Zq), ptr(q_off), rows, ptr(best_f), ptr(cot["g_mean"]),
                                     ptr(cot["g_var"]), ptr(cot["g_ei"]), ptr(dZq), ptr(info), ptr(ws), nb, stream(b.device)),
               "adkf_predict_grad")
    return dZq, info


def pack_exclude(exclude, T: int, rows: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exclusion lists of ``predict_pool`` in the library's layout: ``(excl_idx, excl_off)``, both int64, task t's rows in
    ``excl_idx[excl_off[t]:excl_off[t + 1]]`` sorted ascending, without duplicates or entries outside ``[0, rows)``.
    ``exclude``: None, a list of T index tensors / lists / None, or an ``(excl_idx, excl_off)`` pair (normalised in the same
    way).  Pure torch; runs on CPU tensors too."""
    if exclude is None:
        exclude = [None] * T
    elif (isinstance(exclude, tuple) and len(exclude) == 2 and torch.is_tensor(exclude[1]) and exclude[1].numel() == T + 1
          and torch.is_tensor(exclude[0]) and exclude[0].dim() == 1):
        idx, off = exclude[0], [int(o) for o in exclude[1].tolist()]
        exclude = [idx[off[t]:off[t + 1]] for t in range(T)]
    if len(exclude) != T:
        raise ValueError(f"exclude must hold one index list per task: T = {T}, got {len(exclude)}")
    parts = []
    for e in exclude:
        e = torch.empty(0, dtype=torch.int64) if e is None else torch.as_tensor(e).to(torch.int64).reshape(-1)
        if device is not None:
            e = e.to(device)
        parts.append(torch.unique(e[(e >= 0) & (e < rows)]))   # (sorted)
    dev = device if device is not None else (parts[0].device if parts else "cpu")
    off = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    if parts:
        off[1:] = torch.cumsum(torch.tensor([q.numel() for q in parts], dtype=torch.int64, device=dev), 0)
    idx = torch.cat([q.to(dev) for q in parts]) if parts else torch.empty(0, dtype=torch.int64, device=dev)
    return idx.contiguous(), off


def _support_only(b, name: str) -> None:
    if b.nq != 0:
        raise ValueError(f"{name} takes a support-only batch (no Z_q / y_q): the pool comes in X")


def _in_range(value, lo: int, hi: int, what: str) -> int:
    value = int(value)
    if value < lo or value > hi:
        raise ValueError(f"{what} must be in [{lo}, {hi}], got {value}")
    return value


def _phi_and_pool(b, phi, X):
    """``phi`` as the batch takes it and the pool ``X`` as float32 ``[rows, d]``."""
    phi = b.check_phi(phi)
    X = _f32(X, "X")
    if X.dim() != 2 or X.shape[1] != b.d:
        raise ValueError(f"X must be [rows, d] = [rows, {b.d}], got {tuple(X.shape)}")
    return phi, X


def _on_device(b, **tensors) -> None:
    for name, t in tensors.items():
        if t is not None and t.device != b.device:
            raise ValueError(f"{name} lives on {t.device}, the batch on {b.device}")


def _sample_table(b, t, name: str, what: str) -> int:
    """S of a table of samples ``[T, S]``, S at most 64 (``what``: what the S entries are)."""
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != b.T:
        raise ValueError(f"{name} must be a tensor [T, S] = [{b.T}, S], got {tuple(t.shape) if torch.is_tensor(t) else t!r}")
    return _in_range(t.shape[1], 1, _lib.TS_SAMPLES_MAX, what)


def _exclusion(b, exclude, n: int, rows: int):
    """``(excl_idx, excl_off)`` of ``n`` lists on the batch's device, ``(None, None)`` without ``exclude``."""
    return (None, None) if exclude is None else pack_exclude(exclude, n, rows, b.device)


def _selection(b, n: int, topk: int):
    """The outputs of a selection of ``topk`` rows for each of ``n`` lists: ``(top_idx, top_val, info)``."""
    top_idx = _new(b, n, topk, dtype=torch.int64) if topk > 0 else None
    top_val = _new(b, n, topk) if topk > 0 else None
    return top_idx, top_val, _new(b, b.T, dtype=torch.int32)


def _pool_call(lib, entry: str, b, phi, flags: int, X, args, info, scratch_bytes: int) -> None:
    """One pool entry of the library: ``args`` are the entry's own, between ``rows`` and ``info``."""
    sb = int(scratch_bytes)
    scratch = torch.empty(sb, dtype=torch.uint8, device=b.device) if sb else None
    ws, nb = b.workspace()
    cb = b.c_struct()
    _lib.check(getattr(lib, entry)(C.byref(cb), ptr(phi), flags, ptr(X), X.shape[0], *args, ptr(info), ptr(ws), nb, ptr(scratch), sb,
                                   stream(b.device)), entry)


def predict_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, latent: bool = False, best_f: Optional[torch.Tensor] = None,
                 maximize: bool = False, score: str = "ei", want_mean: bool = True, want_var: bool = True,
                 want_ei: Optional[bool] = None, topk: int = 0, exclude=None, log_ei: bool = False):
    """Every task of the support-only batch ``b`` scores the SAME pool ``X [rows, d]`` in one ``adkf_predict_pool`` call.
    Returns ``dict(mean, var, ei, top_idx, top_val, info)``: the per-row outputs asked for as ``[T, rows]`` tensors (None
    otherwise; ``want_ei`` defaults to "``best_f`` given"), ``top_idx [T, topk]`` (int64) / ``top_val [T, topk]`` - each task's
    ``topk`` (at most 64) rows of largest score, descending, equal scores by ascending row, -1 / -inf where fewer are eligible -
    and ``info [T]``.  ``score``: ``"ei"`` (needs ``best_f``) or ``"mean"`` (+mean with ``maximize``, -mean without).
    ``log_ei``: ``ei`` and the ``"ei"`` score (hence ``top_val``) are log EI, which keeps an order where float32 EI is 0 on every
    row; it needs something that reads it (``want_ei``, or ``topk > 0`` with ``score="ei"``).
    ``exclude``: rows a task may not select (``pack_exclude``).  With no per-row output and ``topk > 0`` nothing of size
    T x rows is allocated or written."""
    lib = _lib.load()
    _support_only(b, "predict_pool")
    if score not in ("ei", "mean"):
        raise ValueError(f"score must be 'ei' or 'mean', got {score!r}")
    topk = _in_range(topk, 0, _lib.POOL_TOPK_MAX, "topk")
    phi, X = _phi_and_pool(b, phi, X)
    if best_f is not None:
        best_f = _f32(best_f, "best_f").reshape(-1)
        if best_f.numel() != b.T:
            raise ValueError(f"best_f must have T = {b.T} entries")
    if want_ei is None:
        want_ei = best_f is not None
    if (want_ei or (topk > 0 and score == "ei")) and best_f is None:
        raise ValueError("ei and ranking by ei need best_f [T]")
    if not (want_mean or want_var or want_ei or topk > 0):
        raise ValueError("no output asked for")
    if log_ei and not (want_ei or (topk > 0 and score == "ei")):
        raise ValueError("log_ei without want_ei or a selection ranked by ei: nothing would read it")
    rows = X.shape[0]
    excl_idx, excl_off = _exclusion(b, exclude if topk > 0 else None, b.T, rows)
    _on_device(b, X=X, best_f=best_f)
    mean = _new(b, b.T, rows) if want_mean else None
    var = _new(b, b.T, rows) if want_var else None
    ei = _new(b, b.T, rows) if want_ei else None
    top_idx, top_val, info = _selection(b, b.T, topk)
    flags = (_lib.PM_LATENT if latent else 0) | (_lib.PM_MAXIMIZE if maximize else 0) | (_lib.PM_SCORE_MEAN if score == "mean" else 0)
    flags |= _lib.PM_LOG_EI if log_ei else 0
    args = (ptr(best_f), ptr(excl_idx), ptr(excl_off), ptr(mean), ptr(var), ptr(ei), topk, ptr(top_idx), ptr(top_val))
    _pool_call(lib, "adkf_predict_pool", b, phi, flags, X, args, info, lib.adkf_predict_pool_scratch_bytes(b.T, topk))
    return dict(mean=mean, var=var, ei=ei, top_idx=top_idx, top_val=top_val, info=info)


def _believer_pool(name: str, b: GPBatch, phi, X, best_f, q, maximize, log_ei, exclude, want_trace):
    """The body of ``believer_pool`` (``name = "believer_pool"``, isotropic batches) and ``believer_pool_ard`` (ARD batches)."""
    lib = _lib.load()
    ard = name == "believer_pool_ard"
    _support_only(b, name)
    if b.ard and not ard:
        raise ValueError("believer_pool does not support ARD batches: use believer_pool_ard")
    if ard and not b.ard:
        raise ValueError("believer_pool_ard takes an ARD batch (GPBatch(..., ard=True)): use believer_pool")
    q = _in_range(q, 1, _lib.POOL_TOPK_MAX, "q")
    phi, X = _phi_and_pool(b, phi, X)
    if best_f is None:
        raise ValueError(f"{name} needs best_f [T]")
    best_f = _f32(best_f, "best_f").reshape(-1)
    if best_f.numel() != b.T:
        raise ValueError(f"best_f must have T = {b.T} entries")
    rows = X.shape[0]
    _on_device(b, X=X, best_f=best_f)
    excl_idx, excl_off = _exclusion(b, exclude, b.T, rows)
    sel_idx, sel_val, info = _selection(b, b.T, q)
    sel_mean, sel_var = _new(b, b.T, q), _new(b, b.T, q)
    trace = _new(b, b.T, q, rows) if want_trace else None
    flags = (_lib.PM_MAXIMIZE if maximize else 0) | (_lib.PM_LOG_EI if log_ei else 0)
    args = (ptr(best_f), ptr(excl_idx), ptr(excl_off), q, ptr(trace), ptr(sel_idx), ptr(sel_val), ptr(sel_mean), ptr(sel_var))
    _pool_call(lib, "adkf_" + name, b, phi, flags, X, args, info, lib.adkf_believer_pool_scratch_bytes(b.T, b.ns, b.d, q))
    return dict(sel_idx=sel_idx, sel_val=sel_val, sel_mean=sel_mean, sel_var=sel_var, trace=trace, info=info)


def believer_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, best_f: torch.Tensor, q: int, maximize: bool = False,
                  log_ei: bool = False, exclude=None, want_trace: bool = False):
    """A Kriging-believer batch per task from the shared pool ``X [rows, d]`` in one ``adkf_believer_pool`` call: ``q`` (at most
    64) sequential-greedy EI picks, each believed at its posterior mean, so that a pick lowers the variance - hence the EI - of its
    neighbours and moves the incumbent before the next one is chosen.  Step 0 is ``predict_pool(topk=1)``.  Returns
    ``dict(sel_idx, sel_val, sel_mean, sel_var, trace, info)``: ``sel_idx [T, q]`` (int64) the picks in pick order and
    ``sel_val`` their scores (EI, or log EI with ``log_ei``) at the step they were picked, -1 / -inf from the step at which no
    eligible row was left; ``sel_mean`` the believed values, ``sel_var`` the latent variance each pick had when it was picked;
    ``trace [T, q, rows]`` (``want_trace``, else None) the score of every row at every step; ``info [T]``.  ``exclude``: rows a
    task may not select (``pack_exclude``).  ARD batches go to ``believer_pool_ard``."""
    return _believer_pool("believer_pool", b, phi, X, best_f, q, maximize, log_ei, exclude, want_trace)


def believer_pool_ard(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, best_f: torch.Tensor, q: int, maximize: bool = False,
                      log_ei: bool = False, exclude=None, want_trace: bool = False):
    """``believer_pool`` for ARD batches (``phi [T, 2 + d]``) in one ``adkf_believer_pool_ard`` call: the same picks on the scaled
    features ``(x - mu) / l`` with one lengthscale per feature dimension.  Step 0 is ``predict_pool(topk=1)`` on the same ARD
    batch; arguments and the returned dict are those of ``believer_pool``.  Raises ``ValueError`` for a batch that is not an ARD
    batch."""
    return _believer_pool("believer_pool_ard", b, phi, X, best_f, q, maximize, log_ei, exclude, want_trace)


def liar_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, best_f: torch.Tensor, q: int, lie=None, labels: Optional[torch.Tensor] = None,
              maximize: bool = False, log_ei: bool = False, exclude=None, want_trace: bool = False):
    """A constant-liar or label-replay batch per task from the shared pool ``X [rows, d]`` in one ``adkf_liar_pool`` call, for
    isotropic and ARD batches alike: ``believer_pool`` with the believed value supplied.  ``q`` (at most 64) sequential-greedy EI
    picks; each pick is conditioned as a noisy observation on the first finite value of its entry in ``labels`` (``[rows]``, one
    table for all tasks, or ``[T, rows]``), the task's ``lie`` and its own posterior mean - so the posterior MEAN moves inside the
    call, as well as the variance and the incumbent.  ``lie``: a tensor ``[T]``, or ``"min"`` / ``"max"`` / ``"mean"`` of each
    task's own support labels (maximising, CL-min explores harder than the believer and CL-max stays on its peak; minimising swaps
    the two: Ginsbourger et al. 2010).  With
    ``labels`` the call plays ``q`` iterations of a replay at fixed ``phi`` (BoTorch's ``condition_on_observations``).  At least
    one of ``lie`` and ``labels``.  Returns ``believer_pool``'s dict - ``sel_mean`` / ``sel_var`` the conditioned mean and latent
    variance each pick had when it was picked - plus ``sel_lie [T, q]``, the value each pick was conditioned on (0 where there was
    no pick), and ``inc [T, q + 1]``, the incumbent before step 0 and after every step."""
    lib = _lib.load()
    _support_only(b, "liar_pool")
    q = _in_range(q, 1, _lib.POOL_TOPK_MAX, "q")
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    if best_f is None:
        raise ValueError("liar_pool needs best_f [T]")
    best_f = _f32(best_f, "best_f").reshape(-1)
    if best_f.numel() != b.T:
        raise ValueError(f"best_f must have T = {b.T} entries")
    if lie is None and labels is None:
        raise ValueError("liar_pool needs lie or labels: without either it is believer_pool")
    if isinstance(lie, str):
        if lie not in ("min", "max", "mean"):
            raise ValueError(f"lie must be a tensor [T] or one of 'min', 'max', 'mean', got {lie!r}")
        n_s = b.n_s.to(torch.int64) if b.n_s is not None else torch.full((b.T,), b.ns, dtype=torch.int64, device=b.device)
        live = torch.arange(b.ns, device=b.device)[None, :] < n_s[:, None]
        y = b.y_s.to(torch.float32)
        if lie == "mean":
            lie = torch.where(live, y, torch.zeros_like(y)).sum(1) / n_s.clamp(min=1).to(torch.float32)
        else:
            pad = float("inf") if lie == "min" else float("-inf")
            y = torch.where(live, y, torch.full_like(y, pad))
            lie = y.min(1).values if lie == "min" else y.max(1).values
    if lie is not None:
        lie = _f32(lie, "lie").reshape(-1)
        if lie.numel() != b.T:
            raise ValueError(f"lie must have T = {b.T} entries")
    stride = 0
    if labels is not None:
        labels = _f32(labels, "labels")
        if tuple(labels.shape) == (b.T, rows):
            stride = rows
        elif tuple(labels.shape) != (rows,):
            raise ValueError(f"labels must be [rows] = [{rows}] or [T, rows] = [{b.T}, {rows}], got {tuple(labels.shape)}")
    _on_device(b, X=X, best_f=best_f, lie=lie, labels=labels)
    excl_idx, excl_off = _exclusion(b, exclude, b.T, rows)
    sel_idx, sel_val, info = _selection(b, b.T, q)
    sel_mean, sel_var, sel_lie, inc = _new(b, b.T, q), _new(b, b.T, q), _new(b, b.T, q), _new(b, b.T, q + 1)
    trace = _new(b, b.T, q, rows) if want_trace else None
    flags = (_lib.PM_MAXIMIZE if maximize else 0) | (_lib.PM_LOG_EI if log_ei else 0)
    args = (ptr(best_f), ptr(lie), ptr(labels), stride, ptr(excl_idx), ptr(excl_off), q, ptr(trace), ptr(sel_idx), ptr(sel_val),
            ptr(sel_mean), ptr(sel_var), ptr(sel_lie), ptr(inc))
    _pool_call(lib, "adkf_liar_pool", b, phi, flags, X, args, info, lib.adkf_liar_pool_scratch_bytes(b.T, b.ns, b.d, q))
    return dict(sel_idx=sel_idx, sel_val=sel_val, sel_mean=sel_mean, sel_var=sel_var, sel_lie=sel_lie, inc=inc, trace=trace, info=info)


def rff_basis(kernel, d: int, m: int, generator: Optional[torch.Generator] = None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A random-Fourier basis ``(omega [m, d], phase [m])`` of ``kernel`` AT UNIT LENGTHSCALE, as ``thompson_pool`` takes it:
    ``(1/m) sum_j 2 cos(omega_j.x + phase_j) cos(omega_j.y + phase_j)`` estimates ``kappa(|x - y|)``.  RBF: the rows of ``omega``
    are N(0, I); Matern-5/2: multivariate Student-t with 5 degrees of freedom, ``z / sqrt(g / 5)`` with ``g ~ chi^2_5`` per row;
    ``phase`` is uniform on [0, 2 pi).  Drawn in float64 on the generator's device (the CPU without one), returned as float32 on
    ``device``.  Pure torch; runs without a GPU."""
    import math

    kind = kernel_id(kernel)
    d, m = int(d), int(m)
    if d < 1 or m < 1:
        raise ValueError(f"rff_basis needs d >= 1 and m >= 1, got d = {d}, m = {m}")
    gdev = generator.device if generator is not None else torch.device("cpu")
    omega = torch.randn(m, d, dtype=torch.float64, generator=generator, device=gdev)
    if kind == KERNEL_MATERN52:
        chi2 = (torch.randn(m, 5, dtype=torch.float64, generator=generator, device=gdev) ** 2).sum(1, keepdim=True)
        omega = omega / torch.sqrt(chi2 / 5.0)
    phase = torch.rand(m, dtype=torch.float64, generator=generator, device=gdev) * (2.0 * math.pi)
    omega, phase = omega.float(), phase.float().clamp_(max=6.2831850)   # (float32 rounding must not reach 2 pi)
    if device is not None:
        omega, phase = omega.to(device), phase.to(device)
    return omega.contiguous(), phase.contiguous()


def _basis_and_draws(b, omega, phase, S: int, generator, w, eps):
    """The basis and the standard normal draws of the pathwise calls (``thompson_pool``, ``qei_pool``), checked:
    ``(omega [m, d], phase [m], m, w [T, S, m], eps [T, S, ns])``; ``w`` / ``eps`` are drawn from ``generator`` (on its device) where
    they are not given, ``w`` first."""
    omega, phase = _f32(omega, "omega"), _f32(phase, "phase")
    if omega.dim() != 2 or omega.shape[1] != b.d:
        raise ValueError(f"omega must be [m, d] = [m, {b.d}], got {tuple(omega.shape)}")
    m = omega.shape[0]
    if m < 64 or m > _lib.TS_FEATURES_MAX or m % 64:
        raise ValueError(f"the number of features must be a multiple of 64 in [64, {_lib.TS_FEATURES_MAX}], got {m}")
    if tuple(phase.shape) != (m,):
        raise ValueError(f"phase must be [m] = [{m}], got {tuple(phase.shape)}")

    def draw(t, shape, name):
        if t is None:
            gdev = generator.device if generator is not None else b.device
            return torch.randn(*shape, dtype=torch.float32, generator=generator, device=gdev).to(b.device).contiguous()
        t = _f32(t, name)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {tuple(t.shape)}")
        return t

    w = draw(w, (b.T, S, m), "w")
    eps = draw(eps, (b.T, S, b.ns), "eps")
    return omega, phase, m, w, eps


def _thompson_pool(name: str, b: GPBatch, phi, X, omega, phase, n_samples, generator, w, eps, maximize, exclude, want_paths):
    """The body of ``thompson_pool`` (``name = "thompson_pool"``, isotropic batches) and ``thompson_pool_ard`` (ARD batches)."""
    lib = _lib.load()
    ard = name == "thompson_pool_ard"
    _support_only(b, name)
    if b.ard and not ard:
        raise ValueError("thompson_pool does not support ARD batches: use thompson_pool_ard")
    if ard and not b.ard:
        raise ValueError("thompson_pool_ard takes an ARD batch (GPBatch(..., ard=True)): use thompson_pool")
    S = _in_range(n_samples, 1, _lib.TS_SAMPLES_MAX, "n_samples")
    phi, X = _phi_and_pool(b, phi, X)
    omega, phase, m, w, eps = _basis_and_draws(b, omega, phase, S, generator, w, eps)
    rows = X.shape[0]
    excl_idx, excl_off = _exclusion(b, exclude, b.T, rows)
    _on_device(b, X=X, omega=omega, phase=phase, w=w, eps=eps)
    paths = _new(b, b.T, S, rows) if want_paths else None
    sel_idx, sel_val, info = _selection(b, b.T, S)
    args = (ptr(omega), ptr(phase), m, ptr(w), ptr(eps), S, ptr(excl_idx), ptr(excl_off), ptr(paths), ptr(sel_idx), ptr(sel_val))
    _pool_call(lib, "adkf_" + name, b, phi, _lib.PM_MAXIMIZE if maximize else 0, X, args, info,
               lib.adkf_thompson_pool_scratch_bytes(b.T, b.ns, S, m))
    return dict(sel_idx=sel_idx, sel_val=sel_val, paths=paths, info=info, w=w, eps=eps)


def thompson_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, omega: torch.Tensor, phase: torch.Tensor, n_samples: int,
                  generator: Optional[torch.Generator] = None, w: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None,
                  maximize: bool = False, exclude=None, want_paths: bool = False):
    """Thompson sampling over the shared pool ``X [rows, d]`` in one ``adkf_thompson_pool`` call: every task of the support-only
    batch ``b`` draws ``n_samples`` (at most 64) pathwise posterior functions on the basis ``(omega [m, d], phase [m])``
    (``rff_basis``; m a multiple of 64, at most 4096), and each function picks its best eligible row.  Returns
    ``dict(sel_idx [T, S] int64, sel_val [T, S], paths [T, S, rows] or None, info [T], w [T, S, m], eps [T, S, ns])``:
    ``sel_val`` is the score of the pick, +f with ``maximize`` and -f without; -1 / -inf where no row is eligible.  ``w`` / ``eps``
    are the standard normal draws: given, or drawn here from ``generator`` (on its device) and returned.  ``exclude``: rows a task
    may not select (``pack_exclude``).  ARD batches go to ``thompson_pool_ard``."""
    return _thompson_pool("thompson_pool", b, phi, X, omega, phase, n_samples, generator, w, eps, maximize, exclude, want_paths)


def thompson_pool_ard(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, omega: torch.Tensor, phase: torch.Tensor, n_samples: int,
                      generator: Optional[torch.Generator] = None, w: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None,
                      maximize: bool = False, exclude=None, want_paths: bool = False):
    """``thompson_pool`` for ARD batches (``phi [T, 2 + d]``) in one ``adkf_thompson_pool_ard`` call: the same draws on the scaled
    features ``(x - mu) / l`` with one lengthscale per feature dimension.  ``(omega, phase)`` is the same basis at unit lengthscale
    (``rff_basis``), shared by all tasks; arguments and the returned dict are those of ``thompson_pool``.  Raises ``ValueError``
    for a batch that is not an ARD batch."""
    return _thompson_pool("thompson_pool_ard", b, phi, X, omega, phase, n_samples, generator, w, eps, maximize, exclude, want_paths)


def qei_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, omega: torch.Tensor, phase: torch.Tensor, n_samples: int, q: int,
             best_f: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, w: Optional[torch.Tensor] = None,
             eps: Optional[torch.Tensor] = None, maximize: bool = False, exclude=None, want_trace: bool = False, want_inc: bool = False):
    """Monte-Carlo q-EI over the shared pool ``X [rows, d]`` in one ``adkf_qei_pool`` call, for isotropic and ARD batches alike: every
    task of the support-only batch ``b`` draws ``n_samples`` (at most 256) pathwise posterior functions - ``thompson_pool``'s, on the
    same basis ``(omega [m, d], phase [m])`` and draws - and picks ``q`` (at most 64) rows by sequential-greedy maximisation of the
    sample average of the joint improvement ``max(0, incumbent_s - min_j f_s(x_j))`` (``maximize``: the mirror image).  Without
    ``best_f`` the incumbent of path s is its own best value over the task's support rows (noisy q-EI, BoTorch's
    ``qNoisyExpectedImprovement``); with ``best_f [T]`` it is that value for every path (``qExpectedImprovement``).  Returns
    ``dict(sel_idx [T, q] int64, sel_val [T, q], trace [T, q, rows] or None, inc [T, q + 1, S] or None, info [T], w, eps)``:
    ``sel_val`` the score of each pick at the step it was picked - their sum is the MC q-EI of the batch - and -1 / -inf from the step
    at which no eligible row was left; ``trace`` (``want_trace``) every row's score at every step; ``inc`` (``want_inc``) the
    incumbents before step 0 and after every step.  ``w`` / ``eps`` as in ``thompson_pool``; ``exclude``: rows a task may not select
    (``pack_exclude``)."""
    lib = _lib.load()
    _support_only(b, "qei_pool")
    S = _in_range(n_samples, 1, _lib.QEI_SAMPLES_MAX, "n_samples")
    q = _in_range(q, 1, _lib.QEI_PICKS_MAX, "q")
    phi, X = _phi_and_pool(b, phi, X)
    omega, phase, m, w, eps = _basis_and_draws(b, omega, phase, S, generator, w, eps)
    if best_f is not None:
        best_f = _f32(best_f, "best_f").reshape(-1)
        if best_f.numel() != b.T:
            raise ValueError(f"best_f must have T = {b.T} entries")
    rows = X.shape[0]
    excl_idx, excl_off = _exclusion(b, exclude, b.T, rows)
    _on_device(b, X=X, omega=omega, phase=phase, w=w, eps=eps, best_f=best_f)
    sel_idx, sel_val, info = _selection(b, b.T, q)
    trace = _new(b, b.T, q, rows) if want_trace else None
    inc = _new(b, b.T, q + 1, S) if want_inc else None
    args = (ptr(omega), ptr(phase), m, ptr(w), ptr(eps), S, ptr(best_f), ptr(excl_idx), ptr(excl_off), q, ptr(trace), ptr(inc),
            ptr(sel_idx), ptr(sel_val))
    _pool_call(lib, "adkf_qei_pool", b, phi, _lib.PM_MAXIMIZE if maximize else 0, X, args, info,
               lib.adkf_qei_pool_scratch_bytes(b.T, b.ns, S, m))
    return dict(sel_idx=sel_idx, sel_val=sel_val, trace=trace, inc=inc, info=info, w=w, eps=eps)


def mes_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, ystar: torch.Tensor, maximize: bool = False, topk: int = 0,
             exclude=None, want_score: Optional[bool] = None):
    """Max-value entropy search (Wang & Jegelka 2017) over the shared pool ``X [rows, d]`` in one ``adkf_mes_pool`` call, for
    isotropic and ARD batches alike.  ``ystar [T, S]`` (S at most 64, on the batch's device) holds samples of each task's optimum
    value - of max f with ``maximize``, of min f without; ``max_value_samples`` draws them.  The score of a row is
    ``mean_s g(gamma_s)`` with ``gamma_s = +-(ystar_s - mean) / sigma`` and ``g(gamma) = gamma phi(gamma) / (2 Phi(gamma)) -
    log Phi(gamma)``: positive, larger where observing the row says more about the optimum value; no ``best_f`` is involved.
    Returns ``dict(score, top_idx, top_val, info)``: ``score [T, rows]`` (``want_score``, which defaults to ``topk == 0``; else
    None), ``top_idx [T, topk]`` (int64) / ``top_val [T, topk]`` as ``predict_pool`` returns them (None with ``topk == 0``) and
    ``info [T]``.  A NaN or infinite ``ystar[t, s]`` makes the scores of task t NaN, which are never selected.  ``exclude``: rows a
    task may not select (``pack_exclude``).  With ``want_score=False`` nothing of size T x rows is allocated or written."""
    lib = _lib.load()
    _support_only(b, "mes_pool")
    topk = _in_range(topk, 0, _lib.POOL_TOPK_MAX, "topk")
    if want_score is None:
        want_score = topk == 0
    if not (want_score or topk > 0):
        raise ValueError("no output asked for")
    S = _sample_table(b, ystar, "ystar", "the number of max-value samples")
    ystar = _f32(ystar, "ystar")
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    _on_device(b, X=X, ystar=ystar)
    excl_idx, excl_off = _exclusion(b, exclude if topk > 0 else None, b.T, rows)
    score = _new(b, b.T, rows) if want_score else None
    top_idx, top_val, info = _selection(b, b.T, topk)
    args = (ptr(ystar), S, ptr(excl_idx), ptr(excl_off), ptr(score), topk, ptr(top_idx), ptr(top_val))
    _pool_call(lib, "adkf_mes_pool", b, phi, _lib.PM_MAXIMIZE if maximize else 0, X, args, info, lib.adkf_predict_pool_scratch_bytes(b.T, topk))
    return dict(score=score, top_idx=top_idx, top_val=top_val, info=info)


def gibbon_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, ystar: torch.Tensor, q: int, maximize: bool = False, exclude=None,
                want_trace: bool = False):
    """A GIBBON batch (Moss et al. 2021; BoTorch's ``qLowerBoundMaxValueEntropy``) per task from the shared pool ``X [rows, d]`` in
    one ``adkf_gibbon_pool`` call, for isotropic and ARD batches alike: ``q`` (at most 64) sequential-greedy picks of the lower bound
    on the information a batch of noisy observations carries about the task's optimum value.  ``ystar [T, S]`` (S at most 64, on the
    batch's device) holds samples of that value, as ``mes_pool`` takes them.  The score of a row at step j is
    ``a(x) + log((v_j + noise) / (v_0 + noise)) / 2``: ``a = -mean_s log1p(-rho2 h(gamma_s)) / 2`` the single-point score
    (``h = tau (gamma + tau)``, ``tau = phi / Phi``, ``rho2 = v_0 / (v_0 + noise)``) and ``v_j`` the latent variance of the row given
    the picks made so far, so a pick lowers the score of its neighbours - which the ``topk`` rows of ``mes_pool`` are.  No
    ``best_f`` is involved.  Returns ``dict(sel_idx, sel_val, sel_mean, sel_var, trace, info)`` as ``believer_pool`` does:
    ``sel_idx [T, q]`` (int64) the picks in pick order and ``sel_val`` their scores at the step they were picked (later ones may be
    negative: a pick counts when its index is not -1 and its value is finite), -1 / -inf from the step at which no eligible row was
    left; ``sel_mean`` the posterior means of the picks, ``sel_var`` the latent variance each pick had when it was picked;
    ``trace [T, q, rows]`` (``want_trace``, else None) the score of every row at every step; ``info [T]``.  A NaN or infinite
    ``ystar[t, s]`` makes the scores of task t NaN: no pick.  ``exclude``: rows a task may not select (``pack_exclude``)."""
    lib = _lib.load()
    _support_only(b, "gibbon_pool")
    q = _in_range(q, 1, _lib.POOL_TOPK_MAX, "q")
    S = _sample_table(b, ystar, "ystar", "the number of max-value samples S")
    ystar = _f32(ystar, "ystar")
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    _on_device(b, X=X, ystar=ystar)
    excl_idx, excl_off = _exclusion(b, exclude, b.T, rows)
    sel_idx, sel_val, info = _selection(b, b.T, q)
    sel_mean, sel_var = _new(b, b.T, q), _new(b, b.T, q)
    trace = _new(b, b.T, q, rows) if want_trace else None
    args = (ptr(ystar), S, ptr(excl_idx), ptr(excl_off), q, ptr(trace), ptr(sel_idx), ptr(sel_val), ptr(sel_mean), ptr(sel_var))
    _pool_call(lib, "adkf_gibbon_pool", b, phi, _lib.PM_MAXIMIZE if maximize else 0, X, args, info,
               lib.adkf_believer_pool_scratch_bytes(b.T, b.ns, b.d, q))
    return dict(sel_idx=sel_idx, sel_val=sel_val, sel_mean=sel_mean, sel_var=sel_var, trace=trace, info=info)


_LS_SCORES = {"straddle": _lib.LS_STRADDLE, "prob": _lib.LS_PROB, "bound": _lib.LS_BOUND}


def _per_task(b, value, name: str) -> torch.Tensor:
    """A scalar or ``[T]`` values as float32 ``[T]`` on the batch's device."""
    if torch.is_tensor(value):
        t = value.detach().to(device=b.device, dtype=torch.float32).reshape(-1)
    else:
        t = torch.as_tensor(value, dtype=torch.float32).reshape(-1).to(b.device)
    if t.numel() == 1:
        t = t.expand(b.T)
    if t.numel() != b.T:
        raise ValueError(f"{name} must be a scalar or have T = {b.T} entries, got {t.numel()}")
    return t.contiguous()


def levelset_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, tau, beta=1.96, q: int, score: str = "straddle", maximize: bool = False,
                  exclude=None, want_trace: bool = False, want_cls: bool = False, want_counts: bool = True):
    """Level-set estimation and batch UCB per task over the shared pool ``X [rows, d]`` in one ``adkf_levelset_pool`` call, for
    isotropic and ARD batches alike: which rows are on the active side of the threshold ``tau`` (``f > tau`` with ``maximize``,
    ``f < tau`` without), how many actives the pool is expected to hold, and ``q`` (at most 64) sequential-greedy picks of what to
    measure next.  ``tau`` and ``beta`` (the width of the confidence band, at least 0) are a scalar or ``[T]``.  With ``sigma_j`` the
    latent deviation of a row given the picks made so far (each pick hallucinated at its mean, as ``believer_pool`` does: the mean
    never moves) the score of a row at step j is, by ``score``:
    ``"straddle"``  ``beta sigma_j - |m - tau|`` (Bryan et al. 2005), positive exactly when the band ``m +- beta sigma_j`` holds tau;
    ``"prob"``      ``log Phi(+-(m - tau) / sigma_j)``, the log probability of being active - it does NOT diversify: the batch is the
    rows most certainly active if the earlier picks land on their means;
    ``"bound"``     ``+-m + beta sigma_j``: UCB with ``maximize``, minus LCB without (GP-BUCB; ``tau`` is not used by the score).
    A row is *undecided* (2) while its straddle is positive, otherwise *active* (0) or *inactive* (1) by the side of tau its mean is on.
    Returns ``dict(sel_idx, sel_val, sel_mean, sel_var, counts, hits, cls, trace, info)``: ``sel_*  [T, q]`` as ``believer_pool``
    returns them; ``counts [T, q, 3]`` (int64) the number of active, inactive and undecided rows of the whole pool at each step and
    ``hits [T, q]`` the expected number of actives ``sum_r Phi(z_j)`` (``want_counts``, else None; at steps j > 0 both are
    hallucinated like the picks - ask for ``q + 1`` steps and drop the last pick to see the counts after a batch of q);
    ``cls [T, rows]`` (int8, ``want_cls``) the class at step 0, -1 for a row that was not evaluated; ``trace [T, q, rows]``
    (``want_trace``) every score; ``info [T]``.  A task whose ``tau`` is not finite or whose ``beta`` is negative or not finite
    scores NaN everywhere: no pick, zero counts.  ``exclude``: rows a task may not select (``pack_exclude``); they are still counted."""
    lib = _lib.load()
    _support_only(b, "levelset_pool")
    if score not in _LS_SCORES:
        raise ValueError(f"score must be one of {sorted(_LS_SCORES)}, got {score!r}")
    q = _in_range(q, 1, _lib.POOL_TOPK_MAX, "q")
    tau, beta = _per_task(b, tau, "tau"), _per_task(b, beta, "beta")
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    _on_device(b, X=X)
    excl_idx, excl_off = _exclusion(b, exclude, b.T, rows)
    sel_idx, sel_val, info = _selection(b, b.T, q)
    sel_mean, sel_var = _new(b, b.T, q), _new(b, b.T, q)
    trace = _new(b, b.T, q, rows) if want_trace else None
    cls = _new(b, b.T, rows, dtype=torch.int8) if want_cls else None
    counts = _new(b, b.T, q, 3, dtype=torch.int64) if want_counts else None
    hits = _new(b, b.T, q) if want_counts else None
    args = (ptr(tau), ptr(beta), _LS_SCORES[score], ptr(excl_idx), ptr(excl_off), q, ptr(trace), ptr(cls), ptr(counts), ptr(hits),
            ptr(sel_idx), ptr(sel_val), ptr(sel_mean), ptr(sel_var))
    _pool_call(lib, "adkf_levelset_pool", b, phi, _lib.PM_MAXIMIZE if maximize else 0, X, args, info,
               lib.adkf_levelset_pool_scratch_bytes(b.T, b.ns, b.d, q))
    return dict(sel_idx=sel_idx, sel_val=sel_val, sel_mean=sel_mean, sel_var=sel_var, counts=counts, hits=hits, cls=cls, trace=trace, info=info)


def kg_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, ref_idx: Optional[torch.Tensor] = None, n_refs: int = 32,
            maximize: bool = False, log: bool = False, topk: int = 0, exclude=None, want_score: bool = True, want_cov: bool = False):
    """The knowledge gradient for correlated beliefs (Frazier, Powell & Dayanik 2009; Scott, Frazier & Powell 2011) over the shared
    pool ``X [rows, d]`` in one ``adkf_kg_pool`` call, for isotropic and ARD batches alike: a row is scored by how much one noisy
    observation there is expected to raise (``maximize``; lower without) the best posterior mean over the row itself and the
    reference rows ``ref_idx [T, M]`` (int64 pool indices, M at most 64, on the batch's device).  Entries outside ``[0, rows)`` are
    skipped - the ``top_idx`` of ``predict_pool`` with its -1 tail can be passed as it is - and a repeated index counts once.  With
    ``ref_idx=None`` each task's ``n_refs`` rows of best posterior mean, in the call's sense, are taken first, from one
    ``predict_pool(score="mean")`` call with no exclusions: rows already queried belong in the discretisation.  ``log``: the score is
    log KG, finite where float32 KG underflows to 0 (-inf for a row with no other line than its own).  Returns ``dict(score, cov,
    ref_mean, ref_idx, top_idx, top_val, info)``: ``score [T, rows]`` (``want_score``, else None), ``cov [T, rows, M]``
    (``want_cov``, else None) the latent posterior covariance of every row with every reference entry (0 for skipped entries),
    ``ref_mean [T, M]`` the entries' posterior means (0 for skipped entries), ``ref_idx`` as used, ``top_idx [T, topk]`` /
    ``top_val`` as ``predict_pool`` returns them (None with ``topk == 0``) and ``info [T]``.  ``exclude``: rows a task may not
    select (``pack_exclude``); they are still scored."""
    lib = _lib.load()
    _support_only(b, "kg_pool")
    topk = _in_range(topk, 0, _lib.POOL_TOPK_MAX, "topk")
    if ref_idx is None:
        n_refs = _in_range(n_refs, 1, _lib.KG_REFS_MAX, "n_refs")
    else:
        if not torch.is_tensor(ref_idx) or ref_idx.dtype != torch.int64 or ref_idx.dim() != 2 or ref_idx.shape[0] != b.T:
            raise ValueError(f"ref_idx must be an int64 tensor [T, M] = [{b.T}, M], got "
                             f"{(tuple(ref_idx.shape), ref_idx.dtype) if torch.is_tensor(ref_idx) else ref_idx!r}")
        _in_range(ref_idx.shape[1], 1, _lib.KG_REFS_MAX, "the number of reference rows M")
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    _on_device(b, X=X)
    if ref_idx is None:
        ref_idx = predict_pool(b, phi, X, maximize=maximize, topk=n_refs, score="mean", want_mean=False, want_var=False, want_ei=False)["top_idx"]
    _on_device(b, ref_idx=ref_idx)
    ref_idx = ref_idx.contiguous()
    M = ref_idx.shape[1]
    excl_idx, excl_off = _exclusion(b, exclude if topk > 0 else None, b.T, rows)
    score = _new(b, b.T, rows) if want_score else None
    cov = _new(b, b.T, rows, M) if want_cov else None
    ref_mean = _new(b, b.T, M)
    top_idx, top_val, info = _selection(b, b.T, topk)
    flags = (_lib.PM_MAXIMIZE if maximize else 0) | (_lib.PM_LOG_EI if log else 0)
    args = (ptr(ref_idx), M, ptr(excl_idx), ptr(excl_off), ptr(score), ptr(cov), ptr(ref_mean), topk, ptr(top_idx), ptr(top_val))
    _pool_call(lib, "adkf_kg_pool", b, phi, flags, X, args, info, lib.adkf_kg_pool_scratch_bytes(b.T, b.ns, b.d, M, topk))
    return dict(score=score, cov=cov, ref_mean=ref_mean, ref_idx=ref_idx, top_idx=top_idx, top_val=top_val, info=info)


def ipv_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, targets, weights: Optional[torch.Tensor] = None, q: int, exclude=None,
             want_trace: bool = False, want_tvar: bool = True):
    """Target-variance batch selection (ALC, Cohn 1996; BoTorch's ``qNegIntegratedPosteriorVariance``; transductive active learning)
    per task from the shared pool ``X [rows, d]`` in one ``adkf_ipv_pool`` call, for isotropic and ARD batches alike: ``q``
    sequential-greedy picks, each the row whose noisy observation lowers the weighted latent posterior variance at the task's target
    rows the most, given the picks before it.  No label is needed, so the whole batch is chosen before anything is measured.
    ``targets [T, M]``: integer pool indices (a tensor or nested lists; ``M + q`` at most 64); ``weights [T, M]``: their weights
    (None: 1).  An entry outside ``[0, rows)``, one whose index an earlier entry of its task has, and one whose weight is ``<= 0``
    or NaN are skipped.  The targets themselves ARE eligible - observing a target is the best single pick; put them in ``exclude``
    if they cannot be measured.  Returns ``dict(sel_idx, sel_val, tvar, trace, info)``: ``sel_idx [T, q]`` (int64) the picks in
    pick order and ``sel_val`` the amount each took off the target variance, -1 / -inf from the step at which no eligible row was
    left (and at every step of a task without a valid target); ``tvar [T, q + 1]`` (``want_tvar``, else None) the weighted target
    variance before the first pick and after each; ``trace [T, q, rows]`` (``want_trace``, else None) the score of every row at
    every step; ``info [T]``.  ``exclude``: rows a task may not select (``pack_exclude``).  A target row with non-finite features
    makes every score of its task NaN: nothing is selected."""
    lib = _lib.load()
    _support_only(b, "ipv_pool")
    q = _in_range(q, 1, _lib.IPV_ENTRIES_MAX - 1, "q")
    M = _int_table(targets, "targets", b.T, None, f"an integer table [T, M] = [{b.T}, M]").shape[1]   # (the check; the indices stay int64)
    _in_range(M, 1, _lib.IPV_ENTRIES_MAX - q, f"the number of target entries M (M + q at most {_lib.IPV_ENTRIES_MAX})")
    if weights is not None:
        weights = torch.as_tensor(weights)
        if tuple(weights.shape) != (b.T, M):
            raise ValueError(f"weights must be [T, M] = [{b.T}, {M}], got {tuple(weights.shape)}")
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    _on_device(b, X=X)
    if weights is not None:
        weights = weights.to(device=b.device, dtype=torch.float32).contiguous()
    targets = torch.as_tensor(targets).to(device=b.device, dtype=torch.int64).contiguous()
    excl_idx, excl_off = _exclusion(b, exclude, b.T, rows)
    sel_idx, sel_val, info = _selection(b, b.T, q)
    tvar = _new(b, b.T, q + 1) if want_tvar else None
    trace = _new(b, b.T, q, rows) if want_trace else None
    args = (ptr(targets), ptr(weights), M, ptr(excl_idx), ptr(excl_off), q, ptr(trace), ptr(sel_idx), ptr(sel_val), ptr(tvar))
    _pool_call(lib, "adkf_ipv_pool", b, phi, 0, X, args, info, lib.adkf_ipv_pool_scratch_bytes(b.T, b.ns, b.d, M, q))
    return dict(sel_idx=sel_idx, sel_val=sel_val, tvar=tvar, trace=trace, info=info)


def jackknife_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, alpha=(0.1,), scaled: bool = False, maximize: bool = False,
                   topk: int = 0, exclude=None, want_lo: bool = True, want_hi: bool = True, want_loo: bool = True):
    """Leave-one-out checks (Rasmussen & Williams, section 5.4.2) and jackknife+ prediction intervals (Barber, Candes, Ramdas &
    Tibshirani 2021) for every row of the shared pool ``X [rows, d]`` in one ``adkf_jackknife_pool`` call, for isotropic and ARD
    batches alike (at most 256 support points per task).  Everything is at the ``phi`` passed - the hyperparameters are NOT refitted
    per fold - and costs no extra factorisation: deleting point i is a rank-one update of the posterior.  ``alpha``: up to 8 levels
    (floats, or a float32 tensor; rounded to float32, whose bits set the ranks); ``[lo[t, l], hi[t, l]]`` covers a new label with
    probability at least ``1 - 2 alpha[l]`` whatever the data's distribution, for the fixed-``phi`` predictor (with ``phi`` fitted on
    the same points: a very good approximation, not a theorem).  ``scaled``: fold widths scaled by the leave-one-out predictive
    deviation at the row, so intervals widen away from the data.  Returns ``dict(lo, hi, loo_mean, loo_var, loo_lpd, top_idx,
    top_val, info)``: ``lo`` / ``hi [T, L, rows]`` (``want_lo`` / ``want_hi``, else None; -inf / +inf where the task has too few
    points for the level, ``floor(alpha (n + 1)) == 0``), ``loo_mean`` / ``loo_var [T, ns]`` the leave-one-out predictive mean and
    observed variance of every support point and ``loo_lpd [T]`` their summed log predictive density (``want_loo``, else None),
    ``top_idx [T, topk]`` / ``top_val`` as ``predict_pool`` returns them on the level-0 score - ``lo`` with ``maximize``, ``-hi``
    without: screening by the bound one can rely on; rows without a finite bound are never selected - and ``info [T]``.
    ``exclude``: rows a task may not select (``pack_exclude``).  With ``want_lo = want_hi = False`` nothing of size T x rows is
    allocated or written."""
    lib = _lib.load()
    _support_only(b, "jackknife_pool")
    topk = _in_range(topk, 0, _lib.POOL_TOPK_MAX, "topk")
    _in_range(b.ns, 1, _lib.JK_POINTS_MAX, "the support size ns (with more labels use a held-out split)")
    alpha = torch.as_tensor(alpha, dtype=torch.float32).reshape(-1)
    L = _in_range(alpha.numel(), 1, _lib.JK_LEVELS_MAX, "the number of levels")
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    _on_device(b, X=X)
    if not (want_lo and rows > 0 or want_hi and rows > 0 or want_loo or topk > 0):
        raise ValueError("no output asked for")
    alpha = alpha.to(b.device).contiguous()
    excl_idx, excl_off = _exclusion(b, exclude if topk > 0 else None, b.T, rows)
    lo = _new(b, b.T, L, rows) if want_lo else None
    hi = _new(b, b.T, L, rows) if want_hi else None
    loo_mean = _new(b, b.T, b.ns) if want_loo else None
    loo_var = _new(b, b.T, b.ns) if want_loo else None
    loo_lpd = _new(b, b.T) if want_loo else None
    top_idx, top_val, info = _selection(b, b.T, topk)
    flags = (_lib.PM_MAXIMIZE if maximize else 0) | (_lib.PM_JK_SCALED if scaled else 0)
    args = (ptr(alpha), L, ptr(excl_idx), ptr(excl_off), ptr(lo), ptr(hi), ptr(loo_mean), ptr(loo_var), ptr(loo_lpd), topk, ptr(top_idx),
            ptr(top_val))
    _pool_call(lib, "adkf_jackknife_pool", b, phi, flags, X, args, info, lib.adkf_jackknife_pool_scratch_bytes(b.T, b.ns, L, topk))
    return dict(lo=lo, hi=hi, loo_mean=loo_mean, loo_var=loo_var, loo_lpd=loo_lpd, top_idx=top_idx, top_val=top_val, info=info)


def loo(b: GPBatch, phi: torch.Tensor):
    """Leave-one-out cross-validation of the fitted tasks at ``phi`` (not refitted per fold): the ``rows = 0`` form of
    ``jackknife_pool``.  Returns ``dict(loo_mean [T, ns], loo_var [T, ns], loo_lpd [T], info [T])``."""
    out = jackknife_pool(b, phi, torch.empty(0, b.d, device=b.device), want_lo=False, want_hi=False)
    return {k: out[k] for k in ("loo_mean", "loo_var", "loo_lpd", "info")}


def max_value_samples(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, omega: torch.Tensor, phase: torch.Tensor, n_samples: int,
                      generator: Optional[torch.Generator] = None, w: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None,
                      maximize: bool = False):
    """``n_samples`` samples of each task's optimum value over the pool ``X [rows, d]``, as ``mes_pool`` takes them: the optima of
    pathwise posterior draws, from ONE ``thompson_pool`` (ARD batches: ``thompson_pool_ard``) call without exclusions and without
    paths.  Returns ``dict(ystar [T, S], info [T], w, eps)``: ``ystar`` holds max f with ``maximize`` and min f without (the call's
    ``sel_val`` is +f and -f; -inf, hence +-inf here, for a skipped task or an empty pool), ``w`` / ``eps`` the standard normal
    draws, given or drawn from ``generator`` as ``thompson_pool`` draws them."""
    draw = thompson_pool_ard if b.ard else thompson_pool
    out = draw(b, phi, X, omega=omega, phase=phase, n_samples=n_samples, generator=generator, w=w, eps=eps, maximize=maximize)
    ystar = out["sel_val"] if maximize else -out["sel_val"]
    return dict(ystar=ystar, info=out["info"], w=out["w"], eps=out["eps"])


def optimum_samples(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, omega: torch.Tensor, phase: torch.Tensor, n_samples: int,
                    generator: Optional[torch.Generator] = None, w: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None,
                    maximize: bool = False):
    """``n_samples`` samples of each task's optimum over the pool ``X [rows, d]`` - its location AND its value, as ``jes_pool`` takes
    them: the optima of pathwise posterior draws, from ONE ``thompson_pool`` (ARD batches: ``thompson_pool_ard``) call without
    exclusions and without paths, with ``max_value_samples``' arguments.  Returns ``dict(opt_idx [T, S] int64, opt_val [T, S],
    info [T], w, eps)``: ``opt_idx`` is the pool row at which draw s attains its optimum (-1 for a skipped task or an empty pool),
    ``opt_val`` the value there in its natural sign - max f with ``maximize``, min f without (+-inf where ``opt_idx`` is -1) -
    and ``w`` / ``eps`` the standard normal draws, given or drawn from ``generator`` as ``thompson_pool`` draws them."""
    draw = thompson_pool_ard if b.ard else thompson_pool
    out = draw(b, phi, X, omega=omega, phase=phase, n_samples=n_samples, generator=generator, w=w, eps=eps, maximize=maximize)
    opt_val = out["sel_val"] if maximize else -out["sel_val"]
    return dict(opt_idx=out["sel_idx"], opt_val=opt_val, info=out["info"], w=out["w"], eps=out["eps"])


def jes_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, opt_idx: torch.Tensor, opt_val: torch.Tensor, cond_noise: float = 1e-6,
             maximize: bool = False, topk: int = 0, exclude=None, want_score: Optional[bool] = None):
    """Joint entropy search (Hvarfner, Hutter & Nardi 2022; BoTorch's ``qLowerBoundJointEntropySearch`` at q = 1) over the shared
    pool ``X [rows, d]`` in one ``adkf_jes_pool`` call, for isotropic and ARD batches alike.  ``opt_idx [T, S]`` (int64 pool rows)
    and ``opt_val [T, S]`` (S at most 64, both on the batch's device) hold samples of each task's optimum, location and value
    together - of max f with ``maximize``, of min f without; ``optimum_samples`` draws them.  A row is scored by the entropy of the
    noisy observation there minus the mean over the samples of its entropy given ``f(x*_s) = f*_s`` (under the noise variance
    ``cond_noise``, finite and >= 0) and ``f <= f*_s``, moment-matched: non-negative, larger where observing the row says more about
    the optimum; no ``best_f`` is involved.  Entries of ``opt_idx`` outside ``[0, rows)`` are skipped samples (``thompson_pool``'s
    -1 can be passed as it is), a repeated row counts each time; with no valid sample, or a NaN or infinite ``opt_val`` on a valid
    one, the scores of that task are NaN, which are never selected.  Returns ``dict(score, opt_mean, opt_var, top_idx, top_val,
    info)``: ``score [T, rows]`` (``want_score``, which defaults to ``topk == 0``; else None), ``opt_mean [T, S]`` / ``opt_var`` the
    posterior mean and latent variance at each sampled location (0 for skipped samples), ``top_idx [T, topk]`` (int64) /
    ``top_val [T, topk]`` as ``predict_pool`` returns them (None with ``topk == 0``) and ``info [T]``.  ``exclude``: rows a task may
    not select (``pack_exclude``); they are still scored."""
    lib = _lib.load()
    _support_only(b, "jes_pool")
    topk = _in_range(topk, 0, _lib.POOL_TOPK_MAX, "topk")
    if want_score is None:
        want_score = topk == 0
    if not torch.is_tensor(opt_idx) or opt_idx.dtype != torch.int64 or opt_idx.dim() != 2 or opt_idx.shape[0] != b.T:
        raise ValueError(f"opt_idx must be an int64 tensor [T, S] = [{b.T}, S], got "
                         f"{(tuple(opt_idx.shape), opt_idx.dtype) if torch.is_tensor(opt_idx) else opt_idx!r}")
    S = _in_range(opt_idx.shape[1], 1, _lib.TS_SAMPLES_MAX, "the number of optimum samples S")
    if not torch.is_tensor(opt_val) or tuple(opt_val.shape) != (b.T, S):
        raise ValueError(f"opt_val must be a tensor [T, S] = [{b.T}, {S}], got {tuple(opt_val.shape) if torch.is_tensor(opt_val) else opt_val!r}")
    cond_noise = float(cond_noise)
    if not (0.0 <= cond_noise < float("inf")):
        raise ValueError(f"cond_noise must be finite and >= 0, got {cond_noise}")
    opt_val = _f32(opt_val, "opt_val")
    opt_idx = opt_idx.contiguous()
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    _on_device(b, X=X, opt_idx=opt_idx, opt_val=opt_val)
    excl_idx, excl_off = _exclusion(b, exclude if topk > 0 else None, b.T, rows)
    score = _new(b, b.T, rows) if want_score else None
    opt_mean, opt_var = _new(b, b.T, S), _new(b, b.T, S)
    top_idx, top_val, info = _selection(b, b.T, topk)
    args = (ptr(opt_idx), ptr(opt_val), S, cond_noise, ptr(excl_idx), ptr(excl_off), ptr(score), ptr(opt_mean), ptr(opt_var), topk,
            ptr(top_idx), ptr(top_val))
    _pool_call(lib, "adkf_jes_pool", b, phi, _lib.PM_MAXIMIZE if maximize else 0, X, args, info,
               lib.adkf_jes_pool_scratch_bytes(b.T, b.ns, b.d, S, topk))
    return dict(score=score, opt_mean=opt_mean, opt_var=opt_var, top_idx=top_idx, top_val=top_val, info=info)


def pareto_front(Y, maximize=(False, False), ref=None) -> torch.Tensor:
    """The staircase of the two-objective values ``Y [n, 2]`` as ``ehvi_pool`` cleans a front on the device: points with a NaN leave,
    then (with ``ref``) points not strictly better than the reference point in both coordinates, then points weakly dominated by
    another one (of exact duplicates the one of lowest index stays).  ``maximize``: the sense per objective.  Returns ``[P, 2]`` in
    the caller's units, sorted as the device sorts it: by the first objective from its best value to its worst (the second objective
    then runs from worst to best).  Pure torch; runs on CPU tensors too."""
    Y = torch.as_tensor(Y)
    if Y.dim() != 2 or Y.shape[1] != 2:
        raise ValueError(f"Y must be [n, 2], got {tuple(Y.shape)}")
    if not Y.is_floating_point():
        Y = Y.float()
    sg = torch.tensor([-1.0 if m else 1.0 for m in maximize], dtype=Y.dtype, device=Y.device)
    F = Y * sg   # everything below minimises
    valid = ~torch.isnan(F).any(1)
    if ref is not None:
        r = torch.as_tensor(ref, dtype=Y.dtype, device=Y.device).reshape(2) * sg
        valid = valid & (F[:, 0] < r[0]) & (F[:, 1] < r[1])
    i = torch.arange(F.shape[0], device=Y.device)
    a, c = F[:, 0], F[:, 1]
    weak = (a[None, :] <= a[:, None]) & (c[None, :] <= c[:, None])   # [i, j]: j is nowhere worse than i
    first = (a[None, :] < a[:, None]) | (c[None, :] < c[:, None]) | (i[None, :] < i[:, None])
    dominated = (weak & first & valid[None, :] & (i[None, :] != i[:, None])).any(1)
    S = F[valid & ~dominated]
    return S[torch.argsort(S[:, 0], stable=True)] * sg


def _int_table(x, name: str, G: Optional[int], width: Optional[int], what: str) -> torch.Tensor:
    """An integer table [G, width] on the host (None: any extent), from a tensor or nested lists."""
    try:
        t = torch.as_tensor(x)
    except Exception:
        t = None
    if t is None or t.is_floating_point() or t.dim() != 2 or (G is not None and t.shape[0] != G) or (width is not None and t.shape[1] != width):
        raise ValueError(f"{name} must be {what}, got {tuple(t.shape) if t is not None else x!r}")
    return t.to(torch.int32)


def ehvi_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, obj, ref, front=None, front_n=None, obj_maximize=None, con=None,
              con_thr=None, con_geq=None, log: bool = False, topk: int = 0, exclude=None, want_score: Optional[bool] = None,
              want_stair: bool = False):
    """Constrained expected hypervolume improvement ACROSS the tasks of the batch (Emmerich et al. 2011, Yang et al. 2019; BoTorch's
    analytic ``ExpectedHypervolumeImprovement`` weighted as its ``ConstrainedExpectedImprovement`` weights EI; ``log``: their log
    forms) over the shared pool ``X [rows, d]`` in one ``adkf_ehvi_pool`` call, for isotropic and ARD batches alike.  The T tasks are
    properties of the same rows; group g names its objective tasks ``obj[g] = (t1, t2)`` (``t2 == -1``: one objective, plain
    constrained EI with ``best_f = ref[g, 0]``), their senses ``obj_maximize[g]`` (default: minimise both), the reference point
    ``ref[g]``, its front ``front[g, :front_n[g]]`` ``[G, P, 2]`` in the objectives' own units (P at most 64; ``pareto_front`` makes
    one, but any set of points will do: the device cleans it) and up to four constraint tasks ``con[g]`` (-1: unused) with thresholds
    ``con_thr[g]``, feasible when the latent ``f <= thr`` (``con_geq[g, c] = 1``: when ``f >= thr``).  A task may serve in several
    groups.  A group that cannot be evaluated - a task index out of range, both objectives the same task, a member task that is
    empty or failed, a NaN in ``ref`` or in a used threshold - scores NaN and selects nothing.
    Returns ``dict(score, top_idx, top_val, stair, stair_n, info)``: ``score [G, rows]`` (``want_score``, which defaults to
    ``topk == 0``; else None), ``top_idx [G, topk]`` (int64) / ``top_val`` as ``predict_pool`` returns them per task (None with
    ``topk == 0``), ``stair [G, P, 2]`` / ``stair_n [G]`` (int32) the cleaned staircase per group (``want_stair``; else None) and
    ``info [T]``.  ``exclude``: rows a GROUP may not select (``pack_exclude`` over G lists); they are still scored."""
    lib = _lib.load()
    _support_only(b, "ehvi_pool")
    topk = _in_range(topk, 0, _lib.POOL_TOPK_MAX, "topk")
    if want_score is None:
        want_score = topk == 0
    obj = _int_table(obj, "obj", None, 2, "an integer table [G, 2] of task indices (-1 in the second column: one objective)")
    G = obj.shape[0]
    if G < 1:
        raise ValueError("obj must be an integer table [G, 2] with at least one group")
    ref = torch.as_tensor(ref, dtype=torch.float32) if not torch.is_tensor(ref) else ref.float()
    if tuple(ref.shape) != (G, 2):
        raise ValueError(f"ref must be [G, 2] = [{G}, 2], got {tuple(ref.shape)}")
    if obj_maximize is not None:
        obj_maximize = _int_table(torch.as_tensor(obj_maximize).to(torch.int32), "obj_maximize", G, 2, f"a 0 | 1 table [G, 2] = [{G}, 2]")
    P = 0
    if front is not None:
        front = torch.as_tensor(front, dtype=torch.float32) if not torch.is_tensor(front) else front.float()
        if front.dim() != 3 or front.shape[0] != G or front.shape[2] != 2:
            raise ValueError(f"front must be [G, P, 2] = [{G}, P, 2], got {tuple(front.shape)}")
        P = _in_range(front.shape[1], 0, _lib.EHVI_FRONT_MAX, "the number of front points P")
        if P == 0:
            front = None
    if front_n is None:
        front_n = torch.full((G,), P, dtype=torch.int32)
    else:
        front_n = torch.as_tensor(front_n).to(torch.int32).reshape(-1)
        if front_n.numel() != G:
            raise ValueError(f"front_n must be [G] = [{G}], got {tuple(front_n.shape)}")
    Cn = 0
    if con is not None:
        con = _int_table(con, "con", G, None, f"an integer table [G, C] = [{G}, C] of task indices (-1: unused)")
        Cn = _in_range(con.shape[1], 0, _lib.EHVI_CONS_MAX, "the number of constraints C")
        if Cn == 0:
            con = None
    if Cn > 0:
        if con_thr is None:
            raise ValueError("con_thr must be given with con")
        con_thr = torch.as_tensor(con_thr, dtype=torch.float32) if not torch.is_tensor(con_thr) else con_thr.float()
        if tuple(con_thr.shape) != (G, Cn):
            raise ValueError(f"con_thr must be [G, C] = [{G}, {Cn}], got {tuple(con_thr.shape)}")
        con_geq = torch.zeros(G, Cn, dtype=torch.int32) if con_geq is None else _int_table(
            torch.as_tensor(con_geq).to(torch.int32), "con_geq", G, Cn, f"a 0 | 1 table [G, C] = [{G}, {Cn}]")
    else:
        con_thr = con_geq = None
    if topk == 0 and not want_score and not want_stair:
        raise ValueError("no output requested: topk == 0, want_score and want_stair are all off")
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    dev = b.device
    put = lambda t: None if t is None else t.to(dev).contiguous()
    obj, obj_maximize, ref, front, front_n, con, con_thr, con_geq = (put(t) for t in (obj, obj_maximize, ref, front, front_n, con, con_thr, con_geq))
    excl_idx, excl_off = _exclusion(b, exclude if topk > 0 else None, G, rows)
    score = _new(b, G, rows) if want_score else None
    stair = _new(b, G, P, 2) if want_stair else None
    stair_n = _new(b, G, dtype=torch.int32) if want_stair else None
    top_idx, top_val, info = _selection(b, G, topk)
    args = (G, ptr(obj), ptr(obj_maximize), ptr(ref), ptr(front), ptr(front_n), P, ptr(con), ptr(con_thr), ptr(con_geq), Cn, ptr(excl_idx),
            ptr(excl_off), ptr(score), ptr(stair) if P > 0 else None, ptr(stair_n), topk, ptr(top_idx), ptr(top_val))
    _pool_call(lib, "adkf_ehvi_pool", b, phi, _lib.PM_LOG_EI if log else 0, X, args, info, lib.adkf_ehvi_pool_scratch_bytes(b.T, G, topk))
    return dict(score=score, top_idx=top_idx, top_val=top_val, stair=stair, stair_n=stair_n, info=info)


_MIX_SCORES = {"ei": 0, "log_ei": _lib.PM_LOG_EI, "mean": _lib.PM_SCORE_MEAN, "bald": _lib.PM_SCORE_BALD}


def mix_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, members, weights=None, best_f: Optional[torch.Tensor] = None,
             score: str = "ei", latent: bool = False, maximize: bool = False, want_mean: bool = True, want_var: bool = True,
             want_score: Optional[bool] = None, topk: int = 0, exclude=None):
    """Hyperparameter-marginalised prediction and acquisition (the integrated acquisition of Snoek et al. 2012; BoTorch's average
    over the MCMC batch of a fully Bayesian model) over the shared pool ``X [rows, d]`` in one ``adkf_mix_pool`` call, for isotropic
    and ARD batches alike.  The T tasks are models of the same rows - ``replicate_batch`` makes M copies of every task, which then
    take M samples of ``phi`` (``phi_laplace_samples``).  Group g averages its member tasks ``members[g]`` ``[G, M]`` (M at most
    64; -1: unused) with ``weights[g]`` (default: equal; normalised by the library; a zero weight leaves the entry unused).  A task
    may serve in several groups.  Returns ``dict(mean, var, score, top_idx, top_val, info)``: ``mean [G, rows]`` the mixture mean,
    ``var`` its total variance (mean of the members' variances, with their noise unless ``latent``, plus the variance of their
    means), ``score`` (``want_score``, which defaults to ``topk == 0``) and the selection by it as ``predict_pool`` returns one
    per task.  ``score``: ``"ei"`` the integrated EI, ``"log_ei"`` its logarithm formed without EI (both need ``best_f [T]``, per
    member task), ``"mean"`` (+mean with ``maximize``, -mean without) or ``"bald"``, the disagreement of the members
    ``(log var - sum_i wt_i log v_i) / 2`` (Riis et al. 2022; BoTorch's ``qBayesianActiveLearningByDisagreement``): an
    active-learning score.  A group that cannot be evaluated - an index out of range, a negative or non-finite weight, no used
    entry, a used member that is empty or failed - is NaN and selects nothing.  A group with one member has ``predict_pool``'s bits.
    ``exclude``: rows a GROUP may not select (``pack_exclude`` over G lists)."""
    lib = _lib.load()
    _support_only(b, "mix_pool")
    if score not in _MIX_SCORES:
        raise ValueError(f"score must be 'ei', 'log_ei', 'mean' or 'bald', got {score!r}")
    topk = _in_range(topk, 0, _lib.POOL_TOPK_MAX, "topk")
    if want_score is None:
        want_score = topk == 0
    members = _int_table(members, "members", None, None, "an integer table [G, M] of task indices (-1: unused)")
    G = members.shape[0]
    if G < 1:
        raise ValueError("members must be an integer table [G, M] with at least one group")
    M = _in_range(members.shape[1], 1, _lib.MIX_MEMBERS_MAX, "the number of members M")
    if weights is not None:
        weights = torch.as_tensor(weights, dtype=torch.float32) if not torch.is_tensor(weights) else weights.float()
        if tuple(weights.shape) != (G, M):
            raise ValueError(f"weights must be [G, M] = [{G}, {M}], got {tuple(weights.shape)}")
    reads_ei = score in ("ei", "log_ei") and (want_score or topk > 0)
    if best_f is not None:
        best_f = best_f.float().reshape(-1)
        if best_f.numel() != b.T:
            raise ValueError(f"best_f must have T = {b.T} entries")
    if reads_ei and best_f is None:
        raise ValueError("the ei and log_ei scores need best_f [T]")
    if not (want_mean or want_var or want_score or topk > 0):
        raise ValueError("no output requested: topk == 0, want_mean, want_var and want_score are all off")
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    dev = b.device
    members = members.to(dev).contiguous()
    weights = None if weights is None else weights.to(dev).contiguous()
    best_f = None if best_f is None else _f32(best_f.to(dev), "best_f")
    excl_idx, excl_off = _exclusion(b, exclude if topk > 0 else None, G, rows)
    mean = _new(b, G, rows) if want_mean else None
    var = _new(b, G, rows) if want_var else None
    sc = _new(b, G, rows) if want_score else None
    top_idx, top_val, info = _selection(b, G, topk)
    flags = (_lib.PM_LATENT if latent else 0) | (_lib.PM_MAXIMIZE if maximize else 0) | _MIX_SCORES[score]
    args = (G, ptr(members), ptr(weights), M, ptr(best_f), ptr(excl_idx), ptr(excl_off), ptr(mean), ptr(var), ptr(sc), topk, ptr(top_idx),
            ptr(top_val))
    _pool_call(lib, "adkf_mix_pool", b, phi, flags, X, args, info, lib.adkf_mix_pool_scratch_bytes(b.T, G, topk))
    return dict(mean=mean, var=var, score=sc, top_idx=top_idx, top_val=top_val, info=info)


def rank_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, best_f: Optional[torch.Tensor] = None, maximize: bool = False,
              score: str = "ei", log_ei: bool = False, latent: bool = False, topk: int = 0, rank_rows=None, exclude=None):
    """Large selections and row ranks over the shared pool ``X [rows, d]`` in one ``adkf_rank_pool`` call, for isotropic and ARD
    batches alike: what a virtual screen asks beyond a BO batch.  The score, the eligibility and the order are ``predict_pool``'s
    (``score``: ``"ei"``, which needs ``best_f [T]`` and is log EI with ``log_ei``, or ``"mean"``), but ``topk`` goes up to 65536
    instead of 64, and ``rank_rows`` - a ``[T, M]`` int64 tensor, or a list of T index lists (padded with -1), M at most 1024 - names
    rows whose place in each task's ranking is wanted: known actives, for enrichment factors.  Returns ``dict(top_idx, top_val,
    ref_rank, ref_val, n_ranked, info)``: ``top_idx [T, topk]`` / ``top_val`` as ``predict_pool`` returns them (None with
    ``topk == 0``), ``ref_rank [T, M]`` (int64) the number of eligible rows that come strictly before the named row - 0-based, so an
    eligible row with ``ref_rank < topk`` is ``top_idx[t, ref_rank]``; an excluded row gets the place it would take; -1 for an entry
    outside the pool or a NaN score - with ``ref_val`` that row's score (None, None without ``rank_rows``), ``n_ranked [T]`` (int64)
    the rows a task ranked (neither excluded nor NaN), and ``info [T]``.  ``exclude``: rows a task may not list
    (``pack_exclude``).  Nothing of size T x rows is allocated."""
    lib = _lib.load()
    _support_only(b, "rank_pool")
    if score not in ("ei", "mean"):
        raise ValueError(f"score must be 'ei' or 'mean', got {score!r}")
    if log_ei and score != "ei":
        raise ValueError("log_ei with score='mean': nothing would read it")
    topk = _in_range(topk, 0, _lib.RANK_K_MAX, "topk")
    if rank_rows is not None:
        if not torch.is_tensor(rank_rows):
            lists = [[int(i) for i in (l if l is not None else [])] for l in rank_rows]
            width = max([len(l) for l in lists], default=0)
            rank_rows = torch.tensor([l + [-1] * (width - len(l)) for l in lists], dtype=torch.int64).reshape(len(lists), width)
        if rank_rows.dtype != torch.int64 or rank_rows.dim() != 2 or rank_rows.shape[0] != b.T:
            raise ValueError(f"rank_rows must be an int64 tensor [T, M] = [{b.T}, M] or T index lists, got "
                             f"{(tuple(rank_rows.shape), rank_rows.dtype)}")
        _in_range(rank_rows.shape[1], 0, _lib.RANK_REFS_MAX, "the number of ranked rows M")
        if rank_rows.shape[1] == 0:
            rank_rows = None
    if best_f is not None:
        best_f = torch.as_tensor(best_f).float().reshape(-1)
        if best_f.numel() != b.T:
            raise ValueError(f"best_f must have T = {b.T} entries")
    if score == "ei" and best_f is None:
        raise ValueError("ranking by ei needs best_f [T]")
    phi, X = _phi_and_pool(b, phi, X)
    rows = X.shape[0]
    dev = b.device
    best_f = None if best_f is None else _f32(best_f.to(dev), "best_f")
    _on_device(b, X=X)
    M = 0 if rank_rows is None else rank_rows.shape[1]
    ref_idx = None if rank_rows is None else rank_rows.to(dev).contiguous()
    ref_rank = _new(b, b.T, M, dtype=torch.int64) if M else None
    ref_val = _new(b, b.T, M) if M else None
    n_ranked = _new(b, b.T, dtype=torch.int64)
    excl_idx, excl_off = _exclusion(b, exclude, b.T, rows)
    top_idx, top_val, info = _selection(b, b.T, topk)
    flags = (_lib.PM_LATENT if latent else 0) | (_lib.PM_MAXIMIZE if maximize else 0) | (_lib.PM_SCORE_MEAN if score == "mean" else 0)
    flags |= _lib.PM_LOG_EI if log_ei else 0
    args = (ptr(best_f), ptr(excl_idx), ptr(excl_off), topk, ptr(top_idx), ptr(top_val), ptr(ref_idx), M, ptr(ref_rank), ptr(ref_val),
            ptr(n_ranked))
    _pool_call(lib, "adkf_rank_pool", b, phi, flags, X, args, info, lib.adkf_rank_pool_scratch_bytes(b.T, topk, M, b.d))
    return dict(top_idx=top_idx, top_val=top_val, ref_rank=ref_rank, ref_val=ref_val, n_ranked=n_ranked, info=info)


def replicate_batch(b: GPBatch, M: int):
    """``(bm, members)``: a support-only batch in which task t of ``b`` occupies the tasks ``t * M .. t * M + M - 1`` - the same
    data, ``n_s``, priors, kernel and ARD flag, no reuse flags (its workspace is its own) - and ``members = arange(T * M).view(T, M)``
    (int32, on the host), the groups of ``mix_pool`` that average a task's M replicas."""
    M = _in_range(M, 1, _lib.MIX_MEMBERS_MAX, "the number of replicas M")
    rep = lambda t: None if t is None else t.repeat_interleave(M, dim=0)
    bm = GPBatch(rep(b.Z_s), rep(b.y_s), rep(b.priors), b.kernel, n_s=rep(b.n_s), ard=b.ard)
    return bm, torch.arange(b.T * M, dtype=torch.int32).view(b.T, M)


def laplace_draws(H, n_s, eps, max_sd: float = 2.0):
    """The offsets ``[T, S, h]`` (float64) of Laplace draws around a MAP point: ``Q diag(lambda^-1/2) eps_s`` with
    ``n_s[t] H[t] = Q diag(lambda) Q^T`` the precision of task t - ``H [T, h, h]`` the Hessian of the per-point objective, which
    is symmetrised here - and ``eps [T, S, h]`` standard normal.  Eigenvalues are floored at ``1 / max_sd^2``: where the posterior
    is flat or H is indefinite a direction has standard deviation ``max_sd``.  Pure torch; runs on CPU tensors."""
    H = torch.as_tensor(H, dtype=torch.float64)
    eps = torch.as_tensor(eps, dtype=torch.float64)
    if H.dim() != 3 or H.shape[1] != H.shape[2]:
        raise ValueError(f"H must be [T, h, h], got {tuple(H.shape)}")
    T, h = H.shape[0], H.shape[1]
    if eps.dim() != 3 or eps.shape[0] != T or eps.shape[2] != h:
        raise ValueError(f"eps must be [T, S, h] = [{T}, S, {h}], got {tuple(eps.shape)}")
    n = torch.as_tensor(n_s, dtype=torch.float64).reshape(-1)
    if n.numel() != T:
        raise ValueError(f"n_s must have T = {T} entries, got {n.numel()}")
    if not max_sd > 0:
        raise ValueError(f"max_sd must be positive, got {max_sd}")
    P = 0.5 * (H + H.transpose(1, 2)) * n.view(T, 1, 1)
    lam, Q = torch.linalg.eigh(P)
    lam = lam.clamp_min(1.0 / (max_sd * max_sd))
    return torch.einsum("tij,tsj->tsi", Q, eps * lam.rsqrt().unsqueeze(1))


def hessian_by_differences(grad, phi, step: float):
    """``H [T, h, h]`` (float64, symmetrised) of a batch of objectives by central differences of their exact gradient:
    ``grad(phi [T, h]) -> [T, h]`` is called 2 h times, all tasks at once; column j is ``(grad(phi + step e_j) - grad(phi -
    step e_j)) / (2 step)``.  Pure torch; ``phi`` keeps its dtype and device for the calls."""
    T, h = phi.shape
    H = torch.empty(T, h, h, dtype=torch.float64)
    for j in range(h):
        e = torch.zeros(h, dtype=phi.dtype, device=phi.device)
        e[j] = step
        # the step that was taken, not the one asked for: phi + e rounds
        gp, gm = grad(phi + e), grad(phi - e)
        dx = ((phi + e) - (phi - e))[:, j].double().cpu()
        H[:, :, j] = (gp.double().cpu() - gm.double().cpu()) / dx.unsqueeze(1)
    return 0.5 * (H + H.transpose(1, 2))


LAPLACE_STEP = 1e-2


def phi_laplace_samples(b: GPBatch, phi: torch.Tensor, n_samples: int, *, generator: Optional[torch.Generator] = None, eps=None,
                        step: float = LAPLACE_STEP, max_sd: float = 2.0, keep_map: bool = True) -> torch.Tensor:
    """``phi [T, n_samples, 3]``: draws from the Laplace approximation of the posterior over the hyperparameters around the MAP
    point ``phi [T, 3]`` of ``fit``, for isotropic batches.  The Hessian of the per-point objective comes from central differences
    of ``mll_value_grad``'s exact gradient (6 evaluations, all tasks at once; ``hessian_by_differences``); the objective is divided
    by the number of points after the priors are added, so the precision is ``n_s[t] H``.  The draws are made in float64 on the
    host (``laplace_draws``: eigenvalues floored at ``1 / max_sd^2``) from ``eps [T, n_samples, 3]``, or from ``generator``.
    ``keep_map``: draw 0 is ``phi`` itself.
    ``step``: on the 31 golden ``gp_*`` fixtures the differenced Hessian of the CPU twin's ``adkf_mll_value_grad`` is within
    ``max |H_d - H| / max |H|`` = 1.2e-5, 4.4e-6, 2.7e-5, 1.1e-4, 6.8e-4 and 2.7e-3 (worst fixture) of the ``H`` of its
    ``adkf_ift_hypergrad`` at steps 1e-3, 3e-3, 1e-2, 2e-2, 5e-2 and 1e-1.  The twin's gradient is a float64 value rounded once; the
    device's is float32 arithmetic, whose rounding error is divided by the step, so the default is 1e-2, one notch above the twin's
    optimum: 2.7e-5 of truncation error, far below what the eigenvalue floor and the Laplace approximation itself leave."""
    if b.ard:
        raise ValueError("phi_laplace_samples covers isotropic batches only: the Laplace Hessian of an ARD batch (2 + d by 2 + d per "
                         "task, 2 (2 + d) gradient evaluations) is not built")
    n_samples = _in_range(n_samples, 1, _lib.MIX_MEMBERS_MAX, "n_samples")
    phi = b.check_phi(phi)
    T = b.T
    if eps is None:
        eps = torch.randn(T, n_samples, 3, dtype=torch.float64, generator=generator)
    H = hessian_by_differences(lambda p: mll_value_grad(b, p)[1], phi, step)
    n = torch.full((T,), b.ns) if b.n_s is None else b.n_s.cpu()
    off = laplace_draws(H, n, eps, max_sd)
    if keep_map:
        off[:, 0] = 0.0
    return (phi.double().cpu().unsqueeze(1) + off).float().to(b.device)


def gumbel_pool(b: GPBatch, phi: torch.Tensor, X: torch.Tensor, *, n_samples: Optional[int] = None, u: Optional[torch.Tensor] = None,
                generator: Optional[torch.Generator] = None, maximize: bool = False):
    """Gumbel max-value sampling (Wang & Jegelka 2017, section 3.1; BoTorch's ``_sample_max_value_Gumbel``) over the shared pool
    ``X [rows, d]`` in one ``adkf_gumbel_pool`` call, for isotropic and ARD batches alike: samples of each task's optimum value as
    ``mes_pool`` takes them, from the pool's posterior marginals alone (no random-Fourier basis).  The marginals are taken as
    independent; the quartiles of ``Pr[max < z] = prod_i Phi((z - m_i) / sigma_i)`` are found by two passes of 64 probes, a Gumbel
    ``(a, b)`` is fitted to them and ``ystar = a - b log(-log u)`` is drawn.  Returns ``dict(ystar [T, S], quant [T, 3],
    gumbel [T, 2], u [T, S], info [T])``: ``ystar`` holds samples of max f with ``maximize`` and of min f without; ``quant`` (the
    quartiles) and ``gumbel`` (a, b) are in the score's sense, of +f with ``maximize`` and of -f without.  ``u`` (uniforms in (0, 1),
    on the batch's device) is given, or ``n_samples`` (at most 64) of them per task are drawn here from ``generator`` (on its device)
    and returned.  Skipped tasks and an empty pool give -inf in ``quant`` and ``gumbel`` and -inf / +inf in ``ystar``.  A task's
    result is the same bits alone or in a batch, and under any permutation of the pool's rows."""
    lib = _lib.load()
    _support_only(b, "gumbel_pool")
    if u is None:
        if n_samples is None:
            raise ValueError("gumbel_pool needs n_samples or u")
        S = _in_range(n_samples, 1, _lib.TS_SAMPLES_MAX, "n_samples")
    else:
        S = _sample_table(b, u, "u", "the number of samples")
        if n_samples is not None and int(n_samples) != S:
            raise ValueError(f"n_samples = {n_samples} does not match u [T, {S}]")
    phi, X = _phi_and_pool(b, phi, X)
    if u is None:
        gdev = generator.device if generator is not None else b.device
        u = torch.rand(b.T, S, dtype=torch.float32, generator=generator, device=gdev).to(b.device).contiguous()
    else:
        u = _f32(u, "u")
    _on_device(b, X=X, u=u)
    ystar, quant, gumbel = _new(b, b.T, S), _new(b, b.T, 3), _new(b, b.T, 2)
    info = _new(b, b.T, dtype=torch.int32)
    args = (ptr(u), S, ptr(ystar), ptr(quant), ptr(gumbel))
    _pool_call(lib, "adkf_gumbel_pool", b, phi, _lib.PM_MAXIMIZE if maximize else 0, X, args, info, lib.adkf_gumbel_pool_scratch_bytes(b.T))
    return dict(ystar=ystar, quant=quant, gumbel=gumbel, u=u, info=info)


def double_path_tasks(b: GPBatch) -> torch.Tensor:
    """[T] int32: 1 where the last ``ift_hypergrad`` / ``outer_nll_value_grad`` on this batch sent the task through the float64
    path (ill-conditioned tasks, csrc/refine64.h).  Diagnostic."""
    lib = _lib.load()
    flagged = _new(b, b.T, dtype=torch.int32)
    ws, nb = b.workspace()
    cb = b.c_struct()
    _lib.check(lib.adkf_double_path_tasks(C.byref(cb), ptr(flagged), ptr(ws), nb, stream(b.device)), "adkf_double_path_tasks")
    return flagged


def outer_nll_value_grad(b: GPBatch, phi: torch.Tensor, want_grads=True):
    lib = _lib.load()
    phi = b.check_phi(phi)
    f = _new(b, b.T)
    g = _new(b, b.T, b.h) if want_grads else None
    dZs = _new(b, b.T, b.ns, b.d) if want_grads else None
    dZq = _new(b, b.T, b.nq, b.d) if want_grads else None
    info = _new(b, b.T, dtype=torch.int32)
    ws, nb = b.workspace()
    cb = b.c_struct()
    _lib.check(lib.adkf_outer_nll_value_grad(C.byref(cb), ptr(phi), ptr(f), ptr(g), ptr(dZs), ptr(dZq), ptr(info),
                                             ptr(ws), nb, stream(b.device)), "adkf_outer_nll_value_grad")
    return f, g, dZs, dZq, info


def ift_hypergrad(b: GPBatch, phi: torch.Tensor, ignore_grad_correction=False, ignore_direct_grad=False, out_dZ=None,
                  cg_maxiter: Optional[int] = None, cg_tol: float = 1e-6):
    """Returns dict(f_out, dZ_s, dZ_q, g_phi, v, H, info): the IFT hypergradient at the feature level.
    ``out_dZ = (dZ_s, dZ_q)``: optional preallocated contiguous float32 outputs (e.g. two halves of one buffer).
    ARD batches: H is None (never formed), ``cg_iters`` reports the conjugate-gradient iterations per task."""
    lib = _lib.load()
    phi = b.check_phi(phi)
    flags = (_lib.IGNORE_GRAD_CORRECTION if ignore_grad_correction else 0) | (_lib.IGNORE_DIRECT_GRAD if ignore_direct_grad else 0)
    if out_dZ is not None:
        dZ_s, dZ_q = out_dZ
        assert dZ_s.is_contiguous() and dZ_q.is_contiguous() and dZ_s.dtype == torch.float32 and dZ_q.dtype == torch.float32
        assert dZ_s.shape == b.Z_s.shape and dZ_q.shape == b.Z_q.shape
    else:
        dZ_s, dZ_q = _new(b, b.T, b.ns, b.d), _new(b, b.T, b.nq, b.d)
    ws, nb = b.workspace()
    cb = b.c_struct()
    if b.ard:
        out = dict(f_out=_new(b, b.T), dZ_s=dZ_s, dZ_q=dZ_q, g_phi=_new(b, b.T, b.h), v=_new(b, b.T, b.h), H=None,
                   info=_new(b, b.T, dtype=torch.int32), cg_iters=_new(b, b.T, dtype=torch.int32))
        _lib.check(lib.adkf_ift_hypergrad_cg(C.byref(cb), ptr(phi), flags, int(cg_maxiter or 48), float(cg_tol), ptr(out["f_out"]),
                                             ptr(dZ_s), ptr(dZ_q), ptr(out["g_phi"]), ptr(out["v"]), ptr(out["cg_iters"]),
                                             ptr(out["info"]), ptr(ws), nb, stream(b.device)), "adkf_ift_hypergrad_cg")
        return out
    out = dict(f_out=_new(b, b.T), dZ_s=dZ_s, dZ_q=dZ_q, g_phi=_new(b, b.T, 3),
               v=_new(b, b.T, 3), H=_new(b, b.T, 9), info=_new(b, b.T, dtype=torch.int32))
    _lib.check(lib.adkf_ift_hypergrad(C.byref(cb), ptr(phi), flags, ptr(out["f_out"]), ptr(out["dZ_s"]), ptr(out["dZ_q"]),
                                      ptr(out["g_phi"]), ptr(out["v"]), ptr(out["H"]), ptr(out["info"]), ptr(ws), nb,
                                      stream(b.device)), "adkf_ift_hypergrad")
    out["H"] = out["H"].view(b.T, 3, 3)
    return out
