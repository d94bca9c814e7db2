"""The Bayesian-optimisation caller of the same GP op: ``create_gp`` + the GP-EI loop of
bayes_opt/bo_utils.py:342-455, on the HIP library.  The GP is fitted on the queried points, Expected Improvement is
evaluated for EVERY candidate with one ``adkf_predict`` call (the reference loops over candidates one by one).  Candidate
pools beyond ``adkf_max_points()`` rows - or any pool with ``streaming=True`` - go through ``adkf_predict_marginal``, the
streaming marginal prediction (no size cap, workspace independent of the pool size); ``run_gp_ei_bo(streaming=True)`` then
gets EI straight from that one call.  ``run_gp_ei_bo_batched`` runs many replicates of that loop over the same pool at once: one
batched fit and one ``adkf_predict_pool`` call per iteration, which returns each replicate's best candidates itself (or one
``adkf_believer_pool`` call for a Kriging-believer batch; with ``ard=True`` the batch is an ARD batch and that call is
``adkf_believer_pool_ard``; ``batch="liar"``: one ``adkf_liar_pool`` call for a constant-liar batch).  With ``refit_every=r`` it
refits every ``r`` iterations and plays the iterations in between, at fixed hyperparameters, with one ``adkf_liar_pool`` call on the
pool's label table.
``run_gp_ts_bo_batched`` is the same loop under Thompson sampling: one batched fit and one ``adkf_thompson_pool`` call (with
``ard=True``: ``adkf_thompson_pool_ard``) per iteration, in which every replicate draws posterior functions over the whole pool
and each function picks its own best candidate - a diverse batch of ``query_batch_size > 1`` picks from one pass, with no
``best_f`` and nothing that can underflow.  Both EI loops take ``acquisition="log_ei"``: the same candidates ranked by log EI
(``ADKF_PM_LOG_EI``), which stays finite where float32 EI is 0 on the whole pool and the ``"ei"`` loops fall back to random picks.
``run_gp_qei_bo_batched`` is the loop under Monte-Carlo q-EI: one batched fit and one ``adkf_qei_pool`` call per iteration, which scores
the ``query_batch_size`` picks jointly over pathwise posterior draws and, by default, against each draw's own best value at the
queried points (noisy q-EI) instead of the best observed label.
``run_gp_mes_bo_batched`` is the loop under max-value entropy search: one batched fit, one ``gp_ops.max_value_samples`` call (the
minima of pathwise posterior draws over the whole pool) and one ``adkf_mes_pool`` call per iteration, with no ``best_f`` in the score.
``run_gp_kg_bo_batched`` is the loop under the knowledge gradient for correlated beliefs: one batched fit, one mean top-``n_refs`` call
for the reference rows and one ``adkf_kg_pool`` call (log KG) per iteration; it prices the observation noise and needs no ``best_f``.
``run_gp_jes_bo_batched`` is the loop under joint entropy search: one batched fit, one ``gp_ops.optimum_samples`` call (the minima of
pathwise posterior draws over the whole pool, location and value) and one ``adkf_jes_pool`` call per iteration.
``run_gp_ipv_al_batched`` is not an optimisation loop but the active-learning one: one batched fit and one ``adkf_ipv_pool`` call per
round, which returns the batch of rows whose labels lower the posterior variance at given target rows the most.

Only the Matern-5/2 branch exists here (the Tanimoto kernel of the reference's fingerprint baseline is not a
distance-based kernel and is out of the library's scope).
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import gp_ops
from .models import ExactGPLayer, ExactMarginalLogLikelihood, GaussianLikelihood, fit_gpytorch_scipy


def compute_median_lengthscale_init(gp_input: torch.Tensor) -> torch.Tensor:
    """bo_utils.py:458-461 (same median heuristic as the model's)."""
    b = gp_ops.GPBatch(gp_input.detach()[None].float().contiguous(), torch.zeros(1, gp_input.shape[0], device=gp_input.device),
                       torch.zeros(1, 4, device=gp_input.device), gp_ops.KERNEL_RBF)
    return gp_ops.median_lengthscale(b)[0]


def create_gp(train_x: torch.Tensor, train_y: torch.Tensor, kernel_type: str, device, noise_init: float, noise_prior: bool):
    """bo_utils.py:423-455: (likelihood, model, mll) with noise initialised at ``noise_init`` (optionally under a
    LogNormal prior with that mode) and a Matern-5/2 kernel whose lengthscale starts at, and has its prior mode at, the
    median heuristic of ``train_x``."""
    if kernel_type != "matern":
        raise ValueError(f"kernel_type {kernel_type!r}: only 'matern' is available on the HIP path")
    scale = 0.25
    prior = (math.log(noise_init) + scale ** 2, scale) if noise_prior else None
    likelihood = GaussianLikelihood(noise_prior=prior).to(device)
    model = ExactGPLayer(train_x, train_y, likelihood, "matern").to(device)
    likelihood.noise = noise_init
    l0 = compute_median_lengthscale_init(train_x)
    bk = model.covar_module.base_kernel
    bk.register_prior("lengthscale_prior", (torch.log(l0).item() + scale ** 2, scale))
    bk.lengthscale = torch.ones_like(bk.lengthscale) * l0
    mll = ExactMarginalLogLikelihood(likelihood, model).to(device)
    return likelihood, model, mll


def _support_batch(model: ExactGPLayer, mll: ExactMarginalLogLikelihood):
    Z = model.train_inputs[0].detach().float().contiguous()
    y = model.train_targets.detach().float().contiguous()
    b = gp_ops.GPBatch(Z[None], y[None], mll.priors_row(Z.device), model.kernel_id, ard=model.ard)
    phi = torch.cat([p.detach().reshape(-1) for p in mll.raw_params()])[None]
    return b, phi


@torch.no_grad()
def streaming_posterior(model: ExactGPLayer, mll: ExactMarginalLogLikelihood, X: torch.Tensor, best_f: Optional[float] = None,
                        maximize: bool = False, log_ei: bool = False):
    """(mean, latent variance, EI or None) at every row of X in ONE ``adkf_predict_marginal`` call, for pools of any size.
    ``log_ei`` (needs ``best_f``): log EI in the place of EI."""
    b, phi = _support_batch(model, mll)
    X = X.detach().float().contiguous()
    q_off = torch.tensor([0, X.shape[0]], dtype=torch.int64, device=X.device)
    bf = None if best_f is None else torch.full((1,), float(best_f), dtype=torch.float32, device=X.device)
    mean, var, ei, info = gp_ops.predict_marginal(b, phi, X, q_off, latent=True, best_f=bf, maximize=maximize, log_ei=log_ei)
    gp_ops.check_info(info, "BO posterior")
    return mean, var.clamp_min(1e-12), ei


@torch.no_grad()
def latent_posterior(model: ExactGPLayer, mll: ExactMarginalLogLikelihood, X: torch.Tensor,
                     streaming: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Mean and variance of the LATENT function at X (``model.posterior(X)`` without observation noise, which is what
    BoTorch's analytic acquisition functions read).  ``streaming``: True - ``adkf_predict_marginal``; False - ``adkf_predict``
    (the joint path, at most ``adkf_max_points()`` rows); None - streaming only when X has more rows than that."""
    if streaming is None:
        streaming = X.shape[0] > gp_ops._lib.load().adkf_max_points()
    if streaming:
        mean, var, _ = streaming_posterior(model, mll, X)
        return mean, var
    Z = model.train_inputs[0].detach().float().contiguous()
    y = model.train_targets.detach().float().contiguous()
    b = gp_ops.GPBatch(Z[None], y[None], mll.priors_row(Z.device), model.kernel_id, Z_q=X.detach().float().contiguous()[None],
                       ard=model.ard)
    phi = torch.cat([p.detach().reshape(-1) for p in mll.raw_params()])[None]
    mean, var, _, info = gp_ops.predict(b, phi, want_var=True)
    gp_ops.check_info(info, "BO posterior")
    noise = model.likelihood.noise.detach().reshape(())
    return mean[0], (var[0] - noise).clamp_min(1e-12)


def expected_improvement(mean: torch.Tensor, var: torch.Tensor, best_f: float, maximize: bool = False) -> torch.Tensor:
    """botorch.acquisition.analytic.ExpectedImprovement: sigma * (u Phi(u) + phi(u)), u = +-(mean - best_f) / sigma."""
    sigma = var.sqrt()
    u = (mean - best_f) / sigma
    if not maximize:
        u = -u
    normal = torch.distributions.Normal(torch.zeros_like(u), torch.ones_like(u))
    return sigma * (u * normal.cdf(u) + torch.exp(normal.log_prob(u)))


def log_expected_improvement(mean: torch.Tensor, var: torch.Tensor, best_f: float, maximize: bool = False) -> torch.Tensor:
    """log of ``expected_improvement`` without passing through it (botorch's LogExpectedImprovement; Ament et al. 2023):
    log sigma + log h(u), h(u) = phi(u) + u Phi(u), finite for any u.  In float64 whatever the input dtype, which the result
    has: h itself for u > -1; below, with a = -u, h = phi(u) (1 - a sqrt(pi / 2) erfcx(a / sqrt 2)) down to u = -30 (the bracket
    cancels to ~1 / a^2: an absolute error of a few eps64 a^2) and beyond that its asymptotic series
    a^-2 (1 - 3 a^-2 + 15 a^-4 - ...), eight terms.  The host restatement of ``ADKF_PM_LOG_EI``."""
    sigma = var.double().sqrt()
    u = (mean.double() - best_f) / sigma
    if not maximize:
        u = -u
    a = -u
    direct = torch.log(torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi) + u * 0.5 * torch.erfc(-u / math.sqrt(2.0)))
    mid = torch.log1p(-a * math.sqrt(math.pi / 2.0) * torch.special.erfcx(a / math.sqrt(2.0)))
    w = 1.0 / (a * a)
    series = torch.zeros_like(w)
    for c in (34459425.0, -2027025.0, 135135.0, -10395.0, 945.0, -105.0, 15.0, -3.0):   # (-1)^k (2k + 1)!!, k = 8 .. 1 (Horner)
        series = (series + c) * w
    tail = torch.log(w) + torch.log1p(series)
    log_h = torch.where(u > -1.0, direct, -0.5 * a * a - 0.5 * math.log(2.0 * math.pi) + torch.where(u > -30.0, mid, tail))
    return (sigma.log() + log_h).to(mean.dtype)


def _acquisition(acquisition: str) -> bool:
    """True for "log_ei", False for "ei"."""
    if acquisition not in ("ei", "log_ei"):
        raise ValueError(f"acquisition must be 'ei' or 'log_ei', got {acquisition!r}")
    return acquisition == "log_ei"


def run_gp_ei_bo(x_all: torch.Tensor, y_all: torch.Tensor, num_init_points: int, query_batch_size: int, num_bo_iters: int,
                 kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                 rng: Optional[np.random.Generator] = None, streaming: bool = False, acquisition: str = "ei") -> List[int]:
    """bo_utils.py:342-397 (minimisation; points sorted by ascending y).  Returns the BO record: the best initial index
    followed by the queried indices in the order the reference appends them.  ``streaming``: EI of the whole pool from one
    ``adkf_predict_marginal`` call (no pool-size cap).  ``acquisition``: ``"ei"`` (the reference's: a candidate counts when its EI
    is positive, and random picks fill in for the rest - all of them once float32 EI has underflowed on the pool) or
    ``"log_ei"`` (the same ranking on log EI; a candidate counts when its score is finite, so a pool with finite predictions
    never needs the random fallback)."""
    log = _acquisition(acquisition)
    rng = rng or np.random.default_rng()
    n = x_all.shape[0]
    y_all = (y_all - y_all.mean()) / y_all.std()
    queried = rng.choice(np.arange(init_from, n), size=num_init_points, replace=False).tolist()
    record = [min(queried)]
    for _ in range(num_bo_iters):
        xq, yq = x_all[queried], y_all[queried]
        best = yq.min().item()
        likelihood, model, mll = create_gp(xq, yq, kernel_type, device, noise_init, noise_prior)
        fit_gpytorch_scipy(mll)
        if streaming:
            acq = streaming_posterior(model, mll, x_all, best_f=best, maximize=False, log_ei=log)[2].cpu()
        else:
            mean, var = latent_posterior(model, mll, x_all)
            acq = (log_expected_improvement if log else expected_improvement)(mean, var, best, maximize=False).cpu()
        acq[queried] = -float("inf")
        if log:   # usable: a finite score
            acq[~torch.isfinite(acq)] = -float("inf")
            nonzero = int((acq > -float("inf")).sum())
        else:
            nonzero = int((acq > 0).sum())
        free = lambda taken: [i for i in range(n) if i not in taken]
        if nonzero == 0:
            pick = rng.choice(free(queried), size=query_batch_size, replace=False).tolist()
        elif nonzero < query_batch_size:
            pick = torch.topk(acq, query_batch_size).indices[:nonzero].tolist()
            pick += rng.choice(free(queried + pick), size=query_batch_size - nonzero, replace=False).tolist()
        else:
            pick = torch.topk(acq, query_batch_size).indices.tolist()
        queried = list(set(queried + pick))
        record.extend(pick[::-1])
    return record


def _bo_start(x_all: torch.Tensor, y_all: torch.Tensor, num_init_points: int, init_from: int, rngs, dim=None):
    """The start of a batched loop: ``y_all`` standardised (``dim=0``: each column), the pool as float32 and each replicate's initial
    design, drawn from its own generator.  Returns ``(y_all, X, queried)``."""
    y_all = (y_all - y_all.mean(dim)) / y_all.std(dim)
    X = x_all.detach().float().contiguous()
    queried = [rng.choice(np.arange(init_from, x_all.shape[0]), size=num_init_points, replace=False).tolist() for rng in rngs]
    return y_all, X, queried


def _fit_tasks(name: str, x_all: torch.Tensor, tasks, X: torch.Tensor, kernel_type: str, device, noise_init: float, noise_prior: bool,
               ard: bool):
    """ONE batch of the tasks ``(indices, target column)`` - initial parameters and priors as ``create_gp`` makes them for each, with
    ``ard`` the lengthscale expanded to one per feature dimension - fitted by ONE ``gp_ops.fit``.  Returns ``(b, phi)``, the batch
    flagged to reuse the fit's distances and inner quantities."""
    sizes = [len(q) for q, _ in tasks]
    ns = max(sizes)
    Zs = torch.zeros(len(tasks), ns, X.shape[1], dtype=torch.float32, device=X.device)
    ys = torch.zeros(len(tasks), ns, dtype=torch.float32, device=X.device)
    pri, phi0 = [], []
    for t, (q, y) in enumerate(tasks):
        _, model, mll = create_gp(x_all[q], y[q], kernel_type, device, noise_init, noise_prior)
        Zs[t, :sizes[t]] = model.train_inputs[0].detach().float()
        ys[t, :sizes[t]] = model.train_targets.detach().float()
        pri.append(mll.priors_row(X.device))
        p0 = torch.cat([p.detach().reshape(-1) for p in mll.raw_params()])
        phi0.append((torch.cat([p0[:2], p0[2:3].expand(X.shape[1])]) if ard else p0)[None])
    n_s = None if min(sizes) == ns else torch.tensor(sizes, dtype=torch.int32)
    b = gp_ops.GPBatch(Zs, ys, torch.cat(pri), model.kernel_id, n_s=n_s, ard=ard or model.ard)
    phi, _, _, _, info = gp_ops.fit(b, torch.cat(phi0))
    gp_ops.check_info(info, f"{name} fit")
    b.flags |= gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    return b, phi


def _path_generators(rngs) -> List[torch.Generator]:
    """One torch generator per replicate, seeded from the replicate's own generator."""
    return [torch.Generator().manual_seed(int(rng.integers(0, 2 ** 62))) for rng in rngs]


def _pathwise_draws(gens, S: int, n_features: int, queried, device):
    """The prior weights ``w [R, S, m]`` and noise draws ``eps [R, S, ns]`` of a pathwise posterior draw, replicate r's from ``gens[r]``,
    the noise draws at the replicate's own support size (zeros beyond it)."""
    sizes = [len(q) for q in queried]
    w = torch.empty(len(gens), S, n_features, dtype=torch.float32)
    eps = torch.zeros(len(gens), S, max(sizes), dtype=torch.float32)
    for r, g in enumerate(gens):
        w[r] = torch.randn(S, n_features, generator=g)
        eps[r, :, :sizes[r]] = torch.randn(S, sizes[r], generator=g)
    return w.to(device), eps.to(device)


def _take_picks(top_idx: torch.Tensor, usable: torch.Tensor, query_batch_size: int, rngs, queried, records, n: int,
                reverse: bool = False) -> None:
    """The end of an iteration of the batched loops: replicate r takes the usable prefix of its
    candidates ``top_idx[r]`` (``usable[r]``: a prefix mask), fills a shortfall with random rows it has not queried, drawn from its own
    generator ``rngs[r]``, and adds the picks to ``queried[r]`` and ``records[r]`` (both updated in place; ``reverse``: to the record in
    reverse order, as ``run_gp_ei_bo`` appends them)."""
    for r, rng in enumerate(rngs):
        nonzero = int(usable[r].sum())
        pick = top_idx[r, :nonzero].tolist()
        if nonzero < query_batch_size:
            taken = set(queried[r] + pick)
            pick += rng.choice([i for i in range(n) if i not in taken], size=query_batch_size - nonzero, replace=False).tolist()
        queried[r] = list(set(queried[r] + pick))
        records[r].extend(pick[::-1] if reverse else pick)


@torch.no_grad()
def run_gp_ei_bo_batched(x_all: torch.Tensor, y_all: torch.Tensor, num_init_points: int, query_batch_size: int, num_bo_iters: int,
                         kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                         rngs: List[np.random.Generator], acquisition: str = "ei", batch: str = "topk",
                         ard: bool = False, marginalize: int = 0, lie="min", refit_every: int = 1) -> List[List[int]]:
    """``len(rngs)`` replicates of ``run_gp_ei_bo`` over the same pool at once; returns their records.  Per iteration the
    replicates' queried sets form ONE batch (initial parameters and priors as ``create_gp`` makes them for each), fitted by ONE
    ``gp_ops.fit`` with ``fit_gpytorch_scipy``'s options and scored by ONE ``gp_ops.predict_pool`` call that excludes each
    replicate's queried points and returns its ``query_batch_size`` best candidates: no EI vector ever exists.  Every replicate
    draws from its own generator in the order the sequential loop does.  ``acquisition``: as ``run_gp_ei_bo``; with ``"log_ei"``
    the call ranks by log EI and a returned candidate counts when its score is finite and its index is not -1.
    ``batch``: ``"topk"`` takes the ``query_batch_size`` rows of largest EI, as the sequential loop does (they tend to be
    neighbours of the winner); ``"believer"`` takes the Kriging-believer batch of ONE ``gp_ops.believer_pool`` call instead -
    sequential-greedy EI in which every pick is believed at its posterior mean - under the same rule for what counts.  With
    ``query_batch_size = 1`` the two are the same loop.
    ``ard``: one lengthscale per feature dimension (the reference's ``ard_num_dims``) - each replicate's ``create_gp`` start is
    expanded to ``[2 + d]`` as ``run_gp_ts_bo_batched(ard=True)`` expands it; the batch is an ARD batch, which ``predict_pool``
    takes as it is and for which ``"believer"`` calls ``gp_ops.believer_pool_ard``.
    ``marginalize``: 0 scores at the MAP point of the fit.  ``M >= 2`` (at most 64, ``batch="topk"``, isotropic) integrates the
    acquisition over the hyperparameters (Snoek et al. 2012): after the fit each replicate draws ``M - 1`` Laplace samples of its
    ``phi`` from a torch generator of its own (``gp_ops.phi_laplace_samples``; member 0 is the MAP point), the batch is replicated M
    times (``gp_ops.replicate_batch``) and ONE ``gp_ops.mix_pool`` call ranks the pool by the members' average EI (or by its
    logarithm) per replicate, under the same exclusions and the same rule for what counts.
    ``batch="liar"``: the constant-liar batch of ONE ``gp_ops.liar_pool`` call - the believer's loop with every pick conditioned on
    ``lie`` (``"min"``, ``"max"``, ``"mean"`` of the replicate's own labels, or a tensor with one value per replicate) instead of on
    its posterior mean, under the believer's rule for what counts.  With ``query_batch_size = 1`` it is the ``"topk"`` loop.
    ``refit_every``: 1 refits the hyperparameters in every iteration.  ``r > 1`` (``query_batch_size = 1``, no ``marginalize``)
    refits every ``r`` iterations: each fit is followed by ONE ``gp_ops.liar_pool`` call that plays ``min(r, iterations left)``
    iterations at the fitted ``phi`` - each step picks by EI, reads the pick's true label from ``y_all``, updates mean, variance
    and incumbent - and its picks extend the records as that many iterations would: the usable prefix counts, random free rows
    fill the rest."""
    log = _acquisition(acquisition)
    if batch not in ("topk", "believer", "liar"):
        raise ValueError(f"batch must be 'topk', 'believer' or 'liar', got {batch!r}")
    refit_every = int(refit_every)
    if refit_every < 1:
        raise ValueError(f"refit_every must be at least 1, got {refit_every}")
    if refit_every > 1 and query_batch_size != 1:
        raise ValueError("refit_every > 1 needs query_batch_size = 1: the replay plays single-pick iterations")
    if refit_every > 1 and marginalize:
        raise ValueError("refit_every > 1 needs marginalize = 0: the replay conditions one model, not a mixture")
    marginalize = int(marginalize)
    if marginalize == 1 or not 0 <= marginalize <= 64:
        raise ValueError(f"marginalize must be 0 or in [2, 64], got {marginalize}")
    if marginalize and batch != "topk":
        raise ValueError("marginalize needs batch='topk': the believer's greedy steps condition one model, not a mixture")
    if marginalize and ard:
        raise ValueError("marginalize needs ard=False: the Laplace samples cover isotropic batches only")
    n = x_all.shape[0]
    y_all, X, queried = _bo_start(x_all, y_all, num_init_points, init_from, rngs)
    records = [[min(q)] for q in queried]
    gens = _path_generators(rngs) if marginalize else None

    labels = y_all.detach().float().to(X.device).contiguous() if refit_every > 1 else None
    done = 0
    while done < num_bo_iters:
        steps = min(refit_every, num_bo_iters - done) if refit_every > 1 else 1
        done += steps
        b, phi = _fit_tasks("run_gp_ei_bo_batched", x_all, [(q, y_all) for q in queried], X, kernel_type, device, noise_init, noise_prior,
                            ard)
        best_f = torch.tensor([y_all[q].min().item() for q in queried], dtype=torch.float32, device=X.device)
        if refit_every > 1:
            out = gp_ops.liar_pool(b, phi, X, best_f=best_f, q=steps, labels=labels, maximize=False, log_ei=log, exclude=queried)
            gp_ops.check_info(out["info"], "BO posterior")
            top_idx, top_val = out["sel_idx"].cpu(), out["sel_val"].cpu()
            usable = (torch.isfinite(top_val) & (top_idx >= 0)) if log else top_val > 0
            _take_picks(top_idx, usable.long().cumprod(1).bool(), steps, rngs, queried, records, n)
            continue
        if batch == "liar":
            out = gp_ops.liar_pool(b, phi, X, best_f=best_f, q=query_batch_size, lie=lie, maximize=False, log_ei=log, exclude=queried)
            top_idx, top_val = out["sel_idx"].cpu(), out["sel_val"].cpu()
        elif batch == "believer":
            believe = gp_ops.believer_pool_ard if b.ard else gp_ops.believer_pool
            out = believe(b, phi, X, best_f=best_f, q=query_batch_size, maximize=False, log_ei=log, exclude=queried)
            top_idx, top_val = out["sel_idx"].cpu(), out["sel_val"].cpu()
        elif marginalize:
            M = marginalize
            b.flags &= ~gp_ops.REUSE_INNER   # the sampler evaluates the gradient away from the fit's phi
            eps = torch.stack([torch.randn(M, 3, dtype=torch.float64, generator=g) for g in gens])
            phis = gp_ops.phi_laplace_samples(b, phi, M, eps=eps)
            bm, members = gp_ops.replicate_batch(b, M)
            out = gp_ops.mix_pool(bm, phis.reshape(-1, 3), X, members=members, best_f=best_f.repeat_interleave(M),
                                  score="log_ei" if log else "ei", latent=True, maximize=False, want_mean=False, want_var=False,
                                  want_score=False, topk=query_batch_size, exclude=queried)
            top_idx, top_val = out["top_idx"].cpu(), out["top_val"].cpu()
        else:
            out = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best_f, maximize=False, want_mean=False, want_var=False,
                                      want_ei=False, topk=query_batch_size, exclude=queried, log_ei=log)
            top_idx, top_val = out["top_idx"].cpu(), out["top_val"].cpu()
        gp_ops.check_info(out["info"], "BO posterior")
        usable = (torch.isfinite(top_val) & (top_idx >= 0)) if log else top_val > 0   # (a prefix of each row: descending scores)
        if batch in ("believer", "liar"):   # a believer score can round above its predecessor: keep the prefix
            usable = usable.long().cumprod(1).bool()
        _take_picks(top_idx, usable, query_batch_size, rngs, queried, records, n, reverse=True)
    return records


@torch.no_grad()
def run_gp_ts_bo_batched(x_all: torch.Tensor, y_all: torch.Tensor, num_init_points: int, query_batch_size: int, num_bo_iters: int,
                         kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                         rngs: List[np.random.Generator], n_features: int = 1024, oversample: int = 4,
                         feature_seed: int = 0, ard: bool = False) -> List[List[int]]:
    """``len(rngs)`` replicates of a Thompson-sampling BO loop over the same pool at once (minimisation, as ``run_gp_ei_bo``);
    returns their records: the best initial index, then the picks in pick order.  Per iteration the replicates' queried sets are
    fitted by ONE ``gp_ops.fit`` (as ``run_gp_ei_bo_batched``) and ONE ``gp_ops.thompson_pool`` call draws
    ``S = min(64, query_batch_size * oversample)`` posterior functions per replicate on a random-Fourier basis of ``n_features``
    features (drawn once from ``feature_seed``), each function picking its best row among those the replicate has not queried.  A
    replicate takes the first ``query_batch_size`` distinct picks in sample order; a shortfall is filled with random free rows from
    its generator.  The prior weights and noise draws of replicate r come from a torch generator seeded from ``rngs[r]``, the noise
    draws at the replicate's own support size: a replicate's record does not depend on which other replicates share the batch.
    ``ard``: one lengthscale per feature dimension (the reference's ``ard_num_dims``) - each replicate's ``create_gp`` start is
    expanded to ``[2 + d]``, every lengthscale at the median heuristic (as ARD ``adkf_init_params`` starts), under the same
    priors; the batch is an ARD batch and the draws come from ``gp_ops.thompson_pool_ard``."""
    n = x_all.shape[0]
    if not 1 <= query_batch_size <= gp_ops._lib.TS_SAMPLES_MAX:
        raise ValueError(f"query_batch_size must be in [1, {gp_ops._lib.TS_SAMPLES_MAX}], got {query_batch_size}")
    y_all, X, queried = _bo_start(x_all, y_all, num_init_points, init_from, rngs)
    S = min(gp_ops._lib.TS_SAMPLES_MAX, query_batch_size * max(1, int(oversample)))
    omega, phase = gp_ops.rff_basis(kernel_type, X.shape[1], n_features, generator=torch.Generator().manual_seed(int(feature_seed)),
                                    device=X.device)
    records = [[min(q)] for q in queried]
    gens = _path_generators(rngs)

    def free(taken):
        taken = set(taken)
        return [i for i in range(n) if i not in taken]

    for _ in range(num_bo_iters):
        b, phi = _fit_tasks("run_gp_ts_bo_batched", x_all, [(q, y_all) for q in queried], X, kernel_type, device, noise_init, noise_prior,
                            ard)
        w, eps = _pathwise_draws(gens, S, n_features, queried, X.device)
        draw = gp_ops.thompson_pool_ard if b.ard else gp_ops.thompson_pool
        out = draw(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, maximize=False, exclude=queried)
        gp_ops.check_info(out["info"], "BO posterior")
        sel = out["sel_idx"].cpu().tolist()
        for r, rng in enumerate(rngs):
            pick: List[int] = []
            for i in sel[r]:
                if i >= 0 and i not in pick:
                    pick.append(i)
                if len(pick) == query_batch_size:
                    break
            if len(pick) < query_batch_size:
                pick += rng.choice(free(queried[r] + pick), size=query_batch_size - len(pick), replace=False).tolist()
            queried[r] = list(set(queried[r] + pick))
            records[r].extend(pick)
    return records


@torch.no_grad()
def run_gp_qei_bo_batched(x_all: torch.Tensor, y_all: torch.Tensor, num_init_points: int, query_batch_size: int, num_bo_iters: int,
                          kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                          rngs: List[np.random.Generator], n_samples: int = 128, n_features: int = 1024, noisy: bool = True,
                          feature_seed: int = 0, ard: bool = False) -> List[List[int]]:
    """``len(rngs)`` replicates of a Monte-Carlo q-EI BO loop over the same pool at once (minimisation, as ``run_gp_ei_bo``); returns
    their records: the best initial index, then the picks in pick order.  Per iteration the replicates' queried sets are fitted by ONE
    ``gp_ops.fit`` (as ``run_gp_ei_bo_batched``) and ONE ``gp_ops.qei_pool`` call picks each replicate's ``query_batch_size`` (at most
    64) rows jointly: sequential-greedy q-EI by a sample average over ``n_samples`` (at most 256) pathwise posterior draws on a
    random-Fourier basis of ``n_features`` features (drawn once from ``feature_seed``), among the rows the replicate has not queried.
    ``noisy`` (the default): noisy q-EI - the incumbent of every draw is its own best value over the replicate's queried points, so a
    lucky measurement does not set the bar; otherwise the incumbent is the best observed label.  A pick counts while its score is
    positive (a prefix: the scores of a call never increase); the rest are random free rows from the replicate's generator.  The
    draws of replicate r come from a torch generator seeded from ``rngs[r]`` (``_pathwise_draws``): a replicate's record does not
    depend on which other replicates share the batch.  ``ard``: as ``run_gp_ts_bo_batched``; the call is the same."""
    n = x_all.shape[0]
    if not 1 <= query_batch_size <= gp_ops._lib.QEI_PICKS_MAX:
        raise ValueError(f"query_batch_size must be in [1, {gp_ops._lib.QEI_PICKS_MAX}], got {query_batch_size}")
    if not 1 <= n_samples <= gp_ops._lib.QEI_SAMPLES_MAX:
        raise ValueError(f"n_samples must be in [1, {gp_ops._lib.QEI_SAMPLES_MAX}], got {n_samples}")
    y_all, X, queried = _bo_start(x_all, y_all, num_init_points, init_from, rngs)
    omega, phase = gp_ops.rff_basis(kernel_type, X.shape[1], n_features, generator=torch.Generator().manual_seed(int(feature_seed)),
                                    device=X.device)
    records = [[min(q)] for q in queried]
    gens = _path_generators(rngs)

    for _ in range(num_bo_iters):
        b, phi = _fit_tasks("run_gp_qei_bo_batched", x_all, [(q, y_all) for q in queried], X, kernel_type, device, noise_init, noise_prior,
                            ard)
        w, eps = _pathwise_draws(gens, n_samples, n_features, queried, X.device)
        best_f = None if noisy else torch.tensor([y_all[q].min().item() for q in queried], dtype=torch.float32, device=X.device)
        out = gp_ops.qei_pool(b, phi, X, omega=omega, phase=phase, n_samples=n_samples, q=query_batch_size, best_f=best_f, w=w, eps=eps,
                              maximize=False, exclude=queried)
        gp_ops.check_info(out["info"], "BO posterior")
        top_idx, top_val = out["sel_idx"].cpu(), out["sel_val"].cpu()
        usable = ((top_val > 0) & (top_idx >= 0)).long().cumprod(1).bool()
        _take_picks(top_idx, usable, query_batch_size, rngs, queried, records, n)
    return records


@torch.no_grad()
def run_gp_mes_bo_batched(x_all: torch.Tensor, y_all: torch.Tensor, num_init_points: int, query_batch_size: int, num_bo_iters: int,
                          kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                          rngs: List[np.random.Generator], n_features: int = 1024, oversample: int = 4,
                          feature_seed: int = 0, ard: bool = False, n_max_samples: int = 16,
                          max_value: str = "thompson", batch: str = "topk") -> List[List[int]]:
    """``len(rngs)`` replicates of a max-value entropy search BO loop (Wang & Jegelka 2017) over the same pool at once
    (minimisation, as ``run_gp_ei_bo``); returns their records: the best initial index, then the picks in descending score.  Per
    iteration the replicates' queried sets are fitted by ONE ``gp_ops.fit`` (as ``run_gp_ei_bo_batched``), ONE
    ``gp_ops.max_value_samples`` call draws ``n_max_samples`` (at most 64) samples of each replicate's minimum over the WHOLE pool -
    the minima of pathwise posterior draws on a random-Fourier basis of ``n_features`` features (drawn once from ``feature_seed``) -
    each clamped to be no worse than the replicate's best observed value, and ONE ``gp_ops.mes_pool`` call scores the pool and
    returns each replicate's ``query_batch_size`` best rows among those it has not queried.  A returned candidate counts when its
    index is not -1 and its score is finite; a shortfall is filled with random free rows from the replicate's generator, as in
    ``run_gp_ei_bo_batched``.  No ``best_f`` enters the score and nothing can underflow.  The prior weights and noise draws of
    replicate r come from a torch generator seeded from ``rngs[r]``, the noise draws at the replicate's own support size: a
    replicate's record does not depend on which other replicates share the batch.  ``oversample`` is accepted for the signature of
    ``run_gp_ts_bo_batched`` and not used.  ``ard``: as ``run_gp_ts_bo_batched``; the same two calls serve ARD batches.
    ``max_value``: ``"thompson"`` (the default) as described; ``"gumbel"`` draws the samples with ONE ``gp_ops.gumbel_pool`` call
    instead - a Gumbel fitted to the quartiles of the maximum of the pool's independent marginals (Wang & Jegelka 2017, section 3.1) -
    which needs no basis (none is drawn) and only ``n_max_samples`` uniforms per replicate, replicate r's from its own generator.
    ``batch``: ``"topk"`` (the default) takes the ``query_batch_size`` rows of largest MES score as described (they tend to be
    neighbours of the winner and carry almost the same information); ``"gibbon"`` replaces the ``mes_pool`` call with ONE
    ``gp_ops.gibbon_pool(q=query_batch_size)`` call on the same clamped samples - the greedy GIBBON batch (Moss et al. 2021), in
    which a pick lowers the score of the rows correlated with it - keeps the usable prefix of its picks (index not -1, value
    finite; later values may be negative) and fills a shortfall in the same way; the records are in pick order.  At
    ``query_batch_size = 1`` the two are DIFFERENT loops: GIBBON's single-point score ``a`` is not the MES score ``g``."""
    n = x_all.shape[0]
    if max_value not in ("thompson", "gumbel"):
        raise ValueError(f"max_value must be 'thompson' or 'gumbel', got {max_value!r}")
    if batch not in ("topk", "gibbon"):
        raise ValueError(f"batch must be 'topk' or 'gibbon', got {batch!r}")
    gumbel = max_value == "gumbel"
    if not 1 <= query_batch_size <= gp_ops._lib.POOL_TOPK_MAX:
        raise ValueError(f"query_batch_size must be in [1, {gp_ops._lib.POOL_TOPK_MAX}], got {query_batch_size}")
    S = int(n_max_samples)
    if not 1 <= S <= gp_ops._lib.TS_SAMPLES_MAX:
        raise ValueError(f"n_max_samples must be in [1, {gp_ops._lib.TS_SAMPLES_MAX}], got {n_max_samples}")
    y_all, X, queried = _bo_start(x_all, y_all, num_init_points, init_from, rngs)
    if not gumbel:
        omega, phase = gp_ops.rff_basis(kernel_type, X.shape[1], n_features, generator=torch.Generator().manual_seed(int(feature_seed)),
                                        device=X.device)
    records = [[min(q)] for q in queried]
    gens = _path_generators(rngs)

    for _ in range(num_bo_iters):
        b, phi = _fit_tasks("run_gp_mes_bo_batched", x_all, [(q, y_all) for q in queried], X, kernel_type, device, noise_init, noise_prior,
                            ard)
        if gumbel:
            u = torch.stack([torch.rand(S, generator=g) for g in gens])
            mv = gp_ops.gumbel_pool(b, phi, X, u=u.to(X.device), maximize=False)
        else:
            w, eps = _pathwise_draws(gens, S, n_features, queried, X.device)
            mv = gp_ops.max_value_samples(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, maximize=False)
        gp_ops.check_info(mv["info"], "BO posterior")
        # the minimum of f is no worse than the best value seen
        best = [y_all[q].min().item() for q in queried]
        ystar = torch.minimum(mv["ystar"], torch.tensor(best, dtype=torch.float32, device=X.device)[:, None])
        if batch == "gibbon":
            out = gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=query_batch_size, maximize=False, exclude=queried)
            top_idx, top_val = out["sel_idx"].cpu(), out["sel_val"].cpu()
        else:
            out = gp_ops.mes_pool(b, phi, X, ystar=ystar, maximize=False, topk=query_batch_size, exclude=queried)
            top_idx, top_val = out["top_idx"].cpu(), out["top_val"].cpu()
        gp_ops.check_info(out["info"], "BO posterior")
        usable = torch.isfinite(top_val) & (top_idx >= 0)   # (a prefix of each row: descending scores, the -1 / -inf tail last)
        if batch == "gibbon":   # pick order, not score order: keep the prefix
            usable = usable.long().cumprod(1).bool()
        _take_picks(top_idx, usable, query_batch_size, rngs, queried, records, n)
    return records


@torch.no_grad()
def run_gp_kg_bo_batched(x_all: torch.Tensor, y_all: torch.Tensor, num_init_points: int, query_batch_size: int, num_bo_iters: int,
                         kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                         rngs: List[np.random.Generator], ard: bool = False, n_refs: int = 32) -> List[List[int]]:
    """``len(rngs)`` replicates of a knowledge-gradient BO loop (Frazier, Powell & Dayanik 2009) over the same pool at once
    (minimisation, as ``run_gp_ei_bo``); returns their records: the best initial index, then the picks in descending score.  Per
    iteration the replicates' queried sets are fitted by ONE ``gp_ops.fit`` (as ``run_gp_ei_bo_batched``), ONE
    ``gp_ops.predict_pool(score="mean", topk=n_refs)`` call with no exclusions takes each replicate's ``n_refs`` (at most 64) rows
    of lowest posterior mean over the WHOLE pool - queried rows included: they belong in the discretisation - and ONE
    ``gp_ops.kg_pool(log=True, topk=query_batch_size, exclude=queried)`` call scores the pool against them and returns each
    replicate's best rows among those it has not queried.  The score is log KG, which keeps an order where float32 KG is 0 on every
    row; it prices the observation noise and needs no ``best_f``.  A returned candidate counts when its index is not -1 and its
    score is finite; a shortfall is filled with random free rows from the replicate's generator, as in ``run_gp_mes_bo_batched``.
    Nothing random enters the score: a replicate's record does not depend on which other replicates share the batch."""
    n = x_all.shape[0]
    if not 1 <= query_batch_size <= gp_ops._lib.POOL_TOPK_MAX:
        raise ValueError(f"query_batch_size must be in [1, {gp_ops._lib.POOL_TOPK_MAX}], got {query_batch_size}")
    M = int(n_refs)
    if not 1 <= M <= gp_ops._lib.KG_REFS_MAX:
        raise ValueError(f"n_refs must be in [1, {gp_ops._lib.KG_REFS_MAX}], got {n_refs}")
    y_all, X, queried = _bo_start(x_all, y_all, num_init_points, init_from, rngs)
    records = [[min(q)] for q in queried]

    for _ in range(num_bo_iters):
        b, phi = _fit_tasks("run_gp_kg_bo_batched", x_all, [(q, y_all) for q in queried], X, kernel_type, device, noise_init, noise_prior,
                            ard)
        refs = gp_ops.predict_pool(b, phi, X, maximize=False, topk=M, score="mean", want_mean=False, want_var=False, want_ei=False)
        gp_ops.check_info(refs["info"], "BO posterior")
        out = gp_ops.kg_pool(b, phi, X, ref_idx=refs["top_idx"], maximize=False, log=True, topk=query_batch_size, exclude=queried,
                             want_score=False)
        gp_ops.check_info(out["info"], "BO posterior")
        top_idx, top_val = out["top_idx"].cpu(), out["top_val"].cpu()
        usable = torch.isfinite(top_val) & (top_idx >= 0)   # (a prefix of each row: descending scores, the -1 / -inf tail last)
        _take_picks(top_idx, usable, query_batch_size, rngs, queried, records, n)
    return records


def _batch_size(query_batch_size: int) -> int:
    if not 1 <= query_batch_size <= gp_ops._lib.POOL_TOPK_MAX:
        raise ValueError(f"query_batch_size must be in [1, {gp_ops._lib.POOL_TOPK_MAX}], got {query_batch_size}")
    return int(query_batch_size)


@torch.no_grad()
def run_gp_lse_al_batched(x_all: torch.Tensor, y_all: torch.Tensor, tau: float, num_init_points: int, query_batch_size: int, num_iters: int,
                          kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                          rngs: List[np.random.Generator], beta: float = 1.96, maximize: bool = True, ard: bool = False,
                          return_counts: bool = False):
    """``len(rngs)`` replicates of a level-set active-learning loop (the straddle of Bryan et al. 2005 with the hallucinated batches of
    Gotovos et al. 2013) over the same pool at once: which rows have ``y > tau`` (``y < tau`` without ``maximize``)?  ``tau`` is given
    in the units of ``y_all`` and mapped through the loop's standardisation of the labels.  Per iteration the replicates' queried
    sets are fitted by ONE ``gp_ops.fit`` (as ``run_gp_ei_bo_batched``) and ONE ``gp_ops.levelset_pool(score="straddle",
    q=query_batch_size, exclude=queried)`` call returns each replicate's batch: the rows whose confidence band ``m +- beta sigma``
    straddles tau the most, each pick shrinking the bands of its neighbours before the next is taken.  A pick counts when its index
    is not -1 and its score is finite; random free rows from the replicate's generator fill the rest.  Returns the records (the
    lowest initial index, then the picks in pick order); with ``return_counts`` also ``counts [iterations, R, 3]`` (int64), the
    number of active, inactive and undecided pool rows each replicate saw BEFORE each iteration's batch.  Nothing random enters the
    score: a replicate's record does not depend on which other replicates share the batch."""
    n = x_all.shape[0]
    q = _batch_size(query_batch_size)
    mean, std = y_all.mean(), y_all.std()
    y_all, X, queried = _bo_start(x_all, y_all, num_init_points, init_from, rngs)
    tau_std = float((tau - mean) / std)
    records = [[min(s)] for s in queried]
    seen = []
    for _ in range(num_iters):
        b, phi = _fit_tasks("run_gp_lse_al_batched", x_all, [(s, y_all) for s in queried], X, kernel_type, device, noise_init, noise_prior,
                            ard)
        out = gp_ops.levelset_pool(b, phi, X, tau=tau_std, beta=beta, q=q, score="straddle", maximize=maximize, exclude=queried)
        gp_ops.check_info(out["info"], "level-set posterior")
        seen.append(out["counts"][:, 0].cpu())
        top_idx, top_val = out["sel_idx"].cpu(), out["sel_val"].cpu()
        usable = (torch.isfinite(top_val) & (top_idx >= 0)).long().cumprod(1).bool()
        _take_picks(top_idx, usable, q, rngs, queried, records, n)
    if return_counts:
        return records, (torch.stack(seen) if seen else torch.zeros(0, len(rngs), 3, dtype=torch.int64))
    return records


@torch.no_grad()
def run_gp_ucb_bo_batched(x_all: torch.Tensor, y_all: torch.Tensor, num_init_points: int, query_batch_size: int, num_bo_iters: int,
                          kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                          rngs: List[np.random.Generator], beta: float = 2.0, ard: bool = False) -> List[List[int]]:
    """``len(rngs)`` replicates of a GP-BUCB loop (Desautels, Krause and Burdick 2014) over the same pool at once (minimisation, as
    ``run_gp_ei_bo``); returns their records: the best initial index, then the picks in pick order.  Per iteration the replicates'
    queried sets are fitted by ONE ``gp_ops.fit`` and ONE ``gp_ops.levelset_pool(score="bound", q=query_batch_size,
    exclude=queried)`` call returns each replicate's batch: sequential-greedy picks of the lowest confidence bound ``m - beta
    sigma_j``, the variance downdated by every pick (hallucinated at its mean, so the mean never moves) before the next is taken.
    It needs no incumbent.  A pick counts when its index is not -1 and its score is finite; random free rows fill the rest."""
    n = x_all.shape[0]
    q = _batch_size(query_batch_size)
    y_all, X, queried = _bo_start(x_all, y_all, num_init_points, init_from, rngs)
    records = [[min(s)] for s in queried]
    for _ in range(num_bo_iters):
        b, phi = _fit_tasks("run_gp_ucb_bo_batched", x_all, [(s, y_all) for s in queried], X, kernel_type, device, noise_init, noise_prior,
                            ard)
        out = gp_ops.levelset_pool(b, phi, X, tau=0.0, beta=beta, q=q, score="bound", maximize=False, exclude=queried, want_counts=False)
        gp_ops.check_info(out["info"], "BO posterior")
        top_idx, top_val = out["sel_idx"].cpu(), out["sel_val"].cpu()
        usable = (torch.isfinite(top_val) & (top_idx >= 0)).long().cumprod(1).bool()
        _take_picks(top_idx, usable, q, rngs, queried, records, n)
    return records


@torch.no_grad()
def run_gp_ipv_al_batched(x_all: torch.Tensor, y_all: torch.Tensor, target_idx, num_init_points: int, query_batch_size: int,
                          num_rounds: int, kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                          rngs: List[np.random.Generator], ard: bool = False, exclude_targets: bool = True) -> List[List[int]]:
    """``len(rngs)`` replicates of a transductive active-learning loop over the same pool at once: which rows to label so that the
    predictions at the rows ``target_idx`` (pool indices, shared by the replicates) get as good as possible.  Returns their records:
    the rows each replicate labelled, in the order it chose them.  Per round the replicates' labelled sets are fitted by ONE
    ``gp_ops.fit`` (as ``run_gp_ei_bo_batched``) and ONE ``gp_ops.ipv_pool(q=query_batch_size, exclude=labelled)`` call returns each
    replicate's greedy batch: every pick lowers the posterior variance at the targets the most given the picks before it, and no
    label is needed inside a batch.  ``exclude_targets``: the targets cannot be measured - they are excluded, and a target drawn
    into an initial design is exchanged for a random free row.  ``query_batch_size`` plus the number of targets is at most 64.  A
    returned candidate counts when its index is not -1 and its score is finite; a shortfall is filled with random free rows from the
    replicate's generator, as in ``run_gp_mes_bo_batched``.  Nothing random enters the score."""
    n = x_all.shape[0]
    targets = torch.as_tensor(target_idx).reshape(-1)
    if targets.is_floating_point() or targets.numel() < 1 or int(targets.min()) < 0 or int(targets.max()) >= n:
        raise ValueError(f"target_idx must hold at least one integer pool index in [0, {n})")
    tgt = sorted(set(int(i) for i in targets.tolist()))
    M, cap = len(tgt), gp_ops._lib.IPV_ENTRIES_MAX
    if M >= cap:
        raise ValueError(f"at most {cap - 1} distinct targets, got {M}")
    if not 1 <= query_batch_size <= cap - M:
        raise ValueError(f"query_batch_size must be in [1, {cap - M}] with {M} targets, got {query_batch_size}")
    if num_rounds < 0:
        raise ValueError(f"num_rounds must not be negative, got {num_rounds}")
    y_all, X, labelled = _bo_start(x_all, y_all, num_init_points, init_from, rngs)
    if exclude_targets:
        for r, rng in enumerate(rngs):
            hit = [i for i in labelled[r] if i in tgt]
            if hit:
                free = [i for i in range(init_from, n) if i not in tgt and i not in labelled[r]]
                labelled[r] = [i for i in labelled[r] if i not in tgt] + rng.choice(free, size=len(hit), replace=False).tolist()
    # what a replicate may not pick: its labelled rows and, with exclude_targets, the targets.  _take_picks adds each round's picks
    # to blocked[r] itself (it is the loop's `queried`), which is what keeps a later round from choosing them again
    blocked = [rows_r + tgt if exclude_targets else list(rows_r) for rows_r in labelled]
    records = [[] for _ in rngs]

    for _ in range(num_rounds):
        b, phi = _fit_tasks("run_gp_ipv_al_batched", x_all, [(rows_r, y_all) for rows_r in labelled], X, kernel_type, device,
                            noise_init, noise_prior, ard)
        out = gp_ops.ipv_pool(b, phi, X, targets=[tgt] * len(rngs), q=query_batch_size, exclude=blocked)
        gp_ops.check_info(out["info"], "AL posterior")
        sel_idx, sel_val = out["sel_idx"].cpu(), out["sel_val"].cpu()
        usable = torch.isfinite(sel_val) & (sel_idx >= 0)   # (a prefix of each row: the -1 / -inf tail comes last)
        _take_picks(sel_idx, usable, query_batch_size, rngs, blocked, records, n)
        for r in range(len(rngs)):
            labelled[r] = labelled[r] + records[r][-query_batch_size:]
    return records


@torch.no_grad()
def run_gp_jes_bo_batched(x_all: torch.Tensor, y_all: torch.Tensor, num_init_points: int, query_batch_size: int, num_bo_iters: int,
                          kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                          rngs: List[np.random.Generator], n_features: int = 1024, oversample: int = 4,
                          feature_seed: int = 0, ard: bool = False, n_opt_samples: int = 16,
                          cond_noise: float = 1e-6) -> List[List[int]]:
    """``len(rngs)`` replicates of a joint entropy search BO loop (Hvarfner, Hutter & Nardi 2022) over the same pool at once
    (minimisation, as ``run_gp_ei_bo``); returns their records: the best initial index, then the picks in descending score.  Per
    iteration the replicates' queried sets are fitted by ONE ``gp_ops.fit`` (as ``run_gp_ei_bo_batched``), ONE
    ``gp_ops.optimum_samples`` call draws ``n_opt_samples`` (at most 64) samples of each replicate's minimum over the WHOLE pool,
    location and value together - the minima of pathwise posterior draws on a random-Fourier basis of ``n_features`` features (drawn
    once from ``feature_seed``) - and ONE ``gp_ops.jes_pool(topk=query_batch_size, exclude=queried)`` call scores the pool
    against them, conditioning on each sampled optimum under the noise variance ``cond_noise``, and returns each replicate's best rows
    among those it has not queried.  The sampled value is NOT clamped to the best observation, as ``run_gp_mes_bo_batched`` clamps
    it: location and value are one joint sample.  A returned candidate counts when its index is not -1 and its score is finite; a
    shortfall is filled with random free rows from the replicate's generator, as in ``run_gp_mes_bo_batched``.  The prior weights and
    noise draws of replicate r come from a torch generator seeded from ``rngs[r]``, exactly as ``run_gp_mes_bo_batched`` draws them,
    the noise draws at the replicate's own support size: a replicate's record does not depend on which other replicates share the
    batch.  ``oversample`` is accepted for the signature of ``run_gp_ts_bo_batched`` and not used.  ``ard``: as
    ``run_gp_ts_bo_batched``; the same two calls serve ARD batches."""
    n = x_all.shape[0]
    if not 1 <= query_batch_size <= gp_ops._lib.POOL_TOPK_MAX:
        raise ValueError(f"query_batch_size must be in [1, {gp_ops._lib.POOL_TOPK_MAX}], got {query_batch_size}")
    S = int(n_opt_samples)
    if not 1 <= S <= gp_ops._lib.TS_SAMPLES_MAX:
        raise ValueError(f"n_opt_samples must be in [1, {gp_ops._lib.TS_SAMPLES_MAX}], got {n_opt_samples}")
    if not 0.0 <= float(cond_noise) < float("inf"):
        raise ValueError(f"cond_noise must be finite and >= 0, got {cond_noise}")
    y_all, X, queried = _bo_start(x_all, y_all, num_init_points, init_from, rngs)
    omega, phase = gp_ops.rff_basis(kernel_type, X.shape[1], n_features, generator=torch.Generator().manual_seed(int(feature_seed)),
                                    device=X.device)
    records = [[min(q)] for q in queried]
    gens = _path_generators(rngs)

    for _ in range(num_bo_iters):
        b, phi = _fit_tasks("run_gp_jes_bo_batched", x_all, [(q, y_all) for q in queried], X, kernel_type, device, noise_init, noise_prior,
                            ard)
        w, eps = _pathwise_draws(gens, S, n_features, queried, X.device)
        opt = gp_ops.optimum_samples(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps, maximize=False)
        gp_ops.check_info(opt["info"], "BO posterior")
        out = gp_ops.jes_pool(b, phi, X, opt_idx=opt["opt_idx"], opt_val=opt["opt_val"], cond_noise=cond_noise, maximize=False,
                              topk=query_batch_size, exclude=queried, want_score=False)
        gp_ops.check_info(out["info"], "BO posterior")
        top_idx, top_val = out["top_idx"].cpu(), out["top_val"].cpu()
        usable = torch.isfinite(top_val) & (top_idx >= 0)   # (a prefix of each row: descending scores, the -1 / -inf tail last)
        _take_picks(top_idx, usable, query_batch_size, rngs, queried, records, n)
    return records


def _hypervolume_2d(Y: torch.Tensor, maximize, ref: torch.Tensor) -> float:
    """The area dominated by the points ``Y [n, 2]`` and bounded by ``ref``, on the host (``gp_ops.pareto_front``'s staircase)."""
    sg = torch.tensor([-1.0 if m else 1.0 for m in maximize], dtype=torch.float64)
    st = gp_ops.pareto_front(Y.double().cpu(), maximize, ref.double().cpu()) * sg
    r = ref.double().cpu() * sg
    hv, right = 0.0, float(r[0])
    for i in range(st.shape[0] - 1, -1, -1):   # from the worst first coordinate to the best: one rectangle per step
        hv += (right - float(st[i, 0])) * (float(r[1]) - float(st[i, 1]))
        right = float(st[i, 0])
    return hv


def _ehvi_ref_point(Y: torch.Tensor, maximize) -> torch.Tensor:
    """The worst queried value per objective plus 0.1 of the queried range (BoTorch's heuristic).  An objective whose queried values
    are all equal has no range: the margin is then 0.1 (of the unit variance the columns are standardised to), so that the reference
    point never lies ON the queried points - which would clean the whole front away."""
    lo, hi = Y.min(0).values, Y.max(0).values
    mx = torch.tensor([bool(m) for m in maximize], device=Y.device)
    margin = 0.1 * torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    return torch.where(mx, lo - margin, hi + margin)


@torch.no_grad()
def run_gp_ehvi_bo_batched(x_all: torch.Tensor, y_all: torch.Tensor, num_init_points: int, query_batch_size: int, num_bo_iters: int,
                           kernel_type: str, device, init_from: int, noise_init: float, noise_prior: bool,
                           rngs: List[np.random.Generator], maximize=(False, False), acquisition: str = "log_ehvi",
                           ard: bool = False):
    """``len(rngs)`` replicates of a two-objective BO loop by expected hypervolume improvement over the same pool at once; ``y_all``
    is ``[n, 2]``, ``maximize`` the sense per objective.  R replicates make 2 R tasks in ONE batch - task 2 r + j is objective j of
    replicate r - and group r = (2 r, 2 r + 1).  Per iteration the queried sets are fitted by ONE ``gp_ops.fit`` and ONE
    ``gp_ops.ehvi_pool(topk=query_batch_size, exclude=queried)`` call scores the pool for every replicate against the front of its
    own queried values (``gp_ops.pareto_front``) and its reference point - the worst queried value per objective plus 0.1 of the
    queried range (0.1 where the range is 0), recomputed every iteration - and returns its best rows among those it has not queried.
    A replicate whose queried values have more than 64 non-dominated points is beyond ``ehvi_pool``'s front and raises.  Each column
    of ``y_all`` is standardised once.  ``acquisition``: ``"log_ehvi"`` (a candidate counts when its index is not -1 and its score is finite) or
    ``"ehvi"`` (when its score is positive); a shortfall is filled with random free rows from the replicate's generator, as in
    ``run_gp_mes_bo_batched``.  Returns ``(records, hypervolume)``: per replicate the initial indices followed by the picks in
    descending score, and the dominated hypervolume of its queried values (standardised units) after the initial design and after
    every iteration, all against the FINAL reference point - computed on the host."""
    R, n = len(rngs), x_all.shape[0]
    if not 1 <= query_batch_size <= gp_ops._lib.POOL_TOPK_MAX:
        raise ValueError(f"query_batch_size must be in [1, {gp_ops._lib.POOL_TOPK_MAX}], got {query_batch_size}")
    if y_all.dim() != 2 or tuple(y_all.shape) != (n, 2):
        raise ValueError(f"y_all must be [n, 2] = [{n}, 2], got {tuple(y_all.shape)}")
    if acquisition not in ("log_ehvi", "ehvi"):
        raise ValueError(f"acquisition must be 'log_ehvi' or 'ehvi', got {acquisition!r}")
    log = acquisition == "log_ehvi"
    maximize = tuple(bool(m) for m in maximize)
    y_all, X, queried = _bo_start(x_all, y_all, num_init_points, init_from, rngs, dim=0)
    records = [list(q) for q in queried]
    history = [[list(q)] for q in queried]
    obj = torch.tensor([[2 * r, 2 * r + 1] for r in range(R)], dtype=torch.int32)
    obj_max = torch.tensor([[int(maximize[0]), int(maximize[1])]] * R, dtype=torch.int32)

    for _ in range(num_bo_iters):
        fronts, refs = [], []
        for r, q in enumerate(queried):
            Yq = y_all[q].float()
            refs.append(_ehvi_ref_point(Yq, maximize))
            fronts.append(gp_ops.pareto_front(Yq.cpu(), maximize))
            if fronts[-1].shape[0] > gp_ops._lib.EHVI_FRONT_MAX:   # (a truncated front would overstate every improvement)
                raise ValueError(f"replicate {r} has {fronts[-1].shape[0]} non-dominated queried points; ehvi_pool takes a front of at most "
                                 f"{gp_ops._lib.EHVI_FRONT_MAX}")
        P = max(1, max(f.shape[0] for f in fronts))
        front = torch.zeros(R, P, 2)
        for r, f in enumerate(fronts):
            front[r, :f.shape[0]] = f
        front_n = torch.tensor([f.shape[0] for f in fronts], dtype=torch.int32)
        b, phi = _fit_tasks("run_gp_ehvi_bo_batched", x_all, [(q, y_all[:, j]) for q in queried for j in range(2)], X, kernel_type, device,
                            noise_init, noise_prior, ard)
        out = gp_ops.ehvi_pool(b, phi, X, obj=obj, ref=torch.stack(refs).cpu(), front=front, front_n=front_n, obj_maximize=obj_max, log=log,
                               topk=query_batch_size, exclude=queried, want_score=False)
        gp_ops.check_info(out["info"], "BO posterior")
        top_idx, top_val = out["top_idx"].cpu(), out["top_val"].cpu()
        usable = (torch.isfinite(top_val) if log else top_val > 0) & (top_idx >= 0)   # (a prefix of each row)
        _take_picks(top_idx, usable, query_batch_size, rngs, queried, records, n)
        for r in range(R):
            history[r].append(list(records[r]))
    hypervolume = []
    for r in range(R):
        ref = _ehvi_ref_point(y_all[records[r]].float(), maximize)
        hypervolume.append([_hypervolume_2d(y_all[q].float(), maximize, ref) for q in history[r]])
    return records, hypervolume
