"""Meta-test path: adapt the GP to each test task's support set, predict its query molecules, score.

Mirrors ``run_on_batches(train=False)`` / ``evaluate_adkt_model`` (fs_mol/utils/adaptive_dkt_utils.py:70-175) and the
metric records of fs_mol/utils/metrics.py:21-60,110-150 (same field names, same conventions: predictions >= 0.5 count as
positive, ``zero_division=1``, ROC-AUC 0.0 for single-class tasks, out-of-sample R^2 against a zero baseline because
regression labels are standardised with support statistics).

Two entry points:

* ``run_on_batches``      - the reference-shaped loop, one query batch at a time through ``ADKTModel.forward``;
* ``meta_test``           - every task of a ``MetaBatch`` at once: ONE feature-extractor forward (no grad), then
                            ``adkf_init_params -> adkf_fit -> adkf_predict`` on the whole batch (the fit's A^-1, alpha
                            are reused by the prediction).  No hypergradient is involved.
* ``adapt_and_test``      - MoleculeNet's test protocol (MoleculeNet/chem_lib/models/adkfift_trainer.py:222-283): per test task,
                            ``update_step_test`` hypergradient steps on the task's adaptation batches from the saved weights,
                            then the final fit on the support set and the prediction of the query loader.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .meta_batch import DKTBatch, MetaBatch, collate_meta_batch, meta_features


@dataclass(frozen=True)
class BinaryEvalMetrics:
    size: int
    acc: float
    balanced_acc: float
    f1: float
    prec: float
    recall: float
    roc_auc: float
    avg_precision: float
    kappa: float


@dataclass(frozen=True)
class NumericEvalMetrics:
    size: int
    mse: float
    mae: float
    r2: float


def compute_binary_task_metrics(predictions, labels) -> BinaryEvalMetrics:
    from sklearn import metrics as skm

    predictions = np.asarray(predictions, dtype=np.float64)
    labels = np.asarray(labels).astype(bool)
    hard = predictions >= 0.5
    single_class = labels.all() or not labels.any()
    return BinaryEvalMetrics(
        size=len(predictions),
        acc=float(skm.accuracy_score(labels, hard)),
        balanced_acc=float(skm.balanced_accuracy_score(labels, hard)),
        f1=float(skm.f1_score(labels, hard, zero_division=1)),
        prec=float(skm.precision_score(labels, hard, zero_division=1)),
        recall=float(skm.recall_score(labels, hard, zero_division=1)),
        roc_auc=0.0 if single_class else float(skm.roc_auc_score(labels, predictions)),
        avg_precision=float(skm.average_precision_score(labels, predictions)),
        kappa=float(skm.cohen_kappa_score(labels, hard)),
    )


def r2_score_os(y_true, y_pred, y_train_mean: float = 0.0) -> float:
    """Out-of-sample R^2: the baseline is the TRAINING mean (0 after standardisation), fs_mol/utils/metrics.py:127-143."""
    y_true = np.asarray(y_true, dtype=np.float64)
    y_pred = np.asarray(y_pred, dtype=np.float64)
    assert y_true.shape == y_pred.shape
    den = ((y_true - y_train_mean) ** 2).sum()
    assert den != 0
    return float(1.0 - ((y_true - y_pred) ** 2).sum() / den)


def compute_numeric_task_metrics(predictions, labels) -> NumericEvalMetrics:
    p = np.asarray(predictions, dtype=np.float64)
    y = np.asarray(labels, dtype=np.float64)
    assert p.shape == y.shape
    return NumericEvalMetrics(size=len(p), mse=float(((p - y) ** 2).mean()), mae=float(np.abs(p - y).mean()), r2=r2_score_os(y, p))


def avg_task_metrics_list(results: Sequence) -> Dict[str, Tuple[float, float]]:
    """mean / std of every field over repeated samples of one task (metrics.py:83-93, 176-186)."""
    out = {}
    for f in dataclasses.fields(type(results[0])):
        v = [getattr(r, f.name) for r in results]
        out[f.name] = (float(np.mean(v)), float(np.std(v)))
    return out


def avg_metrics_over_tasks(task_results: Dict[str, Sequence]) -> Dict[str, Tuple[float, float]]:
    """mean / std across tasks of the per-task means (metrics.py:63-80, 153-173)."""
    per_task = {k: avg_task_metrics_list(v) for k, v in task_results.items()}
    first = next(iter(task_results.values()))[0]
    out = {}
    for f in dataclasses.fields(type(first)):
        v = [m[f.name][0] for m in per_task.values()]
        out[f.name] = (float(np.mean(v)), float(np.std(v)))
    return out


def _score(model, preds: np.ndarray, labels: np.ndarray):
    if model.config.use_numeric_labels:
        return compute_numeric_task_metrics(preds, labels)
    return compute_binary_task_metrics(preds, labels)


def run_on_batches(model, batches: List[DKTBatch], batch_labels: List[torch.Tensor], batch_numeric_labels: List[torch.Tensor],
                   train: bool = False):
    """Reference-shaped: per query batch {train-mode forward (re-initialises the GP on the support set), inner fit,
    eval-mode forward}; predictions are ``sigmoid(mean)`` (classification) or ``mean`` (regression)."""
    from .models import fit_gpytorch_scipy

    if train:
        assert len(batches) == 1
    preds, labels = [], []
    for feats, lab, num in zip(batches, batch_labels, batch_numeric_labels):
        model.train()
        _ = model(feats, train_loss=True)
        fit_gpytorch_scipy(model.mll)
        if not train:
            model.eval()
            with torch.no_grad():
                post = model(feats, train_loss=None)
                if model.config.use_numeric_labels:
                    preds.append(post.mean.detach().cpu().numpy())
                    labels.append(num.detach().cpu().numpy())
                else:
                    preds.append(torch.sigmoid(post.mean).detach().cpu().numpy())
                    labels.append(lab.detach().cpu().numpy())
    if train:
        return None
    return _score(model, np.concatenate(preds), np.concatenate(labels))


@torch.no_grad()
def meta_test(model, mb: MetaBatch, max_evals: int = 200, gtol: float = 1e-5, ftol: float = 2.22e-9, want_var: bool = False,
              streaming: bool = False):
    """All tasks at once.  Returns (predictions [T, Nq_max], variance or None, phi* [T, h], n_evals [T]); padded query
    slots hold 0.  Classification predictions are already passed through the sigmoid.  ``streaming``: fit on a support-only
    batch and predict the packed query rows with ``gp_ops.predict_marginal`` (no padding to the largest query set, no size
    cap); same layout out."""
    from . import gp_ops

    cfg = model.config
    was_training = model.training
    model.eval()
    Z_s, Z_q = meta_features(model, mb)
    y_s, _ = mb.labels(cfg.use_numeric_labels)
    dev = Z_s.device
    priors = torch.empty(mb.num_tasks, 4, dtype=torch.float32, device=dev)
    b = gp_ops.GPBatch(Z_s.float().contiguous(), y_s.to(dev).float().contiguous(), priors, cfg.gp_kernel,
                       Z_q=None if streaming else Z_q.float().contiguous(), n_s=mb.n_s, n_q=None if streaming else mb.n_q,
                       ard=cfg.use_ard)
    phi0, _ = gp_ops.init_params_batch(b, cfg.use_numeric_labels, cfg.use_lengthscale_prior)
    b.flags = gp_ops.REUSE_DIST | gp_ops.DEFER_REFINE     # (the prediction redoes ill-conditioned tasks in float64 itself)
    phi, _, _, n_evals, info = gp_ops.fit(b, phi0, max_evals, gtol, ftol)
    gp_ops.check_info(info, "meta-test inner fit")
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    if streaming:
        Zq_p, q_off = gp_ops.pack_rows(Z_q.float(), mb.n_q)
        mean_p, var_p, _, info = gp_ops.predict_marginal(b, phi, Zq_p, q_off, want_var=want_var)
        mean = gp_ops.unpack_rows(mean_p, q_off, Z_q.shape[1])
        var = gp_ops.unpack_rows(var_p, q_off, Z_q.shape[1]) if want_var else None
    else:
        mean, var, _, info = gp_ops.predict(b, phi, want_var=want_var)
    gp_ops.check_info(info, "meta-test prediction")
    if was_training:
        model.train()
    preds = mean if cfg.use_numeric_labels else torch.sigmoid(mean) * mb.q_mask.to(dev)
    return preds, var, phi, n_evals


@torch.no_grad()
def screen(model, mb: MetaBatch, X_features: torch.Tensor, k: int, maximize: bool = True, max_evals: int = 200):
    """Virtual screening: every task of ``mb`` is fitted on its support set, then ranks the SAME library ``X_features [rows, d]``
    (rows in the model's feature space) by posterior mean in one ``gp_ops.predict_pool`` call, or beyond 64 rows per task in one
    ``gp_ops.rank_pool`` call.  Returns (top_idx [T, k] int64, top_val [T, k], phi*): each task's ``k`` (at most 65536) best rows,
    best first (largest mean with ``maximize``, smallest without; ``top_val`` is +mean / -mean accordingly).  Nothing of size
    T x rows is allocated."""
    from . import gp_ops

    cfg = model.config
    was_training = model.training
    model.eval()
    Z_s, _ = meta_features(model, mb)
    y_s, _ = mb.labels(cfg.use_numeric_labels)
    priors = torch.empty(mb.num_tasks, 4, dtype=torch.float32, device=Z_s.device)
    b = gp_ops.GPBatch(Z_s.float().contiguous(), y_s.to(Z_s.device).float().contiguous(), priors, cfg.gp_kernel, n_s=mb.n_s, ard=cfg.use_ard)
    phi0, _ = gp_ops.init_params_batch(b, cfg.use_numeric_labels, cfg.use_lengthscale_prior)
    b.flags = gp_ops.REUSE_DIST | gp_ops.DEFER_REFINE
    phi, _, _, _, info = gp_ops.fit(b, phi0, max_evals)
    gp_ops.check_info(info, "screening inner fit")
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    if int(k) <= gp_ops._lib.POOL_TOPK_MAX:
        out = gp_ops.predict_pool(b, phi, X_features, maximize=maximize, score="mean", want_mean=False, want_var=False, topk=k)
    else:
        out = gp_ops.rank_pool(b, phi, X_features, maximize=maximize, score="mean", topk=k)
    gp_ops.check_info(out["info"], "screening prediction")
    if was_training:
        model.train()
    return out["top_idx"], out["top_val"], phi


def select_support(model, mb: MetaBatch, X_features: torch.Tensor, targets, q: int, exclude=None, max_evals: int = 200):
    """Which rows to label next: every task of ``mb`` is fitted on its support set, then chooses ``q`` rows of the SAME library
    ``X_features [rows, d]`` (rows in the model's feature space) whose labels would lower the posterior variance at its target rows
    ``targets [T, M]`` (library indices; ``M + q`` at most 64) the most, in one ``gp_ops.ipv_pool`` call - ``screen``'s twin for the
    question "what should I measure" instead of "what is best".  Returns (sel_idx [T, q] int64, sel_val [T, q], tvar [T, q + 1],
    phi*): the picks in pick order, what each took off the summed target variance, and that variance before and after each pick.
    ``exclude``: rows a task may not choose (``gp_ops.pack_exclude``) - the targets themselves, if they cannot be measured."""
    from . import gp_ops

    cfg = model.config
    was_training = model.training
    model.eval()
    Z_s, _ = meta_features(model, mb)
    y_s, _ = mb.labels(cfg.use_numeric_labels)
    priors = torch.empty(mb.num_tasks, 4, dtype=torch.float32, device=Z_s.device)
    b = gp_ops.GPBatch(Z_s.float().contiguous(), y_s.to(Z_s.device).float().contiguous(), priors, cfg.gp_kernel, n_s=mb.n_s, ard=cfg.use_ard)
    phi0, _ = gp_ops.init_params_batch(b, cfg.use_numeric_labels, cfg.use_lengthscale_prior)
    b.flags = gp_ops.REUSE_DIST | gp_ops.DEFER_REFINE
    phi, _, _, _, info = gp_ops.fit(b, phi0, max_evals)
    gp_ops.check_info(info, "support selection inner fit")
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    out = gp_ops.ipv_pool(b, phi, X_features, targets=targets, q=q, exclude=exclude)
    gp_ops.check_info(out["info"], "support selection")
    if was_training:
        model.train()
    return out["sel_idx"], out["sel_val"], out["tvar"], phi


def _fitted_support(model, mb: MetaBatch, max_evals: int, what: str):
    """The support-only batch of ``mb`` on the model's features, fitted as ``screen`` fits it: (b, phi*), b set to reuse the fit."""
    from . import gp_ops

    cfg = model.config
    Z_s, _ = meta_features(model, mb)
    y_s, _ = mb.labels(cfg.use_numeric_labels)
    priors = torch.empty(mb.num_tasks, 4, dtype=torch.float32, device=Z_s.device)
    b = gp_ops.GPBatch(Z_s.float().contiguous(), y_s.to(Z_s.device).float().contiguous(), priors, cfg.gp_kernel, n_s=mb.n_s, ard=cfg.use_ard)
    phi0, _ = gp_ops.init_params_batch(b, cfg.use_numeric_labels, cfg.use_lengthscale_prior)
    b.flags = gp_ops.REUSE_DIST | gp_ops.DEFER_REFINE
    phi, _, _, _, info = gp_ops.fit(b, phi0, max_evals)
    gp_ops.check_info(info, f"{what} inner fit")
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    return b, phi


@torch.no_grad()
def find_actives(model, mb: MetaBatch, X_features: torch.Tensor, tau, beta=1.96, q: int = 0, maximize: bool = True, exclude=None,
                 max_evals: int = 200):
    """Thresholded screening: every task of ``mb`` is fitted on its support set, then sorts the SAME library ``X_features [rows, d]``
    (rows in the model's feature space) against the threshold ``tau`` (a scalar or ``[T]``) in one ``gp_ops.levelset_pool`` call -
    ``screen``'s twin for "which rows are active, how many are there, and what must I measure to decide the rest".  A row is active
    (0) or inactive (1) when its confidence band ``m +- beta sigma`` lies wholly on one side of tau (above it means active with
    ``maximize``, below it without) and undecided (2) while the band holds tau.  Returns (cls [T, rows] int8, counts [T, 3] int64,
    hits [T], sel_idx [T, q] int64, counts_after [T, 3], phi*): the class of every row (-1: not evaluated), the number of active,
    inactive and undecided rows, the expected number of actives ``sum_r Phi(+-(m - tau) / sigma)``, the ``q`` (at most 63) rows whose
    labels would settle the most - a straddle batch, each pick shrinking its neighbours' bands before the next is taken - and the
    counts that batch would leave if every pick came back at its posterior mean (``counts`` itself with ``q = 0``).  ``exclude``:
    rows a task may not pick (``gp_ops.pack_exclude``); they are classified and counted all the same."""
    from . import gp_ops

    q = gp_ops._in_range(q, 0, gp_ops._lib.POOL_TOPK_MAX - 1, "q")
    was_training = model.training
    model.eval()
    b, phi = _fitted_support(model, mb, max_evals, "level-set")
    out = gp_ops.levelset_pool(b, phi, X_features, tau=tau, beta=beta, q=q + 1, score="straddle", maximize=maximize, exclude=exclude,
                               want_cls=True)
    gp_ops.check_info(out["info"], "level-set estimation")
    if was_training:
        model.train()
    return out["cls"], out["counts"][:, 0], out["hits"][:, 0], out["sel_idx"][:, :q], out["counts"][:, q], phi


def enrichment_from_ranks(ranks: torch.Tensor, n_ranked: torch.Tensor, fractions=(0.01, 0.05)) -> torch.Tensor:
    """Enrichment factors from ranks (CPU tensors, pure torch): ``ranks [T, M]`` the 0-based ranks of each task's actives (-1: not
    ranked), ``n_ranked [T]`` the rows each task ranked.  ``ef[t, f]`` is the share of task t's ranked actives with
    ``rank < ceil(f * n_ranked[t])``, divided by ``f``: 1 for a random order, ``1 / f`` at most.  NaN for a task without ranked
    actives.  Returns float64 ``[T, len(fractions)]``."""
    ranks, n_ranked = torch.as_tensor(ranks).to(torch.int64), torch.as_tensor(n_ranked).to(torch.int64).reshape(-1)
    if ranks.dim() != 2 or ranks.shape[0] != n_ranked.numel():
        raise ValueError(f"ranks must be [T, M] with n_ranked [T], got {tuple(ranks.shape)} and {tuple(n_ranked.shape)}")
    fractions = [float(f) for f in fractions]
    if not fractions or any(not (0.0 < f <= 1.0) for f in fractions):
        raise ValueError(f"fractions must lie in (0, 1], got {fractions}")
    ranked = ranks >= 0
    n_act = ranked.sum(1).double()
    ef = torch.empty(ranks.shape[0], len(fractions), dtype=torch.float64)
    for i, f in enumerate(fractions):
        cut = torch.ceil(f * n_ranked.double()).to(torch.int64)
        hits = (ranked & (ranks < cut[:, None])).sum(1).double()
        ef[:, i] = hits / n_act / f   # (0 / 0: NaN)
    return ef


@torch.no_grad()
def enrichment(model, mb: MetaBatch, X_features: torch.Tensor, actives, fractions=(0.01, 0.05), maximize: bool = True, exclude=None,
               max_evals: int = 200):
    """Retrospective screening: every task of ``mb`` is fitted on its support set as ``screen`` fits it, ranks the SAME library
    ``X_features [rows, d]`` by posterior mean and reports where its known actives ``actives`` (``[T, M]`` int64 library indices or
    T index lists, at most 1024 per task, -1: unused) come in that ranking, in one ``gp_ops.rank_pool`` call.  Returns (ranks [T, M]
    int64, n_ranked [T] int64, ef [T, len(fractions)] float64 on the CPU, phi*): the 0-based rank of every active (-1: not ranked),
    the rows each task ranked and the enrichment factors of ``enrichment_from_ranks``.  ``exclude``: rows a task leaves out of its
    ranking (``gp_ops.pack_exclude``) - its own support rows, usually."""
    from . import gp_ops

    was_training = model.training
    model.eval()
    b, phi = _fitted_support(model, mb, max_evals, "enrichment")
    out = gp_ops.rank_pool(b, phi, X_features, maximize=maximize, score="mean", rank_rows=actives, exclude=exclude)
    gp_ops.check_info(out["info"], "enrichment ranking")
    if was_training:
        model.train()
    ranks = out["ref_rank"] if out["ref_rank"] is not None else torch.empty(b.T, 0, dtype=torch.int64, device=b.device)
    ef = enrichment_from_ranks(ranks.cpu(), out["n_ranked"].cpu(), fractions)
    return ranks, out["n_ranked"], ef, phi


def predict_intervals(model, mb: MetaBatch, X_features: torch.Tensor, alpha=0.1, scaled: bool = True, k: int = 0, maximize: bool = True,
                      max_evals: int = 200):
    """How far the predictions can be trusted: every task of ``mb`` is fitted on its support set, then gives every row of the SAME
    library ``X_features [rows, d]`` (rows in the model's feature space) a jackknife+ prediction interval in one
    ``gp_ops.jackknife_pool`` call - distribution-free, coverage at least ``1 - 2 alpha``, no label held out (at most 256 support
    points per task).  ``alpha``: one level or up to 8.  The hyperparameters are those of the one fit, NOT refitted per fold, so
    the coverage is a very good approximation rather than a theorem.  Returns (lo [T, L, rows], hi [T, L, rows], top_idx [T, k],
    top_val [T, k], phi*): the selection ranks the rows by the bound one can rely on at the first level (``lo`` with ``maximize``,
    ``-hi`` without); None, None with ``k == 0``."""
    from . import gp_ops

    was_training = model.training
    model.eval()
    b, phi = _fitted_support(model, mb, max_evals, "interval")
    levels = (alpha,) if isinstance(alpha, (int, float)) else alpha
    out = gp_ops.jackknife_pool(b, phi, X_features, alpha=levels, scaled=scaled, maximize=maximize, topk=k, want_loo=False)
    gp_ops.check_info(out["info"], "interval prediction")
    if was_training:
        model.train()
    return out["lo"], out["hi"], out["top_idx"], out["top_val"], phi


def loo_check(model, mb: MetaBatch, max_evals: int = 200):
    """Leave-one-out cross-validation of every task of ``mb`` at its fitted hyperparameters (not refitted per fold), at no extra
    factorisation: (loo_mean [T, ns], loo_var [T, ns], loo_lpd [T], phi*) - each support point's prediction and observed variance
    from the other points, and the summed log predictive density, a calibration check that needs no validation set."""
    from . import gp_ops

    was_training = model.training
    model.eval()
    b, phi = _fitted_support(model, mb, max_evals, "leave-one-out")
    out = gp_ops.loo(b, phi)
    gp_ops.check_info(out["info"], "leave-one-out check")
    if was_training:
        model.train()
    return out["loo_mean"], out["loo_var"], out["loo_lpd"], phi


@torch.no_grad()
def explain_hits(model, mb: MetaBatch, X_features: torch.Tensor, idx: torch.Tensor, of: str = "mean", maximize: bool = True,
                 max_evals: int = 200) -> torch.Tensor:
    """Why these rows: every task of ``mb`` is fitted on its support set as ``screen`` fits it, then returns the gradient of its
    prediction at its chosen rows of the library ``X_features [rows, d]`` with respect to the rows' features - ``[T, k, d]``, the
    saliency at the feature layer, ready to be pushed back through the extractor.  ``idx [T, k]`` (int64 library indices, typically
    ``screen``'s ``top_idx``; -1 or out of range: a zero row).  ``of``: "mean", "var", or the acquisition "ei" / "log_ei" against each
    task's best support label (largest with ``maximize``).  The chosen rows are gathered into ONE packed ``gp_ops.predict_grad`` call:
    nothing of size T x rows is allocated."""
    from . import gp_ops

    if of not in ("mean", "var", "ei", "log_ei"):
        raise ValueError(f'of must be "mean", "var", "ei" or "log_ei", got {of!r}')
    was_training = model.training
    model.eval()
    b, phi = _fitted_support(model, mb, max_evals, "explanation")
    dev = b.device
    idx = torch.as_tensor(idx).to(device=dev, dtype=torch.int64)
    if idx.dim() != 2 or idx.shape[0] != b.T:
        raise ValueError(f"idx must be [T, k] = [{b.T}, k], got {tuple(idx.shape)}")
    T, k = idx.shape
    X = X_features.to(dev).float()
    valid = (idx >= 0) & (idx < X.shape[0])
    Zq = X[idx[valid]].contiguous()   # task-major: the valid rows of task 0, then those of task 1, ...
    q_off = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    q_off[1:] = torch.cumsum(valid.sum(1), 0)
    out = torch.zeros(T, k, b.d, dtype=torch.float32, device=dev)
    if Zq.shape[0] > 0:
        ones = torch.ones(Zq.shape[0], dtype=torch.float32, device=dev)
        kw = {}
        if of in ("ei", "log_ei"):
            n_s = b.n_s if b.n_s is not None else torch.full((T,), b.ns, dtype=torch.int32, device=dev)
            y = b.y_s.masked_fill(torch.arange(b.ns, device=dev)[None, :] >= n_s[:, None], float("-inf") if maximize else float("inf"))
            kw = dict(g_ei=ones, best_f=(y.max(1).values if maximize else y.min(1).values), maximize=maximize, log_ei=of == "log_ei")
        else:
            kw = {"g_" + of: ones}
        dZq, info = gp_ops.predict_grad(b, phi, Zq, q_off, **kw)
        gp_ops.check_info(info, "explanation")
        out[valid] = dZq
    if was_training:
        model.train()
    return out


def evaluate_tasks(model, tasks: Sequence[DKTBatch], names: Optional[Sequence[str]] = None, tasks_per_call: int = 64,
                   max_evals: int = 200, streaming: bool = False) -> Dict[str, object]:
    """``evaluate_adkt_model`` for tasks that are already in memory: per-task metric records, ``tasks_per_call`` tasks
    per library call (one disconnected graph each).  ``streaming`` is passed to ``meta_test``."""
    names = list(names) if names is not None else [f"task{i}" for i in range(len(tasks))]
    dev = model.device
    out: Dict[str, object] = {}
    for lo in range(0, len(tasks), tasks_per_call):
        chunk = tasks[lo:lo + tasks_per_call]
        mb = collate_meta_batch(chunk).to(dev)
        preds, _, _, _ = meta_test(model, mb, max_evals=max_evals, streaming=streaming)
        preds = preds.cpu().numpy()
        for k, task in enumerate(chunk):
            nq = task.num_query_samples
            lab = task.query_numeric_labels if model.config.use_numeric_labels else task.query_labels
            out[names[lo + k]] = _score(model, preds[k, :nq], lab.detach().cpu().numpy())
    return out


def adapt_and_test(model, optimizer, saved_state_dict, adapt_data, eval_data, update_step_test: int = 1, clip_value: float = 1.0):
    """One test task of ``Meta_Trainer.test_step`` (MoleculeNet/chem_lib/models/adkfift_trainer.py:225-283) for an ``ADKFModel``.

    ``adapt_data`` / ``eval_data``: dicts with ``s_data``, ``s_label`` and ``data_loader`` (an iterable of query batches with
    ``.to(device)`` and ``.y``), as ``get_data_sample(task_id, train=False)`` builds them.  From ``saved_state_dict`` (:226), for the
    first ``update_step_test`` batches of the adaptation loader (:229-271): re-initialise and fit the GP tail on the support set,
    IFT hypergradient of the predictive loss of the batch (fused HIP path: ONE extractor backward), clip-by-global-norm
    ``clip_value``, ``optimizer.step()``.  Then (:273-281) fit on the evaluation support set and return
    ``(sigmoid(posterior mean), labels)`` over the evaluation loader, plus the per-step outer losses."""
    from .hypergradient import cauchy_hypergradient
    from .models import fit_gpytorch_scipy

    model.load_state_dict(saved_state_dict)
    dev = model.device
    losses = []
    if update_step_test > 0:
        for i, batch in enumerate(adapt_data["data_loader"]):
            optimizer.zero_grad()
            batch = batch.to(dev) or batch          # torch_geometric's Batch.to returns the moved batch; stand-ins may move in place
            model.train()
            model(s_data=adapt_data["s_data"], q_data=None, s_label=adapt_data["s_label"], train_loss=True)      # a3/a4
            fit_gpytorch_scipy(model.mll)                                                                         # a7
            model.train()
            f_outer, f_inner = model.task_losses((adapt_data["s_data"], batch, adapt_data["s_label"]))
            loss = cauchy_hypergradient(f_outer, f_inner, tuple(model.feature_extractor_params()), tuple(model.gp_params()), dev,
                                        ignore_grad_correction=False)                                             # a9
            torch.nn.utils.clip_grad_norm_(model.feature_extractor_params(), clip_value)
            optimizer.step()
            losses.append(float(loss))
            if i >= update_step_test - 1:
                break
    model.train()
    model(s_data=eval_data["s_data"], q_data=None, s_label=eval_data["s_label"], train_loss=True)
    fit_gpytorch_scipy(model.mll)
    model.eval()
    with torch.no_grad():
        q_preds, q_labels = model.forward_query_loader(eval_data["s_data"], eval_data["data_loader"], train_loss=None,
                                                       s_label=eval_data["s_label"])
    return q_preds, q_labels, losses
