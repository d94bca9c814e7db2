"""GPU: the reference-shaped Python surface (ADKTModel modes, fit_gpytorch_scipy, cauchy_hypergradient fused path,
DKLModel, meta_step harness) against the float64 oracle / the reference-produced fixtures."""
import math
import os
from dataclasses import dataclass

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@dataclass
class Part:
    fingerprints: torch.Tensor
    descriptors: torch.Tensor


@dataclass
class Batch:  # the fields of fs_mol/data/dkt.py:32-46 that the model reads
    support_features: Part
    query_features: Part
    support_labels: torch.Tensor
    query_labels: torch.Tensor
    support_numeric_labels: torch.Tensor
    query_numeric_labels: torch.Tensor


def make_batch(dev, ns=16, nq=24, seed=0):
    g = torch.Generator().manual_seed(seed)
    fp = lambda n: torch.poisson(torch.full((n, 2048), 0.05), generator=g)
    ds = lambda n: torch.randn(n, 42, generator=g)
    lab = lambda n: torch.rand(n, generator=g) > 0.5
    num = lambda n: torch.randn(n, generator=g)
    return Batch(Part(fp(ns).to(dev), ds(ns).to(dev)), Part(fp(nq).to(dev), ds(nq).to(dev)), lab(ns).to(dev), lab(nq).to(dev),
                 num(ns).to(dev), num(nq).to(dev))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _oracle_closures(model, batch, numeric, kind):
    """float64 CPU restatement of the same model: fc head in torch, GP tail = oracle."""
    from oracle import gp_oracle as O

    names = [n for n, _ in model.named_parameters() if not n.startswith("gp_")]
    Xs = batch.support_features.fingerprints.double().cpu()
    Xq = batch.query_features.fingerprints.double().cpu()
    if numeric:
        ys, yq = batch.support_numeric_labels.double().cpu(), batch.query_numeric_labels.double().cpu()
    else:
        ys, yq = (batch.support_labels.double().cpu() - 0.5) * 2, (batch.query_labels.double().cpu() - 0.5) * 2
    pr = model.mll.priors_row(torch.device("cpu"))[0].double().tolist()
    pri = O.Priors(*pr)

    def feats(po, X):
        W1, b1, W2, b2 = po
        return torch.relu(X @ W1.T + b1) @ W2.T + b2

    f_in = lambda po, pi: O.f_inner(feats(po, Xs), ys, torch.cat([p.reshape(-1) for p in pi]), pri, kind)
    f_out = lambda po, pi: O.f_outer(feats(po, Xs), ys, feats(po, Xq), yq, torch.cat([p.reshape(-1) for p in pi]), kind)
    return f_out, f_in, names


@pytest.mark.parametrize("kernel,numeric", [("matern", False), ("rbf", True)])
def test_adkt_model_modes_and_fused_hypergradient(dev, kernel, numeric):
    from adkf_ift_amd.hypergradient import cauchy_hypergradient
    from adkf_ift_amd.models import ADKTModel, ADKTModelConfig, fit_gpytorch_scipy
    from oracle import gp_oracle as O
    from oracle.hypergrad_oracle import dense_ift_hypergradient

    torch.manual_seed(0)
    cfg = ADKTModelConfig(used_features="ecfp+fc", gp_kernel=kernel, use_numeric_labels=numeric, fc_hidden_dim=32, fc_out_dim=16)
    model = ADKTModel(cfg).to(dev)
    batch = make_batch(dev)
    kind = 0 if kernel == "rbf" else 1
    # mode 1: re-initialisation (returns None, fresh GP params with the median heuristic)
    model.train()
    assert model(batch, train_loss=True) is None
    names = [n for n, _ in model.named_parameters() if n.startswith("gp_")]
    assert names == ["gp_likelihood.noise_covar.raw_noise", "gp_model.covar_module.raw_outputscale",
                     "gp_model.covar_module.base_kernel.raw_lengthscale"]
    assert [tuple(p.shape) for p in model.gp_params()] == [(1,), (), (1, 1)]
    Zs = model._features(batch.support_features).detach()
    l0 = O.median_lengthscale_init(Zs.double().cpu()).item()
    assert abs(model.gp_model.covar_module.base_kernel.lengthscale.item() - l0) <= 1e-5 * l0
    assert abs(model.gp_likelihood.noise.item() - (0.01 if numeric else 0.1)) < 1e-6
    # inner fit through the BoTorch-shaped entry point
    _, info = fit_gpytorch_scipy(model.mll)
    assert info["max_abs_grad"] < 5e-4
    # mode 2/3: f_inner and f_outer values + first-order autograd
    f_outer, f_inner = model.task_losses(batch)
    po, pi = tuple(model.feature_extractor_params()), tuple(model.gp_params())
    fo_ref, fi_ref, _ = _oracle_closures(model, batch, numeric, kind)
    po64 = tuple(p.detach().double().cpu().requires_grad_(True) for p in po)
    pi64 = tuple(p.detach().double().cpu().requires_grad_(True) for p in pi)
    vi, vo = f_inner(po, pi), f_outer(po, pi)
    ri, ro = fi_ref(po64, pi64), fo_ref(po64, pi64)
    assert abs(vi.item() - ri.item()) <= 1e-4 * abs(ri.item())
    assert abs(vo.item() - ro.item()) <= 1e-4 * abs(ro.item())
    g_got = torch.autograd.grad(vo, po + pi)
    g_ref = torch.autograd.grad(ro, po64 + pi64)
    # (the last-layer bias has an exactly-zero gradient - distances are translation invariant - so errors are
    # measured against the largest gradient entry of the whole parameter set, not per tensor)
    gscale = max(b.abs().max().item() for b in g_ref[: len(po)])
    for a, b in zip(g_got, g_ref):
        assert (a.double().cpu() - b).abs().max() <= 2e-4 * max(b.abs().max().item(), gscale)
    # the fused IFT hypergradient == the reference algorithm (dense) on the float64 restatement
    val = cauchy_hypergradient(f_outer, f_inner, po, pi, dev)
    ref_val = dense_ift_hypergradient(fo_ref, fi_ref, po64, pi64)
    assert abs(val.item() - ref_val.item()) <= 1e-4 * abs(ref_val.item())
    hscale = max(b.grad.abs().max().item() for b in po64)
    for a, b in zip(po, po64):
        assert (a.grad.double().cpu() - b.grad).abs().max() <= 2e-4 * max(b.grad.abs().max().item(), hscale), (a.shape,)
    for a, b in zip(pi, pi64):
        assert (a.grad.double().cpu() - b.grad).abs().max() <= 2e-4 * max(b.grad.abs().max().item(), 1e-2)
    # first-order flag
    cauchy_hypergradient(f_outer, f_inner, po, pi, dev, ignore_grad_correction=True)
    for a, b in zip(po, g_ref[: len(po)]):
        assert (a.grad.double().cpu() - b).abs().max() <= 2e-4 * max(b.abs().max().item(), gscale)
    # eval mode: posterior with noise
    model.eval()
    post = model(batch, train_loss=None)
    Zq = model._features(batch.query_features).detach()
    ys = batch.support_numeric_labels if numeric else (batch.support_labels.float() - 0.5) * 2
    phi = torch.cat([p.detach().reshape(-1) for p in pi]).double().cpu()
    mean, cov = O.predict(Zs.double().cpu(), ys.double().cpu(), Zq.double().cpu(), phi, kind)
    assert (post.mean.double().cpu() - mean).abs().max() <= 1e-4 * mean.abs().max()
    assert (post.covariance_matrix.double().cpu() - cov).abs().max() <= 1e-4 * cov.abs().max()
    yq = batch.query_numeric_labels if numeric else (batch.query_labels.float() - 0.5) * 2
    lp = post.log_prob(yq)
    assert abs(lp.item() + O.f_outer(Zs.double().cpu(), ys.double().cpu(), Zq.double().cpu(), yq.double().cpu(), phi, kind).item()) <= 2e-4 * abs(lp.item())


def test_dkl_model_surface(dev):
    from adkf_ift_amd.models import DKLModel, DKLModelConfig
    from oracle import gp_oracle as O

    torch.manual_seed(1)
    model = DKLModel(DKLModelConfig(used_features="ecfp+fc", gp_kernel="rbf", use_lengthscale_prior=True, fc_hidden_dim=16, fc_out_dim=8)).to(dev)
    batch = make_batch(dev, seed=3)
    model.train()
    loss = model.compute_loss(model(batch, train=True))
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    Zs = model._features(batch.support_features).detach().double().cpu()
    ys = (batch.support_labels.double().cpu() - 0.5) * 2
    phi = torch.cat([p.detach().reshape(-1) for p in model.mll.raw_params()]).double().cpu()
    # no noise prior in DKL (fs_mol/models/dkl.py:86): evaluate the oracle's terms without it
    noise, os_, ls = O.transform_phi(phi)
    A = O.kernel_matrix(Zs, Zs, os_, ls, 0) + noise * torch.eye(Zs.shape[0], dtype=torch.float64)
    ref = -(O.mvn_log_prob(ys, torch.zeros_like(ys), A) + O.lognormal_log_prob(ls, 0.0, 0.25)) / Zs.shape[0]
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
    model.eval()
    post = model(batch, train=False)
    assert post.mean.shape == (24,) and torch.isfinite(post.mean).all()


def test_batched_meta_step_equals_per_task_reference_loop(dev):
    """Config-3 shape: GNN + fc features (PyTorch-ROCm) -> HIP GP path, few-shot molecular tasks with ragged sizes.
    The batched meta-step (one extractor forward/backward for all tasks) must give the gradient of the reference-shaped
    per-task loop: model(batch, train_loss=True) -> fit_gpytorch_scipy -> cauchy_hypergradient -> mean over tasks."""
    from adkf_ift_amd.hypergradient import cauchy_hypergradient
    from adkf_ift_amd.meta_batch import collate_meta_batch, model_meta_step
    from adkf_ift_amd.models import ADKTModel, fit_gpytorch_scipy
    from test_meta_batch import random_task, small_model

    torch.manual_seed(0)
    model = ADKTModel(small_model()).to(dev)
    with torch.no_grad():
        for blk in model.graph_feature_extractor.gnn.gnn_blocks:
            blk.alpha.fill_(0.5)
    tasks = [random_task(16, 24, 11).to(dev), random_task(12, 30, 12).to(dev), random_task(16, 9, 13).to(dev)]
    # reference-shaped loop (fs_mol/utils/adaptive_dkt_utils.py:361-407)
    acc = [torch.zeros_like(p) for p in model.feature_extractor_params()]
    losses = []
    for b in tasks:
        model.train()
        model(b, train_loss=True)
        fit_gpytorch_scipy(model.mll)
        f_outer, f_inner = model.task_losses(b)
        val = cauchy_hypergradient(f_outer, f_inner, tuple(model.feature_extractor_params()), tuple(model.gp_params()), dev)
        losses.append(val.item() / b.num_query_samples)
        for a, p in zip(acc, model.feature_extractor_params()):
            a += p.grad / len(tasks)
    # batched path
    mb = collate_meta_batch(tasks).to(dev)
    for p in model.parameters():
        p.grad = None
    from adkf_ift_amd.trainer import MetaStepConfig
    cfg = MetaStepConfig(gp_kernel="matern", clip_value=None)
    got_losses, _ = model_meta_step(model, None, mb, cfg, check=True)
    scale = max(a.abs().max().item() for a in acc)
    for a, p in zip(acc, model.feature_extractor_params()):
        if "mp_norm_layer" in [n for n, q in model.named_parameters() if q is p][0]:
            continue
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        assert (g - a).abs().max().item() <= 2e-3 * scale, ((g - a).abs().max().item(), scale)
    assert np.abs(got_losses.cpu().numpy() - np.array(losses)).max() <= 1e-3 * np.abs(losses).max()


def test_dkt_model_joint_mll_and_test_time_adaptation(dev):
    """fs_mol/models/dkt.py: training loss = -MLL of support U query under shared GP parameters; evaluation conditions
    on the support set, optionally after re-fitting from the saved meta-learned parameters."""
    from adkf_ift_amd.models import DKTModel, DKTModelConfig
    from oracle import gp_oracle as O

    torch.manual_seed(2)
    model = DKTModel(DKTModelConfig(used_features="ecfp+fc", gp_kernel="matern", fc_hidden_dim=16, fc_out_dim=8)).to(dev)
    batch = make_batch(dev, ns=16, nq=24, seed=5)
    model.train()
    loss = model.compute_loss(model(batch))
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    Zs = model._features(batch.support_features).detach().double().cpu()
    Zq = model._features(batch.query_features).detach().double().cpu()
    ys, yq = (batch.support_labels.double().cpu() - 0.5) * 2, (batch.query_labels.double().cpu() - 0.5) * 2
    phi = torch.cat([p.detach().reshape(-1) for p in model.mll.raw_params()]).double().cpu()
    noise, os_, ls = O.transform_phi(phi)
    Z, y = torch.cat([Zs, Zq]), torch.cat([ys, yq])
    A = O.kernel_matrix(Z, Z, os_, ls, 1) + noise * torch.eye(40, dtype=torch.float64)
    ref = -O.mvn_log_prob(y, torch.zeros_like(y), A) / 40
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
    model.save_gp_params()
    model.eval()
    post = model(batch)
    mean, cov = O.predict(Zs, ys, Zq, phi, 1)
    assert (post.mean.double().cpu() - mean).abs().max().item() <= 1e-4 * max(1.0, mean.abs().max().item())
    model.test_time_adaptation = True
    post2 = model(batch)
    phi2 = torch.cat([p.detach().reshape(-1) for p in model.mll.raw_params()]).double().cpu()
    def nll(p):   # no priors in DKT (fs_mol/models/dkt.py:85)
        n_, o_, l_ = O.transform_phi(p)
        return -O.mvn_log_prob(ys, torch.zeros_like(ys), O.kernel_matrix(Zs, Zs, o_, l_, 1) + n_ * torch.eye(16, dtype=torch.float64)) / 16
    assert nll(phi2).item() < nll(phi).item()
    mean2, _ = O.predict(Zs, ys, Zq, phi2, 1)
    assert (post2.mean.double().cpu() - mean2).abs().max().item() <= 1e-4 * max(1.0, mean2.abs().max().item())


def test_moleculenet_adkf_model_fused_hypergradient(dev):
    """MoleculeNet/chem_lib/models/adkf_model.py + adkfift_trainer.py:173-201 with a stand-in encoder: reinit + fit +
    cauchy_hypergradient through the pluggable-encoder model equals the dense reference algorithm on the oracle."""
    from types import SimpleNamespace
    from adkf_ift_amd.hypergradient import cauchy_hypergradient
    from adkf_ift_amd.models import ADKFModel, fit_gpytorch_scipy
    from oracle import gp_oracle as O
    from oracle.hypergrad_oracle import dense_ift_hypergradient

    class Enc(torch.nn.Module):   # signature of the reference's GNN_Encoder: (x, edge_index, edge_attr, batch) -> (emb, node_emb)
        def __init__(self):
            super().__init__()
            self.l1, self.l2 = torch.nn.Linear(10, 16), torch.nn.Linear(16, 6)
        def forward(self, x, edge_index, edge_attr, batch):
            return self.l2(torch.tanh(self.l1(x))), None

    torch.manual_seed(4)
    g = torch.Generator().manual_seed(4)
    data = lambda n: SimpleNamespace(x=torch.randn(n, 10, generator=g).to(dev), edge_index=None, edge_attr=None, batch=None,
                                     y=(torch.rand(n, generator=g) > 0.5).to(dev), to=lambda d: None)
    s_data, q_data = data(20), data(32)
    q_data.to = lambda d: q_data
    model = ADKFModel(Enc(), 6, "matern").to(dev)
    model.train()
    assert model(s_data, q_data, train_loss=True, s_label=s_data.y) is None      # re-initialises the GP tail
    fit_gpytorch_scipy(model.mll)
    f_outer, f_inner = model.task_losses((s_data, q_data, s_data.y))
    po, pi = tuple(model.feature_extractor_params()), tuple(model.gp_params())
    val = cauchy_hypergradient(f_outer, f_inner, po, pi, dev)
    # oracle: same encoder in float64 on the CPU
    enc64 = Enc().double()
    enc64.load_state_dict({k: v.double().cpu() for k, v in model.mol_encoder.state_dict().items()})
    names = [n for n, _ in enc64.named_parameters()]
    Xs, Xq = s_data.x.double().cpu(), q_data.x.double().cpu()
    ys, yq = (s_data.y.double().cpu() - 0.5) * 2, (q_data.y.double().cpu() - 0.5) * 2
    pri = O.Priors(*model.mll.priors_row(torch.device("cpu"))[0].double().tolist())
    from torch.func import functional_call as fc
    feats = lambda p, X: fc(enc64, dict(zip(names, p)), (X, None, None, None))[0]
    fin = lambda p, q: O.f_inner(feats(p, Xs), ys, torch.cat([t.reshape(-1) for t in q]), pri, 1)
    fout = lambda p, q: O.f_outer(feats(p, Xs), ys, feats(p, Xq), yq, torch.cat([t.reshape(-1) for t in q]), 1)
    p64 = tuple(p.detach().double().cpu().requires_grad_() for p in enc64.parameters())
    q64 = tuple(p.detach().double().cpu().requires_grad_() for p in pi)
    ref_val = dense_ift_hypergradient(fout, fin, p64, q64)
    assert abs(val.item() - ref_val.item()) <= 1e-4 * abs(ref_val.item())
    scale = max(q.grad.abs().max().item() for q in p64)
    for p, q in zip(po, p64):
        assert (p.grad.double().cpu() - q.grad).abs().max().item() <= 2e-4 * scale
    model.eval()
    probs, labels = model.forward_query_loader(s_data, [q_data], s_label=s_data.y)
    assert probs.shape == (32,) and labels.shape == (32,) and ((probs > 0) & (probs < 1)).all()


def test_moleculenet_test_time_adaptation_vs_per_step_oracle(dev):
    """MoleculeNet/chem_lib/models/adkfift_trainer.py:225-283 (``update_step_test`` hypergradient steps per test task before the
    final fit) through ``evaluate.adapt_and_test``, against the per-step float64 oracle loop evaluated AT THE DEVICE'S fitted phi:
    step k: theta_k -> (device: reinit, fit -> phi_k) -> oracle dense IFT hypergradient at (theta_k^oracle, phi_k) -> clip 1.0 ->
    SGD step; finally the oracle's predictive mean at the device's last phi."""
    from types import SimpleNamespace
    from adkf_ift_amd import evaluate as E
    from adkf_ift_amd.models import ADKFModel
    from oracle import gp_oracle as O
    from oracle.hypergrad_oracle import dense_ift_hypergradient

    class Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.l1, self.l2 = torch.nn.Linear(10, 16), torch.nn.Linear(16, 6)
        def forward(self, x, edge_index, edge_attr, batch):
            return self.l2(torch.tanh(self.l1(x))), None

    torch.manual_seed(8)
    g = torch.Generator().manual_seed(8)
    def data(n):
        d = SimpleNamespace(x=torch.randn(n, 10, generator=g).to(dev), edge_index=None, edge_attr=None, batch=None,
                            y=(torch.rand(n, generator=g) > 0.5).to(dev))
        d.to = lambda device: d
        return d
    s_data = data(20)
    adapt_loader = [data(24), data(16), data(32)]        # the third batch must not be used (update_step_test = 2)
    eval_loader = [data(12), data(9)]
    model = ADKFModel(Enc(), 6, "matern").to(dev)
    saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
    lr = 0.05
    opt = torch.optim.SGD(model.feature_extractor_params(), lr=lr)
    # record the phi the device fits in every adaptation step (the oracle is evaluated there) through the public surface
    phis = []
    from adkf_ift_amd import models as M
    orig_fit = M.fit_gpytorch_scipy
    def spy(mll, *a, **k):
        out = orig_fit(mll, *a, **k)
        phis.append(torch.cat([p.detach().reshape(-1) for p in mll.raw_params()]).double().cpu())
        return out
    M.fit_gpytorch_scipy = spy
    try:
        adapt = {"s_data": s_data, "s_label": s_data.y, "data_loader": adapt_loader}
        evald = {"s_data": s_data, "s_label": s_data.y, "data_loader": eval_loader}
        with torch.no_grad():
            for p in model.parameters():
                p.add_(1.0)                               # must be undone by load_state_dict(saved_state_dict) (:226)
        preds, labels, losses = E.adapt_and_test(model, opt, saved, adapt, evald, update_step_test=2)
    finally:
        M.fit_gpytorch_scipy = orig_fit
    assert len(phis) == 3 and len(losses) == 2            # two adaptation fits + the final one
    assert preds.shape == (21,) and labels.shape == (21,)
    # ---- oracle loop (float64, CPU) ----
    enc64 = Enc().double()
    enc64.load_state_dict({k[len("mol_encoder."):]: v.double().cpu() for k, v in saved.items() if k.startswith("mol_encoder.")})
    names = [n for n, _ in enc64.named_parameters()]
    from torch.func import functional_call as fc
    feats = lambda p, X: fc(enc64, dict(zip(names, p)), (X, None, None, None))[0]
    Xs, ys = s_data.x.double().cpu(), (s_data.y.double().cpu() - 0.5) * 2
    theta = [p.detach().clone() for p in enc64.parameters()]
    for k in range(2):
        Xq, yq = adapt_loader[k].x.double().cpu(), (adapt_loader[k].y.double().cpu() - 0.5) * 2
        with torch.no_grad():
            _, pri = O.init_phi(feats(tuple(theta), Xs), False, True)
        fin = lambda p, q: O.f_inner(feats(p, Xs), ys, torch.cat([t.reshape(-1) for t in q]), pri, 1)
        fout = lambda p, q: O.f_outer(feats(p, Xs), ys, feats(p, Xq), yq, torch.cat([t.reshape(-1) for t in q]), 1)
        p64 = tuple(t.clone().requires_grad_() for t in theta)
        q64 = (phis[k][0:1].clone().requires_grad_(), phis[k][1].clone().requires_grad_(), phis[k][2:3].reshape(1, 1).clone().requires_grad_())
        val = dense_ift_hypergradient(fout, fin, p64, q64)
        assert abs(losses[k] - val.item()) <= 2e-4 * abs(val.item()), (k, losses[k], val.item())
        total = torch.sqrt(sum((q.grad ** 2).sum() for q in p64))
        coef = min(1.0, 1.0 / (float(total) + 1e-6))      # torch.nn.utils.clip_grad_norm_(..., 1.0)
        theta = [t - lr * coef * q.grad for t, q in zip(theta, p64)]
    scale = max(float((t - s.double().cpu()).abs().max()) for t, s in zip(theta, (saved["mol_encoder." + n] for n in names)))
    assert scale > 0.0
    for t, n in zip(theta, names):                         # the adapted weights: 2e-4 of the largest movement
        got = dict(model.mol_encoder.named_parameters())[n].detach().double().cpu()
        assert float((got - t).abs().max()) <= 2e-4 * scale, n
    with torch.no_grad():
        Zs = feats(tuple(theta), Xs)
        want = torch.cat([torch.sigmoid(O.predict(Zs, ys, feats(tuple(theta), q.x.double().cpu()), phis[2], 1)[0]) for q in eval_loader])
    assert float((preds.double().cpu() - want).abs().max()) <= 2e-4


def test_bayes_opt_gp_ei_loop(dev):
    """bayes_opt/bo_utils.py create_gp + EI: the fitted GP's latent posterior and EI values against the oracle, and
    a short BO run on a toy objective whose minimiser must be found."""
    from adkf_ift_amd import bayes_opt as BO
    from adkf_ift_amd.models import fit_gpytorch_scipy
    from oracle import gp_oracle as O

    g = torch.Generator().manual_seed(0)
    X = torch.randn(60, 5, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)           # ascending y: index 0 is the optimum
    idx = [40, 45, 50, 55, 59, 30]
    ys = (y - y.mean()) / y.std()
    lik, model, mll = BO.create_gp(X[idx], ys[idx], "matern", dev, noise_init=0.01, noise_prior=True)
    fit_gpytorch_scipy(mll)
    mean, var = BO.latent_posterior(model, mll, X)
    phi = torch.cat([p.detach().reshape(-1) for p in mll.raw_params()]).double().cpu()
    m_ref, cov = O.predict(X[idx].double().cpu(), ys[idx].double().cpu(), X.double().cpu(), phi, 1)
    noise = O.transform_phi(phi)[0]
    v_ref = cov.diagonal() - noise
    assert (mean.double().cpu() - m_ref).abs().max().item() <= 1e-4 * max(1.0, m_ref.abs().max().item())
    free = [i for i in range(60) if i not in idx]
    assert (var.double().cpu()[free] - v_ref[free]).abs().max().item() <= 2e-4 * v_ref.abs().max().item()
    ei = BO.expected_improvement(mean, var, ys[idx].min().item())
    s = v_ref.clamp_min(1e-12).sqrt()
    u = (ys[idx].min().item() - m_ref) / s
    nrm = torch.distributions.Normal(0.0, 1.0)
    ei_ref = s * (u * nrm.cdf(u) + torch.exp(nrm.log_prob(u)))
    assert (ei.double().cpu()[free] - ei_ref[free]).abs().max().item() <= 1e-3 * ei_ref[free].abs().max().item()
    rec = BO.run_gp_ei_bo(X, y, num_init_points=6, query_batch_size=2, num_bo_iters=8, kernel_type="matern", device=dev,
                          init_from=20, noise_init=0.01, noise_prior=True, rng=np.random.default_rng(0))
    assert len(rec) == 1 + 8 * 2 and len(set(rec[1:])) == 16
    assert min(rec) <= 2          # reaches (one of) the best three points out of 60 within 16 queries


def test_graph_replay_equals_eager(dev):
    """GraphedGPBackend: the captured init -> fit -> hypergradient sequence replayed on new inputs gives exactly what the
    eager backend computes (the library enqueues only kernels/memsets, so it is graph-capturable as the ABI promises)."""
    from adkf_ift_amd.synthetic import make_tasks
    from adkf_ift_amd.trainer import GraphedGPBackend, HipGPBackend, MetaStepConfig

    cfg = MetaStepConfig(gp_kernel="matern", inner_max_evals=60)
    graphed, eager = GraphedGPBackend(), HipGPBackend()
    for first in (0, 50):     # second round: same shapes, different data -> pure replay
        tasks = make_tasks(6, 24, 16, N_q=20, first_task=first)
        Zs, Zq = tasks.features()
        args = (Zs.to(dev), tasks.y_s.to(dev), Zq.to(dev), tasks.y_q.to(dev), cfg)
        got = [t.clone() for t in graphed.run(*args)]
        want = eager.run(*args)
        for a, b, name in zip(got, want, ("phi", "f_out", "dZ_s", "dZ_q", "info_fit", "info")):
            assert torch.equal(a, b), name
    assert len(graphed._graphs) == 1


@pytest.mark.parametrize("kind", ["PNA", "MultiAggr"])
def test_fused_pna_aggregation_equals_torch_path(dev, kind):
    """csrc/pna.h: the fused sum | mean | std | max aggregation (forward and backward) against the index_add /
    scatter_reduce formulation it replaces (which tests/test_gnn.py pins to the naive restatement of the reference):
    same extractor, float32 on the GPU (fused) vs float64 on the CPU (PyTorch ops)."""
    from adkf_ift_amd.gnn import GNNConfig, GraphFeatureExtractor, GraphFeatureExtractorConfig, GraphReadoutConfig
    from test_gnn import random_graphs

    torch.manual_seed(0)
    cfg = GraphFeatureExtractorConfig(gnn_config=GNNConfig(type=kind, hidden_dim=16, num_heads=4, per_head_dim=6, intermediate_dim=24,
                                                          num_layers=3),
                                      readout_config=GraphReadoutConfig(num_heads=3, head_dim=5, output_dim=10))
    ref = GraphFeatureExtractor(cfg).double()
    with torch.no_grad():
        for blk in ref.gnn.gnn_blocks:
            blk.alpha.fill_(0.6)
    gpu = GraphFeatureExtractor(cfg).to(dev)
    gpu.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    batch = random_graphs(9, seed=4, empty_type=1)      # isolated nodes, a single-atom graph, an empty edge type
    out_ref = ref(batch)
    b32 = batch.to(dev)
    b32.node_features = b32.node_features.float()
    out = gpu(b32)
    assert (out.double().cpu() - out_ref).abs().max().item() <= 2e-5 * out_ref.abs().max().item()
    w = torch.randn(out_ref.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    (out_ref * w).sum().backward()
    (out * w.float().to(dev)).sum().backward()
    scale = max(p.grad.abs().max().item() for n, p in ref.named_parameters() if p.grad is not None)
    for (n, p), (_, q) in zip(ref.named_parameters(), gpu.named_parameters()):
        if p.grad is None:
            assert q.grad is None, n
            continue
        assert (q.grad.double().cpu() - p.grad).abs().max().item() <= 2e-4 * scale, n


@pytest.mark.parametrize("clip, wd", [(1.0, 0.0), (1e9, 0.0), (None, 0.0), (0.3, 0.01)])
def test_clip_adam_equals_clip_grad_norm_plus_torch_adam(dev, clip, wd):
    """H: adkf_grad_sumsq + adkf_clip_adam_step == {grad *= 1/T, clip_grad_norm_, torch.optim.Adam.step} over several
    steps, for sizes with and without a 4-element tail, and the optimiser state interchanges with torch's."""
    from adkf_ift_amd.trainer import ClipAdam, _mean_and_clip_

    g = torch.Generator().manual_seed(5)
    shapes = [(256, 256), (1027,), (3, 5)]
    ref = [torch.randn(s, generator=g).to(dev).requires_grad_(True) for s in shapes]
    new = [p.detach().clone().requires_grad_(True) for p in ref]
    o_ref = torch.optim.Adam(ref, lr=1e-2, weight_decay=wd)
    o_new = ClipAdam(new, lr=1e-2, weight_decay=wd)
    scale = 1.0 / 16.0
    for step in range(4):
        grads = [torch.randn(s, generator=g).to(dev) * 10.0 ** (step - 1) for s in shapes]
        for p, q, gr in zip(ref, new, grads):
            p.grad = gr.clone()
            q.grad = gr.clone()
        if clip is None:
            torch._foreach_mul_([p.grad for p in ref], scale)
        else:
            torch._foreach_mul_([p.grad for p in ref], scale)
            torch.nn.utils.clip_grad_norm_(ref, clip)
        o_ref.step()
        o_new.clip_step(scale, clip)
        for p, q in zip(ref, new):
            assert (q.grad - p.grad).abs().max() <= 2e-6 * p.grad.abs().max(), (step, "clipped gradient")
            assert (q - p).abs().max() <= 2e-6 * p.abs().max() + 1e-7, (step, "parameter")
    for p, q in zip(ref, new):
        sr, sn = o_ref.state[p], o_new.state[q]
        assert float(sr["step"]) == float(sn["step"]) == 4.0
        assert (sr["exp_avg"] - sn["exp_avg"]).abs().max() <= 2e-6 * sr["exp_avg"].abs().max()
        assert (sr["exp_avg_sq"] - sn["exp_avg_sq"]).abs().max() <= 4e-6 * sr["exp_avg_sq"].abs().max()
    # state interchange: a torch Adam continues from ClipAdam's state and vice versa
    o_t = torch.optim.Adam(new, lr=1e-2, weight_decay=wd)
    o_t.load_state_dict(o_new.state_dict())
    o_c = ClipAdam(ref, lr=1e-2, weight_decay=wd)
    o_c.load_state_dict(o_ref.state_dict())
    for p, q in zip(ref, new):
        gr = torch.randn(p.shape, generator=g).to(dev)
        p.grad, q.grad = gr.clone(), gr.clone()
    o_t.step()
    o_c.clip_step(1.0, None)
    for p, q in zip(ref, new):
        assert (q - p).abs().max() <= 4e-6 * p.abs().max() + 1e-7
    # determinism: the same gradient gives the same bits twice (fixed partial-sum order)
    a = [torch.zeros(1 << 16, device=dev).requires_grad_(True) for _ in range(2)]
    gr = torch.randn(1 << 16, generator=g).to(dev)
    outs = []
    for p in a:
        p.grad = gr.clone()
        ClipAdam([p], lr=1e-2).clip_step(1.0, 1.0)
        outs.append(p.detach().clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("T,N,Nq,d,kern", [(1, 2, 1, 3, "rbf"), (3, 2, 5, 1, "matern"), (300, 17, 9, 5, "rbf"),
                                           (9, 129, 40, 33, "matern"), (5, 64, 130, 7, "rbf"), (2, 200, 200, 35, "rbf")])
def test_awkward_shapes_match_oracle(dev, T, N, Nq, d, kern):
    """Edges of the launch geometry: task counts that are not multiples of 8 (XCD map), two points, feature widths with K tails
    (3, 5, 7, 33, 35: checked staging path + fused row norms), support / query counts just past the register-resident size."""
    from adkf_ift_amd import gp_ops
    from adkf_ift_amd.synthetic import make_tasks
    from oracle import gp_oracle as O

    tasks = make_tasks(T, N, d, N_q=Nq)
    Zs, Zq = tasks.features()
    phi, pri, _ = gp_ops.init_params(Zs.to(dev))
    b = gp_ops.GPBatch(Zs.to(dev), tasks.y_s.to(dev), pri, kern, Z_q=Zq.to(dev), y_q=tasks.y_q.to(dev))
    phi, f, gn, ne, info = gp_ops.fit(b, phi, max_evals=40)
    gp_ops.check_info(info)
    out = gp_ops.ift_hypergrad(b, phi)
    gp_ops.check_info(out["info"])
    kind = gp_ops.kernel_id(kern)
    for t in sorted({0, T // 2, T - 1}):
        p = O.Priors(*pri[t].double().cpu().tolist())
        q = O.full_reference_quantities(Zs[t], tasks.y_s[t], Zq[t], tasks.y_q[t], phi[t].double().cpu(), p, kind)
        assert abs(f[t].item() - q["f_in"]) <= 1e-5 * abs(q["f_in"])
        assert abs(out["f_out"][t].item() - q["f_out"]) <= 1e-5 * abs(q["f_out"])
        ref = np.asarray(q["dZs_total"])
        assert np.abs(out["dZ_s"][t].cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()
        refq = np.asarray(q["dZq_total"])
        assert np.abs(out["dZ_q"][t].cpu().numpy() - refq).max() <= 1e-4 * max(np.abs(refq).max(), 1e-30)


@pytest.mark.parametrize("shape, clip, wd", [((256, 256), 1.0, 0.0), ((64, 128), None, 0.01), ((1027,), 0.3, 0.0), ((512, 256), 1e9, 0.0)])
def test_one_launch_clip_adam_and_the_planes_it_writes(dev, shape, clip, wd):
    """H: adkf_clip_adam_step_one (one tensor, one launch) == {grad *= 1/T, clip_grad_norm_, torch.optim.Adam.step}; the bfloat16 planes
    it writes for a [K, N] weight are adkf_split_planes_t of the UPDATED weight bit for bit; fresh_planes goes stale on an in-place
    change of the weight; beyond ADKF_CLIP_ADAM_ONE_MAX the two-launch form runs and writes no planes."""
    from adkf_ift_amd import dense
    from adkf_ift_amd.trainer import ClipAdam

    g = torch.Generator().manual_seed(11)
    p = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
    q = p.detach().clone().requires_grad_(True)
    o_ref = torch.optim.Adam([p], lr=1e-2, weight_decay=wd)
    o_new = ClipAdam([q], lr=1e-2, weight_decay=wd)
    two_d = len(shape) == 2
    one_launch = q.numel() <= ClipAdam.ONE_MAX
    if two_d:
        planes = torch.full((3, shape[1], shape[0]), -1, dtype=torch.int16, device=dev)
        o_new.attach_planes(q, planes)
        assert o_new.fresh_planes(q) is None
    scale = 1.0 / 16.0
    for step in range(3):
        gr = torch.randn(shape, generator=g).to(dev) * 10.0 ** (step - 1)
        p.grad, q.grad = gr.clone(), gr.clone()
        p.grad.mul_(scale)
        if clip is not None:
            torch.nn.utils.clip_grad_norm_([p], clip)
        o_ref.step()
        o_new.clip_step(scale, clip)
        assert (q.grad - p.grad).abs().max() <= 2e-6 * p.grad.abs().max(), step
        assert (q - p).abs().max() <= 2e-6 * p.abs().max() + 1e-7, step
        if two_d and one_launch:
            got = o_new.fresh_planes(q)
            assert got is planes
            assert torch.equal(got, dense._split_t(q.detach())), step
        elif two_d:
            assert o_new.fresh_planes(q) is None
    sr, sn = o_ref.state[p], o_new.state[q]
    assert float(sr["step"]) == float(sn["step"]) == 3.0
    assert (sr["exp_avg"] - sn["exp_avg"]).abs().max() <= 2e-6 * sr["exp_avg"].abs().max()
    assert (sr["exp_avg_sq"] - sn["exp_avg_sq"]).abs().max() <= 4e-6 * sr["exp_avg_sq"].abs().max()
    if two_d and one_launch:
        with torch.no_grad():
            q.mul_(1.0)      # any in-place change: the planes no longer belong to the weights
        assert o_new.fresh_planes(q) is None
    # same gradient, same bits: every workgroup (and every rank) re-adds the squares in one fixed order
    outs = []
    for _ in range(2):
        a = torch.zeros(shape, device=dev).requires_grad_(True)
        a.grad = gr.clone()
        ClipAdam([a], lr=1e-2).clip_step(1.0, 1.0)
        outs.append(a.detach().clone())
    assert torch.equal(outs[0], outs[1])


def test_feature_map_forward_on_the_optimisers_planes_is_the_split_one_bit_for_bit(dev):
    """The C2 stand-in feature map: with planes_from(opt) the forward product after an optimiser step reads the planes that step wrote;
    Z is identical to the one computed through adkf_split_planes_t."""
    from adkf_ift_amd.synthetic import LinearFeatureMap
    from adkf_ift_amd.trainer import ClipAdam

    g = torch.Generator().manual_seed(3)
    T, N, d = 128, 128, 256
    X_s, X_q = torch.randn(T, N, d, generator=g).to(dev), torch.randn(T, N, d, generator=g).to(dev)
    W = torch.randn(d, d, generator=g).to(dev).requires_grad_(True)
    opt = ClipAdam([W], lr=1e-2)
    fm, fm_split = LinearFeatureMap(X_s, X_q, W), LinearFeatureMap(X_s, X_q, W)
    fm.planes_from(opt)
    for step in range(2):
        Z = fm()
        assert torch.equal(Z, fm_split()), step
        W.grad = None
        Z.square().mean().backward()
        opt.clip_step(1.0, 1.0)
        assert opt.fresh_planes(W) is not None
    assert torch.equal(fm(), fm_split())
