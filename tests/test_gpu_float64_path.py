"""GPU: the float64 path of ill-conditioned tasks (csrc/refine64.h: k_refine64, k_tail64; the FP64-MFMA products r64_mm_direct /
r64_mm_staged, the register, in-LDS and blocked inverses, r64_mv / r64_mv_cols, r64_distances) held to FLOAT64 accuracy on the seeded cases
of tests/r64_inputs.py: every output of a flagged task against oracle.gp_oracle in float64 at the float32 phi, within 2 (S_k + R slack_k) -
what the reference itself moves by when one transformed hyper-parameter moves by four float32 ulps, plus the one rounding of the output
(r64_inputs.py's docstring; tests/test_r64_inputs.py shows the bounds are 4 to 1000 times sharper than the suite's 1e-4 x slack and that a
task left on the float32 path would miss them by more than ten times).  Tasks are flagged by their conditioning alone; no switch is set.

Outputs that keep a float32 step BY DESIGN, with a yardstick of their own (twice the error of a CPU float32 emulation of exactly that
step applied to the float64 reference, r64_inputs.predict_float32_step):
  * the predictive variance and covariance of adkf_predict: level 1 of k_refine64 hands C = K_qs A^-1 back rounded to float32
    (csrc/refine64.h, "if (a.C)" in refine64_task; host_gp.h predict_core) and k_predict (csrc/kernels.h) / ProbS finish in float32,
    s - sum_j C_ij K_ij + noise being a cancellation from s down to the noise.
The predictive MEAN goes the same way (k_predict: sum_j C_ij y_j in float32) and still meets the float64 bound.

tools/float64_path_check.py writes every (case, task, entry point, output, error, bound) of this file to
profiles/float64_path_check.json.  Worst error / bound there: see WORST below."""
import numpy as np
import pytest
import torch

import r64_inputs as I

pytestmark = pytest.mark.gpu

TOL = 1e-4      # what unflagged tasks are held to (x slack), as in tests/test_gpu_stress.py
# worst error / bound of the run behind profiles/float64_path_check.json: (ratio, case, task, entry point, output)
#   260 outputs held to the float64 bound: 0.46 (tiny, task 0, ift_hypergrad, H: 3.50e-07 under 7.59e-07), median 0.055
#     (the workspace test's second case, not in the file: 0.60, odd_twin, task 1, H: 3.50e-07 under 5.86e-07)
#   20 outputs held to the float32 step of adkf_predict: 0.91 (wide_d, task 0, predict, pred_cov: 2.33e-05 under 2.55e-05), median 0.46
#   24 outputs of unflagged neighbours at 1e-4 x slack: 0.82 (neighbours_130, task 2, grad_phi f_out)
WORST = (0.912, "wide_d", 0, "predict", "pred_cov")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


# ---- batches and references -------------------------------------------------------------------------------------------------------------
def make_batch(c, dev, labels=True, priors=None):
    """The case as a GPBatch, its priors filled in as the library does (adkf_init_params on the batch)."""
    from adkf_ift_amd import gp_ops

    T, ld, ldq = c["Z_s"].shape[0], c["Z_s"].shape[1], c["Z_q"].shape[1]
    ragged_s, ragged_q = any(n != ld for n in c["n_s"]), any(m != ldq for m in c["n_q"])
    b = gp_ops.GPBatch(c["Z_s"].to(dev), c["y_s"].to(dev), torch.empty(T, 4, device=dev) if priors is None else priors, c["kernel"],
                       Z_q=c["Z_q"].to(dev), y_q=c["y_q"].to(dev) if labels else None,
                       n_s=torch.tensor(c["n_s"], dtype=torch.int32) if ragged_s else None,
                       n_q=torch.tensor(c["n_q"], dtype=torch.int32) if ragged_q else None)
    if priors is None:
        gp_ops.init_params_batch(b, True, True)
    return b


def refs_of(c, b):
    """The float64 reference of every task, with the batch's float32 priors read back."""
    pri = b.priors.cpu().tolist()
    return [I.reference(c["name"], t, tuple(pri[t])) for t in range(len(c["n_s"]))]


def _np(x):
    return x.detach().cpu().numpy()


def ift_outputs(out, t, n, m):
    return {"H": _np(out["H"][t]), "f_out": _np(out["f_out"][t]), "g_out": _np(out["g_phi"][t]), "v": _np(out["v"][t]),
            "dZs_total": _np(out["dZ_s"][t, :n]), "dZq_total": _np(out["dZ_q"][t, :m])}


def rec(c, t, entry, output, got, want, bound, held_to):
    return dict(case=c["name"], task=t, entry=entry, output=output, error=I.rel(got, want), bound=float(bound), held_to=held_to)


def check(records):
    for r in records:
        print("%-15s t%d %-34s %-10s %.2e / %.2e  (%s)" % (r["case"], r["task"], r["entry"], r["output"], r["error"], r["bound"], r["held_to"]))
    bad = [r for r in records if not r["error"] <= r["bound"]]
    assert not bad, [(r["case"], r["task"], r["entry"], r["output"], "%.2e > %.2e" % (r["error"], r["bound"])) for r in bad]


def assert_flags(b, c):
    from adkf_ift_amd import gp_ops
    assert gp_ops.double_path_tasks(b).cpu().tolist() == list(c["flags"]), (c["name"], "float64 path taken by other tasks than intended")


def assert_padding_zero(c, out):
    for t, (n, m) in enumerate(zip(c["n_s"], c["n_q"])):
        assert float(out["dZ_s"][t, n:].abs().sum()) == 0.0 and float(out["dZ_q"][t, m:].abs().sum()) == 0.0, (c["name"], t)


# ---- the measurements (tools/float64_path_check.py calls them too) -----------------------------------------------------------------------
def measure_ift(dev, name, c=None, b=None, entry="ift_hypergrad", direct=True, correction=True):
    """adkf_ift_hypergrad on a case: flagged tasks against the float64 bound, the others against 1e-4 x slack."""
    from adkf_ift_amd import gp_ops

    c = c or I.case(name)
    b = b or make_batch(c, dev)
    out = gp_ops.ift_hypergrad(b, c["phi"].to(dev), ignore_grad_correction=not correction, ignore_direct_grad=not direct)
    assert int(out["info"].abs().max()) == 0, (name, out["info"].tolist())
    assert_flags(b, c)
    assert_padding_zero(c, out)
    records = []
    for t, ref in enumerate(refs_of(c, b)):
        n, m = c["n_s"][t], c["n_q"][t]
        got, q = ift_outputs(out, t, n, m), dict(ref["q"])
        q["dZs_total"], q["dZq_total"], q["v"] = I.combine(ref["q"], direct, correction)
        fns = {"dZs_total": lambda r: I.combine(r, direct, correction)[0], "dZq_total": lambda r: I.combine(r, direct, correction)[1]}
        for k in I.IFT_KEYS:
            if not np.abs(q[k]).max() > 0.0:      # a part switched off: exactly zero
                assert float(np.abs(got[k]).max()) == 0.0, (name, t, entry, k)
                continue
            if c["flags"][t]:
                records.append(rec(c, t, entry, k, got[k], q[k], I.bound(ref, k, fn=fns.get(k)), "float64"))
            else:
                records.append(rec(c, t, entry, k, got[k], q[k], I.old_tolerance(ref, k), "1e-4 x slack"))
    return records, out


def measure_outer(dev, name):
    """adkf_outer_nll_value_grad (no Hessian, hence no correction): f_out, grad_phi f_out and the direct dL/dZ."""
    from adkf_ift_amd import gp_ops

    c = I.case(name)
    b = make_batch(c, dev)
    f, g, dZs, dZq, info = gp_ops.outer_nll_value_grad(b, c["phi"].to(dev))
    assert int(info.abs().max()) == 0
    assert_flags(b, c)
    assert_padding_zero(c, dict(dZ_s=dZs, dZ_q=dZq))
    records = []
    for t, ref in enumerate(refs_of(c, b)):
        n, m = c["n_s"][t], c["n_q"][t]
        q = ref["q"]
        for k, got, want, fn in (("f_out", f[t], q["f_out"], None), ("g_out", g[t], q["g_out"], None),
                                 ("dZs_total", dZs[t, :n], q["dZs_direct"], lambda r: r["dZs_direct"]),
                                 ("dZq_total", dZq[t, :m], q["dZq_direct"], lambda r: r["dZq_direct"])):
            records.append(rec(c, t, "outer_nll_value_grad", k, _np(got), want, I.bound(ref, k, fn=fn), "float64"))
    return records


def measure_mll(dev, name):
    """adkf_mll_value_grad: f_in and its gradient.  A task flagged through Sigma_q alone is NOT flagged here (level 0 of k_refine64 looks
    at the sweep of A only) and A is well conditioned: the ordinary 1e-4."""
    from adkf_ift_amd import gp_ops

    c = I.case(name)
    b = make_batch(c, dev)
    f, g, _, info = gp_ops.mll_value_grad(b, c["phi"].to(dev))
    assert int(info.abs().max()) == 0
    records = []
    for t, ref in enumerate(refs_of(c, b)):
        by_a = c["flag_by"][t] == "A"
        for k, got in (("f_in", f[t]), ("g_in", g[t])):
            records.append(rec(c, t, "mll_value_grad", k, _np(got), ref["q"][k], I.bound(ref, k) if by_a else TOL, "float64" if by_a else "1e-4"))
    return records


def measure_predict(dev, name, labels):
    """adkf_predict with and without query labels: the mean against the float64 bound, variance and covariance against twice the CPU
    emulation of the float32 step they keep (the module docstring); the ordinary 1e-4 for a task flagged through Sigma_q alone."""
    from adkf_ift_amd import gp_ops

    c = I.case(name)
    b = make_batch(c, dev)
    if not labels:
        b = make_batch(c, dev, labels=False, priors=b.priors)
    mean, var, cov, info = gp_ops.predict(b, c["phi"].to(dev), want_var=True, want_cov=True)
    assert int(info.abs().max()) == 0
    entry = "predict" if labels else "predict without y_q"
    records = []
    for t, ref in enumerate(refs_of(c, b)):
        m, by_a = c["n_q"][t], c["flag_by"][t] == "A"
        step = I.predict_float32_step(name, t)
        got = {"pred_mean": mean[t, :m], "pred_var": var[t, :m], "pred_cov": cov[t, :m, :m]}
        for k in got:
            if not by_a:
                bnd, held = TOL, "1e-4"
            elif k == "pred_mean":
                bnd, held = I.bound(ref, k), "float64"
            else:
                bnd, held = max(2.0 * step[k], I.bound(ref, k)), "2 x float32 step"
            records.append(rec(c, t, entry, k, _np(got[k]), ref["q"][k], bnd, held))
        assert float(mean[t, m:].abs().sum()) == 0.0 and float(var[t, m:].abs().sum()) == 0.0
    return records


def measure_reuse(dev, name):
    """adkf_ift_hypergrad with REUSE_DIST | REUSE_INNER after adkf_mll_value_grad at the same phi."""
    from adkf_ift_amd import gp_ops

    c = I.case(name)
    b = make_batch(c, dev)
    _, _, _, info = gp_ops.mll_value_grad(b, c["phi"].to(dev))
    assert int(info.abs().max()) == 0
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    return measure_ift(dev, name, c, b, entry="ift_hypergrad after mll (REUSE)")[0]


FLAG_COMBOS = [(True, False, "ift_hypergrad ignore_grad_correction"), (False, True, "ift_hypergrad ignore_direct_grad"),
               (False, False, "ift_hypergrad ignore both")]


def all_records(dev):
    """Every comparison of this file (tools/float64_path_check.py)."""
    out = []
    for name in I.ACCURACY_CASES:
        out += measure_ift(dev, name)[0]
    for name in I.ENTRY_CASES:
        out += measure_outer(dev, name) + measure_mll(dev, name) + measure_predict(dev, name, True) + measure_predict(dev, name, False)
        for direct, correction, entry in FLAG_COMBOS:
            out += measure_ift(dev, name, entry=entry, direct=direct, correction=correction)[0]
        out += measure_reuse(dev, name)
    return out


# ---- 1. float64 accuracy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", I.ACCURACY_CASES)
def test_flagged_tasks_meet_float64_accuracy(dev, name):
    """adkf_ift_hypergrad on every case: exactly the intended tasks take the float64 path, info is zero, padding rows of dL/dZ are exactly
    zero, and H, f_out, grad_phi f_out, v and both dL/dZ of every flagged task are within the float64 bound."""
    check(measure_ift(dev, name)[0])


# ---- 2. the other entry points on flagged tasks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", I.ENTRY_CASES)
def test_outer_nll_value_grad_without_the_hessian(dev, name):
    check(measure_outer(dev, name))


@pytest.mark.parametrize("name", I.ENTRY_CASES)
def test_mll_value_grad(dev, name):
    check(measure_mll(dev, name))


@pytest.mark.parametrize("labels", [True, False], ids=["with_y_q", "without_y_q"])
@pytest.mark.parametrize("name", I.ENTRY_CASES)
def test_predict(dev, name, labels):
    check(measure_predict(dev, name, labels))


@pytest.mark.parametrize("direct, correction, entry", FLAG_COMBOS, ids=["no_correction", "no_direct", "neither"])
@pytest.mark.parametrize("name", I.ENTRY_CASES)
def test_cotangent_flags_on_flagged_tasks(dev, name, direct, correction, entry):
    """ADKF_IGNORE_GRAD_CORRECTION / ADKF_IGNORE_DIRECT_GRAD: the reference's direct and correction parts combined the same way (a part
    switched off is exactly zero, v is zero without the correction)."""
    check(measure_ift(dev, name, entry=entry, direct=direct, correction=correction)[0])


@pytest.mark.parametrize("name", I.ENTRY_CASES)
def test_hypergradient_on_a_reused_inner_stage(dev, name):
    check(measure_reuse(dev, name))


# ---- 3. neighbours ----------------------------------------------------------------------------------------------------------------------
def _every_output(dev, c):
    from adkf_ift_amd import gp_ops

    b = make_batch(c, dev)
    phi = c["phi"].to(dev)
    f_in, g_in, _, info0 = gp_ops.mll_value_grad(b, phi)
    mean, var, _, info1 = gp_ops.predict(b, phi)
    out = gp_ops.ift_hypergrad(b, phi)
    flagged = gp_ops.double_path_tasks(b)
    return dict(out, f_in=f_in, g_in=g_in, mean=mean, var=var, info0=info0, info1=info1, flagged=flagged, priors=b.priors)


@pytest.mark.parametrize("name", I.NEIGHBOUR_CASES)
def test_the_tail_overwrites_its_own_tasks_only(dev, name):
    """A flagged task between two well-conditioned ones: each task alone (same padded sizes) and inside the batch give the same bits in
    every output; the unflagged tasks meet 1e-4 x slack, the flagged one the float64 bound."""
    c = I.case(name)
    records, _ = measure_ift(dev, name)
    check(records)
    together = _every_output(dev, c)
    assert together["flagged"].cpu().tolist() == [0, 1, 0]
    for t in range(3):
        alone = _every_output(dev, I.single_task(c, t))
        for k, v in alone.items():
            assert torch.equal(v[0], together[k][t]), (name, t, k)


# ---- 4. workspace state -----------------------------------------------------------------------------------------------------------------
def test_nothing_of_the_previous_batch_survives_in_the_workspace(dev):
    """Two different flagged cases of one shape in turn on ONE batch object and workspace, then the first again: the third result is the
    first, bit for bit (stale parked exponentials, float64 distances or arrival state would show), and the second meets its bounds."""
    from adkf_ift_amd import gp_ops

    first, second = I.case("odd"), I.case("odd_twin")
    b = make_batch(first, dev)
    ws = b.workspace()[0].data_ptr()

    def run(c):
        for k in ("Z_s", "y_s", "Z_q", "y_q"):
            getattr(b, k).copy_(c[k].to(dev))
        gp_ops.init_params_batch(b, True, True)
        records, out = measure_ift(dev, c["name"], c, b, entry="ift_hypergrad on a used workspace")
        check(records)
        return {k: v.clone() for k, v in out.items()}

    one, _, three = run(first), run(second), run(first)
    assert b.workspace()[0].data_ptr() == ws
    for k in one:
        assert torch.equal(one[k], three[k]), k
