"""CPU: the inputs of tests/test_gpu_float64_path.py (tests/r64_inputs.py) have the properties its comparisons rely on - the test of the
tests.  Every task sits a factor of two on its side of the float64 path's threshold, every flagged task has an output on which the float32
restatement of the reference misses the bound by a factor of ten (a task silently left on the float32 path would fail), every bound is at
least three times sharper than the 1e-4 x slack the rest of the suite holds the same output to, and the references are finite with a
positive definite predictive covariance.  Run with -s to read the figures.  No GPU, no library call."""
import numpy as np
import pytest
import torch

import r64_inputs as I

TASKS = [(name, t) for name in I.CASES for t in range(len(I.CASES[name]["tasks"]))]
ALL_KEYS = I.IFT_KEYS + ("f_in", "g_in", "pred_mean", "pred_var", "pred_cov")


def test_the_cases_cover_the_branches_of_the_path():
    """The shapes the float64 path branches on (csrc/refine64.h): the chunk of 32 pivots, 128 points in registers / blocked beyond, the
    128-wide K chunk of the staged products, parked exponentials up to 128 + 128 points; both kernels; ragged batches with padding."""
    shape = {name: (I.CASES[name]["ld"], I.CASES[name]["d"]) for name in I.CASES}
    assert shape["tiny"] == ((2, 1), 1)
    assert shape["odd"] == ((40, 24), 5) and I.CASES["odd"]["tasks"][0][:2] == (33, 20)
    assert shape["full"] == ((128, 128), 3)
    assert shape["wide_d"] == ((33, 20), 130)
    assert shape["leftover_a"] == ((130, 129), 5) and shape["leftover_b"] == ((129, 20), 3)
    assert shape["mixed_a"] == ((128, 130), 3) and shape["mixed_b"] == ((130, 20), 3)
    assert shape["three_blocks"] == ((257, 3), 3) and len(I.CASES["three_blocks"]["tasks"]) == 1
    assert shape["sigma_only"] == ((3, 40), 2)
    assert shape["neighbours_128"][0][0] <= 128 and shape["neighbours_130"][0][0] == 130
    for name in I.NEIGHBOUR_CASES:
        assert I.case(name)["flags"] == (0, 1, 0)
    assert {I.CASES[name]["kernel"] for name in I.CASES} == {I.RBF, I.MATERN}
    assert I.CASES["odd"]["ld"] == I.CASES["odd_twin"]["ld"] and I.CASES["odd"]["d"] == I.CASES["odd_twin"]["d"]
    assert all(1 <= len(I.CASES[name]["tasks"]) <= 3 for name in I.CASES)
    for name in I.CASES:
        c = I.case(name)
        for t, (n, m) in enumerate(zip(c["n_s"], c["n_q"])):
            assert torch.isfinite(c["Z_s"]).all() and torch.isfinite(c["Z_q"]).all() and torch.isfinite(c["phi"]).all()
            assert (c["Z_s"][t, n:] == I.JUNK_ZS).all() and (c["y_s"][t, n:] == I.JUNK_YS).all()
            assert (c["Z_q"][t, m:] == I.JUNK_ZQ).all() and (c["y_q"][t, m:] == I.JUNK_YQ).all()
            noise, os_, _ = (float(v) for v in I.O.transform_phi(c["phi"][t].double()))
            assert abs(os_ - 1.0) < 1e-6 and (0.0029 < noise < 0.0101 if c["flags"][t] else abs(noise - 0.1) < 1e-6)


@pytest.mark.parametrize("name, t", TASKS)
def test_tasks_sit_a_factor_of_two_off_the_threshold(name, t):
    """float64 LDL^T pivot ratios: at least 60 where the task is meant to be flagged (for A, or for Sigma_q ALONE in the Sigma_q-only
    case), at most 15 for both where it is not - so that the float32 sweep lands on the same side of 30."""
    by = I.case(name)["flag_by"][t]
    ra, rs = I.pivot_ratios(name, t)
    print(name, t, "flagged by", by, "pivot ratio of A %.1f, of Sigma_q %.1f" % (ra, rs))
    if by == "A":
        assert ra >= I.FLAG_MIN
    elif by == "S":
        assert rs >= I.FLAG_MIN and ra <= I.UNFLAG_MAX
    else:
        assert ra <= I.UNFLAG_MAX and rs <= I.UNFLAG_MAX


@pytest.mark.parametrize("name, t", TASKS)
def test_references_are_finite_and_bounds_are_sharp(name, t):
    ref = I.reference(name, t)
    q = ref["q"]
    for k, v in q.items():
        assert np.isfinite(v).all(), k
    assert np.linalg.eigvalsh(q["pred_cov"]).min() > 0.0
    for k in ALL_KEYS:
        b, old = I.bound(ref, k), I.old_tolerance(ref, k)
        print(name, t, k, "bound %.2e, 1e-4 x slack %.2e: %.0f x sharper" % (b, old, old / b))
        assert b >= 2.0 * I.R                 # (never below the rounding of the output itself)
        assert 3.0 * b <= old, (k, b, old)
    # the combinations of the ADKF_IGNORE_* flags have bounds of their own
    for direct, correction in ((True, False), (False, True)):
        for i, k in enumerate(("dZs_total", "dZq_total")):
            if i == 1 and not direct:
                continue
            b = I.bound(ref, k, fn=lambda r: I.combine(r, direct, correction)[i])
            assert 3.0 * b <= 1e-4, (k, direct, correction, b)


@pytest.mark.parametrize("name, t", [(n, t) for n, t in TASKS if I.case(n)["flags"][t]])
def test_a_task_left_on_float32_would_fail(name, t):
    """The reference restated in float32 (the same formulas, the same inputs) misses the bound of at least one of the outputs of
    ift_hypergrad by a factor of ten."""
    ref, e32 = I.reference(name, t), I.float32_restatement_errors(name, t)
    ratio = {k: e32[k] / I.bound(ref, k) for k in I.IFT_KEYS}
    worst = max(ratio, key=ratio.get)
    print(name, t, "float32 restatement: %s off by %.1e, %.0f x its bound" % (worst, e32[worst], ratio[worst]))
    assert ratio[worst] > 10.0, ratio


@pytest.mark.parametrize("name", I.ENTRY_CASES)
def test_the_float32_step_of_predict_is_what_keeps_its_variance_off_the_bound(name):
    """adkf_predict finishes in float32 from C rounded to float32 (r64_inputs.predict_float32_step): the emulation of exactly that step
    on the float64 reference stays far inside 1e-4, and its mean stays inside the float64 bound - only variance and covariance need
    the yardstick of their own."""
    c = I.case(name)
    for t in range(len(c["n_s"])):
        ref, step = I.reference(name, t), I.predict_float32_step(name, t)
        print(name, t, {k: "%.1e (bound %.1e)" % (v, I.bound(ref, k)) for k, v in step.items()})
        assert step["pred_mean"] <= I.bound(ref, "pred_mean")
        assert 2.0 * step["pred_var"] <= 1e-4 and 2.0 * step["pred_cov"] <= 1e-4
