"""GPU: the selection of the pool calls when fewer than k candidates are offered (a pool, or a last tile, shorter than k).  The
shared list merge (predict_stream.h: pm_list_merge) once read its k-th entry with a shuffle behind `valid && ...`: the invalid lanes
were switched off, lane k - 1 among them, the read returned 0, and the threshold became (score 0, row 0) - only rows with a
POSITIVE score were taken from such a tile.  Every eligible row is ranked, whatever the sign of its score, and the tail is -1 / -inf."""
import numpy as np
import pytest
import torch

import kg_ref as R
import test_gpu_believer_pool as BV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def _check(out, score, k, tag):
    """top_idx / top_val are the sort of score under the unique order, then the -1 / -inf tail."""
    for t in range(score.shape[0]):
        wi, wv = R.topk_of(score[t], k)
        assert np.array_equal(out["top_idx"][t].cpu().numpy(), wi), (tag, t, out["top_idx"][t].tolist(), wi.tolist())
        assert np.array_equal(out["top_val"][t].cpu().numpy().view(np.int32), wv.view(np.int32)), (tag, t)


@pytest.mark.parametrize("rows,k", [(3, 4), (1, 2), (5, 64), (67, 8)])
def test_short_lists_keep_rows_of_every_sign(dev, rows, k):
    """predict_pool ranked by the mean in both senses (one of them has negative scores on most rows), by log EI far below the
    incumbent (every score negative) and mes_pool (positive scores: the case that always worked).  rows = 67: the last tile offers 3
    candidates to a list that is already full - the same defect: lane k - 1 = 7 is not one of the 3 valid lanes, so a last-tile row
    with a score <= 0 was dropped although it beat the list's k-th entry (a second test inside the insertion loop, where every lane
    is on, kept rows from being taken wrongly)."""
    from adkf_ift_amd import gp_ops

    b, phi, Zs, ys, n_s, X, _ = BV._explicit(dev, "matern", [48, 45, 31], 16, 300, 548)
    Xs = X[:rows].contiguous()
    negative = 0
    for maximize in (False, True):
        out = gp_ops.predict_pool(b, phi, Xs, score="mean", maximize=maximize, topk=k, want_var=False)
        gp_ops.check_info(out["info"])
        m = out["mean"].cpu().numpy()
        score = m if maximize else -m
        negative += int((score < 0).sum())
        _check(out, score, k, ("mean", maximize))
        assert bool((out["top_idx"][:, :min(rows, k)] >= 0).all())
    assert negative >= b.T * rows   # (a row is negative in one of the two senses)
    best = torch.full((b.T,), -50.0, device=dev)
    out = gp_ops.predict_pool(b, phi, Xs, best_f=best, log_ei=True, topk=k, want_var=False)
    score = out["ei"].cpu().numpy()
    assert (score < 0).all() and np.isfinite(score).all()
    _check(out, score, k, "log ei")
    assert bool((out["top_idx"][:, :min(rows, k)] >= 0).all())
    out = gp_ops.mes_pool(b, phi, Xs, ystar=torch.full((b.T, 2), -3.0, device=dev), topk=k, want_score=True)
    _check(out, out["score"].cpu().numpy(), k, "mes")
