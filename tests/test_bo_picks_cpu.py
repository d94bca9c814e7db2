"""bayes_opt._take_picks, the end of an iteration of every batched BO loop but the Thompson one: hand-written cases, and the EI loop's
former inline branches - kept here verbatim - on equal seeds.  No GPU, no library."""
import numpy as np
import torch

from adkf_ift_amd.bayes_opt import _take_picks


def _state(seeds, queried):
    return [np.random.default_rng(s) for s in seeds], [list(q) for q in queried], [[min(q)] for q in queried]


def test_a_full_prefix_is_taken_as_it_is_and_draws_nothing():
    rngs, queried, records = _state([0, 1], [[3, 9], [4]])
    top_idx = torch.tensor([[7, 2, 5], [0, 8, 1]])
    _take_picks(top_idx, torch.ones(2, 3, dtype=torch.bool), 3, rngs, queried, records, 12)
    assert records == [[3, 7, 2, 5], [4, 0, 8, 1]]
    assert [sorted(q) for q in queried] == [[2, 3, 5, 7, 9], [0, 1, 4, 8]]
    for s, rng in enumerate(rngs):   # no draw was made
        assert rng.integers(0, 2 ** 62) == np.random.default_rng(s).integers(0, 2 ** 62)


def test_a_partial_prefix_is_filled_from_the_rows_not_yet_taken():
    rngs, queried, records = _state([5], [[0, 1, 2]])
    top_idx = torch.tensor([[6, 4, -1, -1]])
    usable = torch.tensor([[True, True, False, False]])
    _take_picks(top_idx, usable, 4, rngs, queried, records, 9)
    fill = np.random.default_rng(5).choice([3, 5, 7, 8], size=2, replace=False).tolist()   # ascending free rows, one draw of two
    assert records == [[0, 6, 4] + fill]
    assert sorted(queried[0]) == sorted([0, 1, 2, 6, 4] + fill)
    assert len(set(records[0][1:])) == 4 and not set(fill) & {0, 1, 2, 4, 6}


def test_an_empty_prefix_is_one_draw_of_the_whole_batch():
    rngs, queried, records = _state([11], [[2, 5]])
    top_idx = torch.full((1, 3), -1)
    _take_picks(top_idx, torch.zeros(1, 3, dtype=torch.bool), 3, rngs, queried, records, 8)
    fill = np.random.default_rng(11).choice([0, 1, 3, 4, 6, 7], size=3, replace=False).tolist()
    assert records == [[2] + fill]
    assert sorted(queried[0]) == sorted([2, 5] + fill)


def test_reverse_turns_the_record_not_the_picks():
    top_idx = torch.tensor([[6, 4, -1]])
    usable = torch.tensor([[True, True, False]])
    rngs, queried, records = _state([2], [[0, 1]])
    _take_picks(top_idx, usable, 3, rngs, queried, records, 9)
    rngs_r, queried_r, records_r = _state([2], [[0, 1]])
    _take_picks(top_idx, usable, 3, rngs_r, queried_r, records_r, 9, reverse=True)
    assert records_r[0] == [0] + records[0][1:][::-1]
    assert queried_r == queried
    assert records[0][1:3] == [6, 4] and records_r[0][2:] == [4, 6]


def _ei_inline(top_idx, usable, query_batch_size, rngs, queried, records, n):
    """run_gp_ei_bo_batched's pick branches as they stood before _take_picks had ``reverse`` (a verbatim copy)."""

    def free(taken):
        taken = set(taken)
        return [i for i in range(n) if i not in taken]

    for r, rng in enumerate(rngs):
        nonzero = int(usable[r].sum())   # of the query_batch_size best: all that the branches below distinguish
        if nonzero == 0:
            pick = rng.choice(free(queried[r]), size=query_batch_size, replace=False).tolist()
        elif nonzero < query_batch_size:
            pick = top_idx[r, :nonzero].tolist()
            pick += rng.choice(free(queried[r] + pick), size=query_batch_size - nonzero, replace=False).tolist()
        else:
            pick = top_idx[r].tolist()
        queried[r] = list(set(queried[r] + pick))
        records[r].extend(pick[::-1])


def test_reverse_is_the_ei_loops_former_inline_branches():
    n, q, R = 40, 4, 6
    g = torch.Generator().manual_seed(0)
    init = [np.random.default_rng(100 + r).choice(n, size=5, replace=False).tolist() for r in range(R)]
    a = _state(range(R), init)
    b = _state(range(R), init)
    for it in range(4):   # replicate r has r usable candidates (capped): empty, partial and full prefixes, iteration after iteration
        top_idx = torch.full((R, q), -1, dtype=torch.int64)
        usable = torch.zeros(R, q, dtype=torch.bool)
        for r in range(R):
            taken = set(a[1][r])
            cand = [i for i in torch.randperm(n, generator=g).tolist() if i not in taken]
            k = min(q, (r + it) % (q + 2))
            top_idx[r, :k] = torch.tensor(cand[:k], dtype=torch.int64)
            usable[r, :k] = True
        _take_picks(top_idx, usable, q, a[0], a[1], a[2], n, reverse=True)
        _ei_inline(top_idx, usable, q, b[0], b[1], b[2], n)
        assert a[1] == b[1] and a[2] == b[2], it
    for ra, rb in zip(a[0], b[0]):   # the generators stand at the same place
        assert ra.integers(0, 2 ** 62) == rb.integers(0, 2 ** 62)
    for r in range(R):
        assert len(a[2][r]) == 1 + 4 * q and len(set(a[1][r])) == 5 + 4 * q
