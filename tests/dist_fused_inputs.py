"""Feature sets of full 128 + 128 batches for the median select that runs INSIDE the distance launch (csrc/dist_task.h, SELECT instance;
csrc/median_select.h).  That select cannot be fed a matrix, only features, so the histogram's hard cases are made out of rows whose
squared distances the float32 pipeline reproduces exactly.  tests/test_gpu_dist_fused.py runs the kernels on them,
tests/test_dist_fused_inputs.py checks without a GPU that they are what they claim.

All constructions put one non-zero entry in a row ("axis rows"): row k is s_k e_k, row 64 + k is -s_k e_k (k < 64, so d >= 64), the column
mean is exactly 0, two rows on different axes are s_j^2 + s_k^2 apart and the two rows of one axis 4 s_k^2.
  (a) s_k = s for every k: 8 064 candidates equal 2 s^2 and 64 equal 4 s^2, the rank lies inside a run of thousands of ties.  The tasks of
      a batch alternate s = 1 and s = 3: the medians 2.0 (0x40000000) and 18.0 (0x41900000) differ in exponent bits and in a mantissa bit.
  (b) s_k = 2^(k mod 13): the candidates span 2 .. 2^26, min and max share no leading bit and the common-prefix step returns nothing.
      4^a + 4^b is not always a float32 (2^24 + 1 is not): such a distance is the ONE rounding of |x|^2 + |y|^2, the inner product of two
      rows on different axes being exactly 0, and float32(exact) is what every evaluation order gives.
  (c) coincident rows.  One row differs from 127 equal ones: the only positive candidates are the 127 pairs with that row, all of ONE value
      (128 points cannot have fewer positive pairs than 127).  The odd tasks of the batch have all rows equal: no positive candidate, l0 = 0.
  (d) (a) with row 1 made equal to row 0: 8 127 positive candidates (odd) where (a) has 8 128 (even); the column mean is +-s / 128 in two
      columns and every centred entry, norm and product a small multiple of s^2 / 2^14.
The rows of every task but the first are permuted and the axes shifted by a task-dependent offset, so no two tasks agree and the values
sit in different lanes.  Query rows are small multiples of the support row on their axis ((c): small integers around the common row).

Nothing here may be modified by a test: the cases are cached."""
import functools

import numpy as np
import torch

N = 128
CASES = ("a", "b", "c", "d")


def min_d(case):
    return 1 if case == "c" else 64


def _axis_task(scales, t, d, g):
    """Z_s, Z_q (int64) of one task of axis rows: scales[k] on axis off + k."""
    off = (5 * t) % (d - 63)
    Zs, Zq = torch.zeros(N, d, dtype=torch.int64), torch.zeros(N, d, dtype=torch.int64)
    for k in range(64):
        Zs[k, off + k], Zs[64 + k, off + k] = scales[k], -scales[k]
    for i in range(N):
        k = (5 * i + 3) % 64
        Zq[i, off + k] = (1, -2, 3, -1)[i % 4] * scales[k]
    return Zs, Zq


@functools.lru_cache(maxsize=None)
def fused_batch(case, T, d):
    """-> dict(Z_s, Z_q [T, 128, d] float32; mean [T, d], D2ss, D2qs, D2qq [T, 128, 128] float32: the exact values rounded ONCE;
    exact: the same three blocks in float64 (exact); n_pos [T]: the count of positive candidates)"""
    assert case in CASES and d >= min_d(case)
    g = torch.Generator().manual_seed(9800 + 97 * CASES.index(case) + 7 * T + d)
    Zs, Zq = torch.zeros(T, N, d, dtype=torch.int64), torch.zeros(T, N, d, dtype=torch.int64)
    for t in range(T):
        if case == "c":
            r = torch.randint(-9, 10, (d,), generator=g)
            Zs[t] = r
            if t % 2 == 0:
                Zs[t, (17 * t + 127) % N, t % d] += 128 * (1 + t)        # the mean moves by the integer 1 + t in that column
            Zq[t] = r + torch.randint(-3, 4, (N, d), generator=g)
            continue
        s = (1, 3)[t % 2]
        scales = [1 << (k % 13) for k in range(64)] if case == "b" else [s] * 64
        zs, zq = _axis_task(scales, t, d, g)
        if case == "d":
            zs[1] = zs[0]
        perm = torch.randperm(N, generator=g) if t else torch.arange(N)
        Zs[t], Zq[t] = zs[perm], zq
    mean = Zs.double().sum(1) / N                     # float64: exact (integers / 128)
    xs, xq = Zs.double() - mean[:, None, :], Zq.double() - mean[:, None, :]
    blocks = []
    for X, Y in ((xs, xs), (xq, xs), (xq, xq)):
        nx, ny = (X * X).sum(2), (Y * Y).sum(2)
        blocks.append(nx[:, :, None] + ny[:, None, :] - 2 * X @ Y.transpose(1, 2))   # exact in float64: multiples of 2^-14 below 2^30
    iu = np.triu_indices(N, 1)
    n_pos = [int((blocks[0][t].numpy()[iu] > 0).sum()) for t in range(T)]
    return dict(Z_s=Zs.float(), Z_q=Zq.float(), mean=mean.float(), D2ss=blocks[0].float(), D2qs=blocks[1].float(), D2qq=blocks[2].float(),
                exact=blocks, mean64=mean, n_pos=n_pos)
