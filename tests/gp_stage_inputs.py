"""Seeded inputs of the tests of the GP pipeline's first stage (k_colmean, the distance launch of csrc/host_gp.h::stage_dist, k_median and
the k_lg_med_hist / k_lg_med_pick radix select), built on the CPU, each with its exact answer.  tests/test_gpu_dist_median.py runs the
kernels on them, tests/test_gp_stage_inputs.py checks (without a GPU) that they have the properties the exact comparisons rely on and which
wrong kernel each of them would catch, and tools/dist_kernel_yardsticks.py writes profiles/dist_kernel_yardsticks.json from them.

Exact recipes of the distance stage: integer-valued features whose column mean over the support rows is an exact integer c.  Half the
rows are random integers in [-m, m], the other half their negatives, an all-zero row is added for an odd count, the rows are shuffled and
c is added per column; query rows are any integers in [-m, m] plus c.  Under
        4 m^2 k < 2^24   (k: non-zero entries of a centred row; d for the dense recipes, 1 for the sparse one)
        n (m + |c|) < 2^24
the column sums, the centred entries, the squared norms, the inner products, every partial sum of them and |x|^2 + |y|^2 - 2 x.y are
integers below 2^24: the float32 answer is the integer distance on the FP32 pipe and on the split-bfloat16 pipe alike (products of
bfloat16 pieces of such values and their partial sums are exact).
  (a) m = 15, c = 0;   (b) m = 15, |c| up to 4096 (uncentred, |x|^2 passes 2^24 from d = 32 on);
  (c) one non-zero entry per row, 11 bits wide (1024 <= |v| <= 2047, never a multiple of 8: piece 1 of the split is non-zero on every
      entry), all rows of a task in ONE column (another column for every task), so that every pair has a non-zero inner product;
  (d) like (a), task 0 with two coincident rows (and their two coincident negatives), task 1 with all rows equal.
Rows >= n of Z_s and Z_q hold JUNK (finite: the header promises only that padding is ignored on input).

Hand-made D2ss matrices of the median kernels: float32 bit patterns, positive normal finite candidates in the strict upper triangle of the
first n rows, another arbitrary pattern each in the lower triangle, on the diagonal and outside n x n.

Nothing here may be modified by a test: the cases are cached."""
import functools

import numpy as np
import torch

from dense_kernel_inputs import pieces
from test_x3_split import KEPT

TWO24 = 2 ** 24
JUNK = 3.0e4


# ---- the workspace layout (csrc/host_gp.h::carve): the one place in the tests that knows it ------------------------------------------------
def align256(nbytes):
    return (nbytes + 255) // 256 * 256


def stage_view(ws, T, ns, nq, d):
    """float32 views (mean [T, d], D2ss [T, ns, ns], D2qs [T, nq, ns], D2qq [T, nq, nq]) into a workspace (any 1-d tensor of bytes, host or
    device) and the byte offset at which D2qq - the last region of the stage - ends.  Every region starts at a multiple of 256 bytes."""
    flat = ws.view(torch.uint8).reshape(-1)
    off, end, views = 0, 0, []
    for shape in ((T, d), (T, ns, ns), (T, nq, ns), (T, nq, nq)):
        n = int(np.prod(shape))
        views.append(flat[off:off + 4 * n].view(torch.float32).view(shape))
        if n:
            end = off + 4 * n
        off += align256(4 * n)
    return views[0], views[1], views[2], views[3], end


def lg_med_bytes(T):
    """Size of the radix select's scratch (prefix[T], rank[T], hist[T, 256]): the only thing past the distances a median call may write."""
    return align256(258 * 4 * T)


# ---- exact recipes of the distance stage --------------------------------------------------------------------------------------------
def _paired(g, n, draw):
    """n rows: draw(n // 2) and its negative, a zero row for odd n, shuffled."""
    p = draw(n // 2)
    rows = torch.cat((p, -p, torch.zeros(n % 2, p.shape[1], dtype=p.dtype)))
    return rows[torch.randperm(n, generator=g)]


def _sparse_draw(g, d, col):
    def draw(k):
        v = torch.randint(1024, 2048, (k,), generator=g)
        v = torch.where(v % 8 == 0, v + 1 + torch.randint(0, 7, (k,), generator=g), v)      # 11 significant bits, piece 1 never zero
        rows = torch.zeros(k, d, dtype=torch.int64)
        rows[:, col] = v * (1 - 2 * torch.randint(0, 2, (k,), generator=g))
        return rows
    return draw


def _cvec(c, d):
    """The column means of a task: +-c, c / 2, c / 4 in turn (integers; all zero for c = 0)."""
    k = torch.arange(d)
    return (torch.full((d,), c, dtype=torch.int64) >> (k % 3)) * (1 - 2 * (k % 2))


RECIPES = {"a": (15, 0), "b": (15, 4096), "c": (2047, 0), "d": (15, 0)}


@functools.lru_cache(maxsize=None)
def exact_batch(recipe, n_s, n_q, ld_s, ld_q, d, seed=0):
    """One ragged batch of an exact recipe.  n_s, n_q: tuples of task sizes (n_q ignored when ld_q == 0); ld_s, ld_q: padded sizes.
    Returns Z_s [T, ld_s, d], Z_q [T, ld_q, d] or None, the sizes, c [T, d] (the exact column means; 0 for an empty task) and the integer
    distances D2ss, D2qs, D2qq (int64, zero outside n_x x n_y)."""
    m, c0 = RECIPES[recipe]
    T = len(n_s)
    g = torch.Generator().manual_seed(9000 + 131 * seed + 7 * ld_s + 3 * ld_q + d + ord(recipe))
    nz = 1 if recipe == "c" else d
    assert 4 * m * m * nz < TWO24 and max(max(n_s), 1) * (m + abs(c0)) < TWO24, "the recipe's own conditions"
    Zs = torch.full((T, ld_s, d), JUNK)
    Zq = torch.full((T, ld_q, d), JUNK) if ld_q else None
    c = torch.zeros(T, d, dtype=torch.int64)
    D = [torch.zeros(T, ld_s, ld_s, dtype=torch.int64), torch.zeros(T, ld_q, ld_s, dtype=torch.int64), torch.zeros(T, ld_q, ld_q, dtype=torch.int64)]
    for t in range(T):
        n, nq = n_s[t], (n_q[t] if ld_q else 0)
        col = (0, d - 1, d // 2)[t % 3]
        dense = lambda k: torch.randint(-m, m + 1, (k, d), generator=g)
        draw = _sparse_draw(g, d, col) if recipe == "c" else dense
        xs = _paired(g, n, draw) if n else torch.zeros(0, d, dtype=torch.int64)
        if recipe == "d" and t == 0 and n >= 4:          # two coincident rows, and their two coincident negatives
            p = dense(n // 2)
            p[1] = p[0]
            xs = torch.cat((p, -p, torch.zeros(n % 2, d, dtype=torch.int64)))[torch.randperm(n, generator=g)]
        if recipe == "d" and t == 1 and n:               # all rows equal: the mean is that row
            xs = dense(1).expand(n, d).clone()
        ct = _cvec(c0, d) if n else torch.zeros(d, dtype=torch.int64)      # (an empty task has mean 0: its queries stay uncentred)
        xq = draw(nq) if nq else torch.zeros(0, d, dtype=torch.int64)
        c[t] = ct + (xs[0] if recipe == "d" and t == 1 and n else 0)
        Zs[t, :n] = (xs + ct).float()
        if ld_q:
            Zq[t, :nq] = (xq + ct).float()
        xs_c, xq_c = xs + ct - c[t], xq + ct - c[t]                     # what the kernel sees after the centring
        if n:
            assert (xs_c.sum(0) == 0).all(), "the column mean is exactly c"
        for blk, (X, Y) in enumerate(((xs_c, xs_c), (xq_c, xs_c), (xq_c, xq_c))):
            if X.shape[0] and Y.shape[0]:
                nx, ny, xy = (X * X).sum(1), (Y * Y).sum(1), X @ Y.t()
                # every partial sum the kernel may form, in any order, is an integer below 2^24
                assert int(nx.max()) + int(ny.max()) + 2 * int((X.abs() @ Y.abs().t()).max()) < TWO24
                D[blk][t, :X.shape[0], :Y.shape[0]] = nx[:, None] + ny[None, :] - 2 * xy
    assert Zs.abs().max() < TWO24 and torch.equal(Zs, Zs.round())
    return dict(Z_s=Zs, Z_q=Zq, n_s=tuple(n_s), n_q=tuple(n_q) if ld_q else None, c=c, D2ss=D[0], D2qs=D[1], D2qq=D[2], m=m, c0=c0)


def ragged_sizes(ld):
    """T = 3: n = ld, ld - 1 and max(ld - 64, 2) (0 where ld is 0)."""
    return (ld, max(ld - 1, 0), max(ld - 64, 2) if ld else 0)


# (ns_max, nq_max) of the distance tests.  (65, 130): 4, 6 and 9 tiles in the three blocks, both boundaries of ProbDistMulti::select inside
# one task's tile range; (128, 132): 16-byte loads and stores, a two-tile mirror; (130, 61): a leading dimension that is no multiple of 4
DIST_SHAPES = [(5, 3), (64, 64), (65, 130), (128, 132), (130, 61), (192, 0), (260, 68)]
# d: 1, 3, 31 on the FP32 pipe with scalar loads; 32 one K chunk of the split-bfloat16 pipe; 33 a ragged second chunk, scalar loads; 36, 64, 100
DIST_D = [1, 3, 31, 32, 33, 36, 64, 100]


def dist_cases():
    """(ns_max, nq_max, d): every shape with d = 32 and d = 31, every d with (65, 130) and (128, 132)."""
    out = [(ns, nq, d) for ns, nq in DIST_SHAPES for d in (32, 31)]
    out += [(ns, nq, d) for d in DIST_D if d not in (31, 32) for ns, nq in ((65, 130), (128, 132))]
    return out


def gemm_form_f32(Z, mean, n, Y=None, ny=None, center=True):
    """numpy float32 evaluation of |x|^2 + |y|^2 - 2 x.y on the (centred) rows: what the stage computes, in plain float32."""
    X = Z[:n].numpy().astype(np.float32)
    Yv = X if Y is None else Y[:ny].numpy().astype(np.float32)
    mu = mean.numpy().astype(np.float32) if center else np.float32(0)
    X, Yv = X - mu, Yv - mu
    nx, nyv = (X * X).sum(1, dtype=np.float32), (Yv * Yv).sum(1, dtype=np.float32)
    return (nx[:, None] + nyv[None, :]) - np.float32(2) * (X @ Yv.T)


def gemm_form_split(X, Y, drop=()):
    """The same with the inner product from the kept terms of the three-piece split (float64 sum of the exact piece products, the
    terms in ``drop`` left out), the norms and the last three operations in float32.  X, Y: centred float32 tensors."""
    pa, pb = pieces(X), pieces(Y)
    acc = sum(pa[i].astype(np.float64) @ pb[j].astype(np.float64).T for i, j in KEPT if (i, j) not in drop)
    x, y = X.numpy(), Y.numpy()
    nx, ny = (x.astype(np.float64) ** 2).sum(1).astype(np.float32), (y.astype(np.float64) ** 2).sum(1).astype(np.float32)
    return (nx[:, None] + ny[None, :]) - np.float32(2) * acc.astype(np.float32)


# ---- random features: the yardstick of the distance stage ----------------------------------------------------------------------------------
RANDOM_D = (32, 96)
RANDOM_NS, RANDOM_NQ = 130, 68


@functools.lru_cache(maxsize=None)
def random_case(d):
    g = torch.Generator().manual_seed(9500 + d)
    return dict(Z_s=torch.randn(RANDOM_NS, d, generator=g), Z_q=torch.randn(RANDOM_NQ, d, generator=g))


def dist_unit_errors(blocks, Zs, Zq, mean):
    """{block: max |D - D64| / (|x|^2 + |y|^2 + 2 sum |x||y|)} of three float32 blocks (ss, qs, qq) against float64, the scale taken on the
    rows centred with ``mean`` (float32; the differences are formed in float64, where they are exact)."""
    xs, xq = Zs.double() - mean.double(), Zq.double() - mean.double()
    out = {}
    for name, got, X, Y in (("ss", blocks[0], xs, xs), ("qs", blocks[1], xq, xs), ("qq", blocks[2], xq, xq)):
        ref = (X[:, None, :] - Y[None, :, :]).pow(2).sum(-1)
        scale = X.pow(2).sum(1)[:, None] + Y.pow(2).sum(1)[None, :] + 2 * X.abs() @ Y.abs().t()
        out[name] = float(((torch.as_tensor(got).double() - ref).abs() / scale).max())
    return out


def f32_sequential_blocks(Zs, Zq):
    """The stage in float32 on the CPU, every sum sequential and every product rounded by itself: the column mean over the support rows, the
    centring, the squared norms, the inner products, |x|^2 + |y|^2 - 2 x.y.  Returns (mean, [D2ss, D2qs, D2qq])."""
    s = torch.zeros(Zs.shape[1])
    for i in range(Zs.shape[0]):
        s += Zs[i]
    mean = s / Zs.shape[0]
    xs, xq = Zs - mean, Zq - mean

    def seq(a, b):      # sum_k a[:, k] b[:, k]^T in k order
        acc, tmp = torch.zeros(a.shape[0], b.shape[0]), torch.empty(a.shape[0], b.shape[0])
        bt = b.t().contiguous()
        for k in range(a.shape[1]):
            torch.mul(a[:, k:k + 1], bt[k:k + 1], out=tmp)
            acc += tmp
        return acc

    def norms(a):
        acc = torch.zeros(a.shape[0])
        for k in range(a.shape[1]):
            acc += a[:, k] * a[:, k]
        return acc

    ns_, nq_ = norms(xs), norms(xq)
    blocks = [(nx[:, None] + ny[None, :]) - 2 * seq(X, Y) for X, Y, nx, ny in ((xs, xs, ns_, ns_), (xq, xs, nq_, ns_), (xq, xq, nq_, nq_))]
    return mean, blocks


@functools.lru_cache(maxsize=None)
def dist_yardstick(d):
    """{block: unit error of the float32 sequential evaluation} on random_case(d).  The GPU test's bound is twice it."""
    c = random_case(d)
    mean, blocks = f32_sequential_blocks(c["Z_s"], c["Z_q"])
    return dist_unit_errors(blocks, c["Z_s"], c["Z_q"], mean)


def split_emulation_errors(d):
    """{dropped terms: {block: unit error}} of the emulated split-bfloat16 stage on random_case(d): all six terms (key ()), and the
    five- and four-term variants that drop x0 y2, x2 y0 or both."""
    c = random_case(d)
    mean = c["Z_s"].double().mean(0).float()
    xs, xq = c["Z_s"] - mean, c["Z_q"] - mean
    out = {}
    for drop in ((), ((0, 2),), ((2, 0),), ((0, 2), (2, 0))):
        blocks = [gemm_form_split(X, Y, drop) for X, Y in ((xs, xs), (xq, xs), (xq, xq))]
        out[drop] = dist_unit_errors(blocks, c["Z_s"], c["Z_q"], mean)
    return out


# ---- hand-made D2ss matrices of the median kernels -------------------------------------------------------------------------------------------
BASE = 0x41800000          # 16.0: candidates in [16, 32) give l0 in [2.83, 4), where inv_softplus and log are well conditioned
MEDIAN_KINDS = ("distinct_even", "distinct_odd", "ties_inside", "ties_first", "ties_last", "zeros", "low7", "mid8", "hi8", "exponent", "all_zero")
# which wrong selections a kind is built to expose (where the count of candidates allows it at all: see catches())
_CATCHES = {"distinct_even": ("upper", "rank+1", "rank-1", "middle_twice"), "distinct_odd": ("rank+1", "rank-1", "middle_twice"),
            "ties_inside": (), "ties_first": ("rank-1",), "ties_last": ("upper", "rank+1"), "zeros": ("zeros_counted", "rank+1", "rank-1"),
            "all_zero": (), "low7": ("rank+1",), "mid8": ("rank-1",), "hi8": ("rank+1",), "exponent": ("rank-1",)}


def _value_set(kind):
    """The sorted distinct bit patterns a tied kind draws from."""
    if kind.startswith("ties"):
        return [BASE + 0x1000, BASE + 0x2000, BASE + 0x3000]
    if kind == "low7":          # agree in bits 30-7: 26 values five ulps apart (one ulp apart, sqrt(0.5 v) would merge neighbours)
        return [BASE + 0x2A80 + 5 * k for k in range(26)]
    if kind == "mid8":          # differ only in bits 14-7
        return [BASE + 0x2A0055 + (k << 7) for k in range(256)]
    if kind == "hi8":           # differ only in bits 22-15
        return [BASE + 0x2A55 + (k << 15) for k in range(256)]
    if kind == "exponent":      # differ only in bits 30-23: every normal exponent but the lowest
        return [(e << 23) | 0x2A5555 for e in range(2, 255)]
    raise ValueError(kind)


def _tied(vals, N, edge, g):
    """N sorted candidates from ``vals`` whose lower median (rank r = (N - 1) // 2) sits at the LAST element of a run of equal values
    (rank r + 1 holds the next value), at the FIRST (rank r - 1 holds the previous value) or INSIDE a run."""
    r, nv = (N - 1) // 2, len(vals)
    s = nv // 2 if nv > 3 else 1
    lo_hi = {"last": (s + 1, s + 1), "first": (s, s), "inside": (s + 1, s)}[edge]
    pick = lambda pool, k: [pool[i] for i in torch.randint(0, len(pool), (k,), generator=g).tolist()]
    out = sorted(pick(vals[:lo_hi[0]], r)) + [vals[s]] + sorted(pick(vals[lo_hi[1]:], N - 1 - r))
    if edge == "last" and r + 1 < N:
        out[r + 1] = vals[s + 1]
    if edge == "first" and r >= 1:
        out[r - 1] = vals[s - 1]
    if edge == "inside":
        if r >= 1:
            out[r - 1] = vals[s]
        if r + 1 < N:
            out[r + 1] = vals[s]
    return out


@functools.lru_cache(maxsize=None)
def median_matrix(kind, n, ld, seed=0):
    """float32 [ld, ld]: the candidates of ``kind`` in the strict upper triangle of the first n rows, in random order."""
    g = torch.Generator().manual_seed(9700 + 17 * seed + 1000 * MEDIAN_KINDS.index(kind) + 3 * n + ld)
    N = n * (n - 1) // 2
    if kind in ("distinct_even", "distinct_odd", "zeros"):
        cand = [BASE + 16 * (k + 1) for k in range(N)]                  # 16 ulps apart, all in [16, 32)
        assert 16 * (N + 1) < 1 << 23
        n_zero = N * 3 // 10 if kind == "zeros" else 0
        if kind != "zeros" and N >= 2 and (N % 2 == 0) != (kind == "distinct_even"):
            n_zero = 1                                                  # one non-candidate makes the count of positives even / odd
        for i in torch.randperm(N, generator=g)[:n_zero].tolist():
            cand[i] = 0
    elif kind == "all_zero":            # no positive candidate: l0 is exactly 0
        cand = [0] * N
    else:
        edge = {"ties_inside": "inside", "ties_first": "first", "ties_last": "last", "low7": "last", "mid8": "first", "hi8": "last",
                "exponent": "first"}[kind]
        cand = _tied(_value_set(kind), N, edge, g) if N else []
    cand = torch.tensor(cand, dtype=torch.int64)[torch.randperm(N, generator=g)] if N else torch.zeros(0, dtype=torch.int64)
    iu = torch.triu_indices(n, n, 1)
    if kind.startswith("distinct") and n % 2 == 1 and n >= 5:
        # the middle row (which k_median folds onto itself) holds the smallest candidates: counted twice, they pull the median down
        mid = iu[0] == (n - 1) // 2
        k = int(mid.sum())
        order = torch.argsort(torch.where(cand > 0, cand, torch.full_like(cand, 1 << 40)), stable=True)
        small = torch.zeros(N, dtype=torch.bool)
        small[order[:k]] = True
        smallest, rest = cand[small], cand[~small]
        cand = torch.empty_like(cand)
        cand[mid], cand[~mid] = smallest, rest
    # everything the kernels must NOT read: lower triangle positive values below every candidate of the binade kinds (they would pull the
    # median down), diagonal above them all, outside n x n negative, huge and tiny values
    M = torch.empty(ld, ld, dtype=torch.int64)
    M[:] = torch.tensor([0xC1A00000, 0x7F000000, 0x00800001, 0xFF7FFFFF])[torch.randint(0, 4, (ld, ld), generator=g)]
    lower = 0x3F800000 + torch.randint(0, 1 << 22, (n, n), generator=g)
    diag = 0x43000000 + torch.randint(0, 1 << 22, (n,), generator=g)
    blk = lower.clone()
    blk[torch.arange(n), torch.arange(n)] = diag
    blk[iu[0], iu[1]] = cand
    M[:n, :n] = blk
    out = (M & 0xFFFFFFFF).numpy().astype(np.uint32)
    return torch.from_numpy(out.view(np.float32).copy())


def candidates(D2, n):
    """Sorted positive entries of the strict upper triangle of the first n rows, as int32 bit patterns (numpy)."""
    b = D2.contiguous().view(torch.int32)[:n, :n].numpy()
    c = b[np.triu_indices(n, 1)]
    return np.sort(c[c > 0])


def _l0_of(bits):
    return np.sqrt(np.float32(0.5) * np.int32(bits).view(np.float32))       # float32 sqrt: correctly rounded, once


def exact_l0(D2, n):
    """The reference: the positive entries of the strict upper triangle sorted by their int32 bit pattern, index (count - 1) // 2,
    sqrt(0.5 v) rounded once to float32; 0 without a positive entry."""
    c = candidates(D2, n) if n >= 2 else np.zeros(0, np.int32)
    return _l0_of(c[(len(c) - 1) // 2]) if len(c) else np.float32(0)


def wrong_l0(D2, n):
    """What plausible wrong selections would return: the upper median, a rank off by one either way, zeros counted as candidates, the
    middle row of an odd n counted twice (k_median folds rows i and n - 1 - i; the middle row is folded onto itself)."""
    c = candidates(D2, n)
    if not len(c):
        return {}
    r = (len(c) - 1) // 2
    b = D2.contiguous().view(torch.int32)[:n, :n].numpy()
    allc = np.sort(b[np.triu_indices(n, 1)])
    out = {"upper": c[len(c) // 2], "rank+1": c[min(r + 1, len(c) - 1)], "rank-1": c[max(r - 1, 0)], "zeros_counted": allc[(len(allc) - 1) // 2]}
    mid = b[(n - 1) // 2, (n - 1) // 2 + 1:n] if n % 2 else np.zeros(0, np.int32)
    tw = np.sort(np.concatenate((c, mid[mid > 0])))
    out["middle_twice"] = tw[(len(tw) - 1) // 2]
    return {k: _l0_of(v) if v > 0 else np.float32(0) for k, v in out.items()}


def catches(kind, D2, n):
    """The wrong selections this matrix is built to expose AND can, given its count of candidates: a sole candidate has no neighbour,
    an odd count no upper median, an even n no middle row."""
    c = candidates(D2, n)
    N, r = len(c), (len(c) - 1) // 2
    b = D2.contiguous().view(torch.int32)[:n, :n].numpy()
    ok = {"upper": N % 2 == 0 and N >= 2, "rank+1": r + 1 < N, "rank-1": r >= 1, "zeros_counted": bool((b[np.triu_indices(n, 1)] == 0).any()),
          "middle_twice": n % 2 == 1 and n >= 5}
    return [w for w in _CATCHES[kind] if ok[w]]


def check_spacing(D2, n):
    """Neighbouring DISTINCT order statistics stay distinct under sqrt(0.5 v) in float32."""
    u = np.unique(candidates(D2, n))
    l = _l0_of(u)
    return bool(np.all(np.diff(l) > 0)) and bool(np.all(np.isfinite(l))) and bool(np.all(u >= 0x00800000))


# batches of the median tests: (ns_max, [(n, kind), ...]) - several n and several kinds side by side, so that a task's result cannot
# come from its neighbour's histogram or prefix; single-point and empty tasks (l0 = 0) among them
def _mix(ns, start=0):
    return [(n, MEDIAN_KINDS[(start + i) % len(MEDIAN_KINDS)]) for i, n in enumerate(ns)]


MEDIAN_BATCHES = {
    "k_median<512,16> ld=128": (128, _mix([2, 3, 4, 5, 127, 128] * 5 + [1, 0, 128])),
    "k_median<512,16> ld=7": (7, _mix([7] * 10)),
    "k_median<1024,32> ld=129": (129, _mix([2, 128, 129] * 10 + [1, 129], 1)),
    "k_median<1024,32> ld=256": (256, _mix([255, 256] * 5) + _mix([256, 255] * 5)),
    "radix select ld=257": (257, _mix([2, 3, 256, 257] * 5) + _mix([257, 256] * 5 + [1, 0, 257], 3)),
    "radix select ld=300": (300, _mix([299] * 10)),
    "radix select ld=257 T=70": (257, _mix([2, 3, 4, 5, 9, 12, 17] * 10)),
}
