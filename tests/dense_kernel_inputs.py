"""Seeded float32 inputs of the dense-kernel tests (csrc/dense_x3.h), built on the CPU, each with its exact answer.
tests/test_gpu_dense_kernels.py runs the kernels on them, tests/test_dense_kernel_inputs.py checks (without a GPU) that they have the
properties the exact comparisons rely on and that a kernel with one product term missing could not pass them, and
tools/dense_kernel_yardsticks.py writes profiles/dense_kernel_yardsticks.json from them.

The exact recipes choose data on which the correct answer - and every partial sum of products of PIECES, in any order - is a float32,
so the comparison is ``torch.equal`` and no tolerance exists:
  * dense integers: |x| < 2^bx, |w| < 2^bw, bias in +-64, with n (2^bx - 1)(2^bw - 1) + 128 <= 2^24 for the contraction length n
    (the looser n 2^(bx + bw) + 128 overshoots 2^24 by exactly the 128 for every pair of the table; what has to stay below 2^24 is the
    sum of the magnitudes, and of the magnitudes of the pieces, which the CPU test evaluates on the data).  Three quarters of the
    entries have their top bit set, so that an operand of more than 8 bits has a non-zero piece 1 on more than a quarter of them;
  * sparse wide: one operand holds odd integers of 22 significant bits (three non-zero pieces), the other 0, +-1, +-2 with at most two
    non-zeros along the contraction (one +-1 or +-2, one +-1: the sum stays below 3 2^22 + 64 < 2^24), at cyclic positions;
  * one-hot, wide exponents: row m of x has one non-zero, an odd 12-bit significand times 2^e, e in [-60, 40]; w is dense, a 12-bit
    significand times 2^f, f in [-40, 40]: every output is one 24-bit product plus exact zeros.  With a bias the answer is that
    product plus the bias rounded ONCE, which the float32 addition of the two exact floats gives.
Nothing here may be modified by a test: the cases are cached."""
import functools

import numpy as np
import torch

from test_x3_split import KEPT, _bf16_rn, _split3   # the numpy cut and the six kept terms: stated once, there

TWO24 = float(2 ** 24)

# ---- shapes and layouts the GPU file runs ------------------------------------------------------------------------------
# (M, N, K) -> (ldx - K, ldy - N, bytes by which y starts past a 16-byte boundary)
FWD_SHAPES = {(1, 1, 32): (0, 3, 0), (127, 15, 32): (4, 0, 4), (128, 16, 64): (0, 0, 0), (129, 17, 96): (4, 3, 0),
              (200, 130, 160): (0, 3, 4), (257, 129, 256): (4, 0, 0), (130, 260, 512): (4, 3, 4)}
FWD_BITS = {32: (10, 9), 64: (9, 9), 96: (9, 8), 128: (9, 8), 160: (9, 7), 256: (9, 7), 512: (9, 6)}
# (M, N, K) -> (ldg - N, ldx - K)
WGRAD_SHAPES = {(1, 1, 1): (0, 0), (31, 5, 7): (1, 3), (33, 129, 130): (0, 0), (129, 16, 257): (1, 3), (1000, 200, 136): (0, 0),
                (4099, 33, 70): (1, 3), (8193, 8, 8): (1, 3)}
NONFINITE_SHAPE = (200, 130, 96)
ROUNDING_K = (32, 256)          # check 6: M = N = 256 through k_dense3; K = 256 also through k_dense3_sk
SAME_SIGN = (512, 512, 256)     # check 7: outputs 512 x 512, contraction 256


def wgrad_bits(M):
    for top, bits in ((33, (10, 8)), (256, (9, 7)), (1024, (8, 6)), (8193, (6, 5))):
        if M <= top:
            return bits
    raise ValueError(M)


def sk_cases(cus):
    """The six k_dense3_sk cases for a device of ``cus`` compute units: one, two and three row tiles for the busiest workgroup; all
    three K; one, two and three column tiles; N = 1, 129 and 202 (16-byte and 4-byte stores in one row); an odd ldy; a misaligned y.
    (M, N, K, ldx - K, ldy - N, y offset in bytes, recipe, wide operand, bias)"""
    m1, m2, m3 = 128 * (cus - 1) + 1, 128 * cus + 77, 128 * (2 * cus + 2) + 5
    return [(m1, 1, 64, 0, 3, 0, "ints", "x", True),
            (m2, 129, 128, 4, 0, 0, "sparse", "x", False),      # ldy = 129: odd
            (m3, 260, 256, 0, 0, 0, "ints", "w", True),
            (m2, 202, 256, 0, 2, 0, "sparse", "w", False),      # ldy = 204, aligned: 16-byte stores up to column 199, then two of 4 bytes
            (m1, 130, 128, 4, 2, 4, "ints", "x", True),         # y starts 4 bytes past a 16-byte boundary
            (m3, 64, 64, 4, 0, 0, "sparse", "x", False)]


def takes_persistent_form(M, K, cus):
    """adkf_dense_forward's own selection rule (csrc/host_dense.h)."""
    return K in (64, 128, 256) and -(-M // 128) >= cus


def wgrad_ranges(M, N, K, cus):
    """Row ranges of adkf_dense_weight_grad (csrc/host_dense.h::dense_tn_splits); its scratch is 4 N K bytes for each."""
    tiles = -(-N // 128) * -(-K // 128)
    s = max(1, min(-(-4 * cus // tiles), (M + 127) // 128, 64))
    rps = -(-(-(-M // s)) // 32) * 32
    return -(-M // rps)


# ---- the split: values and the CPU cut ------------------------------------------------------------------------------------
SPLIT_SHAPES = [(1, 8), (4, 2), (3, 40), (256, 34), (5, 104)]       # (rows, K); 5 x 104: 260 pairs, a ragged second block
SPLIT_T_SHAPES = [(2, 4), (34, 12), (64, 130), (256, 256)]          # (K, N)


def cpu_cut(x):
    """The three planes of a float32 tensor as bfloat16 bit patterns [3, ...] (int16): torch's CPU conversion rounds to nearest even."""
    x0 = x.bfloat16()
    r = x - x0.float()
    x1 = r.bfloat16()
    x2 = (r - x1.float()).bfloat16()
    return torch.stack((x0, x1, x2)).view(torch.int16)


def planes_sum(planes):
    """float64 sum of the three decoded planes"""
    return planes.view(torch.bfloat16).double().sum(0)


@functools.lru_cache(maxsize=None)
def split_values(n):
    """n float32 values on which the split is held to the CPU cut: normal data at six scales, exact ties under an even and an odd
    upper half, values that round up into the next binade, +-0, bfloat16 values, 0x7F7F7FFF (the largest float that does not round to
    inf) and 2^-108 - in a seeded order, repeated or cut to n."""
    g = torch.Generator().manual_seed(8000)
    bits = [0x3F808000, 0x3F818000, 0x40498000, 0x404A8000, 0x40008000, 0x40018000,           # ties: even / odd upper half
            0x3FFFFFFF, 0x3FFF8000, 0x407FFFFF, 0x3FFFC000, 0x3FFF7FFF,                           # up into the next binade (and just not)
            0x00000000, 0x3F800000, 0x40200000, 0x7F7F0000, 0x00800000, 0x7F7F7FFF, 0x09800000]   # 0, bfloat16 values, 2^-108
    pos = torch.tensor(bits, dtype=torch.int32).view(torch.float32)
    special = torch.cat((pos, -pos))
    normal = torch.cat([torch.randn(256, generator=g) * s for s in (1e-30, 1e-3, 1.0, 37.0, 1e20, 1e30)])
    normal = torch.copysign(normal.abs().clamp(min=2.0 ** -108), normal)      # (the few 1e-30 draws below 2^-108: see denormal_values)
    pool = torch.cat((special.repeat(8), normal))
    pool = pool[torch.randperm(pool.numel(), generator=g)]
    return pool[torch.arange(n) % pool.numel()].clone()


@functools.lru_cache(maxsize=None)
def denormal_values(n):
    """Values below 2^-108, where a piece is a bfloat16 denormal: run and reported, nothing asserted."""
    g = torch.Generator().manual_seed(8001)
    pool = torch.cat((torch.randn(64, generator=g) * 1e-34, torch.randn(64, generator=g) * 1e-37, torch.randn(64, generator=g) * 1e-40,
                      torch.tensor([2.0 ** -109, 2.0 ** -120 * 1.5, 2.0 ** -126, 2.0 ** -127, 2.0 ** -133, 2.0 ** -149])))
    pool = pool[pool.abs() < 2.0 ** -108]
    return pool[torch.arange(n) % pool.numel()].clone()


# ---- the pieces --------------------------------------------------------------------------------------------------------
def pieces(t):
    """The three bfloat16 pieces of a float32 tensor (round to nearest even at every cut), as float32 numpy arrays."""
    return _split3(t.numpy(), _bf16_rn)


def term_products(a, b):
    """{(i, j): a_i b_j^T in float64} for the six kept terms (a [M, n], b [N, n]: the contraction runs along the rows of both)."""
    pa, pb = pieces(a), pieces(b)
    return {(i, j): pa[i].astype(np.float64) @ pb[j].astype(np.float64).T for i, j in KEPT}


def _ints(g, shape, bits):
    top = 1 << bits
    hi = torch.randint(top // 2, top, shape, generator=g)
    lo = torch.randint(0, top // 2, shape, generator=g)
    mag = torch.where(torch.rand(shape, generator=g) < 0.75, hi, lo)
    return (mag * (1 - 2 * torch.randint(0, 2, shape, generator=g))).float()


def _wide22(g, shape):
    mag = 2 * torch.randint(2 ** 20, 2 ** 21, shape, generator=g) + 1          # odd, in (2^21, 2^22)
    return (mag * (1 - 2 * torch.randint(0, 2, shape, generator=g))).float()


def _sparse(g, rows, n, stride=1):
    """[rows, n]: row r holds +-1 at (7 r stride + 3) mod n and +-1 or +-2 at (r stride) mod n (one non-zero where the two coincide)."""
    s = torch.zeros(rows, n)
    r = torch.arange(rows)
    sign = lambda: (1 - 2 * torch.randint(0, 2, (rows,), generator=g)).float()
    s[r, (7 * r * stride + 3) % n] = sign()
    s[r, (r * stride) % n] = sign() * torch.randint(1, 3, (rows,), generator=g).float()
    return s


def _bias(g, N):
    return torch.randint(-64, 65, (N,), generator=g).float()


def _forward_case(x, w, b):
    y64 = x.double() @ w.double().t()
    return dict(x=x, w=w, b=b, y64=y64, ref=y64.float(), ref_bias=(y64 + b.double()).float())


# ---- forward recipes: y[M, N] = x[M, K] w[N, K]^T (+ b) -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_ints(M, N, K, wide):
    g = torch.Generator().manual_seed(1000 + M + 7 * N + 13 * K + (wide == "w"))
    bx, bw = FWD_BITS[K] if wide == "x" else FWD_BITS[K][::-1]
    return _forward_case(_ints(g, (M, K), bx), _ints(g, (N, K), bw), _bias(g, N))


@functools.lru_cache(maxsize=None)
def forward_sparse(M, N, K, wide):
    g = torch.Generator().manual_seed(2000 + M + 7 * N + 13 * K + (wide == "w"))
    if wide == "x":
        return _forward_case(_wide22(g, (M, K)), _sparse(g, N, K), _bias(g, N))
    return _forward_case(_sparse(g, M, K), _wide22(g, (N, K)), _bias(g, N))


@functools.lru_cache(maxsize=None)
def forward_onehot(M, N, K):
    g = torch.Generator().manual_seed(3000 + M + 7 * N + 13 * K)
    sign = lambda shape: (1 - 2 * torch.randint(0, 2, shape, generator=g)).float()
    sig = (2 * torch.randint(2 ** 10, 2 ** 11, (M,), generator=g) + 1).float()          # odd, 12 bits
    x = torch.zeros(M, K)
    x[torch.arange(M), torch.arange(M) % K] = torch.ldexp(sign((M,)) * sig, torch.randint(-60, 41, (M,), generator=g))
    w = torch.ldexp(sign((N, K)) * torch.randint(2 ** 11, 2 ** 12, (N, K), generator=g).float(), torch.randint(-40, 41, (N, K), generator=g))
    c = _forward_case(x, w, _bias(g, N))
    c["ref_bias"] = c["ref"] + c["b"]          # two exact floats, one float32 addition: rounded once
    return c


def forward_cases(M, N, K):
    """(name, case) of every exact recipe at one shape, the two-sided ones both ways round."""
    return [("ints/x", forward_ints(M, N, K, "x")), ("ints/w", forward_ints(M, N, K, "w")),
            ("sparse/x", forward_sparse(M, N, K, "x")), ("sparse/w", forward_sparse(M, N, K, "w")), ("onehot", forward_onehot(M, N, K))]


# ---- weight-gradient recipes: dw[N, K] = g[M, N]^T x[M, K] ---------------------------------------------------------------
def _wgrad_case(gm, x):
    dw64 = gm.double().t() @ x.double()
    return dict(g=gm, x=x, dw64=dw64, ref=dw64.float())


@functools.lru_cache(maxsize=None)
def wgrad_ints(M, N, K, wide):
    g = torch.Generator().manual_seed(4000 + M + 7 * N + 13 * K + (wide == "x"))
    bg, bx = wgrad_bits(M) if wide == "g" else wgrad_bits(M)[::-1]
    return _wgrad_case(_ints(g, (M, N), bg), _ints(g, (M, K), bx))


@functools.lru_cache(maxsize=None)
def wgrad_sparse(M, N, K, wide):
    """The sparse operand's non-zeros run along the rows (the contraction): column c at rows (c s) mod M and (7 c s + 3) mod M, with
    s = M // columns (at least 1), so that the row ranges of a long contraction are all reached."""
    g = torch.Generator().manual_seed(5000 + M + 7 * N + 13 * K + (wide == "x"))
    cols = K if wide == "g" else N
    sp = _sparse(g, cols, M, max(1, M // cols)).t().contiguous()
    return _wgrad_case(_wide22(g, (M, N)), sp) if wide == "g" else _wgrad_case(sp, _wide22(g, (M, K)))


def wgrad_cases(M, N, K):
    return [("ints/g", wgrad_ints(M, N, K, "g")), ("ints/x", wgrad_ints(M, N, K, "x")),
            ("sparse/g", wgrad_sparse(M, N, K, "g")), ("sparse/x", wgrad_sparse(M, N, K, "x"))]


# ---- random data of the two rounding checks -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def normal_case(M, N, K, seed=0):
    """x ~ 1.5 N(0, 1), w ~ N(0, 1) / sqrt(K).  The first 256 rows of a longer x are the 256-row case's."""
    g = torch.Generator().manual_seed(6000 + K + seed)
    x = torch.randn(256, K, generator=g) * 1.5
    w = torch.randn(N, K, generator=g) / K ** 0.5
    if M > 256:
        x = torch.cat((x, torch.randn(M - 256, K, generator=g) * 1.5))
    return dict(x=x[:M].contiguous(), w=w)


@functools.lru_cache(maxsize=None)
def same_sign_case(rows_a, rows_b, n, seed=0):
    """Two operands uniform in [1, 2), [rows_a, n] and [rows_b, n]: the dropped terms cannot cancel."""
    g = torch.Generator().manual_seed(7000 + seed)
    return dict(a=1.0 + torch.rand(rows_a, n, generator=g), b=1.0 + torch.rand(rows_b, n, generator=g))


def f32_sequential(x, w):
    """The float32 sum of the float32 products x[m, k] w[n, k] in k order: the yardstick of check 6."""
    acc = torch.zeros(x.shape[0], w.shape[0])
    tmp = torch.empty_like(acc)
    wt = w.t().contiguous()
    for k in range(x.shape[1]):
        torch.mul(x[:, k:k + 1], wt[k:k + 1], out=tmp)      # (rounded by itself: no fused multiply-add)
        acc += tmp
    return acc


def unit_error(y, x, w):
    """max |y - x w^T| / sum_k |x||w|, the reference and the scale in float64."""
    xd, wd = x.double(), w.double()
    return (((y.double() - xd @ wd.t()).abs()) / (xd.abs() @ wd.abs().t() + 1e-300)).max().item()


def five_term_errors(x, w):
    """{dropped term: unit error of the sum of the other five products}, and the six-term error under the key ``None``."""
    t = term_products(x, w)
    exact = x.double().numpy() @ w.double().numpy().T
    scale = np.abs(x.double().numpy()) @ np.abs(w.double().numpy()).T + 1e-300
    six = sum(t.values())
    out = {None: float(np.max(np.abs(six - exact) / scale))}
    for drop in KEPT:
        out[drop] = float(np.max(np.abs(six - t[drop] - exact) / scale))
    return out


def rounding_bound(x, w, five_min):
    """Check 6: 2 x the float32 sequential sum's error, and never past half the smallest five-term error."""
    yard = unit_error(f32_sequential(x, w), x, w)
    return min(2.0 * yard, 0.5 * five_min), yard
