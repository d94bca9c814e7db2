"""CPU: adkf_ehvi_pool without a GPU - the reference of ehvi_ref.py against quadrature, Monte Carlo and known answers; the entry is
exported, refuses cleanly with no device and checks every argument before any launch; gp_ops.ehvi_pool's, gp_ops.pareto_front's and
the BO loop's argument handling; the CPU twin against the reference (isotropic and ARD, RBF and Matern, P = 0, 1, 7 and 64, C = 0, 2
and 4, mixed senses, linear and log) and the semantics of the call on the twin; and that the bound of the GPU test is informative on
the GPU test's problems."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import believer_ref as B
import ehvi_ref as R
import jes_ref as J
from adkf_ift_amd import _lib
from test_believer_pool_ard_cpu import ard_posterior
from test_predict_pool_cpu import _problem, _twin, lib  # noqa: F401  (lib: the fixture)

BADARG, SIZE, WORKSPACE, LAUNCH = -1, -2, -3, -4
ARD = 4
LATENT, MAXIMIZE, LOG = 1, 2, 16
EPS32 = R.EPS32
CHUNK = _lib.EHVI_CHUNK_ROWS

# the problems of tests/test_gpu_ehvi_pool.py's score test: (kernel, n_s, d, rows, P, C)
GPU_CASES = [("rbf", [32, 29, 21, 30], 16, 200, 7, 0), ("matern", [200, 133, 64], 16, 130, 64, 2), ("matern", [32, 32], 3, 65, 1, 1),
             ("matern", [200, 133, 64], 16, 130, 64, 2), ("rbf", [32, 29, 21, 30], 16, 200, 33, 0)]
# the fronts of the first three are made of support labels and clean down to 1 to 7 points; the last two are anti-chains, every point
# of which survives: staircases of 64 steps (65 strips: the most there can be) and of 33 (34 strips: not a multiple of the four waves)
GPU_CHAIN = [False, False, False, True, True]


def gpu_problem(case):
    """(Zs, ys, X, phi, groups) of a GPU score case, on the host."""
    kernel, n_s, d, rows, P, Cn = GPU_CASES[case]
    Zs, ys, X, phi = J.problem(n_s, d, rows, 1300 + case)
    return Zs, ys, X, phi, R.make_groups(ys.numpy(), n_s, P, Cn, 7 + case, chain=GPU_CHAIN[case])


# ---- the reference checks itself
def _toy_front(seed, P):
    g = np.random.default_rng(seed)
    x = np.sort(g.uniform(-1.0, 1.0, P))
    y = np.sort(g.uniform(-1.0, 1.0, P))[::-1]
    return np.stack([x, y], 1), np.array([1.3, 1.2])


def test_the_reference_against_quadrature_and_monte_carlo():
    compared = 0
    for seed, P in ((1, 0), (2, 1), (3, 4), (4, 9)):
        F, r = _toy_front(seed, P)
        a, b = R.staircase(F, r)
        g = np.random.default_rng(100 + seed)
        for _ in range(3):
            m1, m2, s1, s2 = g.uniform(-1, 1), g.uniform(-1, 1), g.uniform(0.1, 0.8), g.uniform(0.1, 0.8)
            val, _ = R.ehvi(np.array([m1]), np.array([s1 * s1]), np.array([m2]), np.array([s2 * s2]), a, b, r[0], r[1])
            quad = R.by_quadrature(m1, s1, m2, s2, a, b, r[0], r[1])
            assert abs(val[0] - quad) <= 1e-9 * max(1.0, quad), (seed, P, val[0], quad)
            mc, se = R.by_monte_carlo(m1, s1, m2, s2, a, b, r[0], r[1], seed=seed)
            assert abs(val[0] - mc) <= 4.5 * se, (seed, P, val[0], mc, se)
            compared += 1
    assert compared == 12


def test_the_reference_on_known_answers():
    g = np.random.default_rng(5)
    rows = 50
    m1, m2, v1, v2 = g.normal(size=rows), g.normal(size=rows), g.uniform(0.01, 1.0, rows), g.uniform(0.01, 1.0, rows)
    r = np.array([1.0, 0.8])
    # an empty front: the product of two EIs; one objective: EI
    e1, e2 = R.ei(m1, v1, r[0])[0], R.ei(m2, v2, r[1])[0]
    val, _ = R.ehvi(m1, v1, m2, v2, (), (), r[0], r[1])
    assert np.abs(val - e1 * e2).max() <= 1e-15
    assert np.array_equal(R.group_ref(m1, v1, None, None, (), (), r[0], None)["lin"], e1)
    z = (r[0] - m1) / np.sqrt(v1)
    from scipy import special as sp
    assert np.abs(e1 - np.sqrt(v1) * (z * sp.ndtr(z) + np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi))).max() <= 1e-15
    # junk changes nothing: a dominated point, one outside ref, a duplicate, a NaN; a permutation gives the same staircase
    F, _ = _toy_front(6, 6)
    a, b = R.staircase(F, r)
    junk = np.concatenate([F, [[F[2, 0] + 0.01, F[2, 1] + 0.01], [1.5, -2.0], [-2.0, 0.8], F[4], [np.nan, 0.0]]])
    a2, b2 = R.staircase(junk, r)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and len(a) == 6
    a3, b3 = R.staircase(junk[g.permutation(len(junk))], r)
    assert np.array_equal(a, a3) and np.array_equal(b, b3)
    base, _ = R.ehvi(m1, v1, m2, v2, a, b, r[0], r[1])
    # swapping the objectives with their columns
    sa, sb = R.staircase(F[:, ::-1], r[::-1])
    swapped, _ = R.ehvi(m2, v2, m1, v1, sa, sb, r[1], r[0])
    assert np.abs(base - swapped).max() <= 1e-12
    # one more non-dominated point never raises the score
    more = np.concatenate([F, [[0.5 * (a[2] + a[3]), 0.5 * (b[2] + b[3]) - 0.4 * (b[2] - b[3])]]])
    a4, b4 = R.staircase(more, r)
    assert len(a4) == 7
    assert (R.ehvi(m1, v1, m2, v2, a4, b4, r[0], r[1])[0] <= base + 1e-15).all()
    # maximised objectives: the same number on the negated problem
    am, bm = R.staircase(-F, -r, (True, True))
    assert np.array_equal(am, a) and np.array_equal(bm, b)
    # the log reference is the log of the linear one where both exist, and finite where the linear one has underflowed
    cons = [(m2, v2, 0.1, False), (m1, v1, -0.2, True)]
    gr = R.group_ref(m1, v1, m2, v2, a, b, r[0], r[1], cons)
    assert np.abs(gr["log"] - np.log(gr["lin"])).max() <= 1e-12
    far = R.group_ref(m1 + 60.0, v1 * 1e-2, m2 + 50.0, v2 * 1e-2, a, b, r[0], r[1])
    assert (far["lin"] == 0).all() and np.isfinite(far["log"]).all() and (far["log"] < -1000).all()


def test_pareto_front_obeys_the_cleaning_rule():
    from adkf_ift_amd import gp_ops

    g = np.random.default_rng(8)
    for mx in ((False, False), (True, False), (True, True)):
        Y = g.normal(size=(40, 2)).astype(np.float32)
        Y[7] = Y[3]; Y[11, 0] = np.nan
        ref = np.array([-1.0 if mx[0] else 1.0, -1.2 if mx[1] else 1.2], np.float32)
        st = gp_ops.pareto_front(torch.from_numpy(Y), mx, torch.from_numpy(ref)).numpy()
        a, b = R.staircase(Y, ref, mx)
        sg = np.array([-1.0 if m else 1.0 for m in mx])
        assert np.array_equal(st * sg, np.stack([a, b], 1)) and 1 < len(a) < 40
        # without a reference point only dominance cleans
        free = gp_ops.pareto_front(torch.from_numpy(Y), mx).numpy()
        a, b = R.staircase(Y, np.array([np.inf, np.inf]) * sg, mx)
        assert np.array_equal(free * sg, np.stack([a, b], 1))
    assert gp_ops.pareto_front(torch.zeros(0, 2)).shape == (0, 2)
    with pytest.raises(ValueError, match="Y must be"):
        gp_ops.pareto_front(torch.zeros(4, 3))


# ---- the entry of the device library
def _host_call(lib, T=3, ns=16, nq=0, d=8, rows=10, G=2, P=4, Cn=2, k=3, ard=False, flags=0, x=True, obj=True, ref=True, front=True,
               front_n=True, con=(True, True, True), outs=(True, False, False), top=(True, True), excl=(False, False), info=True, ws=True,
               ws_short=0, scratch_short=0, scratch_off=0):
    """Host memory stands in for device memory: nothing is dereferenced on the host."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    Zs, ys, pri, phi = torch.zeros(T, ns, d), torch.zeros(T, ns), torch.zeros(T, 4), torch.zeros(T, 2 + d if ard else 3)
    Zq_b = torch.zeros(T, max(nq, 1), d)
    X = torch.zeros(max(rows, 1), d) if x else None
    Gm, Pm, Cm, kk = max(G, 1), min(max(P, 1), 64), min(max(Cn, 1), 4), min(max(k, 0), 64)
    obj_t, mx_t, ref_t = torch.zeros(Gm, 2, dtype=torch.int32), torch.zeros(Gm, 2, dtype=torch.int32), torch.zeros(Gm, 2)
    front_t, fn_t = torch.zeros(Gm, Pm, 2), torch.zeros(Gm, dtype=torch.int32)
    con_t, thr_t, geq_t = torch.zeros(Gm, Cm, dtype=torch.int32), torch.zeros(Gm, Cm), torch.zeros(Gm, Cm, dtype=torch.int32)
    score, stair, stair_n = torch.zeros(Gm * max(rows, 1)), torch.zeros(Gm * Pm * 2), torch.zeros(Gm, dtype=torch.int32)
    inf = torch.zeros(T, dtype=torch.int32)
    top_idx, top_val = torch.zeros(Gm * max(kk, 1), dtype=torch.int64), torch.zeros(Gm * max(kk, 1))
    e_idx, e_off = torch.zeros(4, dtype=torch.int64), torch.zeros(Gm + 1, dtype=torch.int64)
    nb = (lib.adkf_workspace_bytes_ard if ard else lib.adkf_workspace_bytes)(T, ns, 0, d)
    wsb = torch.zeros(nb // 4 + 64)
    sb = lib.adkf_ehvi_pool_scratch_bytes(T, Gm, kk)
    scratch = torch.zeros(sb // 4 + 64)
    b = _lib.Batch()
    b.T, b.ns_max, b.nq_max, b.d, b.kernel, b.flags = T, ns, nq, d, 0, ARD if ard else 0
    b.n_s = b.n_q = None
    b.Z_s, b.y_s, b.priors = Zs.data_ptr(), ys.data_ptr(), pri.data_ptr()
    b.Z_q = Zq_b.data_ptr() if nq else None
    b.y_q = None
    return lib.adkf_ehvi_pool(C.byref(b), p(phi), flags, p(X), rows, G, p(obj_t) if obj else None, p(mx_t), p(ref_t) if ref else None,
                              p(front_t) if front else None, p(fn_t) if front_n else None, P, p(con_t) if con[0] else None,
                              p(thr_t) if con[1] else None, p(geq_t) if con[2] else None, Cn, p(e_idx) if excl[0] else None,
                              p(e_off) if excl[1] else None, p(score) if outs[0] else None, p(stair) if outs[1] else None,
                              p(stair_n) if outs[2] else None, k, p(top_idx) if top[0] else None, p(top_val) if top[1] else None,
                              p(inf) if info else None, p(wsb) if ws else None, nb - ws_short, C.c_void_p(scratch.data_ptr() + scratch_off),
                              sb - scratch_short, None)


def test_the_entry_is_exported(lib):
    assert "adkf_ehvi_pool" in _lib.SIGNATURES and "adkf_ehvi_pool_scratch_bytes" in _lib.SIGNATURES
    fn = lib.adkf_ehvi_pool   # a library without the entry point fails here
    assert fn.restype is C.c_int and len(fn.argtypes) == 30
    assert _lib.EHVI_FRONT_MAX == 64 and _lib.EHVI_CONS_MAX == 4 and CHUNK % 64 == 0 and CHUNK > 0


def test_the_scratch_size(lib):
    f = lib.adkf_ehvi_pool_scratch_bytes
    assert len(f.argtypes) == 3   # T, G, k: rows, ns and d are no arguments
    base = f(3, 2, 0)
    assert base >= 2 * 3 * CHUNK * 4 and base % 8 == 0           # stage A's mean and variance of one chunk
    assert f(4, 2, 0) - base >= 2 * CHUNK * 4
    assert all(f(T + 1, 2, 5) > f(T, 2, 5) for T in range(1, 40))
    assert all(f(3, G + 1, 5) >= f(3, G, 5) for G in range(1, 300)) and f(3, 300, 5) > f(3, 1, 5) and f(3, 10000, 5) > f(3, 4096, 5)
    assert all(f(3, 7, k + 1) > f(3, 7, k) for k in range(0, 64))
    assert all(f(T, G, k) % 8 == 0 for T in (1, 5) for G in (1, 3, 5000) for k in (0, 1, 7, 64))
    for bad in ((0, 2, 0), (-1, 2, 0), (3, 0, 0), (3, -2, 4), (3, 2, -1), (3, 2, 65)):
        assert f(*bad) == 0, bad


def test_no_device_returns_launch_error(lib):
    if torch.cuda.is_available():
        pytest.skip("this is the no-device check")
    assert _host_call(lib) == LAUNCH
    assert _host_call(lib, rows=0, x=False) == LAUNCH
    assert _host_call(lib, ard=True, d=12, rows=7, P=0, front=False, Cn=0, con=(False, False, False), k=0, flags=LOG) == LAUNCH
    assert _host_call(lib, ns=200, rows=5, G=600, P=64, Cn=4, k=64, outs=(True, True, True), excl=(True, True)) == LAUNCH
    assert _host_call(lib, k=0, outs=(False, True, False), top=(False, False)) == LAUNCH
    assert _host_call(lib, k=0, outs=(False, False, True), top=(False, False)) == LAUNCH


def test_bad_arguments_are_rejected_before_any_launch(lib):
    assert _host_call(lib, nq=4) == BADARG                                     # a batch with a query set
    assert _host_call(lib, rows=-1) == BADARG
    assert _host_call(lib, x=False) == BADARG                                  # rows > 0 without X
    for G in (0, -3):
        assert _host_call(lib, G=G) == BADARG
    for P in (-1, 65):
        assert _host_call(lib, P=P) == SIZE
    for Cn in (-1, 5):
        assert _host_call(lib, Cn=Cn) == SIZE
    assert _host_call(lib, k=65) == SIZE
    assert _host_call(lib, obj=False) == BADARG
    assert _host_call(lib, ref=False) == BADARG
    assert _host_call(lib, front_n=False) == BADARG
    assert _host_call(lib, front=False) == BADARG                              # P > 0 without front
    for con in ((False, True, True), (True, False, True), (True, True, False)):
        assert _host_call(lib, con=con) == BADARG                              # C > 0 without con, con_thr or con_geq
    assert _host_call(lib, info=False) == BADARG
    assert _host_call(lib, ws=False) == BADARG
    assert _host_call(lib, excl=(True, False)) == BADARG                       # excl_idx without excl_off
    assert _host_call(lib, k=-1) == BADARG
    assert _host_call(lib, top=(False, True)) == BADARG
    assert _host_call(lib, top=(True, False)) == BADARG
    assert _host_call(lib, k=0, outs=(False, False, False)) == BADARG          # no output at all
    assert _host_call(lib, scratch_off=4) == BADARG                            # a misaligned scratch
    for bit in (LATENT, MAXIMIZE, 4, 8, 32):
        assert _host_call(lib, flags=bit) == BADARG                            # flag bits other than LOG_EI
        assert _host_call(lib, flags=bit | LOG) == BADARG
    assert _host_call(lib, ws_short=1) == WORKSPACE
    assert _host_call(lib, ard=True, ws_short=1) == WORKSPACE
    assert _host_call(lib, scratch_short=1) == WORKSPACE


def test_gp_ops_argument_handling(lib):
    from adkf_ift_amd import gp_ops

    iso = types.SimpleNamespace(nq=0, ard=False, T=3, d=5)
    obj, ref = [[0, 1], [2, -1]], torch.zeros(2, 2)
    with pytest.raises(ValueError, match="support-only"):
        gp_ops.ehvi_pool(types.SimpleNamespace(nq=3, ard=False, T=3, d=5), None, None, obj=obj, ref=ref)
    for k in (-1, 65):
        with pytest.raises(ValueError, match="topk must be"):
            gp_ops.ehvi_pool(iso, None, None, obj=obj, ref=ref, topk=k)
    for bad in (torch.zeros(2, 2), [0, 1], [[0, 1, 2]], torch.zeros(0, 2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="obj must be"):
            gp_ops.ehvi_pool(iso, None, None, obj=bad, ref=ref)
    for bad in (torch.zeros(3, 2), torch.zeros(2), [[0.0, 1.0]]):
        with pytest.raises(ValueError, match="ref must be"):
            gp_ops.ehvi_pool(iso, None, None, obj=obj, ref=bad)
    for bad in (torch.zeros(2, 4), torch.zeros(3, 4, 2), torch.zeros(2, 4, 3)):
        with pytest.raises(ValueError, match="front must be"):
            gp_ops.ehvi_pool(iso, None, None, obj=obj, ref=ref, front=bad)
    with pytest.raises(ValueError, match="front points P must be"):
        gp_ops.ehvi_pool(iso, None, None, obj=obj, ref=ref, front=torch.zeros(2, 65, 2))
    with pytest.raises(ValueError, match="constraints C must be"):
        gp_ops.ehvi_pool(iso, None, None, obj=obj, ref=ref, con=torch.zeros(2, 5, dtype=torch.int32), con_thr=torch.zeros(2, 5))
    with pytest.raises(ValueError, match="no output"):
        gp_ops.ehvi_pool(iso, None, None, obj=obj, ref=ref, want_score=False)


def test_the_bo_loop_checks_its_arguments():
    from adkf_ift_amd import bayes_opt as BO

    X, y = torch.randn(20, 3), torch.randn(20, 2)
    for q in (0, 65):
        with pytest.raises(ValueError, match="query_batch_size must be"):
            BO.run_gp_ehvi_bo_batched(X, y, 4, q, 1, "matern", "cpu", 10, 0.01, True, rngs=[np.random.default_rng(0)])
    for bad in (torch.randn(20), torch.randn(20, 3), torch.randn(19, 2)):
        with pytest.raises(ValueError, match=r"y_all must be \[n, 2\]"):
            BO.run_gp_ehvi_bo_batched(X, bad, 4, 2, 1, "matern", "cpu", 10, 0.01, True, rngs=[np.random.default_rng(0)])
    with pytest.raises(ValueError, match="acquisition must be"):
        BO.run_gp_ehvi_bo_batched(X, y, 4, 2, 1, "matern", "cpu", 10, 0.01, True, rngs=[np.random.default_rng(0)], acquisition="ei")
    # the reference point: the worst value plus 0.1 of the range per sense, and never on the points when an objective has no range
    Y = torch.tensor([[0.0, 2.0], [1.0, 2.0], [0.5, 2.0]])
    assert torch.allclose(BO._ehvi_ref_point(Y, (False, False)), torch.tensor([1.1, 2.1]))
    assert torch.allclose(BO._ehvi_ref_point(Y, (True, True)), torch.tensor([-0.1, 1.9]))
    assert abs(BO._hypervolume_2d(Y, (False, False), torch.tensor([1.1, 2.1])) - 1.1 * 0.1) < 1e-6


# ---- the twin
def _ehvi_twin():
    cpu_twin, _ = _twin()
    tw = cpu_twin.load()
    fn = tw.adkf_ehvi_pool   # a twin library without the entry point fails here
    fn.restype, fn.argtypes = _lib.SIGNATURES["adkf_ehvi_pool"]
    sb = tw.adkf_ehvi_pool_scratch_bytes
    sb.restype, sb.argtypes = _lib.SIGNATURES["adkf_ehvi_pool_scratch_bytes"]
    assert sb(3, 2, 5) == 0
    return fn


def ehvi_call(fn, b, phi, X, grp, log=False, k=0, excl=None, want_score=True, ok=True):
    """The twin's adkf_ehvi_pool on host arrays: dict(score, stair, stair_n, top_idx, top_val, info)."""
    pp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rows, G, P, Cn = X.shape[0], grp["G"], grp["P"], grp["C"]
    score = np.full((G, rows), -7.0, np.float32) if want_score else None
    stair = np.full((G, max(P, 1), 2), np.nan, np.float32)
    stair_n = np.full(G, -7, np.int32)
    info = np.empty(b.T, np.int32)
    top_idx = np.full((G, max(k, 1)), -7, np.int64)
    top_val = np.full((G, max(k, 1)), np.nan, np.float32)
    e_idx, e_off = excl if excl is not None else (None, None)
    rc = fn(C.byref(b.c), pp(phi), LOG if log else 0, pp(X), rows, G, pp(grp["obj"]), pp(grp["obj_max"]), pp(grp["ref"]), pp(grp["front"]),
            pp(grp["front_n"]), P, pp(grp["con"]), pp(grp["con_thr"]), pp(grp["con_geq"]), Cn, pp(e_idx), pp(e_off), pp(score),
            pp(stair) if P else None, pp(stair_n), k, pp(top_idx) if k else None, pp(top_val) if k else None, pp(info), None, 0, None, 0, None)
    assert rc == 0
    if ok:
        assert (info == 0).all()
    return dict(score=score, stair=stair[:, :P], stair_n=stair_n, top_idx=top_idx, top_val=top_val, info=info)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _mv(b, Zs, ys, n_s, X, phi, kind, ard):
    posts = [(ard_posterior(Zs[t, :n_s[t]].numpy(), ys[t, :n_s[t]], X, phi[t], kind) if ard else
              B.posterior(Zs[t, :n_s[t]], ys[t, :n_s[t]], X, phi[t], kind)) for t in range(b.T)]
    return np.stack([p[0] for p in posts]), np.stack([p[1].diagonal() for p in posts])


def _check_stair(out, grp):
    from adkf_ift_amd import gp_ops

    for g in range(grp["G"]):
        two = grp["obj"][g, 1] >= 0 and grp["P"] > 0
        want = gp_ops.pareto_front(torch.from_numpy(grp["front"][g, :grp["front_n"][g]]), [bool(x) for x in grp["obj_max"][g]],
                                   torch.from_numpy(grp["ref"][g])).numpy() if two else np.zeros((0, 2), np.float32)
        n = out["stair_n"][g]
        assert n == len(want), (g, n, len(want))
        assert np.array_equal(_bits(out["stair"][g, :n]), _bits(want)) and (out["stair"][g, n:] == 0).all(), g


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("kind,ard,P,Cn,chain", [(0, False, 0, 0, False), (1, False, 1, 2, False), (0, True, 7, 4, False), (1, True, 64, 2, False),
                                                 (1, False, 64, 0, False), (0, False, 7, 2, False), (1, False, 64, 2, True), (0, True, 64, 0, True),
                                                 (0, False, 33, 1, True)])
def test_cpu_twin_against_the_reference(kind, ard, P, Cn, chain, log):
    """The twin rounds a float64 evaluation to float32 at the boundary; its posterior and the oracle's differ by float64 rounding:
    |score - ref| <= 2 eps32 |ref| + 1e-8.  The staircase it returns is gp_ops.pareto_front's.  chain: an anti-chain front, whose
    staircase keeps all P points (asserted) - label fronts clean down to a handful."""
    fn = _ehvi_twin()
    rows = 40
    b, Zs, ys, n_s, X, phi, _ = _problem(kind, ard, 80 + kind + 2 * ard, rows=rows)
    m, v = _mv(b, Zs, ys, n_s, X, phi, kind, ard)
    compared = 0
    for two in (True, False):
        grp = R.make_groups(ys.numpy(), n_s, P, Cn, 5 + P, two=two, chain=chain)
        out = ehvi_call(fn, b, phi, X, grp, log=log)
        _check_stair(out, grp)
        if chain and two:
            assert (out["stair_n"] == P).all(), out["stair_n"]
        for g in range(grp["G"]):
            ref = R.score_ref(m, v, grp, g)["log" if log else "lin"]
            err = np.abs(out["score"][g].astype(np.float64) - ref)
            assert (err <= 2 * EPS32 * np.abs(ref) + 1e-8).all(), (two, g, float(err.max()))
            compared += ref.size
    assert compared == 2 * 3 * rows


def test_semantics_on_the_twin():
    fn = _ehvi_twin()
    rows = 70
    b, Zs, ys, n_s, X, phi, _ = _problem(1, False, 91, rows=rows)
    X[10] = X[3]; X[41] = X[3]; X[69] = X[20]          # exact duplicate rows: bit-equal scores
    grp = R.make_groups(ys.numpy(), n_s, 7, 2, 3)
    base = ehvi_call(fn, b, phi, X, grp)
    # exclusions per group, the order on duplicates, and score == NULL gives the same selection
    lists = [sorted({int(np.argmax(base["score"][0])), 5, 6}), [], sorted(set(range(rows)) - {3, 10, 41, 50})]
    e_idx = np.array([i for l in lists for i in l], np.int64)
    e_off = np.array([0] + list(np.cumsum([len(l) for l in lists])), np.int64)
    for log, k in ((False, 1), (False, 7), (True, 64)):
        out = ehvi_call(fn, b, phi, X, grp, log=log, k=k, excl=(e_idx, e_off))
        for g in range(3):
            idx, val = R.topk_of(out["score"][g], k, lists[g])
            assert np.array_equal(out["top_idx"][g], idx) and np.array_equal(_bits(out["top_val"][g]), _bits(val)), (log, k, g)
        if k == 64:
            got = out["top_idx"][2, :4].tolist()
            assert (out["top_idx"][2, 4:] == -1).all() and np.isneginf(out["top_val"][2, 4:]).all()
            assert got.index(3) < got.index(10) < got.index(41)
        quiet = ehvi_call(fn, b, phi, X, grp, log=log, k=k, excl=(e_idx, e_off), want_score=False)
        assert np.array_equal(quiet["top_idx"], out["top_idx"]) and np.array_equal(_bits(quiet["top_val"]), _bits(out["top_val"]))
    # a task shared by two groups, and a group alone has the bits it has among three
    for g in range(3):
        one = {key: (val[g:g + 1] if isinstance(val, np.ndarray) else val) for key, val in grp.items()}
        one["G"] = 1
        alone = ehvi_call(fn, b, phi, X, one)
        assert np.array_equal(_bits(alone["score"][0]), _bits(base["score"][g])), g
    # the NaN rule, case by case: the group is NaN and selects nothing, the other groups keep their bits
    def broken(**kw):
        bad = {key: (val.copy() if isinstance(val, np.ndarray) else val) for key, val in grp.items()}
        for key, (idx, val) in kw.items():
            bad[key][idx] = val
        return bad
    cases = [broken(obj=((1, 0), 3)), broken(obj=((1, 0), -1)), broken(obj=((1, 1), 7)), broken(obj=((1, 1), -2)), broken(obj=((1, 1), 1)),
             broken(ref=((1, 0), np.nan)), broken(ref=((1, 1), np.nan)), broken(con=((1, 1), 5)), broken(con=((1, 0), -3)),
             broken(con_thr=((1, 1), np.nan))]
    for i, bad in enumerate(cases):
        out = ehvi_call(fn, b, phi, X, bad, k=4)
        assert np.isnan(out["score"][1]).all() and (out["top_idx"][1] == -1).all() and np.isneginf(out["top_val"][1]).all(), i
        for g in (0, 2):
            assert np.array_equal(_bits(out["score"][g]), _bits(base["score"][g])), (i, g)
    # an unused constraint entry (-1) with a NaN threshold is not read; a NaN second ref coordinate is not read with one objective
    fine = broken(con=((1, 1), -1), con_thr=((1, 1), np.nan))
    assert np.isfinite(ehvi_call(fn, b, phi, X, fine)["score"]).all()
    single = R.make_groups(ys.numpy(), n_s, 0, 0, 3, two=False)
    single["ref"][:, 1] = np.nan
    assert np.isfinite(ehvi_call(fn, b, phi, X, single)["score"]).all()
    # an empty pool: nothing selected, the staircase still returned
    out = ehvi_call(fn, b, phi, X[:0], grp, k=3)
    assert (out["top_idx"] == -1).all() and np.isneginf(out["top_val"]).all()
    _check_stair(out, grp)
    # a NaN pool row scores NaN in every group (each task sees it) and its neighbours keep their bits
    Xn = X.copy()
    Xn[12, 2] = np.nan
    out = ehvi_call(fn, b, phi, Xn, grp, k=5)
    keep = np.arange(rows) != 12
    assert np.isnan(out["score"][:, 12]).all() and np.array_equal(_bits(out["score"][:, keep]), _bits(base["score"][:, keep]))
    assert not (out["top_idx"] == 12).any()


def test_an_empty_task_makes_its_groups_nan_on_the_twin():
    from oracle import cpu_twin

    fn = _ehvi_twin()
    b, Zs, ys, n_s, X, phi, _ = _problem(0, False, 93, rows=30)
    grp = R.make_groups(ys.numpy(), n_s, 7, 0, 3)
    base = ehvi_call(fn, b, phi, X, grp)
    n0 = n_s.copy()
    n0[1] = 0
    b0 = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((3, 4), np.float32), 0, n_s=n0)
    out = ehvi_call(fn, b0, phi, X, grp, k=2)
    assert np.isnan(out["score"][0]).all() and np.isnan(out["score"][1]).all() and (out["top_idx"][:2] == -1).all()   # groups (0, 1), (1, 2)
    assert np.array_equal(_bits(out["score"][2]), _bits(base["score"][2]))                                                 # group (2, 0)


# ---- the GPU test's bound is informative on the GPU test's problems
@pytest.mark.parametrize("case", range(len(GPU_CASES)))
def test_the_gpu_problems_have_an_informative_bound(case):
    """Conditions on the inputs of tests/test_gpu_ehvi_pool.py's score test, through the twin's posterior (float64): over the rows with a
    linear score above 1e-30, which are at least half of the pool, the median of eps32 unit / ref is at most 1e-3; and at least a
    quarter of the rows of the log test's problem (the same groups under a far reference, far_groups) have a float32 linear score of
    exactly 0."""
    from oracle import cpu_twin

    fn = _ehvi_twin()
    kernel, n_s, d, rows, P, Cn = GPU_CASES[case]
    Zs, ys, X, phi, grp = gpu_problem(case)
    kind = 0 if kernel == "rbf" else 1
    b = cpu_twin.CpuBatch(Zs.numpy(), ys.numpy(), np.zeros((len(n_s), 4), np.float32), kind, n_s=np.array(n_s, np.int32))
    Xh, ph = np.ascontiguousarray(X.numpy(), np.float32), phi.numpy()
    m, v = _mv(b, Zs, ys, n_s, Xh, ph, kind, False)
    big, total, ratios = 0, 0, []
    for g in range(grp["G"]):
        gr = R.score_ref(m, v, grp, g)
        on = gr["lin"] > 1e-30
        big += int(on.sum()); total += on.size
        ratios.append((R.bound_linear(gr) / gr["lin"])[on])
    med = float(np.median(np.concatenate(ratios)))
    print(f"case {case}: {big} of {total} rows above 1e-30, median eps32 unit / ref = {med:.2e}")
    assert 2 * big >= total and med <= 1e-3
    if GPU_CHAIN[case]:
        assert (ehvi_call(fn, b, ph, Xh, grp)["stair_n"] == P).all()   # every point of the anti-chain is a step
    for by in (MID_SHIFT, 25.0):
        out = ehvi_call(fn, b, ph, Xh, far_groups(grp, by))
        zero, size = int((out["score"] == 0).sum()), out["score"].size
        print(f"case {case}: {zero} of {size} rows with a float32 linear score of 0 with the reference moved by {by}")
        assert 4 * zero >= size
        if by == MID_SHIFT:   # ... and a positive one on at least a twentieth: zeros and non-zeros side by side
            assert 20 * int((out["score"] > 0).sum()) >= size


MID_SHIFT = 4.0


def far_groups(grp, by=25.0):
    """The groups with the reference point (and the front with it) moved ``by`` label units (the labels are sin + noise, of order 1)
    towards "better" in both objectives.  At 25 the linear score is 0 on every row, in float32 and in float64, and the log form
    runs in the deep tail of pm_log_ei; at MID_SHIFT it is 0 in float32 on part of the pool and positive on the rest - where the
    ordering of the log form matters."""
    far = {key: (val.copy() if isinstance(val, np.ndarray) else val) for key, val in grp.items()}
    shift = np.where(far["obj_max"] != 0, by, -by).astype(np.float32)
    far["ref"] = far["ref"] + shift
    if far["front"] is not None:
        far["front"] = far["front"] + shift[:, None, :]
    return far
