"""Bitwise comparison of the pool calls between two builds of the library (a refactoring must return the other build's bits).

    python tools/pool_bits.py dump OUT.pt        in each of the two trees (each with its own built library), on the GPU; or twice in one
                                                 tree, once with ADKF_LIB naming the other build of the library
    python tools/pool_bits.py compare A.pt B.pt  exit status 1 and the names of the arrays that differ, if any

dump runs, on the problems of the GPU tests (tests/test_gpu_believer_pool._explicit: plain at 48 points, refined at 200, global slots
at 1024; the ARD problem of tests/test_gpu_believer_pool_ard; tests/test_gpu_predict_pool._ill_batch, whose flagged tasks take the
float64 walks; tests/test_gpu_believer_pool_ard._f64_batch, an ARD batch whose tasks are all flagged, under float64_ard - the ARD
instances of the float64 walks): believer_pool with EI and with log EI and gibbon_pool, each with trace, predict_pool(log EI, k = 8),
believer_pool_ard, kg_pool with KG and with log KG (score, cov, ref_mean and the selection; M = 16 reference rows of lowest posterior
mean, a -1 and a repetition among them), and ehvi_pool on the problems of tests/test_gpu_ehvi_pool.py's score test (score, staircase
and selection, linear and log, with and without the constraints); on each of the six problems also mes_pool and jes_pool (score and k = 8; the optima of
jes_pool at the first eight reference rows of kg_pool, their -1 and their repetition included), gumbel_pool on fixed uniforms and
thompson_pool / thompson_pool_ard (m = 64 features and four paths from seeded generators, with the paths; also 64 paths on 128 features and
37 on 256, minimising and maximising) and qei_pool (the 64-feature basis, 80 paths in two sample blocks, four noisy picks, with trace
and incumbents; skipped where ADKF_LIB names a build without the entry) and liar_pool (a constant lie at the tasks' smallest label with
log EI, and a shared label table, each with trace; the isotropic, the ARD and both float64 problems; skipped likewise) - and saves every
returned tensor.  Then the records of the six batched BO loops of adkf_ift_amd.bayes_opt, as int64 tensors under records/: a generated pool of
400 rows in 6 dimensions, 4 initial points, batches of 2, 2 iterations, 3 replicates, 64 features, fixed seeds; the EI loop also with
batch="believer" and with ard=True, the MES loop also with max_value="gumbel" and with batch="gibbon".  compare looks at the arrays both
files have, so a tree can be held against one from before a call existed.  All lists are full (pools of 130 to 333 rows), so the
arrays do not depend on how a short list is merged."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _bind_what_the_library_has(entry):
    """ADKF_LIB may name a build of the library from before an entry existed (the way a refactoring is held against its parent commit
    from one tree): the entries that build does not export leave the binding table before the library is loaded, and dump skips
    their calls.  Returns whether `entry` is there."""
    import ctypes

    import torch  # noqa: F401  (before the library, as _lib.load has it)

    from adkf_ift_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if not hasattr(lib, n)]:
        del _lib.SIGNATURES[name]
    return entry in _lib.SIGNATURES


def dump(path):
    import torch

    import test_gpu_believer_pool as BV
    import test_gpu_believer_pool_ard as BVA
    import test_gpu_predict_pool as P
    from adkf_ift_amd import gp_ops

    dev = torch.device("cuda:0")
    out = {}
    have_qei = _bind_what_the_library_has("adkf_qei_pool")
    have_liar = _bind_what_the_library_has("adkf_liar_pool")

    def put(tag, o):
        for k, v in o.items():
            if torch.is_tensor(v):
                out[f"{tag}/{k}"] = v.cpu()

    def kg_refs(b, phi, X):
        refs = gp_ops.predict_pool(b, phi, X, topk=16, score="mean", want_mean=False, want_var=False, want_ei=False)["top_idx"].clone()
        refs[:, 4] = -1
        refs[:, 5] = refs[:, 0]
        return refs

    def liar(tag, b, phi, X, best, q):
        """liar_pool with a constant lie and with a shared label table on one problem"""
        if not have_liar:
            return
        Xc = X.cpu()
        labels = (torch.sin(Xc[:, : min(b.d, 4)].sum(-1)) + 0.1 * torch.randn(Xc.shape[0], generator=torch.Generator().manual_seed(9))).to(dev)
        put(f"liar/{tag}/lie", gp_ops.liar_pool(b, phi, X, best_f=best, q=q, lie="min", log_ei=True, want_trace=True))
        put(f"liar/{tag}/labels", gp_ops.liar_pool(b, phi, X, best_f=best, q=q, labels=labels, want_trace=True))

    def sampled(tag, b, phi, X, ystar, refs):
        """mes_pool, jes_pool, gumbel_pool and the batch's kind of thompson_pool on one problem"""
        put(f"mes/{tag}", gp_ops.mes_pool(b, phi, X, ystar=ystar, topk=8, want_score=True))
        wide = (ystar[:, :1] - torch.linspace(0.0, 0.7, 8, device=dev)[None]).contiguous()
        put(f"jes/{tag}", gp_ops.jes_pool(b, phi, X, opt_idx=refs[:, :8].contiguous(), opt_val=wide, topk=8, want_score=True))
        put(f"gumbel/{tag}", gp_ops.gumbel_pool(b, phi, X, u=torch.linspace(0.05, 0.95, 5, device=dev).repeat(b.T, 1)))
        omega, phase = gp_ops.rff_basis(b.kernel, b.d, 64, generator=torch.Generator().manual_seed(11), device=dev)
        draw = gp_ops.thompson_pool_ard if b.ard else gp_ops.thompson_pool
        put(f"thompson/{tag}", draw(b, phi, X, omega=omega, phase=phase, n_samples=4, generator=torch.Generator().manual_seed(12), want_paths=True))
        for S, m in ((64, 128), (37, 256)):   # a full and a partial sample block, more features, both senses
            om, ph = gp_ops.rff_basis(b.kernel, b.d, m, generator=torch.Generator().manual_seed(11), device=dev)
            for mx in (False, True):
                put(f"thompson/{tag}/S={S}/m={m}/maximize={mx}", draw(b, phi, X, omega=om, phase=ph, n_samples=S, maximize=mx,
                                                                  generator=torch.Generator().manual_seed(12), want_paths=True))
        if have_qei:
            put(f"qei/{tag}", gp_ops.qei_pool(b, phi, X, omega=omega, phase=phase, n_samples=80, q=4, generator=torch.Generator().manual_seed(13),
                                              want_trace=True, want_inc=True))

    for kernel, n_s, d, rows, q in (("matern", [48, 45, 31], 16, 300, 8), ("rbf", [200, 197, 133], 64, 333, 8), ("matern", [1024, 700], 12, 130, 4)):
        b, phi, Zs, ys, n_s, X, best = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
        ystar = (ys.min(1).values[:, None] - torch.linspace(0.1, 1.0, 5)[None]).to(dev).contiguous()
        for log in (False, True):
            put(f"believer/{kernel}{max(n_s)}/log_ei={log}", gp_ops.believer_pool(b, phi, X, best_f=best.to(dev), q=q, log_ei=log, want_trace=True))
        put(f"gibbon/{kernel}{max(n_s)}", gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=q, want_trace=True))
        liar(f"{kernel}{max(n_s)}", b, phi, X, best.to(dev), q)
        put(f"predict_pool/{kernel}{max(n_s)}", gp_ops.predict_pool(b, phi, X, best_f=best.to(dev), topk=8, log_ei=True))
        refs = kg_refs(b, phi, X)
        for log in (False, True):
            put(f"kg/{kernel}{max(n_s)}/log={log}", gp_ops.kg_pool(b, phi, X, ref_idx=refs, log=log, topk=8, want_cov=True))
        sampled(f"{kernel}{max(n_s)}", b, phi, X, ystar, refs)
    b, phi, Zs, ys, n_s, X, best = BVA._explicit(dev, "matern", [48, 45, 31], 12, 300, 548)
    put("believer_ard", gp_ops.believer_pool_ard(b, phi, X, best_f=best.to(dev), q=8, want_trace=True))
    liar("ard", b, phi, X, best.to(dev), 8)
    put("kg_ard", gp_ops.kg_pool(b, phi, X, ref_idx=kg_refs(b, phi, X), log=True, topk=8, want_cov=True))
    sampled("ard", b, phi, X, (ys.min(1).values[:, None] - torch.linspace(0.1, 1.0, 5)[None]).to(dev).contiguous(), kg_refs(b, phi, X))
    b, phi, Zs, ys, n_s, _ = P._ill_batch(dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.cat([P._pool(300, 2, 3), b.Z_s[1, :5].cpu()]).to(dev)
    best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(len(n_s))], device=dev)
    put("float64/believer", gp_ops.believer_pool(b, phi, X, best_f=best, q=6, want_trace=True))
    liar("float64", b, phi, X, best, 6)
    for log in (False, True):
        put(f"float64/kg/log={log}", gp_ops.kg_pool(b, phi, X, ref_idx=kg_refs(b, phi, X), log=log, topk=8, want_cov=True))
    put("float64/gibbon", gp_ops.gibbon_pool(b, phi, X, ystar=(best[:, None] - torch.tensor([[1.0, 2.0]], device=dev)).contiguous(), q=6, want_trace=True))
    sampled("float64", b, phi, X, (best[:, None] - torch.tensor([[1.0, 2.0]], device=dev)).contiguous(), kg_refs(b, phi, X))
    b, phi, Zs, ys, n_s, X, best = BVA._f64_batch(dev)   # ARD, every task flagged: the <true> instances of the float64 walks
    best = best.to(dev)
    ystar = (best[:, None] - torch.tensor([[1.0, 2.0]], device=dev)).contiguous()
    put("float64_ard/believer", gp_ops.believer_pool_ard(b, phi, X, best_f=best, q=6, want_trace=True))
    liar("float64_ard", b, phi, X, best, 6)
    for log in (False, True):
        put(f"float64_ard/kg/log={log}", gp_ops.kg_pool(b, phi, X, ref_idx=kg_refs(b, phi, X), log=log, topk=8, want_cov=True))
    put("float64_ard/gibbon", gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=6, want_trace=True))
    sampled("float64_ard", b, phi, X, ystar, kg_refs(b, phi, X))
    import test_gpu_ehvi_pool as EV
    from test_ehvi_pool_cpu import GPU_CASES

    for case in range(len(GPU_CASES)):
        b, phi, X, grp, _, _ = EV._built_case(dev, case)
        free = dict(grp, C=0, con=None, con_thr=None, con_geq=None)
        for log in (False, True):
            put(f"ehvi/case{case}/log={log}", EV._call(b, phi, X, grp, log=log, topk=8, want_score=True, want_stair=True))
            if grp["C"] > 0:
                put(f"ehvi/case{case}/log={log}/C=0", EV._call(b, phi, X, free, log=log, topk=8, want_score=True))
    import numpy as np

    from adkf_ift_amd import bayes_opt as BO

    g = torch.Generator().manual_seed(3)
    Xb = torch.randn(400, 6, generator=g)
    yb = torch.stack([((Xb - 0.3) ** 2).sum(1), ((Xb + 0.4) ** 2).sum(1)], 1)
    order = torch.argsort(yb[:, 0])
    Xb, yb = Xb[order].to(dev), yb[order].to(dev)
    args = (4, 2, 2, "matern", dev, 200, 0.01, True)
    rngs = lambda: [np.random.default_rng(40 + r) for r in range(3)]
    runs = {"ei": (BO.run_gp_ei_bo_batched, {}), "ei_believer": (BO.run_gp_ei_bo_batched, dict(batch="believer")),
            "ei_ard": (BO.run_gp_ei_bo_batched, dict(ard=True, acquisition="log_ei")), "ts": (BO.run_gp_ts_bo_batched, dict(n_features=64)),
            "mes": (BO.run_gp_mes_bo_batched, dict(n_features=64)), "mes_gumbel": (BO.run_gp_mes_bo_batched, dict(max_value="gumbel")),
            "mes_gibbon": (BO.run_gp_mes_bo_batched, dict(n_features=64, batch="gibbon")), "kg": (BO.run_gp_kg_bo_batched, {}),
            "jes": (BO.run_gp_jes_bo_batched, dict(n_features=64))}
    for tag, (loop, kw) in runs.items():
        out[f"records/{tag}"] = torch.tensor(loop(Xb, yb[:, 0].contiguous(), *args, rngs=rngs(), **kw), dtype=torch.int64)
    rec, hv = BO.run_gp_ehvi_bo_batched(Xb, yb, *args, rngs=rngs(), maximize=(False, False))
    out["records/ehvi"] = torch.tensor(rec, dtype=torch.int64)
    out["records/ehvi_hypervolume"] = torch.tensor(hv, dtype=torch.float64)
    torch.save(out, path)
    print("saved", len(out), "arrays to", path)


def compare(pa, pb):
    import torch

    a, b = torch.load(pa), torch.load(pb)
    both = [k for k in a if k in b]
    if len(both) != len(a) or len(both) != len(b):   # calls one of the trees does not have: compared on the arrays both have
        print("arrays in one file only:", len(set(a) ^ set(b)), "with prefixes", sorted({k.split("/")[0] for k in set(a) ^ set(b)}))
    if not both:
        print("no array in common")
        return 1
    bad = [k for k in both if a[k].shape != b[k].shape or not torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8))]
    print("arrays compared", len(both), "different", bad)
    by_call = {}
    for k in both:
        by_call[k.split("/")[0]] = by_call.get(k.split("/")[0], 0) + 1
    print("per call:", ", ".join(f"{c} {n}" for c, n in sorted(by_call.items())))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
