"""Bitwise comparison of the pool calls between two builds of the library (a refactoring must return the other build's bits).

    python tools/pool_bits.py dump OUT.pt        in each of the two trees (each with its own built library), on the GPU
    python tools/pool_bits.py compare A.pt B.pt  exit status 1 and the names of the arrays that differ, if any

dump runs, on the problems of the GPU tests (tests/test_gpu_believer_pool._explicit: plain at 48 points, refined at 200, global slots
at 1024; the ARD problem of tests/test_gpu_believer_pool_ard; tests/test_gpu_predict_pool._ill_batch, whose flagged tasks take the
float64 walks): believer_pool with EI and with log EI and gibbon_pool, each with trace, predict_pool(log EI, k = 8), believer_pool_ard,
kg_pool with KG and with log KG (score, cov, ref_mean and the selection; M = 16 reference rows of lowest posterior mean, a -1 and a
repetition among them), and ehvi_pool on the problems of tests/test_gpu_ehvi_pool.py's score test (score, staircase and selection, linear
and log, with and without the constraints) - and saves every returned tensor.  compare looks at the arrays both files have, so a
tree can be held against one from before a call existed.  All lists are full (pools of 130 to 333 rows), so the arrays do not depend on how a short list is
merged."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(path):
    import torch

    import test_gpu_believer_pool as BV
    import test_gpu_believer_pool_ard as BVA
    import test_gpu_predict_pool as P
    from adkf_ift_amd import gp_ops

    dev = torch.device("cuda:0")
    out = {}

    def put(tag, o):
        for k, v in o.items():
            if torch.is_tensor(v):
                out[f"{tag}/{k}"] = v.cpu()

    def kg_refs(b, phi, X):
        refs = gp_ops.predict_pool(b, phi, X, topk=16, score="mean", want_mean=False, want_var=False, want_ei=False)["top_idx"].clone()
        refs[:, 4] = -1
        refs[:, 5] = refs[:, 0]
        return refs

    for kernel, n_s, d, rows, q in (("matern", [48, 45, 31], 16, 300, 8), ("rbf", [200, 197, 133], 64, 333, 8), ("matern", [1024, 700], 12, 130, 4)):
        b, phi, Zs, ys, n_s, X, best = BV._explicit(dev, kernel, n_s, d, rows, 500 + max(n_s))
        ystar = (ys.min(1).values[:, None] - torch.linspace(0.1, 1.0, 5)[None]).to(dev).contiguous()
        for log in (False, True):
            put(f"believer/{kernel}{max(n_s)}/log_ei={log}", gp_ops.believer_pool(b, phi, X, best_f=best.to(dev), q=q, log_ei=log, want_trace=True))
        put(f"gibbon/{kernel}{max(n_s)}", gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=q, want_trace=True))
        put(f"predict_pool/{kernel}{max(n_s)}", gp_ops.predict_pool(b, phi, X, best_f=best.to(dev), topk=8, log_ei=True))
        refs = kg_refs(b, phi, X)
        for log in (False, True):
            put(f"kg/{kernel}{max(n_s)}/log={log}", gp_ops.kg_pool(b, phi, X, ref_idx=refs, log=log, topk=8, want_cov=True))
    b, phi, Zs, ys, n_s, X, best = BVA._explicit(dev, "matern", [48, 45, 31], 12, 300, 548)
    put("believer_ard", gp_ops.believer_pool_ard(b, phi, X, best_f=best.to(dev), q=8, want_trace=True))
    put("kg_ard", gp_ops.kg_pool(b, phi, X, ref_idx=kg_refs(b, phi, X), log=True, topk=8, want_cov=True))
    b, phi, Zs, ys, n_s, _ = P._ill_batch(dev)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.cat([P._pool(300, 2, 3), b.Z_s[1, :5].cpu()]).to(dev)
    best = torch.tensor([float(ys[t, :n_s[t]].median()) for t in range(len(n_s))], device=dev)
    put("float64/believer", gp_ops.believer_pool(b, phi, X, best_f=best, q=6, want_trace=True))
    for log in (False, True):
        put(f"float64/kg/log={log}", gp_ops.kg_pool(b, phi, X, ref_idx=kg_refs(b, phi, X), log=log, topk=8, want_cov=True))
    put("float64/gibbon", gp_ops.gibbon_pool(b, phi, X, ystar=(best[:, None] - torch.tensor([[1.0, 2.0]], device=dev)).contiguous(), q=6, want_trace=True))
    import test_gpu_ehvi_pool as EV
    from test_ehvi_pool_cpu import GPU_CASES

    for case in range(len(GPU_CASES)):
        b, phi, X, grp, _, _ = EV._built_case(dev, case)
        free = dict(grp, C=0, con=None, con_thr=None, con_geq=None)
        for log in (False, True):
            put(f"ehvi/case{case}/log={log}", EV._call(b, phi, X, grp, log=log, topk=8, want_score=True, want_stair=True))
            if grp["C"] > 0:
                put(f"ehvi/case{case}/log={log}/C=0", EV._call(b, phi, X, free, log=log, topk=8, want_score=True))
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
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
