"""Bitwise comparison of the CPU twin (adkf_ift_amd/csrc/cpu/adkf_gp_cpu.cpp) between two builds of it: a refactoring of the twin must
return the other build's bits and the other build's return codes.  Host only; pool_bits.py is the sibling for the library.

    python tools/twin_bits.py dump OUT.pt        in each of the two trees (oracle/cpu_twin.build() compiles the tree's own twin)
    python tools/twin_bits.py compare A.pt B.pt  exit status 1 and the names of the arrays / return codes that differ, if any

dump calls every exported entry through oracle/cpu_twin.load() and adkf_ift_amd._lib.SIGNATURES (PARAMS below names the leading
parameters of each pool prototype; the trailing workspace / scratch / stream arguments are filled with NULL / 0) and saves every
output array, info and the return code.  The problems are those of tests/test_predict_pool_cpu._problem (T = 3, ns_max = 12, ragged
n_s, d = 5) with 97 pool rows, three of them planted duplicates: both kernels, isotropic and ARD, each as it is ("ok") and with a
NaN label in task 0 (NaN rows), task 1 at n_s = 0 and a NaN feature in task 2, whose factorisation fails ("edge": info != 0).  Per
entry: every combination of the flags it knows (the refused ones are recorded as return codes), k (or q) = 8 with every per-row output, k = 0 with per-row outputs, the selection alone, the
call without an exclusion list, rows = 0; the exclusion lists leave the last task (group) four eligible rows, fewer than k.  kg, ipv
and jes get a -1, a row outside the pool and a repeated row among their indices, ipv a zero weight, mes / gibbon / jes a non-finite
sample in task 0 of "ok", ehvi and mix a group with a task outside the batch.  The non-pool entries run through oracle/cpu_twin's wrappers.
Under rc/: for every pool entry the return code of each single fault - every pointer NULL, every count at -1, 0 and 100000, an
unknown flag, and the batch faults (a query set, a bad kernel, T = 0, no labels, no priors, the other kind of batch) - and of every
pair of a count at 100000 (ADKF_E_SIZE) with one of the ADKF_E_BADARG faults."""
import ctypes as C
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

POOL = "b phi flags X rows "
EXCL = "excl_idx excl_off "
TOPK = "k top_idx top_val info"
PARAMS = {
    "adkf_predict_marginal": "b phi flags X q_off rows best_f mean var ei info",
    "adkf_predict_marginal_ard": "b phi flags X q_off rows best_f mean var ei info",
    "adkf_predict_pool": POOL + "best_f " + EXCL + "mean var ei " + TOPK,
    "adkf_mes_pool": POOL + "ystar S " + EXCL + "score " + TOPK,
    "adkf_gumbel_pool": POOL + "u S ystar_out quant gumbel info",
    "adkf_thompson_pool": POOL + "omega phase m w eps S " + EXCL + "paths sel_idx sel_val info",
    "adkf_thompson_pool_ard": POOL + "omega phase m w eps S " + EXCL + "paths sel_idx sel_val info",
    "adkf_believer_pool": POOL + "best_f " + EXCL + "q trace sel_idx sel_val sel_mean sel_var info",
    "adkf_believer_pool_ard": POOL + "best_f " + EXCL + "q trace sel_idx sel_val sel_mean sel_var info",
    "adkf_gibbon_pool": POOL + "ystar S " + EXCL + "q trace sel_idx sel_val sel_mean sel_var info",
    "adkf_kg_pool": POOL + "ref_idx M " + EXCL + "score cov ref_mean " + TOPK,
    "adkf_ipv_pool": POOL + "ref_idx tgt_w M " + EXCL + "q trace sel_idx sel_val tvar info",
    "adkf_jes_pool": POOL + "ref_idx opt_val S cond_noise " + EXCL + "score opt_mean opt_var " + TOPK,
    "adkf_jackknife_pool": POOL + "alpha L " + EXCL + "lo hi loo_mean loo_var loo_lpd " + TOPK,
    "adkf_ehvi_pool": POOL + "G obj obj_max ref front front_n P con con_thr con_geq C " + EXCL + "score stair stair_n " + TOPK,
    "adkf_mix_pool": POOL + "G mem w M best_f " + EXCL + "mean var score " + TOPK,
}
# the flag bits each entry knows (include/adkf_gp.h): LATENT 1, MAXIMIZE 2, SCORE_MEAN 4, LOG_EI 16, SCORE_BALD 32, JK_SCALED 64
FLAGS = {"adkf_predict_marginal": (1, 2, 16), "adkf_predict_marginal_ard": (1, 2, 16), "adkf_predict_pool": (1, 2, 4, 16), "adkf_mes_pool": (2,),
         "adkf_gumbel_pool": (2,), "adkf_thompson_pool": (2,), "adkf_thompson_pool_ard": (2,), "adkf_believer_pool": (2, 16),
         "adkf_believer_pool_ard": (2, 16), "adkf_gibbon_pool": (2,), "adkf_kg_pool": (2, 16), "adkf_ipv_pool": (), "adkf_jes_pool": (2,),
         "adkf_jackknife_pool": (2, 64), "adkf_ehvi_pool": (16,), "adkf_mix_pool": (1, 2, 4, 16, 32)}
ROWS, K, S, M = 97, 8, 5, 6


def dump(path):
    import numpy as np
    import torch

    import test_predict_pool_cpu as P
    from adkf_ift_amd._lib import SIGNATURES
    from oracle import cpu_twin

    lib = cpu_twin.load()
    out = {}
    f32, i64, i32 = np.float32, np.int64, np.int32

    def call(name, kw, batch=None):
        """the entry on the named arguments (arrays, numbers, None), the rest of the prototype NULL / 0; returns the code"""
        types = SIGNATURES[name][1]
        names = PARAMS[name].split()
        args = []
        for i, ty in enumerate(types):
            v = kw.get(names[i]) if i < len(names) else None
            if i == 0:
                v = None if kw["b"] is None else C.byref(batch if batch is not None else kw["b"].c)
            elif isinstance(v, np.ndarray):
                v = v.ctypes.data
            elif v is None and ty is not C.c_void_p:
                v = 0
            args.append(v)
        return int(getattr(lib, name)(*args))

    def inputs(name, b, phi, X, best, rng, edge):
        """the named arguments of one full call: k (q) = 8, every output; the outputs start as NaN / -7, so what a call leaves is seen"""
        T, R = b.T, X.shape[0]
        G = 4 if name in ("adkf_ehvi_pool", "adkf_mix_pool") else T   # what the lists and the selection are counted in
        lists = [[3, 5, 50], []] + [[]] * (G - 3) + [sorted(set(range(R)) - {3, 10, 41, 60})]
        kw = dict(b=b, phi=phi, flags=0, X=X, rows=R, best_f=best, k=K, q=K, S=S, M=M, L=4, m=64, G=G, P=5, C=2, cond_noise=0.01,
                  excl_idx=np.array([i for l in lists for i in l if i < R], i64), excl_off=None, info=np.full(T, -7, i32))
        kw["excl_off"] = np.array([0] + list(np.cumsum([len([i for i in l if i < R]) for l in lists])), i64)
        kw["q_off"] = np.array([0, R // 3, R // 3, R], i64)
        ystar = (best[:, None] + rng.standard_normal((T, S))).astype(f32)
        kw["opt_val"] = ystar.copy()
        if not edge:
            ystar[0, 1] = np.inf; kw["opt_val"][0, 2] = np.nan   # a non-finite sample in task 0: NaN scores
        kw["ystar"] = ystar
        kw["u"] = rng.uniform(size=(T, S)).astype(f32)
        kw["omega"], kw["phase"] = rng.standard_normal((64, b.d)).astype(f32), rng.uniform(0, 6.28, 64).astype(f32)
        kw["w"], kw["eps"] = rng.standard_normal((T, S, 64)).astype(f32), rng.standard_normal((T, S, b.ns)).astype(f32)
        ref = rng.integers(0, max(R, 1), (T, M)).astype(i64)
        ref[:, 1] = -1; ref[:, 3] = ref[:, 0]; ref[:, 4] = R + 2   # a -1, a repetition, a row outside the pool
        kw["ref_idx"] = ref
        kw["tgt_w"] = np.abs(rng.standard_normal((T, M))).astype(f32)
        kw["tgt_w"][:, 2] = 0.0
        kw["alpha"] = np.array([0.1, 0.3, 0.0, 0.5], f32)
        if name == "adkf_ehvi_pool":
            kw.update(obj=np.array([[0, 1], [0, -1], [2, -1], [0, 7]], i32), obj_max=np.array([[0, 1], [1, 0], [0, 0], [0, 0]], i32),
                      ref=np.array([[1.5, -1.5], [-1.0, 0.0], [1.0, 0.0], [1.0, 1.0]], f32), front=rng.standard_normal((G, 5, 2)).astype(f32),
                      front_n=np.array([5, 3, 0, 2], i32), con=np.array([[2, -1], [1, 2], [-1, -1], [0, 1]], i32),
                      con_thr=rng.standard_normal((G, 2)).astype(f32), con_geq=np.array([[1, 0], [0, 1], [0, 0], [1, 1]], i32))
        if name == "adkf_mix_pool":
            kw.update(M=3, mem=np.array([[0, 1, 2], [0, -1, 0], [2, 2, -1], [0, 9, 1]], i32), w=np.abs(rng.standard_normal((G, 3))).astype(f32))
        fl = lambda *s: np.full(s, np.nan, f32)
        for o in ("mean", "var", "ei", "score"):
            kw[o] = fl(R) if name.startswith("adkf_predict_marginal") else fl(G, R)
        kw.update(top_idx=np.full((G, K), -7, i64), top_val=fl(G, K), sel_idx=np.full((T, max(K, S)), -7, i64), sel_val=fl(T, max(K, S)),
                  sel_mean=fl(T, K), sel_var=fl(T, K), trace=fl(T, K, R), tvar=fl(T, K + 1), paths=fl(T, S, R), ystar_out=fl(T, S),
                  quant=fl(T, 3), gumbel=fl(T, 2), cov=fl(T, R, M), ref_mean=fl(T, M), opt_mean=fl(T, S), opt_var=fl(T, S), lo=fl(T, 4, R),
                  hi=fl(T, 4, R), loo_mean=fl(T, b.ns), loo_var=fl(T, b.ns), loo_lpd=fl(T), stair=fl(G, 5, 2), stair_n=np.full(G, -7, i32))
        return {k: v for k, v in kw.items() if k in PARAMS[name].split()}

    INS = "b phi X best_f excl_idx excl_off q_off ystar opt_val u omega phase w eps ref_idx tgt_w alpha obj obj_max ref front front_n con con_thr con_geq mem".split()

    def record(tag, name, kw, batch=None):
        rc = call(name, kw, batch)
        out[f"rc/{tag}"] = torch.tensor(rc)
        for k, v in kw.items():
            if isinstance(v, np.ndarray) and k not in INS:
                out[f"{tag}/{k}"] = torch.from_numpy(v.copy())

    def problem(kind, ard, edge, rows=ROWS):
        b, Zs, ys, n_s, X, phi, best = P._problem(kind, ard, 70 + kind + 2 * ard, rows=max(rows, 1))
        X = X[:rows]
        if rows > 41:
            X[10] = X[3]; X[41] = X[3]; X[96 % rows] = X[20]   # exact duplicate rows: bit-equal scores
        if edge:
            b.y_s[0, 2] = np.nan; b.n_s[1] = 0; b.Z_s[2, 3, 0] = np.nan   # NaN rows, no points, info != 0 (the batch points at these arrays)
        return b, phi, X, best

    for name in PARAMS:
        ard_only, iso_only = name.endswith("_ard"), name in ("adkf_predict_marginal", "adkf_thompson_pool", "adkf_believer_pool")
        per_row = [p for p in ("mean", "var", "ei", "score", "trace", "paths", "cov", "ref_mean", "opt_mean", "opt_var", "lo", "hi", "loo_mean",
                               "loo_var", "loo_lpd", "stair", "stair_n", "sel_mean", "sel_var", "tvar", "quant", "gumbel") if p in PARAMS[name].split()]
        for kind, ard, edge in itertools.product((0, 1), (False, True), (False, True)):
            if (ard and iso_only) or (not ard and ard_only):
                continue
            tag = f"{name[5:]}/kind{kind}{'/ard' if ard else ''}/{'edge' if edge else 'ok'}"
            mk = lambda rows=ROWS: inputs(name, *problem(kind, ard, edge, rows), np.random.default_rng(5), edge)
            for r in range(len(FLAGS[name]) + 1):
                for bits in itertools.combinations(FLAGS[name], r):
                    record(f"{tag}/flags{sum(bits)}", name, dict(mk(), flags=sum(bits)))
            record(f"{tag}/rows0", name, mk(0))
            record(f"{tag}/no_excl", name, dict(mk(), excl_idx=None, excl_off=None))
            record(f"{tag}/no_per_row", name, dict(mk(), **{p: None for p in per_row}))
            record(f"{tag}/defaults", name, dict(mk(), **{p: None for p in ("tgt_w", "obj_max") + ("w",) * (name == "adkf_mix_pool")}, C=0))
            if "k" in PARAMS[name].split():
                record(f"{tag}/k0", name, dict(mk(), k=0, top_idx=None, top_val=None))
        # return codes of the refused calls, on the problem's first variant
        kind, ard = 1, ard_only
        tag = f"faults/{name[5:]}"
        types = SIGNATURES[name][1]
        mk = lambda: inputs(name, *problem(kind, ard, False), np.random.default_rng(5), False)
        code = lambda t, kw, batch=None: out.__setitem__(f"rc/{tag}/{t}", torch.tensor(call(name, kw, batch)))
        single = {"flags=1024": dict(flags=1024)}
        for i, p in enumerate(PARAMS[name].split()):
            if types[i] is C.c_void_p or i == 0:
                single[f"{p}=NULL"] = {p: None}
            elif p == "cond_noise":
                single.update({f"{p}={v}": {p: v} for v in (-1.0, float("nan"), float("inf"))})
            elif p != "flags":
                single.update({f"{p}={v}": {p: v} for v in (-1, 0, 100000) if not (v == 100000 and p in ("rows", "G"))})
        single.pop("excl_idx=NULL", None)   # (allowed)
        for t, over in single.items():
            code(t, dict(mk(), **over))

        def batch_with(**fields):
            kw = mk()
            c = type(kw["b"].c).from_buffer_copy(kw["b"].c)
            for f, v in fields.items():
                setattr(c, f, v)
            return kw, c

        held = np.zeros((3, 4, 5), f32)
        batches = {"nq_max=4": dict(nq_max=4, Z_q=held.ctypes.data), "kernel=7": dict(kernel=7), "T=0": dict(T=0), "y_s=NULL": dict(y_s=None),
                   "priors=NULL": dict(priors=None), "Z_s=NULL": dict(Z_s=None)}
        if ard_only or iso_only:
            batches["other_kind"] = dict(flags=0 if ard else 4)
        for t, fields in batches.items():
            code(t, *batch_with(**fields))
        for t, over in single.items():   # the pairs: a count beyond its maximum with a fault of the other code
            if not t.endswith("=100000"):
                continue
            for t2 in ("rows=-1", "flags=1024", "X=NULL", "info=NULL", "excl_off=NULL", "phi=NULL", "k=-1", "q=0", "top_idx=NULL", "sel_idx=NULL"):
                if t2 in single and t2.split("=")[0] != t.split("=")[0]:
                    code(f"{t}+{t2}", dict(mk(), **over, **single[t2]))
            for t2 in ("nq_max=4", "priors=NULL"):
                kw, c = batch_with(**batches[t2])
                code(f"{t}+{t2}", dict(kw, **over), c)

    # the entries outside the pool family, through oracle/cpu_twin's wrappers, and the scalar ones
    g = torch.Generator().manual_seed(9)
    T, ns, nq, d = 3, 12, 7, 5
    Zs, Zq = torch.randn(T, ns, d, generator=g).numpy(), torch.randn(T, nq, d, generator=g).numpy()
    ys, yq = torch.randn(T, ns, generator=g).numpy(), torch.randn(T, nq, generator=g).numpy()
    for kind, edge in itertools.product((0, 1), (False, True)):
        tag = f"gp/kind{kind}/{'edge' if edge else 'ok'}"
        y = ys.copy()
        if edge:
            y[2, 3] = np.nan
        n_s = np.array([12, 7, 10], i32)
        phi0, pri, l0 = cpu_twin.init_params(Zs, n_s=n_s)
        b = cpu_twin.CpuBatch(Zs, y, pri, kind, Z_q=Zq, y_q=yq, n_s=n_s, n_q=np.array([7, 4, 6], i32))
        b0 = cpu_twin.CpuBatch(Zs, y, pri, kind, n_s=n_s)
        l0m = np.empty(T, f32)
        out[f"rc/{tag}/median"] = torch.tensor(int(lib.adkf_median_lengthscale(C.byref(b0.c), l0m.ctypes.data, None, 0, None)))
        phi, *fit = cpu_twin.fit(b0, phi0, 40)
        res = dict(phi0=phi0, pri=pri, l0=l0, l0m=l0m, phi=phi, **{f"fit{i}": a for i, a in enumerate(fit)})
        res.update({f"mll{i}": a for i, a in enumerate(cpu_twin.mll_value_grad(b0, phi))})
        res.update({f"predict{i}": a for i, a in enumerate(cpu_twin.predict(b, phi, want_cov=True))})
        res.update({f"outer{i}": a for i, a in enumerate(cpu_twin.outer_nll_value_grad(b, phi))})
        for flags in (0, 1, 2, 3):
            res.update({f"ift{flags}_{k}": a for k, a in cpu_twin.ift_hypergrad(b, phi, flags).items()})
        out.update({f"{tag}/{k}": torch.from_numpy(np.ascontiguousarray(a)) for k, a in res.items()})
    for name, (res, types) in SIGNATURES.items():
        if hasattr(lib, name) and res is C.c_size_t:
            out[f"rc/scalar/{name}"] = torch.tensor(int(getattr(lib, name)(*([3] * len(types)))))
    out["rc/scalar/adkf_max_points"] = torch.tensor(int(lib.adkf_max_points()))
    torch.save(out, path)
    print("saved", sum(not k.startswith("rc/") for k in out), "arrays and", sum(k.startswith("rc/") for k in out), "return codes to", path)


def compare(pa, pb):
    import torch

    a, b = torch.load(pa), torch.load(pb)
    if set(a) != set(b):
        print("entries in one file only:", sorted(set(a) ^ set(b)))
        return 1
    same = lambda x, y: x.shape == y.shape and x.dtype == y.dtype and x.numpy().tobytes() == y.numpy().tobytes()
    arrays, codes = [k for k in a if not k.startswith("rc/")], [k for k in a if k.startswith("rc/")]
    bad_a, bad_c = [k for k in arrays if not same(a[k], b[k])], [k for k in codes if int(a[k]) != int(b[k])]
    print("arrays compared", len(arrays), "different", bad_a)
    print("return codes compared", len(codes), "different", bad_c)
    return 1 if bad_a or bad_c else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
