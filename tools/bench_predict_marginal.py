#!/usr/bin/env python
"""Streaming marginal prediction (adkf_predict_marginal) against the joint path (adkf_predict(want_var=True)) where the latter
accepts the shape.  Both are timed on the same work: from the features, with the fit's A^-1, alpha and scalars reused
(REUSE_INNER only), so each computes its own distances.  One JSON line per shape: rows/s, GB/s (query features read once plus
the outputs), the FLOP/s each path EXECUTES (its own count, below) with the marginal path's fractions of the FP32-matrix-pipe
bound (155 TFLOP/s) and of the HBM bound (6.29 TB/s), and the workspace bytes.  The last line runs the
tools/bench_meta_test.py shape through meta_test(streaming=True) and streaming=False.
--ard: the same shapes with ARD batches (adkf_predict_marginal_ard) at a per-dimension phi - the median-heuristic lengthscale
with a seeded +-30 % spread, evaluated once, then timed with REUSE_INNER - against isotropic streaming at the median lengthscale,
the two timed alternately in this process (median of --reps single calls each), and ARD adkf_predict(want_var=True) where its
workspace allows the shape.
--pool: shared-pool prediction (adkf_predict_pool) at T=16 ns=128 d=256, one pool of 262 144 rows, Matern, REUSE_INNER, EI:
(i) predict_pool writing mean, var and ei, (ii) predict_pool returning the 16 best rows per task and nothing per row, against
what the packed call offers for the same results: (iii) predict_marginal on the pool replicated T times, (iv) the same followed
by torch.topk over the [T, rows] view.  The four are timed alternately in this process (median of --reps single calls each) and
reported with the device memory each needs for the pool, the outputs and the scratch.  A second line times
run_gp_ei_bo_batched with 16 replicates against 16 sequential run_gp_ei_bo(streaming=True) runs (--skip-bo leaves it out).
--thompson: Thompson sampling over the same pool (adkf_thompson_pool, S = 16 samples, m = 1024 features, paths = NULL) timed
alternately with variant (ii) above in this process (median of --reps single calls each; use --reps 9).  S conditioned picks cost S
passes of (ii) with the library as it stands, so the line carries thompson_s < S * ii_pool_topk_s as "beats_S_passes", the matrix
FLOP the call executes per (task, row) - 2 d m (X Omega^T, computed per task) + 2 m S + 2 d ns + 2 ns S - and its fraction of the
FP32-matrix bound.  --out FILE also writes the line to FILE.
--thompson --ard: the same shape for ARD batches (adkf_thompson_pool_ard): one ARD batch and one isotropic batch are fitted on
the same data, and the two Thompson calls (REUSE_INNER, paths = NULL) are timed alternately in this process (median of --reps
single calls each).  The line holds both times, their ratio, the float64-flagged tasks of each batch, the bit-equality of a
repeated ARD call and the distinct picks per task; exit status 1 if the ratio exceeds 1.15.
--believer: Kriging-believer batch selection (adkf_believer_pool, trace = NULL) at T=16 ns=128 d=256, one pool of 100 000 rows, q = 8,
Matern, REUSE_INNER, timed alternately in this process (median of --reps single calls each) with what a caller can do without it:
q calls of adkf_predict_pool(k = 1) on the same batch (which leaves out the refit such a caller would also need).  The line holds
both times, their ratio against the estimate from the tile's products (1.5 at ns = 128), the scratch bytes, the bit-equality of step 0
with predict_pool and of a repeated call, and the picks shared with the EI top-q.
--believer --ard: the same shape for ARD batches (adkf_believer_pool_ard): one ARD batch and one isotropic batch are fitted on the
same data, and four calls (REUSE_INNER, trace = NULL) are timed alternately in this process (median of --reps single calls each;
use --reps 7): the ARD believer, the isotropic believer, ARD predict_pool(topk=1) and isotropic predict_pool(topk=1).  The yardstick
for the ARD believer's ratio to the isotropic one is predict_pool's ARD / isotropic ratio of the same run: the ARD walk adds one load
and one multiply per staged query element, and the believer adds nothing ARD-specific on top.  The line holds the four times, both
ratios, each series' spread (max - min) / median, the float64-flagged tasks of each batch, the bit-equality of step 0 with ARD
predict_pool and of a repeated call, and the distinct picks per task.
--mes: max-value entropy search (adkf_mes_pool, score = NULL, k = 8) at T=16 ns=128 d=256, one pool of 100 000 rows, Matern,
REUSE_INNER, for S = 1, 16 and 64 max-value samples, timed alternately in this process (median of --reps single calls each) with
adkf_predict_pool(k = 8, log EI, nothing per row) on the same fitted batch and pool: the same walk with one evaluation of the
bracket per row where MES makes S.  The line holds the four times, the ratio to the log-EI call per S, each series' spread
(max - min) / median and the bit-equality of a repeated call.  No target: the line is what says whether the S evaluations show.
--gibbon: GIBBON batch max-value entropy search (adkf_gibbon_pool, q = 8, S = 16, trace = NULL) on --mes's batch and pool (T=16 ns=128
d=256, 100 000 rows, Matern, REUSE_INNER), timed alternately in this process (median of --reps single calls each) with
adkf_believer_pool(q = 8, log EI) - the same q walks and downdate with one evaluation per row and step where GIBBON makes S - and
with q calls of adkf_mes_pool(S = 16, k = 8), the same S evaluations per row and walk without the downdate.  The line holds the
three times, both ratios, each series' spread (max - min) / median, the scratch bytes, the bit-equality of a repeated call and how
many picks each task's batch shares with its MES top-q.  No target.
--gumbel: Gumbel max-value sampling (adkf_gumbel_pool, S = 16 uniforms per task) on --mes's batch and pool (T=16 ns=128 d=256, 100 000
rows, Matern, REUSE_INNER), timed alternately in this process (median of --reps single calls each) with adkf_predict_pool(k = 8,
log EI, nothing per row) and with gp_ops.max_value_samples at S = 16, m = 1024 (w and eps already on the device).  The call is three
walks of the pool, each with an epilogue of 64 evaluations per row like MES at S = 64.  The line holds the three times, both
ratios, each series' spread (max - min) / median, the scratch bytes and the bit-equality of a repeated call.  No target.
--kg: knowledge-gradient selection (adkf_kg_pool, log KG, k = 8, nothing per row) on --mes's batch and pool (T=16 ns=128 d=256, 100 000
rows, Matern, REUSE_INNER) with M = 32 and M = 64 reference rows (each task's rows of lowest posterior mean, taken once, outside the
timing), timed alternately in this process (median of --reps single calls each) with adkf_predict_pool(k = 8, log EI, nothing per
row) - the same walk without the reference panel and the envelope - and with adkf_believer_pool(q = 8, log EI), eight walks whose
last carries a panel of 7 stored rows.  The line holds the four times, the ratios, each series' spread (max - min) / median, the
scratch bytes and the bit-equality of a repeated call.  No target.
--jes: joint entropy search (adkf_jes_pool, k = 8, nothing per row) on --mes's batch and pool (T=16 ns=128 d=256, 100 000 rows, Matern,
REUSE_INNER) with S = 16 and S = 64 optimum samples (one gp_ops.optimum_samples call per S at m = 1024, outside the timing), timed
alternately in this process (median of --reps single calls each) with adkf_kg_pool(log KG, k = 8) at M = S on the same rows - the same
reference panel followed by the envelope where JES makes S evaluations - with adkf_mes_pool(k = 8) on the same values - the same S
evaluations without the panel - and with adkf_predict_pool(k = 8, log EI, nothing per row).  The line holds the times, the ratios, each
series' spread (max - min) / median, the scratch bytes and the bit-equality of a repeated call.  No target.
--ipv: target-variance batch selection (adkf_ipv_pool, q = 16, no trace) at T=64 ns=128 d=64, 100 000 rows, Matern, REUSE_INNER, with
M = 16 and M = 48 random target rows per task, timed alternately in this process (median of --reps single calls each) with
adkf_believer_pool(q = 16, log EI): the same sixteen walks, whose panel has j columns at step j where this entry's has M + j, without
the j M multiply-adds a row.  The line holds the three times, the ratios, each series' spread (max - min) / median, the scratch
bytes and the bit-equality of a repeated call.  No target.
--ehvi: constrained EHVI across tasks (adkf_ehvi_pool, k = 8, nothing per row) on --mes's batch and pool: 8 two-objective groups
(2 g, 2 g + 1) with mixed senses, fronts of P points drawn around the support labels, in log form at P = 16 and P = 64, in linear form
at P = 16, and at P = 16 with C = 2 constraint tasks - random fronts, which clean down to a handful of steps - and on an anti-chain of
64 points, every one a step of the staircase (65 strips a row: the most there can be), in log form, in linear form and in log form
with C = 2, timed alternately in this process (median of --reps single calls each) with
adkf_predict_pool(latent, mean and var, no selection) - what its stage A runs per chunk - and adkf_predict_pool(k = 8, log EI,
nothing per row).  The line holds the times, the ratios, the share of stage A, each series' spread, the scratch bytes, the staircase
sizes and the bit-equality of a repeated call.  No target.
Usage: python tools/bench_predict_marginal.py [--reps 5] [--skip-meta-test] [--ard] [--skip-large] [--pool] [--skip-bo] [--thompson [--ard]] [--believer [--ard]] [--mes] [--gibbon] [--gumbel] [--kg] [--jes] [--ipv] [--ehvi] [--out FILE]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adkf_ift_amd import _lib, gp_ops

FP32_MFMA = 155e12
HBM = 6.29e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / 1e3 / reps


def _refined(b):
    """[T] bool: tasks that take the refined-C step (more than 128 points, or S_CONDA above 3: problems.h ProbCres's gate); the
    scalars sit in the support-only workspace after W_ss (carve() order of csrc/host_gp.h)."""
    return (_scal(b)[:, 47] > 3.0) | (b.ns > 128)


def flops_marginal(T, ns, d, rows, n_refined_rows):
    # support distances (upper tiles of the symmetric block) + per row: distances 2 ns d, C = K A^-1 2 ns^2, refined rows R 2 ns^2
    t = -(-ns // 64)
    return T * 64 * 64 * d * t * (t + 1) + rows * (2.0 * ns * d + 2.0 * ns * ns) + n_refined_rows * 2.0 * ns * ns


def flops_joint(T, ns, nq, d, n_refined_tasks):
    # adkf_predict: the support, query-support and query-query distance blocks (symmetric ones: upper tiles), C, and for
    # refined tasks ProbCres + ProbCfix
    ts, tq = -(-ns // 64), -(-nq // 64)
    return (T * 64 * 64 * d * (ts * (ts + 1) + tq * (tq + 1)) + T * 2.0 * nq * ns * d + T * 2.0 * nq * ns * ns
            + n_refined_tasks * 4.0 * nq * ns * ns)


def shape(T, ns, d, rows_per_task, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "rbf")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    refined = _refined(b)
    b.flags = gp_ops.REUSE_INNER
    rows = T * rows_per_task
    Zq = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):   # (a [rows, d] @ W product at once would need a second copy of the pool)
        Zq[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    q_off = torch.arange(T + 1, device=dev, dtype=torch.int64) * rows_per_task
    best = torch.zeros(T, device=dev)
    lib = _lib.load()
    rec = {"shape": f"T={T} ns={ns} d={d} rows/task={rows_per_task}", "rows": rows, "refined_tasks": int(refined.sum()),
           "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d))}
    byte_row = 4.0 * d + 12.0
    dt = timed(lambda: gp_ops.predict_marginal(b, phi, Zq, q_off, best_f=best), reps)
    fl = flops_marginal(T, ns, d, rows, int(refined.sum()) * rows_per_task)
    rec.update({"marginal_s": dt, "marginal_rows_per_s": rows / dt, "marginal_GB_per_s": rows * byte_row / dt / 1e9,
                "marginal_TFLOP_per_s": fl / dt / 1e12, "marginal_frac_fp32_mfma_bound": fl / dt / FP32_MFMA,
                "marginal_frac_hbm_bound": rows * byte_row / dt / HBM})
    if rows_per_task <= lib.adkf_max_points():
        # the same fitted parameters on a batch with the padded query set: A^-1, alpha and the scalars written into ITS workspace
        # by a fit from phi* (which stays put: converged), then timed with REUSE_INNER only - its distance stage runs
        bj = gp_ops.GPBatch(Zs, ys, b.priors, "rbf", Z_q=Zq.view(T, rows_per_task, d), y_q=torch.zeros(T, rows_per_task, device=dev))
        phij, _, _, _, info = gp_ops.fit(bj, phi, 200)
        gp_ops.check_info(info)
        rec["joint_fit_phi_max_abs_change"] = float((phij - phi).abs().max())
        bj.flags = gp_ops.REUSE_INNER
        dtj = timed(lambda: gp_ops.predict(bj, phij, want_var=True), reps)
        flj = flops_joint(T, ns, rows_per_task, d, int(refined.sum()))
        rec.update({"adkf_predict_s": dtj, "adkf_predict_rows_per_s": rows / dtj, "adkf_predict_TFLOP_per_s": flj / dtj / 1e12,
                    "adkf_predict_workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, rows_per_task, d)),
                    "speedup_vs_adkf_predict": dtj / dt})
    print(json.dumps(rec), flush=True)


def once(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / 1e3


def shape_ard(T, ns, d, rows_per_task, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    ba = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "rbf", ard=True)
    phi0, l0 = gp_ops.init_params_batch(ba, True, True)
    gs = torch.Generator().manual_seed(1)
    spread = 1.0 + 0.3 * (2.0 * torch.rand(T, d, generator=gs, dtype=torch.float64) - 1.0)
    phi = phi0.clone()
    phi[:, 2:] = torch.log(torch.expm1(l0.double().cpu()[:, None] * spread)).float().to(dev)
    bi = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "rbf")
    phii, _ = gp_ops.init_params_batch(bi, True, True)   # (noise, outputscale, the median lengthscale)
    rows = T * rows_per_task
    Zq = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        Zq[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    q_off = torch.arange(T + 1, device=dev, dtype=torch.int64) * rows_per_task
    best = torch.zeros(T, device=dev)
    lib = _lib.load()
    fa = lambda: gp_ops.predict_marginal(ba, phi, Zq, q_off, best_f=best)
    fi = lambda: gp_ops.predict_marginal(bi, phii, Zq, q_off, best_f=best)
    for b, f in ((ba, fa), (bi, fi)):   # evaluate at phi once; the timed calls reuse it
        b.flags = 0
        f()
        b.flags = gp_ops.REUSE_INNER
    torch.cuda.synchronize()
    ta, ti = [], []
    for _ in range(reps):
        ta.append(once(fa))
        ti.append(once(fi))
    dt, dti = float(np.median(ta)), float(np.median(ti))
    rec = {"shape": f"ARD T={T} ns={ns} d={d} rows/task={rows_per_task}", "rows": rows, "refined_tasks_ard": int(_refined(ba).sum()),
           "refined_tasks_isotropic": int(_refined(bi).sum()), "workspace_bytes_ard": int(lib.adkf_workspace_bytes_ard(T, ns, 0, d)),
           "workspace_bytes_isotropic": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "ard_s": dt, "isotropic_s": dti, "ard_over_isotropic": dt / dti, "ard_rows_per_s": rows / dt,
           "ard_s_all": ta, "isotropic_s_all": ti}
    if rows_per_task <= lib.adkf_max_points():
        bj = gp_ops.GPBatch(Zs, ys, ba.priors, "rbf", Z_q=Zq.view(T, rows_per_task, d), y_q=torch.zeros(T, rows_per_task, device=dev),
                            ard=True)
        _, _, _, info = gp_ops.predict(bj, phi, want_var=True)   # the inner quantities at phi into ITS workspace
        gp_ops.check_info(info)
        bj.flags = gp_ops.REUSE_INNER
        dtj = timed(lambda: gp_ops.predict(bj, phi, want_var=True), reps)
        rec.update({"ard_adkf_predict_s": dtj, "ard_adkf_predict_workspace_bytes": int(lib.adkf_workspace_bytes_ard(T, ns, rows_per_task, d)),
                    "speedup_vs_ard_adkf_predict": dtj / dt})
    print(json.dumps(rec), flush=True)


def shape_pool(T, ns, d, rows, k, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    Xrep = X.repeat(T, 1)   # what the packed layout needs: every task its own copy of the pool
    q_off = torch.arange(T + 1, device=dev, dtype=torch.int64) * rows
    f1 = lambda: gp_ops.predict_pool(b, phi, X, best_f=best)
    f2 = lambda: gp_ops.predict_pool(b, phi, X, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=k)
    f3 = lambda: gp_ops.predict_marginal(b, phi, Xrep, q_off, best_f=best)
    f4 = lambda: torch.topk(gp_ops.predict_marginal(b, phi, Xrep, q_off, best_f=best)[2].view(T, rows), k, dim=1)
    o1, o2, o3, o4 = f1(), f2(), f3(), f4()
    torch.cuda.synchronize()
    same_rows = all(torch.equal(o1[n].view(-1), o3[j]) for j, n in enumerate(("mean", "var", "ei")))
    same_top = torch.equal(o2["top_val"], o4.values)   # (torch.topk does not promise an order among equal values: compare the values)
    ts = [[], [], [], []]
    for _ in range(reps):
        for q, f in enumerate((f1, f2, f3, f4)):
            ts[q].append(once(f))
    m = [float(np.median(x)) for x in ts]
    lib = _lib.load()
    pool_b, out_b = 4 * rows * d, 3 * 4 * T * rows
    rec = {"shape": f"pool T={T} ns={ns} d={d} rows={rows} k={k} matern REUSE_INNER EI", "refined_tasks": int(_refined(b).sum()),
           "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "i_pool_rows_s": m[0], "ii_pool_topk_s": m[1], "iii_packed_replicated_s": m[2], "iv_packed_replicated_topk_s": m[3],
           "i_over_iii": m[0] / m[2], "ii_over_iv": m[1] / m[3], "task_rows_per_s_i": T * rows / m[0], "task_rows_per_s_ii": T * rows / m[1],
           "i_bytes": pool_b + out_b, "ii_bytes": pool_b + int(lib.adkf_predict_pool_scratch_bytes(T, k)) + T * k * 12,
           "iii_bytes": T * pool_b + out_b, "iv_bytes": T * pool_b + out_b + T * k * 12,
           "pool_equals_packed_bitwise": bool(same_rows), "topk_values_equal": bool(same_top), "all_s": ts}
    print(json.dumps(rec), flush=True)


def shape_thompson(T, ns, d, rows, S, m, reps, dev, out_path=None):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    gc = torch.Generator().manual_seed(1)
    omega, phase = gp_ops.rff_basis("matern", d, m, generator=gc, device=dev)
    w, eps = torch.randn(T, S, m, generator=gc).to(dev), torch.randn(T, S, ns, generator=gc).to(dev)
    f_ts = lambda: gp_ops.thompson_pool(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps)
    f_ii = lambda: gp_ops.predict_pool(b, phi, X, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=16)
    o1, o2 = f_ts(), f_ts()
    f_ii()
    torch.cuda.synchronize()
    gp_ops.check_info(o1["info"])
    ts = [[], []]
    for _ in range(reps):
        ts[0].append(once(f_ts))
        ts[1].append(once(f_ii))
    t_ts, t_ii = float(np.median(ts[0])), float(np.median(ts[1]))
    lib = _lib.load()
    fl = T * rows * (2.0 * d * m + 2.0 * m * S + 2.0 * d * ns + 2.0 * ns * S)
    fl_ii = T * rows * (2.0 * d * ns + 2.0 * ns * ns)
    rec = {"shape": f"thompson T={T} ns={ns} d={d} rows={rows} S={S} m={m} matern REUSE_INNER paths=NULL", "design": "X Omega^T per task (not shared)",
           "float64_tasks": int((_scal(b)[:, 45] > 30.0).sum()), "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "scratch_bytes": int(lib.adkf_thompson_pool_scratch_bytes(T, ns, S, m)),
           "thompson_s": t_ts, "ii_pool_topk_s": t_ii, "thompson_over_ii": t_ts / t_ii, "S_times_ii_s": S * t_ii, "beats_S_passes": bool(t_ts < S * t_ii),
           "matrix_flop_over_ii": fl / fl_ii, "thompson_TFLOP_per_s": fl / t_ts / 1e12, "thompson_frac_fp32_mfma_bound": fl / t_ts / 157.3e12,
           "cosines_per_s": T * rows * float(m) / t_ts, "distinct_picks_per_task_min": int(min(len(set(r)) for r in o1["sel_idx"].cpu().tolist())),
           "repeat_is_bit_equal": bool(torch.equal(o1["sel_idx"], o2["sel_idx"]) and torch.equal(o1["sel_val"], o2["sel_val"])), "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def shape_thompson_ard(T, ns, d, rows, S, m, reps, dev, out_path=None):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    bi = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(bi, True, True)
    bi.flags = gp_ops.REUSE_DIST
    phi_i, _, _, _, info = gp_ops.fit(bi, phi0, 200)
    gp_ops.check_info(info)
    bi.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    ba = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern", ard=True)
    phi0, _ = gp_ops.init_params_batch(ba, True, True)
    phi_a, _, _, n_evals, info = gp_ops.fit(ba, phi0, 100)
    gp_ops.check_info(info)
    ba.flags = gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    gc = torch.Generator().manual_seed(1)
    omega, phase = gp_ops.rff_basis("matern", d, m, generator=gc, device=dev)
    w, eps = torch.randn(T, S, m, generator=gc).to(dev), torch.randn(T, S, ns, generator=gc).to(dev)
    kw = dict(omega=omega, phase=phase, n_samples=S, w=w, eps=eps)
    f_a = lambda: gp_ops.thompson_pool_ard(ba, phi_a, X, **kw)
    f_i = lambda: gp_ops.thompson_pool(bi, phi_i, X, **kw)
    o1, o2 = f_a(), f_a()
    oi = f_i()
    torch.cuda.synchronize()
    gp_ops.check_info(o1["info"]); gp_ops.check_info(oi["info"])
    ts = [[], []]
    for _ in range(reps):
        ts[0].append(once(f_a))
        ts[1].append(once(f_i))
    t_a, t_i = float(np.median(ts[0])), float(np.median(ts[1]))
    lib = _lib.load()
    ell = torch.nn.functional.softplus(phi_a[:, 2:])
    rec = {"shape": f"thompson ard T={T} ns={ns} d={d} rows={rows} S={S} m={m} matern REUSE_INNER paths=NULL",
           "float64_tasks_ard": int((_scal(ba)[:, 45] > 30.0).sum()), "float64_tasks_isotropic": int((_scal(bi)[:, 45] > 30.0).sum()),
           "workspace_bytes_ard": int(lib.adkf_workspace_bytes_ard(T, ns, 0, d)), "workspace_bytes_isotropic": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "scratch_bytes": int(lib.adkf_thompson_pool_scratch_bytes(T, ns, S, m)),
           "ard_fit_evals_max": int(n_evals.max()), "ard_lengthscale_min": float(ell.min()), "ard_lengthscale_max": float(ell.max()),
           "thompson_ard_s": t_a, "thompson_isotropic_s": t_i, "ard_over_isotropic": t_a / t_i, "within_1_15": bool(t_a <= 1.15 * t_i),
           "distinct_picks_per_task_min_ard": int(min(len(set(r)) for r in o1["sel_idx"].cpu().tolist())),
           "distinct_picks_per_task_min_isotropic": int(min(len(set(r)) for r in oi["sel_idx"].cpu().tolist())),
           "repeat_is_bit_equal": bool(torch.equal(o1["sel_idx"], o2["sel_idx"]) and torch.equal(o1["sel_val"], o2["sel_val"])), "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def shape_believer(T, ns, d, rows, q, reps, dev, out_path=None):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    top1 = lambda: gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=1)
    f_bv = lambda: gp_ops.believer_pool(b, phi, X, best_f=best, q=q)
    f_q = lambda: [top1() for _ in range(q)]
    o1, o2 = f_bv(), f_bv()
    ref = top1()
    topq = gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=q)
    torch.cuda.synchronize()
    gp_ops.check_info(o1["info"])
    ts = [[], [], []]
    for _ in range(reps):
        ts[0].append(once(f_bv))
        ts[1].append(once(f_q))
        ts[2].append(once(top1))
    t_bv, t_q, t_1 = (float(np.median(x)) for x in ts)
    lib = _lib.load()
    shared = [len(set(a) & set(c)) for a, c in zip(o1["sel_idx"].cpu().tolist(), topq["top_idx"].cpu().tolist())]
    rec = {"shape": f"believer T={T} ns={ns} d={d} rows={rows} q={q} matern REUSE_INNER trace=NULL", "refined_tasks": int(_refined(b).sum()),
           "float64_tasks": int((_scal(b)[:, 45] > 30.0).sum()), "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "scratch_bytes": int(lib.adkf_believer_pool_scratch_bytes(T, ns, d, q)),
           "believer_s": t_bv, "q_calls_of_predict_pool_k1_s": t_q, "one_predict_pool_k1_s": t_1, "believer_over_q_calls": t_bv / t_q,
           "step_over_one_pass": t_bv / (q * t_1), "estimate_step_over_one_pass": 1.5,
           "step_0_is_predict_pool_bitwise": bool(torch.equal(o1["sel_idx"][:, 0], ref["top_idx"][:, 0]) and torch.equal(o1["sel_val"][:, 0], ref["top_val"][:, 0])),
           "repeat_is_bit_equal": bool(all(torch.equal(o1[n], o2[n]) for n in ("sel_idx", "sel_val", "sel_mean", "sel_var"))),
           "distinct_picks_per_task_min": int(min(len(set(r)) for r in o1["sel_idx"].cpu().tolist())),
           "picks_shared_with_ei_top_q_per_task": shared, "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def shape_mes(T, ns, d, rows, k, reps, dev, out_path=None):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    f_lei = lambda: gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=k, log_ei=True)
    Ss = (1, 16, 64)
    # samples of min f: below the smallest label, spread over one prior standard deviation
    ystar = {S: (ys.min(1).values[:, None] - torch.rand(T, S, device=dev, generator=g)).contiguous() for S in Ss}
    f_mes = {S: (lambda S=S: gp_ops.mes_pool(b, phi, X, ystar=ystar[S], topk=k)) for S in Ss}
    o1, o2 = f_mes[16](), f_mes[16]()
    f_lei()
    torch.cuda.synchronize()
    gp_ops.check_info(o1["info"])
    ts = {"log_ei": [], **{f"mes_S{S}": [] for S in Ss}}
    for _ in range(reps):
        ts["log_ei"].append(once(f_lei))
        for S in Ss:
            ts[f"mes_S{S}"].append(once(f_mes[S]))
    med = {n: float(np.median(x)) for n, x in ts.items()}
    lib = _lib.load()
    rec = {"shape": f"mes T={T} ns={ns} d={d} rows={rows} k={k} matern REUSE_INNER score=NULL", "refined_tasks": int(_refined(b).sum()),
           "float64_tasks": int((_scal(b)[:, 45] > 30.0).sum()), "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "scratch_bytes": int(lib.adkf_predict_pool_scratch_bytes(T, k)),
           "predict_pool_log_ei_s": med["log_ei"], **{f"mes_S{S}_s": med[f"mes_S{S}"] for S in Ss},
           **{f"mes_S{S}_over_log_ei": med[f"mes_S{S}"] / med["log_ei"] for S in Ss},
           "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()},
           "repeat_is_bit_equal": bool(torch.equal(o1["top_idx"], o2["top_idx"]) and torch.equal(o1["top_val"], o2["top_val"])),
           "all_selected": bool((o1["top_idx"] >= 0).all() and torch.isfinite(o1["top_val"]).all()), "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def shape_gumbel(T, ns, d, rows, k, S, m, reps, dev, out_path=None):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    u = torch.rand(T, S, device=dev, generator=g)
    omega, phase = gp_ops.rff_basis("matern", d, m, generator=torch.Generator().manual_seed(0), device=dev)
    w, eps = torch.randn(T, S, m, device=dev, generator=g), torch.randn(T, S, ns, device=dev, generator=g)
    f_lei = lambda: gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=k, log_ei=True)
    f_gb = lambda: gp_ops.gumbel_pool(b, phi, X, u=u)
    f_mv = lambda: gp_ops.max_value_samples(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps)
    o1, o2 = f_gb(), f_gb()
    f_lei(); f_mv()
    torch.cuda.synchronize()
    gp_ops.check_info(o1["info"])
    ts = {"log_ei": [], "gumbel": [], "max_value_samples": []}
    for _ in range(reps):
        ts["log_ei"].append(once(f_lei))
        ts["gumbel"].append(once(f_gb))
        ts["max_value_samples"].append(once(f_mv))
    med = {n: float(np.median(x)) for n, x in ts.items()}
    lib = _lib.load()
    same = lambda x, y: bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
    rec = {"shape": f"gumbel T={T} ns={ns} d={d} rows={rows} S={S} matern REUSE_INNER; predict_pool k={k} log EI; max_value_samples m={m}",
           "refined_tasks": int(_refined(b).sum()), "float64_tasks": int((_scal(b)[:, 45] > 30.0).sum()),
           "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d)), "scratch_bytes": int(lib.adkf_gumbel_pool_scratch_bytes(T)),
           "thompson_scratch_bytes": int(lib.adkf_thompson_pool_scratch_bytes(T, ns, S, m)),
           "predict_pool_log_ei_s": med["log_ei"], "gumbel_s": med["gumbel"], "max_value_samples_s": med["max_value_samples"],
           "gumbel_over_log_ei": med["gumbel"] / med["log_ei"], "gumbel_over_max_value_samples": med["gumbel"] / med["max_value_samples"],
           "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()},
           "repeat_is_bit_equal": all(same(o1[n], o2[n]) for n in ("ystar", "quant", "gumbel")),
           "all_finite": bool(torch.isfinite(o1["ystar"]).all()), "gumbel_b_range": [float(o1["gumbel"][:, 1].min()), float(o1["gumbel"][:, 1].max())],
           "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def shape_kg(T, ns, d, rows, k, Ms, reps, dev, out_path=None):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    refs = {M: gp_ops.predict_pool(b, phi, X, topk=M, score="mean", want_mean=False, want_var=False, want_ei=False)["top_idx"] for M in Ms}
    f_lei = lambda: gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=k, log_ei=True)
    f_bv = lambda: gp_ops.believer_pool(b, phi, X, best_f=best, q=k, log_ei=True)
    f_kg = {M: (lambda M=M: gp_ops.kg_pool(b, phi, X, ref_idx=refs[M], log=True, topk=k, want_score=False)) for M in Ms}
    o1 = {M: f_kg[M]() for M in Ms}
    o2 = {M: f_kg[M]() for M in Ms}
    f_lei(); f_bv()
    torch.cuda.synchronize()
    for M in Ms:
        gp_ops.check_info(o1[M]["info"])
    ts = {"log_ei": [], "believer_log_ei": [], **{f"kg_M{M}": [] for M in Ms}}
    for _ in range(reps):
        ts["log_ei"].append(once(f_lei))
        ts["believer_log_ei"].append(once(f_bv))
        for M in Ms:
            ts[f"kg_M{M}"].append(once(f_kg[M]))
    med = {n: float(np.median(x)) for n, x in ts.items()}
    lib = _lib.load()
    rec = {"shape": f"kg T={T} ns={ns} d={d} rows={rows} k={k} log KG matern REUSE_INNER score=NULL; predict_pool k={k} log EI; believer q={k} log EI",
           "refined_tasks": int(_refined(b).sum()), "float64_tasks": int((_scal(b)[:, 45] > 30.0).sum()),
           "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "scratch_bytes": {str(M): int(lib.adkf_kg_pool_scratch_bytes(T, ns, d, M, k)) for M in Ms},
           "predict_pool_log_ei_s": med["log_ei"], "believer_log_ei_s": med["believer_log_ei"],
           "kg_s": {str(M): med[f"kg_M{M}"] for M in Ms},
           "kg_over_log_ei": {str(M): med[f"kg_M{M}"] / med["log_ei"] for M in Ms},
           "kg_over_believer": {str(M): med[f"kg_M{M}"] / med["believer_log_ei"] for M in Ms},
           "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()},
           "repeat_is_bit_equal": bool(all(torch.equal(o1[M]["top_idx"], o2[M]["top_idx"]) and
                                           torch.equal(o1[M]["top_val"].view(torch.int32), o2[M]["top_val"].view(torch.int32)) for M in Ms)),
           "all_selected": bool(all((o1[M]["top_idx"] >= 0).all() and torch.isfinite(o1[M]["top_val"]).all() for M in Ms)),
           "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def shape_ipv(T, ns, d, rows, q, Ms, reps, dev, out_path=None):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    tg = {M: torch.stack([torch.randperm(rows, device=dev, generator=g)[:M] for _ in range(T)]) for M in Ms}
    f_bv = lambda: gp_ops.believer_pool(b, phi, X, best_f=best, q=q, log_ei=True)
    f_ipv = {M: (lambda M=M: gp_ops.ipv_pool(b, phi, X, targets=tg[M], q=q)) for M in Ms}
    o1 = {M: f_ipv[M]() for M in Ms}
    o2 = {M: f_ipv[M]() for M in Ms}
    f_bv()
    torch.cuda.synchronize()
    for M in Ms:
        gp_ops.check_info(o1[M]["info"])
    ts = {"believer_log_ei": [], **{f"ipv_M{M}": [] for M in Ms}}
    for _ in range(reps):
        ts["believer_log_ei"].append(once(f_bv))
        for M in Ms:
            ts[f"ipv_M{M}"].append(once(f_ipv[M]))
    med = {n: float(np.median(x)) for n, x in ts.items()}
    lib = _lib.load()
    rec = {"shape": f"ipv T={T} ns={ns} d={d} rows={rows} q={q} matern REUSE_INNER trace=NULL; believer q={q} log EI",
           "refined_tasks": int(_refined(b).sum()), "float64_tasks": int((_scal(b)[:, 45] > 30.0).sum()),
           "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "scratch_bytes": {str(M): int(lib.adkf_ipv_pool_scratch_bytes(T, ns, d, M, q)) for M in Ms},
           "believer_log_ei_s": med["believer_log_ei"],
           "ipv_s": {str(M): med[f"ipv_M{M}"] for M in Ms},
           "ipv_over_believer": {str(M): med[f"ipv_M{M}"] / med["believer_log_ei"] for M in Ms},
           "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()},
           "repeat_is_bit_equal": bool(all(torch.equal(o1[M]["sel_idx"], o2[M]["sel_idx"]) and
                                           torch.equal(o1[M]["sel_val"].view(torch.int32), o2[M]["sel_val"].view(torch.int32)) and
                                           torch.equal(o1[M]["tvar"].view(torch.int32), o2[M]["tvar"].view(torch.int32)) for M in Ms)),
           "all_selected": bool(all((o1[M]["sel_idx"] >= 0).all() and torch.isfinite(o1[M]["sel_val"]).all() for M in Ms)),
           "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def shape_ehvi(T, ns, d, rows, k, reps, dev, out_path=None):
    """T / 2 two-objective groups (2 g, 2 g + 1) with mixed senses, fronts from the support labels padded with jittered copies."""
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    G = T // 2
    hg = torch.Generator().manual_seed(1)
    yh = ys.cpu()
    obj = torch.tensor([[2 * q, 2 * q + 1] for q in range(G)], dtype=torch.int32)
    mx = torch.tensor([[q % 2, (q // 2) % 2] for q in range(G)], dtype=torch.int32)
    pts = torch.stack([yh[0::2], yh[1::2]], 2)                                     # [G, ns, 2]
    lo_, hi_ = pts.min(1).values, pts.max(1).values
    ref = torch.where(mx != 0, lo_ - 0.1 * (hi_ - lo_), hi_ + 0.1 * (hi_ - lo_))
    front = {P: (pts[:, torch.randint(ns, (P,), generator=hg)] + 0.05 * torch.randn(G, P, 2, generator=hg)) for P in (16, 64)}
    # an anti-chain over the label range, from (best, worst) to (worst, best): every one of its 64 points is a step of the staircase
    u = (torch.arange(64) + 0.5) / 64
    best_, worst_ = torch.where(mx != 0, hi_, lo_), torch.where(mx != 0, lo_, hi_)
    chain = torch.stack([best_[:, None, 0] + u[None] * (worst_ - best_)[:, None, 0],
                         best_[:, None, 1] + (1 - u[None]) * (worst_ - best_)[:, None, 1]], 2)[:, torch.randperm(64, generator=hg)]
    con = torch.tensor([[(2 * q + 2) % T, (2 * q + 3) % T] for q in range(G)], dtype=torch.int32)
    thr = torch.tensor([[float(yh[(2 * q + 2) % T].median()), float(yh[(2 * q + 3) % T].median())] for q in range(G)])
    kw = dict(obj=obj, ref=ref, obj_maximize=mx, topk=k, want_score=False, want_stair=True)
    variants = {"log_P16": dict(front=front[16], log=True), "log_P64": dict(front=front[64], log=True), "lin_P16": dict(front=front[16]),
                "log_P16_C2": dict(front=front[16], log=True, con=con, con_thr=thr),
                "log_chain64": dict(front=chain, log=True), "lin_chain64": dict(front=chain),
                "log_chain64_C2": dict(front=chain, log=True, con=con, con_thr=thr)}
    f_e = {n: (lambda v=v: gp_ops.ehvi_pool(b, phi, X, **kw, **v)) for n, v in variants.items()}
    f_mv = lambda: gp_ops.predict_pool(b, phi, X, latent=True, want_mean=True, want_var=True)
    f_lei = lambda: gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=k, log_ei=True)
    o1 = {n: f() for n, f in f_e.items()}
    o2 = {n: f() for n, f in f_e.items()}
    f_mv(); f_lei()
    torch.cuda.synchronize()
    for n in o1:
        gp_ops.check_info(o1[n]["info"])
    ts = {"mean_var": [], "log_ei": [], **{n: [] for n in f_e}}
    for _ in range(reps):
        ts["mean_var"].append(once(f_mv))
        ts["log_ei"].append(once(f_lei))
        for n, f in f_e.items():
            ts[n].append(once(f))
    med = {n: float(np.median(x)) for n, x in ts.items()}
    lib = _lib.load()
    rec = {"shape": f"ehvi T={T} G={G} ns={ns} d={d} rows={rows} k={k} matern REUSE_INNER score=NULL; predict_pool latent mean+var; predict_pool k={k} log EI",
           "refined_tasks": int(_refined(b).sum()), "float64_tasks": int((_scal(b)[:, 45] > 30.0).sum()),
           "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d)), "scratch_bytes": int(lib.adkf_ehvi_pool_scratch_bytes(T, G, k)),
           "chunk_rows": int(_lib.EHVI_CHUNK_ROWS), "stair_points": {n: o1[n]["stair_n"].tolist() for n in o1},
           "predict_pool_mean_var_s": med["mean_var"], "predict_pool_log_ei_s": med["log_ei"], "ehvi_s": {n: med[n] for n in f_e},
           "ehvi_over_mean_var": {n: med[n] / med["mean_var"] for n in f_e}, "ehvi_over_log_ei": {n: med[n] / med["log_ei"] for n in f_e},
           # stage A is prediction's own launch per chunk with both outputs: the mean_var call is its cost, the rest is the score kernels
           "stage_a_share": {n: med["mean_var"] / med[n] for n in f_e},
           "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()},
           "repeat_is_bit_equal": bool(all(torch.equal(o1[n]["top_idx"], o2[n]["top_idx"]) and
                                           torch.equal(o1[n]["top_val"].view(torch.int32), o2[n]["top_val"].view(torch.int32)) for n in o1)),
           "all_selected": bool(all((o1[n]["top_idx"] >= 0).all() and torch.isfinite(o1[n]["top_val"]).all() for n in o1)),
           "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def shape_jes(T, ns, d, rows, k, Ss, m, reps, dev, out_path=None):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    omega, phase = gp_ops.rff_basis("matern", d, m, generator=torch.Generator().manual_seed(0), device=dev)
    opt = {}
    for S in Ss:
        w, eps = torch.randn(T, S, m, device=dev, generator=g), torch.randn(T, S, ns, device=dev, generator=g)
        opt[S] = gp_ops.optimum_samples(b, phi, X, omega=omega, phase=phase, n_samples=S, w=w, eps=eps)
        gp_ops.check_info(opt[S]["info"])
    f_lei = lambda: gp_ops.predict_pool(b, phi, X, latent=True, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=k, log_ei=True)
    f_jes = {S: (lambda S=S: gp_ops.jes_pool(b, phi, X, opt_idx=opt[S]["opt_idx"], opt_val=opt[S]["opt_val"], topk=k, want_score=False)) for S in Ss}
    f_kg = {S: (lambda S=S: gp_ops.kg_pool(b, phi, X, ref_idx=opt[S]["opt_idx"], log=True, topk=k, want_score=False)) for S in Ss}
    f_mes = {S: (lambda S=S: gp_ops.mes_pool(b, phi, X, ystar=opt[S]["opt_val"], topk=k, want_score=False)) for S in Ss}
    o1 = {S: f_jes[S]() for S in Ss}
    o2 = {S: f_jes[S]() for S in Ss}
    f_lei()
    for S in Ss:
        f_kg[S](); f_mes[S]()
    torch.cuda.synchronize()
    for S in Ss:
        gp_ops.check_info(o1[S]["info"])
    ts = {"log_ei": [], **{f"{n}_S{S}": [] for S in Ss for n in ("jes", "kg", "mes")}}
    for _ in range(reps):
        ts["log_ei"].append(once(f_lei))
        for S in Ss:
            ts[f"jes_S{S}"].append(once(f_jes[S]))
            ts[f"kg_S{S}"].append(once(f_kg[S]))
            ts[f"mes_S{S}"].append(once(f_mes[S]))
    med = {n: float(np.median(x)) for n, x in ts.items()}
    lib = _lib.load()
    rec = {"shape": f"jes T={T} ns={ns} d={d} rows={rows} k={k} matern REUSE_INNER score=NULL cond_noise=1e-6; kg log KG M=S on opt_idx; mes on opt_val; predict_pool k={k} log EI",
           "refined_tasks": int(_refined(b).sum()), "float64_tasks": int((_scal(b)[:, 45] > 30.0).sum()),
           "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "scratch_bytes": {str(S): int(lib.adkf_jes_pool_scratch_bytes(T, ns, d, S, k)) for S in Ss},
           "distinct_locations_per_task_min": {str(S): int(min(len(set(r)) for r in opt[S]["opt_idx"].cpu().tolist())) for S in Ss},
           "predict_pool_log_ei_s": med["log_ei"],
           "jes_s": {str(S): med[f"jes_S{S}"] for S in Ss}, "kg_s": {str(S): med[f"kg_S{S}"] for S in Ss}, "mes_s": {str(S): med[f"mes_S{S}"] for S in Ss},
           "jes_over_kg": {str(S): med[f"jes_S{S}"] / med[f"kg_S{S}"] for S in Ss},
           "jes_over_mes": {str(S): med[f"jes_S{S}"] / med[f"mes_S{S}"] for S in Ss},
           "jes_over_log_ei": {str(S): med[f"jes_S{S}"] / med["log_ei"] for S in Ss},
           "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()},
           "repeat_is_bit_equal": bool(all(torch.equal(o1[S]["top_idx"], o2[S]["top_idx"]) and
                                           torch.equal(o1[S]["top_val"].view(torch.int32), o2[S]["top_val"].view(torch.int32)) for S in Ss)),
           "all_selected": bool(all((o1[S]["top_idx"] >= 0).all() and torch.isfinite(o1[S]["top_val"]).all() for S in Ss)),
           "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def shape_gibbon(T, ns, d, rows, q, S, reps, dev, out_path=None):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    b = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(b, True, True)
    b.flags = gp_ops.REUSE_DIST
    phi, _, _, _, info = gp_ops.fit(b, phi0, 200)
    gp_ops.check_info(info)
    b.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    # samples of min f: below the smallest label, spread over one prior standard deviation (--mes's)
    ystar = (ys.min(1).values[:, None] - torch.rand(T, S, device=dev, generator=g)).contiguous()
    f_gb = lambda: gp_ops.gibbon_pool(b, phi, X, ystar=ystar, q=q)
    f_bv = lambda: gp_ops.believer_pool(b, phi, X, best_f=best, q=q, log_ei=True)
    mes1 = lambda: gp_ops.mes_pool(b, phi, X, ystar=ystar, topk=q)
    f_mes = lambda: [mes1() for _ in range(q)]
    o1, o2 = f_gb(), f_gb()
    f_bv(); topq = mes1()
    torch.cuda.synchronize()
    gp_ops.check_info(o1["info"])
    ts = {"gibbon": [], "believer_log_ei": [], "q_calls_of_mes_pool": []}
    for _ in range(reps):
        ts["gibbon"].append(once(f_gb))
        ts["believer_log_ei"].append(once(f_bv))
        ts["q_calls_of_mes_pool"].append(once(f_mes))
    med = {n: float(np.median(x)) for n, x in ts.items()}
    lib = _lib.load()
    shared = [len(set(a) & set(c)) for a, c in zip(o1["sel_idx"].cpu().tolist(), topq["top_idx"].cpu().tolist())]
    rec = {"shape": f"gibbon T={T} ns={ns} d={d} rows={rows} q={q} S={S} matern REUSE_INNER trace=NULL", "refined_tasks": int(_refined(b).sum()),
           "float64_tasks": int((_scal(b)[:, 45] > 30.0).sum()), "workspace_bytes": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "scratch_bytes": int(lib.adkf_believer_pool_scratch_bytes(T, ns, d, q)),
           "gibbon_s": med["gibbon"], "believer_log_ei_s": med["believer_log_ei"], "q_calls_of_mes_pool_s": med["q_calls_of_mes_pool"],
           "gibbon_over_believer": med["gibbon"] / med["believer_log_ei"], "gibbon_over_q_calls_of_mes_pool": med["gibbon"] / med["q_calls_of_mes_pool"],
           "spread_max_minus_min_over_median": {n: (max(x) - min(x)) / float(np.median(x)) for n, x in ts.items()},
           "repeat_is_bit_equal": bool(all(torch.equal(o1[n].view(torch.int32), o2[n].view(torch.int32)) for n in ("sel_idx", "sel_val", "sel_mean", "sel_var"))),
           "all_selected": bool((o1["sel_idx"] >= 0).all() and torch.isfinite(o1["sel_val"]).all()),
           "distinct_picks_per_task_min": int(min(len(set(r)) for r in o1["sel_idx"].cpu().tolist())),
           "picks_shared_with_mes_top_q_per_task": shared, "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def shape_believer_ard(T, ns, d, rows, q, reps, dev, out_path=None):
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    Zs = torch.randn(T, ns, d, device=dev, generator=g) @ W
    ys = torch.sin(Zs[..., :4].sum(-1))
    bi = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern")
    phi0, _ = gp_ops.init_params_batch(bi, True, True)
    bi.flags = gp_ops.REUSE_DIST
    phi_i, _, _, _, info = gp_ops.fit(bi, phi0, 200)
    gp_ops.check_info(info)
    bi.flags = gp_ops.REUSE_DIST | gp_ops.REUSE_INNER
    ba = gp_ops.GPBatch(Zs, ys, torch.empty(T, 4, device=dev), "matern", ard=True)
    phi0, _ = gp_ops.init_params_batch(ba, True, True)
    phi_a, _, _, n_evals, info = gp_ops.fit(ba, phi0, 100)
    gp_ops.check_info(info)
    ba.flags = gp_ops.REUSE_INNER
    X = torch.empty(rows, d, device=dev)
    for lo in range(0, rows, 1 << 16):
        X[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, rows - lo), d, device=dev, generator=g) @ W
    best = ys.median(1).values.contiguous()
    kw = dict(latent=True, best_f=best, want_mean=False, want_var=False, want_ei=False, topk=1)
    fs = [lambda: gp_ops.believer_pool_ard(ba, phi_a, X, best_f=best, q=q), lambda: gp_ops.believer_pool(bi, phi_i, X, best_f=best, q=q),
          lambda: gp_ops.predict_pool(ba, phi_a, X, **kw), lambda: gp_ops.predict_pool(bi, phi_i, X, **kw)]
    o1, o2 = fs[0](), fs[0]()
    oi, ref = fs[1](), fs[2]()
    fs[3]()
    torch.cuda.synchronize()
    gp_ops.check_info(o1["info"]); gp_ops.check_info(oi["info"])
    ts = [[], [], [], []]
    for _ in range(reps):
        for k, f in enumerate(fs):
            ts[k].append(once(f))
    t_ba, t_bi, t_pa, t_pi = (float(np.median(x)) for x in ts)
    spread = [float((max(x) - min(x)) / np.median(x)) for x in ts]
    lib = _lib.load()
    ell = torch.nn.functional.softplus(phi_a[:, 2:])
    rec = {"shape": f"believer ard T={T} ns={ns} d={d} rows={rows} q={q} matern REUSE_INNER trace=NULL",
           "float64_tasks_ard": int((_scal(ba)[:, 45] > 30.0).sum()), "float64_tasks_isotropic": int((_scal(bi)[:, 45] > 30.0).sum()),
           "refined_tasks_ard": int(_refined(ba).sum()), "refined_tasks_isotropic": int(_refined(bi).sum()),
           "workspace_bytes_ard": int(lib.adkf_workspace_bytes_ard(T, ns, 0, d)), "workspace_bytes_isotropic": int(lib.adkf_workspace_bytes(T, ns, 0, d)),
           "scratch_bytes": int(lib.adkf_believer_pool_scratch_bytes(T, ns, d, q)),
           "ard_fit_evals_max": int(n_evals.max()), "ard_lengthscale_min": float(ell.min()), "ard_lengthscale_max": float(ell.max()),
           "believer_ard_s": t_ba, "believer_isotropic_s": t_bi, "predict_pool_k1_ard_s": t_pa, "predict_pool_k1_isotropic_s": t_pi,
           "believer_ard_over_isotropic": t_ba / t_bi, "predict_pool_ard_over_isotropic": t_pa / t_pi,
           "spread_max_minus_min_over_median": dict(zip(("believer_ard", "believer_isotropic", "predict_pool_ard", "predict_pool_isotropic"), spread)),
           "step_0_is_predict_pool_bitwise": bool(torch.equal(o1["sel_idx"][:, 0], ref["top_idx"][:, 0]) and torch.equal(o1["sel_val"][:, 0], ref["top_val"][:, 0])),
           "repeat_is_bit_equal": bool(all(torch.equal(o1[n], o2[n]) for n in ("sel_idx", "sel_val", "sel_mean", "sel_var"))),
           "distinct_picks_per_task_min_ard": int(min(len(set(r)) for r in o1["sel_idx"].cpu().tolist())),
           "distinct_picks_per_task_min_isotropic": int(min(len(set(r)) for r in oi["sel_idx"].cpu().tolist())), "all_s": ts}
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return rec


def _scal(b):
    """The per-task scalars [T, 64] of a support-only workspace (carve() order of csrc/host_gp.h; slot 45 is the pivot ratio that flags
    a task for the float64 path above 30)."""
    ws, _ = b.workspace()
    al = lambda nfloat: (nfloat * 4 + 255) // 256 * 256
    off = al(b.T * b.d) + 4 * al(b.T * b.ns * b.ns) + al(b.T * 16 * b.ns)
    return ws[off:off + b.T * 64 * 4].view(torch.float32).view(b.T, 64).cpu()


def bo_shape(R, dev, loops=10):
    from adkf_ift_amd import bayes_opt as BO
    g = torch.Generator().manual_seed(3)
    X = torch.randn(10000, 6, generator=g)
    y = ((X - 0.3) ** 2).sum(1)
    order = torch.argsort(y)
    X, y = X[order].to(dev), y[order].to(dev)
    kw = dict(num_init_points=6, query_batch_size=2, num_bo_iters=3, kernel_type="matern", device=dev, init_from=5000, noise_init=0.01,
              noise_prior=True)
    batched = lambda: BO.run_gp_ei_bo_batched(X, y, rngs=[np.random.default_rng(s) for s in range(R)], **kw)
    sequential = lambda: [BO.run_gp_ei_bo(X, y, rng=np.random.default_rng(s), streaming=True, **kw) for s in range(R)]
    out = {"shape": f"GP-EI BO: {R} replicates, pool 10000 x 6, 6 initial points, 3 iterations of 2 queries; wall time of {loops} runs"}
    BO.run_gp_ei_bo_batched(X, y, rngs=[np.random.default_rng(99)], **kw)   # warm-up of both paths
    BO.run_gp_ei_bo(X, y, rng=np.random.default_rng(99), streaming=True, **kw)
    for name, f in (("batched", batched), ("sequential", sequential), ("batched_2", batched), ("sequential_2", sequential)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(loops):
            rec = f()
        torch.cuda.synchronize()
        out[name + "_walltime_s"] = time.perf_counter() - t0
        out.setdefault("records", {})[name] = rec
    out["records_equal"] = out["records"]["batched"] == out["records"]["sequential"]
    del out["records"]
    out["speedup"] = min(out["sequential_walltime_s"], out["sequential_2_walltime_s"]) / min(out["batched_walltime_s"], out["batched_2_walltime_s"])
    print(json.dumps(out), flush=True)


def meta_test_shape(dev):
    from adkf_ift_amd import evaluate as E
    from adkf_ift_amd.models import ADKTModel, ADKTModelConfig
    from adkf_ift_amd.synthetic import meta_test_tasks
    tasks, sizes = meta_test_tasks(157, 64)
    model = ADKTModel(ADKTModelConfig()).to(dev)
    out = {"shape": f"meta-test protocol: 157 tasks, support 64, query sizes {int(sizes.min())}..{int(sizes.max())}, 16 tasks per call"}
    for streaming in (False, True):
        E.evaluate_tasks(model, tasks[:4], tasks_per_call=4, streaming=streaming)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.evaluate_tasks(model, tasks, tasks_per_call=16, streaming=streaming)
        torch.cuda.synchronize()
        out["streaming_walltime_s" if streaming else "padded_walltime_s"] = time.perf_counter() - t0
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-meta-test", action="store_true")
    ap.add_argument("--ard", action="store_true", help="ARD batches against isotropic streaming (no meta-test line)")
    ap.add_argument("--skip-large", action="store_true", help="leave out the 1 x 256 x 512 shape with 1M rows")
    ap.add_argument("--pool", action="store_true", help="shared-pool prediction against the packed call on a replicated pool, and the batched BO loop")
    ap.add_argument("--skip-bo", action="store_true")
    ap.add_argument("--thompson", action="store_true", help="adkf_thompson_pool against variant (ii) of --pool, timed alternately")
    ap.add_argument("--believer", action="store_true", help="adkf_believer_pool against q calls of adkf_predict_pool(k = 1), timed alternately")
    ap.add_argument("--mes", action="store_true", help="adkf_mes_pool at S = 1, 16, 64 against adkf_predict_pool(k, log EI), timed alternately")
    ap.add_argument("--gibbon", action="store_true", help="adkf_gibbon_pool(q = 8, S = 16) against adkf_believer_pool(q = 8, log EI) and q calls of adkf_mes_pool(S = 16), timed alternately")
    ap.add_argument("--gumbel", action="store_true", help="adkf_gumbel_pool against adkf_predict_pool(k, log EI) and max_value_samples(S = 16, m = 1024), timed alternately")
    ap.add_argument("--kg", action="store_true", help="adkf_kg_pool(log KG, k = 8) at M = 32 and 64 against adkf_predict_pool(k, log EI) and adkf_believer_pool(q = 8, log EI), timed alternately")
    ap.add_argument("--jes", action="store_true", help="adkf_jes_pool(k = 8) at S = 16 and 64 against adkf_kg_pool(log KG, k = 8) at M = S, adkf_mes_pool(k = 8) and adkf_predict_pool(k, log EI), timed alternately")
    ap.add_argument("--ipv", action="store_true", help="adkf_ipv_pool(q = 16) at M = 16 and 48 targets against adkf_believer_pool(q = 16, log EI) at T = 64, ns = 128, d = 64, 100 000 rows, timed alternately")
    ap.add_argument("--ehvi", action="store_true", help="adkf_ehvi_pool(k = 8) over 8 two-objective groups - log form at P = 16 and 64, linear at P = 16, P = 16 with C = 2, and a 64-step anti-chain staircase (log, linear, log with C = 2) - against adkf_predict_pool(latent mean and var) and adkf_predict_pool(k, log EI), timed alternately")
    ap.add_argument("--out", default=None, help="--thompson, --believer (each with or without --ard), --mes, --gibbon, --gumbel, --kg, --jes, --ipv, --ehvi: also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.mes:
        shape_mes(16, 128, 256, 100000, 8, a.reps, dev, a.out)
        return
    if a.kg:
        shape_kg(16, 128, 256, 100000, 8, (32, 64), a.reps, dev, a.out)
        return
    if a.jes:
        shape_jes(16, 128, 256, 100000, 8, (16, 64), 1024, a.reps, dev, a.out)
        return
    if a.ipv:
        shape_ipv(64, 128, 64, 100000, 16, (16, 48), a.reps, dev, a.out)
        return
    if a.ehvi:
        shape_ehvi(16, 128, 256, 100000, 8, a.reps, dev, a.out)
        return
    if a.gibbon:
        shape_gibbon(16, 128, 256, 100000, 8, 16, a.reps, dev, a.out)
        return
    if a.gumbel:
        shape_gumbel(16, 128, 256, 100000, 8, 16, 1024, a.reps, dev, a.out)
        return
    if a.believer and a.ard:
        shape_believer_ard(16, 128, 256, 100000, 8, a.reps, dev, a.out)
        return
    if a.believer:
        shape_believer(16, 128, 256, 100000, 8, a.reps, dev, a.out)
        return
    if a.thompson and a.ard:
        rec = shape_thompson_ard(16, 128, 256, 262144, 16, 1024, a.reps, dev, a.out)
        sys.exit(0 if rec["within_1_15"] else 1)
    if a.thompson:
        rec = shape_thompson(16, 128, 256, 262144, 16, 1024, a.reps, dev, a.out)
        sys.exit(0 if rec["beats_S_passes"] else 1)
    if a.pool:
        shape_pool(16, 128, 256, 262144, 16, a.reps, dev)
        if not a.skip_bo:
            bo_shape(16, dev)
        return
    run = shape_ard if a.ard else shape
    run(16, 128, 2048, 4096, a.reps, dev)
    run(16, 128, 2048, 65536, a.reps, dev)
    if not a.skip_large:
        run(1, 256, 512, 1000000, a.reps, dev)
    if not a.skip_meta_test and not a.ard:
        meta_test_shape(dev)


if __name__ == "__main__":
    main()
