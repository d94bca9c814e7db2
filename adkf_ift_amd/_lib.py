"""ctypes binding of libadkf_gp.so (include/adkf_gp.h).  There is NO fallback: if the HIP library is not
built, importing the GP operators raises."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libadkf_gp.so")
if os.environ.get("ADKF_LIB"):   # diagnostics: an alternative build of the same sources (e.g. with -DADKF_* experiment macros)
    LIB_PATH = os.environ["ADKF_LIB"]

KERNEL_RBF = 0
KERNEL_MATERN52 = 1
IGNORE_GRAD_CORRECTION = 1
IGNORE_DIRECT_GRAD = 2
INFO_OUTER_BASE = 100000
PM_LATENT = 1     # adkf_predict_marginal: var without the observation noise
PM_MAXIMIZE = 2   # ... ei for maximisation
PM_SCORE_MEAN = 4  # adkf_predict_pool: rank by the posterior mean instead of ei
PM_LOG_EI = 16    # ... ei, and the ei score of adkf_predict_pool, hold log EI (8 is not a flag)
POOL_TOPK_MAX = 64
KG_REFS_MAX = 64         # adkf_kg_pool: reference rows per task
IPV_ENTRIES_MAX = 64     # adkf_ipv_pool: targets plus picks per task
EHVI_FRONT_MAX = 64      # adkf_ehvi_pool: front points per group
EHVI_CONS_MAX = 4        # ... constraint tasks per group
EHVI_CHUNK_ROWS = 16384  # ... pool rows per chunk of its walk
PM_SCORE_BALD = 32       # adkf_mix_pool: rank by the disagreement of the members
MIX_MEMBERS_MAX = 64     # ... member tasks per group
PM_JK_SCALED = 64        # adkf_jackknife_pool: fold widths scaled by the leave-one-out predictive deviation
JK_POINTS_MAX = 256      # ... support points per task
JK_LEVELS_MAX = 8        # ... levels per call
MIX_CHUNK_ROWS = 16384   # ... pool rows per chunk of its walk
TS_SAMPLES_MAX = 64      # adkf_thompson_pool: posterior draws per task
TS_FEATURES_MAX = 4096   # ... random Fourier features (a multiple of 64, at least 64)
LS_STRADDLE, LS_PROB, LS_BOUND = 0, 1, 2   # adkf_levelset_pool: the score kinds
QEI_SAMPLES_MAX = 256    # adkf_qei_pool: posterior draws per task
QEI_PICKS_MAX = 64       # ... picks per task
RANK_K_MAX = 65536       # adkf_rank_pool: rows listed per task
RANK_REFS_MAX = 1024     # ... rows ranked per task
RANK_CHUNK_ROWS = 16384  # ... pool rows per chunk of its walk

ERRORS = {-1: "bad argument", -2: "unsupported size (see adkf_max_points)", -3: "workspace too small",
          -4: "HIP launch failed"}


class Batch(C.Structure):
    _fields_ = [("T", C.c_int32), ("ns_max", C.c_int32), ("nq_max", C.c_int32), ("d", C.c_int32),
                ("kernel", C.c_int32), ("flags", C.c_int32),
                ("n_s", C.c_void_p), ("n_q", C.c_void_p), ("Z_s", C.c_void_p), ("y_s", C.c_void_p),
                ("Z_q", C.c_void_p), ("y_q", C.c_void_p), ("priors", C.c_void_p)]


class MsgEt(C.Structure):
    """adkf_msg_et_t"""
    _fields_ = [("src", C.c_void_p), ("tgt", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("dW", C.c_void_p),
                ("db", C.c_void_p), ("E", C.c_int32)]


class FitOptions(C.Structure):
    _fields_ = [("max_evals", C.c_int32), ("exact_evals", C.c_int32), ("gtol", C.c_float), ("ftol", C.c_float),
                ("ev_start", C.c_void_p), ("ev_stop", C.c_void_p)]


_lib = None

# name -> (restype, argtypes); kept in one table so tests can check every declared symbol is exported
SIGNATURES = {
    "adkf_version": (C.c_char_p, []),
    "adkf_last_hip_error": (C.c_char_p, []),
    "adkf_max_points": (C.c_int, []),
    "adkf_path_info": (C.c_int, [C.c_int32, C.c_int32]),
    "adkf_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "adkf_median_lengthscale": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_init_params": (C.c_int, [C.POINTER(Batch), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_mll_value_grad": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_fit": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.POINTER(FitOptions), C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_predict": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_predict_marginal": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_predict_marginal_ard": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_predict_grad": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_predict_pool_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "adkf_predict_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_thompson_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "adkf_thompson_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_thompson_pool_ard": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_qei_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "adkf_qei_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_believer_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "adkf_believer_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_believer_pool_ard": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_mes_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_gumbel_pool_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "adkf_gumbel_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_gibbon_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_liar_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "adkf_liar_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_levelset_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "adkf_levelset_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "adkf_kg_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 5),
    "adkf_kg_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_jes_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 5),
    "adkf_jes_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_ipv_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 5),
    "adkf_ipv_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_jackknife_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "adkf_jackknife_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_ehvi_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "adkf_ehvi_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_mix_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "adkf_mix_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_rank_pool_scratch_bytes": (C.c_size_t, [C.c_int32] * 4),
    "adkf_rank_pool": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_outer_nll_value_grad": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_ift_hypergrad": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "adkf_check_info": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "adkf_workspace_bytes_ard": (C.c_size_t, [C.c_int32] * 4),
    "adkf_msg_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "adkf_msg_backward_scratch_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "adkf_msg_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_size_t, C.c_void_p]),
    "adkf_readout_pool": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 5 + [C.c_void_p] * 7),
    "adkf_readout_pool_backward": (C.c_int, [C.c_void_p] * 10 + [C.c_int32] * 5 + [C.c_void_p] * 6),
    "adkf_readout_pool_hidden": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_void_p] * 9),
    "adkf_readout_pool_hidden_backward": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] + [C.c_void_p] * 9 + [C.c_int32] * 5 + [C.c_void_p] * 6),
    "adkf_pna_aggregate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "adkf_pna_aggregate_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "adkf_pna_aggregate_backward_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                   C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "adkf_block_combine": (C.c_int, [C.c_void_p] * 8 + [C.c_float, C.c_int32, C.c_int32] + [C.c_void_p] * 5),
    "adkf_block_combine_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "adkf_block_combine_backward": (C.c_int, [C.c_void_p] * 11 + [C.c_int32, C.c_int32] + [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p]),
    "adkf_split_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "adkf_split_planes_t": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "adkf_dense_forward": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p]),
    "adkf_dense_weight_grad_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "adkf_dense_weight_grad": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    "adkf_grad_sumsq": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "adkf_clip_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_float,
                                      C.c_float, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "adkf_clip_adam_step_one": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_double,
                                          C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_void_p]),
    "adkf_ift_hypergrad_cg": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "adkf_double_path_tasks": (C.c_int, [C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
            "The GP path has no CPU or PyTorch fallback.")
    # torch first: its bundled HIP runtime must be the one in the process before this library binds to libamdhip64
    # (loaded the other way round, the library sees "no ROCm-capable device" for streams created by torch)
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def ptr(t):
    """Device address of tensor ``t`` for a C entry; ``None`` (an output or input not asked for) stays ``None``."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device) -> C.c_void_p:
    """torch's current stream on ``device``: every entry launches on the stream the caller's tensors are ordered on."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(rc: int, what: str):
    if rc != 0:
        detail = f" ({_lib.adkf_last_hip_error().decode()})" if rc == -4 and _lib is not None else ""
        raise RuntimeError(f"{what} failed: {ERRORS.get(rc, rc)}{detail}")
