"""ctypes binding of libgpk.so (include/gpk.h).

The product path has exactly one compute backend: the gfx950 HIP library.  If it is not
built, or no gfx950 device is visible, every call raises — there is no CPU fallback.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPK_LIB_PATH") or os.path.join(_HERE, "_lib", "libgpk.so")

GPK_OK, GPK_EINVAL, GPK_ENOTPD, GPK_EHIP, GPK_ERCCL, GPK_ENOMEM, GPK_ENODEV = range(7)
GPK_FLAG_FORCE_BIG_GEMM = 1  # include/gpk.h
GPK_FLAG_FORCE_BIG_SPD = 2
GPK_FLAG_FORCE_SMALL_SPD = 4
GPK_FLAG_FORCE_HUGE_GEMM = 8
GPK_FLAG_NO_FAST_GRAPH = 16
GPK_FLAG_FAST_FIRST = 32
GPK_FLAG_NO_DCLASS = 64
GPK_FLAG_NO_CHAIN = 128
GPK_FLAG_NO_CHAIN_AUG = 256
GPK_FLAG_FORCE_WIDE_SPD = 512
GPK_FLAG_FORCE_NARROW_SPD = 1024
GPK_FLAG_SPLIT_FACTORS = 2048
GPK_FLAG_FORCE_CHAIN_MULTI = 4096
GPK_FLAG_REFINE_ALL = 8192
GPK_FLAG_NO_REFINE = 16384
GPK_FLAG_MATRIX_GEMV = 32768
GPK_FLAG_NO_QUARTER_TILES = 65536
GPK_FLAG_DD_CONTRACTION = 131072
GPK_FLAG_NO_DD_CONTRACTION = 262144
GPK_FLAG_ONE_SWEEP_UPDATE = 524288
GPK_FLAG_NO_QUARTER_FIRST = 1048576
GPK_FLAG_REFINE_FWD1_ONLY = 2097152
GPK_FLAG_NO_CLASS_BINS = 4194304
GPK_FLAG_NO_CLASS_PIPE = 8388608
GPK_FLAG_NO_CHAIN_LOOKAHEAD = 16777216
GPK_FLAG3_REFINE, GPK_FLAG3_REFINE_GEMM = 1, 2  # gpk_problem3.flags (their own bit space)
REFINE_GEMM, REFINE_FUSED = 0, 1  # refinement routes (gpk_refine_info3, gpk_refine_panel)
REFINE_COND_LB = 100.0  # csrc/gpk_internal.h: a refinement gate opens above this bound
GPK_INV_SWEEP, GPK_INV_CHAIN, GPK_INV_CHAIN_AUG, GPK_INV_BIG, GPK_INV_BIG_WIDE, GPK_INV_CHAIN_MULTI = range(6)
INV_PATH_NAMES = {0: "sweep", 1: "chain", 2: "chain_aug", 3: "big", 4: "big_wide", 5: "chain_multi"}
KIND_IDS = {"SE_Cos_1d": 0, "Matern52_Cos_1d": 1, "SE_1d": 2, "Matern52_1d": 3}
EQ_IDS = {"poisson": 0, "allencahn": 1, "advection": 2}

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


class GPKError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libgpk error {code}: {msg}")
        self.code = code


class NotPositiveDefinite(GPKError):
    pass


class gpk_problem(ctypes.Structure):
    _fields_ = [
        ("dim", ctypes.c_int32), ("eq", ctypes.c_int32), ("kind", ctypes.c_int32),
        ("n1", ctypes.c_int32), ("n2", ctypes.c_int32), ("q", ctypes.c_int32),
        ("x1", _dp), ("x2", _dp), ("src", _dp), ("bvals", _dp), ("bidx", _ip),
        ("nb", ctypes.c_int32),
        ("jitter", ctypes.c_double), ("llk_weight", ctypes.c_double),
        ("logdet", ctypes.c_double), ("beta", ctypes.c_double),
        ("lr", ctypes.c_double), ("b1", ctypes.c_double), ("b2", ctypes.c_double),
        ("eps", ctypes.c_double),
        ("device", ctypes.c_int32), ("flags", ctypes.c_int32),
        ("uoff", _dp),
    ]


class gpk_problem3(ctypes.Structure):
    _fields_ = [
        ("eq", ctypes.c_int32), ("kind", ctypes.c_int32),
        ("n1", ctypes.c_int32), ("n2", ctypes.c_int32), ("n3", ctypes.c_int32), ("q", ctypes.c_int32),
        ("x1", _dp), ("x2", _dp), ("x3", _dp), ("src", _dp), ("bvals", _dp),
        ("jitter", ctypes.c_double), ("llk_weight", ctypes.c_double), ("logdet", ctypes.c_double),
        ("lr", ctypes.c_double), ("b1", ctypes.c_double), ("b2", ctypes.c_double),
        ("eps", ctypes.c_double),
        ("device", ctypes.c_int32), ("flags", ctypes.c_int32),
    ]


class gpk_operator3(ctypes.Structure):
    _fields_ = [
        ("order", ctypes.c_int32 * 3), ("coef", ctypes.c_double * 3), ("react", ctypes.c_double * 3),
        ("faces", ctypes.c_int32),
    ]


class gpk_operator3x(ctypes.Structure):
    _fields_ = [
        ("c2", ctypes.c_double * 3), ("c1", ctypes.c_double * 3), ("react", ctypes.c_double * 3),
        ("faces", ctypes.c_int32),
    ]


class gpk_coef3(ctypes.Structure):
    _fields_ = [("a", ctypes.POINTER(ctypes.c_double) * 3), ("rho", ctypes.POINTER(ctypes.c_double))]


class gpk_bdata3(ctypes.Structure):
    _fields_ = [("dfaces", ctypes.c_int32), ("dvals", ctypes.POINTER(ctypes.c_double))]


class gpk_conv3(ctypes.Structure):
    _fields_ = [("g", ctypes.c_double * 3)]


class gpk_cross3(ctypes.Structure):
    _fields_ = [("m", ctypes.c_double * 3)]


class gpk_drift3(ctypes.Structure):
    _fields_ = [("b", ctypes.POINTER(ctypes.c_double) * 3)]


class gpk_high3(ctypes.Structure):
    _fields_ = [("c4", ctypes.c_double * 3), ("c3", ctypes.c_double * 3)]


class gpk_bicross3(ctypes.Structure):
    _fields_ = [("q", ctypes.c_double * 3)]


class gpk_gradsq3(ctypes.Structure):
    _fields_ = [("s", ctypes.c_double * 3), ("x", ctypes.c_double * 3)]


class gpk_gemm_case(ctypes.Structure):
    _fields_ = [
        ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32), ("K2", ctypes.c_int32),
        ("A", _dp), ("B", _dp), ("A2", _dp), ("B2", _dp),
        ("lda", ctypes.c_int32), ("ldb", ctypes.c_int32), ("lda2", ctypes.c_int32), ("ldb2", ctypes.c_int32),
        ("ta", ctypes.c_int32), ("tb", ctypes.c_int32), ("ta2", ctypes.c_int32), ("tb2", ctypes.c_int32),
        ("alpha", ctypes.c_double), ("alpha2", ctypes.c_double), ("beta", ctypes.c_double),
        ("C0", _dp), ("C", _dp),
        ("ldc0", ctypes.c_int32), ("ldc", ctypes.c_int32),
        ("epi", ctypes.c_int32), ("ac", ctypes.c_int32),
        ("F", _dp), ("U", _dp), ("Q1", _dp), ("Q2", _dp),
        ("Ys", _dp), ("Y", _dp),
        ("ldf", ctypes.c_int32), ("ldy", ctypes.c_int32),
        ("vscale", ctypes.c_int32), ("vscale2", ctypes.c_int32),
        ("gate", ctypes.c_int32), ("red_cap", ctypes.c_int32),
        ("red", _dp), ("red2", _dp),
        ("tiles", ctypes.c_int32),
    ]


EXPORTS = {
    "gpk_abi_version": ([], ctypes.c_int),
    "gpk_last_error": ([], ctypes.c_char_p),
    "gpk_device_count": ([_ip], ctypes.c_int),
    "gpk_kernel_matrices": ([ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_int32, _dp,
                             ctypes.c_int32, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_double,
                             _dp, _dp], ctypes.c_int),
    "gpk_create": ([ctypes.POINTER(gpk_problem), ctypes.c_double,
                    ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_destroy": ([ctypes.c_void_p], ctypes.c_int),
    "gpk_num_params": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "gpk_set_params": ([ctypes.c_void_p, _dp, ctypes.c_int64], ctypes.c_int),
    "gpk_get_params": ([ctypes.c_void_p, _dp, ctypes.c_int64], ctypes.c_int),
    "gpk_set_opt_state": ([ctypes.c_void_p, ctypes.c_int64, _dp, _dp, ctypes.c_int64], ctypes.c_int),
    "gpk_get_opt_state": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), _dp, _dp,
                           ctypes.c_int64], ctypes.c_int),
    "gpk_loss_grad": ([ctypes.c_void_p, _dp, _dp], ctypes.c_int),
    "gpk_step": ([ctypes.c_void_p, ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_prepare": ([ctypes.c_void_p, ctypes.c_int32], ctypes.c_int),
    "gpk_sync": ([ctypes.c_void_p], ctypes.c_int),
    "gpk_predict": ([ctypes.c_void_p, _dp, ctypes.c_int32, _dp, ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_predict_deriv": ([ctypes.c_void_p, _dp, ctypes.c_int32, _dp, ctypes.c_int32, ctypes.c_int32,
                           ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_evaluate": ([ctypes.c_void_p, _dp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_criterion": ([ctypes.c_void_p, _dp], ctypes.c_int),
    "gpk_profile_stages": ([ctypes.c_void_p, ctypes.c_int32, _dp, ctypes.c_int32, _ip], ctypes.c_int),
    "gpk_stage_name": ([ctypes.c_void_p, ctypes.c_int32], ctypes.c_char_p),
    "gpk_time_spd_inverse": ([ctypes.c_void_p, ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_bench_kernel": ([ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int32, _dp, _dp, _dp], ctypes.c_int),
    "gpk_kernel_pairs": ([ctypes.c_int32, ctypes.c_int32, _dp, _dp, ctypes.c_int64, _dp, _dp, _dp,
                          ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_fields_dd": ([ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_int32, ctypes.c_double,
                       ctypes.c_double, _dp, _dp], ctypes.c_int),
    "gpk_forward_field": ([ctypes.c_void_p, ctypes.c_int32, _dp, ctypes.c_int64], ctypes.c_int),
    "gpk_comm_unique_id": ([ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32], ctypes.c_int),
    "gpk_create_sharded": ([ctypes.POINTER(gpk_problem), ctypes.c_double, ctypes.c_int32, ctypes.c_int32,
                            ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_group_create": ([ctypes.POINTER(gpk_problem), ctypes.c_double, ctypes.c_int32,
                          ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_group_step": ([ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32, ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_group_loss_grad": ([ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32, _dp, _dp], ctypes.c_int),
    "gpk_shard_info": ([ctypes.c_void_p, _ip, _ip, _ip, _ip], ctypes.c_int),
    "gpk_shard_plan": ([ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64], ctypes.c_int),
    "gpk_inverse_path": ([ctypes.c_void_p, _ip], ctypes.c_int),
    "gpk_set_chain_capacity": ([ctypes.c_int32], ctypes.c_int),
    "gpk_set_spd_big_workgroups": ([ctypes.c_int32], ctypes.c_int),
    "gpk_set_wait_limit": ([ctypes.c_int32], ctypes.c_int),
    "gpk_set_wait_limit_chunk": ([ctypes.c_int32, ctypes.c_int32], ctypes.c_int),
    "gpk_graph_mode": ([ctypes.c_void_p, _ip, ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "gpk_distance_classes": ([_dp, ctypes.c_int32, _ip, _ip], ctypes.c_int),
    "gpk_class_count": ([ctypes.c_void_p, ctypes.c_int32, _ip], ctypes.c_int),
    "gpk_class_sum_path": ([ctypes.c_void_p, _ip], ctypes.c_int),
    "gpk_class_pipe": ([ctypes.c_void_p, _ip], ctypes.c_int),
    "gpk_create3": ([ctypes.POINTER(gpk_problem3), ctypes.c_double,
                     ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_create3_op": ([ctypes.POINTER(gpk_problem3), ctypes.POINTER(gpk_operator3), ctypes.c_double,
                        ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_operator_info3": ([ctypes.c_void_p, ctypes.POINTER(gpk_operator3)], ctypes.c_int),
    "gpk_create3_opx": ([ctypes.POINTER(gpk_problem3), ctypes.POINTER(gpk_operator3x), ctypes.c_double,
                         ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_operator_info3x": ([ctypes.c_void_p, ctypes.POINTER(gpk_operator3x)], ctypes.c_int),
    "gpk_create3_opv": ([ctypes.POINTER(gpk_problem3), ctypes.POINTER(gpk_operator3x), ctypes.POINTER(gpk_coef3),
                         ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_coef_info3": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "gpk_create3_opn": ([ctypes.POINTER(gpk_problem3), ctypes.POINTER(gpk_operator3x), ctypes.POINTER(gpk_coef3),
                         ctypes.POINTER(gpk_bdata3), ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_bdata_info3": ([ctypes.c_void_p, _ip, _ip], ctypes.c_int),
    "gpk_boundary_terms3": ([ctypes.c_void_p, _dp], ctypes.c_int),
    "gpk_create3_opc": ([ctypes.POINTER(gpk_problem3), ctypes.POINTER(gpk_operator3x), ctypes.POINTER(gpk_coef3),
                         ctypes.POINTER(gpk_bdata3), ctypes.POINTER(gpk_conv3), ctypes.c_double,
                         ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_conv_info3": ([ctypes.c_void_p, _dp], ctypes.c_int),
    "gpk_create3_opm": ([ctypes.POINTER(gpk_problem3), ctypes.POINTER(gpk_operator3x), ctypes.POINTER(gpk_coef3),
                         ctypes.POINTER(gpk_bdata3), ctypes.POINTER(gpk_conv3), ctypes.POINTER(gpk_cross3),
                         ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_cross_info3": ([ctypes.c_void_p, _dp], ctypes.c_int),
    "gpk_create3_opb": ([ctypes.POINTER(gpk_problem3), ctypes.POINTER(gpk_operator3x), ctypes.POINTER(gpk_coef3),
                         ctypes.POINTER(gpk_bdata3), ctypes.POINTER(gpk_conv3), ctypes.POINTER(gpk_cross3),
                         ctypes.POINTER(gpk_drift3), ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_drift_info3": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "gpk_create3_oph": ([ctypes.POINTER(gpk_problem3), ctypes.POINTER(gpk_operator3x), ctypes.POINTER(gpk_coef3),
                         ctypes.POINTER(gpk_bdata3), ctypes.POINTER(gpk_conv3), ctypes.POINTER(gpk_cross3),
                         ctypes.POINTER(gpk_drift3), ctypes.POINTER(gpk_high3), ctypes.c_double,
                         ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_high_info3": ([ctypes.c_void_p, _dp, _dp], ctypes.c_int),
    "gpk_create3_opq": ([ctypes.POINTER(gpk_problem3), ctypes.POINTER(gpk_operator3x), ctypes.POINTER(gpk_coef3),
                         ctypes.POINTER(gpk_bdata3), ctypes.POINTER(gpk_conv3), ctypes.POINTER(gpk_cross3),
                         ctypes.POINTER(gpk_drift3), ctypes.POINTER(gpk_high3), ctypes.POINTER(gpk_bicross3),
                         ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_bicross_info3": ([ctypes.c_void_p, _dp], ctypes.c_int),
    "gpk_create3_opg": ([ctypes.POINTER(gpk_problem3), ctypes.POINTER(gpk_operator3x), ctypes.POINTER(gpk_coef3),
                         ctypes.POINTER(gpk_bdata3), ctypes.POINTER(gpk_conv3), ctypes.POINTER(gpk_cross3),
                         ctypes.POINTER(gpk_drift3), ctypes.POINTER(gpk_high3), ctypes.POINTER(gpk_bicross3),
                         ctypes.POINTER(gpk_gradsq3), ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
    "gpk_gradsq_info3": ([ctypes.c_void_p, _dp, _dp], ctypes.c_int),
    "gpk_destroy3": ([ctypes.c_void_p], ctypes.c_int),
    "gpk_num_params3": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)], ctypes.c_int),
    "gpk_set_params3": ([ctypes.c_void_p, _dp, ctypes.c_int64], ctypes.c_int),
    "gpk_get_params3": ([ctypes.c_void_p, _dp, ctypes.c_int64], ctypes.c_int),
    "gpk_loss_grad3": ([ctypes.c_void_p, _dp, _dp], ctypes.c_int),
    "gpk_step3": ([ctypes.c_void_p, ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_set_opt_state3": ([ctypes.c_void_p, ctypes.c_int64, _dp, _dp, ctypes.c_int64], ctypes.c_int),
    "gpk_get_opt_state3": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), _dp, _dp,
                            ctypes.c_int64], ctypes.c_int),
    "gpk_predict3": ([ctypes.c_void_p, _dp, ctypes.c_int32, _dp, ctypes.c_int32, _dp, ctypes.c_int32,
                      _dp], ctypes.c_int),
    "gpk_predict_deriv3": ([ctypes.c_void_p, _dp, ctypes.c_int32, _dp, ctypes.c_int32, _dp, ctypes.c_int32,
                            _ip, _dp], ctypes.c_int),
    "gpk_evaluate3": ([ctypes.c_void_p, _dp, ctypes.c_int64, _ip, _dp], ctypes.c_int),
    "gpk_criterion3": ([ctypes.c_void_p, _dp], ctypes.c_int),
    "gpk_stage_variants3": ([ctypes.c_void_p, _ip, ctypes.c_int32, _ip], ctypes.c_int),
    "gpk_loss_terms3": ([ctypes.c_void_p, _dp], ctypes.c_int),
    "gpk_refine_info3": ([ctypes.c_void_p, _dp, _ip, _ip], ctypes.c_int),
    "gpk_refine_panel": ([ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _dp, _dp, _dp, _dp,
                          ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_mode_gemm": ([ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                       ctypes.c_int32, ctypes.c_double, _dp, _dp, ctypes.c_double, _dp, _dp,
                       ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_point_contract": ([ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_int32, _dp, ctypes.c_int32, _dp, _dp,
                            _dp, ctypes.c_int32, _dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                            ctypes.c_int32, _dp, ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_assemble_pairs": ([ctypes.c_int32, _dp, ctypes.c_int32, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_double,
                            ctypes.c_double, ctypes.c_double, _dp, _dp], ctypes.c_int),
    "gpk_assemble_pairs2": ([ctypes.c_int32, _dp, ctypes.c_int32, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_double,
                             ctypes.c_double, ctypes.c_double, _dp, _dp, _dp], ctypes.c_int),
    "gpk_assemble_pairs4": ([ctypes.c_int32, _dp, ctypes.c_int32, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_double,
                             ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _dp, _dp, _dp],
                            ctypes.c_int),
    "gpk_assemble_pairs5": ([ctypes.c_int32, _dp, ctypes.c_int32, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_double,
                             ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _dp, _dp, _dp, _dp],
                            ctypes.c_int),
    "gpk_assemble_pairs_time": ([ctypes.c_int32, _dp, ctypes.c_int32, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_double,
                                 ctypes.c_double, ctypes.c_int32, ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_dgemm": ([ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, _dp,
                   ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                   ctypes.c_double, _dp, ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_int32, ctypes.c_int32,
                   ctypes.c_double, _dp, _dp, ctypes.c_int32, ctypes.c_int32, _dp], ctypes.c_int),
    "gpk_dgemm_epi": ([ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(gpk_gemm_case), ctypes.c_double],
                      ctypes.c_int),
    "gpk_dgemv_epi": ([ctypes.c_int32, ctypes.c_int32, _dp, _ip, _dp, ctypes.c_int32, ctypes.c_double,
                       ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_double, _dp, ctypes.c_double,
                       ctypes.c_int32, ctypes.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_int32, _dp],
                      ctypes.c_int),
    "gpk_wide_schedule": ([ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int64],
                          ctypes.c_int),
    "gpk_trace_reset": ([], ctypes.c_int),
    "gpk_trace_read": ([ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                        ctypes.c_int32], ctypes.c_int),
}

_LIB = None


def load():
    """Load libgpk.so (raises if it has not been built — no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GPKError(GPK_ENODEV, f"{LIB_PATH} not built; run __graft_entry__.build() "
                                       "or `make -C gaussian-process-slover-for-high-freq-pde_amd/csrc`")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in EXPORTS.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _LIB = lib
    return _LIB


def check(rc):
    if rc != GPK_OK:
        msg = load().gpk_last_error().decode(errors="replace")
        if rc == GPK_ENOTPD:
            raise NotPositiveDefinite(rc, msg)
        raise GPKError(rc, msg)


def dptr(a):
    return a.ctypes.data_as(_dp)


def f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


GEMM_AUTO, GEMM_SMALL, GEMM_BIG, GEMM_TILE128 = 0, 1, 2, 3


def dgemm(A, B, ta=False, tb=False, alpha=1.0, A2=None, B2=None, ta2=False, tb2=False, alpha2=1.0,
          beta=0.0, C0=None, variant=GEMM_AUTO, iters=0):
    """The step's fp64 MFMA GEMM kernels (gpk_dgemm) on host arrays: returns (C, avg_us) with
    C = alpha op(A) op(B) [+ alpha2 op(A2) op(B2)] [+ beta C0]; avg_us is the average device time
    of `iters` back-to-back launches (None when iters = 0).  Dimensions must be multiples of 32."""
    A, B = f64(A), f64(B)
    M, K = (A.shape[1], A.shape[0]) if ta else A.shape
    N = B.shape[0] if tb else B.shape[1]
    C = np.zeros((M, N)) if C0 is None else f64(C0).copy()
    K2, pa2, pb2, lda2, ldb2 = 0, None, None, 1, 1
    if A2 is not None:
        A2, B2 = f64(A2), f64(B2)
        K2 = A2.shape[0] if ta2 else A2.shape[1]
        pa2, pb2, lda2, ldb2 = dptr(A2), dptr(B2), A2.shape[1], B2.shape[1]
    us = ctypes.c_double(0.0)
    check(load().gpk_dgemm(variant, M, N, K, alpha, dptr(A), A.shape[1], int(ta), dptr(B), B.shape[1],
                           int(tb), K2, alpha2, pa2, lda2, int(ta2), pb2, ldb2, int(tb2), beta,
                           dptr(C) if C0 is not None else None, dptr(C), N, iters,
                           ctypes.byref(us) if iters else None))
    return C, (us.value if iters else None)


EPI_STORE, EPI_RESID, EPI_QUAD = 0, 1, 2  # include/gpk.h GPK_EPI_*
GATE_NONE, GATE_OPEN, GATE_CLOSED = 0, 1, 2  # GPK_GATE_*
GEMM_TILE_SIDE = {GEMM_SMALL: 16, GEMM_BIG: 64, GEMM_TILE128: 128}
SENTINEL = -1.25e300  # what dgemm_epi / dgemv_epi fill their outputs with before the launch


def _padded(a, pad):
    """A C-contiguous copy of the 2D array a in a buffer with `pad` more columns (SENTINEL there);
    returns (buffer, view of the copy)."""
    a = np.asarray(a, dtype=np.float64)
    buf = np.full((a.shape[0], a.shape[1] + pad), SENTINEL)
    buf[:, :a.shape[1]] = a
    return buf, buf[:, :a.shape[1]]


def gemm_case_shape(c):
    """(M, N, K, K2) of a dgemm_epi case."""
    A, B = np.asarray(c["A"]), np.asarray(c["B"])
    M, K = (A.shape[1], A.shape[0]) if c.get("ta") else A.shape
    N = B.shape[0] if c.get("tb") else B.shape[1]
    K2 = 0
    if c.get("A2") is not None:
        A2 = np.asarray(c["A2"])
        K2 = A2.shape[0] if c.get("ta2") else A2.shape[1]
    return M, N, K, K2


def dgemm_epi(variant, cases, v=1.0, spare=2):
    """One launch of the step's GEMM kernels with their fused epilogues (gpk_dgemm_epi) on a batch of
    1..4 cases.  A case is a dict: A, B [ta, tb], optional second product A2, B2 [ta2, tb2], alpha,
    alpha2, beta, C0 [inplace: C0 is passed as C itself], epi [ac, F, U, Q1, Q2], vscale, vscale2,
    Ys (asks for the side output Y), red / red2 (True asks for the partials), gate, and pad (extra
    columns in every array's leading dimension).  Outputs are filled with SENTINEL before the call
    (C with C0 when inplace); the partial arrays have `spare` entries beyond the tile count.
    Returns one dict per case: C, Y, red, red2 (None where not asked for), tiles, and the whole
    padded buffers C_buf, Y_buf."""
    n = len(cases)
    arr = (gpk_gemm_case * max(n, 1))()
    outs, keep = [], []
    for g, c in zip(arr, cases):
        pad = int(c.get("pad", 0))
        M, N, K, K2 = gemm_case_shape(c)
        g.M, g.N, g.K, g.K2 = M, N, K, K2

        def put(name, ldname=None):
            if c.get(name) is None:
                return None
            buf, view = _padded(c[name], pad)
            keep.append(buf)
            setattr(g, name, dptr(buf))
            if ldname:
                setattr(g, ldname, buf.shape[1])
            return view

        put("A", "lda"), put("B", "ldb"), put("A2", "lda2"), put("B2", "ldb2")
        put("F", "ldf"), put("U", "ldf"), put("Q1", "ldf"), put("Q2", "ldf"), put("Ys", "ldy")
        g.ta, g.tb, g.ta2, g.tb2 = (int(bool(c.get(k))) for k in ("ta", "tb", "ta2", "tb2"))
        g.alpha, g.alpha2, g.beta = float(c.get("alpha", 1.0)), float(c.get("alpha2", 1.0)), float(c.get("beta", 0.0))
        g.epi, g.ac = int(c.get("epi", EPI_STORE)), int(bool(c.get("ac")))
        g.vscale, g.vscale2, g.gate = int(bool(c.get("vscale"))), int(bool(c.get("vscale2"))), int(c.get("gate", GATE_NONE))
        inplace = bool(c.get("inplace"))
        Cbuf, C = _padded(c["C0"] if inplace else np.full((M, N), SENTINEL), pad)
        g.C, g.ldc = dptr(Cbuf), Cbuf.shape[1]
        if inplace:
            g.C0, g.ldc0 = g.C, g.ldc
        else:
            put("C0", "ldc0")
        out = {"C": C, "C_buf": Cbuf, "Y": None, "Y_buf": None, "red": None, "red2": None}
        if c.get("Ys") is not None:
            out["Y_buf"], out["Y"] = _padded(np.full((M, N), SENTINEL), pad)
            g.Y = dptr(out["Y_buf"])
        t = GEMM_TILE_SIDE.get(variant, 16)
        g.red_cap = -(-M // t) * -(-N // t) + spare
        for name in ("red", "red2"):
            if c.get(name):
                out[name] = np.full(g.red_cap, SENTINEL)
                setattr(g, name, dptr(out[name]))
        outs.append(out)
    check(load().gpk_dgemm_epi(int(variant), n, arr, float(v)))
    for g, out in zip(arr, outs):
        out["tiles"] = g.tiles
    return outs


def dgemv_epi(x, A=None, cid=None, cv=None, cdiag=0.0, ident=0, rows=None, alpha=1.0, C0=None, inplace=False,
              beta=0.0, epi=EPI_STORE, ac=False, F=None, U=None, U0=None, Q1=None, Q2=None, red=False,
              red2=False, gate=GATE_NONE, pad=0):
    """One launch of the step's GEMV with its epilogues (gpk_dgemv_epi): y = alpha A x + ... for the
    matrix A (rows x p) or the class form (cid int32 rows x p, cv, cdiag, ident).  inplace passes C0
    as y itself; pad adds columns to the operand's leading dimension.  y and the partials are
    filled with SENTINEL before the call.  Returns (y, red, red2), None where not asked for."""
    x = f64(x).reshape(-1)
    p = x.size
    op = np.asarray(A if A is not None else cid)
    rows = op.shape[0] if rows is None else int(rows)
    if A is not None:
        opbuf, _ = _padded(np.asarray(A)[:rows], pad)
        pa, pc, pv, ncls = dptr(opbuf), None, None, 0
    else:
        opbuf = np.full((rows, op.shape[1] + pad), -1, dtype=np.int32)
        opbuf[:, :op.shape[1]] = op[:rows]
        cv = f64(cv).reshape(-1)
        pa, pc, pv, ncls = None, opbuf.ctypes.data_as(_ip), dptr(cv), cv.size
    vec = {k: (None if a is None else f64(a).reshape(-1)) for k, a in
           dict(C0=C0, F=F, U=U, U0=U0, Q1=Q1, Q2=Q2).items()}
    y = vec["C0"].copy() if inplace else np.full(rows, SENTINEL)
    ptr = {k: (None if a is None else dptr(a)) for k, a in vec.items()}
    if inplace:
        ptr["C0"] = dptr(y)
    nblk = (rows + 3) // 4
    r1 = np.full(nblk, SENTINEL) if red else None
    r2 = np.full(nblk, SENTINEL) if red2 else None
    check(load().gpk_dgemv_epi(p, rows, pa, pc, pv, ncls, float(cdiag), int(ident), opbuf.shape[1], dptr(x),
                               float(alpha), ptr["C0"], float(beta), int(epi), int(bool(ac)), ptr["F"], ptr["U"],
                               ptr["U0"], ptr["Q1"], ptr["Q2"], None if r1 is None else dptr(r1),
                               None if r2 is None else dptr(r2), int(gate), dptr(y)))
    return y, r1, r2


MODE_SLAB, MODE_PERMUTE, MODE_SLAB32, MODE_SLAB64 = 0, 1, 2, 3


def mode_gemm(Mat, T, k, alpha=1.0, beta=0.0, C0=None, inplace=False, variant=MODE_SLAB, iters=0):
    """One mode-k product (gpk_mode_gemm) on host arrays: returns (C, avg_us) with
    C = alpha (Mat x_k T) [+ beta C0], T a 3-axis array, Mat (m, T.shape[k - 1]), k in 1..3.
    inplace: C0 is passed as C itself (the in-place update).  Mode 2: variant MODE_SLAB is the
    slab-batched kernel, MODE_PERMUTE the permute -> GEMM -> permute route.  Sizes are multiples
    of 32; avg_us is None when iters = 0."""
    Mat, T = f64(Mat), f64(T)
    d1, d2, d3 = T.shape
    m = Mat.shape[0]
    shape = [d1, d2, d3]
    if 1 <= k <= 3:  # (the library rejects any other k)
        shape[k - 1] = m
    C = np.zeros(shape) if C0 is None else f64(C0).copy().reshape(shape)
    c0 = None
    if C0 is not None:
        c0 = C if inplace else f64(C0).copy().reshape(shape)
    us = ctypes.c_double(0.0)
    check(load().gpk_mode_gemm(int(variant), int(k), d1, d2, d3, m, float(alpha), dptr(Mat), dptr(T),
                               float(beta), dptr(c0) if c0 is not None else None, dptr(C), int(iters),
                               ctypes.byref(us) if iters else None))
    return C, (us.value if iters else None)


def refine_panel(Kinv, Kc, B, X, side=0, route=REFINE_FUSED, iters=0):
    """One refinement step on host operands (gpk_refine_panel): (X + Kinv (B - Kc X), avg_us) for
    side 0 (X, B: P x M), (X + (B - X Kc) Kinv, avg_us) for side 1 (X, B: M x P); route REFINE_GEMM
    or REFINE_FUSED; avg_us is None when iters = 0."""
    Kinv, Kc, B = f64(Kinv), f64(Kc), f64(B)
    out = f64(X).copy()
    P = Kinv.shape[0]
    M = out.shape[1] if side == 0 else out.shape[0]
    if Kinv.shape != (P, P) or Kc.shape != (P, P) or B.shape != out.shape or out.shape != ((P, M) if side == 0 else (M, P)):
        raise ValueError("refine_panel: operand shapes do not match")
    us = ctypes.c_double()
    check(load().gpk_refine_panel(int(route), int(side), P, M, dptr(Kinv), dptr(Kc), dptr(B), dptr(out),
                                  int(iters), ctypes.byref(us)))
    return out, (us.value if iters else None)


def deriv_orders(deriv, dim):
    """`deriv` as a tuple of dim ints (an int is accepted for dim 1); the library checks the range."""
    d = (deriv,) if isinstance(deriv, (int, np.integer)) else tuple(deriv)
    if len(d) != dim:
        raise ValueError("deriv needs one order per axis (%d)" % dim)
    return tuple(int(v) for v in d)


def point_contract(kind, t, x, paras, T, C=1, sp=None, sj=None, sc=1, deriv=0, iters=0):
    """The scattered-point contraction on host operands (gpk_point_contract): (out, avg_us) with
    out[p, c] = sum_{j < n} field(t[p], x[j]) T.flat[p sp + j sj + c sc], field = kappa / D_x1_kappa
    / DD_x1_kappa for deriv 0 / 1 / 2 at the kernel parameters `paras`, out (m, C).  The default
    strides read T as a contiguous [m][n][C] array (sj = C, sp = n C); sp = 0 broadcasts one [n][C]
    block to every point.  avg_us is None when iters = 0."""
    t, x, T = f64(t).reshape(-1), f64(x).reshape(-1), f64(T).reshape(-1)
    lw, ll, fr = (f64(paras[k]).reshape(-1) for k in ("log-w", "log-ls", "freq"))
    m, n, C = t.size, x.size, int(C)
    sj = C if sj is None else int(sj)
    sp = n * sj if sp is None else int(sp)
    if min(m, n, C) > 0 and sp >= 0 and sj > 0 and sc > 0 and T.size < (m - 1) * sp + (n - 1) * sj + (C - 1) * sc + 1:
        raise ValueError("point_contract: T is shorter than the strides address")
    out = np.empty((max(m, 1), max(C, 1)))
    us = ctypes.c_double()
    k = KIND_IDS[kind] if isinstance(kind, str) else int(kind)
    check(load().gpk_point_contract(k, int(deriv), dptr(t), m, dptr(x), n, dptr(lw), dptr(ll), dptr(fr),
                                    lw.size, dptr(T), sp, sj, int(sc), C, dptr(out), int(iters),
                                    ctypes.byref(us)))
    return out, (us.value if iters else None)


def assemble_pairs(kind, x, paras, jitter=0.0, c2=1.0, c1=0.0):
    """The step's per-pair assembly kernel on one axis (gpk_assemble_pairs): (K, D), both (n, n).
    c1 == 0: D = DD_x1_kappa; c2 == 0: D = D_x1_kappa (both unweighted, as the step assembles them);
    otherwise the mixed block c2 DD_x1_kappa + c1 D_x1_kappa."""
    x = f64(x).reshape(-1)
    lw, ll, fr = (f64(paras[k]).reshape(-1) for k in ("log-w", "log-ls", "freq"))
    n = x.size
    K, D = np.empty((max(n, 1), max(n, 1))), np.empty((max(n, 1), max(n, 1)))
    k = KIND_IDS[kind] if isinstance(kind, str) else int(kind)
    check(load().gpk_assemble_pairs(k, dptr(x), n, dptr(lw), dptr(ll), dptr(fr), lw.size, float(jitter),
                                    float(c2), float(c1), dptr(K), dptr(D)))
    return K, D


def assemble_pairs2(kind, x, paras, jitter=0.0, c2=1.0, c1=0.0):
    """The two-block mode of the same kernel (gpk_assemble_pairs2), which a convective axis
    assembles in: (K, D, D1), D = c2 DD_x1_kappa + c1 D_x1_kappa at any weights, D1 = D_x1_kappa."""
    x = f64(x).reshape(-1)
    lw, ll, fr = (f64(paras[k]).reshape(-1) for k in ("log-w", "log-ls", "freq"))
    n = x.size
    K, D, D1 = (np.empty((max(n, 1), max(n, 1))) for _ in range(3))
    k = KIND_IDS[kind] if isinstance(kind, str) else int(kind)
    check(load().gpk_assemble_pairs2(k, dptr(x), n, dptr(lw), dptr(ll), dptr(fr), lw.size, float(jitter),
                                     float(c2), float(c1), dptr(K), dptr(D), dptr(D1)))
    return K, D, D1


def assemble_pairs4(kind, x, paras, jitter=0.0, c4=0.0, c3=0.0, c2=1.0, c1=0.0, split=False):
    """The high-order modes of the same kernel (gpk_assemble_pairs4), which an axis with a third- or
    fourth-order term assembles in: (K, D), D = c4 D4 + c3 D3 + c2 DD_x1_kappa + c1 D_x1_kappa at any
    weights; split: the two-block mode, (K, D, D1) with D1 = D_x1_kappa."""
    x = f64(x).reshape(-1)
    lw, ll, fr = (f64(paras[k]).reshape(-1) for k in ("log-w", "log-ls", "freq"))
    n = x.size
    K, D, D1 = (np.empty((max(n, 1), max(n, 1))) for _ in range(3))
    k = KIND_IDS[kind] if isinstance(kind, str) else int(kind)
    check(load().gpk_assemble_pairs4(k, dptr(x), n, dptr(lw), dptr(ll), dptr(fr), lw.size, float(jitter),
                                     float(c4), float(c3), float(c2), float(c1), dptr(K), dptr(D),
                                     dptr(D1) if split else None))
    return (K, D, D1) if split else (K, D)


def assemble_pairs5(kind, x, paras, jitter=0.0, c4=0.0, c3=0.0, c2=1.0, c1=0.0, split=False):
    """The modes an axis of a bi-pair assembles in (gpk_assemble_pairs5): assemble_pairs4's blocks and
    D2 = DD_x1_kappa alone: (K, D, D2), or with split (K, D, D1, D2)."""
    x = f64(x).reshape(-1)
    lw, ll, fr = (f64(paras[k]).reshape(-1) for k in ("log-w", "log-ls", "freq"))
    n = x.size
    K, D, D1, D2 = (np.empty((max(n, 1), max(n, 1))) for _ in range(4))
    k = KIND_IDS[kind] if isinstance(kind, str) else int(kind)
    check(load().gpk_assemble_pairs5(k, dptr(x), n, dptr(lw), dptr(ll), dptr(fr), lw.size, float(jitter),
                                     float(c4), float(c3), float(c2), float(c1), dptr(K), dptr(D),
                                     dptr(D1) if split else None, dptr(D2)))
    return (K, D, D1, D2) if split else (K, D, D2)


def assemble_pairs_time(kind, x, paras, c2=1.0, c1=0.0, split=False, iters=200):
    """Mean device time in us of the per-pair assembly launch (gpk_assemble_pairs_time): the mode
    c2 and c1 select, or with split modes 2 and 1 as two launches."""
    x = f64(x).reshape(-1)
    lw, ll, fr = (f64(paras[k]).reshape(-1) for k in ("log-w", "log-ls", "freq"))
    us = ctypes.c_double()
    k = KIND_IDS[kind] if isinstance(kind, str) else int(kind)
    check(load().gpk_assemble_pairs_time(k, dptr(x), x.size, dptr(lw), dptr(ll), dptr(fr), lw.size, float(c2),
                                         float(c1), int(bool(split)), int(iters), ctypes.byref(us)))
    return us.value
