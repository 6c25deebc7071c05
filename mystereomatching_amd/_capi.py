"""ctypes binding of the C-ABI in include/sm_capi.h (libsm_hip.so, built in-tree).

The HIP library is the only compute path: if it is missing or fails to load this module raises;
there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsm_hip.so")

SM_OK, SM_EINVAL, SM_ENOMEM, SM_EHIP, SM_ESTATE = 0, 1, 2, 3, 4
# costCalculate's strings (cpp:954-987) with sm_cost_method's values; "ZNCC" (7, reserved) is left out on
# purpose: the reference's ZNCC volume is undefined on a border frame
COST_METHODS = {"censusGrad": 0, "Census": 1, "ADCensus": 2, "AD": 3, "SD": 4, "BT": 5, "grad": 6, "TruncAD": 8,
                "adGrad": 9, "ADCensusGrad": 10}
AGGREGATIONS = {"": 0, "none": 0, "CBCA": 1, "GF": 2, "NL": 3, "FIF": 5, "AWS": 7,
                "BF": 9, "GFNL": 10}   # 4, 6 and 8 are reserved
FIF_IMPROVE, FIF_PLAIN = 0, 1
AWS_DEFAULTS = (17, 17, 5.0)   # radius_v, radius_u, gamma_c (sm_aws_config)
BF_DEFAULTS = (12, 12)         # ksize_v, ksize_u (sm_bf_config)
GFNL_VAR_THRESH = 400.0        # sm_gfnl_config
CBCA_DW_DEFAULTS = (23, 23, 30, 0, 5.0)   # arm_l2, arm_l_out2, arm_c_thresh2, arm_c_thresh_out2, arm_len_thres
SE_REFERENCE, SE_FLOAT = 0, 1
# sm_refine_ext_config's values when a stage is on: pkr_ratio, disp_pkr, bg_ipl_depth, se_mode
REFINE_EXT_DEFAULTS = (0.1, -64, 1000, SE_REFERENCE)
# sm_refine_da_config's values: canny_low, canny_high, blur_side, blur_centre
REFINE_DA_DEFAULTS = (20, 60, 84, 87)
# sm_refine_outlier_config's values: disp_mis (DISP_MIS, h:217), interpolate_type (interpolateType, h:310)
REFINE_OUTLIER_DEFAULTS = (-48, 0)
OPTIMIZATIONS = {"": 0, "wta": 0, "sgm": 1, "so": 2}
# sm_so_config: the scan-line optimiser behind optimization "so" (the call commented in at cpp:1096-1100) by the
# reference's function name, and the value that keeps a function's own Pn2 / Pn3 literals
SO_VARIANTS = {"so": 0, "so_R2L": 1, "so_T2D": 2}
SO_PN_DEFAULT = -1.0


class sm_params(C.Structure):
    """Mirror of struct sm_params (include/sm_capi.h); field order must match."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("rows", C.c_int32), ("cols", C.c_int32), ("num_disparities", C.c_int32),
        ("cost_method", C.c_int32), ("aggregation", C.c_int32), ("optimization", C.c_int32),
        ("census_rv", C.c_int32), ("census_ru", C.c_int32), ("census_ring", C.c_int32),
        ("lam_cen", C.c_float), ("lam_g", C.c_float), ("grad_trunc", C.c_float),
        ("grad_adaptive", C.c_int32),
        ("lam_ad", C.c_float), ("lam_cen_adc", C.c_float), ("ad_trunc_adc", C.c_float),
        ("ad_trunc_ad", C.c_float),
        ("arm_l", C.c_int32), ("arm_l_out", C.c_int32), ("arm_c_thresh", C.c_int32),
        ("arm_c_thresh_out", C.c_int32), ("arm_min_l", C.c_int32),
        ("cbca_iterations", C.c_int32), ("sgm_paths", C.c_int32),
        ("sgm_p1", C.c_float), ("sgm_p2", C.c_float),
        ("sgm_cor_dif_thres", C.c_int32), ("sgm_redu_coeff", C.c_int32),
        ("compute_right_view", C.c_int32), ("keep_final_volume", C.c_int32),
        ("batch_capacity", C.c_int32),
        ("do_refine", C.c_int32), ("lr_max_diff", C.c_float), ("do_region_vote", C.c_int32),
        ("region_vote_nums", C.c_int32), ("rv_ratio", C.c_float), ("rv_s", C.c_int32),
        ("do_proper_ipol", C.c_int32), ("disp_occ", C.c_int32), ("do_last_median_blur", C.c_int32),
        ("sub_batch", C.c_int32), ("num_streams", C.c_int32), ("fuse_norm_scan", C.c_int32),
        ("gf_eps", C.c_float), ("gf_mode", C.c_int32), ("nl_sigma", C.c_double),
        ("lr_consis", C.c_int32),
        ("placement_trials", C.c_int32),
        ("fuse_cost_scan", C.c_int32),
        ("fif_mode", C.c_int32), ("fif_eps", C.c_float), ("fif_pn", C.c_float),
    ]


class sm_create_opts(C.Structure):
    """Mirror of struct sm_create_opts (include/sm_capi.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("so_float_minima", C.c_int32)]


class sm_stage_err(C.Structure):
    """Mirror of struct sm_stage_err (include/sm_capi.h): one (pair, stage, region) of the error table."""

    _fields_ = [("count", C.c_uint32), ("invalid", C.c_uint32), ("bad", C.c_uint32 * 4), ("sum_sq", C.c_double)]


# the same record as a numpy dtype (StereoBatch.stage_errors)
STAGE_ERR_DTYPE = [("count", "<u4"), ("invalid", "<u4"), ("bad", "<u4", (4,)), ("sum_sq", "<f8")]
EVAL_REGIONS = ("nonocc", "all", "disc")   # I_mask's order (cpp:2073-2075)
EVAL_MAX_THRES = 4


# Every SM_API symbol declared in include/sm_capi.h: (name, restype, argtypes).
_P = C.c_void_p
_u8p = C.POINTER(C.c_uint8)
SIGNATURES = [
    ("sm_params_default", None, [C.POINTER(sm_params), C.c_int32, C.c_int32, C.c_int32]),
    ("sm_create", C.c_int, [C.POINTER(_P), C.POINTER(sm_params), C.c_int32]),
    ("sm_create_opts_default", None, [C.POINTER(sm_create_opts)]),
    ("sm_create_ex", C.c_int, [C.POINTER(_P), C.POINTER(sm_params), C.POINTER(sm_create_opts), C.c_int32]),
    ("sm_destroy", C.c_int, [_P]),
    ("sm_last_error", C.c_char_p, [_P]),
    ("sm_status_string", C.c_char_p, [C.c_int]),
    ("sm_set_images", C.c_int, [_P, _P, _P, C.c_size_t, _P, _P, C.c_size_t]),
    ("sm_cost_calculate", C.c_int, [_P]),
    ("sm_solve_all", C.c_int, [_P, C.c_int32, C.c_float]),
    ("sm_disp_optimize", C.c_int, [_P, _P]),
    ("sm_solve_all_pyr", C.c_int, [C.POINTER(_P), C.c_int32, C.c_float]),
    ("sm_pyr_down", C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    ("sm_pyr_down_f32", C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    ("sm_refine", C.c_int, [_P, _P]),
    ("sm_get_disp", C.c_int, [_P, C.c_int32, _P]),
    ("sm_set_disp", C.c_int, [_P, C.c_int32, _P]),
    ("sm_get_volume", C.c_int, [_P, C.c_int32, _P]),
    ("sm_get_arms", C.c_int, [_P, C.c_int32, _P]),
    ("sm_upload_batch", C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    ("sm_run", C.c_int, [_P, C.c_int32, C.c_float, _P]),
    ("sm_pyramid_config", C.c_int, [_P, C.c_int32]),
    ("sm_pyramid_level", C.c_void_p, [_P, C.c_int32]),
    ("sm_pyramid_levels", C.c_int32, [_P]),
    ("sm_download_disp", C.c_int, [_P, C.c_int32, _P]),
    ("sm_download_disp_async", C.c_int, [_P, C.c_int32, _P]),
    ("sm_upload_batch_async", C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    ("sm_upload_wait", C.c_int, [_P]),
    ("sm_download_wait", C.c_int, [_P, C.c_int32]),
    ("sm_run_batch", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_float, _P]),
    ("sm_run_batch_multi", C.c_int, [C.POINTER(_P), C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_float, _P]),
    ("sm_set_schedule", C.c_int, [_P, C.c_int32, C.c_int32]),
    ("sm_placement_trials_ms", C.c_int32, [_P, C.POINTER(C.c_double), C.c_int32]),
    ("sm_placement_kept", C.c_int32, [_P]),
    ("sm_synchronize", C.c_int, [_P]),
    ("sm_stream", C.c_void_p, [_P]),
    ("sm_profile_enable", C.c_int, [_P, C.c_int32]),
    ("sm_profile_read", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.POINTER(C.c_int32)]),
    ("sm_profile_reset", C.c_int, [_P]),
    ("sm_cal_err", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("sm_expf_host", C.c_float, [C.c_float]),
    ("sm_expf_device_range", C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    ("sm_div_area_check", C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    ("sm_copy_ceiling", C.c_int, [_P, C.c_uint64, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("sm_get_census", C.c_int, [_P, C.c_int32, _P]),
    ("sm_aws_config", C.c_int, [_P, C.c_int32, C.c_int32, C.c_float]),
    ("sm_bgr2lab_host", None, [_P, C.c_size_t, _P]),
    ("sm_get_aws_lab", C.c_int, [_P, C.c_int32, _P]),
    ("sm_bf_config", C.c_int, [_P, C.c_int32, C.c_int32]),
    ("sm_gfnl_config", C.c_int, [_P, C.c_float]),
    ("sm_get_gfnl_mask", C.c_int, [_P, _P]),
    ("sm_vmtop_config", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32]),
    ("sm_set_volume", C.c_int, [_P, C.c_int32, _P]),
    ("sm_get_top_disp", C.c_int, [_P, C.c_int32, _P]),
    ("sm_cbca_double_config", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float]),
    ("sm_get_cbca_dw_mask", C.c_int, [_P, _P]),
    ("sm_cbca_intersect_config", C.c_int, [_P, C.c_int32]),
    ("sm_get_cbca_area", C.c_int, [_P, C.c_int32, _P]),
    ("sm_refine_ext_config", C.c_int, [_P, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("sm_get_pkr_mask", C.c_int, [_P, _P]),
    ("sm_get_subpixel", C.c_int, [_P, _P]),
    ("sm_download_subpixel", C.c_int, [_P, C.c_int32, _P]),
    ("sm_refine_da_config", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("sm_get_da_edges", C.c_int, [_P, _P]),
    ("sm_da_run_image", C.c_int, [_P, _P, C.c_int32, _P, _P, _P]),
    ("sm_set_da_edges", C.c_int, [_P, _P]),
    ("sm_refine_outlier_config", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("sm_get_lrc_mask", C.c_int, [_P, _P]),
    ("sm_so_config", C.c_int, [_P, C.c_int32, C.c_float, C.c_float]),
    ("sm_eval_config", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    ("sm_upload_truth", C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    ("sm_eval_stage_count", C.c_int32, [_P]),
    ("sm_eval_stage_name", C.c_char_p, [_P, C.c_int32]),
    ("sm_get_stage_errors", C.c_int, [_P, C.c_int32, _P]),
    ("sm_get_stage_maps", C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    ("sm_eval_stage_host", None, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), _P]),
]

_lib = None


def load() -> C.CDLL:
    """Load libsm_hip.so (raises OSError/FileNotFoundError when absent: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # SM_HIP_LIB: an alternative build of the same library (tuning sweeps, tools/build_variants.sh)
    path = os.environ.get("SM_HIP_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C mystereomatching_amd/csrc`")
    lib = C.CDLL(path)
    for name, res, args in SIGNATURES:
        if path != LIB_PATH and not hasattr(lib, name):
            continue  # an older tuning build may predate a diagnostic entry point
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class SMError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"sm status {status}: {msg}")
        self.status = status


def check(lib, ctx, status: int, what: str = ""):
    if status != SM_OK:
        msg = lib.sm_last_error(ctx).decode() if ctx else lib.sm_status_string(status).decode()
        raise SMError(status, f"{what}: {msg}" if what else msg)


def default_params(max_disp: int, rows: int, cols: int, **overrides) -> sm_params:
    lib = load()
    p = sm_params()
    lib.sm_params_default(C.byref(p), max_disp, rows, cols)
    for k, v in overrides.items():
        if k == "cost_method" and isinstance(v, str):
            v = COST_METHODS[v]
        elif k == "aggregation" and isinstance(v, str):
            v = AGGREGATIONS[v]
        elif k == "optimization" and isinstance(v, str):
            v = OPTIMIZATIONS[v]
        if not hasattr(p, k):
            raise AttributeError(f"sm_params has no field {k!r}")
        setattr(p, k, v)
    return p


def create_opts(so_float_minima: bool = False) -> sm_create_opts:
    """What sm_create_opts_default fills in, then the fields given."""
    o = sm_create_opts()
    o.struct_size = C.sizeof(sm_create_opts)
    o.so_float_minima = int(bool(so_float_minima))
    return o


# cost methods with a gradient term: BF's box sums over them are not exact (sm_validate.cpp, cost_has_grad_ext)
_BF_INEXACT_COSTS = (COST_METHODS["grad"], COST_METHODS["adGrad"], COST_METHODS["ADCensusGrad"])


def so_needs_float_minima(p: sm_params) -> bool:
    """The combinations sm_create refuses and sm_create_ex with so_float_minima = 1 runs: optimization "so" after GF or
    GFNL, or after BF with inexact sums (a gradient cost method, or AD / SD with ad_trunc_ad off the 2^-25 grid or
    above 1024: bf_exact in sm_validate.cpp).  The reference runs them without a switch, so the facades take this
    for their automatic setting."""
    if p.optimization != OPTIMIZATIONS["so"]:
        return False
    if p.aggregation in (AGGREGATIONS["GF"], AGGREGATIONS["GFNL"]):
        return True
    if p.aggregation != AGGREGATIONS["BF"]:
        return False
    if p.cost_method in _BF_INEXACT_COSTS:
        return True
    if p.cost_method not in (COST_METHODS["AD"], COST_METHODS["SD"]):
        return False
    t = float(p.ad_trunc_ad)
    return not (t <= 1024.0 and math.ldexp(t, 25) == math.floor(math.ldexp(t, 25)))


def create(lib, p: sm_params, device: int, so_float_minima=None):
    """sm_create, or sm_create_ex where the float-minima optimisers are asked for (True), or needed and not refused
    (None: automatic).  Returns (ctx, status, the entry point's name)."""
    ctx = C.c_void_p()
    fm = so_needs_float_minima(p) if so_float_minima is None else bool(so_float_minima)
    if not fm:
        return ctx, lib.sm_create(C.byref(ctx), C.byref(p), device), "sm_create"
    o = create_opts(so_float_minima=True)
    return ctx, lib.sm_create_ex(C.byref(ctx), C.byref(p), C.byref(o), device), "sm_create_ex"


def ptr(a):
    """Raw data pointer of a C-contiguous numpy array."""
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return C.c_void_p(a.ctypes.data)
