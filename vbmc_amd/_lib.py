"""ctypes binding of libvbmc_hip.so (include/vbmc_hip.h).

The product path has NO CPU fallback: importing this module without the built
library, or creating a Context without a gfx950 device, raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

# (GPU_MAX_HW_QUEUES: raised by the library itself, inside vbmc_ctx_create ahead of its first HIP call -- round 5; importing this module no
# longer touches the process environment.  An application that initialises another HIP user first -- bench.py imports torch -- sets it
# itself.)

_HERE = os.path.dirname(os.path.abspath(__file__))
# VBMC_HIP_LIB: an alternative build of the SAME library (kernel A/B experiments, tools/ent_experiments.py)
LIB_PATH = os.environ.get("VBMC_HIP_LIB") or os.path.join(_HERE, "lib", "libvbmc_hip.so")

ABI_VERSION = 8   # include/vbmc_hip.h: VBMC_ABI_VERSION
# the launch forms vbmc_ctx_last_launch reports (include/vbmc_hip.h: VBMC_ENTFORM_* / VBMC_LJFORM_*; 0: none ran)
ENTFORM_LB, ENTFORM_VALU, ENTFORM_MFMA, ENTFORM_LANE = 1, 2, 3, 4
LJFORM_VALU_WAVE, LJFORM_VALU_SPLIT, LJFORM_MFMA_GRAD, LJFORM_MFMA_VALUE, LJFORM_ROLE_MFMA, LJFORM_ROLE_LANE = 1, 2, 3, 4, 5, 6
VBMC_OK, VBMC_ERR_INVALID, VBMC_ERR_NO_DEVICE, VBMC_ERR_HIP, VBMC_ERR_UNSUPPORTED, VBMC_ERR_NOT_POSDEF = range(6)
_STATUS_NAMES = {0: "OK", 1: "INVALID", 2: "NO_DEVICE", 3: "HIP", 4: "UNSUPPORTED", 5: "NOT_POSDEF"}


class VbmcHipError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("libvbmc_hip: %s: %s" % (_STATUS_NAMES.get(status, status), msg))
        self.status = status
        self.message = msg


class VbmcUnsupported(VbmcHipError):
    """Option outside the accelerated path; the caller should fall through to the reference .m."""


_dp = C.POINTER(C.c_double)


def new_args(Struct):
    """An instance of one of the mirrors below with ``struct_size`` set, as every entry point that takes one checks first."""
    return Struct(struct_size=C.sizeof(Struct))


class Limits(C.Structure):
    """vbmc_limits (include/vbmc_hip.h)"""
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in (
        "max_D", "max_K", "max_N", "max_Na", "max_T_vargrad", "delta_ok", "meanfun_mask")]


class ElboArgs(C.Structure):
    """vbmc_elbo_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("D", C.c_int32), ("K", C.c_int32), ("R", C.c_int32),
        ("optimize", C.c_int32 * 4),
        ("theta", _dp),
        ("vp_mu", _dp), ("vp_sigma", _dp), ("vp_lambda", _dp), ("vp_w", _dp), ("vp_delta", _dp),
        ("Ns", C.c_int32),
        ("eps_mode", C.c_int32),
        ("eps", _dp),
        ("eps_shared", C.c_int32),
        ("seed", C.c_uint64),
        ("compute_grad", C.c_int32), ("compute_var", C.c_int32), ("separate_K", C.c_int32),
        ("beta", C.c_double),
        ("bnd_lb", _dp), ("bnd_ub", _dp),
        ("TolCon", C.c_double), ("WeightThreshold", C.c_double), ("WeightPenalty", C.c_double),
        ("sparse_cutoff", C.c_double),
        ("F", _dp), ("dF", _dp), ("G", _dp), ("H", _dp), ("dG", _dp), ("dH", _dp),
        ("varG", _dp), ("varGss", _dp), ("I_sk", _dp), ("J_sjk", _dp),
        ("G_s", _dp), ("varG_s", _dp),
        ("chunk_world", C.c_int32),
        ("restart_offset", C.c_int32), ("restart_stride", C.c_int32),
        ("no_jacobian", C.c_int32),
        ("dvarG", _dp),
        ("dG_s", _dp),
        ("dvarG_s", _dp),
        ("plan_restarts", C.c_int32),
    ]


class SliceArgs(C.Structure):
    """vbmc_slice_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("N", C.c_int32), ("D", C.c_int32), ("Nhyp", C.c_int32), ("meanfun", C.c_int32),
        ("noisefun", C.c_int32 * 3),
        ("X", _dp), ("y", _dp), ("s2", _dp),
        ("prior_mu", _dp), ("prior_sigma", _dp), ("prior_df", _dp),
        ("LB", _dp), ("UB", _dp), ("hyp_start", _dp), ("widths", _dp), ("basewidths", _dp),
        ("Ns", C.c_int32), ("Thin", C.c_int32), ("Burnin", C.c_int32), ("Adaptive", C.c_int32),
        ("W", C.c_int32), ("rng_mode", C.c_int32),
        ("seed", C.c_uint64),
        ("Kmax", C.c_int32),
        ("perms", C.POINTER(C.c_int32)),
        ("uniforms", _dp),
        ("samples", _dp), ("logp", _dp), ("widths_out", _dp),
        ("funccount", C.POINTER(C.c_int64)), ("performed", C.POINTER(C.c_int64)),
        ("max_shrink", C.POINTER(C.c_int32)),
        ("rounds", C.POINTER(C.c_int64)),
    ]


class GpTrainArgs(C.Structure):
    """vbmc_gptrain_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("N", C.c_int32), ("D", C.c_int32), ("Nhyp", C.c_int32), ("meanfun", C.c_int32),
        ("noisefun", C.c_int32 * 3),
        ("X", _dp), ("y", _dp), ("s2", _dp),
        ("prior_mu", _dp), ("prior_sigma", _dp), ("prior_df", _dp),
        ("LB", _dp), ("UB", _dp), ("design", _dp),
        ("Ninit", C.c_int32), ("N0", C.c_int32), ("Nopts", C.c_int32), ("Ncov", C.c_int32),
        ("TolFun", C.c_double),
        ("MaxIter", C.c_int32), ("MaxFunEvals", C.c_int32), ("W", C.c_int32), ("hist_cap", C.c_int32),
        ("fill_fvals", _dp), ("fill_order", C.POINTER(C.c_int32)), ("widths_default", _dp),
        ("hyp", _dp), ("nll", _dp), ("best", C.POINTER(C.c_int32)), ("hyp_start", _dp),
        ("iterations", C.POINTER(C.c_int32)), ("funccount", C.POINTER(C.c_int64)), ("exitflag", C.POINTER(C.c_int32)),
        ("performed", C.POINTER(C.c_int64)),
        ("hist_x", _dp), ("hist_f", _dp), ("hist_k", C.POINTER(C.c_int32)),
    ]


class AcqSearchArgs(C.Structure):
    """vbmc_acqsearch_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("acq_id", C.c_int32), ("K", C.c_int32),
        ("vp_mu", _dp), ("vp_sigma", _dp), ("vp_lambda", _dp), ("vp_w", _dp), ("vp_delta", _dp),
        ("ymax", C.c_double), ("var_regularized", C.c_int32), ("TolGPVar", C.c_double),
        ("gplengthscale", _dp), ("X_rescaled", _dp), ("sn2new", _dp),
        ("x0", _dp), ("insigma", _dp), ("LB", _dp), ("UB", _dp),
        ("TolX", C.c_double), ("TolFun", C.c_double), ("TolHistFun", C.c_double),
        ("MaxFunEvals", C.c_int64),
        ("MaxIter", C.c_int32), ("popsize", C.c_int32), ("rng_mode", C.c_int32), ("Gmax", C.c_int32),
        ("seed", C.c_uint64),
        ("Z", _dp),
        ("chunk", C.c_int32), ("trace_cap", C.c_int32),
        ("xmin", _dp), ("fmin", _dp), ("xbest", _dp), ("fbest", _dp), ("xmean", _dp), ("sigma", _dp), ("C", _dp),
        ("evals", C.POINTER(C.c_int64)), ("generations", C.POINTER(C.c_int32)), ("stop", C.POINTER(C.c_int32)),
        ("rounds", C.POINTER(C.c_int64)),
        ("tr_order", C.POINTER(C.c_int32)), ("tr_F", _dp), ("tr_xmean", _dp), ("tr_sigma", _dp),
    ]


class IsSampleArgs(C.Structure):
    """vbmc_is_sample_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("W", C.c_int32), ("Nm", C.c_int32), ("thin", C.c_int32), ("burnin", C.c_int32), ("spec", C.c_int32),
        ("max_steps", C.c_int32), ("max_shrink", C.c_int32),
        ("x0", _dp), ("LB", _dp), ("UB", _dp),
        ("rng_mode", C.c_int32), ("Mmax", C.c_int32),
        ("seed", C.c_uint64),
        ("U", _dp),
        ("chunk", C.c_int32), ("D", C.c_int32), ("S", C.c_int32), ("reserved_", C.c_int32),
        ("Xa", _dp), ("lnw", _dp), ("fs2a", _dp), ("logp", _dp),
        ("funccount", C.POINTER(C.c_int64)), ("performed", C.POINTER(C.c_int64)), ("rounds", C.POINTER(C.c_int64)),
        ("state", C.POINTER(C.c_void_p)),
    ]


class IsSetupArgs(C.Structure):
    """vbmc_is_setup_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("D", C.c_int32), ("S", C.c_int32), ("K", C.c_int32),
        ("vp_mu", _dp), ("vp_sigma", _dp), ("vp_lambda", _dp), ("vp_w", _dp),
        ("Nvp", C.c_int32), ("Nbox", C.c_int32),
        ("W", C.c_int32), ("Nm", C.c_int32), ("thin", C.c_int32), ("burnin", C.c_int32), ("spec", C.c_int32),
        ("max_steps", C.c_int32), ("max_shrink", C.c_int32), ("chunk", C.c_int32),
        ("rng_mode", C.c_int32), ("Mmax", C.c_int32),
        ("seed", C.c_uint64),
        ("B", _dp), ("U", _dp),
        ("Xa1", _dp), ("lnw1", _dp), ("fs2a1", _dp), ("lpdf1", _dp), ("rect_delta", _dp), ("LB", _dp), ("UB", _dp), ("x0", _dp),
        ("idx0", C.POINTER(C.c_int32)), ("n_bad", C.POINTER(C.c_int32)), ("bad", C.POINTER(C.c_uint8)),
        ("Xa", _dp), ("lnw", _dp), ("fs2a", _dp), ("logp", _dp),
        ("funccount", C.POINTER(C.c_int64)), ("performed", C.POINTER(C.c_int64)), ("rounds", C.POINTER(C.c_int64)),
        ("state", C.POINTER(C.c_void_p)),
    ]


class VpDesc(C.Structure):
    """vbmc_vp_desc (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("D", C.c_int32), ("K", C.c_int32),
        ("mu", _dp), ("sigma", _dp), ("lambda", _dp), ("w", _dp),
        ("type", C.POINTER(C.c_int32)),
        ("lb", _dp), ("ub", _dp), ("tmu", _dp), ("tdelta", _dp), ("scale", _dp), ("R", _dp),
    ]


class MtvArgs(C.Structure):
    """vbmc_mtv_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("nkde", C.c_int32), ("nquad", C.c_int32),
        ("Ns", C.c_int64),
        ("seed", C.c_uint64),
        ("block1", _dp), ("block2", _dp),
        ("mtv", _dp), ("xx1", _dp), ("xx2", _dp), ("mesh", _dp),
        ("counts", C.POINTER(C.c_int32)),
        ("nuniq", C.POINTER(C.c_int64)),
        ("tstar", _dp), ("density", _dp),
    ]


class CornerArgs(C.Structure):
    """vbmc_corner_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("D", C.c_int32), ("res", C.c_int32), ("nbins", C.c_int32), ("nq", C.c_int32), ("origflag", C.c_int32), ("balanceflag", C.c_int32),
        ("reserved_", C.c_int32),
        ("Ns", C.c_int64),
        ("seed", C.c_uint64),
        ("block", _dp), ("X_in", _dp), ("bounds", _dp), ("p", _dp),
        ("xx", _dp), ("bounds_out", _dp),
        ("hist", C.POINTER(C.c_int32)),
        ("quant", _dp), ("density", _dp), ("bandwidth", _dp), ("tstar", _dp),
        ("counts2", C.POINTER(C.c_int32)),
    ]


class DiagArgs(C.Structure):
    """vbmc_diag_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("nkde", C.c_int32), ("nquad", C.c_int32),
        ("Ns", C.c_int64),
        ("seed", C.c_uint64),
        ("kl_mat", _dp), ("mtv", _dp), ("maxmtv_mat", _dp), ("mesh", _dp),
        ("counts", C.POINTER(C.c_int32)),
        ("nuniq", C.POINTER(C.c_int64)),
        ("tstar", _dp), ("density", _dp), ("xx", _dp),
    ]


class ModeArgs(C.Structure):
    """vbmc_mode_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("nmax", C.c_int32), ("origflag", C.c_int32), ("max_iter", C.c_int32),
        ("tol_grad", C.c_double),
        ("x", _dp), ("fval", _dp),
        ("idx", C.POINTER(C.c_int32)), ("S_out", C.POINTER(C.c_int32)), ("start_comp", C.POINTER(C.c_int32)),
        ("f0", _dp), ("us", _dp), ("xs", _dp), ("fs", _dp),
        ("iters", C.POINTER(C.c_int32)), ("nfev", C.POINTER(C.c_int32)), ("stop", C.POINTER(C.c_int32)),
    ]


MODE_STOP = {1: "grad", 2: "step", 3: "maxiter"}     # VBMC_MODE_STOP_*


class GsArgs(C.Structure):
    """vbmc_gs_args (include/vbmc_hip.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("D", C.c_int32), ("S", C.c_int32),
        ("E", C.c_int32), ("W", C.c_int32), ("thin", C.c_int32), ("burnin", C.c_int32), ("spec", C.c_int32),
        ("max_steps", C.c_int32), ("max_shrink", C.c_int32), ("chunk", C.c_int32),
        ("rng_mode", C.c_int32), ("Mmax", C.c_int32), ("origflag", C.c_int32), ("Nnn", C.c_int32), ("reserved_", C.c_int32),
        ("Ns", C.c_int64),
        ("seed", C.c_uint64),
        ("U", _dp), ("LB", _dp), ("UB", _dp), ("x0", _dp),
        ("beta", C.c_double), ("VarThresh", C.c_double),
        ("X_rescaled", _dp), ("gplengthscale", _dp), ("sn2new", _dp),
        ("X", _dp), ("Xt", _dp), ("logp", _dp), ("x0_out", _dp), ("varthresh_out", _dp), ("sn2_avg_out", _dp), ("sn2_nn", _dp),
        ("funccount", C.POINTER(C.c_int64)), ("performed", C.POINTER(C.c_int64)), ("rounds", C.POINTER(C.c_int64)),
    ]


class PredPlanInfo(C.Structure):
    """vbmc_pred_plan_info (include/vbmc_hip.h)"""
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in (
        "num_cu", "slab", "cw", "fused", "QS", "PT", "RS", "npass", "units", "grid", "PZ", "maxg", "nblk", "Rmax", "Rmin")]


class VarLaunchInfo(C.Structure):
    """vbmc_var_launch_info (include/vbmc_hip.h)"""
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in (
        "compute_var", "tri_gemm", "symm", "fwd_solve", "bwd_solve", "solve_width", "gram", "vgrad", "sample_lds", "final_lds")]


VARSOLVE_TRSM2, VARSOLVE_SLAB = 1, 2     # VBMC_VARSOLVE_*
VARGRAM_WAVE, VARGRAM_MFMA = 1, 2        # VBMC_VARGRAM_*

# the host-only generator dumps (no device, no context): the argument types behind the leading uint64 seed
_HOST_DUMPS = {
    "vbmc_slice_rng_dump": [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), _dp],
    "vbmc_acq_search_rng_dump": [C.c_int, C.c_int, C.c_int, _dp],
    "vbmc_acq_is_sample_rng_dump": [C.c_int, C.c_int, C.c_int, _dp],
    "vbmc_acq_is_setup_rng_dump": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp],
    "vbmc_vp_rnd_rng_dump": [C.c_int64, C.c_int, C.c_int, C.c_int, _dp, _dp, C.POINTER(C.c_int64)],
    "vbmc_gp_surrogate_sample_rng_dump": [C.c_int, C.c_int, C.c_int, _dp],
}

_lib = None


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH
        )
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    lib.vbmc_abi_version.restype = C.c_int
    lib.vbmc_get_limits.argtypes = [C.POINTER(Limits)]
    lib.vbmc_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.vbmc_ctx_destroy.argtypes = [vp]
    lib.vbmc_ctx_destroy.restype = None
    lib.vbmc_last_error.argtypes = [vp]
    lib.vbmc_last_error.restype = C.c_char_p
    lib.vbmc_ctx_synchronize.argtypes = [vp]
    lib.vbmc_ctx_set_profiling.argtypes = [vp, C.c_int]
    lib.vbmc_ctx_last_kernel_ms.argtypes = [vp, _dp, _dp]
    lib.vbmc_ctx_last_launch.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.vbmc_ctx_last_variance.argtypes = [vp, C.POINTER(VarLaunchInfo)]
    lib.vbmc_gp_upload.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_uint8), C.POINTER(vp)]
    lib.vbmc_gp_free.argtypes = [vp, vp]
    lib.vbmc_gp_free.restype = None
    lib.vbmc_elbo_batch.argtypes = [vp, vp, C.POINTER(ElboArgs)]
    lib.vbmc_elbo_abandon.argtypes = [vp, C.c_int]
    lib.vbmc_elbo_submit.argtypes = [vp, vp, C.POINTER(ElboArgs), C.c_int]
    lib.vbmc_elbo_collect.argtypes = [vp, C.POINTER(ElboArgs), C.c_int]
    lib.vbmc_adam_batch.argtypes = [vp, vp, C.POINTER(ElboArgs), C.c_double, C.c_int, C.c_double, C.c_double, C.c_double,
                                    _dp, _dp, C.POINTER(C.c_int32), _dp, _dp, _dp]
    lib.vbmc_elbo_shard_size.argtypes = [vp, vp, C.POINTER(ElboArgs), C.c_int, C.POINTER(C.c_size_t)]
    lib.vbmc_elbo_shard_begin.argtypes = [vp, vp, C.POINTER(ElboArgs), C.c_int, C.c_int, vp]
    lib.vbmc_elbo_shard_finish.argtypes = [vp, vp, C.POINTER(ElboArgs), C.c_int, vp]
    lib.vbmc_rng_dump.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, _dp]
    lib.vbmc_entropy_plan.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4
    lib.vbmc_entropy_plan.restype = C.c_int
    lib.vbmc_pred_plan.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PredPlanInfo)]
    lib.vbmc_pred_plan.restype = C.c_int
    lib.vbmc_device_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.vbmc_device_free.argtypes = [vp, vp]
    lib.vbmc_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    lib.vbmc_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    i32p = C.POINTER(C.c_int32)
    u8p = C.POINTER(C.c_uint8)
    lib.vbmc_gp_set_noise.argtypes = [vp, vp, i32p, _dp]
    lib.vbmc_gp_post.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p, _dp, _dp, _dp, _dp,
                                 _dp, _dp, _dp, _dp, u8p, C.POINTER(vp)]
    lib.vbmc_gp_pred.argtypes = [vp, vp, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp]
    lib.vbmc_gp_rank1_solves.argtypes = [vp, vp, _dp, _dp, _dp, _dp]
    lib.vbmc_gp_rank1_update.argtypes = [vp, vp, _dp, C.c_double, _dp, _dp, _dp, _dp, _dp, C.POINTER(vp)]
    lib.vbmc_acq_eval.argtypes = [vp, vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.c_int, C.c_double,
                                  _dp, _dp, _dp, _dp, _dp, _dp]
    lib.vbmc_acq_eval_delta.argtypes = lib.vbmc_acq_eval.argtypes + [_dp]
    lib.vbmc_gp_quad.argtypes = [vp, vp, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp]
    lib.vbmc_acq_is_create.argtypes = [vp, vp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.POINTER(vp)]
    lib.vbmc_acq_is_free.argtypes = [vp, vp]
    lib.vbmc_acq_is_free.restype = None
    lib.vbmc_acq_iqr_eval.argtypes = [vp, vp, vp, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp, _dp, _dp]
    lib.vbmc_gp_nlz.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp]
    lib.vbmc_gp_slice_sample.argtypes = [vp, C.POINTER(SliceArgs)]
    lib.vbmc_gp_train_optimize.argtypes = [vp, C.POINTER(GpTrainArgs)]
    lib.vbmc_acq_search.argtypes = [vp, vp, C.POINTER(AcqSearchArgs)]
    lib.vbmc_acq_search_iqr.argtypes = [vp, vp, vp, C.POINTER(AcqSearchArgs)]
    lib.vbmc_acq_is_sample.argtypes = [vp, vp, C.POINTER(IsSampleArgs)]
    lib.vbmc_acq_is_setup.argtypes = [vp, vp, C.POINTER(IsSetupArgs)]
    vpd = C.POINTER(VpDesc)
    lib.vbmc_vp_pdf.argtypes = [vp, vpd, C.c_int64, _dp, C.c_int, C.c_int, C.c_int, C.c_double, _dp, _dp]
    lib.vbmc_vp_rnd.argtypes = [vp, vpd, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_uint64, _dp, _dp, C.POINTER(C.c_int32)]
    lib.vbmc_vp_moments.argtypes = [vp, vpd, C.c_int64, C.c_uint64, _dp, _dp, _dp]
    lib.vbmc_vp_kldiv.argtypes = [vp, vpd, vpd, C.c_int64, C.c_uint64, _dp, _dp, _dp, _dp, _dp]
    lib.vbmc_vp_mtv.argtypes = [vp, vpd, vpd, C.POINTER(MtvArgs)]
    lib.vbmc_vp_corner.argtypes = [vp, vpd, C.POINTER(CornerArgs)]
    lib.vbmc_vp_diagnostics.argtypes = [vp, C.c_int32, C.POINTER(vpd), C.POINTER(DiagArgs)]
    lib.vbmc_vp_mode.argtypes = [vp, vpd, C.POINTER(ModeArgs)]
    lib.vbmc_test_dct.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp]
    lib.vbmc_gp_surrogate_sample.argtypes = [vp, vp, vpd, C.POINTER(GsArgs)]
    lib.vbmc_test_exp.argtypes =[vp, C.c_int, C.c_int, _dp, _dp]
    lib.vbmc_sq_dist.argtypes = [vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp]
    # the communicator inside the library (abi_comm.hip)
    vpp = C.POINTER(vp)
    lib.vbmc_comm_create_all.argtypes = [C.c_int, C.POINTER(C.c_int), vpp]
    lib.vbmc_comm_unique_id.argtypes = [C.c_char_p]
    lib.vbmc_comm_create_rank.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, vpp]
    lib.vbmc_comm_destroy.argtypes = [vp]
    lib.vbmc_comm_destroy.restype = None
    for name in ("vbmc_comm_size", "vbmc_comm_local", "vbmc_comm_rank"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = C.c_int
    lib.vbmc_comm_ctx.argtypes = [vp, C.c_int]
    lib.vbmc_comm_ctx.restype = vp
    lib.vbmc_comm_last_error.argtypes = [vp]
    lib.vbmc_comm_last_error.restype = C.c_char_p
    lib.vbmc_allgather_f64.argtypes = [vp, vpp, vpp, C.c_size_t]
    lib.vbmc_allgather_host_f64.argtypes = [vp, _dp, _dp, C.c_size_t]
    lib.vbmc_gp_upload_all.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_uint8), vpp]
    lib.vbmc_gp_free_all.argtypes = [vp, vpp]
    lib.vbmc_gp_free_all.restype = None
    lib.vbmc_elbo_batch_multi.argtypes = [vp, vpp, C.POINTER(ElboArgs)]
    lib.vbmc_elbo_multi_submit.argtypes = [vp, vpp, C.POINTER(ElboArgs), C.c_int]
    lib.vbmc_elbo_multi_collect.argtypes = [vp, C.POINTER(ElboArgs), C.c_int]
    for name, types in _HOST_DUMPS.items():
        getattr(lib, name).argtypes = [C.c_uint64] + types
    if lib.vbmc_abi_version() != ABI_VERSION:
        raise ImportError("libvbmc_hip.so ABI version mismatch")
    _lib = lib
    return lib


def f64(a, order="F"):
    """Contiguous column-major fp64 copy/view (what MATLAB hands over)."""
    return np.require(np.asarray(a, dtype=np.float64), dtype=np.float64, requirements=["F" if order == "F" else "C", "A"])


def ptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def host_dump(name, seed, *args, hip_error=None):
    """Call the host-only dump ``name`` of _HOST_DUMPS with ``seed`` and ``args`` (integers, and the NumPy arrays it fills) and raise on
    a non-zero status: ValueError, or VbmcHipError with the message ``hip_error`` where one is given."""
    fn = getattr(load(), name)
    assert len(args) == len(_HOST_DUMPS[name]), name
    st = fn(C.c_uint64(int(seed)), *[a.ctypes.data_as(t) if isinstance(a, np.ndarray) else int(a) for a, t in zip(args, _HOST_DUMPS[name])])
    if st != VBMC_OK:
        raise VbmcHipError(st, hip_error) if hip_error else ValueError("%s: bad arguments" % name)


class Context:
    """One HIP stream + device scratch on one GPU (vbmc_ctx)."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        h = C.c_void_p()
        st = self.lib.vbmc_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if st != VBMC_OK:
            raise VbmcHipError(st, "vbmc_ctx_create(device=%d) failed: a gfx950 (MI355X) device is required; "
                                   "there is no CPU fallback" % device)
        self.h = h
        self.device = device

    def check(self, st):
        if st == VBMC_OK:
            return
        msg = self.lib.vbmc_last_error(self.h).decode("utf-8", "replace")
        if st == VBMC_ERR_UNSUPPORTED:
            raise VbmcUnsupported(st, msg)
        raise VbmcHipError(st, msg)

    def synchronize(self):
        self.check(self.lib.vbmc_ctx_synchronize(self.h))

    def set_profiling(self, on=True):
        """on = 2: the dominant kernel timed ALONE (the log joint is not forked beside it), see include/vbmc_hip.h"""
        self.check(self.lib.vbmc_ctx_set_profiling(self.h, 2 if (on is not True and on == 2) else (1 if on else 0)))

    def last_kernel_ms(self):
        a, b = C.c_double(), C.c_double()
        self.check(self.lib.vbmc_ctx_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_launch(self):
        """(ent_form, lj_form) of the last ELBO pass enqueued on this context (test hook: ENTFORM_* / LJFORM_*, 0 where none ran)"""
        a, b = C.c_int(), C.c_int()
        self.check(self.lib.vbmc_ctx_last_launch(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_variance(self):
        """dict of the fields of vbmc_var_launch_info: what the variance stage of the last pass with compute_var != 0 enqueued on
        this context (test hook: VARSOLVE_* / VARGRAM_*; compute_var 0 where none ran)"""
        info = new_args(VarLaunchInfo)
        self.check(self.lib.vbmc_ctx_last_variance(self.h, C.byref(info)))
        return {n: int(getattr(info, n)) for n, _ in VarLaunchInfo._fields_[1:]}

    def rng_dump(self, D, K, R, Ns, seed):
        """eps (R, K, Ns/2, D) that eps_mode 0 consumes for `seed` (test hook)."""
        Mh = (Ns + 1) // 2
        out = np.empty((R, K, Mh, D), dtype=np.float64)
        self.check(self.lib.vbmc_rng_dump(self.h, D, K, R, Ns, C.c_uint64(seed), ptr(out)))
        return out

    def test_exp(self, x, variant=0):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
        y = np.empty_like(x)
        self.check(self.lib.vbmc_test_exp(self.h, x.size, int(variant), ptr(x), ptr(y)))
        return y

    def close(self):
        if getattr(self, "h", None):
            self.lib.vbmc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceGP:
    """Device-resident gp.post(1..S) (vbmc_gp)."""

    def __init__(self, ctx, X, hyp, alpha, L, sW1, Lchol, meanfun, Ncov, Nnoise):
        self.ctx = ctx
        X = f64(X)
        hyp = f64(hyp)
        if hyp.ndim == 1:
            hyp = hyp[:, None]
        alpha = f64(alpha)
        if alpha.ndim == 1:
            alpha = alpha[:, None]
        N, D = X.shape
        Nhyp, S = hyp.shape
        sW1 = f64(np.asarray(sW1).reshape(S))
        lch = np.ascontiguousarray(np.asarray(Lchol, dtype=np.uint8).reshape(S))
        Lp = None
        if L is not None:
            L = f64(L)  # (N, N, S) column-major == MATLAB N x N x S
            assert L.shape == (N, N, S), L.shape
            Lp = ptr(L)
        h = C.c_void_p()
        ctx.check(ctx.lib.vbmc_gp_upload(ctx.h, N, D, S, Nhyp, int(Ncov), int(Nnoise), int(meanfun), ptr(X), ptr(hyp),
                                         ptr(alpha), Lp, ptr(sW1), lch.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(h)))
        self.h = h
        self.N, self.D, self.S = N, D, S

    @classmethod
    def from_handle(cls, ctx, h, N, D, S):
        self = cls.__new__(cls)
        self.ctx, self.h, self.N, self.D, self.S = ctx, h, N, D, S
        return self

    def set_noise(self, noisefun, sn2_mult):
        nf = (C.c_int32 * 3)(*[int(x) for x in (list(noisefun) + [0, 0, 0])[:3]])
        m = f64(np.asarray(sn2_mult, dtype=np.float64).reshape(self.S))
        self.ctx.check(self.ctx.lib.vbmc_gp_set_noise(self.ctx.h, self.h, nf, ptr(m)))

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.vbmc_gp_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
