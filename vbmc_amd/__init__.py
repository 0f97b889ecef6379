"""vbmc_amd: MI355X-native ELBO inner loop of VBMC behind the reference's call surface.

Host-side mirror (Python, because the reference's MATLAB toolchain is absent here) of
negelcbo_vbmc / gplogjoint / entmc_vbmc / entlb_vbmc / gplite_post / gplite_pred / gplite_nlZ /
slicesamplebnd on the GP hyper-parameter posterior / vpsieve_vbmc / vpoptimize_vbmc / fminadam over the C ABI of libvbmc_hip.so
(include/vbmc_hip.h).  All numerics run in hand-written HIP kernels on gfx950; there is
no CPU fallback in this package.
"""
from . import _lib  # noqa: F401
from ._lib import Context, DeviceGP, VbmcHipError, VbmcUnsupported  # noqa: F401
from .vp import get_vptheta, make_vp, rescale_params, vpbounds  # noqa: F401
from .elbo import (Engine, PreparedObjective, default_engine, entlb_vbmc, entmc_vbmc, fminadam_device, gplogjoint,  # noqa: F401
                   negelcbo_batch, negelcbo_shard, negelcbo_vbmc)
from .gplite import (fminfill_design, gp_surrogate_sample_rng_dump, gplite_hypprior, gplite_nlZ, gplite_post, gplite_post_rank1, gplite_pred,  # noqa: F401,E402
                     gplite_quad, gplite_sample, gplite_sample_device, gplite_train, gplite_train_optimize, gplite_train_sample, slice_rng_dump,
                     slicesamplebnd_gp, sq_dist)
from .ensemble import ensemble_slice_sample  # noqa: F401,E402
from .mixture import vbmc_moments, vbmc_rnd  # noqa: F401,E402  (the HOST forms; the device forms are vptools.vbmc_rnd / vbmc_moments)
from . import vptools  # noqa: F401,E402
from .vptools import cornerplot_data, gpsample_vbmc, vbmc_plot_data, vbmc_diagnostics, vbmc_mode, vp_rnd_rng_dump, warpvars  # noqa: F401,E402
from .optimize import (eval_fullelcbo, fminadam, gethpd_vbmc, sieve_evaluate, vbinit_vbmc, vpoptimize_vbmc,  # noqa: F401,E402
                       vpsieve_vbmc)
from .acq import (acq_info, acq_search, acq_search_rng_dump, acqwrapper_vbmc, active_search, activeimportancesampling_vbmc,  # noqa: F401,E402
                  importance_sample_device, importance_sample_rng_dump)
