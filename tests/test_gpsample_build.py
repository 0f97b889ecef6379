"""CPU check beside tests/test_issample_build.py and tests/test_mtv_build.py: the kernels of the surrogate sampler
(vbmc_amd/csrc/gp_surrogate_kernels.h under abi_gp_surrogate.hip) cross-compile for gfx950 with no scratch -- no spilled vector
register, no private segment, read from the compiler's own resource-usage metadata; k_gs_pred for every inner dimension QS = 1 .. 8,
k_gs_finish for its six padded dimensions -- and call no device-library transcendental; both files are part of the build; the library
exports vbmc_gp_surrogate_sample and vbmc_gp_surrogate_sample_rng_dump with ctypes declarations and an argument structure that follow
the header; a NULL args pointer is refused without a device."""
import os
import re

from tests import _abi

ROOT, CSRC = _abi.ROOT, _abi.CSRC
PLAIN = ("k_gs_target", "k_gs_start", "k_gs_sum", "k_gs_thresh")
DTS = (4, 8, 12, 16, 24, 32)


def test_surrogate_kernels_use_no_scratch(tmp_path):
    inst = ["template __global__ void k_gs_pred<%d>(IsPredArgs);" % qs for qs in range(1, 9)]
    inst += ["template __global__ void k_gs_finish<%d>(GsFinishArgs);" % dt for dt in DTS]
    kernels, asm = _abi.kernel_meta("gp_surrogate_kernels.h", inst, r"k_gs_", tmp_path)
    seen = set()
    for k in kernels:
        print(k["name"], k["targs"], "spill", k["vgpr_spill_count"], "private", k["private_segment_fixed_size"])
        assert _abi.no_scratch(k), k
        seen.add(k["name"] + "".join(str(t) for t in k["targs"][:1]))
    want = set(PLAIN) | {"k_gs_pred%d" % q for q in range(1, 9)} | {"k_gs_finish%d" % d for d in DTS}
    assert seen == want, seen ^ want
    names = set(re.findall(r"__global__[^\n]*\b(k_gs_\w+)\(", open(os.path.join(CSRC, "gp_surrogate_kernels.h")).read()))
    assert names == set(PLAIN) | {"k_gs_pred", "k_gs_finish"}, names                              # every kernel of the header
    assert "v_mfma_f64_16x16x4" in asm
    for k in ("exp", "log", "log1p", "pow"):                                                      # no device-library transcendental
        assert not re.search(r"__ocml_%s_f64" % k, asm), k


def test_the_translation_unit_is_part_of_the_build():
    build = open(os.path.join(ROOT, "vbmc_amd", "build.py")).read()
    unit = open(os.path.join(CSRC, "vbmc_hip.hip")).read()
    assert '"abi_gp_surrogate.hip"' in build and '"gp_surrogate_kernels.h"' in build and '#include "abi_gp_surrogate.hip"' in unit
    assert unit.index("abi_vp_tools.hip") < unit.index("abi_gp_surrogate.hip")


def test_library_exports_the_surrogate_sampler():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib, gplite, vptools

    lib = _lib.load()
    hdr = _abi.header_text()
    assert hasattr(lib, "vbmc_gp_surrogate_sample") and hasattr(lib, "vbmc_gp_surrogate_sample_rng_dump")
    assert hasattr(gplite, "gplite_sample") and hasattr(gplite, "gplite_sample_device") and hasattr(vptools, "gpsample_vbmc")
    proto = re.search(r"vbmc_status vbmc_gp_surrogate_sample\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(lib.vbmc_gp_surrogate_sample.argtypes) == 4, proto
    assert lib.vbmc_gp_surrogate_sample.argtypes[2] == C.POINTER(_lib.VpDesc) and lib.vbmc_gp_surrogate_sample.argtypes[3] == C.POINTER(_lib.GsArgs)
    assert re.search(r"vbmc_status vbmc_gp_surrogate_sample_rng_dump\(uint64_t seed, int E, int H, int M, double\* U\);", hdr)
    assert len(lib.vbmc_gp_surrogate_sample_rng_dump.argtypes) == 5
    assert lib.vbmc_abi_version() == 8 and int(re.search(r"#define VBMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    # a null context is refused first, a NULL args pointer and a wrong struct_size before anything is read (no device needed)
    a = _lib.new_args(_lib.GsArgs)
    assert lib.vbmc_gp_surrogate_sample(None, None, None, C.byref(a)) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_gp_surrogate_sample(None, None, None, None) == _lib.VBMC_ERR_INVALID
    # the dump is a pure host function: the block of the importance sampler's generator with E in the place of S
    U = gplite.gp_surrogate_sample_rng_dump(7, 3, 2, 4)
    from vbmc_amd.acq import importance_sample_rng_dump

    assert U.shape == (64, 2, 3, 4) and np_equal(U, importance_sample_rng_dump(7, 3, 2, 4))
    assert float(U.min()) > 0.0 and float(U.max()) < 1.0
    assert lib.vbmc_gp_surrogate_sample_rng_dump(C.c_uint64(1), 0, 2, 4, None) == _lib.VBMC_ERR_INVALID


def np_equal(a, b):
    import numpy as np

    return bool(np.array_equal(a, b))
