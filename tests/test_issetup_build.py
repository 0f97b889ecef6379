"""CPU check beside tests/test_issample_build.py: the translation unit of the one-call set-up (vbmc_amd/csrc/abi_is_setup.hip on top of
is_setup_kernels.h) cross-compiles for gfx950, its kernels k_is_draw, k_is_proposal and k_is_resample use no scratch -- no spilled
vector register, no private segment, read from the compiler's own resource-usage metadata --, and the library exports vbmc_acq_is_setup
and vbmc_acq_is_setup_rng_dump with ctypes declarations that follow the header."""
import os
import re

from tests import _abi

ROOT, CSRC = _abi.ROOT, _abi.CSRC


def test_is_setup_kernels_use_no_scratch(tmp_path):
    kernels, asm = _abi.kernel_meta("is_setup_kernels.h", (), r"k_is_", tmp_path)
    seen = {k["name"]: (k["vgpr_spill_count"], k["private_segment_fixed_size"]) for k in kernels}
    print(seen)
    for k in ("k_is_draw", "k_is_proposal", "k_is_resample"):
        assert seen[k] == (0, 0), (k, seen[k])
    for k in ("exp", "log", "log1p"):                                                            # no device-library transcendental
        assert not re.search(r"__ocml_%s_f64" % k, asm), k


def test_the_translation_unit_is_part_of_the_build():
    build = open(os.path.join(ROOT, "vbmc_amd", "build.py")).read()
    unit = open(os.path.join(CSRC, "vbmc_hip.hip")).read()
    assert '"abi_is_setup.hip"' in build and '"is_setup_kernels.h"' in build and '#include "abi_is_setup.hip"' in unit
    assert unit.index("abi_is_sample.hip") < unit.index("abi_is_setup.hip")


def test_library_exports_the_setup():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "vbmc_acq_is_setup") and len(lib.vbmc_acq_is_setup.argtypes) == 3
    assert hasattr(lib, "vbmc_acq_is_setup_rng_dump") and len(lib.vbmc_acq_is_setup_rng_dump.argtypes) == 7
    hdr = _abi.header_text()
    assert re.search(r"vbmc_status vbmc_acq_is_setup\(vbmc_ctx\* ctx, const vbmc_gp\* gp, const vbmc_is_setup_args\* args\);", hdr)
    assert re.search(r"vbmc_status vbmc_acq_is_setup_rng_dump\(uint64_t seed, int D, int S, int W, int Nvp, int Nbox, double\* B\);", hdr)
    # a wrong struct_size is refused before anything is read (no device needed: the context pointer is checked first)
    a = _lib.new_args(_lib.IsSetupArgs)
    assert lib.vbmc_acq_is_setup(None, None, C.byref(a)) == 1
    # the sampler's entry point still answers as before the two were given a common routine
    b = _lib.new_args(_lib.IsSampleArgs)
    assert lib.vbmc_acq_is_sample(None, None, C.byref(b)) == 1
