"""CPU check beside tests/test_issetup_build.py: the kernels of the variational-posterior tools (vbmc_amd/csrc/vp_tools_kernels.h under
abi_vp_tools.hip) cross-compile for gfx950 and use no scratch -- no spilled vector register, no private segment, read from the
compiler's own resource-usage metadata, for every instantiation of k_vp_pdf, k_vp_draw, k_vp_moments and k_vp_kldiv --, both files are
part of the build, and the library exports the five entry points with ctypes declarations that follow the header."""
import os
import re

from tests import _abi

ROOT, CSRC = _abi.ROOT, _abi.CSRC
KERNELS = ("k_vp_pdf", "k_vp_draw", "k_vp_moments", "k_vp_kldiv")
ENTRY_POINTS = {"vbmc_vp_pdf": 10, "vbmc_vp_rnd": 10, "vbmc_vp_moments": 7, "vbmc_vp_kldiv": 10, "vbmc_vp_rnd_rng_dump": 8}


def test_vp_tools_kernels_use_no_scratch(tmp_path):
    inst = []                        # every instantiation the dispatch of abi_vp_tools.hip names
    for dt in (4, 8, 12, 16, 24, 32):
        inst += ["template __global__ void k_vp_pdf<%d, true>(VptPdfArgs);" % dt, "template __global__ void k_vp_pdf<%d, false>(VptPdfArgs);" % dt,
                 "template __global__ void k_vp_draw<%d>(VptDrawArgs);" % dt, "template __global__ void k_vp_moments<%d>(VptMomArgs);" % dt,
                 "template __global__ void k_vp_kldiv<%d>(VptKlArgs);" % dt]
    kernels, asm = _abi.kernel_meta("vp_tools_kernels.h", inst, r"k_vp_", tmp_path)
    seen = {k["mangled"]: (k["vgpr_spill_count"], k["private_segment_fixed_size"]) for k in kernels}
    print(seen)
    for k in KERNELS:
        inst = [n for n in seen if re.match(r"_Z\d+%s(I|P|$)" % k, n)]
        assert len(inst) == (12 if k == "k_vp_pdf" else 6), (k, inst)
        for n in inst:
            assert seen[n] == (0, 0), (n, seen[n])
    for k in ("exp", "log", "log1p"):                                                            # no device-library transcendental
        assert not re.search(r"__ocml_%s_f64" % k, asm), k


def test_the_translation_unit_is_part_of_the_build():
    build = open(os.path.join(ROOT, "vbmc_amd", "build.py")).read()
    unit = open(os.path.join(CSRC, "vbmc_hip.hip")).read()
    assert '"abi_vp_tools.hip"' in build and '"vp_tools_kernels.h"' in build and '#include "abi_vp_tools.hip"' in unit
    assert unit.index("abi_is_setup.hip") < unit.index("abi_vp_tools.hip")


def test_library_exports_the_vp_tools():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib

    lib = _lib.load()
    hdr = _abi.header_text()
    for name, nargs in ENTRY_POINTS.items():
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
        proto = re.search(r"vbmc_status %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(proto.split(",")) == nargs, (name, proto)
    assert lib.vbmc_abi_version() == 8
    # a wrong struct_size is refused before anything is read; a null context is refused first (no device needed)
    d = _lib.new_args(_lib.VpDesc)
    d.struct_size += 8
    y = (C.c_double * 2)()
    assert lib.vbmc_vp_pdf(None, C.byref(d), 1, y, 1, 1, 0, float("inf"), y, None) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_vp_rnd(None, C.byref(d), 1, 1, 0, float("inf"), 0, None, y, None) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_vp_moments(None, C.byref(d), 10, 0, None, y, None) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_vp_kldiv(None, C.byref(d), C.byref(d), 10, 0, None, None, y, None, None) == _lib.VBMC_ERR_INVALID
    # the host dump needs no device: the permutation is a bijection and the block is reproducible
    import numpy as np

    from vbmc_amd import vptools

    w = np.array([0.5, 0.3, 0.2])
    B, perm = vptools.vp_rnd_rng_dump(3, 1003, 4, w, True)
    B2, perm2 = vptools.vp_rnd_rng_dump(3, 1003, 4, w, True)
    assert np.array_equal(B, B2) and np.array_equal(perm, perm2) and B.shape == (vptools.split_size(w, 1003, True), 5)
    assert len(set(perm.tolist())) == 1003 and 0 <= perm.min() and perm.max() < B.shape[0]
    assert np.all((B[:, 0] > 0) & (B[:, 0] < 1)) and np.all(np.isfinite(B))
