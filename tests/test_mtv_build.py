"""CPU check beside tests/test_vptools_build.py: the kernels of the marginal total variation (vbmc_amd/csrc/mtv_kernels.h under
abi_vp_mtv.hip) cross-compile for gfx950 and use no scratch -- no spilled vector register, no private segment, read from the
compiler's own resource-usage metadata -- and call no device-library transcendental, both files are part of the build, and the
library exports vbmc_vp_mtv with a ctypes declaration and an argument structure that follow the header."""
import os
import re

from tests import _abi

ROOT, CSRC = _abi.ROOT, _abi.CSRC
KERNELS = ("k_mtv_mesh", "k_mtv_bin", "k_mtv_init", "k_mtv_dct", "k_mtv_root", "k_mtv_integral")


def test_mtv_kernels_use_no_scratch(tmp_path):
    kernels, asm = _abi.kernel_meta("mtv_kernels.h", (), r"k_mtv_", tmp_path)
    seen = {k["mangled"]: (k["vgpr_spill_count"], k["private_segment_fixed_size"], k["max_flat_workgroup_size"], k["wavefront_size"]) for k in kernels}
    print(seen)
    names = set(re.findall(r"__global__[^\n]*\b(k_mtv_\w+)\(", open(os.path.join(CSRC, "mtv_kernels.h")).read()))
    assert names == set(KERNELS), names                                                           # every kernel of the header
    for k in KERNELS:
        inst = [n for n in seen if re.match(r"_Z\d+%s\d" % k, n)]
        assert len(inst) == 1, (k, inst)
        assert seen[inst[0]] == (0, 0, 256, 64), (k, seen[inst[0]])                               # no scratch; 256 threads of wave64
    for k in ("exp", "log", "log1p", "cos", "sin", "pow"):                                        # no device-library transcendental
        assert not re.search(r"__ocml_%s_f64" % k, asm), k


def test_the_translation_unit_is_part_of_the_build():
    build = open(os.path.join(ROOT, "vbmc_amd", "build.py")).read()
    unit = open(os.path.join(CSRC, "vbmc_hip.hip")).read()
    assert '"abi_vp_mtv.hip"' in build and '"mtv_kernels.h"' in build and '#include "abi_vp_mtv.hip"' in unit
    assert unit.index("abi_vp_tools.hip") < unit.index("abi_vp_mtv.hip")
    assert "k_mtv_" not in open(os.path.join(CSRC, "vp_tools_kernels.h")).read()


def test_library_exports_vbmc_vp_mtv():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib, vptools

    lib = _lib.load()
    hdr = _abi.header_text()
    assert hasattr(lib, "vbmc_vp_mtv") and hasattr(vptools, "vbmc_mtv")
    proto = re.search(r"vbmc_status vbmc_vp_mtv\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(lib.vbmc_vp_mtv.argtypes) == 4, proto
    assert lib.vbmc_vp_mtv.argtypes[3] == C.POINTER(_lib.MtvArgs)
    assert lib.vbmc_abi_version() == 8 and int(re.search(r"#define VBMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    # a null context is refused first, a wrong struct_size before anything is read (no device needed)
    d, a = _lib.new_args(_lib.VpDesc), _lib.new_args(_lib.MtvArgs)
    assert lib.vbmc_vp_mtv(None, C.byref(d), C.byref(d), C.byref(a)) == _lib.VBMC_ERR_INVALID
    a.struct_size += 8
    assert lib.vbmc_vp_mtv(None, C.byref(d), C.byref(d), C.byref(a)) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_vp_mtv(None, C.byref(d), C.byref(d), None) == _lib.VBMC_ERR_INVALID
