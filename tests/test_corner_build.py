"""CPU check beside tests/test_mtv_build.py: the kernels of the corner-plot data (vbmc_amd/csrc/corner_kernels.h under vbmc_vp_corner in
abi_vp_mtv.hip) cross-compile for gfx950 and use no scratch -- no spilled vector register, no private segment, read from the
compiler's own resource-usage metadata -- and call no device-library transcendental, both new files are part of the build, and the
library exports vbmc_vp_corner with a ctypes declaration and an argument structure that follow the header."""
import os
import re

from tests import _abi

ROOT, CSRC = _abi.ROOT, _abi.CSRC
KERNELS = ("k_corner_range", "k_corner_index", "k_corner_pairs", "k_corner_kde", "k_corner_select")


def test_corner_kernels_use_no_scratch(tmp_path):
    kernels, asm = _abi.kernel_meta("corner_kernels.h", (), r"k_corner_", tmp_path)
    seen = {k["mangled"]: (k["vgpr_spill_count"], k["private_segment_fixed_size"], k["max_flat_workgroup_size"], k["wavefront_size"]) for k in kernels}
    print({k["name"]: (k["vgpr_count"], k["group_segment_fixed_size"]) for k in kernels})
    names = set(re.findall(r"__global__[^\n]*\b(k_corner_\w+)\(", open(os.path.join(CSRC, "corner_kernels.h")).read()))
    assert names == set(KERNELS), names                                                           # every kernel of the header
    for k in KERNELS:
        inst = [n for n in seen if re.match(r"_Z\d+%s\d" % k, n)]
        assert len(inst) == 1, (k, inst)
        assert seen[inst[0]] == (0, 0, 256, 64), (k, seen[inst[0]])                               # no scratch; 256 threads of wave64
    for k in ("exp", "log", "log1p", "cos", "sin", "pow"):                                        # no device-library transcendental
        assert not re.search(r"__ocml_%s_f64" % k, asm), k
    lds = {k["name"]: k["group_segment_fixed_size"] for k in kernels}
    assert lds["k_corner_kde"] <= 64 * 1024 and lds["k_corner_pairs"] == 64 * 64 * 4              # one res^2 tile each


def test_the_new_files_are_part_of_the_build():
    build = open(os.path.join(ROOT, "vbmc_amd", "build.py")).read()
    assert '"corner_kernels.h"' in build and '"corner_host.h"' in build
    unit = open(os.path.join(CSRC, "abi_vp_mtv.hip")).read()
    assert '#include "corner_host.h"' in unit and "vbmc_vp_corner" in unit
    assert '#include "corner_kernels.h"' in open(os.path.join(CSRC, "corner_host.h")).read()
    assert "k_corner_" not in open(os.path.join(CSRC, "mtv_kernels.h")).read()


def test_library_exports_vbmc_vp_corner():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    import vbmc_amd
    from vbmc_amd import _lib, vptools

    lib = _lib.load()
    hdr = _abi.header_text()
    assert hasattr(lib, "vbmc_vp_corner") and hasattr(vptools, "vbmc_plot_data") and hasattr(vptools, "cornerplot_data")
    assert vbmc_amd.vbmc_plot_data is vptools.vbmc_plot_data and vbmc_amd.cornerplot_data is vptools.cornerplot_data
    proto = re.search(r"vbmc_status vbmc_vp_corner\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(lib.vbmc_vp_corner.argtypes) == 3, proto
    assert lib.vbmc_vp_corner.argtypes[2] == C.POINTER(_lib.CornerArgs)
    assert [n for n, _ in _lib.CornerArgs._fields_] == _abi.header_structs()["vbmc_corner_args"]
    assert lib.vbmc_abi_version() == 8 and int(re.search(r"#define VBMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    # a null context is refused first, a wrong struct_size before anything is read (no device needed)
    d, a = _lib.new_args(_lib.VpDesc), _lib.new_args(_lib.CornerArgs)
    assert lib.vbmc_vp_corner(None, C.byref(d), C.byref(a)) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_vp_corner(None, None, C.byref(a)) == _lib.VBMC_ERR_INVALID
    a.struct_size += 8
    assert lib.vbmc_vp_corner(None, C.byref(d), C.byref(a)) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_vp_corner(None, C.byref(d), None) == _lib.VBMC_ERR_INVALID
