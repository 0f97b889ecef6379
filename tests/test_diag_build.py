"""CPU check beside tests/test_mtv_build.py: the kernels of the multi-run diagnostics (vbmc_amd/csrc/diag_kernels.h under
abi_vp_diag.hip) cross-compile for gfx950 in every instantiation the dispatch names and use no scratch -- no spilled vector register,
no private segment, read from the compiler's own resource-usage metadata -- and call no device-library transcendental, both files
are part of the build, and the library exports vbmc_vp_diagnostics with a ctypes declaration and an argument structure that follow
the header field for field; the ABI version is unchanged; what the entry point refuses before it reads anything is refused without
a device."""
import os
import re

from tests import _abi

ROOT, CSRC = _abi.ROOT, _abi.CSRC
KERNELS = {"k_diag_cross_kl": (6, 128), "k_diag_dct": (1, 256)}      # instantiations, threads per workgroup (the integral of every pair
# is k_mtv_integral: tests/test_mtv_build.py)


def test_diag_kernels_use_no_scratch(tmp_path):
    inst = ["template __global__ void k_diag_cross_kl<%d>(DiagKlArgs);" % dt for dt in (4, 8, 12, 16, 24, 32)]
    kernels, asm = _abi.kernel_meta("diag_kernels.h", inst, r"k_diag_", tmp_path)
    seen = {k["mangled"]: (k["vgpr_spill_count"], k["private_segment_fixed_size"], k["max_flat_workgroup_size"], k["wavefront_size"]) for k in kernels}
    print(seen)
    names = set(re.findall(r"__global__[^\n]*\b(k_diag_\w+)\(", open(os.path.join(CSRC, "diag_kernels.h")).read()))
    assert names == set(KERNELS), names                                                           # every kernel of the header
    for k, (count, threads) in KERNELS.items():
        inst = [n for n in seen if re.match(r"_Z\d+%s(I|\d)" % k, n)]
        assert len(inst) == count, (k, inst)
        for n in inst:
            assert seen[n] == (0, 0, threads, 64), (n, seen[n])                                   # no scratch; wave64
    for k in ("exp", "log", "log1p", "cos", "sin", "pow"):                                        # no device-library transcendental
        assert not re.search(r"__ocml_%s_f64" % k, asm), k


def test_the_translation_unit_is_part_of_the_build():
    build = open(os.path.join(ROOT, "vbmc_amd", "build.py")).read()
    unit = open(os.path.join(CSRC, "vbmc_hip.hip")).read()
    assert '"abi_vp_diag.hip"' in build and '"diag_kernels.h"' in build and '#include "abi_vp_diag.hip"' in unit
    assert unit.index("abi_vp_mtv.hip") < unit.index("abi_vp_diag.hip")
    assert "k_diag_" not in open(os.path.join(CSRC, "mtv_kernels.h")).read()


def test_library_exports_vbmc_vp_diagnostics():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    import vbmc_amd
    from vbmc_amd import _lib, vptools

    lib = _lib.load()
    hdr = _abi.header_text()
    assert hasattr(lib, "vbmc_vp_diagnostics") and hasattr(vptools, "vbmc_diagnostics") and vbmc_amd.vbmc_diagnostics is vptools.vbmc_diagnostics
    proto = re.search(r"vbmc_status vbmc_vp_diagnostics\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(lib.vbmc_vp_diagnostics.argtypes) == 4, proto
    assert lib.vbmc_vp_diagnostics.argtypes[1] == C.c_int32
    assert lib.vbmc_vp_diagnostics.argtypes[2] == C.POINTER(C.POINTER(_lib.VpDesc))
    assert lib.vbmc_vp_diagnostics.argtypes[3] == C.POINTER(_lib.DiagArgs)
    assert [f[0] for f in _lib.DiagArgs._fields_][:5] == ["struct_size", "nkde", "nquad", "Ns", "seed"]
    assert lib.vbmc_abi_version() == 8 and int(re.search(r"#define VBMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    # a null context is refused first (no device needed)
    d = _lib.new_args(_lib.VpDesc)
    arr = (C.POINTER(_lib.VpDesc) * 2)(C.pointer(d), C.pointer(d))
    a = _lib.new_args(_lib.DiagArgs)
    assert lib.vbmc_vp_diagnostics(None, 2, arr, C.byref(a)) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_vp_diagnostics(None, 2, arr, None) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_vp_diagnostics(None, 1, None, C.byref(a)) == _lib.VBMC_ERR_INVALID


def test_refusals_before_anything_is_read():
    """Without a device there is no context, and a null context is all the library can be shown (above).  What follows it is read from
    the entry point's text: a wrong struct_size, then R < 2, are refused (INVALID) before the posteriors are looked at, R > 32 is
    UNSUPPORTED, and the fminbnd message names run and dimension.  tests/test_gpu_diag.py runs these refusals on a device."""
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib

    src = open(os.path.join(CSRC, "abi_vp_diag.hip")).read()
    body = src[src.index('extern "C" vbmc_status vbmc_vp_diagnostics'):]
    order = [body.index(s) for s in ("if (!ctx)", "struct_size != sizeof(vbmc_diag_args)", "if (R < 2)", "if (R > DIAG_MAXR)", "vpt_pack(")]
    assert order == sorted(order), order                                                          # the order of the refusals
    assert "VBMC_ERR_UNSUPPORTED" in body[order[3]:order[3] + 120] and "VBMC_ERR_INVALID" in body[order[2]:order[2] + 120]
    # the fminbnd message lives once, in mtv_host.h's pipeline, and names the unit the entry point gives it and the dimension:
    # "run" here, "posterior" in vbmc_vp_mtv
    host = open(os.path.join(CSRC, "mtv_host.h")).read()
    assert len(re.findall(r"fminbnd", host)) == 1 and re.search(r'"%s %d, dimension %d: [^"]*fminbnd[^"]*",\s*unit, c / D \+ 1, c % D \+ 1\)', host)
    assert re.search(r'kde\.begin\(ctx, who, "run", \*args\)', body) and "fminbnd" not in src
    mtv = open(os.path.join(CSRC, "abi_vp_mtv.hip")).read()
    assert re.search(r'kde\.begin\(ctx, who, "posterior", \*args\)', mtv) and "fminbnd" not in mtv
    assert re.search(r'unit = unit_;', host) and len(re.findall(r"\bunit = ", host)) == 2         # set in begin alone (and its default)
    assert "#define DIAG_MAXR 32" in open(os.path.join(CSRC, "diag_kernels.h")).read()
    lib = _lib.load()
    a = _lib.new_args(_lib.DiagArgs)
    a.struct_size += 8
    assert lib.vbmc_vp_diagnostics(None, 2, None, C.byref(a)) == _lib.VBMC_ERR_INVALID
