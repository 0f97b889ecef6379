"""CPU check beside tests/test_diag_build.py: the kernel of the posterior's mode (vbmc_amd/csrc/mode_kernels.h under mode_host.h and
the entry point in abi_vp_tools.hip) cross-compiles for gfx950 in every instantiation the dispatch names and uses no scratch -- no
spilled vector register, no private segment, read from the compiler's own resource-usage metadata --, runs in wave64 at the declared
workgroup size and calls no device-library transcendental; the new files are part of the build; the library exports vbmc_vp_mode with a
ctypes declaration and an argument structure that follow the header; the ABI version is unchanged; what the entry point refuses
before it reads anything is refused without a device, and the order of its refusals is read from its text.

(The entry point lives in abi_vp_tools.hip, not in a file of its own: tests/test_csrc_self_contained.py fixes the set of ABI files.)"""
import os
import re

from tests import _abi

ROOT, CSRC = _abi.ROOT, _abi.CSRC
WIDTHS = (4, 8, 12, 16, 24, 32)


def test_mode_kernel_uses_no_scratch(tmp_path):
    inst = ["template __global__ void k_vp_mode<%d>(ModeArgs);" % dt for dt in WIDTHS]
    kernels, asm = _abi.kernel_meta("mode_kernels.h", inst, r"k_vp_mode", tmp_path)
    seen = {k["targs"]: (k["vgpr_spill_count"], k["private_segment_fixed_size"], k["max_flat_workgroup_size"], k["wavefront_size"]) for k in kernels}
    print({k["targs"]: (k["vgpr_count"], k["sgpr_spill_count"], k["group_segment_fixed_size"]) for k in kernels})
    src = open(os.path.join(CSRC, "mode_kernels.h")).read()
    assert set(re.findall(r"__global__[^\n]*\b(k_\w+)\(", src)) == {"k_vp_mode"}                   # every kernel of the header
    threads = 64 * int(re.search(r"#define MODE_W (\d+)", src).group(1))
    assert threads == 256 and "#define MODE_T (64 * MODE_W)" in src and "__launch_bounds__(MODE_T)" in src
    assert sorted(seen) == [(dt,) for dt in WIDTHS], sorted(seen)
    for dt, got in seen.items():
        assert got == (0, 0, threads, 64), (dt, got)                                              # no scratch; wave64; the declared size
    for k in kernels:
        assert k["group_segment_fixed_size"] <= 64 * 1024, k["mangled"]                           # static LDS
    for k in ("exp", "log", "log1p", "tanh"):                                                     # no device-library transcendental
        assert not re.search(r"__ocml_%s_f64" % k, asm), k
    assert "atomic" not in src.lower().replace("no atomics", "")


def test_the_files_are_part_of_the_build():
    build = open(os.path.join(ROOT, "vbmc_amd", "build.py")).read()
    unit = open(os.path.join(CSRC, "vbmc_hip.hip")).read()
    tools = open(os.path.join(CSRC, "abi_vp_tools.hip")).read()
    assert '"mode_kernels.h"' in build and '"mode_host.h"' in build and '"abi_vp_tools.hip"' in build
    assert '#include "abi_vp_tools.hip"' in unit and '#include "mode_host.h"' in tools
    assert '#include "mode_kernels.h"' in open(os.path.join(CSRC, "mode_host.h")).read()
    assert "k_vp_mode" not in open(os.path.join(CSRC, "vp_tools_kernels.h")).read()
    for fn in ("mode_kernels.h", "mode_host.h"):
        assert "oracle" not in open(os.path.join(CSRC, fn)).read()
    host = open(os.path.join(CSRC, "mode_host.h")).read()
    assert host.count("k_vp_mode<DT>") == 2 and "VPT_FOR_DT" in host                             # the ranking launch and the optimising one


def test_library_exports_vbmc_vp_mode():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    import vbmc_amd
    from vbmc_amd import _lib, vptools

    lib = _lib.load()
    hdr = _abi.header_text()
    assert hasattr(lib, "vbmc_vp_mode") and hasattr(vptools, "vbmc_mode") and vbmc_amd.vbmc_mode is vptools.vbmc_mode
    proto = re.search(r"vbmc_status vbmc_vp_mode\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(lib.vbmc_vp_mode.argtypes) == 3, proto
    assert lib.vbmc_vp_mode.argtypes[1] == C.POINTER(_lib.VpDesc) and lib.vbmc_vp_mode.argtypes[2] == C.POINTER(_lib.ModeArgs)
    assert [f[0] for f in _lib.ModeArgs._fields_] == _abi.header_structs()["vbmc_mode_args"]
    assert [f[0] for f in _lib.ModeArgs._fields_][:5] == ["struct_size", "nmax", "origflag", "max_iter", "tol_grad"]
    assert _lib.ModeArgs.__doc__.split()[0] == "vbmc_mode_args"
    enums = {k: v for k, v in _abi.header_enums().items() if k.startswith("VBMC_MODE_STOP_")}
    assert enums == {"VBMC_MODE_STOP_" + n.upper(): i for i, n in _lib.MODE_STOP.items()} and len(enums) == 3
    assert lib.vbmc_abi_version() == 8 and int(re.search(r"#define VBMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    # a null context is refused first (no device needed), whatever else is wrong
    d = _lib.new_args(_lib.VpDesc)
    a = _lib.new_args(_lib.ModeArgs)
    assert lib.vbmc_vp_mode(None, C.byref(d), C.byref(a)) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_vp_mode(None, None, None) == _lib.VBMC_ERR_INVALID
    a.struct_size += 8
    assert lib.vbmc_vp_mode(None, C.byref(d), C.byref(a)) == _lib.VBMC_ERR_INVALID
    # a stored mode needs no library call at all
    import numpy as np

    vp = {"D": 2, "K": 1, "mode": np.array([0.25, -1.0])}
    assert np.array_equal(vptools.vbmc_mode(vp), vp["mode"]) and vptools.vbmc_mode(vp, nargout=2)[1] is vp


def test_refusals_before_anything_is_read():
    """Without a device there is no context, and a null context is all the library can be shown (above).  What follows it is read from
    the entry point's text: a wrong struct_size, a tol_grad that is not positive (a NaN too), max_iter beyond the cap and a missing
    required output are refused (INVALID) before the posterior is looked at; the posterior's own checks (types 4 .. 13 UNSUPPORTED,
    a non-finite posterior INVALID) are vpt_pack's, as for vbmc_vp_pdf; nothing is uploaded or launched before them.
    tests/test_gpu_mode.py runs these refusals on a device."""
    src = open(os.path.join(CSRC, "abi_vp_tools.hip")).read()
    body = src[src.index('extern "C" vbmc_status vbmc_vp_mode'):]
    marks = ("if (!ctx)", "struct_size != sizeof(vbmc_mode_args)", "!(args->tol_grad > 0.0)", "args->max_iter > MODE_ITER_CAP", "!args->x || !args->fval || !args->idx",
             "vpt_pack(", "mode_run(")
    order = [body.index(s) for s in marks]
    assert order == sorted(order), order
    for i in range(1, 5):
        assert "VBMC_ERR_INVALID" in body[order[i]:order[i + 1]], marks[i]
    host = open(os.path.join(CSRC, "mode_host.h")).read()
    assert host.index("vpt_upload(") < host.index("hipLaunchKernelGGL") and "vpt_pack(" not in host
    kern = open(os.path.join(CSRC, "mode_kernels.h")).read()
    assert "#define MODE_ITER_CAP 1000" in kern and "#define MODE_DEFAULT_ITER 200" in kern and "#define MODE_DEFAULT_NMAX 20" in kern
    assert "iter >= MODE_ITER_CAP" in kern                                                        # the in-kernel loop is bounded by itself
    assert "VPT_LOG_DENORM_MIN" not in kern.split("#pragma once")[1]                              # the density rule of vpt_eval is not applied
