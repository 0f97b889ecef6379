"""CPU check beside tests/test_mtv_build.py: the kernels of the multi-run diagnostics (vbmc_amd/csrc/diag_kernels.h under
abi_vp_diag.hip) cross-compile for gfx950 in every instantiation the dispatch names and use no scratch -- no spilled vector register,
no private segment, read from the compiler's own resource-usage metadata -- and call no device-library transcendental, both files
are part of the build, and the library exports vbmc_vp_diagnostics with a ctypes declaration and an argument structure that follow
the header field for field; the ABI version is unchanged; what the entry point refuses before it reads anything is refused without
a device."""
import os
import re
import subprocess

from tests.test_vptools_build import _struct_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = {"k_diag_cross_kl": (6, 128), "k_diag_dct": (1, 256), "k_diag_integral": (1, 256)}      # instantiations, threads per workgroup


def test_diag_kernels_use_no_scratch(tmp_path):
    src = os.path.join(str(tmp_path), "diag.hip")
    with open(src, "w") as f:
        f.write('#include "%s/diag_kernels.h"\n' % CSRC)
        for dt in (4, 8, 12, 16, 24, 32):
            f.write("template __global__ void k_diag_cross_kl<%d>(DiagKlArgs);\n" % dt)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
                        "--save-temps=obj", "-c", src, "-o", os.path.join(str(tmp_path), "diag.o")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(os.path.join(str(tmp_path), "diag-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = {}
    for rec in asm.split("  - .agpr_count:")[1:]:                                                  # one record per kernel
        name = re.search(r"\n    \.name:\s+(\S+)", rec).group(1)
        if "k_diag_" in name:
            seen[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, rec).group(1))
                               for k in ("vgpr_spill_count", "private_segment_fixed_size", "max_flat_workgroup_size", "wavefront_size"))
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
    hdr = open(os.path.join(ROOT, "include", "vbmc_hip.h")).read()
    assert hasattr(lib, "vbmc_vp_diagnostics") and hasattr(vptools, "vbmc_diagnostics") and vbmc_amd.vbmc_diagnostics is vptools.vbmc_diagnostics
    proto = re.search(r"vbmc_status vbmc_vp_diagnostics\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(lib.vbmc_vp_diagnostics.argtypes) == 4, proto
    assert lib.vbmc_vp_diagnostics.argtypes[1] == C.c_int32
    assert lib.vbmc_vp_diagnostics.argtypes[2] == C.POINTER(C.POINTER(_lib.VpDesc))
    assert lib.vbmc_vp_diagnostics.argtypes[3] == C.POINTER(_lib.DiagArgs)
    assert _struct_names(hdr, "vbmc_diag_args") == [f[0] for f in _lib.DiagArgs._fields_]
    # the field types: every pointer 8 bytes, Ns and seed 64 bits, in the header's order -> the same layout on both sides
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct vbmc_diag_args \{(.*?)\} vbmc_diag_args;", hdr, re.S).group(1), flags=re.S)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    want = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            t = re.sub(r"^const\s+", "", decl).split()[0].rstrip("*")
            base = C.c_double if t == "double" else ctype[t]
            want.append(C.POINTER(base) if "*" in decl else base)
    assert want == [f[1] for f in _lib.DiagArgs._fields_]
    assert [f[0] for f in _lib.DiagArgs._fields_][:5] == ["struct_size", "nkde", "nquad", "Ns", "seed"]
    assert lib.vbmc_abi_version() == 8 and int(re.search(r"#define VBMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    # a null context is refused first (no device needed)
    d = _lib.VpDesc()
    d.struct_size = C.sizeof(_lib.VpDesc)
    arr = (C.POINTER(_lib.VpDesc) * 2)(C.pointer(d), C.pointer(d))
    a = _lib.DiagArgs()
    a.struct_size = C.sizeof(_lib.DiagArgs)
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
    assert re.search(r'"run %d, dimension %d: [^"]*fminbnd', body)                                # the message names run and dimension
    assert "#define DIAG_MAXR 32" in open(os.path.join(CSRC, "diag_kernels.h")).read()
    lib = _lib.load()
    a = _lib.DiagArgs()
    a.struct_size = C.sizeof(_lib.DiagArgs) + 8
    assert lib.vbmc_vp_diagnostics(None, 2, None, C.byref(a)) == _lib.VBMC_ERR_INVALID
