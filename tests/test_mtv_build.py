"""CPU check beside tests/test_vptools_build.py: the kernels of the marginal total variation (vbmc_amd/csrc/mtv_kernels.h under
abi_vp_mtv.hip) cross-compile for gfx950 and use no scratch -- no spilled vector register, no private segment, read from the
compiler's own resource-usage metadata -- and call no device-library transcendental, both files are part of the build, and the
library exports vbmc_vp_mtv with a ctypes declaration and an argument structure that follow the header."""
import os
import re
import subprocess

from tests.test_vptools_build import _struct_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("k_mtv_mesh", "k_mtv_bin", "k_mtv_init", "k_mtv_dct", "k_mtv_root", "k_mtv_integral")


def test_mtv_kernels_use_no_scratch(tmp_path):
    src = os.path.join(str(tmp_path), "mtv.hip")
    with open(src, "w") as f:
        f.write('#include "%s/mtv_kernels.h"\n' % CSRC)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
                        "--save-temps=obj", "-c", src, "-o", os.path.join(str(tmp_path), "mtv.o")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(os.path.join(str(tmp_path), "mtv-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = {}
    for rec in asm.split("  - .agpr_count:")[1:]:                                                  # one record per kernel
        name = re.search(r"\n    \.name:\s+(\S+)", rec).group(1)
        if "k_mtv_" in name:
            seen[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, rec).group(1))
                               for k in ("vgpr_spill_count", "private_segment_fixed_size", "max_flat_workgroup_size", "wavefront_size"))
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
    hdr = open(os.path.join(ROOT, "include", "vbmc_hip.h")).read()
    assert hasattr(lib, "vbmc_vp_mtv") and hasattr(vptools, "vbmc_mtv")
    proto = re.search(r"vbmc_status vbmc_vp_mtv\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(lib.vbmc_vp_mtv.argtypes) == 4, proto
    assert lib.vbmc_vp_mtv.argtypes[3] == C.POINTER(_lib.MtvArgs)
    assert _struct_names(hdr, "vbmc_mtv_args") == [f[0] for f in _lib.MtvArgs._fields_]
    # the field types: every pointer 8 bytes, Ns and seed 64 bits, in the header's order -> the same layout on both sides
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct vbmc_mtv_args \{(.*?)\} vbmc_mtv_args;", hdr, re.S).group(1), flags=re.S)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    want = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            t = re.sub(r"^const\s+", "", decl).split()[0].rstrip("*")
            base = C.c_double if t == "double" else ctype[t]
            want.append(C.POINTER(base) if "*" in decl else base)
    assert want == [f[1] for f in _lib.MtvArgs._fields_]
    assert lib.vbmc_abi_version() == 8 and int(re.search(r"#define VBMC_ABI_VERSION (\d+)", hdr).group(1)) == 8
    # a null context is refused first, a wrong struct_size before anything is read (no device needed)
    d = _lib.VpDesc()
    d.struct_size = C.sizeof(_lib.VpDesc)
    a = _lib.MtvArgs()
    a.struct_size = C.sizeof(_lib.MtvArgs)
    assert lib.vbmc_vp_mtv(None, C.byref(d), C.byref(d), C.byref(a)) == _lib.VBMC_ERR_INVALID
    a.struct_size = C.sizeof(_lib.MtvArgs) + 8
    assert lib.vbmc_vp_mtv(None, C.byref(d), C.byref(d), C.byref(a)) == _lib.VBMC_ERR_INVALID
    assert lib.vbmc_vp_mtv(None, C.byref(d), C.byref(d), None) == _lib.VBMC_ERR_INVALID
