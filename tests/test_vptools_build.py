"""CPU check beside tests/test_issetup_build.py: the kernels of the variational-posterior tools (vbmc_amd/csrc/vp_tools_kernels.h under
abi_vp_tools.hip) cross-compile for gfx950 and use no scratch -- no spilled vector register, no private segment, read from the
compiler's own resource-usage metadata, for every instantiation of k_vp_pdf, k_vp_draw, k_vp_moments and k_vp_kldiv --, both files are
part of the build, and the library exports the five entry points with ctypes declarations that follow the header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("k_vp_pdf", "k_vp_draw", "k_vp_moments", "k_vp_kldiv")
ENTRY_POINTS = {"vbmc_vp_pdf": 10, "vbmc_vp_rnd": 10, "vbmc_vp_moments": 7, "vbmc_vp_kldiv": 10, "vbmc_vp_rnd_rng_dump": 8}


def test_vp_tools_kernels_use_no_scratch(tmp_path):
    src = os.path.join(str(tmp_path), "vpt.hip")
    with open(src, "w") as f:        # every instantiation the dispatch of abi_vp_tools.hip names
        f.write('#include "%s/vp_tools_kernels.h"\n' % CSRC)
        for dt in (4, 8, 12, 16, 24, 32):
            f.write("template __global__ void k_vp_pdf<%d, true>(VptPdfArgs);\ntemplate __global__ void k_vp_pdf<%d, false>(VptPdfArgs);\n" % (dt, dt))
            f.write("template __global__ void k_vp_draw<%d>(VptDrawArgs);\ntemplate __global__ void k_vp_moments<%d>(VptMomArgs);\n" % (dt, dt))
            f.write("template __global__ void k_vp_kldiv<%d>(VptKlArgs);\n" % dt)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
                        "--save-temps=obj", "-c", src, "-o", os.path.join(str(tmp_path), "vpt.o")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(os.path.join(str(tmp_path), "vpt-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = {}
    for m in re.finditer(r"\.name:\s+(_Z\d+k_vp_\S*)\n(.*?)\.wavefront_size", asm, re.S):
        meta = m.group(2)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        priv = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        seen[m.group(1)] = (spill, priv)
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


def _struct_names(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names.append(re.sub(r"[\s*]", "", first.split()[-1]))
            names += [re.sub(r"[\s*]", "", t) for t in rest]
    return names


def test_library_exports_the_vp_tools():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "vbmc_hip.h")).read()
    for name, nargs in ENTRY_POINTS.items():
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
        proto = re.search(r"vbmc_status %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(proto.split(",")) == nargs, (name, proto)
    assert _struct_names(hdr, "vbmc_vp_desc") == [f[0] for f in _lib.VpDesc._fields_]
    assert lib.vbmc_abi_version() == 8
    # a wrong struct_size is refused before anything is read; a null context is refused first (no device needed)
    d = _lib.VpDesc()
    d.struct_size = C.sizeof(_lib.VpDesc) + 8
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
