"""CPU check beside tests/test_issample_build.py: the translation unit of the one-call set-up (vbmc_amd/csrc/abi_is_setup.hip on top of
is_setup_kernels.h) cross-compiles for gfx950, its kernels k_is_draw, k_is_proposal and k_is_resample use no scratch -- no spilled
vector register, no private segment, read from the compiler's own resource-usage metadata --, and the library exports vbmc_acq_is_setup
and vbmc_acq_is_setup_rng_dump with ctypes declarations that follow the header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_is_setup_kernels_use_no_scratch(tmp_path):
    src = os.path.join(str(tmp_path), "iss.hip")
    with open(src, "w") as f:
        f.write('#include "%s/is_setup_kernels.h"\n' % CSRC)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
                        "--save-temps=obj", "-c", src, "-o", os.path.join(str(tmp_path), "iss.o")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(os.path.join(str(tmp_path), "iss-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = {}
    for m in re.finditer(r"\.name:\s+_Z(\d+)(k_is_\S*)\n(.*?)\.wavefront_size", asm, re.S):
        name, meta = m.group(2)[: int(m.group(1))], m.group(3)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        priv = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        seen[name] = (spill, priv)
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
    hdr = open(os.path.join(ROOT, "include", "vbmc_hip.h")).read()
    assert re.search(r"vbmc_status vbmc_acq_is_setup\(vbmc_ctx\* ctx, const vbmc_gp\* gp, const vbmc_is_setup_args\* args\);", hdr)
    assert re.search(r"vbmc_status vbmc_acq_is_setup_rng_dump\(uint64_t seed, int D, int S, int W, int Nvp, int Nbox, double\* B\);", hdr)
    # the struct the mirror declares has the fields, in order, of the header's
    body = re.search(r"typedef struct vbmc_is_setup_args \{(.*?)\} vbmc_is_setup_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names.append(re.sub(r"[\s*]", "", first.split()[-1]))
            names += [re.sub(r"[\s*]", "", t) for t in rest]
    assert names == [f[0] for f in _lib.IsSetupArgs._fields_], names
    # a wrong struct_size is refused before anything is read (no device needed: the context pointer is checked first)
    a = _lib.IsSetupArgs()
    a.struct_size = C.sizeof(_lib.IsSetupArgs)
    assert lib.vbmc_acq_is_setup(None, None, C.byref(a)) == 1
    # the sampler's entry point still answers as before the two were given a common routine
    b = _lib.IsSampleArgs()
    b.struct_size = C.sizeof(_lib.IsSampleArgs)
    assert lib.vbmc_acq_is_sample(None, None, C.byref(b)) == 1
