"""CPU check beside tests/test_acqsearch_iqr_build.py: the kernels of the device-resident importance sampler
(vbmc_amd/csrc/is_sample_kernels.h) compile for gfx950 with no spilled vector registers and no private segment -- k_is_pred for every
inner dimension QS = ceil(D / 4) = 1 .. 8 --, the prediction runs on the fp64 matrix instruction, and the library exports
vbmc_acq_is_sample and vbmc_acq_is_sample_rng_dump with their ctypes declarations under ABI 8."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_is_sample_kernels_do_not_spill(tmp_path):
    src = os.path.join(str(tmp_path), "is.hip")
    with open(src, "w") as f:
        f.write('#include "%s/is_sample_kernels.h"\n' % CSRC)
        for qs in range(1, 9):
            f.write("template __global__ void k_is_pred<%d>(IsPredArgs);\n" % qs)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
                        "--save-temps=obj", "-c", src, "-o", os.path.join(str(tmp_path), "is.o")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(os.path.join(str(tmp_path), "is-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = set()
    for m in re.finditer(r"\.name:\s+_Z(\d+)(k_is_\S*)\n(.*?)\.wavefront_size", asm, re.S):
        name, rest, meta = m.group(2)[: int(m.group(1))], m.group(2)[int(m.group(1)):], m.group(3)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        priv = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        assert spill == 0 and priv == 0, (name, spill, priv)
        qs = re.match(r"ILi(\d+)E", rest)                      # the template argument of k_is_pred<QS>
        seen.add(name + (qs.group(1) if qs else ""))
    assert seen == {"k_is_step", "k_is_finish"} | {"k_is_pred%d" % q for q in range(1, 9)}, seen
    assert "v_mfma_f64_16x16x4" in asm


def test_library_exports_the_sampler():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "vbmc_acq_is_sample") and len(lib.vbmc_acq_is_sample.argtypes) == 3
    assert hasattr(lib, "vbmc_acq_is_sample_rng_dump") and len(lib.vbmc_acq_is_sample_rng_dump.argtypes) == 5
    hdr = open(os.path.join(ROOT, "include", "vbmc_hip.h")).read()
    assert re.search(r"vbmc_status vbmc_acq_is_sample\(vbmc_ctx\* ctx, const vbmc_gp\* gp, const vbmc_is_sample_args\* args\);", hdr)
    assert re.search(r"vbmc_status vbmc_acq_is_sample_rng_dump\(uint64_t seed, int S, int H, int M, double\* U\);", hdr)
    assert "#define VBMC_ABI_VERSION 8" in hdr and lib.vbmc_abi_version() == 8
    # the struct the mirror declares has the fields, in order, of the header's
    body = re.search(r"typedef struct vbmc_is_sample_args \{(.*?)\} vbmc_is_sample_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names.append(re.sub(r"[\s*]", "", first.split()[-1]))
            names += [re.sub(r"[\s*]", "", t) for t in rest]
    assert names == [f[0] for f in _lib.IsSampleArgs._fields_], names
    # a wrong struct_size is refused before anything is read (no device needed: the context pointer is checked first)
    a = _lib.IsSampleArgs()
    a.struct_size = C.sizeof(_lib.IsSampleArgs)
    assert lib.vbmc_acq_is_sample(None, None, C.byref(a)) == 1
