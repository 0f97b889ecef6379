"""CPU check beside tests/test_acqsearch_build.py: the kernels of the IQR acquisition search (vbmc_amd/csrc/iqr_tile_kernels.h) compile
for gfx950 with no spilled vector registers and no private segment, and the library exports vbmc_acq_search_iqr with its ctypes
declaration.  The tile kernel is not templated on the number of importance-point tiles NT = Nap / 16: a workgroup owns ONE tile (grid
(NT, S)), so one instantiation covers NT = 1 .. 16; the check walks every kernel of the header it finds in the code object."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_iqr_tile_kernels_do_not_spill(tmp_path):
    src = os.path.join(str(tmp_path), "it.hip")
    with open(src, "w") as f:
        f.write('#include "%s/iqr_tile_kernels.h"\n' % CSRC)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
                        "--save-temps=obj", "-c", src, "-o", os.path.join(str(tmp_path), "it.o")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(os.path.join(str(tmp_path), "it-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = set()
    for m in re.finditer(r"\.name:\s+_Z(\d+)(k_(?:acq_iqr_tile|iqr_tile_final)\S*)\n(.*?)\.wavefront_size", asm, re.S):
        name, meta = m.group(2)[: int(m.group(1))], m.group(3)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        priv = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        assert spill == 0 and priv == 0, (name, spill, priv)
        seen.add(name)
    assert seen == {"k_acq_iqr_tile", "k_iqr_tile_final"}, seen
    assert "v_mfma_f64_16x16x4" in asm


def test_library_exports_the_iqr_search():
    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "vbmc_acq_search_iqr") and len(lib.vbmc_acq_search_iqr.argtypes) == 4
    hdr = open(os.path.join(ROOT, "include", "vbmc_hip.h")).read()
    assert re.search(r"vbmc_status vbmc_acq_search_iqr\(vbmc_ctx\* ctx, const vbmc_gp\* gp, const vbmc_acq_is\* is, const vbmc_acqsearch_args\* args\);", hdr)
    assert "#define VBMC_ABI_VERSION 8" in hdr and lib.vbmc_abi_version() == 8
