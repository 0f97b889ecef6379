"""CPU check beside tests/test_acqsearch_build.py: the kernels of the IQR acquisition search (vbmc_amd/csrc/iqr_tile_kernels.h) compile
for gfx950 with no spilled vector registers and no private segment, and the library exports vbmc_acq_search_iqr with its ctypes
declaration.  The tile kernel is not templated on the number of importance-point tiles NT = Nap / 16: a workgroup owns ONE tile (grid
(NT, S)), so one instantiation covers NT = 1 .. 16; the check walks every kernel of the header it finds in the code object."""
import re

from tests import _abi



def test_iqr_tile_kernels_do_not_spill(tmp_path):
    kernels, asm = _abi.kernel_meta("iqr_tile_kernels.h", (), r"k_(acq_iqr_tile|iqr_tile_final)", tmp_path)
    seen = set()
    for k in kernels:
        assert _abi.no_scratch(k), k
        seen.add(k["name"])
    assert seen == {"k_acq_iqr_tile", "k_iqr_tile_final"}, seen
    assert "v_mfma_f64_16x16x4" in asm


def test_library_exports_the_iqr_search():
    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "vbmc_acq_search_iqr") and len(lib.vbmc_acq_search_iqr.argtypes) == 4
    hdr = _abi.header_text()
    assert re.search(r"vbmc_status vbmc_acq_search_iqr\(vbmc_ctx\* ctx, const vbmc_gp\* gp, const vbmc_acq_is\* is, const vbmc_acqsearch_args\* args\);", hdr)
    assert "#define VBMC_ABI_VERSION 8" in hdr and lib.vbmc_abi_version() == 8
