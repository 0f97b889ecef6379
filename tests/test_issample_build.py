"""CPU check beside tests/test_acqsearch_iqr_build.py: the kernels of the device-resident importance sampler
(vbmc_amd/csrc/is_sample_kernels.h) compile for gfx950 with no spilled vector registers and no private segment -- k_is_pred for every
inner dimension QS = ceil(D / 4) = 1 .. 8 --, the prediction runs on the fp64 matrix instruction, and the library exports
vbmc_acq_is_sample and vbmc_acq_is_sample_rng_dump with their ctypes declarations under ABI 8."""
import re

from tests import _abi



def test_is_sample_kernels_do_not_spill(tmp_path):
    inst = ["template __global__ void k_is_pred<%d>(IsPredArgs);" % qs for qs in range(1, 9)]
    kernels, asm = _abi.kernel_meta("is_sample_kernels.h", inst, r"k_is_", tmp_path)
    seen = set()
    for k in kernels:
        assert _abi.no_scratch(k), k
        seen.add(k["name"] + "".join(str(t) for t in k["targs"][:1]))      # the template argument of k_is_pred<QS>
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
    hdr = _abi.header_text()
    assert re.search(r"vbmc_status vbmc_acq_is_sample\(vbmc_ctx\* ctx, const vbmc_gp\* gp, const vbmc_is_sample_args\* args\);", hdr)
    assert re.search(r"vbmc_status vbmc_acq_is_sample_rng_dump\(uint64_t seed, int S, int H, int M, double\* U\);", hdr)
    assert "#define VBMC_ABI_VERSION 8" in hdr and lib.vbmc_abi_version() == 8
    # a wrong struct_size is refused before anything is read (no device needed: the context pointer is checked first)
    a = _lib.new_args(_lib.IsSampleArgs)
    assert lib.vbmc_acq_is_sample(None, None, C.byref(a)) == 1
