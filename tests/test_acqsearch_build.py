"""CPU check beside tests/test_slice_build.py: the acquisition search's kernel k_search_step (vbmc_amd/csrc/search_kernels.h) compiles
for gfx950 with no spilled vector registers and no private segment (the criterion of tests/test_quad_build.py) (its matrices live in LDS; one wave walks the whole update, a spill would
put every generation's sequential tail through scratch memory), and the library exports the entry points with a host-only generator
that is the inverse normal CDF of its own uniforms."""
import statistics

import numpy as np

from tests import _abi



def test_search_kernel_does_not_spill(tmp_path):
    kernels, _ = _abi.kernel_meta("search_kernels.h", (), r"k_search_", tmp_path)
    seen = set()
    for k in kernels:
        assert _abi.no_scratch(k), k
        seen.add(k["name"])
    assert seen == {"k_search_step"}, seen


def test_library_exports_the_search_and_its_generator():
    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib
    from vbmc_amd.acq import acq_search_rng_dump

    lib = _lib.load()
    assert hasattr(lib, "vbmc_acq_search") and hasattr(lib, "vbmc_acq_search_rng_dump")
    # the host generator: deterministic in (seed, generation, point, d), independent of the block's extent, standard normal
    Z = acq_search_rng_dump(99, 5, 8, 300)
    assert np.array_equal(Z[:, :, :7], acq_search_rng_dump(99, 5, 8, 7)) and not np.array_equal(Z, acq_search_rng_dump(100, 5, 8, 300))
    z = np.sort(Z.ravel())
    n = z.size
    q = np.array([statistics.NormalDist().inv_cdf((i + 0.5) / n) for i in range(n)])
    assert np.max(np.abs(z - q)[n // 100: -n // 100]) < 0.06 and abs(z.mean()) < 0.03 and abs(z.std() - 1) < 0.03
