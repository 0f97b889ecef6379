"""CPU check beside tests/test_slice_build.py: the acquisition search's kernel k_search_step (vbmc_amd/csrc/search_kernels.h) compiles
for gfx950 with no spilled vector registers and no private segment (the criterion of tests/test_quad_build.py) (its matrices live in LDS; one wave walks the whole update, a spill would
put every generation's sequential tail through scratch memory), and the library exports the entry points with a host-only generator
that is the inverse normal CDF of its own uniforms."""
import os
import re
import statistics
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_search_kernel_does_not_spill(tmp_path):
    src = os.path.join(str(tmp_path), "sr.hip")
    with open(src, "w") as f:
        f.write('#include "%s/search_kernels.h"\n' % CSRC)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
                        "--save-temps=obj", "-c", src, "-o", os.path.join(str(tmp_path), "sr.o")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(os.path.join(str(tmp_path), "sr-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = set()
    for m in re.finditer(r"\.name:\s+_Z(\d+)(k_search_\S*)\n(.*?)\.wavefront_size", asm, re.S):
        name, meta = m.group(2)[: int(m.group(1))], m.group(3)
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        priv = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        assert spill == 0 and priv == 0, (name, spill, priv)
        seen.add(name)
    assert seen == {"k_search_step"}, seen


def test_library_exports_the_search_and_its_generator():
    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib
    from vbmc_amd.acq import acq_search_rng_dump

    lib = _lib.load()
    assert hasattr(lib, "vbmc_acq_search") and hasattr(lib, "vbmc_acq_search_rng_dump")
    hdr = open(os.path.join(ROOT, "include", "vbmc_hip.h")).read()
    body = re.search(r"typedef struct vbmc_acqsearch_args \{(.*?)\} vbmc_acqsearch_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    hdr_fields = [n for n in re.findall(r"[\s\*](\w+)\s*[,;]", body)]
    assert hdr_fields == [f[0] for f in _lib.AcqSearchArgs._fields_], hdr_fields
    # the host generator: deterministic in (seed, generation, point, d), independent of the block's extent, standard normal
    Z = acq_search_rng_dump(99, 5, 8, 300)
    assert np.array_equal(Z[:, :, :7], acq_search_rng_dump(99, 5, 8, 7)) and not np.array_equal(Z, acq_search_rng_dump(100, 5, 8, 300))
    z = np.sort(Z.ravel())
    n = z.size
    q = np.array([statistics.NormalDist().inv_cdf((i + 0.5) / n) for i in range(n)])
    assert np.max(np.abs(z - q)[n // 100: -n // 100]) < 0.06 and abs(z.mean()) < 0.03 and abs(z.std() - 1) < 0.03
