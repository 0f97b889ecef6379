"""CPU: libvbmc_hip.so loads and exports every symbol include/vbmc_hip.h declares."""
import ctypes
import os
import re

import pytest

from tests import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = set()
    for fn in os.listdir(os.path.join(ROOT, "include")):
        if not fn.endswith(".h"):
            continue
        txt = open(os.path.join(ROOT, "include", fn)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        for m in re.finditer(r"\b(vbmc_[a-z0-9_]+)\s*\(", txt):
            names.add(m.group(1))
    return sorted(names)


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g

    g.build()
    from vbmc_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 10
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.vbmc_abi_version() == _abi.header_enums()["VBMC_ABI_VERSION"] == _lib.ABI_VERSION


def test_variance_launch_record_matches_the_header():
    """vbmc_var_launch_info: the ctypes mirror has the header's fields in the header's order, and the enumerators the header's values"""
    from vbmc_amd import _lib

    fields = _abi.header_fields()["vbmc_var_launch_info"]
    assert fields[0] == ("struct_size", ctypes.c_uint32) and all(t is ctypes.c_int32 for _, t in fields[1:])
    assert [n for n, _ in fields] == [n for n, _ in _lib.VarLaunchInfo._fields_]
    assert ctypes.sizeof(_lib.VarLaunchInfo) == 4 * len(fields)
    enum = {k: v for k, v in _abi.header_enums().items() if k.startswith(("VBMC_VARSOLVE_", "VBMC_VARGRAM_"))}
    assert enum == {"VBMC_VARSOLVE_TRSM2": _lib.VARSOLVE_TRSM2, "VBMC_VARSOLVE_SLAB": _lib.VARSOLVE_SLAB,
                    "VBMC_VARGRAM_WAVE": _lib.VARGRAM_WAVE, "VBMC_VARGRAM_MFMA": _lib.VARGRAM_MFMA}
    from tests import _var_cases as C

    assert (C.TRSM2, C.SLAB, C.WAVE, C.MFMA) == (_lib.VARSOLVE_TRSM2, _lib.VARSOLVE_SLAB, _lib.VARGRAM_WAVE, _lib.VARGRAM_MFMA)


def test_every_mirror_has_the_headers_layout(tmp_path):
    """Every struct of include/vbmc_hip.h has exactly one ctypes mirror in _lib (named in the mirror's docstring), with the header's field
    names in the header's order and, field by field, the type the declaration stands for and the offset and size the host C compiler
    gives the header's struct.  (A field of the wrong type and the right size passes a comparison of names and the library's
    struct_size check, and then hands the library a wrong pointer.)  The enumerators and status codes _lib restates have the header's values."""
    from vbmc_amd import _lib, acq

    structs = _abi.header_fields()
    sizes, layout = _abi.header_layout(tmp_path)
    assert len(structs) >= 13 and set(sizes) == set(structs)
    mirrors = {}
    for cls in vars(_lib).values():
        if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure:
            mirrors.setdefault((cls.__doc__ or cls.__name__).split()[0], []).append(cls)
    assert sorted(mirrors) == sorted(structs), sorted(set(mirrors) ^ set(structs))       # a mirror each, none beside them
    for s, (cls, *more) in mirrors.items():
        assert not more, (s, cls, more)
        assert [n for n, _ in cls._fields_] == [n for n, _ in structs[s]], (s, cls._fields_)
        for (n, t), (_, want) in zip(cls._fields_, structs[s]):
            assert t is want, (s, n, t, want)                                            # the header's type, not merely its size
            assert (getattr(cls, n).offset, getattr(cls, n).size) == layout["%s.%s" % (s, n)], (s, n)
        assert ctypes.sizeof(cls) == sizes[s], (s, ctypes.sizeof(cls), sizes[s])
    enums = _abi.header_enums()
    restated = {k: v for k, v in enums.items() if re.match(r"VBMC_(ENTFORM|LJFORM|VARSOLVE|VARGRAM)_|VBMC_(OK|ERR_\w+)$", k)}
    assert len(restated) == 4 + 6 + 2 + 2 + 6, sorted(restated)
    for k, v in restated.items():
        assert getattr(_lib, k if k.startswith(("VBMC_OK", "VBMC_ERR")) else k[5:]) == v, k
        if k.startswith(("VBMC_OK", "VBMC_ERR")):
            assert _lib._STATUS_NAMES[v] == k[5:].replace("ERR_", ""), k
    assert enums["VBMC_ABI_VERSION"] == _lib.ABI_VERSION
    assert {v: k for k, v in enums.items() if k.startswith("VBMC_SEARCH_STOP_")} == \
        {i: "VBMC_SEARCH_STOP_" + n.upper() for i, n in acq.SEARCH_STOP.items()}


def test_no_cpu_fallback_without_gpu():
    """Without a gfx950 device the product path must fail loudly, never compute on the CPU."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import vbmc_amd

    with pytest.raises(vbmc_amd.VbmcHipError):
        vbmc_amd.Context(0)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "vbmc_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, fn)).read()
                assert "oracle" not in txt.replace("no CPU fallback", ""), os.path.join(dirpath, fn)


def test_entropy_plan_reporting_hook():
    """vbmc_entropy_plan is a pure host function (no device needed): the instantiation the library's policy picks.  Locks the
    choices the profiles were taken with: the headline shape runs three k-tiles + a two-component tail on one wave, configs[4]
    three k-tiles + tail on two waves, K = 64 four full k-tiles, D > 34 the VALU kernel."""
    import bench

    assert bench.entropy_kernel_label(10, 50) == "k_entropy_mfma<QS=3,KT=3+tail2,grad>"
    assert bench.entropy_kernel_label(20, 100) == "k_entropy_mfma<QS=6,KT=3+tail2,grad,HV=2>"
    assert bench.entropy_kernel_label(10, 64) == "k_entropy_mfma<QS=3,KT=4,grad>"
    assert bench.entropy_kernel_label(10, 56) == "k_entropy_mfma<QS=3,KT=3+tail8,grad>"
    assert bench.entropy_kernel_label(20, 56) == "k_entropy_mfma<QS=6,KT=4,grad>"          # two values per lane would spill there
    assert bench.entropy_kernel_label(6, 10) == "k_entropy_lane<DT=6,KP=10,grad> (+ log-joint role)"      # the small class (round 6)
    assert bench.entropy_kernel_label(13, 10) == "k_entropy_mfma<QS=4,KT=1,grad>"
    assert bench.entropy_kernel_label(6, 17) == "k_entropy_mfma<QS=2,KT=1+tail1,grad>"
    assert bench.entropy_kernel_label(10, 200) == "k_entropy_mfma<QS=3,KT=3+tail2,grad,HV=4>"
    assert bench.entropy_kernel_label(40, 10).startswith("k_entropy<D=40")


def test_limits_are_the_librarys_and_the_shims_ask_for_them():
    """vbmc_get_limits (a host function) reports what the validation enforces -- the numbers tests/test_gpu_limits.py exercises on the
    device (K = 400 of 512, N = 4500 of 9696) -- and the MATLAB side takes them from there: no shim restates a limit."""
    import ctypes as C
    import glob

    from vbmc_amd import _lib

    lib = _lib.load()
    lim = _lib.new_args(_lib.Limits)
    assert lib.vbmc_get_limits(C.byref(lim)) == 0
    assert (lim.max_D, lim.max_K, lim.max_N, lim.max_Na, lim.delta_ok, lim.meanfun_mask) == (32, 512, 9696, 256, 1, 0b10011)
    assert 3800 <= lim.max_T_vargrad <= 4100          # ("about 4000": five T-vectors beside the reduction scratch in 160 KB)
    bad = _lib.Limits(struct_size=4)
    assert lib.vbmc_get_limits(C.byref(bad)) != 0
    # the device tests reach into the upper half of each range
    txt = open(os.path.join(ROOT, "tests", "test_gpu_limits.py")).read()
    ks = [int(x) for x in re.findall(r"\(\d+, \d+, (\d+), \d, \d+\)", txt)]
    assert max(ks) > lim.max_K // 2 and max(ks) <= lim.max_K
    assert "4500" in txt and 4500 <= lim.max_N
    # no .m file carries the numbers (they drifted once: K <= 256 / N <= 3872 in round 5's shims against 512 / 9696 in the library)
    for f in glob.glob(os.path.join(ROOT, "matlab", "*.m")):
        code = "\n".join(ln.split("%")[0] for ln in open(f).read().split("\n"))
        assert not re.search(r"\bK\s*(<=|>)\s*\d{3}|\bD\s*(<=|>)\s*32\b|size\(gp\.X,1\)\s*<=\s*\d+", code), f
    sup = open(os.path.join(ROOT, "matlab", "vbmc_hip_supported.m")).read()
    assert "vbmc_hip_mex('limits')" in sup and "lim.max_K" in sup and "lim.max_N" in sup and "lim.delta_ok" in sup
