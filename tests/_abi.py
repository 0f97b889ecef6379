"""CPU helpers shared by the build tests and tests/test_abi_symbols.py: one reader of include/vbmc_hip.h, the header's layout as the
host C compiler sees it, and the gfx950 cross-compile with the per-kernel metadata the compiler writes beside the assembly."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "vbmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def header_text(comments=True):
    txt = open(os.path.join(INCLUDE, "vbmc_hip.h")).read()
    return txt if comments else re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


_CTYPE = {"uint8_t": C.c_uint8, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}


def header_fields():
    """{struct: [(field, ctypes type)] in order} for every ``typedef struct vbmc_* { ... } vbmc_*;`` of the header; arrays
    (``int32_t noisefun[3]``) and several declarators on a line (``const double *LB, *UB``) included.  ``void*`` and a pointer to one of the
    library's opaque handles are c_void_p."""
    out = {}
    for name, body in re.findall(r"typedef struct (vbmc_\w+) \{(.*?)\} \1;", header_text(False), re.S):
        out[name] = []
        for decl in (d.strip() for d in body.split(";") if d.strip()):
            base = re.sub(r"^const\s+", "", decl).split()[0].rstrip("*")
            for i, d in enumerate(decl.split(",")):
                t, depth = _CTYPE.get(base), d.count("*")
                if t is None:                                   # void, vbmc_acq_is: only ever behind a pointer
                    t, depth = C.c_void_p, depth - 1
                for _ in range(depth):
                    t = C.POINTER(t)
                arr = re.search(r"\[(\d+)\]", d)
                out[name].append((re.sub(r"\[.*?\]|[\s*]", "", d.split()[-1]), t * int(arr.group(1)) if arr else t))
    return out


def header_structs():
    """{struct: [field names in order]} of header_fields()"""
    return {s: [n for n, _ in fields] for s, fields in header_fields().items()}


def header_enums():
    """{VBMC_NAME: value} of every enumerator and every numeric #define of the header"""
    txt = header_text(False)
    return {k: int(v) for k, v in re.findall(r"\b(VBMC_[A-Z0-9_]+)\s*=\s*(\d+)", txt) + re.findall(r"#define\s+(VBMC_[A-Z0-9_]+)\s+(\d+)\b", txt)}


def header_layout(tmp_path):
    """({struct: sizeof}, {"struct.field": (offsetof, sizeof)}) of every struct of header_structs(), printed by a generated C program that
    includes the header and is built with the host C compiler"""
    structs = header_structs()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vbmc_hip.h"', "int main(void) {"]
    for s, fields in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f) for f in fields]
    src, exe = os.path.join(str(tmp_path), "layout.c"), os.path.join(str(tmp_path), "layout")
    with open(src, "w") as f:
        f.write("\n".join(lines + ["  return 0;", "}", ""]))
    r = subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I" + INCLUDE, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    sizes, fields = {}, {}
    for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n"):
        w = ln.split()
        if len(w) == 2:
            sizes[w[0]] = int(w[1])
        elif len(w) == 3:
            fields[w[0]] = (int(w[1]), int(w[2]))
    return sizes, fields


def kernel_meta(header, instantiations, pattern, tmp_path, flags=()):
    """Cross-compile for gfx950, keeping the assembly: ``header`` of vbmc_amd/csrc with the explicit ``instantiations`` (lines of C++)
    behind it, or -- a name ending in .hip -- that translation unit as it is.  Returns (kernels, asm): for every kernel whose name
    matches ``pattern`` a dict with ``name``, ``mangled``, ``targs`` (the integer and boolean template arguments) and every integer
    entry of the kernel's metadata record -- vgpr_spill_count, private_segment_fixed_size, sgpr_spill_count, vgpr_count,
    max_flat_workgroup_size, wavefront_size ... -- and the whole assembly text."""
    tmp = str(tmp_path)
    os.makedirs(tmp, exist_ok=True)
    if header.endswith(".hip"):
        src = os.path.join(CSRC, header)
    else:
        src = os.path.join(tmp, "unit.hip")
        with open(src, "w") as f:
            f.write('#include "%s/%s"\n' % (CSRC, header) + "".join(ln.rstrip("\n") + "\n" for ln in instantiations))
    stem = os.path.splitext(os.path.basename(src))[0]
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + INCLUDE, *flags, "--save-temps=obj",
                        "-c", src, "-o", os.path.join(tmp, stem + ".o")], capture_output=True, text=True, cwd=tmp)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(os.path.join(tmp, stem + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    kernels = []
    for rec in re.split(r"\n  - (?=\.)", asm[asm.index("amdhsa.kernels:"):])[1:]:          # one record per kernel
        meta = dict(re.findall(r"^    \.(\w+):\s+(\S+)$", "    " + rec, re.M))
        m = re.match(r"_Z(\d+)(.*)", meta["name"])
        name, rest = (m.group(2)[: int(m.group(1))], m.group(2)[int(m.group(1)):]) if m else (meta["name"], "")
        if re.match(pattern, name):
            t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
            k = {key: int(v) for key, v in meta.items() if v.isdigit()}
            k.update(name=name, mangled=meta["name"], targs=tuple(int(x) for x in re.findall(r"L[ib](\d+)E", t.group(1))) if t else ())
            kernels.append(k)
    return kernels, asm


def no_scratch(k):
    """the criterion every build test applies: no spilled vector register, no private segment"""
    return k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0
