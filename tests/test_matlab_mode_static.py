"""CPU: static sanity of the shim matlab/vbmc_hip_mode.m, in the style of tests/test_matlab_diag_static.py (there is no MATLAB here to
run it): its inputs and outputs are the reference function's in the reference's order (recorded as lists of names in
tests/golden/reference_mode_signature.json); it calls only the gateway's 'vp_mode' command, with the arguments the gateway counts and
names; it takes the reference's stored-mode shortcut and stores the mode as the reference does; it falls through to vbmc_mode on
'vbmc_hip:unsupported'; every default tests nargin against the argument's own position; neither the shim nor the gateway's handler
contains arithmetic; no same-named vbmc_mode.m exists; the documents name the command, the shim and the entry point."""
import json
import os
import re

from tests import _mex
from tests.test_matlab_static import _block, _signature, strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "matlab", "vbmc_hip_mode.m")


def test_block_keywords_balance():
    code = strip(open(SHIM).read())
    opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
    ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
    assert opens == ends, (opens, ends)


def test_signature_equals_the_reference():
    with open(os.path.join(ROOT, "tests", "golden", "reference_mode_signature.json")) as f:
        (rname, routs, rargs), = json.load(f)["signatures"]["vbmc_mode.m"]
    got, outs, args = _signature(SHIM)
    assert got == "vbmc_hip_mode" and rname == "vbmc_mode"
    assert outs == routs == ["x", "vp"] and args == rargs == ["vp", "nmax", "origflag"], (outs, args)
    assert not os.path.exists(os.path.join(ROOT, "matlab", "vbmc_mode.m")), "the optimiser is the library's: no same-named shim"


def test_gateway_command_and_argument_count():
    cmds, blk = _mex.gateway_commands(), _mex.gateway_block("vp_mode")
    src = open(SHIM).read()
    assert set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", src)) == {"vp_mode"}
    assert "vp_mode" in cmds and "vbmc_vp_mode(g_ctx" in blk
    min_nrhs, handles, usage, handler = cmds["vp_mode"]
    calls = re.findall(r"vbmc_hip_mex\('vp_mode',([^;]*)\);", src)
    assert calls == ["vp,nmax,origflag,1e-6"], calls                                              # the reference's order, then the tolerance
    names = [t.strip() for t in usage.split(",")]
    assert names == ["vp", "nmax", "origflag", "tol_grad"] and min_nrhs == len(names) + 1 and handles == 0 and handler == "cmd_vp_mode"
    assert max(int(i) for i in re.findall(r"prhs\[(\d+)\]", blk)) == min_nrhs - 1                 # every counted argument is read, none beyond
    rows = [r[0] for r in _mex.gateway_rows()]
    assert rows.index("vp_mode") == rows.index("vp_diag") + 1


def test_handler_is_logic_free():
    blk = _mex.gateway_block("vp_mode")
    code = "\n".join(ln.split("//")[0] for ln in blk.split("\n"))
    for word in ("1e-6", "200", "1000", "20", "exp(", "log(", "sqrt(", "fmax(", "std::max", "std::min", "isnan", "for (", "while ("):   # no default, no loop, no reduction
        assert word not in code, word
    assert not re.search(r"[\w\])]\s*[-+/]\s*[\w(]", code.replace("->", "")), "arithmetic in the handler"          # (* is the pointer's)
    assert blk.count("fill_vp_desc(") == 1 and "zeroed<vbmc_mode_args>()" in blk and code.rstrip().endswith("}")
    assert "return done(st);" in code


def test_shortcut_fall_through_and_defaults():
    src = open(SHIM).read()
    code = strip(src)
    blk = _block(src, "try")
    assert "catch err" in blk and "vbmc_hip:unsupported" in blk and "rethrow(err)" in blk
    assert len(re.findall(r"(?<![\w_])vbmc_mode\(vp,nmax,origflag\)", code)) == 1 and "x = vbmc_mode(vp,nmax,origflag);" in blk
    for pos, (name, default) in enumerate((("nmax", "20"), ("origflag", "true")), start=2):       # vbmc_mode.m:15-16
        assert re.search(r"if nargin < %d \|\| isempty\(%s\); %s = %s; end" % (pos, name, name, default), code), name
    head = code[:code.index("try")]
    assert "if origflag && isfield(vp,'') && ~isempty(vp.mode)" in head and "x = vp.mode;" in head and "return" in head      # :18-19 (strip() empties the literals)
    assert "if origflag && isfield(vp,'mode') && ~isempty(vp.mode)" in src
    tail = code[code.index("catch err"):]
    assert "if nargout > 1 && origflag" in tail and "vp.mode = x;" in tail                        # :53-55
    assert "randi" not in code                                                                     # nothing random in it


def test_no_arithmetic_in_the_shim():
    code = strip(open(SHIM).read())
    for word in ("exp(", "log(", "sqrt(", "sum(", "min(", "max(", "sort(", "fmincon", "fminunc", "vbmc_pdf(", "warpvars_vbmc(", "eps"):
        assert word not in code, word
    body = code[code.index("\n"):].replace("1e-6", "")
    assert not re.search(r"[\w)]\s*[-+*/^]\s*[\w(]", body), "arithmetic in the shim"


def test_documents_name_the_command_and_the_shim():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`vp_mode`" in doc and "vbmc_hip_mode" in doc and "vbmc_vp_mode" in doc
    assert "vbmc_hip_mode" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_vp_mode" in design and "vbmc_vp_mode" in design
