"""CPU: static sanity of the shim matlab/vbmc_hip_mtv.m, in the style of tests/test_matlab_vptools_static.py (there is no MATLAB here to
run it): the gateway implements its command with the argument count the shim passes, its inputs and outputs are the reference
function's in the reference's order (recorded as lists of names in tests/golden/reference_mtv_signature.json), it falls through to
the reference function when an argument is not a variational posterior or on 'vbmc_hip:unsupported', takes its seed from one randi,
contains no arithmetic of the estimator, and no same-named vbmc_mtv.m exists."""
import json
import os
import re

from tests import _mex
from tests.test_matlab_static import _block, _signature, strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "matlab", "vbmc_hip_mtv.m")


def test_block_keywords_balance():
    code = strip(open(SHIM).read())
    opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
    ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
    assert opens == ends, (opens, ends)


def test_signature_equals_the_reference():
    with open(os.path.join(ROOT, "tests", "golden", "reference_mtv_signature.json")) as f:
        (rname, routs, rargs), = json.load(f)["signatures"]["vbmc_mtv.m"]
    got, outs, args = _signature(SHIM)
    assert got == "vbmc_hip_mtv" and rname == "vbmc_mtv"
    assert outs == routs and args == rargs, (outs, args)
    assert not os.path.exists(os.path.join(ROOT, "matlab", "vbmc_mtv.m")), "the vp tools are reached by their vbmc_hip_ names alone"


def test_gateway_command_and_argument_count():
    cmds, blk = _mex.gateway_commands(), _mex.gateway_block("vp_mtv")
    src = open(SHIM).read()
    assert set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", src)) == {"vp_mtv"}
    assert "vp_mtv" in cmds and "vbmc_vp_mtv(g_ctx" in blk
    min_nrhs, handles, usage, _ = cmds["vp_mtv"]
    calls = re.findall(r"vbmc_hip_mex\('vp_mtv',([^;]*)\);", src)
    assert len(calls) == 3 and {len(c.split(",")) for c in calls} == {4}, calls               # nargout 3, 2, 1: vp1, vp2, Ns, seed
    assert all(c.startswith("vp1,vp2,Ns,") for c in calls), calls                              # the reference's order, then the seed
    assert min_nrhs == 5 and handles == 0                                                      # the command's name + 4 arguments
    assert [t.strip() for t in usage.split(",")] == ["vp1", "vp2", "Ns", "seed"]
    for word in ("8192", "100000", "1e5", "exp(", "log(", "cos("):                           # logic-free: no default of the library is restated
        assert word not in blk, word


def test_fall_through_edges():
    src = open(SHIM).read()
    code = strip(src)
    blk = _block(src, "try")
    assert "catch err" in blk and "vbmc_hip:unsupported" in blk and "rethrow(err)" in blk
    assert "randi(2^31-1)" in src
    assert "~isstruct(vp1) || ~isstruct(vp2)" in code                                          # a sample matrix: the reference
    head = code[:code.index("try")]
    assert "vbmc_hip_mtv_reference(vp1,vp2,Ns,nargout)" in head and "return" in head
    assert len(re.findall(r"(?<![\w_])vbmc_mtv\(vp1,vp2,Ns\)", code)) == 2                   # the reference function is the fall-through
    assert "Ns = 1e5" in code                                                                   # vbmc_mtv.m:24


def test_no_estimator_arithmetic():
    code = strip(open(SHIM).read())
    for word in ("exp(", "log(", "sqrt(", "cos(", "fft(", "histc(", "interp1(", "kde1d(", "qtrapz(", "linspace(", "sum(", "min(", "max(", "vbmc_rnd("):
        assert word not in code, word


def test_documents_name_the_command_and_the_shim():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`vp_mtv`" in doc and "vbmc_hip_mtv" in doc and "vbmc_vp_mtv" in doc
