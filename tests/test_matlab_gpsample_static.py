"""CPU: static sanity of the same-named shim matlab/gpsample_vbmc.m, in the style of tests/test_matlab_mtv_static.py (there is no MATLAB
here to run it): its function line is the reference's (names recorded in tests/golden/reference_gpsample_signature.json), the gateway
implements its command with the argument count the shim passes, it falls through to the reference function on
'vbmc_hip:unsupported', takes its seed from one randi, holds no arithmetic of the sampler or of the transform, and the 'gp' branch of
matlab/vbmc_hip_rnd.m still goes to the reference's vbmc_rnd, which finds the shim by path lookup."""
import json
import os
import re

from tests import _mex
from tests.test_matlab_static import _block, _signature, calls, strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "matlab", "gpsample_vbmc.m")


def test_block_keywords_balance():
    code = strip(open(SHIM).read())
    opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
    ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
    assert opens == ends, (opens, ends)


def test_signature_equals_the_reference():
    with open(os.path.join(ROOT, "tests", "golden", "reference_gpsample_signature.json")) as f:
        (rname, routs, rargs), = json.load(f)["signatures"]["gpsample_vbmc.m"]
    got, outs, args = _signature(SHIM)
    assert got == rname == "gpsample_vbmc"
    assert outs == routs and args == rargs, (outs, args)


def test_gateway_command_and_argument_count():
    cmds, blk = _mex.gateway_commands(), _mex.gateway_block("gp_surrogate_sample")
    src = open(SHIM).read()
    assert set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", src)) == {"gp_surrogate_sample"}
    assert "gp_surrogate_sample" in cmds and "vbmc_gp_surrogate_sample(g_ctx" in blk
    min_nrhs, handles, usage, _ = cmds["gp_surrogate_sample"]
    (call,) = re.findall(r"vbmc_hip_mex\('gp_surrogate_sample',([^;]*)\);", src)
    args = re.sub(r"\([^()]*\)", "", call).split(",")                                             # (nested parentheses dropped)
    assert len(args) == 8 and args[0] == "vbmc_hip_gp_handle" and args[1:3] == ["vp", "Ns"] and args[-2:] == ["noise", "opts"], args
    assert min_nrhs == 9                                                                          # the command's name + 8 arguments
    assert [t.strip() for t in usage.split(",")] == ["h", "vp", "Ns", "origflag", "LB", "UB", "noise", "opts"]
    assert handles == 1
    for word in ("20000", "2e4", "exp(", "log(", "sqrt(", "ceil("):                                # logic-free: no default of the library is restated
        assert word not in blk, word


def test_fall_through_and_draws():
    src = open(SHIM).read()
    code = strip(src)
    blk = _block(src, "try")
    assert "catch err" in blk and "vbmc_hip:unsupported" in blk and "rethrow(err)" in blk
    assert "vbmc_hip_reference(''" in code and "ref(vp,gp,Ns,origflag)" in code
    assert calls(src) == ["randi"] and "randi(2^31-1)" in src                                      # one draw: the device stream's seed
    assert "origflag = true" in code                                                               # the reference's default
    for word in ("warpvars", "vbmc_rnd(", "gplite_sample(", "eissample", "sq_dist(", "sqrt(", "log("):
        assert word not in code, word
    rnd = strip(open(os.path.join(ROOT, "matlab", "vbmc_hip_rnd.m")).read())
    assert "ischar(balanceflag)" in rnd and "vbmc_rnd(vp,N,origflag,balanceflag,df)" in rnd        # 'gp': the reference's vbmc_rnd


def test_documents_name_the_command_and_the_shim():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`gp_surrogate_sample`" in doc and "gpsample_vbmc" in doc and "vbmc_gp_surrogate_sample" in doc
