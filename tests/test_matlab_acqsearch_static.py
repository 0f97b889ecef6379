"""CPU: static sanity of matlab/vbmc_hip_acqsearch.m in the style of tests/test_matlab_static.py (there is no MATLAB here to run it):
balanced block keywords, a function line named after the file that takes cmaes_modded's arguments at private/activesample_vbmc.m:282-283
and returns its six outputs, one gateway command that the gateway implements with the argument count the shim passes, a fall-through
to cmaes_modded for everything the device search refuses, and the documented one-line replacement."""
import os
import re

from tests import _mex
from tests.test_matlab_static import _block, _signature, calls, strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFILE = os.path.join(ROOT, "matlab", "vbmc_hip_acqsearch.m")


def test_block_keywords_balance():
    code = strip(open(MFILE).read())
    opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
    ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
    assert opens == ends, (opens, ends)


def test_signature_is_the_call_it_replaces():
    name, outs, args = _signature(MFILE)
    assert name == "vbmc_hip_acqsearch"
    assert outs == ["xmin", "fmin", "counteval", "stopflag", "out", "bestever"]
    assert args == ["fitfun", "xstart", "insigma", "inopts", "vp", "gp", "optimState", "transpose_flag", "acqFun", "acqInfo"]
    src = open(MFILE).read()
    # everything the device search does not take goes to cmaes_modded with the same arguments and the same outputs
    assert re.search(r"\[xmin,fmin,counteval,stopflag,out,bestever\]\s*=\s*cmaes_modded\(fitfun,xstart,insigma,inopts,vp,gp,optimState,"
                     r"transpose_flag,acqFun,acqInfo\)", src)
    blk = _block(src, "    try")
    assert "catch err" in blk and "vbmc_hip:unsupported" in blk and "rethrow(err)" in blk
    for word in ("integervars", "vp.delta > 0", "LBounds", "UBounds", "LBeps_orig", "UBeps_orig"):
        assert word in src, word
    assert calls(src) == ["randi"]                     # the device stream's seed, nothing else


def test_gateway_command_and_argument_counts():
    src = open(MFILE).read()
    cmds, blk = _mex.gateway_commands(), _mex.gateway_block("acq_search")
    assert set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", src)) == {"acq_search"} and "acq_search" in cmds
    min_nrhs, handles, usage, _ = cmds["acq_search"]
    assert "vbmc_acq_search(g_ctx" in blk and handles == 1
    code = re.sub(r"\.\.\.\s*\n", "", src)
    counts = sorted(len(c.split(",")) for c in re.findall(r"vbmc_hip_mex\('acq_search',([^;]*)\);", code))
    assert counts == [11, 14], counts                  # h .. opts, and + gplengthscale, X_rescaled, sn2new for acqfsn2
    assert min_nrhs == 12                                # the command's name + the 11 arguments every call passes
    assert usage.startswith("h, acq_id") and len([t for t in usage.split("[")[0].split(",") if t.strip()]) == 11
    assert len([t for t in re.sub(r"[\[\]]", "", usage).split(",") if t.strip()]) == 14
    for f in ("TolX", "TolFun", "TolHistFun", "MaxFunEvals", "MaxIter", "PopSize", "Seed", "Chunk"):
        assert "'%s'" % f in src and 'scalar_field(op, "%s"' % f in blk, f
    for f in ("xbest", "fbest", "xmean", "sigma", "C", "evals", "generations", "stop", "behind"):
        assert "res.%s" % f in src and '"%s"' % f in blk, f


def test_integration_documents_the_replacement():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "vbmc_hip_acqsearch('acqwrapper_vbmc',x0(:),insigma,cmaes_opts,vp,gp,optimState,1,SearchAcqFcn{idxAcq},optimState.acqInfo{idxAcq})" in doc
    assert "private/activesample_vbmc.m" in doc
