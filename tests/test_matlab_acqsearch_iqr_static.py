"""CPU: static sanity of matlab/vbmc_hip_acqsearch_iqr.m in the style of tests/test_matlab_acqsearch_static.py (there is no MATLAB here
to run it): balanced block keywords, a function line named after the file with vbmc_hip_acqsearch's arguments and outputs, the one new
gateway command implemented with the argument count the shim passes (both handles checked), the fall-through to vbmc_hip_acqsearch
with the same arguments, and the documented replacement line for noisy targets."""
import os
import re

from tests import _mex
from tests.test_matlab_static import _block, _signature, strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFILE = os.path.join(ROOT, "matlab", "vbmc_hip_acqsearch_iqr.m")


def test_block_keywords_balance():
    code = strip(open(MFILE).read())
    opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
    ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
    assert opens == ends, (opens, ends)


def test_signature_and_fall_through():
    name, outs, args = _signature(MFILE)
    assert name == "vbmc_hip_acqsearch_iqr"
    assert (name, outs, args) == ("vbmc_hip_acqsearch_iqr",) + _signature(os.path.join(ROOT, "matlab", "vbmc_hip_acqsearch.m"))[1:]
    src = open(MFILE).read()
    assert re.search(r"\[xmin,fmin,counteval,stopflag,out,bestever\]\s*=\s*vbmc_hip_acqsearch\(fitfun,xstart,insigma,inopts,vp,gp,optimState,"
                     r"transpose_flag,acqFun,acqInfo\)", src)
    assert "cmaes_modded(" not in strip(src)           # the reference's optimiser is reached through vbmc_hip_acqsearch only
    blk = _block(src, "    try")
    assert "catch err" in blk and "vbmc_hip:unsupported" in blk and "rethrow(err)" in blk
    for word in ("integervars", "vp.delta > 0", "LBounds", "UBounds", "LBeps_orig", "UBeps_orig", "ActiveImportanceSampling",
                 "'acqviqr_vbmc'", "'acqimiqr_vbmc'", "vbmc_hip_is_handle(h,optimState.ActiveImportanceSampling"):
        assert word in src, word


def test_gateway_command_and_argument_counts():
    src = open(MFILE).read()
    cmds, blk = _mex.gateway_commands(), _mex.gateway_block("acq_search_iqr")
    assert set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", src)) == {"acq_search_iqr"} and "acq_search_iqr" in cmds
    min_nrhs, handles, usage, _ = cmds["acq_search_iqr"]
    assert "vbmc_acq_search_iqr(g_ctx" in blk
    code = re.sub(r"\.\.\.\s*\n", "", src)
    counts = [len(c.split(",")) for c in re.findall(r"vbmc_hip_mex\('acq_search_iqr',([^;]*)\);", code)]
    assert counts == [14], counts
    assert usage.startswith("h, his, acq_id") and "[" not in usage and len([t for t in usage.split(",") if t.strip()]) == 14
    assert min_nrhs == 15                                                        # the command's name + 14 arguments
    assert handles == 2                                                          # h and his are both checked before the handler runs
    assert "handle_in<vbmc_gp>(prhs[1])" in blk and "handle_in<vbmc_acq_is>(prhs[2])" in blk
    for f in ("TolX", "TolFun", "TolHistFun", "MaxFunEvals", "MaxIter", "PopSize", "Seed", "Chunk"):
        assert "'%s'" % f in src, f
    for f in ("xbest", "fbest", "xmean", "sigma", "C", "evals", "generations", "stop", "behind"):
        assert "res.%s" % f in src, f


def test_integration_documents_the_noisy_target_replacement():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "vbmc_hip_acqsearch_iqr('acqwrapper_vbmc',x0(:),insigma,cmaes_opts,vp,gp,optimState,1,SearchAcqFcn{idxAcq},optimState.acqInfo{idxAcq})" in doc
    assert "vbmc_hip_acqsearch('acqwrapper_vbmc',x0(:),insigma,cmaes_opts,vp,gp,optimState,1,SearchAcqFcn{idxAcq},optimState.acqInfo{idxAcq})" in doc
    assert "acq_search_iqr" in doc
