"""CPU: static sanity of matlab/vbmc_hip_importance_sample.m in the style of tests/test_matlab_acqsearch_iqr_static.py (there is no
MATLAB here to run it): balanced block keywords, a function line named after the file, the one new gateway command implemented with the
argument count the shim passes, the fall-through on 'vbmc_hip:unsupported', the registration of the state handle with
vbmc_hip_is_handle, and no limit of the library restated in a .m file."""
import os
import re

from tests import _mex
from tests.test_matlab_static import _block, _signature, strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFILE = os.path.join(ROOT, "matlab", "vbmc_hip_importance_sample.m")
HANDLE = os.path.join(ROOT, "matlab", "vbmc_hip_is_handle.m")


def test_block_keywords_balance():
    code = strip(open(MFILE).read())
    opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
    ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
    assert opens == ends, (opens, ends)
    code = strip(open(HANDLE).read()).replace("(end)", "(last)")                   # (indexing, not a block)
    opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor|elseif)(?![\w])", code)) - len(re.findall(r"(?<![\w.])elseif(?![\w])", code))
    ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
    assert opens == ends, (opens, ends)


def test_signature_and_fall_through():
    name, outs, args = _signature(MFILE)
    assert name == "vbmc_hip_importance_sample" and outs == ["ais", "ok"]
    assert args == ["ais_step1", "gp", "acqfun", "options", "LB", "UB"]
    src = open(MFILE).read()
    blk = _block(src, "try")
    assert "catch err" in blk and "vbmc_hip:unsupported" in blk and "rethrow(err)" in blk and "return;" in blk
    for word in ("'acqimiqr_vbmc'", "importance_sampling_vp", "ActiveImportanceSamplingMCMCSamples", "ActiveImportanceSamplingMCMCThin",
                 "'islogf2'", "gplite_pred(gp,ais_step1.Xa,[],[],1,0)", "2*(D+1)", "vbmc_hip_gp_handle(gp)"):
        assert word in src, word
    assert "eissample_lite(" not in strip(src)
    for f in ("ais.Xa = Xa", "ais.lnw = lnw", "ais.fs2a = fs2a"):
        assert f in src, f


def test_state_handle_is_registered_where_the_search_looks_for_it():
    src = open(MFILE).read()
    assert "vbmc_hip_is_handle(h,ais,false,his)" in src
    name, outs, args = _signature(HANDLE)
    assert (name, outs, args) == ("vbmc_hip_is_handle", ["his"], ["h", "ais", "use_ctmp", "built"])
    hsrc = strip(open(HANDLE).read())
    assert "nargin > 3" in hsrc and "handle = built" in hsrc and open(HANDLE).read().count("vbmc_hip_mex('is_free',handle)") == 2
    search = open(os.path.join(ROOT, "matlab", "vbmc_hip_acqsearch_iqr.m")).read()
    assert "vbmc_hip_is_handle(h,optimState.ActiveImportanceSampling,id == 10)" in search     # same key, three arguments: a lookup


def test_gateway_command_and_argument_counts():
    src = open(MFILE).read()
    gateway = open(os.path.join(ROOT, "matlab", "vbmc_hip_mex.cpp")).read()
    cmds, blk = _mex.gateway_commands(), _mex.gateway_block("acq_is_sample")
    assert set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", src)) == {"acq_is_sample"} and "acq_is_sample" in cmds
    min_nrhs, handles, usage, _ = cmds["acq_is_sample"]
    assert "vbmc_acq_is_sample(g_ctx" in blk
    code = re.sub(r"\.\.\.\s*\n", "", src)
    counts = [len(c.split(",")) for c in re.findall(r"vbmc_hip_mex\('acq_is_sample',([^;]*)\);", code)]
    assert counts == [6], counts
    assert usage.startswith("h, x0") and len([t for t in usage.split(",") if t.strip()]) == 6
    assert min_nrhs == 7 and handles == 1                                                     # the command's name + 6 arguments
    reader = _mex.gateway_function("read_sampler_opts")                                       # the one reader of the sampler's options
    assert "read_sampler_opts(a, op)" in blk                                                  # the sampler's options: one reader for every command
    for f in ("Thin", "Burnin", "Spec", "Seed", "Chunk"):
        assert "'%s'" % f in src and 'scalar_field(op, "%s"' % f in blk + reader, f
    # the command is logic-free: limits and defaults are the library's
    for lim in ("256", "66", " 20", " 60"):
        assert lim not in blk, lim


def test_no_m_file_restates_a_limit():
    for path in (MFILE, HANDLE):
        code = strip(open(path).read())
        for lim in ("256", "1248", "66", "max_Na"):
            assert lim not in code, (path, lim)


def test_integration_documents_the_shim():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "vbmc_hip_importance_sample(" in doc and "acq_is_sample" in doc
