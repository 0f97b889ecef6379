"""CPU: static sanity of matlab/vbmc_hip_importance_setup.m and of the one-call form of matlab/vbmc_hip_importance_sample.m, in the
style of tests/test_matlab_issample_static.py (there is no MATLAB here to run them): balanced block keywords, a function line named
after the file, the one new gateway command implemented with the argument count the shim passes, the fall-through on
'vbmc_hip:unsupported', the registration of the state handle with vbmc_hip_is_handle, and no limit of the library restated in a .m
file."""
import os
import re

from tests import _mex
from tests.test_matlab_static import _block, _signature, strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFILE = os.path.join(ROOT, "matlab", "vbmc_hip_importance_setup.m")
STEP2 = os.path.join(ROOT, "matlab", "vbmc_hip_importance_sample.m")


def test_block_keywords_balance():
    for path in (MFILE, STEP2):
        code = strip(open(path).read())
        opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
        ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
        assert opens == ends, (path, opens, ends)


def test_signature_and_fall_through():
    name, outs, args = _signature(MFILE)
    assert name == "vbmc_hip_importance_setup" and outs == ["ais", "ok"]
    assert args == ["vp", "gp", "acqfun", "options"]
    src = open(MFILE).read()
    blk = _block(src, "try")
    assert "catch err" in blk and "vbmc_hip:unsupported" in blk and "rethrow(err)" in blk and "return;" in blk
    for word in ("'acqimiqr_vbmc'", "importance_sampling_vp", "vp.delta", "ActiveImportanceSamplingMCMCSamples", "ActiveImportanceSamplingMCMCThin",
                 "ActiveImportanceSamplingVPSamples", "ActiveImportanceSamplingBoxSamples", "vbmc_hip_gp_handle(gp)", "vbmc_hip_supported(gp,vp,true)",
                 "out.n_bad > 0", "numel(gp.post)"):
        assert word in src, word
    code = strip(src)
    for host_work in ("gplite_pred(", "vbmc_rnd(", "eissample_lite(", "cumsum(", "rand("):      # nothing of Step 1 is left to MATLAB
        assert host_work not in code, host_work
    for f in ("ais.Xa = Xa", "ais.lnw = lnw", "ais.fs2a = fs2a", "ais.Xa = out.Xa1", "ais.lnw = out.lnw1", "ais.fs2a = out.fs2a1"):
        assert f in src, f
    assert "vbmc_hip_is_handle(h,ais,false,his)" in src
    # a bad start goes to the two-call shim with the Step 1 arrays and the library's box
    assert "vbmc_hip_importance_sample(ais,gp,acqfun,options,out.LB,out.UB)" in src


def test_the_step_two_shim_takes_the_one_call_form_when_given_vp():
    src = open(STEP2).read()
    code = strip(src)
    assert "isfield(ais_step1,'mu') && ~isfield(ais_step1,'Xa')" in src
    assert "[ais,ok] = vbmc_hip_importance_setup(ais_step1,gp,acqfun,options);" in code
    first = code.index("vbmc_hip_importance_setup(")
    assert first < code.index("options.ActiveImportanceSamplingMCMCSamples")                    # decided before anything of Step 2 is read
    assert "vbmc_hip_importance_sample(vp,gp,acqfun,options)" in src                            # documented in the help text


def test_gateway_command_and_argument_counts():
    src = open(MFILE).read()
    gateway = open(os.path.join(ROOT, "matlab", "vbmc_hip_mex.cpp")).read()
    cmds, blk = _mex.gateway_commands(), _mex.gateway_block("is_setup")
    assert set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", src)) == {"is_setup"} and "is_setup" in cmds
    min_nrhs, handles, usage, _ = cmds["is_setup"]
    assert "vbmc_acq_is_setup(g_ctx" in blk
    code = re.sub(r"\.\.\.\s*\n", "", src)
    counts = [len(c.split(",")) for c in re.findall(r"vbmc_hip_mex\('is_setup',([^;]*)\);", code)]
    assert counts == [6], counts
    assert usage.startswith("h, vp") and len([t for t in usage.split(",") if t.strip()]) == 6
    assert min_nrhs == 7 and handles == 1                                                       # the command's name + 6 arguments
    reader = _mex.gateway_function("read_sampler_opts")                                       # the one reader of the sampler's options
    assert "read_sampler_opts(a, op)" in blk and 'scalar_field(op, "S"' in blk
    for f in ("Thin", "Burnin", "Spec", "Seed", "Chunk", "S"):
        assert "'%s'" % f in src and 'scalar_field(op, "%s"' % f in blk + reader, f
    # the command is logic-free: limits and defaults of the sampler are the library's
    for lim in ("256", "512", " 66", " 20", " 60", "0.05", "0.6745"):
        assert lim not in blk, lim
    for name in ("Xa1", "lnw1", "fs2a1", "lpdf1", "rect_delta", "x0", "idx0", "n_bad", "bad"):
        assert '"%s"' % name in blk, name


def test_no_m_file_restates_a_limit():
    for path in (MFILE, STEP2):
        code = strip(open(path).read())
        for lim in ("256", "512", "1248", "66", "max_Na"):
            assert lim not in code, (path, lim)


def test_documents_name_the_command_and_the_shim():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "vbmc_hip_importance_setup(" in doc and "`is_setup`" in doc and "vbmc_acq_is_setup" in doc
    sup = open(os.path.join(ROOT, "matlab", "vbmc_hip_supported.m")).read()
    assert "vbmc_hip_importance_setup" in sup
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_is_draw" in design and "k_is_proposal" in design and "k_is_resample" in design
    assert "Step 1 stays on the host" not in design
