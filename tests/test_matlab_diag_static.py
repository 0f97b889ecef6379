"""CPU: static sanity of the shim matlab/vbmc_hip_diagnostics.m, in the style of tests/test_matlab_mtv_static.py (there is no MATLAB here
to run it): it calls only the gateway's 'vp_diag' command, with the arguments the gateway counts and names; its inputs are the
reference function's in the reference's order followed by one options struct, its outputs the reference's; it falls through to
vbmc_diagnostics on 'vbmc_hip:unsupported'; it takes its seed from one randi; every default tests nargin against the argument's own
position (the reference's are one too high); it contains no arithmetic of the estimators; no same-named vbmc_diagnostics.m exists;
and the gateway's handler is logic-free."""
import os
import re

from tests import _mex
from tests.test_matlab_static import _block, _signature, strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "matlab", "vbmc_hip_diagnostics.m")
REF_OUTS = ["exitflag", "best", "idx_best", "stats"]                                             # vbmc_diagnostics.m:1
REF_ARGS = ["vp_array", "beta_lcb", "elbo_thresh", "sKL_thresh", "maxmtv_thresh"]


def test_block_keywords_balance():
    code = strip(open(SHIM).read())
    opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
    ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
    assert opens == ends, (opens, ends)


def test_signature_is_the_reference_plus_options():
    got, outs, args = _signature(SHIM)
    assert got == "vbmc_hip_diagnostics" and outs == REF_OUTS and args == REF_ARGS + ["opts"], (outs, args)
    assert not os.path.exists(os.path.join(ROOT, "matlab", "vbmc_diagnostics.m")), "the draws are the library's: no same-named shim"


def test_gateway_command_and_argument_count():
    cmds, blk = _mex.gateway_commands(), _mex.gateway_block("vp_diag")
    src = open(SHIM).read()
    assert set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", src)) == {"vp_diag"}
    assert "vp_diag" in cmds and "vbmc_vp_diagnostics(g_ctx" in blk
    min_nrhs, handles, usage, _ = cmds["vp_diag"]
    calls = re.findall(r"vbmc_hip_mex\('vp_diag',([^;]*)\);", src)
    assert calls == ["Ns,seed,vp_array{:}"], calls                                                # Ns, seed, then one argument per run
    assert min_nrhs == 4 and handles == 0                                                         # the command, Ns, seed and at least one run
    assert [t.strip() for t in re.sub(r"[\[\]]", "", usage).split(",")] == ["Ns", "seed", "vp1", "vp2", "..."]
    assert [t.strip() for t in usage.split("[")[0].split(",")] == ["Ns", "seed", "vp1"]          # the further runs are optional
    for word in ("8192", "100000", "1e5", "exp(", "log(", "cos(", "fmax(", "std::max", "isnan"):   # logic-free: no default, no reduction
        assert word not in blk, word
    assert "R = nrhs - 3" in blk and blk.count("fill_vp_desc(") == 1
    assert "the runs vp1, vp2, ..." in blk.split("\n")[0]


def test_fall_through_and_defaults():
    src = open(SHIM).read()
    code = strip(src)
    blk = _block(src, "try")
    assert "catch err" in blk and "vbmc_hip:unsupported" in blk and "rethrow(err)" in blk
    assert len(re.findall(r"(?<![\w_])vbmc_diagnostics\(vp_array,beta_lcb,elbo_thresh,sKL_thresh,maxmtv_thresh\)", code)) == 2
    assert src.count("randi(2^31-1)") == 1
    for pos, name in enumerate(REF_ARGS[1:] + ["opts"], start=2):                                 # a given argument is used
        assert re.search(r"if nargin < %d \|\| isempty\(%s\)" % (pos, name), code), name
    for name, default in (("beta_lcb", "3"), ("elbo_thresh", "1"), ("sKL_thresh", "1"), ("maxmtv_thresh", "0.2")):
        assert re.search(r"isempty\(%s\); %s = %s; end" % (name, name, re.escape(default)), code), name
    assert "Ns = 1e5" in code                                                                      # vbmc_kldiv.m / vbmc_mtv.m defaults
    assert "max(Nruns/3,2)" in code and code.count("< need") == 3
    assert "min(exitflag,-2)" in code and code.count("min(exitflag,-1)") == 2
    assert "nargin" in src.split("if nargin")[0] and "NaN" in src.split("if nargin")[0]           # both quirks are in the help text


def test_no_estimator_arithmetic():
    code = strip(open(SHIM).read())
    for word in ("exp(", "log(", "sqrt(", "cos(", "fft(", "histc(", "interp1(", "kde1d(", "qtrapz(", "linspace(", "vbmc_rnd(", "vbmc_kldiv(",
                 "vbmc_mtv(", "vbmc_pdf("):
        assert word not in code, word


def test_documents_name_the_command_and_the_shim():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`vp_diag`" in doc and "vbmc_hip_diagnostics" in doc and "vbmc_vp_diagnostics" in doc
