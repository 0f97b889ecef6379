"""CPU: static sanity of the four shims of the variational-posterior tools, matlab/vbmc_hip_pdf.m, vbmc_hip_rnd.m, vbmc_hip_moments.m and
vbmc_hip_kldiv.m, in the style of tests/test_matlab_issetup_static.py (there is no MATLAB here to run them): the gateway implements
their commands with the argument counts the shims pass, their inputs and outputs are the reference functions' in the reference's
order (recorded as lists of names in tests/golden/reference_vptools_signatures.json), they fall through to the reference function on
'vbmc_hip:unsupported', take their seed from one randi, and contain no density or transform arithmetic."""
import json
import os
import re

from tests import _mex
from tests.test_matlab_static import _block, _signature, strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = {"vbmc_hip_pdf": ("vbmc_pdf", "vp_pdf", 6), "vbmc_hip_rnd": ("vbmc_rnd", "vp_rnd", 6), "vbmc_hip_moments": ("vbmc_moments", "vp_moments", 3),
         "vbmc_hip_kldiv": ("vbmc_kldiv", "vp_kldiv", 4)}


def path(name):
    return os.path.join(ROOT, "matlab", name + ".m")


def test_block_keywords_balance():
    for name in SHIMS:
        code = strip(open(path(name)).read())
        opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
        ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
        assert opens == ends, (name, opens, ends)


def test_signatures_equal_the_reference():
    with open(os.path.join(ROOT, "tests", "golden", "reference_vptools_signatures.json")) as f:
        index = json.load(f)["signatures"]
    for name, (ref, _, _) in SHIMS.items():
        got, outs, args = _signature(path(name))
        (rname, routs, rargs), = index[ref + ".m"]
        assert got == name and rname == ref
        assert outs == routs and args == rargs, (name, outs, args, routs, rargs)
        assert not os.path.exists(path(ref)), "a same-named shim would intercept the one-point draws inside activesample_vbmc"


def test_gateway_commands_and_argument_counts():
    cmds = _mex.gateway_commands()
    for name, (ref, cmd, nargs) in SHIMS.items():
        src = re.sub(r"\.\.\.\s*\n", "", open(path(name)).read())
        assert set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", src)) == {cmd}, name
        assert cmd in cmds and "vbmc_%s(g_ctx" % cmd in _mex.gateway_block(cmd)
        min_nrhs, handles, usage, _ = cmds[cmd]
        counts = {len(c.split(",")) for c in re.findall(r"vbmc_hip_mex\('%s',([^;]*)\);" % cmd, strip(src).replace("''", "'%s'" % cmd))}
        assert counts == {nargs}, (name, counts)
        assert min_nrhs == nargs + 1 and handles == 0, cmd                                              # the command's name + its arguments
        assert "[" not in usage and len([t for t in usage.split(",") if t.strip()]) == nargs, (cmd, usage)
    # the commands are logic-free: no limit, default or constant of the library is restated
    blk = "\n".join(_mex.gateway_block(cmd) for _, cmd, _ in SHIMS.values())
    for word in ("512", " 32", "exp(", "log(", "1e5", "1e6"):
        assert word not in blk, word


def test_fall_through_and_seed():
    for name, (ref, cmd, _) in SHIMS.items():
        src = open(path(name)).read()
        blk = _block(src, "try")
        assert "catch err" in blk and "vbmc_hip:unsupported" in blk and "rethrow(err)" in blk, name
        assert re.search(r"(?<![\w_])%s\(" % ref, strip(src)), name                                     # the reference function is the fall-through
        if name != "vbmc_hip_pdf":
            assert "randi(2^31-1)" in src, name                                                          # as vbmc_hip_importance_setup.m takes its seed
    assert "ischar(balanceflag)" in open(path("vbmc_hip_rnd")).read()                                    # 'gp'
    kl = open(path("vbmc_hip_kldiv")).read()
    assert "gaussflag || ~isstruct(vp1) || ~isstruct(vp2)" in kl                                        # vp given as a sample matrix
    assert "~origflag" in open(path("vbmc_hip_moments")).read()


def test_no_density_or_transform_arithmetic():
    for name in SHIMS:
        code = strip(open(path(name)).read())
        for word in ("exp(", "log(", "log1p(", "sqrt(", "bsxfun(", "cumsum(", "randn(", "rand(", "warpvars_vbmc(", "sum(", "cov(", "mean(", "gammaln("):
            assert word not in code, (name, word)
        for lim in ("512", "32"):
            assert not re.search(r"(?<![\w^\-])%s(?!\w)" % lim, code), (name, lim)


def test_documents_name_the_commands_and_the_shims():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, (ref, cmd, _) in SHIMS.items():
        assert "`%s`" % cmd in doc and name in doc and "vbmc_%s" % cmd in doc, name
