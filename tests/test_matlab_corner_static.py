"""CPU: static sanity of the shims matlab/vbmc_hip_cornerdata.m and matlab/vbmc_hip_plot.m, in the style of
tests/test_matlab_mtv_static.py (there is no MATLAB here to run them): balanced blocks, the gateway implements 'vp_corner' with the
argument count the shim passes, one randi per call of the data shim and none in the drawing one, the fall-through to the
reference's vbmc_plot, no numerics beyond the meshes, and no same-named vbmc_plot.m / cornerplot.m."""
import os
import re

from tests import _mex
from tests.test_matlab_static import _block, _signature, calls, strip
from tests.test_mex_gateway_compiles import _calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "matlab", "vbmc_hip_cornerdata.m")
PLOT = os.path.join(ROOT, "matlab", "vbmc_hip_plot.m")
NUMERIC = ("exp(", "log(", "cos(", "fft(", "ifft(", "histc(", "histogram(", "histcounts(", "accumarray(", "kde2d(", "kde1d(", "median(",
           "quantile", "prctile(", "sort(", "sum(", "cumsum(", "mean(", "max(", "min(", "fzero(", "fminbnd(", "vbmc_rnd(", "interp1(", "dct")


def test_block_keywords_balance():
    for f in (DATA, PLOT):
        code = strip(open(f).read())
        opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
        ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
        assert opens == ends, (f, opens, ends)


def test_gateway_command_and_argument_count():
    cmds, blk = _mex.gateway_commands(), _mex.gateway_block("vp_corner")
    src = open(DATA).read()
    assert set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", src)) == {"vp_corner"}
    assert "vp_corner" in cmds and "vbmc_vp_corner(g_ctx" in blk
    min_nrhs, handles, usage, _ = cmds["vp_corner"]
    names = [t.strip() for t in usage.split(",")]
    assert names == ["vp", "X", "Ns", "seed", "balanceflag", "bounds", "res", "nbins", "p"]
    assert min_nrhs == 1 + len(names) == 10 and handles == 0                                     # the command's name + 9 arguments
    got = _calls(src, "vp_corner")
    assert got == [("vp_corner", 9), ("vp_corner", 9)], got                                       # a posterior; a sample matrix
    assert "vbmc_hip_mex('vp_corner',src,[],Ns,seed,balanceflag,bounds,0,0,0.5)" in src           # vp, no matrix; the library's own res and nbins
    assert "vbmc_hip_mex('vp_corner',[],src,0,seed,0,bounds,0,0,0.5)" in src                      # no vp, the matrix
    assert "vbmc_hip_mex" not in open(PLOT).read()                                                # the drawing shim goes through the data shim
    for word in ("4096", "1e5", "exp(", "log(", "cos(", "sqrt("):                                # logic-free: no numerics of the estimator in the handler
        assert word not in blk, word


def test_one_randi_per_call():
    src = open(DATA).read()
    assert calls(src) == ["randi"] and "seed = randi(2^31-1);" in src
    assert src.index("seed = randi(2^31-1);") < src.index("try")                                  # outside both branches: exactly one per call
    assert calls(open(PLOT).read()) == []


def test_fall_through_edges():
    src = open(DATA).read()
    blk = _block(src, "try")
    assert "catch err" in blk and "vbmc_hip:unsupported" in blk and "rethrow(err)" in blk and "'ok',false" in blk
    name, outs, args = _signature(DATA)
    assert name == "vbmc_hip_cornerdata" and outs == ["S", "ok"] and args[:4] == ["src", "names", "truths", "bounds"]
    plot = strip(open(PLOT).read())
    assert open(PLOT).read().startswith("function vbmc_hip_plot(vp_array,stats)\n")               # vbmc_plot's own arguments, no output
    assert len(re.findall(r"(?<![\w_])vbmc_plot\(vp_array,stats\); return;", plot)) == 2          # not a posterior; ~ok
    assert "~isstruct(vp_array{i})" in plot and "if ~ok" in plot
    assert "contour(X,Y,S.density(:,:,pp),10)" in plot and "stairs(" in plot
    assert "for i = 1:Nvps" in plot and "S{i}.median(d)" in plot                                  # a cell array: histograms and medians
    for f in ("vbmc_plot.m", "cornerplot.m", "kde2d.m"):
        assert not os.path.exists(os.path.join(ROOT, "matlab", f)), f


def test_no_numerics():
    for f in (DATA, PLOT):
        code = strip(open(f).read())
        for word in NUMERIC:                                                                      # a call, not a field of the struct
            assert not re.search(r"(?<![\w.])" + re.escape(word), code), (os.path.basename(f), word)
    assert "linspace(" not in strip(open(DATA).read())                                            # the meshes are the drawing shim's
    assert len(re.findall(r"linspace\(", strip(open(PLOT).read()))) == 3


def test_documents_name_the_command_and_the_shims():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`vp_corner`" in doc and "vbmc_hip_cornerdata" in doc and "vbmc_hip_plot" in doc and "vbmc_vp_corner" in doc
