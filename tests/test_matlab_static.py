"""CPU: static sanity of the MATLAB side (there is no MATLAB / Octave here to run it): every .m file under matlab/ and tools/ has
balanced block keywords, a leading function line whose name matches the file, and calls into the MEX gateway only with commands
the gateway implements.  What the checks need to know of the reference's MATLAB files (the function lines of the files the shims
replace, hashes of the code lines of the two callers the shims wrap, the random draws of three files) is stored in
tests/golden/reference_matlab.json; `python tests/test_matlab_static.py <reference root>` regenerates it."""
import glob
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFILES = sorted(glob.glob(os.path.join(ROOT, "matlab", "*.m")) + glob.glob(os.path.join(ROOT, "tools", "*.m")))
REF_FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_matlab.json")
REF_SIEVE_CALLERS = ("misc/vpsieve_vbmc.m", "misc/vpoptimize_vbmc.m")
REF_DRAWS = ("ent/entmc_vbmc.m", "misc/vpoptimize_vbmc.m", "misc/negelcbo_vbmc.m")


def _reference():
    with open(REF_FIXTURE) as f:
        return json.load(f)


def _line_hash(line):
    return hashlib.sha256(line.encode()).hexdigest()[:16]


def strip(txt):
    out = []
    for ln in txt.split("\n"):
        ln = re.sub(r"'[^']*'", "''", ln)
        ln = re.sub(r'"[^"]*"', '""', ln)
        out.append(ln.split("%")[0])
    return "\n".join(out)


def test_block_keywords_balance():
    assert MFILES
    for f in MFILES:
        code = strip(open(f).read())
        opens = len(re.findall(r"(?<![\w.])(function|if|for|while|switch|try|parfor)(?![\w])", code))
        ends = len(re.findall(r"(?<![\w.])end(?![\w(])", code))
        index_like = len(re.findall(r"[\(\[,:]\s*end\b|end\s*[\)\],:+\-]", code))      # x(end), x(end-1), a:end
        assert opens == ends or opens == ends - index_like, (os.path.basename(f), opens, ends, index_like)


def test_function_name_matches_file():
    for f in MFILES:
        first = next(ln for ln in open(f).read().split("\n") if ln.strip() and not ln.strip().startswith("%"))
        m = re.match(r"\s*function\s+(?:\[[^\]]*\]\s*=\s*|\w+\s*=\s*)?(\w+)", first)
        assert m and m.group(1) == os.path.splitext(os.path.basename(f))[0], (os.path.basename(f), first)


def test_mex_commands_exist_in_the_gateway():
    from tests import _mex

    implemented = set(_mex.gateway_commands())                     # the rows of the gateway's command table
    assert implemented, "no commands recognised in the gateway source"
    used = set()
    for f in MFILES:
        used |= set(re.findall(r"vbmc_hip_mex\(\s*'(\w+)'", open(f).read()))
    assert used and used <= implemented, sorted(used - implemented)


def calls(txt):
    """the random-stream draws a MATLAB text makes, in order"""
    return re.findall(r"\b(randn|randi|rand|randperm)\s*\(", strip(txt))


def _signature(path):
    txt = open(path, errors="replace").read()
    m = re.search(r"^\s*function\s+(?:\[([^\]]*)\]|(\w+))?\s*=?\s*(\w+)\s*\(([^)]*)\)", txt, re.M)
    assert m, path
    outs = [t.strip() for t in re.split(r"[,\s]+", (m.group(1) or m.group(2) or "").strip()) if t.strip()]
    args = [t.strip() for t in m.group(4).split(",") if t.strip()]
    return m.group(3), outs, args


def test_shim_signatures_match_the_reference():
    """Drop-in by path lookup only works if a same-named shim takes and returns what the reference function does: compare the
    function lines (names and ORDER of inputs and outputs) with the reference's files (their function lines as recorded in
    tests/golden/reference_matlab.json)."""
    index = _reference()["signatures"]
    checked = 0
    for f in sorted(glob.glob(os.path.join(ROOT, "matlab", "*.m"))):
        base = os.path.basename(f)
        if base.startswith("vbmc_hip_") or base not in index:
            continue                      # helpers of the shim layer itself
        # gplite/private/sq_dist.m and utils/sq_dist.m are the same function; any one of the candidates must match
        name, outs, args = _signature(f)
        cands = index[base]
        assert any(name == n and len(outs) == len(o) and [a.lower() for a in args] == [b.lower() for b in a_]
                   for n, o, a_ in cands), (base, outs, args, cands)
        checked += 1
    assert checked >= 8


def _code_lines(path):
    """Whitespace-stripped code lines (comments and blank lines dropped)."""
    out = []
    for ln in open(path, errors="replace").read().split("\n"):
        o, q = "", False
        for ch in ln:
            if ch == "'":
                q = not q
            if ch == "%" and not q:
                break
            o += ch
        t = re.sub(r"\s+", "", o)
        if t:
            out.append(t)
    return out


def test_caller_shims_do_not_restate_the_reference():
    """matlab/vpsieve_vbmc.m (record and replay around the reference's own sieve) and matlab/vpoptimize_vbmc.m (+ its pruning
    helper) must not carry the reference's text: fewer than 15 % of their code lines, whitespace-stripped, occur in the
    same-named reference file -- block keywords (end / else / try) included in the count; the function line is left out (it is
    the interface: test_shim_signatures_match_the_reference REQUIRES it to be the reference's).  The reference's lines are known by
    their hashes (tests/golden/reference_matlab.json)."""
    hashes = _reference()["code_line_sha256_16"]
    for mine, ref in (("vpsieve_vbmc.m", "misc/vpsieve_vbmc.m"), ("vpoptimize_vbmc.m", "misc/vpoptimize_vbmc.m"),
                      ("vbmc_hip_prune.m", "misc/vpoptimize_vbmc.m"), ("vbmc_hip_sieve.m", "misc/vpsieve_vbmc.m")):
        a = [ln for ln in _code_lines(os.path.join(ROOT, "matlab", mine)) if not ln.startswith("function[")]
        b = set(hashes[ref])
        same = [ln for ln in a if _line_hash(ln) in b]
        assert len(same) < 0.15 * len(a), (mine, len(same), len(a), [ln for ln in same if ln not in ("end", "else", "try")])


def _block(src, head):
    """Text of the block that starts at the line containing `head`, up to its matching `end` (one-line ifs skipped)."""
    lines = src.split("\n")
    i0 = next(i for i, ln in enumerate(lines) if head in ln)
    depth, out = 0, []
    for ln in lines[i0:]:
        code = strip(ln)
        opens = len(re.findall(r"(?<![\w.])(if|for|while|switch|try|function)(?![\w])", code))
        ends = len(re.findall(r"(?<![\w.(:,])end(?![\w(])", code))
        depth += opens - ends
        out.append(ln)
        if depth <= 0:
            break
    return "\n".join(out)


def test_random_draws_per_branch_match_the_reference():
    """Parity mode (VBMC_HIP_PARITY=1) only reproduces a reference run if every shim consumes MATLAB's global stream exactly
    as the reference does: K blocks randn(D,1,Ns/2) per Monte-Carlo entropy evaluation (ent/entmc_vbmc.m:53), NOTHING when
    Ns == 0 (entlb_vbmc), one randi per pruning attempt (misc/vpoptimize_vbmc.m:204), nothing else.  The seed of the device
    stream (a randi) may only be drawn where the device stream is used.  Static: no MATLAB here to run the shims."""
    rd = lambda f: open(os.path.join(ROOT, "matlab", f)).read()  # noqa: E731
    # negelcbo_vbmc: every draw sits inside `if Ns > 0`; there, randn in the parity branch and the seed in the other
    src = rd("negelcbo_vbmc.m")
    blk = _block(src, "if Ns > 0")
    assert sorted(calls(src)) == sorted(calls(blk)) == ["randi", "randn"]
    par, other = blk.split("else", 1)
    assert "vbmc_hip_state('parity')" in par and calls(par) == ["randn"] and calls(other) == ["randi"]
    assert "randn(vp.D,1,Nse/2)" in par and "for j = 1:vp.K" in par       # K blocks, the reference's call
    # entmc_vbmc: same split
    src = rd("entmc_vbmc.m")
    blk = _block(src, "if vbmc_hip_state('parity')")
    par, other = blk.split("else", 1)
    assert sorted(calls(src)) == ["randi", "randn"] and calls(par) == ["randn"] and calls(other) == ["randi"]
    # entlb_vbmc, gplogjoint: deterministic
    assert calls(rd("entlb_vbmc.m")) == [] and calls(rd("gplogjoint.m")) == []
    # pruning: one randi(numel(.)) per attempt, inside the loop
    src = rd("vbmc_hip_prune.m")
    assert calls(src) == ["randi"] and "randi(numel(open))" in _block(src, "while true")
    # the sieve shim draws nothing itself; its batched helper seeds a device stream only for a Monte-Carlo entropy
    assert calls(rd("vpsieve_vbmc.m")) == []
    src = rd("vbmc_hip_sieve.m")
    assert calls(src) == ["randi"] and "if c1.Ns > 0; seed = randi" in src
    # vpoptimize_vbmc: parity mode leaves before any draw (inside_path is false), its own draws are device seeds only
    src = rd("vpoptimize_vbmc.m")
    head = src[: src.index("if isempty(K); K = vp.K; end")]
    assert calls(head) == [] and "inside_path" in head
    assert "vbmc_hip_state('parity')" in _block(src, "function ok = inside_path")
    assert set(calls(src)) == {"randi"} and "randi(2^31-1)" in src and len(calls(src)) == 2
    # the reference's own counts (as recorded in tests/golden/reference_matlab.json), so that drift upstream is noticed
    ref = _reference()["random_draws"]
    assert len(ref["ent/entmc_vbmc.m"]) == 1
    assert ref["misc/vpoptimize_vbmc.m"] == ["randi"] and _reference()["vpoptimize_draws_idx_randi_numel_idx"]
    assert ref["misc/negelcbo_vbmc.m"] == []


def test_gplite_post_keeps_the_device_posterior_and_gplogjoint_falls_through():
    """matlab/gplite_post.m asks 'gp_post' for its sixth output (the device handle) and registers it for the gp it returns -- the
    next evaluation uploads nothing (tests/test_gpu_mex.py runs that sequence through the gateway); matlab/gplogjoint.m catches
    vbmc_hip:unsupported like negelcbo_vbmc.m does and hands the call to the reference."""
    post = open(os.path.join(ROOT, "matlab", "gplite_post.m")).read()
    m = re.search(r"\[([^\]]*)\]\s*=\s*vbmc_hip_mex\('gp_post'", post)
    assert m and len([t for t in m.group(1).split(",") if t.strip()]) == 6
    hname = m.group(1).split(",")[-1].strip()
    assert re.search(r"vbmc_hip_gp_handle\(gp,\s*%s\)" % re.escape(hname), post)
    lj = strip(open(os.path.join(ROOT, "matlab", "gplogjoint.m")).read())
    assert "try" in lj and "catch err" in lj and "vbmc_hip_supported(gp,vp" in lj
    assert re.search(r"strcmp\(err\.identifier,\s*''\)", lj) and "vbmc_hip_reference(''" in lj


def write_reference_fixture(ref_root):
    """tests/golden/reference_matlab.json from a checkout of the reference: no source text, only what the checks above compare."""
    index = {}
    for dp, _, fn in os.walk(ref_root):
        for f in sorted(fn):
            if f.endswith(".m"):
                index.setdefault(f, []).append(os.path.join(dp, f))
    shims = sorted(os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "matlab", "*.m")))
    rd = lambda rel: open(os.path.join(ref_root, rel), errors="replace").read()  # noqa: E731
    fixture = {
        "signatures": {b: [list(_signature(p)) for p in sorted(index[b])] for b in shims if not b.startswith("vbmc_hip_") and b in index},
        "code_line_sha256_16": {rel: sorted({_line_hash(ln) for ln in _code_lines(os.path.join(ref_root, rel))}) for rel in REF_SIEVE_CALLERS},
        "random_draws": {rel: calls(rd(rel)) for rel in REF_DRAWS},
        "vpoptimize_draws_idx_randi_numel_idx": "idx(randi(numel(idx)))" in rd("misc/vpoptimize_vbmc.m"),
    }
    with open(REF_FIXTURE, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    write_reference_fixture(sys.argv[1])
