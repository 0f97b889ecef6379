"""CPU: matlab/vbmc_hip_mex.cpp type-checks against include/vbmc_hip.h (with a mock mex.h: MATLAB is absent here) and every
vbmc_* symbol it references is exported by libvbmc_hip.so -- catches drift between the C ABI and the MEX gateway.  Also the
gateway's command table (tests/_mex.py reads it out of the source): every command once, argument counts that agree with the
usage strings, with what the .m shims pass and with what mexFunction, executed through the mock, refuses."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _mex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEX = os.path.join(ROOT, "matlab", "vbmc_hip_mex.cpp")


def test_gateway_compiles_against_the_abi(tmp_path):
    import __graft_entry__ as g

    g.build()
    obj = str(tmp_path / "vbmc_hip_mex.o")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror=return-type", "-fPIC", "-c", MEX,
                        "-I", os.path.join(ROOT, "tests", "mock_mex"), "-I", os.path.join(ROOT, "include"), "-o", obj],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the documented build line passes no -std flag: the gateway must not need more than the C++11 a mex options file may set
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", MEX, "-I", os.path.join(ROOT, "tests", "mock_mex"),
                        "-I", os.path.join(ROOT, "include")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    und = subprocess.run(["nm", "-u", obj], capture_output=True, text=True).stdout
    wanted = sorted(set(re.findall(r"\b(vbmc_[a-z0-9_]+)\b", und)))
    assert len(wanted) >= 15, wanted
    from vbmc_amd import _lib

    exp = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(vbmc_[a-z0-9_]+)\b", exp))
    assert not [w for w in wanted if w not in exported]


def test_no_long_jump_with_live_cpp_objects():
    """mexErrMsgIdAndTxt long-jumps without running destructors: it may only be called from mexFunction itself."""
    src = open(MEX).read()
    code = src[src.index("#include"):src.index("void mexFunction(")]        # every helper, every handler, the table, dispatch()
    assert "mexErrMsg" not in code
    assert src.count("mexErrMsgIdAndTxt(") == 1 + src[: src.index("#include")].count("mexErrMsgIdAndTxt(")


def test_every_command_occurs_once_in_the_table():
    rows = _mex.gateway_rows()
    names = [r[0] for r in rows]
    assert len(names) >= 37 and len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    src = open(MEX).read()
    for name, _, handles, _, handler in rows:
        assert handles in (0, 1, 2), name
        assert len(re.findall(r"^static int %s\(int" % handler, src, re.M)) == 1, handler       # one handler per command
    assert len({r[4] for r in rows}) == len(rows)
    body = src[src.index("static int dispatch("):src.index("void mexFunction(")]                # dispatch() holds no per-command code
    assert not [n for n in names if '"%s"' % n in body] and "with_handle" not in src


def _mandatory(usage):
    """The names of a usage string in front of its first '[' (the optional trailing arguments)."""
    return [t.strip() for t in usage.split("[")[0].split(",") if t.strip()]


def test_min_nrhs_is_the_usage_string_s_count():
    for name, (min_nrhs, handles, usage, _) in _mex.gateway_commands().items():
        assert min_nrhs == 1 + len(_mandatory(usage)), (name, min_nrhs, usage)
        assert handles <= len(_mandatory(usage)), name                                           # a handle slot is a mandatory argument
        assert usage.count("[") == usage.count("]") <= 1 and (usage.endswith("]") or "[" not in usage), (name, usage)


def _string_end(code, i):
    """Index of the quote that closes the MATLAB string opened at code[i] ('' inside it is a quote); the line's end if none does."""
    j = i + 1
    while j < len(code) and code[j] != "\n":
        if code[j] == "'":
            if code[j + 1: j + 2] != "'":
                return j
            j += 1
        j += 1
    return j


def _is_string_start(code, i):
    """A quote opens a string unless it follows an operand (a name, a number, a closing bracket, another transpose)."""
    return code[i] == "'" and not re.match(r"[\w.)\]}']", code[i - 1: i] or " ")


def _uncommented(code):
    """A MATLAB text without its % comments (a % inside a string is kept) and with its continuation lines joined."""
    out = []
    for ln in code.split("\n"):
        i = 0
        while i < len(ln) and ln[i] != "%":
            i = _string_end(ln, i) + 1 if _is_string_start(ln, i) else i + 1
        out.append(ln[:i])
    return re.sub(r"\.\.\.[^\n]*\n", "", "\n".join(out))


def _calls(code, cmd=r"\w+"):
    """(command, number of arguments after it) of every vbmc_hip_mex('command', ...) call in a MATLAB text; the arguments are
    counted at the top nesting level of the call; comments, strings and continuation lines are skipped.  A call that does not
    close is an error, not a count."""
    code = _uncommented(code)
    out = []
    for m in re.finditer(r"vbmc_hip_mex\(\s*'(%s)'" % cmd, code):
        depth, n, i = 1, 0, m.end()
        while depth:
            assert i < len(code), "unclosed call of %s" % m.group(1)
            ch = code[i]
            if _is_string_start(code, i):
                i = _string_end(code, i)
            elif ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
            elif ch == "," and depth == 1:
                n += 1
            i += 1
        out.append((m.group(1), n))
    return out


def test_shims_use_only_commands_the_gateway_implements():
    cmds = _mex.gateway_commands()
    assert _calls("x = vbmc_hip_mex('a',f(b,c)', ... % vbmc_hip_mex('no',1)\n  'k,l)',[1,2], 'it''s, 100%');  % vbmc_hip_mex('c',\n"
                  "y = a' + vbmc_hip_mex('b');") == [("a", 4), ("b", 0)]
    used = set()
    for fn in os.listdir(os.path.join(ROOT, "matlab")):
        if fn.endswith(".m"):
            used |= set(re.findall(r"vbmc_hip_mex\('([a-z_0-9]+)'", open(os.path.join(ROOT, "matlab", fn)).read()))
    assert used and used <= set(cmds), used - set(cmds)
    # ... and no call falls below its command's argument count (the command string is counted in min_nrhs)
    seen = []
    for fn in sorted(os.listdir(os.path.join(ROOT, "matlab"))):
        if fn.endswith(".m"):
            for cmd, n in _calls(open(os.path.join(ROOT, "matlab", fn)).read()):
                assert n >= cmds[cmd][0] - 1, (fn, cmd, n, cmds[cmd][0])
                seen.append(cmd)
    assert len(seen) >= len(used)


def test_gateway_links_and_runs_against_the_functional_mock():
    """The gateway + tests/mock_mex/mock_mx.cpp + libvbmc_hip.so link into one object and mexFunction EXECUTES (tests/_mex.py):
    without a GPU every command stops at the context ('vbmc_hip:nodevice', raised through the mock's mexErrMsgIdAndTxt), usage
    errors are reported before that, and nothing a failed call created stays alive.  The command-by-command comparison with
    the ctypes path is tests/test_gpu_mex.py."""
    m = _mex.mex()
    with pytest.raises(_mex.MexError) as e:
        m.call(0, 5.0)
    assert e.value.identifier == "vbmc_hip:usage"
    import torch

    if not torch.cuda.is_available():
        with pytest.raises(_mex.MexError) as e:
            m.call(1, "sq_dist", np.zeros((2, 3)))
        assert e.value.identifier == "vbmc_hip:nodevice"
    assert m.live_arrays() == 0
    # the mock's own value mapping: what MATLAB would hand the gateway, read back unchanged
    a = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    h = m.to_mx(a)
    assert np.array_equal(m.from_mx(h), a)
    m.lib.mxDestroyArray(h)
    h = m.to_mx([{"x": 1.0, "s": "ab"}, {"x": np.ones((2, 2)), "s": None}])
    assert m.live_arrays() == 5
    m.lib.mxDestroyArray(h)
    assert m.live_arrays() == 0


def test_short_calls_and_non_handles_are_usage_errors_before_any_device():
    """dispatch() counts the arguments and checks the handle slots from the table before it makes sure of the context: every
    command called with one argument too few raises 'vbmc_hip:usage' with "<name>: <usage>", and so does a double in a handle
    slot of a call that is long enough -- on a machine without a device too -- and nothing such a call created stays alive."""
    m = _mex.mex()
    short = handle_slots = 0
    for name, (min_nrhs, handles, usage, _) in _mex.gateway_commands().items():
        if min_nrhs >= 2:
            with pytest.raises(_mex.MexError) as e:
                m.call(1, name, *([0.0] * (min_nrhs - 2)))
            assert e.value.identifier == "vbmc_hip:usage" and e.value.message == "%s: %s" % (name, usage), (name, e.value.message)
            short += 1
        for bad in range(handles):                           # uint64 in front of the slot under test, doubles from there on
            args = [np.uint64(0)] * bad + [0.0] * (min_nrhs - 1 - bad)
            with pytest.raises(_mex.MexError) as e:
                m.call(1, name, *args)
            assert e.value.identifier == "vbmc_hip:usage" and "uint64 device handle" in e.value.message, (name, bad, e.value.message)
            handle_slots += 1
    assert short >= 32 and handle_slots >= 21
    with pytest.raises(_mex.MexError) as e:
        m.call(1, "no_such_command", 1.0)
    assert e.value.identifier == "vbmc_hip:usage" and e.value.message == "unknown command"
    assert m.live_arrays() == 0
