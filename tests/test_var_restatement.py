"""CPU: the extended-precision restatement tests/_var_ref.py of the variance of the expected log joint against the 50-digit goldens, the
power conditions of every case of tests/_var_cases.py, the float64 oracle's error in the restatement's units -- what the device's bounds
in tests/test_gpu_var_forms.py are built from -- and float64 mutants of the computation that those bounds have to catch.

E_REF_J / E_REF_VAR / E_REF_DVAR: the worst error of oracle/vbmc_ref.gplogjoint against the restatement, in units of u = 2^-53 of the
magnitudes added up (tests/_var_ref.py), as this test measured it (printed with -s) over the cases with K <= 128 -- the oracle's pair loop
is O(K^2 N^2) in Python -- and every diagonal-variance case: J_sjk; varG, varG_s, varGss; dvarG and dvarG_s, the worst block.  The oracle is
locked a quarter above them (CEIL_*: a BLAS that adds in another order); one that stays under half of them only warns.  What sets them:
J at (D 28, N 150, K 100) -- the table of distances feeding exp() at d^2 / 2 in the hundreds -- and the gradient at D = 1, where twelve
inputs on a line make K + sn2 I ill-conditioned and the two substitutions behind invKzk lose what the units do not know of."""
import warnings

import numpy as np
import pytest

from oracle import vbmc_ref as R
from tests import _var_cases as C
from tests import _var_ref as V
from tests._cases import delta_golden_cases, golden_cases, load_delta_golden, load_golden, synth_problem, vp_from_inputs
from tests.test_pred_restatement import DEVICE_FACTOR

E_REF_J = 2779.0      # measured: large_T_full
E_REF_VAR = 44.4      # measured: pad_D29
E_REF_DVAR = 989.0    # measured: pad_D1
CEIL_J, CEIL_VAR, CEIL_DVAR = 1.25 * E_REF_J, 1.25 * E_REF_VAR, 1.25 * E_REF_DVAR
BOUND_J, BOUND_VAR, BOUND_DVAR = DEVICE_FACTOR * E_REF_J, DEVICE_FACTOR * E_REF_VAR, DEVICE_FACTOR * E_REF_DVAR
ORACLE_CASES = sorted(n for n, c in C.CASES.items() if c["K"] <= 128 or c["cv"] == 2)

_seen = {}


# ---- the restatement against the goldens ------------------------------------------------------------------------------------------------
def _golden(path):
    if "delta" in path:
        inp, vp, gp, exp = load_delta_golden(path)
        return vp, gp, exp
    inp, exp = load_golden(path)
    gp = R.gplite_post(inp["hyp"], inp["X"], inp["y"], meanfun=inp["meanfun"])
    for s, post in enumerate(gp["post"]):
        post["alpha"], post["L"] = np.array(exp["alpha"][s]), np.array(exp["L"][s])
    return vp_from_inputs(inp), gp, {k: np.array(v, dtype=np.float64) for k, v in exp.items()}


@pytest.mark.parametrize("path", golden_cases() + delta_golden_cases())
def test_restatement_against_the_50_digit_goldens(path):
    """J_sjk, varG_s (full and diagonal) and, where the file has it, dvarG_s.  The goldens were computed from Cholesky factors of 50
    digits and the gp carries them rounded to float64, so the allowance is one unit of the entry's magnitude -- the goldens' own rounding
    is half of one -- plus u / 2 times the first-order sensitivity to the factor's entries (var_ld's ``lsens``; without it mp_case2,
    eight inputs on a line, is 357 units off in one J).  The values sit under 0.6 of that for J and varG_s; the gradient, two solves
    with the rounded factor bounded to first order only, reaches 1.4 and is held to 2."""
    vp, gp, exp = _golden(path)
    r1 = V.var_ld(gp, vp, 1, lsens=True)
    r2 = V.var_ld(gp, vp, 2, (1, 1, 1, 1), lsens=True)
    ww = np.outer(vp["w"], vp["w"])
    eJ = V.err_units(exp["J_sjk"], r1.J, r1.Jmag + r1.J_lsens / 2)
    eF = V.err_units(exp["varG_s_full"], r1.varF_s, r1.varF_mag + np.sum(ww[None] * r1.J_lsens, axis=(1, 2)) / 2)
    eD = V.err_units(exp["varG_s_diag"], r2.varF_s, r2.varF_mag + np.sum(ww[None] * r2.J_lsens, axis=(1, 2)) / 2)
    print("%s: J %.3f  varG_s full %.3f  diag %.3f" % (path[-20:], eJ, eF, eD))
    assert eJ < 1.0 and eF < 1.0 and eD < 1.0
    if "dvarG_s_diag" in exp:
        eG = V.err_dvar_blocks(exp["dvarG_s_diag"].T, r2.dvarF_s, r2.dvarF_s_mag + r2.dv_lsens / 2, r2.sizes)
        print("   dvarG_s", eG)
        assert max(eG.values()) < 2.0, eG


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_case_meets_the_power_conditions(name):
    c, d = C.CASES[name], C.case_data(name)
    assert d["gp"]["X"].shape == (c["N"], c["D"]) and len(d["gp"]["post"]) == c["S"] and d["thetas"].shape[1] == c["R"] == len(d["refs"])
    C.check_mixed(name, d["gp"])
    for r, ref in enumerate(d["refs"]):
        tp, vg = V.assert_power(ref, c["cv"], c["grad"], "%s, restart %d" % (name, r))
        print("%-18s r%d  min J_kk %.2e eps  worst tile share %s  dvarF data shares %s" % (name, r, V.diag_floor(ref), tp, vg))
    if c["R"] > 1:     # the restarts are distinct problems: J moves by far more than any bound
        assert V.err_J(d["refs"][1].J, d["refs"][0], c["cv"]) > 1e3 * BOUND_J


def test_the_old_recipe_sees_no_off_diagonal_entry():
    """tests/_cases.synth_problem at (28, 150, 100, 2), the shape of test_variance_paths_at_large_parameter_counts: components on distinct
    training inputs, eleven length scales apart -- no off-diagonal pair of any tile has power, and max |J_jk| lies under that test's
    tolerance of 1e-7 max(1, max |J|)"""
    p = synth_problem(7, 28, 150, 100, 2)
    gp = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=4)
    vp = R.make_vp(p["mu"], p["sigma"], p["lam"], eta=p["eta"])
    vp["w"] = np.exp(p["eta"]) / np.sum(np.exp(p["eta"]))
    ref = V.var_ld(gp, vp, 1)
    assert V.tile_power(ref) == 0.0
    off = ~np.eye(100, dtype=bool)
    Jmax, Joff = float(np.max(np.abs(ref.J))), float(np.max(np.abs(ref.J[:, off])))
    print("max |J| %.3g, max off-diagonal |J_jk| %.3g" % (Jmax, Joff))
    assert Joff < 1e-7 * max(1.0, Jmax)
    with pytest.raises(AssertionError):
        V.assert_power(ref, 1, False)


def test_k_var_sample_lds_branch_is_reachable():
    """VAR_SAMPLE_LDS passes 64 KiB when T + K > 3968, the call is refused when VAR_FINAL_LDS passes 160 KiB, 5 T + 2 K + 2 S > 19448:
    both hold at once for K >= 136 among the shapes with D <= 32 -- the case sample_lds_64k is one such shape, large_T_diag is not"""
    shapes = [(D, K) for D in range(1, 33) for K in range(1, 513)
              if C.sample_lds(K, D * K + 2 * K + D) > 65536 and C.final_lds(2, K, D * K + 2 * K + D) <= 160 * 1024]
    assert shapes and min(K for _, K in shapes) == 136 and (8, 361) in shapes and (28, 100) not in shapes


def check_entries(gp, vp, compute_var, grad_flags=(0, 0, 0, 0), jacobian_flag=True, what="", **got):
    """The per-entry comparison for the older variance tests, beside their max(1, max |.|) yardsticks: the inputs must have power, then
    each output given -- J (S x K x K), varF_s (S), varG, varGss, dvarF_s (T x S), dvarF (T) -- is held to the device bounds in the
    restatement's units.  -> the errors"""
    ref = V.var_ld(gp, vp, compute_var, grad_flags, jacobian_flag)
    V.assert_power(ref, compute_var, any(grad_flags), what)
    S, e = len(gp["post"]), {}
    if "J" in got:
        e["J"] = (V.err_J(got["J"], ref, compute_var), BOUND_J)
    if "varF_s" in got:
        e["varF_s"] = (V.err_units(np.atleast_1d(got["varF_s"]), ref.varF_s, ref.varF_mag), BOUND_VAR)
    if "varG" in got:
        e["varG"] = (V.err_units(got["varG"], ref.varG, ref.varG_mag), BOUND_VAR)
    if "varGss" in got and S > 1:
        e["varGss"] = (V.err_units(got["varGss"], ref.varGss, ref.varGss_mag), BOUND_VAR)
    if "dvarF_s" in got:
        e["dvarF_s"] = (max(V.err_dvar_blocks(got["dvarF_s"], ref.dvarF_s, ref.dvarF_s_mag, ref.sizes).values()), BOUND_DVAR)
    if "dvarF" in got:
        e["dvarF"] = (max(V.err_dvar_blocks(got["dvarF"], ref.dvarF, ref.dvarF_mag, ref.sizes).values()), BOUND_DVAR)
    assert set(got) <= {"J", "varF_s", "varG", "varGss", "dvarF_s", "dvarF"}
    print("%s per-entry e: %s" % (what, "  ".join("%s %.1f" % (k, v[0]) for k, v in e.items())))
    over = {k: v for k, v in e.items() if not v[0] <= v[1]}
    assert not over, (what, over)
    return e


MATTERS = 1e4     # tests/test_gpu_delta.py: a case's delta moves each compared quantity by this many times its bound


def delta_matters(name):
    """the reference without vp.delta is MATTERS times the bound away in every compared quantity: a kernel that ignored delta could
    not pass"""
    c, d = C.CASES[name], C.case_data(name)
    ref = d["refs"][0]
    r0 = V.var_ld(d["gp"], dict(d["vps"][0], delta=None), c["cv"], c["flags"] if c["grad"] else (0, 0, 0, 0), c["jac"])
    assert V.err_units(r0.varF_s, ref.varF_s, ref.varF_mag) >= MATTERS * BOUND_VAR and V.err_units(r0.varG, ref.varG, ref.varG_mag) >= MATTERS * BOUND_VAR
    if c["grad"]:
        for k, v in V.err_dvar_blocks(r0.dvarF_s, ref.dvarF_s, ref.dvarF_s_mag, ref.sizes).items():
            assert v >= MATTERS * BOUND_DVAR, (k, v)
    else:
        off = np.broadcast_to(~np.eye(c["K"], dtype=bool)[None], ref.J.shape)
        assert V.err_units(r0.J, ref.J, ref.Jmag, off) >= MATTERS * BOUND_J and V.err_J(r0.J, ref, 2) >= MATTERS * BOUND_J


@pytest.mark.parametrize("name", sorted(n for n, c in C.CASES.items() if c["delta"]))
def test_delta_cases_depend_on_delta(name):
    delta_matters(name)


# ---- the oracle in the restatement's units ---------------------------------------------------------------------------------------------
def oracle_errors(name):
    c, d = C.CASES[name], C.case_data(name)
    eJ = eV = eD = 0.0
    gf = c["flags"] if c["grad"] else (0, 0, 0, 0)
    for vp, ref in zip(d["vps"], d["refs"]):
        a = R.gplogjoint(vp, d["gp"], gf, True, c["jac"], c["cv"], separate_K=not c["grad"], compute_vargrad=c["grad"])
        b = R.gplogjoint(vp, d["gp"], gf, False, c["jac"], c["cv"], compute_vargrad=c["grad"]) if c["S"] > 1 else a
        if not c["grad"]:
            eJ = max(eJ, V.err_J(a["J_sjk"], ref, c["cv"]))
        eV = max(eV, V.err_units(a["varF"], ref.varG, ref.varG_mag), V.err_units(np.atleast_1d(b["varF"]), ref.varF_s, ref.varF_mag))
        if c["S"] > 1:
            eV = max(eV, V.err_units(a["varss"], ref.varGss, ref.varGss_mag))
        if c["grad"]:
            eD = max(eD, max(V.err_dvar_blocks(a["dvarF"], ref.dvarF, ref.dvarF_mag, ref.sizes).values()),
                     max(V.err_dvar_blocks(np.asarray(b["dvarF"]).reshape(ref.dvarF_s.shape), ref.dvarF_s, ref.dvarF_s_mag, ref.sizes).values()))
    return eJ, eV, eD


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_oracle_agrees_with_the_restatement(name):
    _seen[name] = e = oracle_errors(name)
    print("%-18s oracle e: J %8.1f  varG / varG_s / varGss %8.1f  dvarG / dvarG_s %8.1f" % ((name,) + e))
    assert e[0] <= CEIL_J and e[1] <= CEIL_VAR and e[2] <= CEIL_DVAR, e


def test_e_ref_is_what_the_oracle_reaches():
    for name in ORACLE_CASES:
        if name not in _seen:
            _seen[name] = oracle_errors(name)
    e = [max(v[i] for v in _seen.values()) for i in range(3)]
    print("e_ref: J %.1f (E_REF_J = %g)  var %.1f (E_REF_VAR = %g)  dvar %.1f (E_REF_DVAR = %g)" % (e[0], E_REF_J, e[1], E_REF_VAR, e[2], E_REF_DVAR))
    assert e[0] <= CEIL_J and e[1] <= CEIL_VAR and e[2] <= CEIL_DVAR, "the float64 oracle is further from the restatement than recorded: %r" % (e,)
    if e[0] < E_REF_J / 2 or e[1] < E_REF_VAR / 2 or e[2] < E_REF_DVAR / 2:
        warnings.warn("the float64 oracle reaches %r here, under half the recorded e_ref: another BLAS order, or the recorded figures "
                      "want measuring again" % (e,))


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
def _nf_f64(vp, post, D, delta_factor=2.0, same_sigma=False):
    """nf_jk (gplogjoint.m:313-317) in float64; the two mutants: delta^2 where 2 delta^2 belongs, sigma_j for sigma_k"""
    mu, sg, lam = vp["mu"], vp["sigma"], vp["lambda"]
    dl = vp.get("delta")
    dl = np.zeros(D) if dl is None else np.broadcast_to(np.asarray(dl, dtype=np.float64).reshape(-1), (D,))
    hyp = np.asarray(post["hyp"], dtype=np.float64)
    s2 = (2 * sg[:, None] ** 2 + 0 * sg[None, :]) if same_sigma else sg[:, None] ** 2 + sg[None, :] ** 2
    t2 = s2[:, :, None] * lam ** 2 + np.exp(hyp[:D]) ** 2 + delta_factor * dl ** 2
    dm = mu.T[:, None, :] - mu.T[None, :, :]
    nf = np.exp(2 * hyp[D] + np.sum(hyp[:D]) - 0.5 * np.sum(np.log(t2), axis=2) - 0.5 * np.sum(dm ** 2 / t2, axis=2))
    return np.triu(nf) + np.triu(nf, 1).T       # (the pair loop runs over j <= k and mirrors)


def _J_f64(d, r, mutant=None):
    """J_sjk of restart r from the float64 images of the restatement's operands: per sample nf - scale A' B by 16 x 16 tiles"""
    ref, vp, gp = d["refs"][r], d["vps"][r], d["gp"]
    S, K, _ = ref.J.shape
    D, nt = vp["D"], (K + 15) // 16
    out = np.zeros((S, K, K))
    for s in range(S):
        A, B, scale = (np.asarray(x, dtype=np.float64) for x in d["refs"][0 if mutant == "restart0_Z" else r].ops[s])
        n = A.shape[0]
        if mutant in ("cut4", "cut8", "cut32"):
            n -= n % int(mutant[3:])
        q = (A[:n].T @ B[:n]) * scale
        q = np.triu(q) + np.triu(q, 1).T
        tj, tk = 0, nt - 1                                  # the off-diagonal tile furthest from the diagonal
        sj, sk = slice(16 * tj, 16 * tj + 16), slice(16 * tk, min(16 * tk + 16, K))
        if mutant == "tile_zero" and nt > 1:
            q[sj, sk] = 0.0
            q[sk, sj] = 0.0
        if mutant == "tile_swap" and nt > 1:                # the dots of tile (0, 0)'s leading columns in its place
            q[sj, sk] = q[0:16, 0:sk.stop - sk.start].copy()
            q[sk, sj] = q[sj, sk].T
        nf = _nf_f64(vp, gp["post"][s], D, 1.0 if mutant == "delta_once" else 2.0, mutant == "sigma_j_twice")
        out[s] = nf - q
    return out


FULL_CASES = sorted(n for n, c in C.CASES.items() if c["cv"] == 1)
MUTANTS = ["tile_swap", "tile_zero", "cut4", "cut8", "cut32", "restart0_Z", "delta_once", "sigma_j_twice"]


def _worst(name, mutant):
    d = C.case_data(name)
    return max(V.err_J(_J_f64(d, r, mutant), d["refs"][r], 1) for r in range(len(d["refs"])))


def test_the_unmutated_float64_computation_is_within_the_device_bound():
    for name in FULL_CASES:
        assert _worst(name, None) <= BOUND_J, name


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_exceeds_the_device_bound_on_some_case(mutant):
    """float64 variants of the computation, on the CPU: another tile's dots in an off-diagonal tile, a zeroed tile, the inner sum cut to
    a multiple of 4, 8, 32, restart r reading restart 0's operands, delta^2 for 2 delta^2 in tau_jk, sigma_j for sigma_k in nf_jk.
    Each has to pass the device's bound on J by a factor of a thousand on at least one case, or the case table has a hole"""
    caught = {n: e for n in FULL_CASES for e in [_worst(n, mutant)] if e > 1e3 * BOUND_J}
    print(mutant, "caught by", {n: "%.2e" % e for n, e in caught.items()})
    assert caught, mutant
    tiled = [n for n in FULL_CASES if C.CASES[n]["K"] > 16]
    if mutant in ("tile_swap", "tile_zero"):                # every multi-tile case catches these: the power condition at work
        assert set(tiled) <= set(caught), sorted(set(tiled) - set(caught))
