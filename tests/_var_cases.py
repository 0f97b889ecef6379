"""The cases of tests/test_var_restatement.py (CPU) and tests/test_gpu_var_forms.py (device): mixtures whose components overlap, each
shape the smallest that reaches one edge of the variance stage (vbmc_amd/csrc/elbo_pass.h: Pass::variance), with the launch form it has
to report through ``Context.last_variance`` (vbmc_ctx_last_variance) (test infrastructure).

Why overlapping mixtures: tests/_cases.synth_problem puts its components on distinct training inputs, about eleven length scales apart at
D = 28, and J_jk (j != k) is then 1e-10 of J_kk -- below every tolerance, so that no off-diagonal tile of the Gram kernel is seen.
``overlap_problem`` picks C cluster centres among the training inputs and puts component k at centre k mod C plus
ell_min (.) u sqrt(-2 ln rho): u uniform on the sphere, rho log-uniform in [0.05, 0.9], ell_min the smallest length scale over the
hyper-samples; sigma_k about 0.3 mean(ell); lambda normalised as synth_problem does.  The surrogate is tests/_quad_ref.mixed_gp's (S >= 2:
the middle hyper-sample in the low-noise representation), or with every sample low-noise (``low="all"``).

A case is a dict: D, N, K, S, C, cv (compute_var), grad, flags (the optimise flags), jac (jacobian_flag), R (restarts in one call), low,
delta, seed and ``form``: the fields of the reported launch record that must hold.  ``case_data(name)`` makes the surrogate, the vp, the
thetas and the extended-precision reference of every restart once per process."""
import functools
import math

import numpy as np

from oracle import vbmc_ref as R
from tests import _quad_ref as Q
from tests import _var_ref as V
from tests._cases import synth_problem

TRSM2, SLAB, WAVE, MFMA = 1, 2, 1, 2     # VBMC_VARSOLVE_* / VBMC_VARGRAM_* (include/vbmc_hip.h)
CASES = {}
# a case's seed is 5000 + its position; every case meets the power conditions at that seed.  Should a new case fall short, it takes the
# first of 7000, 7001, .. at which the reference alone gives them, entered here: the shares are never lowered
SEEDS = {}


def sample_lds(K, T):
    return (256 + 2 * T + 2 * K) * 8                 # VAR_SAMPLE_LDS (vbmc_amd/csrc/var_kernels.h)


def final_lds(S, K, T):
    return (1024 + 2 * S + 5 * T + 2 * K + 8) * 8    # VAR_FINAL_LDS (vbmc_amd/csrc/elbo_pass.h)


def _full(**kw):
    """compute_var = 1 with a Cholesky sample, N <= 1136: the product with inv(L'), no substitution"""
    return dict(dict(compute_var=1, tri_gemm=1, fwd_solve=0, bwd_solve=0, solve_width=0, gram=MFMA, vgrad=0, sample_lds=0), **kw)


def _diag(kind, width, **kw):
    """compute_var = 2 with its gradient: forward and backward substitution of one form"""
    return dict(dict(compute_var=2, tri_gemm=0, fwd_solve=kind, bwd_solve=kind, solve_width=width, gram=WAVE, vgrad=1), **kw)


def _add(name, D, N, K, S, C, cv, form, grad=None, flags=(1, 1, 1, 1), jac=True, Rn=1, low="mixed", delta=False, meanfun=None):
    assert name not in CASES
    grad = (cv == 2) if grad is None else grad
    T = sum(V.block_sizes(D, K, flags))
    form = dict(form, symm=1 if (low == "all" or (low == "mixed" and S > 1)) else 0, final_lds=final_lds(S, K, T if grad else 0))
    if grad:
        form["sample_lds"] = sample_lds(K, T)
    CASES[name] = dict(D=D, N=N, K=K, S=S, C=C, cv=cv, grad=grad, flags=tuple(flags), jac=jac, R=Rn, low=low, delta=delta, form=form,
                       meanfun=(0, 1, 4)[(D + N + S) % 3] if meanfun is None else meanfun, seed=SEEDS.get(name, 5000 + len(CASES)))


# 1. Gram tiles (k_var_gram_mfma's walk t -> (tj, tk) over the upper triangle, 16 waves): 1, 1, 3, 21 (second trip of the wave loop,
#    clamped edge rows) and 528 tiles (k_var_final's K^2 pair loop); the [1, 0, 1] arrangement; every sample low-noise (no inv(L'):
#    k_symm supplies both operands, the substitution kernels are enqueued and return at once)
for _K in (1, 16, 17, 83, 512):
    _add("tiles_K%d" % _K, 2, 20, _K, 1, 3, 1, _full())
_add("tiles_mixed", 2, 20, 33, 3, 3, 1, _full())
_add("tiles_all_low", 2, 20, 33, 2, 3, 1, _full(tri_gemm=0, fwd_solve=TRSM2, solve_width=4), low="all")
# 2. remainders of the inner dimension in k_var_gram_mfma and k_tri_gemm (32, then 8, then 4 with masking; nend = min(i0 + 16, N))
for _N in (3, 4, 9, 17, 36, 43, 70):
    _add("inner_N%d" % _N, 2, _N, 17, 2, 2, 1, _full())
# 3. padded dimensions of k_var_z<DT> / k_vargrad<DT>
for _D in (1, 12, 13, 17, 21, 25, 29, 32):
    _add("pad_D%d" % _D, _D, 12 if _D == 1 else 40, 6, 2, 2, 2, _diag(TRSM2, 4))
# 4. the forms of the triangular step at their switch points
for _N, _kind, _w in ((512, TRSM2, 4), (513, TRSM2, 8), (1024, TRSM2, 8), (1025, SLAB, 16), (1137, SLAB, 8)):
    _add("solve_N%d" % _N, 3, _N, 5, 2, 2, 2, _diag(_kind, _w), meanfun=4)
_add("product_N1136", 3, 1136, 5, 2, 2, 1, _full(), meanfun=4)
_add("product_N1137", 3, 1137, 5, 2, 2, 1, _full(tri_gemm=0, fwd_solve=SLAB, solve_width=8), meanfun=4)
# 5. hyper-samples: k_var_final's second trip of the 16-wave loop over S and the remainders of its four-sample loads
for _S in (17, 20):
    _add("samples_S%d_full" % _S, 3, 40, 6, _S, 2, 1, _full())
    _add("samples_S%d_diag" % _S, 3, 40, 6, _S, 2, 2, _diag(TRSM2, 4))
# 6. restarts: three distinct thetas in one call (the R-strides of Z, X, J, vg, vs), each column against its own reference
_add("restarts_full", 4, 50, 17, 3, 2, 1, _full(), Rn=3)
_add("restarts_diag", 4, 50, 17, 3, 2, 2, _diag(TRSM2, 4), Rn=3)
# 7. large T: T = 3028, k_var_final's LDS beyond 64 KiB; 28 tiles; and T + K > 3968: k_var_sample's LDS beyond 64 KiB (reachable
#    below the refusal at 160 KiB of k_var_final: T = 3618, K = 361 gives 65 712 B and 158 784 B)
_add("large_T_diag", 28, 150, 100, 2, 3, 2, _diag(TRSM2, 4))
_add("large_T_full", 28, 150, 100, 2, 3, 1, _full())
_add("sample_lds_64k", 8, 20, 361, 2, 3, 2, _diag(TRSM2, 4))
# 8. a per-dimension vp.delta through a multi-tile matrix and through the gradient
_add("delta_full", 4, 50, 33, 3, 2, 1, _full(), delta=True)
_add("delta_diag", 4, 50, 20, 3, 2, 2, _diag(TRSM2, 4), delta=True)
# 9. gradient flags
_add("no_jacobian", 5, 60, 20, 3, 2, 2, _diag(TRSM2, 4), jac=False)
_add("flags_1010", 5, 60, 20, 3, 2, 2, _diag(TRSM2, 4), flags=(1, 0, 1, 0))

assert CASES["large_T_diag"]["form"]["final_lds"] > 65536 > CASES["large_T_diag"]["form"]["sample_lds"]
assert CASES["sample_lds_64k"]["form"]["sample_lds"] > 65536 and CASES["sample_lds_64k"]["form"]["final_lds"] <= 160 * 1024
ORACLE_CASES = sorted(n for n, c in CASES.items() if c["K"] <= 128)      # the oracle's pair loop is O(K^2 N^2) in Python


def check_form(name, rec):
    for k, want in CASES[name]["form"].items():
        assert rec[k] == want, "%s: the launch record has %s = %r, not %r: %r" % (name, k, rec[k], want, rec)


@functools.lru_cache(maxsize=None)
def _gp(seed, D, N, S, meanfun, low):
    if low != "all":
        return Q.mixed_gp(seed, D, N, S, meanfun, low == "mixed")
    # every sample as mixed_gp's low-noise one: sn2 = 9e-8, a quarter of the length scales
    p = synth_problem(seed, D, N, 3, S, meanfun=meanfun)
    hyp = p["hyp"].copy()
    hyp[D + 1, :] = math.log(3e-4)
    hyp[:D, :] += math.log(0.25)
    return R.gplite_post(hyp, p["X"], p["y"], meanfun=meanfun), p


def overlap_problem(seed, gp, K, C, flags=(1, 1, 1, 1), Rn=1, delta=False):
    """-> (vp, thetas T x Rn): the generator of the module docstring; restarts beyond the first move every parameter by 0.05 N(0, 1)"""
    X = np.asarray(gp["X"], dtype=np.float64)
    N, D = X.shape
    rng = np.random.default_rng(seed + 29)
    ell = np.stack([np.exp(np.asarray(p["hyp"][:D], dtype=np.float64)) for p in gp["post"]])
    centres = X[rng.choice(N, size=min(C, N), replace=False)]
    u = rng.standard_normal((K, D))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rho = np.exp(rng.uniform(math.log(0.05), math.log(0.9), size=K))
    mu = (centres[np.arange(K) % centres.shape[0]] + np.min(ell, axis=0)[None, :] * u * np.sqrt(-2.0 * np.log(rho))[:, None]).T.copy()
    sigma = 0.3 * float(np.mean(ell)) * np.exp(0.2 * rng.standard_normal(K))
    lam = np.exp(0.2 * rng.standard_normal(D))
    lam = lam * np.sqrt(D / np.sum(lam ** 2))
    eta = 0.3 * rng.standard_normal(K)
    vp = R.make_vp(mu, sigma, lam, eta=eta, optimize=tuple(bool(f) for f in flags))
    vp["w"] = np.exp(eta) / np.sum(np.exp(eta))
    if delta:    # of the order of ell_min and sigma_k lambda_d, the entries different per dimension
        vp["delta"] = (0.5 + rng.random(D)) * float(np.min(ell))
    parts = [mu.reshape(-1, order="F"), np.log(sigma), np.log(lam), eta]
    theta = np.concatenate([x for x, f in zip(parts, flags) if f])
    thetas = np.repeat(theta[:, None], Rn, axis=1)
    thetas[:, 1:] += 0.05 * rng.standard_normal((theta.size, Rn - 1))
    return vp, np.asfortranarray(thetas)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    c = CASES[name]
    gp, _ = _gp(c["seed"], c["D"], c["N"], c["S"], c["meanfun"], c["low"])
    vp, thetas = overlap_problem(c["seed"], gp, c["K"], c["C"], c["flags"], c["R"], c["delta"])
    return dict(gp=gp, vp=vp, thetas=thetas, vps=[V.vp_of_theta(vp, thetas[:, r]) for r in range(c["R"])])


@functools.lru_cache(maxsize=None)
def case_data(name):
    """case_inputs with ``refs``: var_ld of every restart's vp"""
    c, d = CASES[name], dict(case_inputs(name))
    d["refs"] = [V.var_ld(d["gp"], v, c["cv"], c["flags"] if c["grad"] else (0, 0, 0, 0), c["jac"]) for v in d["vps"]]
    return d


def check_mixed(name, gp):
    c = CASES[name]
    lch = [bool(p["Lchol"]) for p in gp["post"]]
    want = [False] * c["S"] if c["low"] == "all" else [not (c["S"] > 1 and s == c["S"] // 2) for s in range(c["S"])]
    assert lch == want, (name, lch)
