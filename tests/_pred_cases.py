"""The cases of tests/test_pred_restatement.py (CPU) and tests/test_gpu_pred_forms.py (device): each the smallest shape that reaches
one launch form of the prediction (vbmc_amd/csrc/gp_pred.h: pred_forms), with the form it has to report through
``vbmc_amd.gplite.pred_plan`` (test infrastructure).

A case is a dict: D, N, S, Nstar (a number, or a function of the device's compute-unit count where the form depends on it),
meanfun, noisefun, quad, two_kernel (run with VBMC_PRED_FUSED=0 in a child process) and ``form``: the fields of the reported plan
that must hold, each a value or a predicate of (value, plan).  ``case_data(name, num_cu)`` makes the surrogate, the points and the
extended-precision reference once per process; the surrogate comes from the oracle's gplite_post, so device and reference read the
same factors.  GPs with S >= 2 mix Cholesky samples with a low-noise one (tests/_quad_ref.mixed_gp: Lchol = [True, False, True])."""
import functools

import numpy as np

from oracle import vbmc_ref as R
from tests import _pred_ref as P
from tests import _quad_ref as Q
from tests._cases import synth_problem

CASES = {}
EXACT, FAR = 0.10, 0.05   # shares of exact training inputs and of far points among the test points (case_data)
# a case's seed is 1000 + its position, but for these: the first of 3000, 3001, .. at which the reference alone gives the power condition
SEEDS = {"qs_D13": 3004, "quad_qs_D28": 3002, "quad_small_D21_N20": 3003}


def _add(name, D, N, S, Nstar, form, meanfun=None, noisefun=(1, 0, 0), quad=False, two_kernel=False, seed=None, low_noise=True,
         sigma_scale=1.0):
    assert name not in CASES
    CASES[name] = dict(D=D, N=N, S=S, Nstar=Nstar, form=form, meanfun=(0, 1, 4)[(D + N + S) % 3] if meanfun is None else meanfun,
                       noisefun=noisefun, quad=quad, two_kernel=two_kernel, seed=1000 + len(CASES) if seed is None else seed,
                       low_noise=low_noise, sigma_scale=sigma_scale)


def _fused(**kw):
    return dict(dict(fused=1, slab=0), **kw)


def _twok(**kw):
    return dict(dict(fused=0, slab=0), **kw)


def _pt_class(D):
    return 3 if D <= 12 else (2 if D <= 20 else 1)


# ---- fused form -----------------------------------------------------------------------------------------------------------------
# 1. every QS at both ends of its class; four / three / two tiles: the last pass is short
for _D in (1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32):
    _pt = _pt_class(_D)
    _add("qs_D%d" % _D, _D, 40, 2, {3: 50, 2: 40, 1: 20}[_pt], _fused(QS=(_D + 3) // 4, PT=_pt, npass=2), seed=SEEDS.get("qs_D%d" % _D))
# 2. PT set by the LDS: 156928 B / (128 Np)
for _N, _pt in ((400, 3), (401, 2), (608, 2), (609, 1), (1136, 1)):
    _add("lds_N%d" % _N, 3, _N, 1, 50, _fused(PT=_pt, npass=(4 + _pt - 1) // _pt), meanfun=4, seed=2000 + _N)
# 3. small N: one row block, eleven idle waves, the per-wave sums larger than the tile block
for _N in (5, 16, 17):
    _add("small_N%d" % _N, 2, _N, 3, 40, _fused(PT=3, nblk=(_N + 15) // 16))
_add("small_D13_N16", 13, 16, 3, 33, _fused(PT=2, nblk=1))
_add("small_D21_N20", 21, 20, 3, 40, _fused(PT=1, nblk=2))
# 4. Nstar around one tile
for _n in (1, 15, 16, 17):
    _add("nstar_%d" % _n, 5, 50, 3, _n, _fused(PT=3, npass=1))
# 5. RS workgroups share a unit's row tiles (fmu written by rs = 0 alone)
for _N, _rs in ((112, 1), (128, 2), (192, 3), (256, 4), (1136, 4)):
    _add("rs_N%d" % _N, 3, _N, 1, 16, _fused(RS=_rs, units=1, grid=_rs, maxg=_rs), meanfun=4, seed=2000 + _N)
# 6. RS capped by the units: units > num_cu / 2 -> RS = 1, 25 row tiles on one workgroup
_add("rs_capped", 3, 400, 3, lambda cu: 16 * (3 * (cu // 6) + 1) - 5,
     _fused(PT=3, RS=1, nblk=25, units=lambda v, pl: 2 * v > pl["num_cu"]), meanfun=4)
# 7. the walk: units >= 1.5 num_cu with a short last pass; a workgroup goes from a Cholesky sample's unit to a low-noise one's and back
_add("walk", 4, 60, 3, lambda cu: 16 * (3 * ((cu + 1) // 2) + 1) - 5,
     _fused(PT=3, RS=1, units=lambda v, pl: 2 * v >= 3 * pl["num_cu"], grid=lambda v, pl: v == pl["num_cu"]), meanfun=4)
# noise models at the test points (ys2 alone reads them)
_add("noise_110", 5, 50, 2, 17, _fused(), noisefun=(1, 1, 0))
_add("noise_121", 5, 50, 2, 17, _fused(), noisefun=(1, 2, 1))
# 8. the quadrature twins of 1 (one D per PT class), 3 and 7.  The quadrature of a sample whose length scales are far below sigma has
# next to no data term (lnnf = ... + sum ln(ell / tau), :71), more so the larger D: the S = 2 twins of 1 have no low-noise sample, whose
# length scales are a quarter of the others', and the two D >= 13 shapes with one take a quarter of the sigma row
for _D in (4, 16, 28):
    _pt = _pt_class(_D)
    _add("quad_qs_D%d" % _D, _D, 40, 2, {3: 50, 2: 40, 1: 20}[_pt], _fused(QS=(_D + 3) // 4, PT=_pt, npass=2), quad=True, low_noise=False,
         seed=SEEDS.get("quad_qs_D%d" % _D))
for _N in (5, 16, 17):
    _add("quad_small_N%d" % _N, 2, _N, 3, 40, _fused(PT=3, nblk=(_N + 15) // 16), quad=True)
_add("quad_small_D13_N16", 13, 16, 3, 33, _fused(PT=2, nblk=1), quad=True, sigma_scale=0.25)
_add("quad_small_D21_N20", 21, 20, 3, 40, _fused(PT=1, nblk=2), quad=True, sigma_scale=0.25, seed=SEEDS["quad_small_D21_N20"])
_add("quad_walk", 4, 60, 3, lambda cu: 16 * (3 * ((cu + 1) // 2) + 1) - 5,
     _fused(PT=3, RS=1, units=lambda v, pl: 2 * v >= 3 * pl["num_cu"], grid=lambda v, pl: v == pl["num_cu"]), meanfun=4, quad=True)

# ---- two-kernel form (k_pred_ks + k_gp_pred), VBMC_PRED_FUSED=0 --------------------------------------------------------------------
# 9. resident row tiles R = 1 .. 8; 144: 8 + 1 (PRED_MAXR); 160: 8 + 2; 224: 8 + 5 + 1, the first split forced by the LDS
#    (6 x 16 rows x 14 x 16 columns x 8 B > PRED_LDS_MAX); 1136: 71 row tiles in groups that shrink to one tile, under PRED_MAXG
for _r in range(1, 9):
    _add("twok_R%d" % _r, 3, 16 * _r, 1, 40, _twok(maxg=1, Rmax=_r, Rmin=_r), two_kernel=True, meanfun=(0, 1, 4)[_r % 3])
_add("twok_N144", 3, 144, 1, 40, _twok(maxg=2, Rmax=8, Rmin=1), two_kernel=True)
_add("twok_N160", 3, 160, 1, 40, _twok(maxg=2, Rmax=8, Rmin=2), two_kernel=True)
_add("twok_N224", 3, 224, 1, 40, _twok(maxg=3, Rmax=8, Rmin=1), two_kernel=True)
_add("twok_N1136", 3, 1136, 1, 40, _twok(nblk=71, Rmax=8, Rmin=1, maxg=lambda v, pl: 40 < v <= 80), two_kernel=True, meanfun=4, seed=2000 + 1136)
# 10. low-noise and mixed samples: one tile per group over all columns
for _N in (40, 130):
    _add("twok_mixed_N%d" % _N, 3, _N, 3, 40, _twok(Rmin=1, maxg=(_N + 15) // 16), two_kernel=True)
# 11. the point tiles sliced over gridDim.z: one row group, one sample, 33 tiles -> PZ = 2 wherever num_cu >= 2
_add("twok_pz", 3, 64, 1, 16 * 33 - 3, _twok(maxg=1, PZ=lambda v, pl: v >= 2), two_kernel=True)

# ---- slab --------------------------------------------------------------------------------------------------------------------------
# 13. the first slab N (wider slabs stay with tests/test_gpu_limits.py)
_add("slab_N1137", 3, 1137, 2, 20, dict(fused=0, slab=1, cw=8), meanfun=4)


def nstar_of(c, num_cu):
    return c["Nstar"](num_cu) if callable(c["Nstar"]) else c["Nstar"]


def check_form(name, plan):
    for k, want in CASES[name]["form"].items():
        ok = want(plan[k], plan) if callable(want) else plan[k] == want
        assert ok, "%s: the plan reports %s = %r: %r" % (name, k, plan[k], plan)


@functools.lru_cache(maxsize=None)
def _gp(seed, D, N, S, meanfun, noisefun, low_noise=True):
    if noisefun == (1, 0, 0):
        return Q.mixed_gp(seed, D, N, S, meanfun, low_noise)[0]
    # the other noise models: mixed_gp's recipe (sn = 0.03, no low-noise sample) with observation variances s2
    p = synth_problem(seed, D, N, 3, S, meanfun=meanfun)
    nn = R.noisefun_nhyp(noisefun)
    hyp = np.zeros((D + 1 + nn + R.meanfun_nhyp(meanfun, D), S))
    hyp[:D + 1] = p["hyp"][:D + 1]
    hyp[D + 1 + nn:] = p["hyp"][D + 2:]
    hn = [np.log(0.03)] + ([np.log(0.5)] if noisefun[1] == 2 else []) + ([float(np.median(p["y"])), np.log(0.1)] if noisefun[2] == 1 else [])
    hyp[D + 1:D + 1 + nn] = np.array(hn)[:, None]
    s2 = 1e-3 + 1e-2 * np.random.default_rng(seed + 7).random(N)
    return R.gplite_post(hyp, p["X"], p["y"], meanfun=meanfun, noisefun=noisefun, s2=s2)


def quad_sigma(D, seed):
    """the sigma row of tests/test_gpu_quad.py: zero entries leave those coordinates unsmoothed"""
    sg = 0.1 + 0.4 * np.random.default_rng(seed).random(D)
    sg[::3] = 0.0
    if D == 1:
        sg[0] = 0.3
    return sg


@functools.lru_cache(maxsize=None)
def case_inputs(name, num_cu=256):
    """-> dict(gp, Xs, ys, s2s, sigma): the points of tests/_pred_ref.near_data_points with 10 % exact training inputs and 5 % far points.

    The scale of the near points is the SMALLEST length scale over the hyper-samples (the quadrature's tau), not the mean: the low-noise
    sample of a mixed GP has a quarter of the others' length scales, and a point at kernel value rho on the mean scale sits at rho^9 on
    that sample's.  Far points: at D >= 13 none of them passes the power condition's share for the mean (>= 0.9 of the pairs), so a
    share of 10 % would leave not one pair to spare; 5 % does."""
    c = CASES[name]
    gp = _gp(c["seed"], c["D"], c["N"], c["S"], c["meanfun"], tuple(c["noisefun"]), c["low_noise"])
    Nstar = nstar_of(c, num_cu)
    rng = np.random.default_rng(c["seed"] + 17)
    out = dict(gp=gp, ys=None, s2s=None, sigma=None)
    ell = np.stack([np.exp(p["hyp"][:c["D"]]) for p in gp["post"]])
    if c["quad"]:
        sg = c["sigma_scale"] * quad_sigma(c["D"], c["seed"])
        out["Xs"] = P.near_data_points(gp, Nstar, rng, exact=EXACT, far=FAR, scale=np.min(np.sqrt(sg[None, :] ** 2 + ell ** 2), axis=0))
        out["sigma"] = sg
        return out
    out["Xs"] = P.near_data_points(gp, Nstar, rng, exact=EXACT, far=FAR, scale=np.min(ell, axis=0))
    if c["noisefun"][1]:
        out["s2s"] = 1e-3 + 1e-2 * rng.random(Nstar)
    if c["noisefun"][2]:
        out["ys"] = float(np.median(gp["y"])) + rng.standard_normal(Nstar)
    return out


@functools.lru_cache(maxsize=None)
def case_data(name, num_cu=256):
    """case_inputs with ``ref``: pred_ld / quad_ld on them (what the comparing side needs; the child process that only runs the device
    does without)"""
    d = dict(case_inputs(name, num_cu))
    d["ref"] = P.quad_ld(d["gp"], d["Xs"], d["sigma"]) if CASES[name]["quad"] else P.pred_ld(d["gp"], d["Xs"], d["ys"], d["s2s"])
    return d


def check_mixed(name, gp):
    """the Lchol pattern a case counts on: S = 3 and S = 2 surrogates with the constant noise model carry the low-noise sample S // 2"""
    c = CASES[name]
    lch = [bool(p["Lchol"]) for p in gp["post"]]
    if c["S"] >= 2 and c["low_noise"] and tuple(c["noisefun"]) == (1, 0, 0):
        assert lch == [s != c["S"] // 2 for s in range(c["S"])], (name, lch)
    else:
        assert all(lch), (name, lch)


# ---- 12. the two-kernel form through its product entry: the IQR acquisition functions read the cross-kernel matrix (want_ks) -------
IQR_SHAPES = [(20, 90, 2, 37), (32, 40, 1, 20)]     # D, N, S, Na
IQR_NSTAR = 60


@functools.lru_cache(maxsize=None)
def iqr_case_data(shape):
    """-> dict(gp, vp, Xs, Xa, st_o, st_d by name, power figures): the set-up of tests/test_gpu_random_shapes._acquisition_case with the
    test and importance points from near_data_points"""
    D, N, S, Na = shape
    seed = 4000 + D
    p = synth_problem(seed, D, N, 3, S)
    gp = R.gplite_post(p["hyp"], p["X"], p["y"], meanfun=4)
    vp = R.make_vp(p["mu"], p["sigma"], p["lam"], eta=p["eta"])
    vp["w"] = np.exp(p["eta"]) / np.sum(np.exp(p["eta"]))
    rng = np.random.default_rng(seed + 3)
    Xs = P.near_data_points(gp, IQR_NSTAR, rng, exact=EXACT, far=FAR)
    Xa = P.near_data_points(gp, Na, rng, exact=EXACT, far=FAR)
    gl = P.mean_lengthscales(gp)
    gp = dict(gp, X_rescaled=p["X"] / gl[None, :], sn2new=0.02 + 0.1 * rng.random(N))
    st_ = {"ymax": float(np.max(p["y"])), "VarianceRegularizedAcqFcn": False, "TolGPVar": 1e-4, "gplengthscale": gl}
    Kax, Ct = R.acq_is_precompute(gp, Xa)
    fs2a = np.asarray(R.gplite_pred(gp, Xa, None, None, True)[3]).reshape(Na, -1)
    lnw = {"acqviqr": np.zeros((S, Na)), "acqimiqr": 0.5 * rng.standard_normal((S, Na))}
    st_o = {k: dict(st_, ActiveImportanceSampling={"Xa": Xa, "Kax_mat": Kax, "Ctmp_mat": Ct, "fs2a": fs2a, "lnw": v}) for k, v in lnw.items()}
    st_d = {k: dict(st_, ActiveImportanceSampling={"Xa": Xa, "lnw": v}) for k, v in lnw.items()}
    # the cross term Ks' Ctmp beside Ka (acqviqr_vbmc.m:84-90), from the oracle alone
    cross = []
    for s, post in enumerate(gp["post"]):
        ell, sf2 = np.exp(post["hyp"][:D]), np.exp(2 * post["hyp"][D])
        Ks = sf2 * np.exp(-R._acq_sqdist_rows(gp["X"] / ell[None, :], Xs / ell[None, :]) / 2.0)
        Ka = sf2 * np.exp(-R._acq_sqdist_rows(Xs / ell[None, :], Xa / ell[None, :]) / 2.0)
        cross.append(np.abs(Ks.T @ Ct[:, :, s]) > 1e-3 * Ka)
    return dict(gp=gp, vp=vp, Xs=Xs, Xa=Xa, st_o=st_o, st_d=st_d, cross_share=float(np.mean(cross)),
                ref_s=P.pred_ld(gp, Xs), ref_a=P.pred_ld(gp, Xa))
