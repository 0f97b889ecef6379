"""Cases of the device-resident search of the IQR acquisition functions (vbmc_acq_search_iqr): the NumPy restatement
tests/_acqsearch_ref.py::cmaes_chol run over the oracle's acqwrapper_vbmc(X, vp, gp, st, "acqviqr" | "acqimiqr"), on GPs from
tests/_quad_ref.mixed_gp with optimState.ActiveImportanceSampling built as tests/test_gpu_acq.py::iqr_setup builds it (from
oracle.vbmc_ref.acq_is_precompute / gplite_pred).

Each case is (D, N, S, Na, function, regulariser, face, popsize, seed), the smallest that reaches its edge:
  D2     lambda = 6, N = 17: two 16-row chunks, most waves of the tile kernel without one, one importance-point tile
  D3     S = 3 with the middle hyper-sample on the Lchol = false branch, Na = 37: padding inside the last tile, regulariser on
  face   D3 with its start on a face of the box (clamping active from the first generation)
  D5     IMIQR: per-hyper-sample Xa, non-zero lnw, N = 150 no multiple of 16 nor of 128
  D10    S = 1, Na = 100: seven tiles, regulariser on
  D32    IMIQR, lambda = 14, the 33-stride of the point rows
  full   popsize = 16: a full point tile, Na = 256: sixteen tiles
  slab   N = 1264: the prediction's slab form with the cross-kernel tile kept
The seeds are ones for which the restatement's own 12-generation trajectory meets the preconditions of the GPU comparison
(tests/test_acqsearch_iqr_restatement.py asserts them for every case): every gap between neighbouring sorted values above
1e-6 (1 + |F|), every visited value finite and, with the regulariser on, the smallest vtot visited above TolGPVar."""
import numpy as np

from oracle import vbmc_ref as R
from tests import _acqsearch_ref as A

GENS = 12


def iqr_cases():
    return {
        "D2": (2, 17, 1, 16, "acqviqr", False, False, 0, 1),
        "D3": (3, 40, 3, 37, "acqviqr", True, False, 0, 1),
        "face": (3, 40, 3, 37, "acqviqr", True, True, 0, 3),
        "D5": (5, 150, 3, 50, "acqimiqr", False, False, 0, 1),
        "D10": (10, 200, 1, 100, "acqviqr", True, False, 0, 1),
        "D32": (32, 40, 1, 20, "acqimiqr", False, False, 0, 1),
        "full": (4, 200, 1, 256, "acqviqr", False, False, 16, 3),
        "slab": (4, 1264, 1, 16, "acqviqr", False, False, 0, 1),
    }


def build_case(name, seed=None):
    from tests import _quad_ref as Q

    D, N, S, Na, fun, reg, face, popsize, seed0 = iqr_cases()[name]
    seed = seed0 if seed is None else seed
    gp, _ = Q.mixed_gp(seed, D, N, S, 4)
    rng = np.random.default_rng(seed + 70)
    X = gp["X"]
    K = 2
    mu = X[rng.permutation(N)[:K]].T.copy()
    lam = 0.8 + 0.4 * rng.random(D)
    w = rng.dirichlet(np.ones(K))
    vp = R.make_vp(mu, 0.5 + 0.3 * rng.random(K), lam * np.sqrt(D / np.sum(lam ** 2)), eta=np.log(w))
    vp["w"] = w
    gl = np.exp(np.mean(np.stack([q["hyp"][:D] for q in gp["post"]], axis=1), axis=1))
    gp = dict(gp, X_rescaled=X / gl[None, :], sn2new=0.02 + 0.1 * rng.random(N))
    imiqr = fun == "acqimiqr"
    xr = np.max(X, axis=0) - np.min(X, axis=0)
    LB, UB = np.min(X, axis=0) - 0.1 * xr, np.max(X, axis=0) + 0.1 * xr
    x0 = X[int(np.argmax(gp["y"]))] + 0.05 * rng.standard_normal(D)
    x0 = np.minimum(np.maximum(x0, LB), UB)
    if face:
        x0[0] = UB[0]
        x0[-1] = LB[-1]
    # importance points about one length scale from the start (|dx / ell|^2 ~ 1 whatever D): farther away the cross-covariance with the
    # searched points vanishes and the function is flat to the last bit, which no rank comparison survives
    spread = gl / np.sqrt(D)
    Xa = x0[None, :, None] + spread[None, :, None] * rng.standard_normal((Na, D, S)) if imiqr else x0 + spread * rng.standard_normal((Na, D))
    Kax, Ct = R.acq_is_precompute(gp, Xa)
    if imiqr:
        fs2a = np.stack([np.asarray(R.gplite_pred(gp, Xa[:, :, s], None, None, True)[3]).reshape(Na, -1)[:, s] for s in range(S)], axis=1)
    else:
        fs2a = np.asarray(R.gplite_pred(gp, Xa, None, None, True)[3]).reshape(Na, -1)
    lnw = 0.7 * rng.standard_normal((S, Na)) if imiqr else np.zeros((S, Na))
    ais = {"Xa": Xa, "Kax_mat": Kax, "Ctmp_mat": Ct, "fs2a": fs2a, "lnw": lnw}
    st = {"ymax": float(np.max(gp["y"])), "VarianceRegularizedAcqFcn": reg, "TolGPVar": 1e-4, "gplengthscale": gl, "ActiveImportanceSampling": ais}
    lamp = popsize or A.default_popsize(D)
    Z = rng.standard_normal((D, lamp, GENS + 4))
    return {"gp": gp, "vp": vp, "st": st, "acq": fun, "x0": x0, "insigma": 0.5 * spread, "LB": LB, "UB": UB, "Z": Z, "D": D, "lam": lamp,
            "popsize": popsize, "reg": reg, "face": face}


def objective(case):
    """X (lam x D) -> the oracle's acqwrapper_vbmc; ``seen`` collects the smallest vtot and whether every value was finite."""
    seen = {"vtot_min": np.inf, "finite": True}

    def fun(X):
        acq, _, vtot = R.acqwrapper_vbmc(X, case["vp"], case["gp"], case["st"], case["acq"])
        acq = np.asarray(acq, dtype=np.float64).reshape(-1)
        seen["vtot_min"] = min(seen["vtot_min"], float(np.min(vtot)))
        seen["finite"] = seen["finite"] and bool(np.all(np.isfinite(acq)))
        return acq

    return fun, seen


def run_case(case, gens=GENS):
    fun, seen = objective(case)
    ref = A.cmaes_chol(fun, case["x0"], case["insigma"], case["LB"], case["UB"], TolX=0.0, TolFun=0.0, TolHistFun=0.0, MaxIter=gens,
                       popsize=case["popsize"], Z=case["Z"])
    ref["seen"] = seen
    return ref


def preconditions(case, ref):
    """(rank gap, smallest vtot, all finite) and whether they meet the GPU comparison's guard."""
    gap = A.min_rank_gap(ref["trace"])
    ok = gap > 1e-6 and ref["seen"]["finite"] and (not case["reg"] or ref["seen"]["vtot_min"] > case["st"]["TolGPVar"])
    return gap, ref["seen"]["vtot_min"], ref["seen"]["finite"], ok
