"""Step 1 of the IMIQR importance sampler and the resampling of its starting walkers as vbmc_acq_is_setup (include/vbmc_hip.h) states
them, restated in NumPy, and the shared case table of tests/test_issetup_restatement.py (CPU) and tests/test_gpu_issetup.py.

The block  B  holds (D + 1) Na1 + W S doubles, Na1 = Nvp + Nbox:
  point i < Nvp         B[(D + 1) i] uniform: the component c of the 4K-component smoothed mixture, c = #(cdf < u cdf[-1]);
                        B[1 + d + (D + 1) i] standard normal z_d:  x_d = mu[d, c mod K] + (lambda_d sigma4_c) z_d
  point Nvp <= i < Na1  B[(D + 1) i] uniform: the training input j = floor(u N);
                        B[1 + d + (D + 1) i] uniform u_d:  x_d = X[j, d] + (2 u_d - 1) rect_delta_d
  draw i of ensemble s  B[(D + 1) Na1 + i + W s] uniform of the i-th draw without replacement
Every operation that decides a point's bits is one rounded NumPy operation, every sum behind one runs in index order.

Cases (D, N, S, K, Nvp, Nbox, Nm, meanfun, seed): the smallest shapes at which each piece can go wrong
  A  D = 2, N = 21, K = 2, both proposals (19 + 18 = 37 points: no multiple of 16), the middle hyper-sample on the Lchol = false branch
  B  D = 3, N = 37, K = 5, boxes alone (Nvp = 0)
  C  D = 3, N = 37, K = 2, the smoothed mixture alone (Nbox = 0)
  D  D = 10, N = 48, K = 18: 4K = 72 components cross a wave
  P  case A with point 0 planted outside every box and more than 40 sigma from every component
  Z  a hyper-sample whose density is -Inf within reach of the training inputs, and six planted points beyond: one of them is clipped
     onto the face of the box next to a training input -- a start of zero density

Edges (EDGES; the same recipe, the knobs y-scale, "no low-noise hyper-sample", "dead hyper-sample", planted box uniforms):
  R     case A with y times 3000: hyper-samples keep ONE positive weight -- the weights run out on the second of the W = 6 draws
  R9    case A with y times 300: weights underflow to exact zeros, at least W stay positive (no run-out)
  L     Na1 = 256: every lane of the resampling wave holds four weights, 16 point tiles; 4K = 64: one component per lane; N = 130: a
        third trip of the box count; box points planted on the first and on the last training input
  RL    case L's shape with y times 1e6: four and one positive weights of 256 -- the reset of all four weights of every lane, draws from
        the reset weights in lanes 16 and above
  W     D = 32, W = 66 (the limits), Na1 = 129, 4K = 68, N = 70; no low-noise hyper-sample
  K     K = 512: 2048 components, 32 per lane
  O     case A with a hyper-sample under which every point has weight zero (alpha = -1e308, sf2 = e^10, length scales one diameter): the
        resampling starts from ones, every start has zero density
  N<n>  N = 7, 16, 128, 129, 256, 257, 1136 (the top of the resident range): the seams of k_is_pred's row blocks and snake order, a Cholesky and a low-noise hyper-sample,
        Step 1 alone (Nm = 0), 48 points = three point tiles
"""
import math

import numpy as np

from oracle import vbmc_ref as R

U_IQR = 0.6745
SCALES = (0.05, 0.2, 1.0)
LOG_DENORM_MIN = math.log(5e-324)
DRAW_MARGIN = 1e-9


def block_len(D, S, W, Nvp, Nbox):
    return (D + 1) * (Nvp + Nbox) + W * S


def geometry(X):
    """rect_delta = 2 std(X), LB / UB = data range -/+ half the diameter (:27-31, :112), the sums in index order"""
    N, D = X.shape
    rd, LB, UB = np.zeros(D), np.zeros(D), np.zeros(D)
    for d in range(D):
        s = 0.0
        for n in range(N):
            s = s + X[n, d]
        mean = s / N
        q = 0.0
        for n in range(N):
            t = X[n, d] - mean
            q = q + t * t
        rd[d] = 2.0 * math.sqrt(q / (N - 1))
        mn, mx = float(np.min(X[:, d])), float(np.max(X[:, d]))
        diam = mx - mn
        LB[d] = mn - 0.5 * diam
        UB[d] = mx + 0.5 * diam
    return rd, LB, UB


def smoothed(vp):
    """vp_is (:116-126): sigma4, w4 and catrnd's cdf of the 4K components"""
    K = int(vp["K"])
    sig = np.asarray(vp["sigma"], dtype=np.float64).reshape(K)
    w = np.asarray(vp["w"], dtype=np.float64).reshape(K)
    sig4 = np.concatenate([sig] + [np.sqrt(sig * sig + c * c) for c in SCALES])
    ws = 0.0
    for c in range(4 * K):
        ws = ws + w[c % K]
    w4 = np.tile(w, 4) / ws
    return sig4, w4, np.cumsum(w4)


def vp_is(vp):
    K = int(vp["K"])
    sig4, w4, _ = smoothed(vp)
    return dict(vp, K=4 * K, w=w4, mu=np.tile(np.asarray(vp["mu"], dtype=np.float64).reshape(-1, K), (1, 4)), sigma=sig4)


def points(B, vp, X, Nvp, Nbox):
    N, D = X.shape
    K = int(vp["K"])
    mu = np.asarray(vp["mu"], dtype=np.float64).reshape(D, K)
    lam = np.asarray(vp["lambda"], dtype=np.float64).reshape(D)
    sig4, _, cdf = smoothed(vp)
    rd, _, _ = geometry(X)
    Xa = np.zeros((Nvp + Nbox, D))
    for i in range(Nvp + Nbox):
        b = B[(D + 1) * i:(D + 1) * (i + 1)]
        if i < Nvp:
            c = min(int(np.sum(cdf < b[0] * cdf[-1])), 4 * K - 1)
            for d in range(D):
                Xa[i, d] = mu[d, c % K] + (lam[d] * sig4[c]) * b[1 + d]
        else:
            j = min(int(math.floor(b[0] * N)), N - 1)
            for d in range(D):
                Xa[i, d] = X[j, d] + (2.0 * b[1 + d] - 1.0) * rd[d]
    return Xa


def mixture_lpdf(vp4, Xa):
    """log vbmc_pdf(vp_is, Xa, 0, 1): a log-sum-exp over the components; -Inf where the density itself is zero (vbmc_pdf.m:71)"""
    D, K = Xa.shape[1], int(vp4["K"])
    mu = np.asarray(vp4["mu"]).reshape(D, K)
    sig, w = np.asarray(vp4["sigma"]).reshape(K), np.asarray(vp4["w"]).reshape(K)
    lam = np.asarray(vp4["lambda"], dtype=np.float64).reshape(D)
    z = (Xa[:, None, :] - mu.T[None, :, :]) / (sig[None, :, None] * lam[None, None, :])
    lp = np.log(w)[None, :] - D * np.log(sig)[None, :] - np.sum(np.log(lam)) - 0.5 * D * math.log(2 * math.pi) - 0.5 * np.sum(z * z, axis=2)
    m = np.max(lp, axis=1)
    out = m + np.log(np.sum(np.exp(lp - m[:, None]), axis=1))
    return np.where(out < LOG_DENORM_MIN, -np.inf, out)


def proposal_lpdf(Xa, vp, X, Nvp, Nbox, terms=False):
    """the proposal's log density (:301-340), the box terms counted: the two-term log-sum-exp of :335-337; ``terms``: (lpdf, t0, t1)"""
    N, D = X.shape
    w_vp = Nvp / (Nvp + Nbox)
    rd, _, _ = geometry(X)
    t0 = np.full(Xa.shape[0], -np.inf)
    t1 = np.full(Xa.shape[0], -np.inf)
    if Nvp > 0:
        t0 = mixture_lpdf(vp_is(vp), Xa) + math.log(w_vp)
    if Nbox > 0:
        VV = 1.0
        for d in range(D):
            VV = VV * (2.0 * rd[d])
        cnt = np.sum(np.all(np.abs(Xa[:, None, :] - X[None, :, :]) < rd[None, None, :], axis=2), axis=1)
        with np.errstate(divide="ignore"):
            t1 = np.log(cnt / VV / N * (1.0 - w_vp))
    hi, lo = np.maximum(t0, t1), np.minimum(t0, t1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(np.isfinite(hi), hi + np.log1p(np.exp(lo - hi)), -np.inf)
    return (out, t0, t1) if terms else out


def proposal_lpdf_longdouble(Xa, vp, X, Nvp, Nbox):
    """proposal_lpdf's formula in np.longdouble from the same float64 inputs (points, mixture, rect_delta): what the float64 restatement and
    the device are both held against where the number of components is beyond the measured range"""
    ld = np.longdouble
    N, D = X.shape
    K = int(vp["K"])
    w_vp = ld(Nvp) / ld(Nvp + Nbox)
    rd, _, _ = geometry(X)
    n = Xa.shape[0]
    ninf = ld(-np.inf)
    t0 = np.full(n, ninf, dtype=ld)
    t1 = np.full(n, ninf, dtype=ld)
    if Nvp > 0:
        sig = np.asarray(vp["sigma"], dtype=np.float64).reshape(K).astype(ld)
        w = np.asarray(vp["w"], dtype=np.float64).reshape(K).astype(ld)
        lam = np.asarray(vp["lambda"], dtype=np.float64).reshape(D).astype(ld)
        mu = np.tile(np.asarray(vp["mu"], dtype=np.float64).reshape(D, K), (1, 4)).astype(ld)
        sig4 = np.concatenate([sig] + [np.sqrt(sig * sig + ld(c) * ld(c)) for c in SCALES])
        w4 = np.tile(w, 4) / (ld(4) * np.sum(w))
        cst = np.log(w4) - D * np.log(sig4) - np.sum(np.log(lam)) - ld(0.5) * D * ld("1.8378770664093454835606594728112353")
        for i in range(n):
            z = (Xa[i].astype(ld)[None, :] - mu.T) / (sig4[:, None] * lam[None, :])
            lp = cst - ld(0.5) * np.sum(z * z, axis=1)
            m = np.max(lp)
            v = m + np.log(np.sum(np.exp(lp - m)))
            t0[i] = v + np.log(w_vp) if v >= ld(LOG_DENORM_MIN) else ninf
    if Nbox > 0:
        VV = ld(1)
        for d in range(D):
            VV = VV * (ld(2) * ld(rd[d]))
        cnt = np.sum(np.all(np.abs(Xa[:, None, :] - X[None, :, :]) < rd[None, None, :], axis=2), axis=1)
        for i in range(n):
            if cnt[i] > 0:
                t1[i] = np.log(ld(int(cnt[i])) / VV / ld(N) * (ld(1) - w_vp))
    hi, lo = np.maximum(t0, t1), np.minimum(t0, t1)
    out = np.full(n, ninf, dtype=ld)
    for i in range(n):
        if np.isfinite(hi[i]):
            out[i] = hi[i] + np.log1p(np.exp(lo[i] - hi[i])) if np.isfinite(lo[i]) else hi[i]
    return out


def gplite_pred_longdouble(gp, P):
    """(fmu, fs2), n x S each: gplite_pred's formulas (gplite_pred.m:73-104, :120) in np.longdouble from the posterior as it stands in
    float64 (hyp, alpha, L, sW) -- the value the float64 oracle and the device both approximate.  The mean function is evaluated by the
    oracle (a constant mean is exact)."""
    ld = np.longdouble
    X = np.asarray(gp["X"], dtype=np.float64)
    N, D = X.shape
    P = np.asarray(P, dtype=np.float64)
    n, S = P.shape[0], len(gp["post"])
    fmu, fs2 = np.zeros((n, S), dtype=ld), np.zeros((n, S), dtype=ld)
    for s, post in enumerate(gp["post"]):
        hyp = np.asarray(post["hyp"], dtype=np.float64)
        ell = np.exp(hyp[:D].astype(ld))
        sf2 = np.exp(ld(2) * ld(hyp[D]))
        mstar = R.gplite_meanfun(hyp[gp["Ncov"] + gp["Nnoise"]:gp["Ncov"] + gp["Nnoise"] + gp["Nmean"]], P, gp["meanfun"])
        d2 = np.zeros((N, n), dtype=ld)
        for d in range(D):
            t = X[:, d].astype(ld)[:, None] / ell[d] - P[:, d].astype(ld)[None, :] / ell[d]
            d2 = d2 + t * t
        Ks = sf2 * np.exp(-d2 / ld(2))
        fmu[:, s] = np.asarray(mstar, dtype=np.float64).reshape(-1).astype(ld) + Ks.T @ np.asarray(post["alpha"], dtype=np.float64).astype(ld)
        L = np.asarray(post["L"], dtype=np.float64).astype(ld)
        if post["Lchol"]:
            Bv = np.asarray(post["sW"], dtype=np.float64).astype(ld)[:, None] * Ks
            Lt = L.T.copy()
            V = np.zeros((N, n), dtype=ld)
            for i in range(N):                         # L' \ (sW .* Ks), forward substitution
                V[i] = (Bv[i] - Lt[i, :i] @ V[:i]) / Lt[i, i]
            fs2[:, s] = sf2 - np.sum(V * V, axis=0)
        else:
            fs2[:, s] = sf2 + np.sum(Ks * (L @ Ks), axis=0)
        fs2[:, s] = np.maximum(fs2[:, s], ld(0))
    return fmu, fs2


def weights(lpdf, fmu, fs2):
    """lnw (Na1 x S; :337, :148) and the resampling log weight lnw + islogf2 (:207)"""
    with np.errstate(invalid="ignore"):
        lnw = np.where(np.isfinite(lpdf)[:, None], fmu - lpdf[:, None], -np.inf)
    lnw = np.where(np.isfinite(lnw), lnw, -np.inf)
    fs = np.sqrt(np.maximum(fs2, np.finfo(np.float64).tiny))
    lw = lnw + (U_IQR * fs + np.log1p(-np.exp(-2 * U_IQR * fs)))
    return lnw, np.where(np.isfinite(lw), lw, -np.inf)


def resample(lw, u, W, info=None):
    """W draws without replacement from exp(lw - max lw) by catrnd's rule idx = #(cdf < u cdf(end)) (:208-214, :403-408); weights that
    ran out are reset to ones.  Returns the indices and the smallest |u total - cdf entry| / total over the draws.  ``info`` (a dict)
    receives npos, the positive weights at the start, zeros, the finite log weights whose weight is exactly zero, resets, the draws
    in front of which the weights were reset to ones (a start from ones counts as a reset in front of draw 0), and edge, the smallest
    distance of a finite lw - max from the underflow edge log(5e-324)."""
    m = np.max(lw)
    start_ones = not np.isfinite(m)
    w = np.ones_like(lw) if start_ones else np.exp(lw - m)
    if info is not None:
        fin = np.isfinite(lw)
        info.update(npos=0 if start_ones else int(np.sum(w > 0)), zeros=0 if start_ones else int(np.sum(fin & (w == 0))),
                    resets=[0] if start_ones else [], edge=np.inf if start_ones else float(np.min(np.abs((lw[fin] - m) - LOG_DENORM_MIN))))
    idx, margin = [], np.inf
    for i in range(W):
        if not np.sum(w) > 0:
            w = np.ones_like(lw)
            if info is not None:
                info["resets"].append(i)
        cdf = np.cumsum(w)
        t = u[i] * cdf[-1]
        margin = min(margin, float(np.min(np.abs(cdf - t))) / cdf[-1])
        k = min(int(np.sum(cdf < t)), lw.size - 1)
        idx.append(k)
        w[k] = 0.0
    return np.array(idx), margin


def components(B, vp, Nvp):
    """the component of the smoothed mixture each of the first Nvp points is drawn from (points' rule)"""
    D, K = int(vp["D"]), int(vp["K"])
    cdf = smoothed(vp)[2]
    return np.array([min(int(np.sum(cdf < B[(D + 1) * i] * cdf[-1])), 4 * K - 1) for i in range(Nvp)], dtype=int)


def box_inputs(B, D, N, Nvp, Nbox):
    """the training input each box point is drawn around (points' rule)"""
    return np.array([min(int(math.floor(B[(D + 1) * (Nvp + i)] * N)), N - 1) for i in range(Nbox)], dtype=int)


def setup(B, vp, gp, Nvp, Nbox, W, pred=None):
    """Step 1 and the resampling from the block.  pred(Xa) -> (fmu, fs2), Na1 x S each: the oracle's gplite_pred by default."""
    X = np.asarray(gp["X"], dtype=np.float64)
    N, D = X.shape
    S = len(gp["post"])
    Na1 = Nvp + Nbox
    if pred is None:
        def pred(P):
            o = R.gplite_pred(gp, P, None, None, True)
            return np.asarray(o[2]).reshape(P.shape[0], S), np.asarray(o[3]).reshape(P.shape[0], S)
    rd, LB, UB = geometry(X)
    Xa1 = points(B, vp, X, Nvp, Nbox)
    fmu, fs2 = pred(Xa1)
    lpdf, t0, t1 = proposal_lpdf(Xa1, vp, X, Nvp, Nbox, terms=True)
    lnw, lw = weights(lpdf, fmu, fs2)
    out = {"Xa1": Xa1, "lpdf1": lpdf, "lnw1": lnw.T.copy(), "fs2a1": fs2, "fmu1": fmu, "rect_delta": rd, "LB": LB, "UB": UB, "margin": np.inf,
           "t0": t0, "t1": t1, "lw": lw}
    if W > 0:
        idx0 = np.zeros((W, S), dtype=int)
        x0 = np.zeros((S, W, D))
        draws = []
        for s in range(S):
            info = {}
            idx0[:, s], mg = resample(lw[:, s], B[(D + 1) * Na1 + W * s:(D + 1) * Na1 + W * (s + 1)], W, info)
            draws.append(info)
            out["margin"] = min(out["margin"], mg)
            x0[s] = np.clip(Xa1[idx0[:, s]], LB, UB)
        out.update(idx0=idx0, x0=x0, draws=draws)
    return out


# name: (D, N, S, K, Nvp, Nbox, Nm, meanfun, seed)
CASES = {
    "A": (2, 21, 3, 2, 19, 18, 8, 0, 1),
    "B": (3, 37, 3, 5, 0, 24, 8, 1, 1),
    "C": (3, 37, 3, 2, 24, 0, 8, 4, 1),
    "D": (10, 48, 3, 18, 19, 18, 8, 0, 1),
    "P": (2, 21, 3, 2, 19, 18, 8, 0, 2),
    "Z": (2, 21, 3, 2, 19, 18, 8, 1, 1),
}

# name: ((D, N, S, K, Nvp, Nbox, Nm, meanfun, seed), knobs).  Knobs: yscale -- y, sf and a constant mean times it; low_noise = False -- no
# hyper-sample on the Lchol = false branch; dead -- the hyper-sample under which every point has weight zero; plant_box -- the first two
# box points are drawn around the last and the first training input
N_SEAMS = (7, 16, 128, 129, 256, 257, 1136)
N_REFUSED = 1137                                       # the first N whose prediction is the slab form: the sampler answers "unsupported"
EDGES = {
    "R": ((2, 21, 3, 2, 19, 18, 8, 0, 1), {"yscale": 3000.0}),
    "R9": ((2, 21, 3, 2, 19, 18, 8, 0, 1), {"yscale": 300.0}),
    "L": ((3, 130, 2, 16, 128, 128, 8, 1, 1), {"plant_box": True}),
    "RL": ((3, 130, 2, 16, 128, 128, 8, 1, 1), {"yscale": 1e6}),
    "W": ((32, 70, 1, 17, 65, 64, 8, 4, 1), {"low_noise": False}),
    "K": ((2, 40, 1, 512, 40, 0, 8, 0, 1), {}),
    "O": ((2, 21, 3, 2, 19, 18, 8, 0, 1), {"dead": 2}),
}
EDGES.update({"N%d" % n: ((3, n, 2, 2, 24, 24, 0, 1, 1), {}) for n in N_SEAMS})
SEAM_NAMES = tuple("N%d" % n for n in N_SEAMS)


def build_case(name):
    from tests._cases import synth_problem
    from tests._issample_ref import SLOTS, halfmoves_needed

    (D, N, S, K, Nvp, Nbox, Nm, meanfun, seed), knobs = (CASES[name], {}) if name in CASES else EDGES[name]
    p = synth_problem(seed, D, N, K, S, meanfun=meanfun)
    hyp = p["hyp"].copy()
    y = p["y"]
    hyp[D + 1, :] = math.log(0.03)
    if knobs.get("low_noise", True):
        hyp[D + 1, S // 2] = math.log(3e-4)            # the middle hyper-sample on the Lchol = false branch (tests/_quad_ref.py::mixed_gp)
        hyp[:D, S // 2] += math.log(0.25)
    if "yscale" in knobs:                              # importance weights spanning yscale times as many nats
        y = y * knobs["yscale"]
        hyp[D, :] += math.log(knobs["yscale"])
        if meanfun >= 1:
            hyp[D + 2, :] *= knobs["yscale"]
    X = p["X"]
    diam = np.max(X, axis=0) - np.min(X, axis=0)
    if name == "Z":                                    # hyper-sample 1: sf2 = e^10, length scales 0.12 diam -- see below
        hyp[:D, 1] = np.log(0.12 * diam)
        hyp[D, 1] = 5.0
    if "dead" in knobs:                                # sf2 = e^10 and length scales of one diameter: with alpha = -1e308 (below) the
        hyp[:D, knobs["dead"]] = np.log(diam)          # prediction is -Inf within 4.3 diameters of a training input -- at every point
        hyp[D, knobs["dead"]] = 5.0
    gp = R.gplite_post(hyp, X, y, meanfun=meanfun, noisefun=p["noisefun"], s2=p["s2"])
    if "dead" in knobs:
        post = [dict(q) for q in gp["post"]]
        post[knobs["dead"]] = dict(post[knobs["dead"]], alpha=np.full_like(post[knobs["dead"]]["alpha"], -1e308))
        gp = dict(gp, post=post)
    rng = np.random.default_rng(seed + 1700)
    best = X[np.argsort(-gp["y"], kind="stable")[: max(K, N // 2)]]
    pick = rng.permutation(best.shape[0])[np.arange(K) % best.shape[0]]          # (K > N: the component means repeat)
    vp = {"D": D, "K": K, "mu": best[pick].T.copy(), "sigma": 0.3 * np.exp(0.3 * rng.standard_normal(K)),
          "lambda": np.std(X, axis=0, ddof=1) * np.exp(0.1 * rng.standard_normal(D)), "w": rng.dirichlet(np.ones(K))}
    W = 2 * (D + 1)
    Na1 = Nvp + Nbox
    B = np.minimum(np.maximum(rng.random(block_len(D, S, W, Nvp, Nbox)), 2.0 ** -53), 1.0 - 2.0 ** -53)
    for i in range(Nvp):
        B[(D + 1) * i + 1:(D + 1) * (i + 1)] = rng.standard_normal(D)
    if knobs.get("plant_box"):                         # floor(u N) = N - 1 at the largest uniform there is, 0 at the smallest
        B[(D + 1) * Nvp] = 1.0 - 2.0 ** -53
        B[(D + 1) * (Nvp + 1)] = 2.0 ** -53
    planted = None
    if name == "P":                                    # 300 widths of the widest component away: outside every box, zero density
        B[1:D + 1] = 300.0
        planted = 0
    if name == "Z":
        # Hyper-sample 1 has alpha = -1e308: fmu = -Inf wherever sum_n k(x, x_n) >= 1.8, i.e. (sf2 = e^10) within 4.3 length scales of a
        # training input -- the face of the box next to the input with the largest first coordinate lies 0.5 / 0.12 = 4.2 length scales
        # from it --, a huge negative number out to 38.9 length scales = 4.7 diameters, and the mean beyond.  Six points are planted
        # beyond that: five on the diagonals (clipped onto corners of the box, 5.9 length scales from everything: finite) and one
        # straight out from that input (clipped onto the face: -Inf).  Every other point has weight zero under hyper-sample 1.
        post = [dict(q) for q in gp["post"]]
        post[1] = dict(post[1], alpha=np.full_like(post[1]["alpha"], -1e308))
        gp = dict(gp, post=post)
        vp["lambda"] = diam.copy()
        vp["sigma"] = np.full(K, 0.5)
        nstar = int(np.argmax(X[:, 0]))
        sig4 = smoothed(vp)[0]
        targets = [X[nstar] + np.array([6.5 * diam[0], 0.0])] + [0.5 * (np.min(X, axis=0) + np.max(X, axis=0)) + 7.5 * diam * np.array(sg)
                                                                 for sg in ((1, 1), (1, -1), (-1, 1), (-1, -1), (1.1, 1.1))]
        cdf = smoothed(vp)[2]
        for i, t in enumerate(targets):
            c = min(int(np.sum(cdf < B[(D + 1) * i] * cdf[-1])), 4 * K - 1)
            B[(D + 1) * i + 1:(D + 1) * (i + 1)] = (t - vp["mu"][:, c % K]) / (vp["lambda"] * sig4[c])
        planted = 0
    H = W // 2
    M = halfmoves_needed(Nm, H, 1)
    U = np.minimum(np.maximum(rng.random((SLOTS, H, S, M + 1)), 2.0 ** -53), 1.0 - 2.0 ** -53)
    if Nm == 0:                                        # Step 1 alone: no draws, no walkers
        B = B[:(D + 1) * Na1].copy()
        W = 0
    return {"name": name, "gp": gp, "vp": vp, "B": B, "U": U, "D": D, "N": N, "S": S, "K": K, "Nvp": Nvp, "Nbox": Nbox, "Na1": Na1, "W": W,
            "Nm": Nm, "planted": planted}


_RUNS = {}


def run_case(name):
    """the case and the restatement's answer on the oracle's prediction, computed once per process and left unchanged"""
    if name not in _RUNS:
        c = build_case(name)
        _RUNS[name] = (c, setup(c["B"], c["vp"], c["gp"], c["Nvp"], c["Nbox"], c["W"]))
    return _RUNS[name]
