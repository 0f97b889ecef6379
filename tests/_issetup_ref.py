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


def proposal_lpdf(Xa, vp, X, Nvp, Nbox):
    """the proposal's log density (:301-340), the box terms counted: the two-term log-sum-exp of :335-337"""
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
        return np.where(np.isfinite(hi), hi + np.log1p(np.exp(lo - hi)), -np.inf)


def weights(lpdf, fmu, fs2):
    """lnw (Na1 x S; :337, :148) and the resampling log weight lnw + islogf2 (:207)"""
    with np.errstate(invalid="ignore"):
        lnw = np.where(np.isfinite(lpdf)[:, None], fmu - lpdf[:, None], -np.inf)
    lnw = np.where(np.isfinite(lnw), lnw, -np.inf)
    fs = np.sqrt(np.maximum(fs2, np.finfo(np.float64).tiny))
    lw = lnw + (U_IQR * fs + np.log1p(-np.exp(-2 * U_IQR * fs)))
    return lnw, np.where(np.isfinite(lw), lw, -np.inf)


def resample(lw, u, W):
    """W draws without replacement from exp(lw - max lw) by catrnd's rule idx = #(cdf < u cdf(end)) (:208-214, :403-408); weights that
    ran out are reset to ones.  Returns the indices and the smallest |u total - cdf entry| / total over the draws."""
    m = np.max(lw)
    w = np.ones_like(lw) if not np.isfinite(m) else np.exp(lw - m)
    idx, margin = [], np.inf
    for i in range(W):
        if not np.sum(w) > 0:
            w = np.ones_like(lw)
        cdf = np.cumsum(w)
        t = u[i] * cdf[-1]
        margin = min(margin, float(np.min(np.abs(cdf - t))) / cdf[-1])
        k = min(int(np.sum(cdf < t)), lw.size - 1)
        idx.append(k)
        w[k] = 0.0
    return np.array(idx), margin


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
    lpdf = proposal_lpdf(Xa1, vp, X, Nvp, Nbox)
    lnw, lw = weights(lpdf, fmu, fs2)
    out = {"Xa1": Xa1, "lpdf1": lpdf, "lnw1": lnw.T.copy(), "fs2a1": fs2, "fmu1": fmu, "rect_delta": rd, "LB": LB, "UB": UB, "margin": np.inf}
    if W > 0:
        idx0 = np.zeros((W, S), dtype=int)
        x0 = np.zeros((S, W, D))
        for s in range(S):
            idx0[:, s], mg = resample(lw[:, s], B[(D + 1) * Na1 + W * s:(D + 1) * Na1 + W * (s + 1)], W)
            out["margin"] = min(out["margin"], mg)
            x0[s] = np.clip(Xa1[idx0[:, s]], LB, UB)
        out.update(idx0=idx0, x0=x0)
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


def build_case(name):
    from tests._cases import synth_problem
    from tests._issample_ref import SLOTS, halfmoves_needed

    D, N, S, K, Nvp, Nbox, Nm, meanfun, seed = CASES[name]
    p = synth_problem(seed, D, N, K, S, meanfun=meanfun)
    hyp = p["hyp"].copy()
    hyp[D + 1, :] = math.log(0.03)
    hyp[D + 1, S // 2] = math.log(3e-4)                # the middle hyper-sample on the Lchol = false branch (tests/_quad_ref.py::mixed_gp)
    hyp[:D, S // 2] += math.log(0.25)
    X = p["X"]
    diam = np.max(X, axis=0) - np.min(X, axis=0)
    if name == "Z":                                    # hyper-sample 1: sf2 = e^10, length scales 0.12 diam -- see below
        hyp[:D, 1] = np.log(0.12 * diam)
        hyp[D, 1] = 5.0
    gp = R.gplite_post(hyp, X, p["y"], meanfun=meanfun, noisefun=p["noisefun"], s2=p["s2"])
    rng = np.random.default_rng(seed + 1700)
    best = X[np.argsort(-gp["y"], kind="stable")[: max(K, N // 2)]]
    vp = {"D": D, "K": K, "mu": best[rng.permutation(best.shape[0])[:K]].T.copy(), "sigma": 0.3 * np.exp(0.3 * rng.standard_normal(K)),
          "lambda": np.std(X, axis=0, ddof=1) * np.exp(0.1 * rng.standard_normal(D)), "w": rng.dirichlet(np.ones(K))}
    W = 2 * (D + 1)
    Na1 = Nvp + Nbox
    B = np.minimum(np.maximum(rng.random(block_len(D, S, W, Nvp, Nbox)), 2.0 ** -53), 1.0 - 2.0 ** -53)
    for i in range(Nvp):
        B[(D + 1) * i + 1:(D + 1) * (i + 1)] = rng.standard_normal(D)
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
    return {"name": name, "gp": gp, "vp": vp, "B": B, "U": U, "D": D, "N": N, "S": S, "K": K, "Nvp": Nvp, "Nbox": Nbox, "Na1": Na1, "W": W,
            "Nm": Nm, "planted": planted}


_RUNS = {}


def run_case(name):
    """the case and the restatement's answer on the oracle's prediction, computed once per process and left unchanged"""
    if name not in _RUNS:
        c = build_case(name)
        _RUNS[name] = (c, setup(c["B"], c["vp"], c["gp"], c["Nvp"], c["Nbox"], c["W"]))
    return _RUNS[name]
