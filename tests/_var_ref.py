"""Extended-precision restatement of the Bayesian-quadrature variance of the expected log joint (test infrastructure).

``var_ld(gp, vp, compute_var, grad_flags, jacobian_flag)`` restates misc/gplogjoint.m:273-413 (and, for the averaged gradient of the
variance, the expected log joint and its gradient, :160-270, :352-373) in ``numpy.longdouble`` (64-bit mantissa) from the gp dict's own
float64 ``X``, ``hyp``, ``alpha``, ``L``, ``sW``, ``sn2_mult`` and from the vp's float64 ``mu``, ``sigma``, ``lambda``, ``w``, ``eta``
and ``delta``: plain coordinate differences, ``exp``, forward substitution row by row (tests/_pred_ref._fwd) for the Cholesky samples
and the stored -inv(K + sn2 I) for the low-noise ones.  The reference's clamps are applied: max(eps, J_kk) inside varF, max(varF, eps).

Beside each value stands the magnitude that was added up to form it; the error measures are |got - ref| / (u magnitude) per entry,
worst over the array, u = 2^-53, with no floor and no other entry's size in the scale:
    J_jk           nf_jk + sum_n |V_jn V_kn| / sn2_eff           (low-noise sample: nf_jk + |z_j|' |L| |z_k|)
    varF_s, varG   the same pushed through w_j w_k; the between-sample term adds 2 |F_s - Fbar| (|F|_s + |F|bar) / (S - 1) + varFss
    varGss         varFss's part of that, and for std(varF_s): sum_s |v_s - vbar| (|v|_s + |v|bar) / ((S - 1) std) + std
    dvarF          entry by entry the absolute values of the terms :286-303 add, through the Jacobians (:375-396; both sides of the
                   softmax Jacobian diag(w) - w w'), and for the averaged form (:407-409) |F|_s |dF|_s and |F|bar |dF|_s as well
where |F|, |dF| are the magnitudes of the expected log joint and of its gradient formed in the same way."""
from collections import namedtuple

import numpy as np

from tests._pred_ref import EPS, LD, U, _fwd, _ld

# per hyper-sample: J, Jmag, nf (S x K x K; compute_var = 2: the diagonal alone, zeros elsewhere), varF_s / varF_mag (S), F_s / F_mag (S),
# dvarF_s / dvarF_s_mag (T x S), the data and prior parts of dvarF_s before the Jacobians (T x S; dv_data, dv_prior), ops: per sample
# (A, B, scale) with J = nf - scale A' B (N x K operands: what a Gram tile multiplies).  Averaged: varG, varG_mag, varGss, varGss_mag,
# dvarF, dvarF_mag (T).  J_lsens, dv_lsens: see var_ld's ``lsens``.
VarLD = namedtuple("VarLD", "J Jmag nf varF_s varF_mag F_s F_mag dvarF_s dvarF_s_mag dv_data dv_prior ops varG varG_mag varGss varGss_mag "
                            "dvarF dvarF_mag sizes J_lsens dv_lsens")


def vp_of_theta(vp, theta):
    """negelcbo_vbmc.m:33-48 in float64 (what the oracle does, oracle/vbmc_ref.negelcbo_vbmc): the vp a column of theta stands for"""
    vp = dict(vp)
    D, K = int(vp["D"]), int(vp["K"])
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    i = 0
    if vp["optimize_mu"]:
        vp["mu"] = theta[:D * K].reshape(D, K, order="F").copy()
        i = D * K
    if vp["optimize_sigma"]:
        vp["sigma"] = np.exp(theta[i:i + K])
        i += K
    if vp["optimize_lambda"]:
        vp["lambda"] = np.exp(theta[i:i + D])
    if vp["optimize_weights"]:
        vp["eta"] = theta[-K:].copy()
        e = np.exp(vp["eta"])
        vp["w"] = e / np.sum(e)
    return vp


def block_sizes(D, K, flags):
    return [D * K if flags[0] else 0, K if flags[1] else 0, D if flags[2] else 0, K if flags[3] else 0]


def _softmax_jac_ld(eta):
    """gplogjoint.m:366-368 -> (J_w, |diag part| + |outer part|)"""
    e = np.exp(_ld(eta))
    es = np.sum(e)
    outer, diag = np.outer(e, e / es ** 2), np.diag(e / es)
    return diag - outer, diag + outer


def var_ld(gp, vp, compute_var, grad_flags=(0, 0, 0, 0), jacobian_flag=True, lsens=False):
    """``lsens``: fill J_lsens / dv_lsens, the first-order bounds on the change of J and of dvarF_s under a relative perturbation of the
    entries of the Cholesky factors L (|dV| <= |inv(L')| |L'| |V|, |dX| <= |inv(L)| (|L| |X| + |dV| / sn2_eff)): times u / 2 they are what
    rounding a factor to float64 can move the results by (the goldens were computed from factors of 50 digits and carry the rounded ones)"""
    assert compute_var in (1, 2) and gp["meanfun"] in (0, 1, 4)
    flags = tuple(bool(f) for f in grad_flags)
    vgrad = any(flags)
    assert not (vgrad and compute_var == 1)                                                # :29-32
    X = _ld(gp["X"])
    (N, D), K, S = X.shape, int(vp["K"]), len(gp["post"])
    mu, sigma, lam, w = _ld(vp["mu"]).reshape(D, K), _ld(vp["sigma"]).reshape(K), _ld(vp["lambda"]).reshape(D), _ld(vp["w"]).reshape(K)
    delta = vp.get("delta")
    delta = np.zeros(D, dtype=LD) if delta is None or np.size(delta) == 0 else np.broadcast_to(_ld(delta).reshape(-1), (D,))   # :85-89
    Ncov, Nnoise, quadratic = gp["Ncov"], gp["Nnoise"], gp["meanfun"] == 4
    sizes = block_sizes(D, K, flags)
    T = sum(sizes)
    J, Jmag, nfa = (np.zeros((S, K, K), dtype=LD) for _ in range(3))
    varF, varFm, F, Fm = (np.zeros(S, dtype=LD) for _ in range(4))
    dv, dvm, dvd, dvp, dF, dFm, dvl = (np.zeros((T, S), dtype=LD) for _ in range(7))
    Jl = np.zeros((S, K, K), dtype=LD)
    ops = []
    if flags[3] and jacobian_flag:
        Jw, Jw_abs = _softmax_jac_ld(vp["eta"])
    Xt = mu.T[:, :, None] - X.T[None, :, :]                                                # K x D x N  (:92-95)
    ww, w2 = np.outer(w, w), w ** 2
    for s, post in enumerate(gp["post"]):
        hyp = _ld(post["hyp"])
        ell, ln_sf2, sum_lnell = np.exp(hyp[:D]), 2 * hyp[D], np.sum(hyp[:D])
        m0 = hyp[Ncov + Nnoise] if gp["meanfun"] > 0 else LD(0)
        alpha, L = _ld(post["alpha"]).reshape(-1), _ld(post["L"])
        sn2_eff = np.exp(2 * hyp[Ncov]) * LD(post["sn2_mult"])                             # :160
        tau = np.sqrt(sigma[:, None] ** 2 * lam[None, :] ** 2 + ell[None, :] ** 2 + delta[None, :] ** 2)      # K x D  (:164)
        lnnf = ln_sf2 + sum_lnell - np.sum(np.log(tau), axis=1)                            # :165
        dl = Xt / tau[:, :, None]                                                          # :167
        Z = np.exp(lnnf[:, None] - np.sum(dl ** 2, axis=1) / 2)                            # K x N  (:168)
        # ---- the expected log joint and its gradient, with magnitudes (:169-270)
        I = Z @ alpha + m0
        Im = np.abs(Z) @ np.abs(alpha) + abs(m0)
        if quadratic:
            xm, om = hyp[Ncov + Nnoise + 1:Ncov + Nnoise + 1 + D], np.exp(hyp[Ncov + Nnoise + D + 1:Ncov + Nnoise + 2 * D + 1])
            qt = (mu ** 2 + sigma[None, :] ** 2 * lam[:, None] ** 2 - 2 * mu * xm[:, None] + xm[:, None] ** 2 + delta[:, None] ** 2) / om[:, None] ** 2
            I = I - np.sum(qt, axis=0) / 2                                                 # :172-173
            Im = Im + np.sum((mu ** 2 + sigma[None, :] ** 2 * lam[:, None] ** 2 + 2 * np.abs(mu * xm[:, None]) + xm[:, None] ** 2
                              + delta[:, None] ** 2) / om[:, None] ** 2, axis=0) / 2
        F[s], Fm[s] = np.sum(w * I), np.sum(w * Im)                                        # :203
        # dz / d(mu, sigma, lambda), K x D x N and K x N, and their term-wise absolute versions
        dz_mu = -(dl / tau[:, :, None]) * Z[:, None, :]                                    # :207
        lt2, st2 = (lam[None, :] / tau) ** 2, (sigma[:, None] / tau) ** 2                  # K x D
        dz_sg = np.sum(lt2[:, :, None] * (dl ** 2 - 1), axis=1) * (sigma[:, None] * Z)     # :228
        dz_sg_abs = np.sum(lt2[:, :, None] * (dl ** 2 + 1), axis=1) * (sigma[:, None] * Z)
        dz_lm = st2[:, :, None] * (dl ** 2 - 1) * (lam[None, :, None] * Z[:, None, :])     # :249
        dz_lm_abs = st2[:, :, None] * (dl ** 2 + 1) * (lam[None, :, None] * Z[:, None, :])
        if vgrad:
            aa = np.abs(alpha)
            g_mu, g_mu_m = w[:, None] * (dz_mu @ alpha), w[:, None] * (np.abs(dz_mu) @ aa)                     # K x D  (:208)
            g_sg, g_sg_m = w * (dz_sg @ alpha), w * (dz_sg_abs @ aa)                                           # :229
            g_lm, g_lm_m = np.sum(w[:, None] * (dz_lm @ alpha), axis=0), np.sum(w[:, None] * (dz_lm_abs @ aa), axis=0)   # :250
            if quadratic:
                t = w[:, None] * (mu.T - xm[None, :]) / om[None, :] ** 2                   # :210
                g_mu, g_mu_m = g_mu - t, g_mu_m + w[:, None] * (np.abs(mu.T) + np.abs(xm[None, :])) / om[None, :] ** 2
                t = w * sigma * np.sum(lam ** 2 / om ** 2)                                 # :231
                g_sg, g_sg_m = g_sg - t, g_sg_m + t
                t = np.sum(w[:, None] * sigma[:, None] ** 2 * lam[None, :] / om[None, :] ** 2, axis=0)    # :252
                g_lm, g_lm_m = g_lm - t, g_lm_m + t
            g_w, g_w_m = I, Im                                                             # :270
        # ---- the solves (:277-279, :318-322): J = nf - scale A' B
        if post["Lchol"]:
            V = _fwd(L, Z.T.copy())                                                        # N x K: L' \ z_k
            A, B, scale = V, V, 1 / sn2_eff
            qmag = (np.abs(V).T @ np.abs(V)) * scale
            if lsens:
                Li = np.abs(_fwd(L, np.eye(N, dtype=LD)))                                  # |inv(L')|
                dV = Li @ (np.abs(L).T @ np.abs(V))
                Jl[s] = (dV.T @ np.abs(V) + np.abs(V).T @ dV) * scale
                if compute_var == 2:
                    Jl[s] = np.diag(np.diag(Jl[s]))
        else:
            A, B, scale = -(L @ Z.T), Z.T.copy(), LD(1)                                    # invKzk = -L z_k
            qmag = np.abs(Z) @ (np.abs(L) @ np.abs(Z).T)
        ops.append((A, B, scale))
        if compute_var == 1:
            q = (A.T @ B) * scale
            q = (q + q.T) / 2 if not post["Lchol"] else q
            s2 = sigma[:, None] ** 2 + sigma[None, :] ** 2                                 # K x K
            tjk2 = s2[:, :, None] * lam[None, None, :] ** 2 + ell[None, None, :] ** 2 + 2 * delta[None, None, :] ** 2     # :313
            dmu = mu.T[:, None, :] - mu.T[None, :, :]
            nf = np.exp(ln_sf2 + sum_lnell - np.sum(np.log(tjk2), axis=2) / 2 - np.sum(dmu ** 2 / tjk2, axis=2) / 2)     # :314-317
        else:
            q = np.diag(np.sum(A * B, axis=0) * scale)
            qmag = np.diag(np.diag(qmag))
            tkk2 = 2 * sigma[:, None] ** 2 * lam[None, :] ** 2 + ell[None, :] ** 2 + 2 * delta[None, :] ** 2             # :274
            nfk = np.exp(ln_sf2 + sum_lnell - np.sum(np.log(tkk2), axis=1) / 2)            # :275
            nf = np.diag(nfk)
        J[s], Jmag[s], nfa[s] = nf - q, nf + qmag, nf
        Jc = J[s].copy()
        Jc[np.diag_indices(K)] = np.maximum(LD(EPS), np.diag(Jc))                          # :283, :329
        varF[s] = max(np.sum(ww * Jc), LD(EPS))                                            # :329-332, :350
        varFm[s] = np.sum(ww * Jmag[s])
        # ---- gradient of the diagonal variance (:286-303)
        if vgrad:
            if post["Lchol"]:
                Xs = _fwd_back(L, V) * scale                                               # N x K: invKzk = L \ (L' \ z_k) / sn2_eff
            else:
                Xs = A
            Xa = np.abs(Xs)
            Jd = np.maximum(LD(EPS), np.diag(J[s]))
            lt2k, st2k = lam[None, :] ** 2 / tkk2, sigma[:, None] ** 2 / tkk2              # K x D
            d_mu = np.stack([dz_mu[k] @ Xs[:, k] for k in range(K)])                       # K x D
            d_sg = np.sum(dz_sg * Xs.T, axis=1)
            d_lm = np.stack([dz_lm[k] @ Xs[:, k] for k in range(K)])                       # K x D

            def data_mags(Xa):
                return (np.stack([np.abs(dz_mu[k]) @ Xa[:, k] for k in range(K)]), np.sum(dz_sg_abs * Xa.T, axis=1),
                        np.stack([dz_lm_abs[k] @ Xa[:, k] for k in range(K)]))

            d_mu_m, d_sg_m, d_lm_m = data_mags(Xa)
            lparts = [np.zeros((K, D), dtype=LD), np.zeros(K, dtype=LD), np.zeros(D, dtype=LD), np.zeros(K, dtype=LD)]
            if lsens and post["Lchol"]:
                l_mu, l_sg, l_lm = data_mags(Li.T @ (np.abs(L) @ Xa + dV * scale))
                lparts = [2 * w2[:, None] * l_mu, 2 * w2 * l_sg, 2 * np.sum(w2[:, None] * l_lm, axis=0), 2 * w * np.diag(Jl[s])]
            p_sg = sigma * nfk * np.sum(lt2k, axis=1)                                      # :293
            p_lm = st2k * nfk[:, None] * lam[None, :]                                      # :297  sigma^2 nf lam / tau_kk^2
            parts = {  # name -> (data, prior, magnitude) before the Jacobians
                0: (-2 * w2[:, None] * d_mu, np.zeros((K, D), dtype=LD), 2 * w2[:, None] * d_mu_m),                      # :289
                1: (-2 * w2 * d_sg, -2 * w2 * p_sg, 2 * w2 * (d_sg_m + p_sg)),
                2: (-2 * np.sum(w2[:, None] * d_lm, axis=0), -2 * np.sum(w2[:, None] * p_lm, axis=0),
                    2 * np.sum(w2[:, None] * (d_lm_m + p_lm), axis=0)),
                3: (-2 * w * np.diag(q), 2 * w * nfk, 2 * w * np.diag(Jmag[s])),                                        # :301
            }
            wv = 2 * w * Jd                                                                # :301 with the clamp
            i = 0
            for b in range(4):
                n = sizes[b]
                if not n:
                    continue
                dat, pri, mag = parts[b]
                lse = lparts[b]
                val = wv if b == 3 else dat + pri
                gF, gFm = ((g_mu, g_mu_m), (g_sg, g_sg_m), (g_lm, g_lm_m), (g_w, g_w_m))[b]
                if jacobian_flag:                                                          # :352-373, :375-396
                    if b == 1:
                        val, dat, pri, mag, gF, gFm, lse = (x * sigma for x in (val, dat, pri, mag, gF, gFm, lse))
                    elif b == 2:
                        val, dat, pri, mag, gF, gFm, lse = (x * lam for x in (val, dat, pri, mag, gF, gFm, lse))
                    elif b == 3:
                        val, dat, pri, mag, gF, gFm, lse = Jw @ val, Jw @ dat, Jw @ pri, Jw_abs @ mag, Jw @ gF, Jw_abs @ gFm, Jw_abs @ lse
                dvl[i:i + n, s] = np.asarray(lse).reshape(-1)
                dv[i:i + n, s], dvd[i:i + n, s], dvp[i:i + n, s], dvm[i:i + n, s] = (np.asarray(x).reshape(-1) for x in (val, dat, pri, mag))
                dF[i:i + n, s], dFm[i:i + n, s] = np.asarray(gF).reshape(-1), np.asarray(gFm).reshape(-1)
                i += n
    # ---- averaging over the hyper-samples (:399-413)
    zT = np.zeros(T, dtype=LD)
    if S == 1:
        varG, varGm, varGss, varGssm, dvar, dvarm = varF[0], varFm[0], LD(0), LD(0), dv[:, 0].copy(), dvm[:, 0].copy()
    else:
        Fbar, Fbm = np.sum(F) / S, np.sum(Fm) / S
        vss = np.sum((F - Fbar) ** 2) / (S - 1)                                            # :401
        vssm = np.sum(2 * np.abs(F - Fbar) * (Fm + Fbm)) / (S - 1) + vss
        vbar, vbm = np.sum(varF) / S, np.sum(varFm) / S
        sd = np.sqrt(np.sum((varF - vbar) ** 2) / (S - 1))
        varG, varGm = vbar + vss, vbm + vssm                                               # :405
        varGss = vss + sd                                                                  # :404
        varGssm = vssm + sd + (np.sum(np.abs(varF - vbar) * (varFm + vbm)) / ((S - 1) * sd) if sd > 0 else vbm)
        dvar, dvarm = zT, zT
        if vgrad:                                                                          # :407-409
            dvar = np.sum(dv, axis=1) / S + 2 * np.sum(F[None, :] * dF, axis=1) / (S - 1) - 2 * Fbar * np.sum(dF, axis=1) / (S - 1)
            dvarm = np.sum(dvm, axis=1) / S + 2 * np.sum(Fm[None, :] * dFm, axis=1) / (S - 1) + 2 * Fbm * np.sum(dFm, axis=1) / (S - 1)
    return VarLD(J=J, Jmag=Jmag, nf=nfa, varF_s=varF, varF_mag=varFm, F_s=F, F_mag=Fm, dvarF_s=dv, dvarF_s_mag=dvm, dv_data=dvd, dv_prior=dvp,
                 ops=ops, varG=varG, varG_mag=varGm, varGss=varGss, varGss_mag=varGssm, dvarF=dvar, dvarF_mag=dvarm, sizes=sizes, J_lsens=Jl, dv_lsens=dvl)


def _fwd_back(R, V):
    """R \\ V for an upper-triangular R, row by row from the last"""
    Xo = np.empty_like(V)
    n = V.shape[0]
    for i in range(n - 1, -1, -1):
        Xo[i] = (V[i] - R[i, i + 1:] @ Xo[i + 1:]) / R[i, i]
    return Xo


# ---- error measures --------------------------------------------------------------------------------------------------------------------
TINY = float(np.finfo(np.float64).tiny)    # 2^-1022


def err_units(got, ref, mag, mask=None):
    """worst |got - ref| / (u mag + 2^-1022) over the entries (of ``mask``): an entry's own magnitude alone, and no floor but float64's
    smallest normal number -- nf_jk of two components in different clusters at D = 28 is exp(-800): a number in longdouble, zero in
    float64 for the oracle and the device alike"""
    got, ref, mag = _ld(got).reshape(np.shape(ref)), np.asarray(ref, dtype=LD), np.asarray(mag, dtype=LD)
    if mask is not None:
        got, ref, mag = got[mask], ref[mask], mag[mask]
    if not got.size:
        return 0.0
    assert np.all(mag > 0), "an entry with no magnitude"
    return float(np.max(np.abs(got - ref) / (U * mag + TINY)))


def err_J(got, ref, compute_var):
    """``got``: S x K x K.  compute_var = 2: the diagonal alone (the reference and the device leave the rest zero)"""
    K = ref.J.shape[1]
    mask = np.broadcast_to(np.eye(K, dtype=bool)[None], ref.J.shape) if compute_var == 2 else None
    return err_units(got, ref.J, ref.Jmag, mask)


def err_dvar_blocks(got, ref_val, ref_mag, sizes):
    """-> {block: worst error in the block's own entries' units} for a T-vector or a T x S array"""
    out, i = {}, 0
    got = _ld(got).reshape(np.shape(ref_val))
    for name, n in zip(("mu", "sigma", "lambda", "eta"), sizes):
        if n:
            out[name] = err_units(got[i:i + n], ref_val[i:i + n], ref_mag[i:i + n])
        i += n
    return out


# ---- power -----------------------------------------------------------------------------------------------------------------------------
POWER_TILE = 0.15     # share of the off-diagonal pairs of every 16 x 16 tile of the upper triangle that see the data and the prior term
POWER_VG = 0.9        # share of the entries of every block of dvarF whose data term is >= 1e-3 of its prior term (as _pred_ref.POWER_M)


def tile_power(ref):
    """-> the worst share, over the 16 x 16 tiles (tj <= tk) of every sample, of off-diagonal pairs j < k with
    |q_jk| >= 1e-3 sqrt(q_jj q_kk) (the data term, what the tile's dot product computes) and nf_jk >= 1e-3 sqrt(nf_jj nf_kk);
    1.0 where there is no off-diagonal pair (K = 1)"""
    S, K, _ = ref.J.shape
    worst = 1.0
    for s in range(S):
        q = ref.nf[s] - ref.J[s]
        dq, dn = np.sqrt(np.abs(np.diag(q))), np.sqrt(np.diag(ref.nf[s]))
        ok = (np.abs(q) >= 1e-3 * np.outer(dq, dq)) & (ref.nf[s] >= 1e-3 * np.outer(dn, dn))
        up = np.triu(np.ones((K, K), dtype=bool), 1)
        for tk in range((K + 15) // 16):
            for tj in range(tk + 1):
                sl = (slice(16 * tj, 16 * tj + 16), slice(16 * tk, 16 * tk + 16))
                if up[sl].any():
                    worst = min(worst, float(np.sum(ok[sl] & up[sl]) / np.sum(up[sl])))
    return worst


def diag_floor(ref):
    """min J_kk over samples and components, in units of eps: above 1e3, or the clamp max(eps, J_kk) decides"""
    return float(np.min(np.diagonal(ref.J, axis1=1, axis2=2)) / EPS)


def vg_power(ref):
    """-> {block: share of (entry, sample) with |data term| >= 1e-3 |prior term|} of dvarF_s (the mu block has no prior term: 1.0
    where its data term is nonzero)"""
    out, i = {}, 0
    for name, n in zip(("mu", "sigma", "lambda", "eta"), ref.sizes):
        if n:
            d, p = np.abs(ref.dv_data[i:i + n]), np.abs(ref.dv_prior[i:i + n])
            out[name] = float(np.mean((d >= 1e-3 * p) & (d > 0)))
        i += n
    return out


def assert_power(ref, compute_var, vgrad, what=""):
    assert diag_floor(ref) > 1e3, "%s: a J_kk at the clamp (%.3g eps)" % (what, diag_floor(ref))
    tp = tile_power(ref) if compute_var == 1 else None
    if compute_var == 1:
        assert tp >= POWER_TILE, "%s: a tile of the upper triangle does not see the data: worst share %.3f" % (what, tp)
    vg = vg_power(ref) if vgrad else None
    if vgrad:
        assert min(vg.values()) >= POWER_VG, "%s: a block of dvarF without a data term: %r" % (what, vg)
    return tp, vg
