"""The numpy float64 reference of maria_amd.regress: the three formulas of include/mrx.h, ``solve`` and
``fit_common_mode``, plain and slow; the reductions also as double loops."""

import numpy as np


def _terms(x, model):
    t = np.asarray(x, np.float32).astype(np.float64)
    return t if model is None else t - np.asarray(model, np.float32).astype(np.float64)


def _groups(groups, D):
    return np.zeros(D, np.int64) if groups is None else np.asarray(groups, np.int64)


def column_mean(x, u, v, off=None, groups=None, n_groups=1, flags=None, model=None):
    """(S float64, W float64, mean float32, absS float64), each [G, T]: over the rows d of group g with flags[d, t] == 0,
    in ascending d, the sums of u[d] * (term - off[d]) and of v[d], float32(S / W) where W > 0 (else 0), and the sum of
    the magnitudes of S's terms (for rounding bounds)."""
    terms = _terms(x, model)
    D, T = terms.shape
    groups = _groups(groups, D)
    off = np.zeros(D) if off is None else np.asarray(off, np.float64)
    S, W, A = np.zeros((n_groups, T)), np.zeros((n_groups, T)), np.zeros((n_groups, T))
    for d in range(D):
        g = groups[d]
        if g < 0 or g >= n_groups:
            continue
        keep = np.ones(T, bool) if flags is None else np.asarray(flags)[d] == 0
        val = u[d] * (terms[d] - off[d])
        S[g, keep] += val[keep]
        A[g, keep] += np.abs(val[keep])
        W[g, keep] += v[d]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(W > 0, S / np.where(W > 0, W, 1.0), 0.0).astype(np.float32)
    return S, W, mean, A


def column_mean_by_loops(x, u, v, off=None, groups=None, n_groups=1, flags=None, model=None):
    """(S, W, mean) again, by a double loop over samples and rows."""
    D, T = np.shape(x)
    S, W, mean = np.zeros((n_groups, T)), np.zeros((n_groups, T)), np.zeros((n_groups, T), np.float32)
    for t in range(T):
        for d in range(D):
            g = 0 if groups is None else int(groups[d])
            if g < 0 or g >= n_groups or (flags is not None and flags[d][t] != 0):
                continue
            term = float(np.float32(x[d][t]))
            if model is not None:
                term = term - float(np.float32(model[d][t]))
            S[g, t] += float(u[d]) * (term - (0.0 if off is None else float(off[d])))
            W[g, t] += float(v[d])
        for g in range(n_groups):
            if W[g, t] > 0:
                mean[g, t] = np.float32(S[g, t] / W[g, t])
    return S, W, mean


def normal_equations(x, B, groups=None, flags=None, model=None):
    """(N [D, K, K], r [D, K], hits [D] int64, absN, absr): each row against the templates B[g] of its group over its
    unflagged samples, with the sums of the terms' magnitudes; zeros for a row outside every group."""
    terms = _terms(x, model)
    D, T = terms.shape
    B = np.asarray(B, np.float32).astype(np.float64)
    G, K, _ = B.shape
    groups = _groups(groups, D)
    N, r, hits = np.zeros((D, K, K)), np.zeros((D, K)), np.zeros(D, np.int64)
    aN, ar = np.zeros((D, K, K)), np.zeros((D, K))
    for d in range(D):
        g = groups[d]
        if g < 0 or g >= G:
            continue
        keep = np.ones(T, bool) if flags is None else np.asarray(flags)[d] == 0
        b, y = B[g][:, keep], terms[d, keep]
        for i in range(K):
            for j in range(K):
                p = b[i] * b[j]
                N[d, i, j], aN[d, i, j] = p.sum(), np.abs(p).sum()
            p = b[i] * y
            r[d, i], ar[d, i] = p.sum(), np.abs(p).sum()
        hits[d] = int(keep.sum())
    return N, r, hits, aN, ar


def normal_equations_by_loops(x, B, groups=None, flags=None, model=None):
    """(N, r, hits) again, sample by sample."""
    D, T = np.shape(x)
    G, K = len(B), len(B[0])
    N, r, hits = np.zeros((D, K, K)), np.zeros((D, K)), np.zeros(D, np.int64)
    for d in range(D):
        g = 0 if groups is None else int(groups[d])
        if g < 0 or g >= G:
            continue
        for t in range(T):
            if flags is not None and flags[d][t] != 0:
                continue
            term = float(np.float32(x[d][t]))
            if model is not None:
                term = term - float(np.float32(model[d][t]))
            for i in range(K):
                bi = float(np.float32(B[g][i][t]))
                for j in range(K):
                    N[d, i, j] += bi * float(np.float32(B[g][j][t]))
                r[d, i] += bi * term
            hits[d] += 1
    return N, r, hits


def apply(x, B, a, groups=None, sign=-1):
    """y = x + sign * float32(s), s = ((0 + a_0 B_0) + a_1 B_1) + .. in float64; rows outside every group copied."""
    x = np.asarray(x, np.float32)
    B = np.asarray(B, np.float32).astype(np.float64)
    D, T = x.shape
    G, K, _ = B.shape
    groups = _groups(groups, D)
    y = x.copy()
    for d in range(D):
        g = groups[d]
        if g < 0 or g >= G:
            continue
        s = np.zeros(T)
        for i in range(K):
            s = s + a[d, i] * B[g, i]
        f = s.astype(np.float32)
        y[d] = x[d] - f if sign < 0 else x[d] + f
    return y


def solve(N, r, hits, min_hits=8, rcond=1e-10):
    """(a [D, K], ok [D]): row by row, N scaled by its diagonal to M, numpy's Cholesky factor L of M, two triangular
    solves; not ok (a = 0) with hits < max(min_hits, K), a diagonal entry not > 0, a failed factorisation or
    min L_ii^2 < rcond."""
    N, r = np.asarray(N, np.float64), np.asarray(r, np.float64)
    D, K = r.shape
    a, ok = np.zeros((D, K)), np.zeros(D, bool)
    for d in range(D):
        diag = np.diagonal(N[d])
        if hits[d] < max(int(min_hits), K) or not np.all(diag > 0):
            continue
        s = 1.0 / np.sqrt(diag)
        M = (N[d] * s[:, None]) * s[None, :]
        try:
            L = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            continue
        if not (np.diagonal(L) ** 2).min() >= rcond:
            continue
        z = np.linalg.solve(L, r[d] * s)
        a[d], ok[d] = np.linalg.solve(L.T, z) * s, True
    return a, ok


def fit_common_mode(x, groups=None, n_groups=1, flags=None, model=None, extra=None, n_iter=3, min_hits=8, rcond=1e-10):
    """(c [G, T] float32, a [D, K], gains [D], ok [D], B [G, K, T] float32): maria_amd.regress.fit_common_mode step for
    step, c rounded to float32 where the front end rounds it."""
    x = np.asarray(x, np.float32)
    D, T = x.shape
    G = n_groups
    gr = _groups(groups, D)
    grouped = (gr >= 0) & (gr < G)
    Ke = 0 if extra is None else len(extra)
    B = np.ones((G, 2 + Ke, T), np.float32)
    if Ke:
        B[:, 2:, :] = np.asarray(extra, np.float32)[None]
    _, r, hits, _, _ = normal_equations(x, B[:, :1, :], groups=groups, flags=flags, model=model)
    fit = hits >= max(int(min_hits), 1)
    o = np.where(fit, r[:, 0] / np.where(fit, hits, 1), 0.0)
    w = (grouped & fit).astype(np.float64)
    g = np.ones(D)
    for _ in range(n_iter):
        _, _, c, _ = column_mean(x, w * g, (w * g) * g, off=o, groups=groups, n_groups=G, flags=flags, model=model)
        B[:, 1, :] = c
        N, r, hits, _, _ = normal_equations(x, B, groups=groups, flags=flags, model=model)
        a, ok = solve(N, r, hits, min_hits=min_hits, rcond=rcond)
        o = a[:, 0].copy()
        w = np.where(ok, w, 0.0)
        s = np.ones(G)
        for k in range(G):
            rows = grouped & (gr == k)
            den = w[rows].sum()
            if den > 0 and (w[rows] * a[rows, 1]).sum() / den != 0:
                s[k] = (w[rows] * a[rows, 1]).sum() / den
        g = a[:, 1] / s[np.where(grouped, gr, 0)]
    return c, a, g, ok, B
