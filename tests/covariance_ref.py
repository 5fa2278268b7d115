"""numpy float64 restatement of maria_amd.covariance: the rounded z of mrx_tod_gram, its exact sums and its
error bound, the quotients built on G and n, the leading modes, the score and the mode-removal pipeline."""

import numpy as np


def z_of(x, model=None, flags=None, center=None):
    """[D, T] float32: z(d, t) = float32(float64(x) - float64(model) - center[d]) where the flag is 0, else 0.  Two
    float64 subtractions in the header's order, one rounding to float32."""
    term = x.astype(np.float64)
    if model is not None:
        term = term - model.astype(np.float64)
    if center is not None:
        term = term - np.asarray(center, np.float64)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        z = term.astype(np.float32)
    if flags is not None:
        z = np.where(flags != 0, np.float32(0), z)
    return z


def take_rows(a, rows):
    """The rows of ``a`` [D, T] that ``rows`` names, zeros for an entry outside 0 .. D - 1; None: all of them."""
    if rows is None:
        return a
    rows = np.asarray(rows, np.int64)
    ok = (rows >= 0) & (rows < a.shape[0])
    out = np.zeros((rows.size, a.shape[1]), a.dtype)
    out[ok] = a[rows[ok]]
    return out


def gram_exact_int(z, rows=None):
    """G of an integer-valued z as an int64 product: exact."""
    zi = take_rows(z, rows).astype(np.int64)
    return zi @ zi.T


def gram(z, rows=None):
    """``(G, A)`` in float64: the sums of z_i z_j and of |z_i z_j| over time."""
    zr = take_rows(z, rows).astype(np.float64)
    return zr @ zr.T, np.abs(zr) @ np.abs(zr).T


def counts(flags, D, T, rows=None):
    """n[i, j]: the samples both rows keep (T without flags), 0 for a row outside 0 .. D - 1."""
    w = np.ones((D, T), np.int64) if flags is None else (flags == 0).astype(np.int64)
    w = take_rows(w, rows)
    return w @ w.T


def bound(A, T, block):
    """The header's first-order bound on |G - exact|, per element: (block 2^-24 + ceil(T / block) 2^-53) A."""
    return (block * 2.0**-24 + -(-T // block) * 2.0**-53) * A


def finish_group(G, n, min_hits):
    """``(cov, corr, valid, unusable)`` of covariance.finish_group."""
    floor = max(int(min_hits), 1)
    valid = n >= floor
    cov = np.where(valid, G / np.where(valid, n, 1), 0.0)
    dG, dn = np.diag(G), np.diag(n)
    unusable = (dn < floor) | (dG == 0) | ~np.isfinite(dG)
    var = np.where(unusable, 1.0, np.diag(cov))
    both = valid & ~unusable[:, None] & ~unusable[None, :]
    corr = np.where(both, cov / np.sqrt(var[:, None] * var[None, :]), 0.0)
    return cov, corr, valid, unusable


def leading_modes(corr, unusable, k):
    keep = np.flatnonzero(~unusable)
    w, V = np.linalg.eigh(corr[np.ix_(keep, keep)])
    w, V = w[::-1][:k], V[:, ::-1][:, :k]
    V = np.where(V.sum(axis=0) < 0, -V, V)
    U = np.zeros((corr.shape[0], k))
    U[keep] = V
    return w, U


def correlation_score(corr, valid, unusable):
    R = corr.shape[0]
    out = np.full(R, np.nan)
    for i in range(R):
        if unusable[i]:
            continue
        js = [j for j in range(R) if j != i and not unusable[j] and valid[i, j]]
        if js:
            out[i] = np.median(corr[i, js])
    return out


def row_means(x, model=None, flags=None):
    """(mean [D], hits [D]) over the kept samples, float64; 0 where nothing is kept."""
    term = x.astype(np.float64) - (0.0 if model is None else model.astype(np.float64))
    keep = np.ones(x.shape, bool) if flags is None else flags == 0
    hits = keep.sum(axis=1)
    mean = np.where(hits > 0, np.where(keep, term, 0.0).sum(axis=1) / np.maximum(hits, 1), 0.0)
    return mean, hits


def covariance_group(x, rows, model=None, flags=None, min_hits=8):
    """The float64 reference of one group from the data alone: (G, n, cov, corr, valid, unusable, mean)."""
    mean, _ = row_means(x, model, flags)
    z = z_of(x, model, flags, mean)
    G, _ = gram(z, rows)
    n = counts(flags, x.shape[0], x.shape[1], rows)
    return (G, n, *finish_group(G, n, min_hits), mean)


def gram_of_data(x, flags):
    """``gram_of`` for ``remove_modes`` from the data alone, in float64."""
    def gram_of(g, rows, mean):
        G, _ = gram(z_of(x, None, flags, mean), rows)
        return G, counts(flags, x.shape[0], x.shape[1], rows)

    return gram_of


def remove_modes(x, flags, groups, n_groups, gram_of, n_modes, min_hits=8, rcond=1e-10, remove_mean=False):
    """TOD.remove_modes step for step: ``(y float32 [D, T], B float32 [G, 1 + n_modes, T], a [D, K], eigenvalues [G, n_modes],
    U [D, n_modes])``.  ``gram_of(g, rows, mean)`` gives a group's (G, n): the device's own, or ``gram_of_data``.  Everything
    after G is tests/regress_ref.py, which restates the kernels (a template sample and the subtracted combination are
    rounded to float32 where the device rounds them)."""
    import regress_ref as rr

    D, T = x.shape
    mean, _ = row_means(x, None, flags)
    U, sigma, eig = np.zeros((D, n_modes)), np.zeros(D), np.zeros((n_groups, n_modes))
    for g in range(n_groups):
        rows = np.flatnonzero(groups == g)
        G, n = gram_of(g, rows, mean)
        cov, corr, _, unusable = finish_group(G, n, min_hits)
        eig[g], U[rows] = leading_modes(corr, unusable, n_modes)
        sigma[rows] = np.where(unusable, 0.0, np.sqrt(np.diag(cov)))
    live = sigma > 0
    inv = np.where(live, 1.0 / np.where(live, sigma, 1.0), 0.0)
    B = np.ones((n_groups, 1 + n_modes, T), np.float32)
    for k in range(n_modes):
        _, _, B[:, 1 + k, :], _ = rr.column_mean(x, U[:, k] * inv, np.where(live, U[:, k] * U[:, k], 0.0), off=mean, groups=groups,
                                                 n_groups=n_groups, flags=flags)
    N, r, hits, _, _ = rr.normal_equations(x, B, groups=groups, flags=flags)
    a, _ = rr.solve(N, r, hits, min_hits=min_hits, rcond=rcond)
    sub = a.copy()
    if not remove_mean:
        sub[:, 0] = 0.0
    return rr.apply(x, B, sub, groups=groups, sign=-1), B, a, eig, U


def judge(score, groups, usable, n_sigma=5.0, min_correlation=None):
    """(cut [D] bool, median [G], threshold [G]) of covariance.judge from the scores."""
    D = score.shape[0]
    n_g = int(groups.max()) + 1
    cut = np.zeros(D, bool)
    median, threshold = np.full(n_g, np.nan), np.full(n_g, np.nan)
    for g in range(n_g):
        rows = np.flatnonzero(groups == g)
        ok = usable[rows] & np.isfinite(score[rows])
        cut[rows[~ok]] = True
        if ok.any():
            v = score[rows[ok]]
            median[g] = np.median(v)
            scale = 1.4826 * np.median(np.abs(v - median[g]))
            threshold[g] = median[g] - n_sigma * scale
            cut[rows[ok]] = (scale > 0) & (median[g] - v > n_sigma * scale)
            if min_correlation is not None:
                cut[rows[ok]] |= v < min_correlation
    return cut, median, threshold
