"""The numpy float64 reference of maria_amd.subscans: the basis, the two formulas of include/mrx.h with their
operation order, ``solve`` (regress_ref's) and the front end's steps, plain and slow.  Sums are ``math.fsum`` over the
rounded products: the correctly rounded sum, whatever order the device adds in."""

import math

import numpy as np
import regress_ref


def segments(bounds, T):
    """[(lo, hi)] of every segment, clamped to 0 .. T; hi <= lo: empty."""
    b = np.clip(np.asarray(bounds, np.int64), 0, T)
    return [(int(lo), int(hi)) for lo, hi in zip(b[:-1], b[1:])]


def basis(L, K):
    """[K, L] float64: P_0 .. P_{K - 1} on the L samples of a segment, operation for operation as in include/mrx.h."""
    k = np.arange(L, dtype=np.int64)
    u = (2 * k - (L - 1)).astype(np.float64) / np.float64(L - 1) if L > 1 else np.zeros(L)
    P = np.empty((K, L))
    P[0] = 1.0
    if K > 1:
        P[1] = u
    for n in range(1, K - 1):
        c = 1.0 / float(n + 1)
        P[n + 1] = (((float(2 * n + 1) * u) * P[n]) - (float(n) * P[n - 1])) * c
    return P


def _terms(x, model):
    t = np.asarray(x, np.float32).astype(np.float64)
    return t if model is None else t - np.asarray(model, np.float32).astype(np.float64)


def normal_equations(x, bounds, K, flags=None, model=None):
    """(N [D, S, K, K], r [D, S, K], hits [D, S] int64, absN, absr): fsum of the rounded products over the kept samples,
    and the sums of the products' magnitudes (for rounding bounds)."""
    terms = _terms(x, model)
    D, T = terms.shape
    segs = segments(bounds, T)
    S = len(segs)
    N, r, hits = np.zeros((D, S, K, K)), np.zeros((D, S, K)), np.zeros((D, S), np.int64)
    aN, ar = np.zeros((D, S, K, K)), np.zeros((D, S, K))
    for s, (lo, hi) in enumerate(segs):
        if hi <= lo:
            continue
        P = basis(hi - lo, K)
        for d in range(D):
            keep = np.ones(hi - lo, bool) if flags is None else np.asarray(flags)[d, lo:hi] == 0
            b, y = P[:, keep], terms[d, lo:hi][keep]
            for i in range(K):
                for j in range(i, K):
                    p = b[i] * b[j]
                    N[d, s, i, j] = N[d, s, j, i] = math.fsum(p)
                    aN[d, s, i, j] = aN[d, s, j, i] = math.fsum(np.abs(p))
                p = b[i] * y
                r[d, s, i], ar[d, s, i] = math.fsum(p), math.fsum(np.abs(p))
            hits[d, s] = int(keep.sum())
    return N, r, hits, aN, ar


def fit_values(bounds, a, T):
    """[D, T] float64: s = ((0 + a_0 P_0) + a_1 P_1) + .. of every sample's segment; 0 in no segment."""
    a = np.asarray(a, np.float64)
    D, S, K = a.shape
    out = np.zeros((D, T))
    for s, (lo, hi) in enumerate(segments(bounds, T)):
        if hi <= lo:
            continue
        P = basis(hi - lo, K)
        acc = np.zeros((D, hi - lo))
        for i in range(K):
            acc = acc + a[:, s, i, None] * P[i][None, :]
        out[:, lo:hi] = acc
    return out


def apply(x, bounds, a, sign=-1):
    """y = x + sign * float32(s) inside the segments, x elsewhere."""
    x = np.asarray(x, np.float32)
    D, T = x.shape
    f = fit_values(bounds, a, T).astype(np.float32)
    covered = np.zeros(T, bool)
    for lo, hi in segments(bounds, T):
        covered[lo:hi] = True
    y = np.where(covered[None, :], x - f if sign < 0 else x + f, x)
    return y.astype(np.float32)


def fit(x, bounds, K, flags=None, model=None, min_hits=8, rcond=1e-10):
    """(a [D, S, K], ok [D, S]): regress_ref.solve of every (row, segment)."""
    N, r, hits, _, _ = normal_equations(x, bounds, K, flags=flags, model=model)
    D, S = hits.shape
    a, ok = regress_ref.solve(N.reshape(D * S, K, K), r.reshape(D * S, K), hits.reshape(D * S), min_hits=min_hits, rcond=rcond)
    return a.reshape(D, S, K), ok.reshape(D, S)


def filter_subscans(signal, into, bounds, turn, order, flags=None, model=None, min_hits=8, rcond=1e-10, flag_turnarounds=True,
                    flag_failed=True):
    """(y, flags_out, a, ok): TOD.filter_subscans on the host: the fit on ``signal`` less ``model`` over the samples with
    neither a flag nor a turnaround, subtracted from ``into``."""
    D, T = np.shape(signal)
    old = np.zeros((D, T), np.uint8) if flags is None else np.asarray(flags, np.uint8)
    used = old | np.asarray(turn, np.uint8)[None, :]
    a, ok = fit(signal, bounds, order + 1, flags=used, model=model, min_hits=min_hits, rcond=rcond)
    y = apply(into, bounds, a, sign=-1)
    out = used.copy() if flag_turnarounds else old.copy()
    if flag_failed:
        for s, (lo, hi) in enumerate(segments(bounds, T)):
            out[~ok[:, s], lo:hi] |= 1
    return y, out, a, ok
