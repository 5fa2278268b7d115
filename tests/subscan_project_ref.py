"""The numpy float64 restatement of the frozen subscan projector (maria_amd.subscans.freeze / project): the
dense F and F^t of a segment, ``freeze`` step for step, and the ordered product A r of mrx_tod_segment_project."""

import numpy as np
import regress_ref
import subscans_ref as ref


def freeze(N, hits, min_hits=8, rcond=1e-10, dtype=np.float64):
    """(A [D, S, K, K], ok [D, S] uint8): ok as regress_ref.solve's; A = s s^t o M^-1 from the scaled Cholesky factor,
    symmetrised, 0 where the pair is not ok.  ``dtype`` np.longdouble: the same steps in extended precision (the
    yardstick of the float64 ones)."""
    N = np.asarray(N, dtype)
    D, S, K = N.shape[:3]
    A, ok = np.zeros((D, S, K, K), dtype), np.zeros((D, S), np.uint8)
    for d in range(D):
        for s in range(S):
            diag = np.diagonal(N[d, s])
            if hits[d, s] < max(int(min_hits), K) or not np.all(diag > 0):
                continue
            sc = 1.0 / np.sqrt(diag)
            M = (N[d, s] * sc[:, None]) * sc[None, :]
            L = _cholesky(M)
            if L is None or not (np.diagonal(L) ** 2).min() >= rcond:
                continue
            Li = _lower_inverse(L)
            B = ((Li.T @ Li) * sc[:, None]) * sc[None, :]
            A[d, s], ok[d, s] = (B + B.T) * dtype(0.5), 1
    return A, ok


def _cholesky(M):
    """The lower factor by the textbook recurrence in M's own dtype (numpy's LAPACK has no longdouble); None on failure."""
    K = M.shape[0]
    L = np.zeros_like(M)
    for j in range(K):
        p = M[j, j] - np.sum(L[j, :j] ** 2)
        if not p > 0:
            return None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, K):
            L[i, j] = (M[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
    return L


def _lower_inverse(L):
    K = L.shape[0]
    X = np.zeros_like(L)
    for c in range(K):
        for i in range(c, K):
            X[i, c] = ((1.0 if i == c else 0.0) - np.sum(L[i, c:i] * X[c:i, c])) / L[i, i]
    return X


def solve_longdouble(N, r, ok):
    """a [D, S, K] float64: N a = r solved in longdouble (Cholesky of the scaled matrix) where ok, 0 elsewhere."""
    A, _ = freeze(N, np.where(np.asarray(ok) != 0, 2**30, 0), min_hits=0, rcond=0.0, dtype=np.longdouble)
    return np.einsum("dsij,dsj->dsi", A, np.asarray(r, np.longdouble)).astype(np.float64)


def ordered_product(A, r):
    """a [D, S, K]: a_i = s, s = 0.0, s = s + A[i][j] * r[j] for j ascending (two roundings a step)."""
    A, r = np.asarray(A, np.float64), np.asarray(r, np.float64)
    K = r.shape[-1]
    a = np.zeros_like(r)
    for j in range(K):
        a = a + A[..., :, j] * r[..., None, j]
    return a


def dense(L, K, keep, A, transpose=False):
    """[L, L] float64: F = I - T A T^t M, or F^t = I - M T A T^t, of one segment of L samples; ``keep`` [L] bool is M's
    diagonal, A [K, K]."""
    Tm = ref.basis(L, K).T  # [L, K]
    M = np.diag(np.asarray(keep, np.float64))
    F = np.eye(L) - Tm @ np.asarray(A, np.float64) @ Tm.T @ M
    return F.T if transpose else F


def segment_inverse(L, K, keep, min_hits=8, rcond=1e-10, dtype=np.float64):
    """(A [K, K], ok): ``freeze`` of N = T^t M T of one segment, N summed in ``dtype``."""
    P = ref.basis(L, K).astype(dtype)[:, np.asarray(keep, bool)]
    N = P @ P.T
    A, ok = freeze(N[None, None], np.array([[int(np.sum(keep))]]), min_hits=min_hits, rcond=rcond, dtype=dtype)
    return A[0, 0], bool(ok[0, 0])


def project(x, bounds, K, flags=None, transpose=False, min_hits=8, rcond=1e-10, dtype=np.float64):
    """(y [D, T], ok [D, S]): F (or F^t) of every (row, segment) on x in ``dtype`` throughout (no float32 rounding);
    pairs that are not ok and samples in no segment are copied."""
    x = np.asarray(x)
    D, T = x.shape
    y = x.astype(dtype)
    segs = ref.segments(bounds, T)
    ok = np.zeros((D, len(segs)), bool)
    for s, (lo, hi) in enumerate(segs):
        if hi <= lo:
            continue
        L = hi - lo
        P = ref.basis(L, K).astype(dtype)
        for d in range(D):
            keep = np.ones(L, bool) if flags is None else np.asarray(flags)[d, lo:hi] == 0
            A, ok[d, s] = segment_inverse(L, K, keep, min_hits, rcond, dtype)
            if not ok[d, s]:
                continue
            seg = y[d, lo:hi].copy()
            m = keep.astype(dtype)
            if transpose:
                y[d, lo:hi] = seg - m * (P.T @ (A @ (P @ seg)))
            else:
                y[d, lo:hi] = seg - P.T @ (A @ (P @ (m * seg)))
    return y, ok


class Frozen:
    """F' of a whole [D, T] TOD in float64, for dense solves: per segment the basis T_s [L, K] and, per row, C = A T^t M
    [K, L]; ``apply`` is x - T (C x), ``apply_transpose`` x - C^t (T^t x).  The pairs of ``unfitted`` (what a mapper
    reported) must be exactly those the reference cannot fit: they are the identity."""

    def __init__(self, D, T, bounds, K, flags=None, unfitted=(), min_hits=8, rcond=1e-10):
        self.parts = []
        mine = set()
        for s, (lo, hi) in enumerate(ref.segments(bounds, T)):
            if hi <= lo:
                continue
            L = hi - lo
            Tm = ref.basis(L, K).T
            C = np.zeros((D, K, L))
            for d in range(D):
                keep = np.ones(L, bool) if flags is None else np.asarray(flags)[d, lo:hi] == 0
                A, ok = segment_inverse(L, K, keep, min_hits, rcond)
                if ok:
                    C[d] = (A @ Tm.T) * keep[None, :]
                else:
                    mine.add((d, s))
            self.parts.append((lo, hi, Tm, C))
        assert mine == {(int(d), int(s)) for d, s in unfitted}, (sorted(mine), unfitted)

    def apply(self, x):
        y = np.array(x, np.float64)
        for lo, hi, Tm, C in self.parts:
            y[:, lo:hi] -= np.einsum("dkl,dl->dk", C, y[:, lo:hi]) @ Tm.T
        return y

    def apply_transpose(self, x):
        y = np.array(x, np.float64)
        for lo, hi, Tm, C in self.parts:
            y[:, lo:hi] -= np.einsum("dkl,dk->dl", C, y[:, lo:hi] @ Tm)
        return y
