"""The covariance between the detectors of a [D, T] TOD on the device, flagged samples left out of every sum, and what is
built on it: the leading modes of a group's correlation matrix as time templates, and a score that tells a detector
that does not see what its neighbours see (``mrx_tod_gram``).

    term(d, t) = float64(x[d, t]) - float64(model[d, t])
    z(d, t)    = float32(term(d, t) - center[d]) where flags[d, t] == 0, else 0
    G[i, j]    = sum over t of z(rows[i], t) * z(rows[j], t);   n[i, j] = the number of t both rows keep
    cov        = G / n;   corr[i, j] = cov[i, j] / sqrt(cov[i, i] * cov[j, j])

G is summed on the matrix cores: inside a block of ``GRAM_BLOCK`` samples the float32 fused-multiply-add chain in
ascending t, the block sums added in float64 in ascending order, a function of T alone and without atomics, so the same
inputs give the same bits on every call and an entry depends on its two rows only.  The order and the error bound are
written out in include/mrx.h, and tests/covariance_ref.py restates them in numpy.  Everything after G is the
reproducible kernels of maria_amd.cuts and maria_amd.regress and float64 torch."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from ._tod_args import check_count, check_like, check_min_hits, check_x, context

GRAM_BLOCK = 256   # include/mrx.h: MRX_GRAM_BLOCK (the binding's _lib.GRAM_BLOCK)
MAX_GROUPS = 16    # regress.MAX_GROUPS: the templates go through mrx_tod_column_mean
MAX_MODES = 7      # with the constant beside them: regress.MAX_TEMPLATES


class GroupCovariance(NamedTuple):
    """One group of ``covariance``.  ``rows`` [R] int64 (the rows of x, ascending); ``mean`` [R] float64 and ``hits`` [R]
    int64 of each row; ``G``, ``cov``, ``corr`` [R, R] float64; ``n`` [R, R] int64; ``valid`` [R, R] bool (n >= min_hits and at
    least 1); ``unusable`` [R] bool.  ``cov`` is 0 where a pair is not valid, ``corr`` also where a row is unusable."""

    rows: object
    mean: object
    hits: object
    G: object
    n: object
    cov: object
    corr: object
    valid: object
    unusable: object


class Covariance(NamedTuple):
    """``covariance``'s result: ``groups`` (a list of ``GroupCovariance``, one per group, R = 0 for a group without
    rows), ``group_of`` [D] int64 (-1: in no group), ``mean`` and ``sigma`` [D] float64 (sqrt(cov_dd); 0 for a row that is
    unusable or in no group), ``usable`` [D] bool and ``min_hits``."""

    groups: list
    group_of: object
    mean: object
    sigma: object
    usable: object
    min_hits: int


def _check_rows(rows, x):
    """None, or the [R] int32 tensor on x's device of ``rows`` (a tensor or an integer array), R >= 1."""
    import torch

    if rows is None:
        return None
    r = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    if r.ndim != 1 or r.size < 1 or r.dtype.kind not in "iu":
        raise ValueError("rows must be a one-dimensional array of R >= 1 integers")
    r = r.astype(np.int64)
    if r.min() < np.iinfo(np.int32).min or r.max() > np.iinfo(np.int32).max:
        raise ValueError("rows must fit int32")
    return torch.as_tensor(np.ascontiguousarray(r, np.int32)).to(x.device)


def gram(x, center=None, rows=None, flags=None, model=None, counts=True, ctx=None):
    """``(G, n)`` of a [D, T] float32 device tensor ``x`` (any row pitch): [R, R] float64 and [R, R] int64 device tensors
    (the formulas are at the top of the module); n is None without ``counts``.  ``center``: a [D] float64 tensor on x's
    device (None: zeros); ``rows``: R >= 1 integers, the rows that take part in any order (None: all D); an entry
    outside 0 .. D - 1 is a row of zeros.  ``flags`` [D, T] uint8 and ``model`` [D, T] float32, any row pitch.  Everything
    ``mrx_tod_gram`` refuses raises ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    if center is not None and (not isinstance(center, torch.Tensor) or center.dtype != torch.float64 or tuple(center.shape) != (D,)
                               or center.device != x.device):
        raise ValueError(f"center must be a [{D}] float64 tensor on x's device")
    d_rows = _check_rows(rows, x)
    R = D if d_rows is None else int(d_rows.shape[0])
    ld_f = check_like(flags, "flags", x, D, T, "uint8") if flags is not None else 0
    ld_m = check_like(model, "model", x, D, T) if model is not None else 0
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    center = center.contiguous() if center is not None else None
    G = torch.empty((R, R), dtype=torch.float64, device=x.device)
    n = torch.empty((R, R), dtype=torch.int32, device=x.device) if counts else None
    context(ctx, x).call("mrx_tod_gram", ptr(x), ld_x, ptr(model), ld_m, ptr(flags), ld_f, D, T, ptr(d_rows), R, ptr(center), ptr(G), ptr(n))
    return G, (n.to(torch.int64) if counts else None)


def _group_rows(groups, n_groups, D):
    """[D] int64 host array of each row's group, -1 for none."""
    import torch

    G = check_count(n_groups, "n_groups", MAX_GROUPS)
    if groups is None:
        return np.zeros(D, np.int64), G
    g = groups.detach().cpu().numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups)
    if g.ndim != 1 or g.size != D or g.dtype.kind not in "iu":
        raise ValueError(f"groups must be {D} integers, one per row")
    g = g.astype(np.int64)
    return np.where((g >= 0) & (g < G), g, -1), G


def finish_group(rows, mean, hits, G, n, min_hits):
    """The ``GroupCovariance`` of a group's sums: plain float64 torch on their device (host tensors as well).  A pair is
    valid with n >= max(min_hits, 1); cov = G / n there and 0 elsewhere.  A row is unusable with n_ii < max(min_hits, 1),
    G_ii == 0 or G_ii not finite.  corr = cov_ij / sqrt(cov_ii * cov_jj) (one product, one root, one quotient) where the
    pair is valid and both rows usable, 0 elsewhere."""
    import torch

    floor = max(check_min_hits(min_hits), 1)
    valid = n >= floor
    cov = torch.where(valid, G / torch.where(valid, n, torch.ones_like(n)).to(torch.float64), torch.zeros_like(G))
    dG, dn = torch.diagonal(G), torch.diagonal(n)
    unusable = (dn < floor) | (dG == 0) | ~torch.isfinite(dG)
    var = torch.where(unusable, torch.ones_like(dG), torch.diagonal(cov))
    both = valid & ~unusable[:, None] & ~unusable[None, :]
    corr = torch.where(both, cov / torch.sqrt(var[:, None] * var[None, :]), torch.zeros_like(cov))
    return GroupCovariance(rows, mean, hits, G, n, cov, corr, valid, unusable)


def covariance(x, groups=None, n_groups=1, flags=None, model=None, min_hits=8, ctx=None):
    """The ``Covariance`` of the rows of ``x`` ([D, T] float32 device tensor, any row pitch) within each group.  ``groups``:
    [D] integers (None: all rows in group 0), an entry outside 0 .. n_groups - 1 leaving a row out.  Per group: each row's
    mean and hits over its kept samples (``cuts.moments``, the whole row one segment), then ``gram`` of the group's rows
    about those means, then ``finish_group``.  Covariances across groups are not computed."""
    import torch

    from . import cuts

    D, T, _ = check_x(x)
    group_of, n_g = _group_rows(groups, n_groups, D)
    min_hits = check_min_hits(min_hits)
    if flags is not None:
        check_like(flags, "flags", x, D, T, "uint8")
    if model is not None:
        check_like(model, "model", x, D, T)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    ctx = context(ctx, x)
    dev = x.device
    m = cuts.moments(x, None, flags=flags, model=model, ctx=ctx)
    mean, hits = m.mean[:, 0].contiguous(), m.hits[:, 0]
    sigma = torch.zeros(D, dtype=torch.float64, device=dev)
    usable = torch.zeros(D, dtype=torch.bool, device=dev)
    out = []
    for g in range(n_g):
        rows = torch.as_tensor(np.flatnonzero(group_of == g)).to(dev)
        if rows.numel() == 0:
            e = torch.zeros((0, 0), dtype=torch.float64, device=dev)
            out.append(GroupCovariance(rows, mean[rows], hits[rows], e, e.to(torch.int64), e, e, e.to(torch.bool), rows.to(torch.bool)))
            continue
        G, n = gram(x, center=mean, rows=rows, flags=flags, model=model, counts=True, ctx=ctx)
        cg = finish_group(rows, mean[rows], hits[rows], G, n, min_hits)
        out.append(cg)
        sigma[rows] = torch.where(cg.unusable, torch.zeros_like(mean[rows]), torch.sqrt(torch.diagonal(cg.cov)))
        usable[rows] = ~cg.unusable
    return Covariance(out, torch.as_tensor(group_of).to(dev), mean, sigma, usable, min_hits)


def leading_modes(cov_group, k):
    """``(eigenvalues [k], vectors [R, k])``, float64 on the group's device: the k largest eigenvalues, descending, of
    ``corr`` restricted to the usable rows (``torch.linalg.eigh`` in float64) and their unit eigenvectors, zero on the
    unusable rows; each vector's sign is fixed so that the sum of its components is >= 0.  k must be in 1 .. the number
    of usable rows."""
    import torch

    keep = torch.nonzero(~cov_group.unusable)[:, 0]
    R, m = int(cov_group.unusable.shape[0]), int(keep.numel())
    if int(k) != k or not 1 <= int(k) <= m:
        raise ValueError(f"k {k}: an integer in 1 .. {m}, the usable rows")
    k = int(k)
    C = cov_group.corr.to(torch.float64)[keep][:, keep]
    w, V = torch.linalg.eigh(C)
    w, V = torch.flip(w, [0])[:k], torch.flip(V, [1])[:, :k]
    V = torch.where(V.sum(dim=0) < 0, -V, V)
    U = torch.zeros((R, k), dtype=torch.float64, device=C.device)
    U[keep] = V
    return w, U


def loadings(cov, k):
    """``(eigenvalues [G, k], U [D, k])``: ``leading_modes`` of every group of ``cov``, the vectors scattered to the rows of
    x.  A group with fewer than k usable rows gets zeros."""
    import torch

    D, dev = int(cov.mean.shape[0]), cov.mean.device
    k = check_count(k, "k", MAX_MODES)
    eig = torch.zeros((len(cov.groups), k), dtype=torch.float64, device=dev)
    U = torch.zeros((D, k), dtype=torch.float64, device=dev)
    for g, cg in enumerate(cov.groups):
        if int((~cg.unusable).sum()) >= k:
            eig[g], U[cg.rows] = leading_modes(cg, k)
    return eig, U


def mode_templates(x, cov, U, flags=None, model=None, ctx=None):
    """[G, K, T] float32: per group and mode k the flag-aware projection of the normalised rows onto the loading,
    S / W with S[t] = sum_d (U[d, k] / sigma_d) (term(d, t) - mean_d) and W[t] = sum_d U[d, k]^2 over the rows that
    keep t: one ``regress.column_mean`` call per mode, over all groups at once.  ``U`` [D, K] float64 (``loadings``);
    rows with sigma = 0 take no part."""
    import torch

    from . import regress

    D, T, _ = check_x(x)
    if not isinstance(U, torch.Tensor) or U.dim() != 2 or U.shape[0] != D or U.dtype != torch.float64 or U.device != x.device:
        raise ValueError(f"U must be a [{D}, K] float64 tensor on x's device")
    K = check_count(U.shape[1], "K", MAX_MODES)
    n_g = len(cov.groups)
    live = cov.sigma > 0
    inv = torch.where(live, 1.0 / torch.where(live, cov.sigma, torch.ones_like(cov.sigma)), torch.zeros_like(cov.sigma))
    groups = cov.group_of.to(torch.int32)
    B = torch.empty((n_g, K, T), dtype=torch.float32, device=x.device)
    for k in range(K):
        u = (U[:, k] * inv).contiguous()
        v = torch.where(live, U[:, k] * U[:, k], torch.zeros_like(u)).contiguous()
        B[:, k, :], _, _ = regress.column_mean(x, u, v, off=cov.mean, groups=groups, n_groups=n_g, flags=flags, model=model, ctx=ctx)
    return B


def correlation_score(cov_group):
    """[R] float64: per row i the median (the mean of the two middle values) of ``corr[i, j]`` over the other usable rows
    j whose pair with i is valid; NaN for an unusable row and for a row without such a partner."""
    import torch

    corr, ok = cov_group.corr, ~cov_group.unusable
    R = int(ok.shape[0])
    take = cov_group.valid & ok[:, None] & ok[None, :] & ~torch.eye(R, dtype=torch.bool, device=corr.device)
    count = take.sum(dim=1)
    if R == 0:
        return torch.zeros(0, dtype=torch.float64, device=corr.device)
    ranked, _ = torch.sort(torch.where(take, corr, torch.full_like(corr, float("inf"))), dim=1)
    a = torch.clamp(count - 1, min=0) // 2
    b = count // 2
    med = (ranked.gather(1, a[:, None])[:, 0] + ranked.gather(1, b.clamp(max=R - 1)[:, None])[:, 0]) / 2.0
    return torch.where(count > 0, med, torch.full_like(med, float("nan")))


def judge(cov, n_sigma=5.0, min_correlation=None):
    """The rule of ``TOD.cut_uncorrelated`` on a ``Covariance`` (plain torch: host tensors as well): a dict of [D] tensors
    ``score`` (``correlation_score`` scattered to the rows of x, NaN for a row in no group), ``outlier`` (the low-side
    outliers of the score within the group: ``cuts.find_outliers`` at ``n_sigma``, side "low", over the usable rows with a
    score), ``below`` (score < ``min_correlation`` where one is given), ``unusable`` (a grouped row that is unusable or
    has no score) and ``cut``, their OR; and of [G] tensors ``median`` and ``threshold`` = median - n_sigma * 1.4826 *
    median |score - median| (NaN for a group without a score)."""
    import torch

    from . import cuts

    D, dev, n_g = int(cov.mean.shape[0]), cov.mean.device, len(cov.groups)
    score = torch.full((D,), float("nan"), dtype=torch.float64, device=dev)
    for cg in cov.groups:
        if cg.rows.numel():
            score[cg.rows] = correlation_score(cg)
    eligible = cov.usable & torch.isfinite(score)
    outlier, unusable = cuts.find_outliers(score, cov.group_of, n_sigma, "low", eligible)
    below = torch.zeros_like(outlier) if min_correlation is None else eligible & (cov.group_of >= 0) & (score < float(min_correlation))
    median = torch.full((n_g,), float("nan"), dtype=torch.float64, device=dev)
    threshold = median.clone()
    idx = torch.nonzero(eligible & (cov.group_of >= 0))[:, 0]
    if idx.numel():
        med = cuts._group_median(score[idx], cov.group_of[idx], n_g)
        mad = cuts._group_median((score[idx] - med[cov.group_of[idx]]).abs(), cov.group_of[idx], n_g)
        median, threshold = med, med - float(n_sigma) * cuts.MAD_TO_SIGMA * mad
    return {"score": score, "outlier": outlier, "below": below, "unusable": unusable, "cut": outlier | below | unusable,
            "median": median, "threshold": threshold}


def inject_uncorrelated(data, rows, seed=None):
    """A float32 copy of the host array ``data`` [D, T] with the named rows replaced by their own series reversed in time
    (for tests and demonstrations): every statistic of a whole row is what it was, to the rounding of a sum taken in
    another order, and what the row shares with the others sample by sample is gone.  Nothing is drawn: ``seed`` is
    accepted so that the call reads like ``cuts.inject_bad``'s, and must be None or an integer."""
    x = np.array(data, np.float32)
    if x.ndim != 2:
        raise ValueError("data must be a [D, T] array")
    if seed is not None and (isinstance(seed, bool) or int(seed) != seed):
        raise ValueError(f"seed {seed}: None or an integer")
    rows = [int(d) for d in rows]
    if any(not 0 <= d < x.shape[0] for d in rows):
        raise ValueError(f"rows must be in 0 .. {x.shape[0] - 1}")
    for d in rows:
        x[d] = x[d, ::-1].copy()
    return x
