"""Scan-synchronous ground pickup of a [D, T] TOD on the device: a template per detector in bins of a per-sample key (the
boresight azimuth), estimated and subtracted (``mrx_tod_bin_reduce``, ``mrx_tod_bin_apply``).

    kept(d, k)     = { t : bins[t] == k, flags[d, t] == 0 }
    hits[d, k]     = |kept(d, k)|
    sums[d, k]     = sum over kept(d, k) of (float64(x[d, t]) - float64(model[d, t]))
    template[d, k] = float32(sums / hits) where hits >= max(min_hits, 1), else 0
    y[d, t]        = x[d, t] + sign * template[d, bins[t]]       (one float32 operation; bins[t] == -1: y = x)

``bins`` is one int32 key per sample shared by all detectors, -1 for a sample that belongs to no bin: the two device
entries serve any template synchronous with such a key.  Only the azimuth front end (``azimuth_bins``) is built.  The
sums are float64 in an order fixed by the bin lists: reproducible bit for bit from call to call, and a row's result does
not depend on the rows beside it.  The bins are constant across their width: no interpolation between bin centres."""

from __future__ import annotations

import numpy as np

from ._tod_args import check_like, check_min_hits, check_out, check_sign, check_x, context, row_pitch, to_numpy

MAX_BINS = 4096  # mrx_ground.hip: kMaxBins


def _check_n_bins(n_bins):
    if int(n_bins) != n_bins or not 1 <= int(n_bins) <= MAX_BINS:
        raise ValueError(f"n_bins {n_bins}: an integer in 1 .. {MAX_BINS}")
    return int(n_bins)


def azimuth_bins(az, n_bins, lo=None, hi=None):
    """``(bins, lo, hi)``: the int32 [T] bin of every sample of the boresight azimuth ``az`` (radians, ``coords._baz``) in
    ``n_bins`` uniform bins on [lo, hi], float64 on the host.  The azimuth is first unwrapped about its circular mean
    (a = mean + the angle from the mean in [-pi, pi)), so that a scan across 0 / 2 pi is one interval; ``lo`` and ``hi``
    (default: the scan's own extent) are on that unwrapped axis, as this function returns them.
    k = min(floor((a - lo) / (hi - lo) * n_bins), n_bins - 1); samples outside [lo, hi] get -1; where hi == lo (a stare)
    every sample at lo is in bin 0."""
    n_bins = _check_n_bins(n_bins)
    az = np.asarray(az, np.float64)
    if az.ndim != 1 or az.size < 1 or not np.all(np.isfinite(az)):
        raise ValueError("az must be a one-dimensional array of finite angles")
    mean = float(np.arctan2(np.sin(az).mean(), np.cos(az).mean()))
    a = mean + ((az - mean + np.pi) % (2 * np.pi) - np.pi)
    lo = float(a.min()) if lo is None else float(lo)
    hi = float(a.max()) if hi is None else float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)) or hi < lo:
        raise ValueError(f"lo {lo}, hi {hi}: finite, with lo <= hi")
    if hi == lo:
        k = np.zeros(a.shape, np.int64)
    else:
        k = np.minimum(np.floor((a - lo) / (hi - lo) * n_bins), n_bins - 1).astype(np.int64)
    k[(a < lo) | (a > hi)] = -1
    return k.astype(np.int32), lo, hi


def _check_bins(bins, n_bins, T=None):
    """The int32 host array of a [T] key; refuses entries outside -1 .. n_bins - 1 and a wrong length."""
    b = np.asarray(to_numpy(bins))
    if b.ndim != 1 or b.dtype.kind not in "iu":
        raise ValueError("bins must be a one-dimensional integer array")
    if T is not None and b.size != T:
        raise ValueError(f"bins of length {b.size}: one entry per sample, {T}")
    if b.size and (b.min() < -1 or b.max() > n_bins - 1):
        raise ValueError(f"bins must lie in -1 .. n_bins - 1 = {n_bins - 1}")
    return np.ascontiguousarray(b, np.int32)


def bin_lists(bins, n_bins):
    """``(order, start)`` of a [T] key: int32 arrays, bin k owns the sample indices order[start[k] : start[k + 1]], ascending
    within a bin (a stable counting sort); entries of -1 are dropped, so len(order) = start[n_bins] <= T."""
    n_bins = _check_n_bins(n_bins)
    b = _check_bins(bins, n_bins)
    order = np.argsort(b, kind="stable")
    order = order[b[order] >= 0].astype(np.int32)
    start = np.zeros(n_bins + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(b[b >= 0], minlength=n_bins))
    return order, start


def bin_template(x, bins, n_bins, flags=None, model=None, min_hits=1, ctx=None):
    """``(template, hits, sums)`` of a [D, T] float32 device tensor ``x`` (any row pitch) under the [T] key ``bins``
    (-1 .. n_bins - 1): [D, n_bins] device tensors, float32, int64 and float64 (the formulas are at the top of the
    module).  ``flags``: a [D, T] uint8 tensor whose nonzero entries take no part; ``model``: a [D, T] float32 tensor
    subtracted sample by sample before the sum (both any row pitch, on x's device).  A bin with fewer than
    max(min_hits, 1) samples left has template 0.  Everything ``mrx_tod_bin_reduce`` refuses raises ValueError before
    any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    n_bins = _check_n_bins(n_bins)
    b = _check_bins(bins, n_bins, T)
    ld_f = check_like(flags, "flags", x, D, T, "uint8") if flags is not None else 0
    ld_m = check_like(model, "model", x, D, T) if model is not None else 0
    min_hits = check_min_hits(min_hits)
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    order, start = bin_lists(b, n_bins)
    d_order = torch.as_tensor(order if order.size else np.zeros(1, np.int32)).to(x.device)
    d_start = torch.as_tensor(start).to(x.device)
    sums = torch.empty((D, n_bins), dtype=torch.float64, device=x.device)
    hits = torch.empty((D, n_bins), dtype=torch.int32, device=x.device)
    template = torch.empty((D, n_bins), dtype=torch.float32, device=x.device)
    context(ctx, x).call("mrx_tod_bin_reduce", ptr(x), ld_x, ptr(model), ld_m, ptr(flags), ld_f, D, T, ptr(d_order), int(order.size),
                         ptr(d_start), n_bins, min_hits, ptr(sums), ptr(hits), ptr(template))
    return template, hits.to(torch.int64), sums


def apply_template(x, bins, template, sign=-1, out=None, ctx=None):
    """y = x + sign * template[:, bins] (sign -1 or +1; samples with bins == -1 copied) of a [D, T] float32 device tensor
    ``x`` (any row pitch) and a contiguous [D, K] float32 ``template``; returns ``out`` (None: a new tensor; ``x`` itself:
    in place; otherwise a [D, T] float32 tensor of any row pitch that does not overlap x).  Everything
    ``mrx_tod_bin_apply`` refuses raises ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    if not isinstance(template, torch.Tensor) or template.dim() != 2 or template.dtype != torch.float32 or template.shape[0] != D \
            or template.device != x.device or not template.is_contiguous():
        raise ValueError(f"template must be a contiguous [{D}, K] float32 tensor on x's device")
    K = _check_n_bins(template.shape[1])
    b = _check_bins(bins, K, T)
    sign = check_sign(sign)
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    else:
        check_out(out, x, D, T, in_place=True)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    d_bin = torch.as_tensor(b).to(x.device)
    context(ctx, x).call("mrx_tod_bin_apply", ptr(x), ld_x, D, T, ptr(d_bin), ptr(template), K, sign, ptr(out), row_pitch(out))
    return out


def shared_template(sums, hits, min_hits=1):
    """One template for the whole array from ``bin_template``'s [D, K] ``sums`` and ``hits``: float32(sum_d sums /
    sum_d hits) in float64 with torch where the summed hits reach max(min_hits, 1), else 0, as a contiguous [D, K]
    float32 tensor of D equal rows."""
    import torch

    if not isinstance(sums, torch.Tensor) or not isinstance(hits, torch.Tensor) or sums.dim() != 2 or sums.shape != hits.shape:
        raise ValueError("sums and hits must be [D, K] tensors of one shape")
    min_hits = check_min_hits(min_hits)
    n = hits.to(torch.float64).sum(dim=0)
    s = sums.to(torch.float64).sum(dim=0)
    ok = n >= max(min_hits, 1)
    row = torch.where(ok, s / torch.where(ok, n, torch.ones_like(n)), torch.zeros_like(s)).to(torch.float32)
    return row[None, :].expand(sums.shape[0], -1).contiguous()


def synthetic_ground(D, n_bins, amplitude, seed):
    """A smooth [D, n_bins] float32 table for tests and benchmarks: amplitude * (1 + 0.1 d / D) * cos(2 pi k / n_bins +
    phase), phase = ``np.random.default_rng(seed).uniform(0, 2 pi)``: coherent across detectors, a tenth stronger at the
    last than at the first."""
    n_bins = _check_n_bins(n_bins)
    if int(D) != D or int(D) < 1:
        raise ValueError(f"D {D}: an integer >= 1")
    phase = np.random.default_rng(seed).uniform(0.0, 2 * np.pi)
    d, k = np.arange(int(D))[:, None], np.arange(n_bins)[None, :]
    return (float(amplitude) * (1 + 0.1 * d / int(D)) * np.cos(2 * np.pi * k / n_bins + phase)).astype(np.float32)
