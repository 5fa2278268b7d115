"""The numpy float64 reference of maria_amd.ground: the two formulas of include/mrx.h, plain and slow."""

import numpy as np


def bin_reduce(x, bins, n_bins, flags=None, model=None, min_hits=1):
    """(sums float64, hits int64, template float32, absum float64), each [D, n_bins]: over the samples t of a row with
    bins[t] == k and flags[d, t] == 0, the sum of float64(x) - float64(model), their number, float32(sum / hits) where
    hits >= max(min_hits, 1) (else 0), and the sum of the terms' magnitudes (for rounding bounds).  ``bins`` entries
    outside 0 .. n_bins - 1 belong to no bin."""
    x = np.asarray(x, np.float32)
    D, T = x.shape
    bins = np.asarray(bins, np.int64)
    terms = x.astype(np.float64)
    if model is not None:
        terms = terms - np.asarray(model, np.float32).astype(np.float64)
    sums, absum, hits = np.zeros((D, n_bins)), np.zeros((D, n_bins)), np.zeros((D, n_bins), np.int64)
    inside = (bins >= 0) & (bins < n_bins)
    for d in range(D):
        keep = inside if flags is None else inside & (np.asarray(flags)[d] == 0)
        np.add.at(sums[d], bins[keep], terms[d, keep])
        np.add.at(absum[d], bins[keep], np.abs(terms[d, keep]))
        np.add.at(hits[d], bins[keep], 1)
    ok = hits >= max(int(min_hits), 1)
    template = np.where(ok, sums / np.where(ok, hits, 1), 0.0).astype(np.float32)
    return sums, hits, template, absum


def bin_reduce_by_loops(x, bins, n_bins, flags=None, model=None, min_hits=1):
    """(sums, hits, template) again, by a double loop over rows and samples."""
    D, T = np.shape(x)
    sums, hits = np.zeros((D, n_bins)), np.zeros((D, n_bins), np.int64)
    for d in range(D):
        for t in range(T):
            k = int(bins[t])
            if k < 0 or k >= n_bins or (flags is not None and flags[d][t] != 0):
                continue
            term = float(np.float32(x[d][t]))
            if model is not None:
                term = term - float(np.float32(model[d][t]))
            sums[d, k] += term
            hits[d, k] += 1
    template = np.zeros((D, n_bins), np.float32)
    for d in range(D):
        for k in range(n_bins):
            if hits[d, k] >= max(int(min_hits), 1):
                template[d, k] = np.float32(sums[d, k] / float(hits[d, k]))
    return sums, hits, template


def bin_apply(x, bins, template, sign):
    """y = x + sign * template[d, bins[t]] in float32 (one operation); x where bins[t] is outside 0 .. K - 1."""
    x = np.asarray(x, np.float32)
    template = np.asarray(template, np.float32)
    bins = np.asarray(bins, np.int64)
    K = template.shape[1]
    inside = (bins >= 0) & (bins < K)
    y = x.copy()
    g = template[:, bins[inside]]
    y[:, inside] = x[:, inside] - g if sign < 0 else x[:, inside] + g
    return y


def azimuth_bins_by_loop(az, n_bins, lo=None, hi=None):
    """(bins, lo, hi) of maria_amd.ground.azimuth_bins, sample by sample."""
    import math

    mean = math.atan2(float(np.sin(az).mean()), float(np.cos(az).mean()))  # numpy's pairwise means, as the function's
    az = [float(a) for a in az]
    un = []
    for a in az:
        delta = (a - mean + math.pi) % (2 * math.pi) - math.pi
        un.append(mean + delta)
    lo = min(un) if lo is None else lo
    hi = max(un) if hi is None else hi
    out = []
    for a in un:
        if a < lo or a > hi:
            out.append(-1)
        elif hi == lo:
            out.append(0)
        else:
            out.append(min(int(math.floor((a - lo) / (hi - lo) * n_bins)), n_bins - 1))
    return np.array(out, np.int32), lo, hi


def bin_lists_by_loop(bins, n_bins):
    """(order, start): for each bin in turn, the indices that hold it, ascending."""
    order, start = [], [0]
    for k in range(n_bins):
        order += [t for t in range(len(bins)) if bins[t] == k]
        start.append(len(order))
    return np.array(order, np.int32), np.array(start, np.int32)
