"""The numpy float64 reference of maria_amd.cuts: the moments of include/mrx.h with their operation order,
``summarize``, ``find_outliers`` and ``decide``, plain and slow.  Sums are ``math.fsum`` over the rounded terms: the
correctly rounded sum, whatever order the device adds in."""

import math

import numpy as np
from subscans_ref import _terms, segments

HALF_ULP = 2.0**-53
SLACK = 1.001  # second-order terms: below L 2^-53 < 2.3e-13 of the first-order ones for L <= 2049
NAMES = ("mean", "m2", "m3", "m4", "min", "max", "d2")


def naive(v, reverse=False):
    """The float64 sum of ``v`` added one by one, forwards or backwards."""
    s = 0.0
    for a in (v[::-1] if reverse else v):
        s = s + float(a)
    return s


def moments(x, bounds=None, flags=None, model=None, total=math.fsum):
    """A dict of [D, S] arrays: ``hits``, ``pairs`` (int64), ``mean``, ``m2``, ``m3``, ``m4``, ``min``, ``max``, ``d2`` as
    include/mrx.h defines them (mu = total(term) / n, e = term - mu, the powers e e, (e e) e, (e e) (e e), one rounding an
    operation, then total of the products), and for the bounds ``abs1`` = sum|term|, ``abse1`` .. ``abse4`` = sum|e|^k
    and ``length`` (of the segment, repeated down the rows).  ``total``: the summation, math.fsum unless a test wants
    another."""
    terms = _terms(x, model)
    D, T = terms.shape
    segs = segments([0, T] if bounds is None else bounds, T)
    S = len(segs)
    out = {k: np.zeros((D, S)) for k in NAMES + ("abs1", "abse1", "abse2", "abse3", "abse4", "length")}
    out["hits"], out["pairs"] = np.zeros((D, S), np.int64), np.zeros((D, S), np.int64)
    for s, (lo, hi) in enumerate(segs):
        out["length"][:, s] = max(hi - lo, 0)
        if hi <= lo:
            continue
        for d in range(D):
            keep = np.ones(hi - lo, bool) if flags is None else np.asarray(flags)[d, lo:hi] == 0
            t = terms[d, lo:hi]
            n = int(keep.sum())
            both = keep[1:] & keep[:-1]
            out["hits"][d, s], out["pairs"][d, s] = n, int(both.sum())
            if n == 0:
                continue
            kept = t[keep]
            mu = total(kept) / float(n)
            e = kept - mu
            e2 = e * e
            diff = t[1:][both] - t[:-1][both]
            out["mean"][d, s], out["m2"][d, s], out["m3"][d, s], out["m4"][d, s] = mu, total(e2), total(e2 * e), total(e2 * e2)
            out["min"][d, s], out["max"][d, s] = kept.min(), kept.max()
            out["d2"][d, s] = total(diff * diff) if both.any() else 0.0
            out["abs1"][d, s] = math.fsum(np.abs(kept))
            for k in (1, 2, 3, 4):
                out[f"abse{k}"][d, s] = math.fsum(np.abs(e) ** k)
    return out


def bounds_of(m):
    """The derived bounds on |device - reference| of ``mean``, ``d2`` and ``m2`` .. ``m4`` (tests/test_gpu_cuts.py's
    docstring and DESIGN 3.26 derive them), as a dict of [D, S] arrays."""
    L1 = m["length"] + 1.0
    n = np.maximum(m["hits"], 1).astype(np.float64)
    dmu = L1 * HALF_ULP * m["abs1"] / n + HALF_ULP * np.abs(m["mean"])
    out = {"mean": dmu, "d2": L1 * HALF_ULP * m["d2"]}
    lower = {2: m["abse1"], 3: m["abse2"], 4: m["abse3"]}
    for k in (2, 3, 4):
        a = m[f"abse{k}"]
        out[f"m{k}"] = SLACK * (L1 * HALF_ULP * a + (k + 1) * HALF_ULP * a + k * dmu * lower[k])
    return out


def summarize(m):
    """``cuts.summarize`` in numpy on the reference's dict."""
    n, p = m["hits"].astype(np.float64), m["pairs"].astype(np.float64)
    some = m["hits"] > 0
    with np.errstate(all="ignore"):
        var = np.where(some, m["m2"] / n, np.nan)
        spread = some & (m["m2"] > 0)
        return {
            "hits": m["hits"], "pairs": m["pairs"], "mean": np.where(some, m["mean"], np.nan), "min": np.where(some, m["min"], np.nan),
            "max": np.where(some, m["max"], np.nan), "var": var, "std": np.sqrt(var),
            "skew": np.where(spread, np.sqrt(n) * m["m3"] / (m["m2"] * np.sqrt(m["m2"])), np.nan),
            "kurtosis": np.where(spread, n * m["m4"] / (m["m2"] * m["m2"]) - 3.0, np.nan),
            "ptp": np.where(some, m["max"] - m["min"], np.nan),
            "sigma_diff": np.where(m["pairs"] > 0, np.sqrt(m["d2"] / (2.0 * p)), np.nan),
            "flagged_fraction": np.where(m["length"] > 0, 1.0 - n / m["length"], np.nan),
        }


def find_outliers(v, groups, n_sigma, side="both", eligible=None, margins=None, min_rel_scale=None):
    """``(outlier, unusable)`` of ``cuts.find_outliers``, group by group with numpy.median.  ``margins``: a list that
    gains |far - n_sigma scale| / (n_sigma scale) of every judged entry (how far a verdict is from flipping)."""
    v = np.asarray(v, np.float64)
    g = np.zeros(v.shape, np.int64) if groups is None else np.asarray(groups, np.int64)
    eligible = np.ones(v.shape, bool) if eligible is None else np.asarray(eligible, bool)
    ok = (g >= 0) & eligible & np.isfinite(v)
    outlier = np.zeros(v.shape, bool)
    for k in np.unique(g[ok]):
        sel = ok & (g == k)
        med = np.median(v[sel])
        dev = v[sel] - med
        scale = np.full(dev.shape, 1.4826 * np.median(np.abs(dev)))
        if min_rel_scale is not None:
            scale = np.maximum(scale, np.asarray(min_rel_scale)[sel] * np.abs(med))
        far = {"both": np.abs(dev), "high": dev, "low": -dev}[side]
        outlier[sel] = (scale > 0) & (far > float(n_sigma) * scale)
        if margins is not None:
            margins.extend((np.abs(far - float(n_sigma) * scale) / (float(n_sigma) * scale))[scale > 0].tolist())
    return outlier, (g >= 0) & ~ok


def bad_segments(seg, groups=None, n_sigma_segment=5.0, min_hits=8, margins=None):
    """``cuts.bad_segments`` on the reference's summary."""
    D, S = seg["hits"].shape
    if n_sigma_segment is None:
        return np.zeros((D, S), bool)
    g = np.zeros(D, np.int64) if groups is None else np.asarray(groups, np.int64)
    rows = np.broadcast_to(np.where(g >= 0, np.arange(D), -1)[:, None], (D, S))
    pairs = seg["pairs"].astype(np.float64)
    own = np.sqrt(0.75 / np.maximum(pairs, 1.0))
    return find_outliers(seg["sigma_diff"], rows, n_sigma_segment, "high", (seg["hits"] >= max(int(min_hits), 1)) & (pairs > 0), margins, own)[0]


def decide(det, seg, bad, groups=None, n_sigma=5.0, max_flagged=0.5, max_bad_segments=0.5, min_hits=8,
           criteria=("white", "rms", "skew", "kurtosis", "flagged"), margins=None):
    """``(masks, cut_detectors)`` of ``cuts.decide`` on the reference's summaries (``det``: [D, 1])."""
    floor = max(int(min_hits), 1)
    hits = det["hits"][:, 0]
    D, S = seg["hits"].shape
    g = np.zeros(D, np.int64) if groups is None else np.asarray(groups, np.int64)
    eligible = hits >= floor
    with np.errstate(all="ignore"):
        values = {"white": np.log(det["sigma_diff"][:, 0]), "rms": np.log(det["std"][:, 0]), "skew": det["skew"][:, 0],
                  "kurtosis": det["kurtosis"][:, 0]}
    masks = {}
    unusable = (g >= 0) & ~eligible
    for name, v in values.items():
        if name in criteria:
            masks[name], u = find_outliers(v, g, n_sigma, "both", eligible, margins)
            unusable = unusable | u
    if "flagged" in criteria:
        masks["flagged"] = (g >= 0) & (det["flagged_fraction"][:, 0] > max_flagged)
        if margins is not None:
            margins.extend((np.abs(det["flagged_fraction"][:, 0] - max_flagged) / max(max_flagged, 1e-300)).tolist())
    masks["unusable"] = unusable
    nonempty = (seg["hits"] > 0).sum(axis=1).astype(np.float64)
    count = bad.sum(axis=1).astype(np.float64)
    masks["segments"] = (g >= 0) & (count > max_bad_segments * nonempty)
    if margins is not None:
        margins.extend((np.abs(count - max_bad_segments * nonempty) / np.maximum(max_bad_segments * nonempty, 1e-300))[nonempty > 0].tolist())
    cut = np.zeros(D, bool)
    for m in masks.values():
        cut = cut | m
    return masks, cut


def flag_segments(flags, bounds, mask, value):
    """A copy of ``flags`` with ``value`` ORed into every sample of a masked segment; where segments overlap (bounds that
    do not ascend) this is not the device's rule, so the tests give it ascending bounds or clamp first."""
    out = np.array(flags, np.uint8)
    T = out.shape[1]
    for s, (lo, hi) in enumerate(segments(bounds, T)):
        if hi > lo:
            out[np.asarray(mask)[:, s] != 0, lo:hi] |= np.uint8(value)
    return out
