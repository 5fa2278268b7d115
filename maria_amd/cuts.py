"""Statistics per (detector, segment) on the device, and the rules that turn them into cuts (``mrx_tod_segment_moments``,
``mrx_tod_segment_flag``).

``bounds`` [S + 1] int32, ascending, cuts a row of T samples into S segments as in maria_amd.subscans.  In a segment
[lo, hi) of row d, with kept = the samples whose flag is 0, n of them, and the p pairs (t, t + 1) both in it and kept:

    term(d, t) = float64(x[d, t]) - float64(model[d, t])
    mean = sum(term) / n;   e = term - mean;   m2, m3, m4 = sum e^2, sum e^2 e, sum e^2 e^2      (over kept)
    min, max of term over kept;   d2 = sum over the pairs of (term(t + 1) - term(t))^2

Every sum is added in a fixed order (a function of the segment's ends alone), without atomics: the same inputs give the
same bits on every call.  ``summarize`` turns the sums into the usual statistics in float64 torch; ``find_outliers`` is
the robust rule (median and scaled median absolute deviation per group) that ``TOD.cut`` applies to them, and
``flag_segments`` writes a [D, S] verdict into per-sample flags.  The order of the operations is written out in
include/mrx.h, and tests/cuts_ref.py restates it in numpy."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from ._tod_args import check_like, check_min_hits, check_x, context
from .subscans import _check_bounds

MAD_TO_SIGMA = 1.4826  # the median absolute deviation of a Gaussian is sigma / 1.4826
SIDES = ("both", "high", "low")
# sigma_diff of p pairs of white noise: var(sum d^2) = p (8 + 2 * 2) sigma^4 (neighbouring differences share a sample), so
# that the variance estimate scatters by sqrt(3 / p) and its root by half of that, sqrt(0.75 / p), of itself
SIGMA_DIFF_SCATTER = 0.75


class Moments(NamedTuple):
    """[D, S] device tensors of ``moments``: ``hits`` and ``pairs`` int64, the rest float64."""

    hits: object
    pairs: object
    mean: object
    m2: object
    m3: object
    m4: object
    min: object
    max: object
    d2: object


def chunk_bounds(T, length):
    """[S + 1] int32: segments of ``length`` samples from 0 on, the last one shorter where T is no multiple: for scans
    without turnarounds."""
    if int(T) != T or int(T) < 1 or int(length) != length or int(length) < 1:
        raise ValueError(f"T {T}, length {length}: two integers >= 1")
    T, length = int(T), int(length)
    if T > np.iinfo(np.int32).max:
        raise ValueError(f"T {T} does not fit int32")
    return np.append(np.arange(0, T, length, dtype=np.int64), T).astype(np.int32)


def moments(x, bounds=None, flags=None, model=None, ctx=None):
    """``Moments`` of every (row, segment) of ``x`` ([D, T] float32 device tensor, any row pitch): [D, S] device tensors,
    zeros where nothing is kept.  ``bounds`` None: the whole row is one segment.  ``flags`` [D, T] uint8 and ``model``
    [D, T] float32, any row pitch.  Everything ``mrx_tod_segment_moments`` refuses, and bounds that do not ascend, raise
    ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    d_bounds, S = _check_bounds(np.array([0, T], np.int64) if bounds is None else bounds, x)
    ld_f = check_like(flags, "flags", x, D, T, "uint8") if flags is not None else 0
    ld_m = check_like(model, "model", x, D, T) if model is not None else 0
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    stat = torch.empty((D, S, 8), dtype=torch.float64, device=x.device)
    count = torch.empty((D, S, 2), dtype=torch.int32, device=x.device)
    context(ctx, x).call("mrx_tod_segment_moments", ptr(x), ld_x, ptr(model), ld_m, ptr(flags), ld_f, D, T, ptr(d_bounds), S, ptr(stat),
                         ptr(count))
    count = count.to(torch.int64)
    return Moments(count[..., 0], count[..., 1], *(stat[..., i] for i in range(7)))


def summarize(m, lengths=None):
    """The statistics of ``Moments`` ``m`` as a dict of [D, S] tensors, float64 torch on m's device: ``hits``, ``pairs``,
    ``mean``, ``min``, ``max``, ``var`` = m2 / n, ``std``, ``skew`` = sqrt(n) m3 / m2^1.5 and ``kurtosis`` =
    n m4 / m2^2 - 3 (scipy.stats' biased defaults), ``ptp`` = max - min, ``sigma_diff`` = sqrt(d2 / (2 p)) (the white
    level: a drift that is slow against the sample rate does not enter a difference of neighbours) and, with
    ``lengths`` [S] (the segments' lengths, ``numpy.diff`` of the clamped bounds), ``flagged_fraction`` = 1 - n / length.
    NaN where a value is not defined: everything but the counts at n = 0, skew and kurtosis at m2 = 0, sigma_diff at
    p = 0, flagged_fraction at length 0."""
    import torch

    n, p = m.hits.to(torch.float64), m.pairs.to(torch.float64)
    nan = torch.full_like(m.mean, float("nan"))
    some = m.hits > 0
    var = torch.where(some, m.m2 / n, nan)
    spread = some & (m.m2 > 0)
    out = {
        "hits": m.hits, "pairs": m.pairs, "mean": torch.where(some, m.mean, nan), "min": torch.where(some, m.min, nan),
        "max": torch.where(some, m.max, nan), "var": var, "std": torch.sqrt(var),
        "skew": torch.where(spread, torch.sqrt(n) * m.m3 / (m.m2 * torch.sqrt(m.m2)), nan),
        "kurtosis": torch.where(spread, n * m.m4 / (m.m2 * m.m2) - 3.0, nan),
        "ptp": torch.where(some, m.max - m.min, nan),
        "sigma_diff": torch.where(m.pairs > 0, torch.sqrt(m.d2 / (2.0 * p)), nan),
    }
    if lengths is not None:
        length = torch.as_tensor(np.asarray(lengths, np.float64)).to(m.mean.device)
        if length.dim() != 1 or length.shape[0] != m.mean.shape[1]:
            raise ValueError(f"lengths must be the [{m.mean.shape[1]}] lengths of the segments")
        length = length[None, :].expand_as(n)
        out["flagged_fraction"] = torch.where(length > 0, 1.0 - n / length, nan)
    return out


def flag_segments(flags, bounds, mask, value=1, ctx=None):
    """``flags[d, t] |= value`` IN PLACE for every sample t of a segment s with ``mask[d, s]`` nonzero; returns ``flags``
    ([D, T] uint8 device tensor, any row pitch).  ``mask``: a [D, S] bool or uint8 tensor on the flags' device;
    ``value`` in 1 .. 255.  Samples in no segment are not touched.  Everything ``mrx_tod_segment_flag`` refuses, and
    bounds that do not ascend, raise ValueError before any device call."""
    import torch

    from ._lib import ptr

    if not isinstance(flags, torch.Tensor) or flags.dim() != 2 or flags.dtype != torch.uint8 or flags.shape[0] < 1 or flags.shape[1] < 1:
        raise ValueError("flags must be a [D, T] uint8 tensor with D >= 1 and T >= 1")
    D, T = int(flags.shape[0]), int(flags.shape[1])
    ld_f = check_like(flags, "flags", flags, D, T, "uint8")
    d_bounds, S = _check_bounds(bounds, flags)
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (D, S) or mask.device != flags.device:
        raise ValueError(f"mask must be a [{D}, {S}] bool or uint8 tensor on the flags' device")
    if isinstance(value, bool) or int(value) != value or not 1 <= int(value) <= 255:
        raise ValueError(f"value {value}: an integer in 1 .. 255")
    if not flags.is_cuda:
        raise ValueError("flags must be a device tensor")
    d_mask = mask.to(torch.uint8).contiguous()
    context(ctx, flags).call("mrx_tod_segment_flag", ptr(flags), ld_f, D, T, ptr(d_bounds), S, ptr(d_mask), int(value))
    return flags


def _group_median(vals, g, G):
    """[G] float64: the median (the mean of the two middle values) of ``vals`` in every group ``g`` (0 .. G - 1); NaN for
    a group without a value; ``vals`` holds at least one.  One sort by value, one stable sort by group."""
    import torch

    order = torch.argsort(vals)
    order = order[torch.argsort(g[order], stable=True)]
    ranked = vals[order]
    count = torch.bincount(g, minlength=G)
    start = torch.cumsum(count, 0) - count
    some = count > 0
    last = int(ranked.numel()) - 1  # an empty group's start may lie past the end
    a = (start + torch.clamp(count - 1, min=0) // 2).clamp(max=last)
    b = (start + count // 2).clamp(max=last)
    return torch.where(some, (ranked[a] + ranked[b]) / 2.0, torch.full_like(ranked[a], float("nan")))


def find_outliers(v, groups, n_sigma, side="both", eligible=None, min_rel_scale=None):
    """``(outlier, unusable)``, two bool tensors of v's shape.  Per group over the entries of the float64 tensor ``v``
    that are eligible and finite: med = their median, scale = 1.4826 median|v - med|; an entry is an outlier iff
    scale > 0 and v - med > n_sigma scale (``side`` "high"), med - v > n_sigma scale ("low") or |v - med| > n_sigma scale
    ("both").  ``groups``: None (one group) or integers of v's shape (array or tensor), -1 leaving an entry out of
    everything.  ``eligible``: None (all) or a bool tensor of v's shape.  An entry in a group that is not eligible or not
    finite is ``unusable``, and no outlier.  ``min_rel_scale``: None, or a float64 tensor of v's shape: the entry is judged
    with max(scale, min_rel_scale |med|) in place of scale (what the entry's own estimate scatters by, where that is
    known)."""
    import torch

    if not isinstance(v, torch.Tensor) or v.dtype != torch.float64:
        raise ValueError("v must be a float64 tensor")
    if side not in SIDES:
        raise ValueError(f"side {side!r}: one of {SIDES}")
    n_sigma = float(n_sigma)
    if not np.isfinite(n_sigma) or n_sigma <= 0:
        raise ValueError(f"n_sigma {n_sigma}: finite and > 0")
    if groups is None:
        g = torch.zeros(v.shape, dtype=torch.int64, device=v.device)
    else:
        g = groups if isinstance(groups, torch.Tensor) else torch.as_tensor(np.asarray(groups))
        if g.dtype not in (torch.int32, torch.int64) or tuple(g.shape) != tuple(v.shape):
            raise ValueError(f"groups must be integers of v's shape {tuple(v.shape)}")
        g = g.to(v.device, torch.int64)
        if g.numel() and int(g.min()) < -1:
            raise ValueError("groups must be >= -1")
    if eligible is None:
        eligible = torch.ones(v.shape, dtype=torch.bool, device=v.device)
    elif not isinstance(eligible, torch.Tensor) or eligible.dtype != torch.bool or tuple(eligible.shape) != tuple(v.shape) or eligible.device != v.device:
        raise ValueError("eligible must be a bool tensor of v's shape on its device")
    if min_rel_scale is not None and (not isinstance(min_rel_scale, torch.Tensor) or min_rel_scale.dtype != torch.float64
                                      or tuple(min_rel_scale.shape) != tuple(v.shape) or min_rel_scale.device != v.device):
        raise ValueError("min_rel_scale must be a float64 tensor of v's shape on its device")
    shape = v.shape
    v, g, eligible = v.reshape(-1), g.reshape(-1), eligible.reshape(-1)
    grouped = g >= 0
    ok = grouped & eligible & torch.isfinite(v)
    unusable = grouped & ~ok
    outlier = torch.zeros_like(ok)
    if bool(ok.any()):
        G = int(g.max()) + 1
        idx = torch.nonzero(ok)[:, 0]
        vals, gi = v[idx], g[idx]
        med = _group_median(vals, gi, G)
        dev = vals - med[gi]
        scale = (MAD_TO_SIGMA * _group_median(dev.abs(), gi, G))[gi]
        if min_rel_scale is not None:
            scale = torch.maximum(scale, min_rel_scale.reshape(-1)[idx] * med[gi].abs())
        far = {"both": dev.abs(), "high": dev, "low": -dev}[side]
        outlier[idx] = (scale > 0) & (far > n_sigma * scale)
    return outlier.reshape(shape), unusable.reshape(shape)


CRITERIA = ("white", "rms", "skew", "kurtosis", "flagged")


def _check_rules(n_sigma, n_sigma_segment, max_flagged, max_bad_segments, min_hits, criteria):
    """(criteria as a tuple, the least number of kept samples) of ``decide``'s parameters, or ValueError."""
    criteria = (criteria,) if isinstance(criteria, str) else tuple(criteria)
    if not criteria or any(c not in CRITERIA for c in criteria):
        raise ValueError(f"criteria {criteria}: one or more of {CRITERIA}")
    min_hits = check_min_hits(min_hits, allow_bool=False)
    for name, f in (("max_flagged", max_flagged), ("max_bad_segments", max_bad_segments)):
        if not 0.0 <= float(f) <= 1.0:
            raise ValueError(f"{name} {f}: in [0, 1]")
    for name, f in (("n_sigma", n_sigma), ("n_sigma_segment", n_sigma_segment)):
        if not (f is None and name == "n_sigma_segment") and not (np.isfinite(float(f)) and float(f) > 0):
            raise ValueError(f"{name} {f}: finite and > 0")
    return criteria, max(min_hits, 1)


def bad_segments(seg, groups=None, n_sigma_segment=5.0, min_hits=8):
    """[D, S] bool: the noisy segments of the summary ``seg`` of ``summarize``.  A bad segment: max(min_hits, 1) samples
    and a pair kept, and its sigma_diff more than ``n_sigma_segment`` scales above the median of that detector's own
    such segments (None: no segment is judged); the scale is the robust one or sqrt(0.75 / p) of the median, whichever is
    larger: the sigma_diff of p pairs of white noise scatters by that much of itself, which a dozen full segments
    estimate poorly and a short one (the last, cut-off subscan) exceeds.  A detector whose group is -1 is not judged."""
    import torch

    _, floor = _check_rules(1.0, n_sigma_segment, 0.0, 0.0, min_hits, CRITERIA)
    D, S = seg["hits"].shape
    dev = seg["hits"].device
    if n_sigma_segment is None:
        return torch.zeros((D, S), dtype=torch.bool, device=dev)
    rows = torch.arange(D, device=dev)
    if groups is not None:
        g = (groups if isinstance(groups, torch.Tensor) else torch.as_tensor(np.asarray(groups))).to(dev, torch.int64)
        if tuple(g.shape) != (D,):
            raise ValueError(f"groups must be [{D}] integers")
        rows = torch.where(g >= 0, rows, -1)
    own = torch.sqrt(SIGMA_DIFF_SCATTER / torch.clamp(seg["pairs"].to(torch.float64), min=1.0))
    bad, _ = find_outliers(seg["sigma_diff"], rows[:, None].expand(D, S), n_sigma_segment, "high", (seg["hits"] >= floor) & (seg["pairs"] > 0), own)
    return bad


def decide(det, seg, bad, groups=None, n_sigma=5.0, max_flagged=0.5, max_bad_segments=0.5, min_hits=8, criteria=CRITERIA):
    """``(masks, cut_detectors [D] bool)``: the whole-detector rules of ``TOD.cut`` on the summaries ``det`` ([D, 1], the
    whole row as one segment, taken with the bad segments flagged, with ``flagged_fraction``) and ``seg`` ([D, S]) of
    ``summarize`` and ``bad`` of ``bad_segments``; plain torch on their device, so it runs on host tensors as well.  A
    detector is eligible with at least max(min_hits, 1) samples kept.  ``masks``, [D] bool each: per criterion in
    ``criteria`` the outliers within the detector's group (``find_outliers`` at ``n_sigma``, both sides) in log
    sigma_diff ("white"), log std ("rms"), "skew" and "kurtosis"; "flagged": flagged_fraction > max_flagged;
    "unusable": not eligible, or a value of one of those criteria not finite; "segments": more than
    ``max_bad_segments`` of the detector's non-empty segments (one sample kept or more) are bad.  A detector whose
    group is -1 is judged by nothing.  ``cut_detectors`` is the OR of the masks."""
    import torch

    criteria, floor = _check_rules(n_sigma, None, max_flagged, max_bad_segments, min_hits, criteria)
    hits = det["hits"][:, 0]
    D, S = seg["hits"].shape
    dev = hits.device
    if groups is None:
        g = torch.zeros(D, dtype=torch.int64, device=dev)
    else:
        g = (groups if isinstance(groups, torch.Tensor) else torch.as_tensor(np.asarray(groups))).to(dev, torch.int64)
        if tuple(g.shape) != (D,):
            raise ValueError(f"groups must be [{D}] integers")
    eligible = hits >= floor
    values = {"white": torch.log(det["sigma_diff"][:, 0]), "rms": torch.log(det["std"][:, 0]), "skew": det["skew"][:, 0],
              "kurtosis": det["kurtosis"][:, 0]}
    masks = {}
    unusable = (g >= 0) & ~eligible
    for name, v in values.items():
        if name in criteria:
            masks[name], u = find_outliers(v, g, n_sigma, "both", eligible)
            unusable = unusable | u
    if "flagged" in criteria:
        masks["flagged"] = (g >= 0) & (det["flagged_fraction"][:, 0] > float(max_flagged))
    masks["unusable"] = unusable
    nonempty = (seg["hits"] > 0).sum(dim=1)
    masks["segments"] = (g >= 0) & (bad.sum(dim=1).to(torch.float64) > float(max_bad_segments) * nonempty.to(torch.float64))
    cut = torch.zeros(D, dtype=torch.bool, device=dev)
    for m in masks.values():
        cut = cut | m
    return masks, cut


def inject_bad(data, bounds, *, noisy=(), spiky=(), dead=(), noisy_segments=(), seed, factor=6.0, spike_rate=0.02, spike_sigma=12.0,
               dead_level=1e-3):
    """``(out, touched)``: a float32 copy of the host array ``data`` [D, T] with the defects that cuts exist for, and the
    [D, T] bool mask of the samples that were changed (for tests and demonstrations).  With sigma the row's own white
    level, sqrt(mean(diff^2) / 2):

        noisy           rows that gain factor sigma N(0, 1)
        spiky           rows that gain +-spike_sigma sigma at a fraction spike_rate of their samples
        dead            rows replaced by their mean plus dead_level sigma N(0, 1)
        noisy_segments  (row, segment) pairs of ``bounds`` that gain factor sigma N(0, 1)

    Every draw comes from ``numpy.random.default_rng(seed)``, rows in the order given."""
    x = np.array(data, np.float32)
    if x.ndim != 2 or x.shape[1] < 2:
        raise ValueError("data must be a [D, T] array with T >= 2")
    D, T = x.shape
    b = np.clip(np.asarray(bounds, np.int64), 0, T)
    if b.ndim != 1 or b.size < 2 or np.any(np.diff(b) < 0):
        raise ValueError("bounds must be a one-dimensional array of S + 1 >= 2 ascending integers")
    rows = [int(d) for d in (*noisy, *spiky, *dead)] + [int(d) for d, _ in noisy_segments]
    if any(not 0 <= d < D for d in rows) or any(not 0 <= int(s) < b.size - 1 for _, s in noisy_segments):
        raise ValueError(f"rows must be in 0 .. {D - 1} and segments in 0 .. {b.size - 2}")
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(np.mean(np.diff(x.astype(np.float64), axis=1) ** 2, axis=1) / 2.0)
    touched = np.zeros((D, T), bool)
    for d in noisy:
        x[d] += (factor * sigma[d] * rng.standard_normal(T)).astype(np.float32)
        touched[d] = True
    for d in spiky:
        hit = rng.random(T) < spike_rate
        x[d, hit] += (spike_sigma * sigma[d] * rng.choice([-1.0, 1.0], int(hit.sum()))).astype(np.float32)
        touched[d] |= hit
    for d in dead:
        x[d] = (x[d].astype(np.float64).mean() + dead_level * sigma[d] * rng.standard_normal(T)).astype(np.float32)
        touched[d] = True
    for d, s in noisy_segments:
        lo, hi = int(b[s]), int(b[s + 1])
        x[d, lo:hi] += (factor * sigma[d] * rng.standard_normal(hi - lo)).astype(np.float32)
        touched[d, lo:hi] = True
    return x, touched
