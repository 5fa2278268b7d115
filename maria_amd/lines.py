"""Narrow spectral lines (pulse-tube lines and their harmonics, aliased mains, microphonic resonances): found in the Welch
spectrum, tracked per detector, fitted per (detector, time chunk) as an amplitude and a phase and subtracted on the
device, flagged samples left out of every sum (``mrx_tod_line_normal``, ``mrx_tod_line_apply``).

``bounds`` [S + 1] int32, ascending, cuts a row of T samples into S segments as in ``maria_amd.subscans``
(``cuts.chunk_bounds`` gives uniform chunks).  ``nu`` [D, L] float64 holds the frequency of each of L <= 3 lines in each
row, in cycles a sample, in (0, 0.5].  In a segment [lo, hi) the basis of row d has K = n_poly + 2 L functions:

    B_0 = 1, B_1 = u(t)                             the first n_poly <= 2 of them (subscans' u and P_0, P_1): a local baseline
    theta = nu[d, l] * t,  q = theta - rint(theta)  t from the start of the ROW: the phase is continuous across segments
    B_{n_poly + 2 l} = cospi(2 q),  B_{n_poly + 2 l + 1} = sinpi(2 q)
    N[d, s, i, j] = sum over the segment's t with flags[d, t] == 0 of B_i B_j;   r[d, s, i] = of B_i term(d, t)
    y[d, t]       = x[d, t] + sign * float32(sum over i = n_poly .. K - 1, in order, of a[d, s, i] B_i)

The carriers are evaluated in the kernels, in float64, each at its own sample, and never stored.  Only the carriers are
subtracted: the baseline terms are nuisance parameters and stay in the data.  A line a cos(2 pi nu t) + b sin(2 pi nu t) is
A cos(2 pi nu t + phi) with A = hypot(a, b) and phi = atan2(-b, a) (``amplitude_phase``).  Every sum is added in a fixed
order, without atomics; the order of the operations is written out in include/mrx.h, and tests/lines_ref.py restates
it in numpy.  ``find_lines``, ``phase_slope`` and ``line_groups`` are host functions in float64."""

from __future__ import annotations

import numpy as np

from ._tod_args import check_like, check_min_hits, check_out, check_sign, check_x, context, row_pitch, to_numpy
from .regress import solve
from .subscans import _check_bounds

MAX_LINES = 3  # mrx_lines.hip: kMaxLines, the lines of one call
MAX_POLY = 2   # mrx_lines.hip: kMaxPoly, the baseline functions beside them


def _check_n_poly(n_poly):
    if isinstance(n_poly, bool) or int(n_poly) != n_poly or not 0 <= int(n_poly) <= MAX_POLY:
        raise ValueError(f"n_poly {n_poly}: an integer in 0 .. {MAX_POLY}")
    return int(n_poly)


def _check_nu(nu, D):
    """[D, L] float64 (numpy) of ``nu`` ([D, L] or [L], an array or a tensor): 1 .. 3 lines, every entry finite and in
    (0, 0.5] cycles a sample."""
    nu = np.asarray(to_numpy(nu), np.float64)
    if nu.ndim == 1:
        nu = np.broadcast_to(nu[None, :], (D, nu.size))
    if nu.ndim != 2 or nu.shape[0] != D or not 1 <= nu.shape[1] <= MAX_LINES:
        raise ValueError(f"nu must be a [{D}, L] or [L] float64 array with L in 1 .. {MAX_LINES}")
    if not (np.all(np.isfinite(nu)) and np.all(nu > 0.0) and np.all(nu <= 0.5)):
        raise ValueError("nu: every frequency must be finite and in (0, 0.5] cycles a sample")
    return np.ascontiguousarray(nu)


def normal_equations(x, bounds, nu, n_poly=1, flags=None, model=None, ctx=None):
    """``(N, r, hits)`` of every (row, segment) of ``x`` ([D, T] float32 device tensor, any row pitch) against the basis
    above: [D, S, K, K] float64, [D, S, K] float64 and [D, S] int64 device tensors, K = n_poly + 2 L; an empty segment
    gets zeros.  ``nu`` [D, L] or [L] float64, checked on the host.  ``flags`` [D, T] uint8 and ``model`` [D, T] float32,
    any row pitch.  Everything ``mrx_tod_line_normal`` refuses, a frequency outside (0, 0.5] and bounds that do not ascend
    raise ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    n_poly = _check_n_poly(n_poly)
    nu = _check_nu(nu, D)
    L = nu.shape[1]
    K = n_poly + 2 * L
    d_bounds, S = _check_bounds(bounds, x)
    ld_f = check_like(flags, "flags", x, D, T, "uint8") if flags is not None else 0
    ld_m = check_like(model, "model", x, D, T) if model is not None else 0
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    d_nu = torch.as_tensor(nu).to(x.device)
    N = torch.empty((D, S, K, K), dtype=torch.float64, device=x.device)
    r = torch.empty((D, S, K), dtype=torch.float64, device=x.device)
    hits = torch.empty((D, S), dtype=torch.int32, device=x.device)
    context(ctx, x).call("mrx_tod_line_normal", ptr(x), ld_x, ptr(model), ld_m, ptr(flags), ld_f, D, T, ptr(d_bounds), S, ptr(d_nu), L, n_poly,
                         ptr(N), ptr(r), ptr(hits))
    return N, r, hits.to(torch.int64)


def _check_solve(min_hits, rcond):
    min_hits = check_min_hits(min_hits)
    if not 0.0 <= float(rcond) < 1.0:
        raise ValueError(f"rcond {rcond}: in [0, 1)")
    return min_hits, float(rcond)


def fit(x, bounds, nu, n_poly=1, flags=None, model=None, min_hits=8, rcond=1e-10, ctx=None):
    """``(a [D, S, K] float64, ok [D, S] bool)``: every (row, segment)'s least-squares coefficients of the basis,
    ``regress.solve`` of ``normal_equations`` on their [D S, ..] views with its ``min_hits`` and ``rcond``: a pair that is
    not ok (fewer than max(min_hits, K) samples kept, or a basis degenerate on them: a segment shorter than a line's
    period, two lines closer than the inverse of its length) gets a = 0."""
    min_hits, rcond = _check_solve(min_hits, rcond)
    N, r, hits = normal_equations(x, bounds, nu, n_poly=n_poly, flags=flags, model=model, ctx=ctx)
    D, S, K = r.shape
    a, ok = solve(N.view(D * S, K, K), r.view(D * S, K), hits.view(D * S), min_hits=min_hits, rcond=rcond)
    return a.view(D, S, K), ok.view(D, S)


def apply(x, bounds, nu, a, n_poly, sign=-1, out=None, ctx=None):
    """y = x + sign * float32(sum over the carriers of a[d, s, i] B_i) (sign -1 or +1) of a [D, T] float32 device tensor
    ``x`` (any row pitch) and coefficients ``a`` [D, S, n_poly + 2 L] float64, whose first ``n_poly`` entries are not
    read; samples in no segment are copied.  Returns ``out`` (None: a new tensor; ``x`` itself: in place; otherwise a
    [D, T] float32 tensor of any row pitch that does not overlap x).  Everything ``mrx_tod_line_apply`` refuses, a
    frequency outside (0, 0.5] and bounds that do not ascend raise ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    n_poly = _check_n_poly(n_poly)
    nu = _check_nu(nu, D)
    L = nu.shape[1]
    K = n_poly + 2 * L
    d_bounds, S = _check_bounds(bounds, x)
    if not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or tuple(a.shape) != (D, S, K) or a.device != x.device:
        raise ValueError(f"a must be a [{D}, {S}, {K}] float64 tensor on x's device")
    a = a.contiguous()
    sign = check_sign(sign)
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    else:
        check_out(out, x, D, T, in_place=True)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    d_nu = torch.as_tensor(nu).to(x.device)
    context(ctx, x).call("mrx_tod_line_apply", ptr(x), ld_x, D, T, ptr(d_bounds), S, ptr(d_nu), L, n_poly, ptr(a), sign, ptr(out), row_pitch(out))
    return out


def amplitude_phase(a, n_poly):
    """``(A, phi)`` [D, S, L] of coefficients ``a`` [D, S, n_poly + 2 L] (a tensor gives tensors, an array arrays): the
    line of a segment is A cos(2 pi nu t + phi), A = hypot(a_c, a_s) and phi = atan2(-a_s, a_c)."""
    n_poly = _check_n_poly(n_poly)
    if a.ndim != 3 or a.shape[2] <= n_poly or (a.shape[2] - n_poly) % 2 or (a.shape[2] - n_poly) // 2 > MAX_LINES:
        raise ValueError(f"a must be [D, S, {n_poly} + 2 L] with L in 1 .. {MAX_LINES}")
    import torch

    c, s = a[:, :, n_poly::2], a[:, :, n_poly + 1::2]
    if isinstance(a, torch.Tensor):
        return torch.hypot(c, s), torch.atan2(-s, c)
    return np.hypot(c, s), np.arctan2(-s, c)


def line_groups(n):
    """The lines 0 .. n - 1 (in ascending frequency) in groups of at most ``MAX_LINES`` neighbours: a list of ranges."""
    return [range(lo, min(lo + MAX_LINES, n)) for lo in range(0, n, MAX_LINES)]


def _check_groups(groups, D):
    if groups is None:
        return np.zeros(D, np.int64)
    g = np.asarray(to_numpy(groups))
    if g.ndim != 1 or g.size != D or g.dtype.kind not in "iu" or (g.size and g.min() < -1):
        raise ValueError(f"groups must be {D} integers >= -1, one per row")
    return g.astype(np.int64)


def running_median(y, half_window):
    """The median of the 2 half_window + 1 values around each entry of ``y``, the ends repeated beyond the array."""
    h = int(half_window)
    padded = np.pad(np.asarray(y, np.float64), h, mode="edge")
    return np.median(np.lib.stride_tricks.sliding_window_view(padded, 2 * h + 1), axis=-1)


def find_lines(f, psd, groups=None, n_sigma=6.0, half_window=16, f_min=None, f_max=None, max_lines=None):
    """The narrow lines of the spectra ``psd`` [D, F] (or [F]) at the frequencies ``f`` [F] (arrays or tensors;
    ``TOD.psd``), per group of rows, on the host in float64: a list with one float64 array of frequencies per group
    (``groups`` None: one group; an entry of -1 takes part in nothing), strongest first.  For a group:

        y     = log(median over its rows of psd[d] / median_f(psd[d]))
        z     = y - running_median(y, half_window);   sigma = 1.4826 median|z - median z| over the inner bins
        lines = the runs of adjacent bins with z > n_sigma sigma, among the bins that are not within ``half_window`` of
                either end of the spectrum (the 1 / f slope makes a false line in the lowest bins) and lie in
                f_min .. f_max; a run's frequency is the centroid of the excess power max(exp(y) - exp(running median), 0)
                over the run and one bin either side, its strength the largest z in it.

    ``max_lines``: keep the strongest ones only."""
    f = np.asarray(to_numpy(f), np.float64)
    p = np.asarray(to_numpy(psd), np.float64)
    if p.ndim == 1:
        p = p[None, :]
    h = int(half_window)
    if isinstance(half_window, bool) or h != half_window or h < 1:
        raise ValueError(f"half_window {half_window}: an integer >= 1")
    if f.ndim != 1 or p.ndim != 2 or p.shape[1] != f.size or p.shape[0] < 1:
        raise ValueError("f must be [F] and psd [D, F]")
    if f.size < 4 * h + 3:
        raise ValueError(f"a spectrum of {f.size} bins: at least 4 half_window + 3 = {4 * h + 3}")
    if not np.all(np.diff(f) > 0):
        raise ValueError("f must ascend")
    if not (np.isfinite(float(n_sigma)) and float(n_sigma) > 0):
        raise ValueError(f"n_sigma {n_sigma}: finite and > 0")
    if max_lines is not None and (int(max_lines) != max_lines or int(max_lines) < 0):
        raise ValueError(f"max_lines {max_lines}: None or an integer >= 0")
    g = _check_groups(groups, p.shape[0])
    lo = -np.inf if f_min is None else float(f_min)
    hi = np.inf if f_max is None else float(f_max)
    F = f.size
    inner = np.zeros(F, bool)
    inner[h:F - h] = True
    allowed = inner & (f >= lo) & (f <= hi)
    found = []
    for k in range(int(g.max()) + 1 if g.size and g.max() >= 0 else 0):
        rows = p[g == k]
        rows = rows[np.all(np.isfinite(rows), axis=1)] if rows.size else rows
        if rows.shape[0] == 0:
            found.append(np.zeros(0))
            continue
        level = np.median(rows, axis=1)
        rows = rows[level > 0] / level[level > 0, None]
        if rows.shape[0] == 0:
            found.append(np.zeros(0))
            continue
        spec = np.median(rows, axis=0)
        y = np.log(np.maximum(spec, np.finfo(np.float64).tiny))
        base = running_median(y, h)
        z = y - base
        sigma = 1.4826 * float(np.median(np.abs(z[inner] - np.median(z[inner]))))
        hot = allowed & (z > float(n_sigma) * sigma) if sigma > 0 else np.zeros(F, bool)
        idx = np.flatnonzero(hot)
        lines = []
        if idx.size:
            breaks = np.flatnonzero(np.diff(idx) > 1)
            starts, ends = np.concatenate([[0], breaks + 1]), np.concatenate([breaks, [idx.size - 1]])
            excess = np.maximum(np.exp(y) - np.exp(base), 0.0)
            for s, e in zip(starts, ends):
                i0, i1 = int(idx[s]), int(idx[e])
                j0, j1 = max(i0 - 1, 0), min(i1 + 1, F - 1)
                w = excess[j0:j1 + 1]
                lines.append((float(z[i0:i1 + 1].max()), float((w * f[j0:j1 + 1]).sum() / w.sum())))
        lines.sort(key=lambda t: -t[0])
        if max_lines is not None:
            lines = lines[:int(max_lines)]
        found.append(np.array([v for _, v in lines], np.float64))
    return found


def segment_centres(bounds, T):
    """(centre [S] float64, nonempty [S] bool) of the segments of ``bounds`` clamped to 0 .. T: (lo + hi - 1) / 2."""
    b = np.clip(np.asarray(to_numpy(bounds)).astype(np.int64), 0, int(T))
    lo, hi = b[:-1], b[1:]
    return (lo + hi - 1) / 2.0, hi > lo


def phase_slope(a, ok, bounds, T, n_poly, groups=None, per_detector=True):
    """[D, L] float64: the frequency correction, in cycles a sample, that the fitted phases of consecutive segments ask
    for.  A line fitted at nu that really runs at nu + dnu shows the phase phi_s = phi + 2 pi dnu c_s in the segment
    centred on c_s, so for every pair of consecutive non-empty segments that are both ok

        dnu = wrap(phi_{s'} - phi_s) / (2 pi (c_{s'} - c_s)),   wrap to [-pi, pi)

    and a row's correction is the median over its pairs (0 where it has none).  The premise is |dnu| (c_{s'} - c_s) < 1/2.
    ``per_detector`` False: every row of a group gets the median of the corrections of the group's rows that have one."""
    a, ok = np.asarray(to_numpy(a), np.float64), np.asarray(to_numpy(ok)).astype(bool)
    _, phi = amplitude_phase(a, n_poly)
    D, S, L = phi.shape
    centre, nonempty = segment_centres(bounds, T)
    if centre.size != S or ok.shape != (D, S):
        raise ValueError(f"a of {S} segments: bounds has {centre.size}, ok has shape {ok.shape}")
    use = np.flatnonzero(nonempty)
    out = np.zeros((D, L))
    have = np.zeros(D, bool)
    if use.size >= 2:
        first, second = use[:-1], use[1:]
        gap = centre[second] - centre[first]
        both = ok[:, first] & ok[:, second]  # [D, pairs]
        dphi = phi[:, second, :] - phi[:, first, :]
        dphi = dphi - 2.0 * np.pi * np.floor(dphi / (2.0 * np.pi) + 0.5)
        dnu = dphi / (2.0 * np.pi * gap[None, :, None])
        for d in range(D):
            if both[d].any():
                out[d], have[d] = np.median(dnu[d, both[d]], axis=0), True
    if not per_detector:
        g = _check_groups(groups, D)
        for k in np.unique(g[g >= 0]):
            rows = g == k
            if (rows & have).any():
                out[rows] = np.median(out[rows & have], axis=0)[None, :]
    return out


def refine(x, bounds, nu, n_iter=2, per_detector=True, n_poly=1, flags=None, model=None, groups=None, min_hits=8, rcond=1e-10, ctx=None):
    """``nu`` [D, L] float64 (numpy) tracked per detector: ``n_iter`` rounds of one ``fit`` each on the segments of
    ``bounds``, followed by nu <- nu + ``phase_slope`` of the fitted phases (kept inside (0, 0.5]).  The starting error
    times the spacing of the segments must stay below half a cycle: with frequencies known to a Welch bin of ``nperseg``
    samples the segments must not be longer than ``nperseg`` (``TOD.remove_lines`` refuses them)."""
    D, T, _ = check_x(x)
    nu = _check_nu(nu, D).copy()
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or int(n_iter) < 0:
        raise ValueError(f"n_iter {n_iter}: an integer >= 0")
    g = _check_groups(groups, D)
    for _ in range(int(n_iter)):
        a, ok = fit(x, bounds, nu, n_poly=n_poly, flags=flags, model=model, min_hits=min_hits, rcond=rcond, ctx=ctx)
        step = phase_slope(a, ok, bounds, T, n_poly, groups=g, per_detector=per_detector)
        nu = np.clip(nu + step, np.finfo(np.float64).tiny, 0.5)
    return nu


def inject_lines(x, freqs, amps, phases, fs, out=None, ctx=None):
    """``x`` plus the lines amps cos(2 pi freqs t / fs + phases) (each [L] or [D, L]; freqs in the units of ``fs``):
    ``apply`` with sign +1 on one whole-row segment, ``MAX_LINES`` lines a call (for tests and demonstrations).  Returns
    ``out`` (None: a new tensor; ``x``: in place)."""
    import torch

    D, T, _ = check_x(x)
    fs = float(fs)
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError(f"fs {fs}: finite and > 0")
    wide = [np.asarray(to_numpy(v), np.float64) for v in (freqs, amps, phases)]
    wide = [np.broadcast_to(v[None, :], (D, v.size)) if v.ndim == 1 else v for v in wide]
    n = wide[0].shape[1] if wide[0].ndim == 2 else 0
    if n < 1 or any(v.ndim != 2 or v.shape != (D, n) for v in wide):
        raise ValueError(f"freqs, amps and phases must be [L] or [{D}, L] arrays of one shape, L >= 1")
    nu, amp, phi = wide[0] / fs, wide[1], wide[2]
    for k in line_groups(n):  # every refusal before the first launch
        _check_nu(nu[:, list(k)], D)
    bounds = np.array([0, T], np.int32)
    src = x
    for k in line_groups(n):
        k = list(k)
        a = np.empty((D, 1, 2 * len(k)))
        a[:, 0, 0::2], a[:, 0, 1::2] = amp[:, k] * np.cos(phi[:, k]), -amp[:, k] * np.sin(phi[:, k])
        out = apply(src, bounds, nu[:, k], torch.as_tensor(a).to(x.device), 0, sign=+1, out=out, ctx=ctx)
        src = out
    return out
