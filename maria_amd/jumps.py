"""Jumps of a [D, T] TOD on the device: find them, measure them, take them out (``mrx_tod_step_stat``,
``mrx_tod_jump_find``, ``mrx_tod_jump_height``, ``mrx_tod_jump_fix``).

A jump is a sudden, persistent change of a row's baseline (a flux jump of a SQUID read-out, a tracking reset).  With
w = window, g = gap, m = min_count, and a sample VALID if it is inside the row and its flag is 0:

    s[d, t]     = mean of the valid samples of [t + g, t + g + w) - mean of those of [t - g - w, t - g), float64 rounded
                  once to float32; 0 where either side has fewer than m valid samples
    scale[d]    = 1.4826 * the lower median of |s[d, :]|                   (element (T - 1) // 2 of the sorted row)
    peak        : |s[t]| > float32(n_sigma * scale[d]) (strict), |s[u]| < |s[t]| on [t - sep, t), |s[u]| <= |s[t]| on
                  (t, t + sep]: the earliest sample of a plateau, and two peaks are more than sep apart
    flags[d, t] = 1 at a peak, else 2 where a peak p has t - grow_after <= p <= t + grow_before, else 0
    height      : the same difference of means at a jump p, in float64, over [lo, p - g) and [p + g, hi) with
                  lo = max(0, p - g - w, p- + g), hi = min(T, p + g + w, p+ - g) for the row's neighbouring jumps p-, p+
    fix         : y[d, t] = float32(x[d, t] - the sum of the heights of the row's jumps at or before t)

The jumps of a TOD are a list, row after row: ``row_start`` [D + 1] int32 (row d owns ``pos[row_start[d] :
row_start[d + 1]]``) and ``pos`` [n] int32, ascending within a row.  The finder and the fix are comparisons and one
rounded subtraction: reproducible bit for bit.  Inputs must be finite."""

from __future__ import annotations

import numpy as np

from ._tod_args import check_like, check_out, check_scratch_bytes, check_x, context, row_pitch, to_numpy
from .flagging import MAD_TO_SIGMA, _check_grow, _threshold

TILE_SAMPLES = 1024  # consecutive samples of a row one workgroup takes (mrx_jumps.hip: kTileSamples)
MAX_WINDOW = 256
MAX_GAP = 64
MAX_SEP = 512


def _check_window(window, gap, min_count):
    """(w, g, m) as integers; ``min_count`` None is ``window // 2``."""
    if int(window) != window or not 2 <= int(window) <= MAX_WINDOW:
        raise ValueError(f"window {window}: an integer in 2 .. {MAX_WINDOW}")
    if int(gap) != gap or not 0 <= int(gap) <= MAX_GAP:
        raise ValueError(f"gap {gap}: an integer in 0 .. {MAX_GAP}")
    w = int(window)
    if min_count is None:
        min_count = w // 2
    if int(min_count) != min_count or not 1 <= int(min_count) <= w:
        raise ValueError(f"min_count {min_count}: an integer in 1 .. window = {w}")
    return w, int(gap), int(min_count)


def _check_sep(sep, window):
    if sep is None:
        sep = window
    if int(sep) != sep or not 1 <= int(sep) <= MAX_SEP:
        raise ValueError(f"sep {sep}: an integer in 1 .. {MAX_SEP}")
    return int(sep)


def _check_lists(row_start, pos, D, x):
    """(row_start, pos) as int32 tensors on x's device, n; the lists must be what the definitions ask for."""
    rs, ps = np.asarray(to_numpy(row_start)), np.asarray(to_numpy(pos))
    if rs.ndim != 1 or rs.shape[0] != D + 1 or rs.dtype.kind not in "iu":
        raise ValueError(f"row_start must be {D + 1} integers")
    if ps.ndim != 1 or (ps.size and ps.dtype.kind not in "iu"):
        raise ValueError("pos must be a one-dimensional integer array")
    n = int(ps.size)
    rs = rs.astype(np.int64)
    if rs[0] != 0 or rs[-1] != n or np.any(np.diff(rs) < 0):
        raise ValueError(f"row_start must not decrease, from 0 to len(pos) = {n}")
    ps = ps.astype(np.int64)
    T = int(x.shape[1])
    if n and (ps.min() < 0 or ps.max() >= T):
        raise ValueError(f"pos must lie in 0 .. T - 1 = {T - 1}")
    inner = np.ones(n, bool)
    inner[rs[:-1][rs[:-1] < n]] = False  # the first jump of a row has no one before it
    if n and np.any((np.diff(ps, prepend=ps[:1]) < 0) & inner):
        raise ValueError("pos must ascend within a row")
    return rs.astype(np.int32), ps.astype(np.int32), n


def step_statistic(x, window, gap=0, flags=None, min_count=None, ctx=None, out=None):
    """The step statistic s of a [D, T] float32 device tensor ``x`` (any row pitch) as a [D, T] float32 device tensor:
    the mean of the ``window`` valid samples from t + gap on less that of those before t - gap, 0 where a side has fewer
    than ``min_count`` (None: window // 2) of them.  ``flags``: [D, T] uint8 (any row pitch), nonzero keeps a sample out
    of both means.  ``out``: a tensor to write into (any row pitch; its memory must not overlap ``x``'s).  Everything
    ``mrx_tod_step_stat`` refuses raises ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    w, g, m = _check_window(window, gap, min_count)
    ld_f = 0 if flags is None else check_like(flags, "flags", x, D, T, "uint8")
    if out is not None:
        check_out(out, x, D, T)
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    context(ctx, x).call("mrx_tod_step_stat", ptr(x), ld_x, ptr(flags), ld_f, D, T, w, g, m, ptr(out), row_pitch(out))
    return out


def robust_scale(s, scratch_bytes=1 << 30):
    """[D] float64 on s's device: 1.4826 times the lower median (``torch.median``'s rule) of |s| of every row of a
    [D, T] float32 tensor, the scale of a statistic that a few jumps do not move.  |s| is formed ``scratch_bytes //
    (4 T)`` rows at a time (at least one)."""
    import torch

    D, T, _ = check_x(s, "s")
    rows = max(1, min(D, check_scratch_bytes(scratch_bytes) // (4 * T)))
    scale = torch.empty(D, dtype=torch.float64, device=s.device)
    for d0 in range(0, D, rows):
        scale[d0:d0 + rows] = MAD_TO_SIGMA * torch.median(s[d0:d0 + rows].abs(), dim=1).values.double()
    return scale


def find_jumps(x, window=64, n_sigma=8.0, sep=None, grow=(4, 4), flags=None, min_count=None, sigma=None, ctx=None, scratch_bytes=1 << 30):
    """``(row_start, pos, jump_flags, count)`` of a [D, T] float32 device tensor ``x`` (any row pitch): the peaks of the
    step statistic of ``window`` at gap 0 above ``float32(n_sigma * sigma[d])``, at least ``sep`` + 1 (None: window + 1)
    samples apart.  ``sigma``: a scalar or [D] scale; None: ``robust_scale`` of the statistic itself, so that 1/f noise,
    which the difference of means does not average away, raises its own threshold.  ``flags``: samples kept out of the
    means.  row_start [D + 1] and pos [n] int32 list the peaks row after row (``torch.nonzero(jump_flags == 1)``);
    jump_flags [D, T] uint8 is 1 at a peak and 2 within ``grow = (before, after)`` samples of one; count [D] int64 the
    peaks of each row.  The statistic lives in a scratch of at most ``scratch_bytes`` (``scratch_bytes // (4 T)`` rows at a
    time, at least one).  Everything the two entries refuse raises ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    w, _, m = _check_window(window, 0, min_count)
    sep = _check_sep(sep, w)
    before, after = _check_grow(grow)
    ld_f = 0 if flags is None else check_like(flags, "flags", x, D, T, "uint8")
    thresh = None if sigma is None else _threshold(n_sigma, sigma, D)
    if sigma is None:
        _threshold(n_sigma, 0.0, D)
    rows = max(1, min(D, check_scratch_bytes(scratch_bytes) // (4 * T)))
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    ctx = context(ctx, x)
    buf = torch.empty((rows, T), dtype=torch.float32, device=x.device)
    jump_flags = torch.empty((D, T), dtype=torch.uint8, device=x.device)
    count = torch.empty(D, dtype=torch.int32, device=x.device)
    d_thresh = None if thresh is None else torch.as_tensor(thresh).to(x.device)
    for d0 in range(0, D, rows):
        n = min(rows, D - d0)
        s = step_statistic(x[d0:d0 + n], w, 0, flags=None if flags is None else flags[d0:d0 + n], min_count=m, ctx=ctx, out=buf[:n])
        if thresh is None:
            th = (float(n_sigma) * robust_scale(s)).float()
        else:
            th = d_thresh[d0:d0 + n]
        th = th.contiguous()
        f = jump_flags[d0:d0 + n]
        ctx.call("mrx_tod_jump_find", ptr(s), T, n, T, ptr(th), sep, before, after, ptr(f), T, ptr(count[d0:d0 + n]))
    count = count.to(torch.int64)
    at = torch.nonzero(jump_flags == 1)  # sorted by row, then by sample
    row_start = torch.zeros(D + 1, dtype=torch.int32, device=x.device)
    row_start[1:] = torch.cumsum(count, 0).to(torch.int32)
    return row_start, at[:, 1].to(torch.int32).contiguous(), jump_flags, count


def jump_heights(x, row_start, pos, window, gap, flags=None, min_count=None, ctx=None):
    """``(height, ok)`` of the listed jumps of ``x`` ([D, T] float32 device tensor, any row pitch): height [n] float64 the
    mean of the valid samples of [p + gap, hi) less that of [lo, p - gap), the windows ``window`` long and clipped
    ``gap`` samples short of the row's neighbouring jumps; ok [n] bool, False (and height 0) where a side has fewer than
    ``min_count`` (None: window // 2) valid samples.  ``gap`` keeps the samples next to the jump, where the position is
    uncertain and the detector's response settles, out of both means."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    w, g, m = _check_window(window, gap, min_count)
    ld_f = 0 if flags is None else check_like(flags, "flags", x, D, T, "uint8")
    rs, ps, n = _check_lists(row_start, pos, D, x)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    d_rs, d_ps = torch.as_tensor(rs).to(x.device), torch.as_tensor(ps).to(x.device)
    height = torch.zeros(n, dtype=torch.float64, device=x.device)
    ok = torch.zeros(n, dtype=torch.uint8, device=x.device)
    context(ctx, x).call("mrx_tod_jump_height", ptr(x), ld_x, ptr(flags), ld_f, D, T, ptr(d_rs), ptr(d_ps) if n else None, n, w, g, m,
                         ptr(height) if n else None, ptr(ok) if n else None)
    return height, ok.bool()


def cumulative_heights(row_start, height):
    """[n] float64 numpy: the inclusive cumulative sum of ``height`` within each row of the list, added in list order."""
    rs = np.asarray(row_start, np.int64)
    h = np.asarray(height, np.float64)
    cum = np.zeros(h.shape[0], np.float64)
    for d in range(rs.shape[0] - 1):
        cum[rs[d]:rs[d + 1]] = np.cumsum(h[rs[d]:rs[d + 1]])
    return cum


def fix_jumps(x, row_start, pos, height, out=None, ctx=None):
    """y = x less, at every sample, the sum of the ``height`` ([n] float64) of the row's listed jumps at or before it, as
    a [D, T] float32 device tensor: one float64 subtraction a sample, rounded once.  ``out``: a tensor to write into
    (any row pitch); ``out=x`` (or an equal view of x) works in place, any other overlap is refused.  The per-row cumulative sums are formed on the
    host in float64 (``cumulative_heights``): the lists are small."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    rs, ps, n = _check_lists(row_start, pos, D, x)
    h = np.asarray(to_numpy(height), np.float64)
    if h.shape != (n,) or not np.all(np.isfinite(h)):
        raise ValueError(f"height must be {n} finite numbers")
    if out is not None:
        check_out(out, x, D, T, in_place=True)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    d_rs = torch.as_tensor(rs).to(x.device)
    d_ps = torch.as_tensor(ps).to(x.device)
    d_cum = torch.as_tensor(cumulative_heights(rs, h)).to(x.device)
    context(ctx, x).call("mrx_tod_jump_fix", ptr(x), ld_x, D, T, ptr(d_rs), ptr(d_ps) if n else None, ptr(d_cum) if n else None, n,
                         ptr(out), row_pitch(out))
    return out


def draw_jumps(D, T, n_per_row, amplitude, seed, margin=0, spacing=1):
    """The host draw of ``inject_jumps``: ``(pos, heights)``, [D, n_per_row] int64 positions (ascending within a row)
    and float64 signed heights, from ``np.random.default_rng(seed)``.  The positions of a row are distinct nodes
    ``margin + k * spacing`` (those with node + spacing <= T - margin) plus ONE offset in 0 .. spacing - 1 common to the
    row, so that two jumps of a row are at least ``spacing`` apart and every jump at least ``margin`` from the row's
    ends.  The draw order: per row the nodes (``choice`` without replacement) and then the row's offset, then all signs,
    then all magnitudes (uniform in ``amplitude = (lo, hi)``, or the scalar)."""
    n = int(n_per_row)
    if int(margin) != margin or int(margin) < 0 or int(spacing) != spacing or int(spacing) < 1:
        raise ValueError(f"margin {margin}, spacing {spacing}: integers >= 0 and >= 1")
    margin, spacing = int(margin), int(spacing)
    nodes = max(0, (T - 2 * margin) // spacing)
    if n != n_per_row or not 0 <= n <= nodes:
        raise ValueError(f"n_per_row {n_per_row}: an integer in 0 .. {nodes}, the nodes of spacing {spacing} inside the margins")
    lo, hi = (amplitude, amplitude) if np.ndim(amplitude) == 0 else amplitude
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo < 0 or hi < lo:
        raise ValueError(f"amplitude {amplitude!r}: a finite scalar >= 0 or a pair 0 <= lo <= hi")
    rng = np.random.default_rng(seed)
    pos = np.zeros((D, n), np.int64)
    for d in range(D):
        k = np.sort(rng.choice(nodes, n, replace=False)) if n else np.zeros(0, np.int64)
        pos[d] = margin + k * spacing + int(rng.integers(0, spacing))
    sign = 2.0 * rng.integers(0, 2, (D, n)) - 1.0
    return pos, sign * rng.uniform(lo, hi, (D, n))


def inject_jumps(x, n_per_row, amplitude, seed, margin=0, spacing=1):
    """Add ``n_per_row`` jumps to every row of ``x`` ([D, T] float32 tensor, device or host) IN PLACE: the height from
    the jump's position to the row's end, positions and heights from ``draw_jumps``; the steps of a row are summed in
    float64 and added in one float32 addition a sample.  Returns ``(pos, heights)``.  An aid for robustness studies and the
    tests' input; a flux-jump component of the simulation is not built."""
    import torch

    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("x must be a [D, T] float32 tensor")
    D, T = x.shape
    pos, heights = draw_jumps(D, T, n_per_row, amplitude, seed, margin=margin, spacing=spacing)
    step = np.zeros((D, T), np.float64)
    for d in range(D):
        np.add.at(step[d], pos[d], heights[d])
    x.add_(torch.as_tensor(np.cumsum(step, axis=1).astype(np.float32)).to(x.device))
    return pos, heights
