"""Glitch flags and gap filling of a [D, T] TOD on the device (``mrx_tod_median_residual``, ``mrx_tod_glitch_flag``,
``mrx_tod_gap_fill``).

    med[d, t]   = median of x[d, clamp(t + i, 0, T - 1)], -h <= i <= h     (scipy.ndimage.median_filter, mode="nearest")
    r[d, t]     = x[d, t] - med[d, t]                                      (one float32 subtraction)
    sigma[d]    = 1.4826 * the lower median of |r[d, :]|                   (element (T - 1) // 2 of the sorted row)
    detection   : |r[d, s]| > float32(n_sigma * sigma[d])                  (strict)
    flags[d, t] = 1 at a detection, else 2 where a detection s has t - grow_after <= s <= t + grow_before, else 0
    gap fill    : a maximal run [a, b) of nonzero flags becomes the line through (tL, yL) and (tR, yR), the float64 means
                  of the indices and samples of the <= n_fit unflagged samples before a and from b on; a run that touches
                  a row end gets the other side's mean, a row flagged from end to end stays as it is.

The median is a selection, so r, the flags and the counts are reproducible bit for bit.  Inputs must be finite: what NaN
or inf give is unspecified.  The gap fill adds no noise realisation to the line it draws (constrained realisations are not
built): spectra fitted on gap-filled data miss the gaps' share of the white noise."""

from __future__ import annotations

import numpy as np

from ._tod_args import check_count, check_like, check_out, check_scratch_bytes, check_x, context, row_pitch, to_numpy

TILE_SAMPLES = 1024  # consecutive samples of a row one workgroup flags (mrx_glitch.hip: kTileSamples)
MAX_HALF_WINDOW = 15
MAX_GROW = 64
MAX_FIT = 16
MAD_TO_SIGMA = 1.4826


def _check_half_window(h):
    return check_count(h, "half_window", MAX_HALF_WINDOW)


def median_residual(x, half_window=5, ctx=None, out=None):
    """r = x - running median of 2 * half_window + 1 samples (edge rule: the end sample repeated) of a [D, T] float32 device
    tensor ``x`` (any row pitch), as a [D, T] float32 device tensor.  ``out``: a tensor to write into (any row pitch; its
    memory must not overlap ``x``'s).  ``ctx``: a Context bound to torch's current stream (None: one is made for the
    call).  Everything ``mrx_tod_median_residual`` refuses raises ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    h = _check_half_window(half_window)
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    else:
        check_out(out, x, D, T)
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    context(ctx, x).call("mrx_tod_median_residual", ptr(x), ld_x, D, T, h, ptr(out), row_pitch(out))
    return out


def robust_sigma(x, half_window=5, ctx=None, scratch_bytes=1 << 30):
    """[D] float64 on x's device: 1.4826 times the lower median (``torch.median``'s rule) of |median_residual(x)| of every
    row, a noise scale that glitches do not move.  The residuals are made ``scratch_bytes // (4 T)`` detectors at a time
    (at least one), so the scratch stays within ``scratch_bytes`` however large the TOD is."""
    import torch

    D, T, _ = check_x(x)
    h = _check_half_window(half_window)
    scratch_bytes = check_scratch_bytes(scratch_bytes)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    ctx = context(ctx, x)
    rows = max(1, min(D, scratch_bytes // (4 * T)))
    buf = torch.empty((rows, T), dtype=torch.float32, device=x.device)
    sigma = torch.empty(D, dtype=torch.float64, device=x.device)
    for d0 in range(0, D, rows):
        n = min(rows, D - d0)
        r = median_residual(x[d0:d0 + n], h, ctx=ctx, out=buf[:n])
        sigma[d0:d0 + n] = MAD_TO_SIGMA * torch.median(r.abs_(), dim=1).values.double()
    return sigma


def _threshold(n_sigma, sigma, D):
    """[D] float32 host array float32(n_sigma * sigma); refuses what is not finite or is negative."""
    n_sigma = float(n_sigma)
    if not np.isfinite(n_sigma) or n_sigma < 0:
        raise ValueError(f"n_sigma {n_sigma}: finite and >= 0")
    s = np.asarray(to_numpy(sigma), np.float64)
    if s.ndim == 0:
        s = np.full(D, float(s))
    if s.shape != (D,):
        raise ValueError(f"sigma of shape {s.shape}: a scalar or [{D}]")
    if not np.all(np.isfinite(s)) or np.any(s < 0):
        raise ValueError("sigma must be finite and >= 0")
    return (n_sigma * s).astype(np.float32)


def _check_grow(grow):
    try:
        before, after = grow
    except (TypeError, ValueError):
        raise ValueError(f"grow {grow!r}: a pair (before, after)") from None
    for g in (before, after):
        if int(g) != g or not 0 <= int(g) <= MAX_GROW:
            raise ValueError(f"grow {grow!r}: integers in 0 .. {MAX_GROW}")
    return int(before), int(after)


def find_glitches(x, n_sigma=6.0, half_window=5, grow=(2, 8), sigma=None, ctx=None):
    """``(flags, count)`` of a [D, T] float32 device tensor ``x`` (any row pitch): flags [D, T] uint8 (1 a detection
    |r| > float32(n_sigma * sigma[d]), 2 a sample within ``grow = (before, after)`` samples of one, 0 neither), count [D]
    int64 the nonzero flags of each row.  ``sigma``: a scalar or [D] noise scale (None: ``robust_sigma(x, half_window)``).
    A sigma or n_sigma that is not finite or is negative, and everything ``mrx_tod_glitch_flag`` refuses, raise ValueError
    before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    h = _check_half_window(half_window)
    before, after = _check_grow(grow)
    thresh = None if sigma is None else _threshold(n_sigma, sigma, D)
    if sigma is None:
        _threshold(n_sigma, 0.0, D)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    ctx = context(ctx, x)
    if thresh is None:
        thresh = _threshold(n_sigma, robust_sigma(x, h, ctx=ctx), D)
    d_thresh = torch.as_tensor(thresh).to(x.device)
    flags = torch.empty((D, T), dtype=torch.uint8, device=x.device)
    count = torch.empty(D, dtype=torch.int32, device=x.device)
    ctx.call("mrx_tod_glitch_flag", ptr(x), ld_x, D, T, h, ptr(d_thresh), before, after, ptr(flags), T, ptr(count))
    return flags, count.to(torch.int64)


def gap_fill(x, flags, n_fit=4, ctx=None):
    """Fill the samples of ``x`` ([D, T] float32 device tensor, any row pitch) whose ``flags`` ([D, T] uint8, any row pitch)
    are nonzero, IN PLACE, with the line between the means of the <= ``n_fit`` (1 .. 16) unflagged samples either side of
    each run; returns the [D] int64 number of samples written.  Unflagged samples are not touched; no noise is added."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    ld_f = check_like(flags, "flags", x, D, T, "uint8")
    n_fit = check_count(n_fit, "n_fit", MAX_FIT)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    filled = torch.empty(D, dtype=torch.int32, device=x.device)
    context(ctx, x).call("mrx_tod_gap_fill", ptr(x), ld_x, D, T, ptr(flags), ld_f, n_fit, ptr(filled))
    return filled.to(torch.int64)


def downsample_flags(flags, q, chunk_bytes=1 << 28):
    """The flags of a TOD decimated by ``q`` (``TOD.downsample``): [D, ceil(T / q)] uint8, output j 1 if any flag of
    [j q - q, j q + q] within [0, T) is nonzero (+-q samples is the main lobe of ``design_taps(q)``), else 0.  Plain
    torch on the flags' device, ``chunk_bytes`` of flags at a time."""
    import torch

    if not isinstance(flags, torch.Tensor) or flags.dim() != 2 or flags.dtype != torch.uint8:
        raise ValueError("flags must be a [D, T] uint8 tensor")
    if int(q) != q or int(q) < 1:
        raise ValueError(f"q {q}: an integer >= 1")
    q = int(q)
    D, T = flags.shape
    T_out = (T + q - 1) // q
    out = torch.zeros((D, T_out), dtype=torch.uint8, device=flags.device)
    rows = max(1, int(chunk_bytes) // max(1, T))
    for d0 in range(0, D, rows):
        nz = flags[d0:d0 + rows] != 0
        pad = torch.zeros((nz.shape[0], T_out * q), dtype=torch.bool, device=flags.device)
        pad[:, :T] = nz
        block = pad.view(nz.shape[0], T_out, q).any(dim=2)  # any of [j q, j q + q)
        o = block.clone()
        o[:, 1:] |= block[:, :-1]   # [j q - q, j q)
        o[:, :-1] |= pad[:, q::q]   # j q + q, the first sample of the next block
        out[d0:d0 + rows] = o.to(torch.uint8)
    return out


def draw_glitches(D, T, n_per_row, amplitude, seed):
    """The host draw of ``inject_glitches``: ``(onsets, amps)``, [D, n_per_row] int64 onsets (distinct within a row,
    ascending) and float64 signed amplitudes, from ``np.random.default_rng(seed)``: per row the onsets
    (``choice`` without replacement), then all signs, then all magnitudes (uniform in ``amplitude = (lo, hi)``, or the
    scalar)."""
    n = int(n_per_row)
    if n != n_per_row or not 0 <= n <= T:
        raise ValueError(f"n_per_row {n_per_row}: an integer in 0 .. T = {T}")
    lo, hi = (amplitude, amplitude) if np.ndim(amplitude) == 0 else amplitude
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo < 0 or hi < lo:
        raise ValueError(f"amplitude {amplitude!r}: a finite scalar >= 0 or a pair 0 <= lo <= hi")
    rng = np.random.default_rng(seed)
    onsets = np.stack([np.sort(rng.choice(T, n, replace=False)) for _ in range(D)]).astype(np.int64).reshape(D, n)
    sign = 2.0 * rng.integers(0, 2, (D, n)) - 1.0
    return onsets, sign * rng.uniform(lo, hi, (D, n))


def inject_glitches(x, n_per_row, amplitude, tau_samples, seed):
    """Add ``n_per_row`` exponential glitches to every row of ``x`` ([D, T] float32 tensor, device or host) IN PLACE:
    amp * exp(-k / tau_samples) at onset + k for 0 <= k < 4 tau_samples (cut at the row's end), onsets, signs and
    magnitudes from ``draw_glitches``.  Returns the [D, T] bool onset mask on x's device.  An aid for robustness studies
    and the tests' input; a cosmic-ray component of the simulation is not built."""
    import torch

    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("x must be a [D, T] float32 tensor")
    D, T = x.shape
    tau = float(tau_samples)
    if not np.isfinite(tau) or tau <= 0:
        raise ValueError(f"tau_samples {tau_samples}: finite and > 0")
    onsets, amps = draw_glitches(D, T, n_per_row, amplitude, seed)
    k = np.arange(int(np.ceil(4 * tau)))
    k = k[k < 4 * tau]
    col = onsets[:, :, None] + k
    val = (amps[:, :, None] * np.exp(-k / tau)).astype(np.float32)
    row = np.broadcast_to(np.arange(D)[:, None, None], col.shape)
    keep = col < T
    to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a[keep], dt)).to(x.device)  # noqa: E731
    x.index_put_((to(row, np.int64), to(col, np.int64)), to(val, np.float32), accumulate=True)
    mask = torch.zeros((D, T), dtype=torch.bool, device=x.device)
    mask[torch.as_tensor(np.repeat(np.arange(D), onsets.shape[1])).to(x.device), torch.as_tensor(onsets.reshape(-1)).to(x.device)] = True
    return mask
