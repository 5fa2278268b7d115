"""Anti-aliased downsampling of a [D, T] TOD on the device (``mrx_tod_decimate``): a zero-phase FIR low-pass
evaluated at every q-th sample,

    y[d, j] = sum_i h[H + i] x[d, j q + i] / sum_i h[H + i],   -H <= i <= H,  0 <= j q + i < T,   j < T_out = ceil(T / q),

in float64, rounded once to float32.  Output sample j belongs to input time t[j q].  The sum is a correlation (h's index
grows along the sample index); taps that fall outside the row are dropped and the rest renormalised, so a constant row
maps onto itself and the TOD's mean puts no transient into the row's ends (zero padding, scipy's edge rule, would).  For
symmetric taps the result is ``scipy.signal.resample_poly(x, 1, q, window=h)`` over the same call on a row of ones."""

from __future__ import annotations

import numpy as np

from ._tod_args import check_out, check_x, context, row_pitch, to_numpy

TILE_OUTPUTS = 256   # consecutive outputs of a row one workgroup produces (mrx_decimate.hip: kTileOutputs)
MIN_FACTOR, MAX_FACTOR = 2, 32
MAX_TAPS = 1025


def design_taps(q, half_width=10, window="hamming"):
    """``scipy.signal.firwin(2 * half_width * q + 1, 1 / q, window=window)`` in float64: with the defaults exactly the
    filter of ``scipy.signal.decimate(x, q, ftype="fir")``."""
    import scipy.signal

    q, half_width = int(q), int(half_width)
    if not MIN_FACTOR <= q <= MAX_FACTOR:
        raise ValueError(f"q {q}: {MIN_FACTOR} .. {MAX_FACTOR}")
    if half_width < 0 or 2 * half_width * q + 1 > MAX_TAPS:
        raise ValueError(f"half_width {half_width}: 2 * half_width * q + 1 taps must be in 1 .. {MAX_TAPS}")
    return np.asarray(scipy.signal.firwin(2 * half_width * q + 1, 1.0 / q, window=window), np.float64)


def output_length(T, q):
    """T_out = ceil(T / q) = len(range(0, T, q))."""
    return (int(T) + int(q) - 1) // int(q)


def truncated_sums(taps, T, q):
    """[T_out] float64: the sum of the taps that meet a sample of [0, T) at each output, as a prefix-sum difference."""
    h = np.asarray(taps, np.float64)
    H = (h.size - 1) // 2
    first = np.arange(output_length(T, q), dtype=np.int64) * int(q)
    lo = np.maximum(0, H - first)
    hi = np.minimum(h.size - 1, H + (int(T) - 1) - first)
    pre = np.concatenate([[0.0], np.cumsum(h)])
    return pre[hi + 1] - pre[lo]


def _check(x, q, taps):
    """The refusals of ``mrx_tod_decimate`` and the taps' truncated sums, on the host: (D, T, row pitch of x)."""
    D, T, ld_x = check_x(x)
    if int(q) != q or not MIN_FACTOR <= int(q) <= MAX_FACTOR:
        raise ValueError(f"q {q}: an integer in {MIN_FACTOR} .. {MAX_FACTOR}")
    if taps.ndim != 1 or not 1 <= taps.size <= MAX_TAPS or taps.size % 2 == 0:
        raise ValueError(f"taps of shape {taps.shape}: an odd count in 1 .. {MAX_TAPS}")
    if not np.all(np.isfinite(taps)):
        raise ValueError("taps must be finite")
    sums = truncated_sums(taps, T, int(q))
    if not np.all(sums > 0):
        j = int(np.argmin(sums))
        raise ValueError(f"the taps that meet the row at output {j} sum to {sums[j]:g}: every truncated sum must be > 0")
    return D, T, ld_x


def upload_taps(taps, device):
    """The taps as the contiguous float64 tensor on ``device`` that ``decimate(..., device_taps=)`` takes: one upload for
    several calls."""
    import torch

    return torch.as_tensor(np.ascontiguousarray(taps, np.float64)).to(device)


def decimate(x, q, taps=None, ctx=None, out=None, device_taps=None):
    """The [D, T_out] float32 device tensor of a [D, T] float32 device tensor ``x`` (any row pitch) decimated by ``q``
    (2 .. 32) with ``taps`` (float64, an odd count <= 1025; None: ``design_taps(q)``).  ``out``: a [D, T_out] float32
    device tensor to write into (any row pitch; its memory must not overlap ``x``'s).  ``device_taps``: the same taps
    already on x's device (``upload_taps``), to spare the upload every call otherwise makes.  ``ctx``: a
    Context bound to torch's current stream, like every buffer this call allocates (None: one is made for the call).
    Everything ``mrx_tod_decimate`` refuses, and taps whose truncated sum is <= 0 at any output of this T, raise
    ValueError before any device call."""
    import torch

    from ._lib import ptr

    if taps is None:
        if int(q) != q or not MIN_FACTOR <= int(q) <= MAX_FACTOR:
            raise ValueError(f"q {q}: an integer in {MIN_FACTOR} .. {MAX_FACTOR}")
        h = design_taps(q)
    else:
        h = np.ascontiguousarray(to_numpy(taps), np.float64)
    D, T, ld_x = _check(x, q, h)
    q = int(q)
    T_out = output_length(T, q)
    if out is None:
        out = torch.empty((D, T_out), dtype=torch.float32, device=x.device) if x.is_cuda else x.new_empty((D, T_out))
    else:
        check_out(out, x, D, T_out, length="T_out")
    if device_taps is not None and (not isinstance(device_taps, torch.Tensor) or device_taps.dtype != torch.float64
                                    or tuple(device_taps.shape) != h.shape or not device_taps.is_contiguous()
                                    or device_taps.device != x.device):
        raise ValueError(f"device_taps must be the {h.size} taps as a contiguous float64 tensor on x's device")
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    d_taps = upload_taps(h, x.device) if device_taps is None else device_taps
    context(ctx, x).call("mrx_tod_decimate", ptr(x), ld_x, D, T, q, ptr(d_taps), h.size, ptr(out), row_pitch(out))
    return out
