"""Detector time constants: the one-pole lag of every detector and its exact inverse on the device (``mrx_tod_onepole``,
``mrx_tod_onepole_inverse``).

A bolometer answers optical power through a one-pole low-pass of time constant tau (seconds).  At the sample rate fs its
pole is a = exp(-1 / (fs tau)), a = 0 for tau = 0 (no lag), and with g = 1 - a, r = 1 / (1 - a):

    lag          y[0] = x[0] (init "steady": the detector has seen x[0] for ever) or g x[0] (init "zero")
                 y[t] = a y[t - 1] + g x[t]                                 (float64 throughout, stored as float32)
    deconvolve   x[0] = y[0] ("steady") or y[0] r ("zero");   x[t] = (y[t] - a y[t - 1]) r

A row with a = 0 is copied bit for bit by both.  The order of the operations is written out in include/mrx.h, and
tests/timeconst_ref.py restates it in numpy.  Every bit of a row's result depends on that row alone: the same inputs give
the same bits on every call, in place and out of place."""

from __future__ import annotations

import numpy as np

from ._tod_args import check_out, check_x, context, row_pitch, to_numpy

INITS = {"zero": 0, "steady": 1}  # mrx.h: init


def poles(tau, sample_rate):
    """The [D] float64 poles a = exp(-1 / (sample_rate tau)) of the time constants ``tau`` (seconds; a scalar gives one
    pole), 0 where tau = 0.  Negative or non-finite tau, or a sample rate that is not a finite number > 0, raise
    ValueError."""
    tau = np.atleast_1d(np.asarray(tau, np.float64))
    fs = float(sample_rate)
    if tau.ndim != 1 or not np.all(np.isfinite(tau)) or np.any(tau < 0):
        raise ValueError("tau must be a scalar or a one-dimensional array of finite time constants >= 0")
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError(f"sample_rate {sample_rate}: a finite number > 0")
    a = np.zeros(tau.shape, np.float64)
    on = tau > 0
    a[on] = np.exp(-1.0 / (fs * tau[on]))
    return a


def sample_rate_of(t):
    """(n - 1) / (t[-1] - t[0]) of the sample times ``t``, as ``TOD.psd`` takes it."""
    t = np.asarray(t, float)
    if t.ndim != 1 or t.size < 2 or not t[-1] > t[0]:
        raise ValueError("the sample rate needs at least two ascending sample times")
    return (t.size - 1) / (t[-1] - t[0])


def _check_init(init):
    if init not in INITS:
        raise ValueError(f'init {init!r}: "steady" or "zero"')
    return INITS[init]


def _check_poles(a, x, D):
    """The [D] float64 tensor of the poles on x's device: every one finite and in [0, 1)."""
    import torch

    host = np.asarray(to_numpy(a))
    if host.ndim != 1 or host.shape[0] != D or host.dtype != np.float64:
        raise ValueError(f"a must be a [{D}] float64 array or tensor: one pole a row")
    if not np.all((host >= 0.0) & (host < 1.0)):  # (a NaN compares false)
        raise ValueError("every pole must be in [0, 1)")
    if isinstance(a, torch.Tensor) and a.device == x.device and a.is_contiguous():
        return a
    return torch.as_tensor(np.ascontiguousarray(host)).to(x.device)


def _run(entry, x, a, init, out, ctx):
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    d_a = _check_poles(a, x, D)
    init = _check_init(init)
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    else:
        check_out(out, x, D, T, in_place=True)
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    context(ctx, x).call(entry, ptr(x), ld_x, D, T, ptr(d_a), init, ptr(out), row_pitch(out))
    return out


def apply(x, a, init="steady", out=None, ctx=None):
    """The lag: ``x`` ([D, T] float32 device tensor, any row pitch) through every row's one-pole low-pass with the poles
    ``a`` ([D] float64, ``poles``), within 2^-24 |y| + 64 2^-53 max|x| / (1 - a) of the serial float64 recurrence.
    Returns ``out`` (None: a new tensor; ``x`` itself: in place; otherwise a [D, T] float32 tensor of any row pitch that
    does not overlap x).  ``ctx``: a Context bound to torch's current stream (None: one is made for the call).
    Everything ``mrx_tod_onepole`` refuses, and a pole outside [0, 1), raise ValueError before any device call."""
    return _run("mrx_tod_onepole", x, a, init, out, ctx)


def deconvolve(y, a, init="steady", out=None, ctx=None):
    """The exact inverse of ``apply``: the two-tap FIR x[t] = (y[t] - a y[t - 1]) / (1 - a) of every row, bit for bit the
    float64 lines at the top of the module.  Arguments and refusals as ``apply`` (``mrx_tod_onepole_inverse``)."""
    return _run("mrx_tod_onepole_inverse", y, a, init, out, ctx)

