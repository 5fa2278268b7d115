"""A continuously rotating half-wave plate (HWP) in the time domain (``mrx_tod_hwp_modulate``, ``mrx_tod_demodulate``,
csrc/mrx_hwp.hip).

Conventions.  chi(t) is the HWP angle in radians; the carrier is the [T, 2] float64 array (cos 4 chi, sin 4 chi), made
once on the host in float64 and uploaded: the kernels do no trigonometry, so an encoder's measured angles serve as well
as a uniform rotation.  An ideal HWP turns a detector of angle gamma into one of angle 2 chi - gamma; in pW, with
w = mueller_row(gamma),

    d = w_I I + w_I [ Q cos(4 chi - 2 gamma) + U sin(4 chi - 2 gamma) ] = S_I + S_c cos 4 chi + S_s sin 4 chi,

S_I the field of the detector's I weight alone, S_c that of a detector with the Stokes row (0, mueller_row(-gamma)[1],
mueller_row(-gamma)[2]) and S_s the same with mueller_row(pi / 4 - gamma).  An unpolarised detector (gamma NaN) sees no
modulation; atmosphere and noise are not modulated.

Demodulation is a lock-in: with H = (n_taps - 1) / 2 and T_out = ceil(T / q),

    y_t[d, j] =     sum_i hT[H + i]               x[d, j q + i] / sum_i hT[H + i]
    y_q[d, j] = 2 * sum_i hP[H + i] c[j q + i, 0] x[d, j q + i] / sum_i hP[H + i]
    y_u[d, j] = 2 * sum_i hP[H + i] c[j q + i, 1] x[d, j q + i] / sum_i hP[H + i],   -H <= i <= H,  0 <= j q + i < T,

in float64 over the tap index ascending, rounded once to float32; taps outside the row are dropped and the rest
renormalised, as ``downsample.decimate`` does.  For a band-limited sky y_q = w_I (Q cos 2 gamma - U sin 2 gamma) and
y_u = w_I (Q sin 2 gamma + U cos 2 gamma): the Q series of a detector is a detector of angle -gamma with no I weight, the
U series one of angle pi / 4 - gamma."""

from __future__ import annotations

import numpy as np

from ._tod_args import check_like, check_x, context, overlaps, row_pitch, same_rows, to_numpy
from .downsample import MAX_TAPS, _check, output_length, upload_taps

TILE_OUTPUTS = 128  # consecutive outputs of a row one workgroup produces (mrx_hwp.hip: kTileOutputs)
MAX_HARMONICS = 4   # of remove_hwpss: two templates each, regress.MAX_TEMPLATES is 8


class HWP:
    """A half-wave plate turning at ``frequency`` (Hz, > 0) from the angle ``phase`` (radians) at the first sample, in
    the sense ``direction`` (+1 or -1)."""

    def __init__(self, frequency, phase=0.0, direction=+1):
        self.frequency, self.phase = float(frequency), float(phase)
        if not (np.isfinite(self.frequency) and self.frequency > 0):
            raise ValueError(f"frequency {frequency}: a finite number of Hz > 0")
        if not np.isfinite(self.phase):
            raise ValueError(f"phase {phase}: a finite number of radians")
        if direction not in (-1, 1):
            raise ValueError(f"direction {direction}: +1 or -1")
        self.direction = int(direction)

    def angle(self, t):
        """chi(t) = phase + 2 pi direction frequency (t - t[0]), float64."""
        t = np.asarray(t, np.float64)
        return self.phase + 2.0 * np.pi * self.direction * self.frequency * (t - (t[0] if t.size else 0.0))

    def to_metadata(self):
        return {"frequency": self.frequency, "phase": self.phase, "direction": self.direction}

    @classmethod
    def from_metadata(cls, m):
        return cls(m["frequency"], m.get("phase", 0.0), m.get("direction", 1))


def carrier(chi):
    """The [T, 2] float64 carrier (cos 4 chi, sin 4 chi) of the HWP angles ``chi`` [T]."""
    chi = np.asarray(chi, np.float64)
    if chi.ndim != 1:
        raise ValueError("chi must be one-dimensional")
    return np.ascontiguousarray(np.stack([np.cos(4.0 * chi), np.sin(4.0 * chi)], axis=1))


def design_taps(sample_rate, f_hwp, atten_db=120.0, pass_edge=0.5, stop_edge=2.0):
    """The low-pass of the lock-in, a Kaiser design in float64: pass band up to ``pass_edge`` f_hwp, stop band from
    ``stop_edge`` f_hwp at ``atten_db``.  n, beta = scipy.signal.kaiserord(atten_db, (stop_edge - pass_edge) f_hwp /
    (sample_rate / 2)), n made odd, taps = firwin(n, (pass_edge + stop_edge) f_hwp / 2, fs=sample_rate,
    window=("kaiser", beta)).  Mixing moves the unpolarised signal (kelvins of atmosphere) to 4 f_hwp, and the filter has
    to reject it against millikelvins of polarisation: hence 120 dB, which a Hamming window does not reach.  ValueError
    where the design needs more than 1025 taps."""
    import scipy.signal

    fs, f = float(sample_rate), float(f_hwp)
    if not (np.isfinite(fs) and fs > 0 and np.isfinite(f) and f > 0):
        raise ValueError("sample_rate and f_hwp: finite and > 0")
    if not 0 < pass_edge < stop_edge or stop_edge * f >= fs / 2:
        raise ValueError(f"need 0 < pass_edge < stop_edge and stop_edge f_hwp = {stop_edge * f:g} Hz below Nyquist ({fs / 2:g} Hz)")
    n, beta = scipy.signal.kaiserord(float(atten_db), (stop_edge - pass_edge) * f / (fs / 2))
    n = int(n) | 1
    if n > MAX_TAPS:
        raise ValueError(f"the design needs {n} taps, more than {MAX_TAPS}: lower the sample rate, or widen the transition band")
    return np.asarray(scipy.signal.firwin(n, 0.5 * (pass_edge + stop_edge) * f, fs=fs, window=("kaiser", beta)), np.float64)


def max_factor(sample_rate, f_hwp, pass_edge=0.5, stop_edge=2.0):
    """The largest integer q whose aliases stay out of the pass band: sample_rate / q - stop_edge f_hwp >= pass_edge
    f_hwp (0 where even q = 1 does not).  The condition is held to one part in 10^6: a sample rate read off time stamps
    (60 s of epoch seconds in float64 give 400 Hz to 4 parts in 10^9) must not lose a factor to its last digits."""
    return int(np.floor(float(sample_rate) / ((float(pass_edge) + float(stop_edge)) * float(f_hwp)) * (1 + 1e-6)))


def _host_taps(taps):
    return np.ascontiguousarray(to_numpy(taps), np.float64)


def _device_carrier(c, T, device):
    """The [T, 2] float64 carrier as a contiguous tensor on ``device`` (a numpy array is uploaded)."""
    import torch

    if isinstance(c, torch.Tensor):
        if c.dtype != torch.float64 or tuple(c.shape) != (T, 2):
            raise ValueError(f"carrier must be a [{T}, 2] float64 array")
        return c.to(device).contiguous()
    c = np.asarray(c)
    if c.dtype != np.float64 or c.shape != (T, 2):
        raise ValueError(f"carrier must be a [{T}, 2] float64 array")
    return torch.as_tensor(np.ascontiguousarray(c)).to(device)


def demodulate(x, carrier, q, taps_t=None, taps_p=None, ctx=None, out=None, want_t=True):
    """``(y_t, y_q, y_u)``, the [D, T_out] float32 device tensors of the formulas at the top of the module, of a [D, T]
    float32 device tensor ``x`` (any row pitch), the [T, 2] float64 ``carrier`` (numpy, or a tensor) and the factor ``q``
    (2 .. 32).  ``taps_t`` and ``taps_p``: float64, one odd count <= 1025 (``design_taps``); one of them given serves for
    both.  ``want_t`` False: polarisation only, y_t is None and y_q, y_u hold the bits of the three-output call.
    ``out``: the three tensors to write into (y_t's place None without ``want_t``), [D, T_out] float32 on x's device with
    ONE row pitch, overlapping neither x nor each other.  ``ctx``: a Context bound to torch's current stream (None: one
    is made for the call).  Everything ``mrx_tod_demodulate`` refuses, and taps whose truncated sum is <= 0 at any output
    of this T, raise ValueError before any device call."""
    import torch

    from ._lib import ptr

    if taps_t is None and taps_p is None:
        raise ValueError("no taps: give taps_p (design_taps(sample_rate, f_hwp)), taps_t, or both")
    hp = _host_taps(taps_t if taps_p is None else taps_p)
    ht = hp if taps_t is None else _host_taps(taps_t)
    D, T, ld_x = _check(x, q, hp)
    if want_t:
        _check(x, q, ht)
        if ht.size != hp.size:
            raise ValueError(f"taps_t has {ht.size} taps and taps_p {hp.size}: one count for both")
    q = int(q)
    T_out = output_length(T, q)
    d_carrier = _device_carrier(carrier, T, x.device)
    names = ("y_t", "y_q", "y_u")
    if out is None:
        buf = torch.empty((3 if want_t else 2, D, T_out), dtype=torch.float32, device=x.device)
        outs = [buf[0], buf[1], buf[2]] if want_t else [None, buf[0], buf[1]]
    else:
        outs = list(out)
        if len(outs) != 3 or (outs[0] is None) != (not want_t):
            raise ValueError("out must be (y_t, y_q, y_u), y_t None exactly where want_t is False")
        seen = [x]
        for name, o in zip(names, outs):
            if o is None:
                continue
            check_like(o, f"out's {name}", x, D, T_out, length="T_out")
            if D > 1 and o.stride(0) != outs[1].stride(0):
                raise ValueError("out's tensors must have one row pitch")
            if any(overlaps(o, a) for a in seen):
                raise ValueError("out's tensors must overlap neither x nor each other")
            seen.append(o)
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    d_hp = upload_taps(hp, x.device)
    d_ht = (d_hp if ht is hp else upload_taps(ht, x.device)) if want_t else None
    context(ctx, x).call("mrx_tod_demodulate", ptr(x), ld_x, D, T, q, ptr(d_carrier), ptr(d_ht), ptr(d_hp), hp.size, ptr(outs[0]),
                         ptr(outs[1]), ptr(outs[2]), row_pitch(outs[1]))
    return tuple(outs)


def modulate(s_i, s_c, s_s, carrier, out=None, ctx=None):
    """float32(s_i + s_c cos 4 chi + s_s sin 4 chi), evaluated in float64 and rounded once (``mrx_tod_hwp_modulate``), of
    three [D, T] float32 device tensors of ONE row pitch and the [T, 2] float64 ``carrier``.  ``out``: None (a new
    tensor), ``s_i`` itself or an equal view of it (in place), or a [D, T] float32 tensor of any row pitch that overlaps none of the three.
    Everything the entry refuses raises ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld = check_x(s_i, "s_i")
    for name, a in (("s_c", s_c), ("s_s", s_s)):
        if check_like(a, name, s_i, D, T) != ld:
            raise ValueError("s_i, s_c and s_s must have one row pitch")
    d_carrier = _device_carrier(carrier, T, s_i.device)
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=s_i.device)
    ld_out = check_like(out, "out", s_i, D, T)
    if any(overlaps(out, a) for a in (s_c, s_s) + (() if same_rows(out, s_i) else (s_i,))):
        raise ValueError("out must be s_i or overlap none of the inputs")
    if not s_i.is_cuda:
        raise ValueError("s_i must be a device tensor")
    context(ctx, s_i).call("mrx_tod_hwp_modulate", ptr(s_i), ptr(s_c), ptr(s_s), ld, D, T, ptr(d_carrier), ptr(out), ld_out)
    return out


def polarized_rows(dets):
    """The indices of the detectors with a polarisation angle (gamma not NaN), ascending."""
    return np.flatnonzero(~np.isnan(np.asarray(dets.gamma, float)))


def demodulated_detectors(dets, polarized_only=True):
    """The ``Detectors`` table of a demodulated TOD: T rows for every detector, then the Q rows and then the U rows of
    the polarised ones, ``polarized_rows(dets)`` (with ``polarized_only`` False of every detector, an unpolarised one's
    being rows of no weight; an unpolarised detector carries no polarisation signal).  ``offsets``,
    ``band_index``, ``primary_size`` and ``time_constant`` are repeated; ``gamma`` is gamma, -gamma and pi / 4 - gamma;
    and the Stokes-row override (``Detectors.stokes_rows``) is (mueller00, 0, 0, 0) for a T row and
    (0, mueller_row(g')[1], mueller_row(g')[2], 0) for a Q or U row of angle g'."""
    from .instrument import Detectors
    from .map import mueller_row

    gamma = np.asarray(dets.gamma, float)
    pol = polarized_rows(dets) if polarized_only else np.arange(dets.n)
    idx = np.concatenate([np.arange(dets.n), pol, pol])
    g = np.concatenate([gamma, -gamma[pol], np.pi / 4 - gamma[pol]])
    stokes = np.zeros((idx.size, 4))
    stokes[: dets.n, 0] = dets.mueller00()
    stokes[dets.n:, 1:3] = mueller_row(g[dets.n:])[:, 1:3]
    return Detectors(dets.offsets[idx], dets.bands, dets.band_index[idx], dets.primary_size[idx], g,
                     time_constant=dets.time_constant[idx], stokes=stokes)


def harmonic_templates(chi, harmonics=(1, 2)):
    """The [2 K, T] float32 templates cos k chi, sin k chi of the K ``harmonics`` k (positive integers), in that order
    harmonic by harmonic, computed in float64 and rounded: the HWP synchronous signal's basis for ``TOD.regress``."""
    chi = np.asarray(chi, np.float64)
    ks = [int(k) for k in harmonics]
    if chi.ndim != 1 or not ks or any(k < 1 or k != h for k, h in zip(ks, harmonics)) or len(set(ks)) != len(ks):
        raise ValueError("chi must be one-dimensional and harmonics distinct positive integers")
    return np.stack([f(k * chi) for k in ks for f in (np.cos, np.sin)]).astype(np.float32)


def inject_hwpss(tod, amplitudes, hwp=None, into=None, ctx=None, device="cuda:0"):
    """A new TOD with an HWP synchronous signal added to the field ``into`` (default: the first):
    sum_k a_k cos k chi + b_k sin k chi with ``amplitudes`` = {k: (a_k, b_k)}, each a scalar or one per detector, through
    ``regress.apply(..., sign=+1)`` on ``harmonic_templates``.  ``hwp`` None: ``tod.metadata["hwp"]``.  An aid for the
    tests and for robustness studies, like ``flagging.inject_glitches``; the simulation itself adds no such signal."""
    import torch

    from . import regress

    hwp = HWP.from_metadata(tod.metadata["hwp"]) if hwp is None else hwp
    ks = sorted(amplitudes)
    B = harmonic_templates(hwp.angle(tod.coords.t), ks)
    D = tod.dets.n
    a = np.stack([np.broadcast_to(np.asarray(amplitudes[k][j], float), (D,)) for k in ks for j in (0, 1)], axis=1)
    data, _, _, _, into, ctx = tod._device_fields(None, into, ctx, device)
    x = data[into]
    regress.apply(x, torch.as_tensor(B).to(x.device)[None], torch.as_tensor(np.ascontiguousarray(a)).to(x.device), sign=+1, out=x, ctx=ctx)
    return tod._derived(data=data, record={})
